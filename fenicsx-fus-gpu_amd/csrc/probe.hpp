// Point sensors: the degree-P GLL interpolant of a dof vector at a fixed set of points, evaluated after every time step
// and recorded / accumulated on the device (the device counterpart of the reference's ``u_n_.eval(x_eval, cell_eval)``
// loop over its collection window, cuda/demo_linear_piston.py / cuda/demo_nonlinear_bowl.py).
//
// One thread per point.  The host locates every point once (cell + reference coordinates) and tabulates the three
// 1-D Lagrange rows of the point, ``w[p][3][n]`` (x, y, z), so the kernel is a gather of the cell's n^3 dofs and a
// tensor contraction: value = sum_ijk Lx[i] Ly[j] Lz[k] u[dofmap[c][i n^2 + j n + k]], summed in double.  The host sorts
// the points by cell, so neighbouring lanes read neighbouring (often the same) dofmap rows.
//
// Outputs, each optional (null = off), of the value rounded to T (so that the peaks are bitwise the extrema of the series):
//   rec[slot][p]                       T      the time series row
//   pmax[p] / pmin[p]                  double running maximum / minimum
//   hre[h][p] += v coef[2h], him[h][p] += v coef[2h + 1]   double, h < H   (coef: this step's cos / sin factors, device memory)
// Every accumulator of a point belongs to its thread alone: no atomics.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fus {

constexpr int kProbeThreads = 256;
// the inner (z) loop is unrolled whole up to n = 7, in 6s above: fp64 P >= 7 unrolled whole needs 66-84 VGPRs (fewer than 8 waves per SIMD)
template <int n>
constexpr int kProbeUnroll = n <= 7 ? n : 6;

template <typename T, int P>
__global__ __launch_bounds__(kProbeThreads) void probe_eval_kernel(const T* __restrict__ u, const int32_t* __restrict__ cells,
                                                                   const int32_t* __restrict__ dofmap, const T* __restrict__ w,
                                                                   int64_t npts, int64_t ncells, T* __restrict__ rec,
                                                                   double* __restrict__ pmax, double* __restrict__ pmin,
                                                                   double* __restrict__ hre, double* __restrict__ him,
                                                                   const double* __restrict__ coef, int H) {
  constexpr int n = P + 1;
  const int64_t p = (int64_t)blockIdx.x * kProbeThreads + threadIdx.x;
  if (p >= npts) return;
  const int64_t c = cells[p];
  double acc;
  if (c < 0 || c >= ncells) {
    acc = __builtin_nan("");  // a point the host did not locate (cannot happen through PointSensors): NaN, never a stray read
  } else {
    const int32_t* dm = dofmap + c * (n * n * n);
    const T* lx = w + p * (3 * n);
    const T* ly = lx + n;
    const T* lz = ly + n;
    // z innermost (the fastest index of the dofmap row); the outer two loops stay rolled so that the registers hold one
    // row of n dofs, not the n^3 gather (fp64 P >= 7 would not fit 8 waves per SIMD otherwise)
    acc = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
      double sx = 0.0;
#pragma unroll 1
      for (int j = 0; j < n; ++j) {
        const int32_t* row = dm + (i * n + j) * n;
        double sy = 0.0;
#pragma unroll(kProbeUnroll<n>)
        for (int k = 0; k < n; ++k) sy += (double)lz[k] * (double)u[row[k]];
        sx += (double)ly[j] * sy;
      }
      acc += (double)lx[i] * sx;
    }
  }
  const T vt = (T)acc;
  const double v = (double)vt;
  if (rec) rec[p] = vt;  // rec already points at row ``slot``
  if (pmax) pmax[p] = fmax(pmax[p], v);
  if (pmin) pmin[p] = fmin(pmin[p], v);
  for (int h = 0; h < H; ++h) {
    hre[h * npts + p] += v * coef[2 * h];
    him[h * npts + p] += v * coef[2 * h + 1];
  }
}

template <typename T, int P>
inline hipError_t launch_probe_eval(const T* u, const int32_t* cells, const int32_t* dofmap, const T* w, int64_t npts, int64_t ncells,
                                    T* rec, double* pmax, double* pmin, double* hre, double* him, const double* coef, int H,
                                    hipStream_t stream) {
  if (npts <= 0) return hipSuccess;
  const int64_t nblocks = (npts + kProbeThreads - 1) / kProbeThreads;
  hipLaunchKernelGGL((probe_eval_kernel<T, P>), dim3((unsigned)nblocks), dim3(kProbeThreads), 0, stream, u, cells, dofmap, w, npts,
                     ncells, rec, pmax, pmin, hre, him, coef, H);
  return hipGetLastError();
}

}  // namespace fus
