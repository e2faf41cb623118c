// Sampled source waveforms: the source-facet term and the point-source term of one RK4 stage with an ARBITRARY signal per element /
// point, read from a table on the device (sources.SampledWaveform) instead of the analytic A Env(s) cos(w0 s + phi) of
// source_array.hpp / point_source.hpp.
//
// The table is double[R][Nt][2]: row r holds, per sample k, the value w_r and the derivative dw_r/ds at s_k = t0 + k dt, interleaved.
// The interpolant is the cubic Hermite of value and derivative on each interval (C1, exact at the nodes):
//   x = (s - t0) / dt
//   x < 0, x > Nt - 1 or x not a number: nothing is contributed (the waveform is ZERO outside [t0, t0 + (Nt - 1) dt])
//   k = min(floor(x), Nt - 2),  th = x - k            (the last node is reached with k = Nt - 2, th = 1)
//   w    = h00 w_k + h10 dt d_k + h01 w_{k+1} + h11 dt d_{k+1}
//   dw   = (h00' w_k + h01' w_{k+1}) / dt + h10' d_k + h11' d_{k+1}
//   h00  = (1 + 2 th) (1 - th)^2    h10  = th (1 - th)^2         h01  = th^2 (3 - 2 th)    h11  = th^2 (th - 1)
//   h00' = 6 th (th - 1)            h10' = (1 - th) (1 - 3 th)   h01' = -h00'              h11' = th (3 th - 2)
// The four numbers of an interval, (w_k, d_k, w_{k+1}, d_{k+1}), are 32 contiguous bytes at a 16-byte aligned address: two 16-byte
// loads.  Index arithmetic is 64-bit.  sources.SampledWaveform.values is this arithmetic in numpy.
//
//   facet:  g_e(t) = a_e A w_{r(e)}(t - tau_e),  dg_e/dt alike      set A:  y[dmA[f][i]] += (g_e cA1[f] + dg_e cA2[f]) detJA[f][i]
//   point:  g_p(t) = a_p A w_{r(p)}(t - tau_p)                              y[dofmap[c][ijk]] += g_p Lx[i] Ly[j] Lz[k]
// r = row_of_element[e] (row_of_point[p]); a row outside [0, R) is a silent element: skipped, never dereferenced.  Set B of the facet
// launch is the absorbing term of facet_source_array_kernel, unchanged: a stage keeps ONE facet launch.  The stage block is the
// SourceStage of source_array.hpp, of which only ``t`` and ``A`` are read: a captured step rewrites the same six words.
//
// These are kernels of their own, not a branch of the analytic ones: those stay the code they are (their register pins are tests), and
// a table walk next to two sincospi would cost them their 64 VGPRs.  The time arithmetic and the interpolation are fp64 for fp32 fields
// too; the value is rounded to T once, before the add.  Float atomics, never load + store, and at most 64 VGPRs / 8 waves per SIMD, for
// the reason given in source_array.hpp: next to a halo the launch runs while the interior stiffness launch holds the CUs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "source_array.hpp"

namespace fus {

// the table of a launch, by value in the kernel arguments
struct WaveTable {
  const double* tab;  // double[R][Nt][2], 16-byte aligned
  int64_t R, Nt;
  double t0, dt;
};

// (w, dw) of row ``r`` (0 <= r < R, checked by the caller) at time ``s``; false: outside the table, nothing to add
template <bool kDerivative>
__device__ inline bool wave_eval(const WaveTable& wt, int64_t r, double s, double& w, double& dw) {
  const double x = (s - wt.t0) / wt.dt;
  if (!(x >= 0.0 && x <= (double)(wt.Nt - 1))) return false;  // a NaN fails both
  int64_t k = (int64_t)x;
  if (k > wt.Nt - 2) k = wt.Nt - 2;
  const double th = x - (double)k;
  const double2* p = reinterpret_cast<const double2*>(wt.tab) + (r * wt.Nt + k);
  const double2 a = p[0], b = p[1];
  const double um = 1.0 - th;
  const double h00 = (1.0 + 2.0 * th) * (um * um), h10 = th * (um * um);
  const double h01 = (th * th) * (3.0 - 2.0 * th), h11 = (th * th) * (th - 1.0);
  w = h00 * a.x + h10 * (wt.dt * a.y) + h01 * b.x + h11 * (wt.dt * b.y);
  if (kDerivative) {
    const double d00 = 6.0 * th * (th - 1.0), d10 = um * (1.0 - 3.0 * th), d11 = th * (3.0 * th - 2.0);
    dw = (d00 * a.x - d00 * b.x) / wt.dt + d10 * a.y + d11 * b.y;
  } else {
    dw = 0.0;
  }
  return true;
}

template <typename T>
__global__ void __launch_bounds__(256, 8)
    facet_source_wave_kernel(T* __restrict__ y, const T* __restrict__ cA1, const T* __restrict__ cA2, const T* __restrict__ detJA,
                             const int32_t* __restrict__ dmA, const int32_t* __restrict__ eid, int64_t totalA,
                             const double* __restrict__ amp, const double* __restrict__ delay, const int32_t* __restrict__ row_of,
                             WaveTable wt, const T* __restrict__ xB, const T* __restrict__ cB, const T* __restrict__ detJB,
                             const int32_t* __restrict__ dmB, int64_t totalB, int N, SourceStage st, const double* __restrict__ sdev) {
  if (sdev != nullptr) {
    st.t = sdev[0];
    st.A = sdev[2];
  }
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < totalA + totalB; idx += stride) {
    if (idx < totalA) {
      const int64_t f = idx / N;
      const int e = eid[f];
      if (e < 0) continue;  // inactive facet
      const int64_t r = row_of[e];
      if (r < 0 || r >= wt.R) continue;  // silent element
      double w, dw;
      if (!wave_eval<true>(wt, r, st.t - delay[e], w, dw)) continue;
      if (w == 0.0 && dw == 0.0) continue;
      const double a = amp[e] * st.A;
      double c = (a * w) * (double)cA1[f];
      if (cA2 != nullptr) c += (a * dw) * (double)cA2[f];
      unsafeAtomicAdd(y + dmA[idx], (T)(c * (double)detJA[idx]));
    } else {
      const int64_t j = idx - totalA;
      const int64_t f = j / N;
      const int32_t dof = dmB[j];
      unsafeAtomicAdd(y + dof, xB[dof] * (cB[f] * detJB[j]));
    }
  }
}

template <typename T>
inline hipError_t launch_facet_source_wave(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA, const int32_t* eid,
                                           int64_t nentA, const double* amp, const double* delay, const int32_t* row_of,
                                           const WaveTable& wt, const T* xB, const T* cB, const T* detJB, const int32_t* dmB,
                                           int64_t nentB, int N, const SourceStage& st, const double* sdev, hipStream_t stream) {
  const int64_t total = (nentA + nentB) * (int64_t)N;
  if (total <= 0) return hipSuccess;
  int64_t nblocks = (total + 255) / 256;
  if (nblocks > 4096) nblocks = 4096;
  hipLaunchKernelGGL((facet_source_wave_kernel<T>), dim3((unsigned)nblocks), dim3(256), 0, stream, y, cA1, cA2, detJA, dmA, eid,
                     nentA * (int64_t)N, amp, delay, row_of, wt, xB, cB, detJB, dmB, nentB * (int64_t)N, N, st, sdev);
  return hipGetLastError();
}

// the thread mapping and the skips of point_source_kernel: one thread per (point, i, j), a row of n adds along z
template <typename T, int P>
__global__ void __launch_bounds__(kPointSourceThreads, 8)
    point_source_wave_kernel(T* __restrict__ y, const int32_t* __restrict__ cells, const int32_t* __restrict__ dofmap,
                             const T* __restrict__ w, int64_t npts, int64_t ncells, const double* __restrict__ amp,
                             const double* __restrict__ delay, const int32_t* __restrict__ row_of, WaveTable wt, SourceStage st) {
  constexpr int n = P + 1;
  const int64_t idx = (int64_t)blockIdx.x * kPointSourceThreads + threadIdx.x;
  if (idx >= npts * (n * n)) return;
  const int64_t p = idx / (n * n);
  const int ij = (int)(idx - p * (n * n));
  const int64_t c = cells[p];
  if (c < 0 || c >= ncells) return;  // a point the host did not locate
  const int64_t r = row_of[p];
  if (r < 0 || r >= wt.R) return;  // silent point
  double val, dval;
  if (!wave_eval<false>(wt, r, st.t - delay[p], val, dval)) return;
  const T* lx = w + p * (3 * n);
  const T* ly = lx + n;
  const T* lz = ly + n;
  const double g = (amp[p] * st.A * val) * ((double)lx[ij / n] * (double)ly[ij % n]);
  if (g == 0.0) return;
  const int32_t* row = dofmap + c * (n * n * n) + ij * n;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const T v = (T)(g * (double)lz[k]);
    if (v != T(0)) unsafeAtomicAdd(y + row[k], v);
  }
}

// npts == 0: no launch
template <typename T, int P>
inline hipError_t launch_point_source_wave(T* y, const int32_t* cells, const int32_t* dofmap, const T* w, int64_t npts, int64_t ncells,
                                           const double* amp, const double* delay, const int32_t* row_of, const WaveTable& wt,
                                           const SourceStage& st, hipStream_t stream) {
  if (npts <= 0) return hipSuccess;
  constexpr int n = P + 1;
  const int64_t nblocks = (npts * (n * n) + kPointSourceThreads - 1) / kPointSourceThreads;
  hipLaunchKernelGGL((point_source_wave_kernel<T, P>), dim3((unsigned)nblocks), dim3(kPointSourceThreads), 0, stream, y, cells, dofmap, w,
                     npts, ncells, amp, delay, row_of, wt, st);
  return hipGetLastError();
}

}  // namespace fus
