// Shock capturing: a per-cell smoothness sensor that sets the cell's artificial diffusivity -- CDNA4 (gfx950) kernel.
//
// Persson-Peraire: the share of a cell's energy held by its highest Legendre modes tells a resolved field (the share falls like
// P^-4) from a steepening one (it stays O(1)).  Per cell: gather u through the dofmap, nodal -> modal with ONE n x n table Vinv (the
// inverse of V[j][k] = sqrt((2k+1)/2) P_k(xi_j), so that the modes are orthonormal on [-1, 1]^3), tot = sum of all n^3 squared modes,
// top = the sum over the shell where any of the three indices equals P, s = log10(top / tot), a sine ramp of half-width kappa around
// s0 from 0 to 1, eps = max(ramp * eps_max, hold * eps before), and cc4 = cc4_base - eps * scale: ONE number per cell into the array
// the Westervelt cell pass reads as its second cell constant.  The field is never written.
//
// The shape is stiffness_col_kernel's (stiffness.hpp) without its scatter: n^2 threads per cell, CPB cells per workgroup, thread
// (ty, tz) keeps the column of n values along tx in registers; the dofmap read is contiguous over a cell's threads; every load --
// dofmap, the gather, the lead thread's four per-cell values -- is issued before the first barrier.  The tx direction runs in
// registers against Vinv at compile-time indices (scalar loads), ty and tz through two LDS cubes with the padded cell stride.
//
// The energies are formed in double for float fields too.  A thread squares and adds its n modes in the order kx = 0 .. P; the cell's
// n^2 partial pairs go through LDS in a fixed order (thread (ty, 0) adds its row over tz = 0 .. P into its own slot, the lead thread
// adds the n row sums over ty = 0 .. P), so two launches on the same data give the same bits.  There is no atomic operation.
// The partials reuse the first cube, which is dead by then (fp32, P = 1: they are larger than one cube and run on into the second,
// behind one more barrier), so the kernel's LDS is two cubes and the table.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stiffness.hpp"

namespace fus {

// what sensor[e] holds where log10(top / tot) is not formed: a quiet cell (tot <= 8 floor^2) or one without any top-mode energy
// (FUS_SENSOR_QUIET of include/fus_gpu_sensor.h; log10 of a ratio of doubles is above -650)
constexpr double kSensorQuiet = -1000.0;

template <typename T, int P, int CPB>
struct modal_sensor_lds {
  static constexpr int n2 = (P + 1) * (P + 1);
  static constexpr int cube_bytes = CPB * lds_cell_stride<T, P>() * (int)sizeof(T);
  static constexpr int part_bytes = 2 * CPB * n2 * (int)sizeof(double);
  // the partial pairs lie over the first cube; where they are the larger (fp32, P = 1) they reach into the second, which the tz
  // pass still reads: one more barrier
  static constexpr bool spill = part_bytes > cube_bytes;
  static constexpr int bytes = 2 * cube_bytes;
  static_assert(cube_bytes % 16 == 0 && part_bytes <= bytes, "the partial pairs fit the two cubes");
};

template <typename T, int P, int CPB>
__global__ void __launch_bounds__((col_block_threads<P, CPB>()))
    modal_sensor_kernel(const T* __restrict__ u, const int32_t* __restrict__ dofmap, const T* __restrict__ Vinv,
                        const T* __restrict__ cc4_base, const T* __restrict__ scale, const double* __restrict__ eps_max,
                        double* __restrict__ eps, double* __restrict__ sensor, T* __restrict__ cc4, int64_t ncell, double s0,
                        double kappa, double floor8, double hold) {
  constexpr int n = P + 1, n2 = n * n, Nd = n2 * n;
  constexpr int S = lds_cell_stride<T, P>();
  using L = modal_sensor_lds<T, P, CPB>;

  __shared__ T sV[n2];
  __shared__ __attribute__((aligned(16))) unsigned char raw[L::bytes];
  T* sa = reinterpret_cast<T*>(raw);                   // modes along tx, nodes along ty, tz
  T* sb = reinterpret_cast<T*>(raw + L::cube_bytes);   // modes along tx, ty, nodes along tz
  double* part = reinterpret_cast<double*>(raw);       // (tot, top) of every column, over sa

  const int tid = threadIdx.x;
  const int lc = tid / n2;      // cell within the workgroup
  const int t = tid - lc * n2;  // column id = ty * n + tz
  const int ty = t / n, tz = t - ty * n;
  const int64_t cell = (int64_t)blockIdx.x * CPB + lc;
  const bool active = (lc < CPB) && (cell < ncell);
  const bool lead = active && t == 0;

  if (tid < n2) sV[tid] = Vinv[tid];

  double e_prev = 0.0, e_max = 0.0;
  T c_base = T(0), sc = T(0);
  if (active) {
    const int32_t* dm = dofmap + cell * Nd + t;
    int32_t dof[n];
#pragma unroll
    for (int ix = 0; ix < n; ++ix) dof[ix] = dm[ix * n2];
    if (lead) {
      e_prev = eps[cell];
      e_max = eps_max[cell];
      c_base = cc4_base[cell];
      sc = scale[cell];
    }
    T x[n];
#pragma unroll
    for (int ix = 0; ix < n; ++ix) x[ix] = u[dof[ix]];
    // tx direction: registers x the table at compile-time indices (scalar loads)
    T* ca = sa + lc * S + t;
#pragma unroll
    for (int kx = 0; kx < n; ++kx) {
      T acc = T(0);
#pragma unroll
      for (int ix = 0; ix < n; ++ix) acc += Vinv[kx * n + ix] * x[ix];
      ca[kx * n2] = acc;
    }
  }
  __syncthreads();

  if (active) {  // ty direction: this thread's ty is now the mode index ky
    T vy[n];
#pragma unroll
    for (int i = 0; i < n; ++i) vy[i] = sV[ty * n + i];
    const T* cy = sa + lc * S + tz;  // + kx n^2 + iy n
    T* cb = sb + lc * S + t;
#pragma unroll
    for (int kx = 0; kx < n; ++kx) {
      T acc = T(0);
#pragma unroll
      for (int i = 0; i < n; ++i) acc += vy[i] * cy[kx * n2 + i * n];
      cb[kx * n2] = acc;
    }
  }
  __syncthreads();

  double tot = 0.0, top = 0.0;
  if (active) {  // tz direction, and the column's two energies in double
    T vz[n];
#pragma unroll
    for (int i = 0; i < n; ++i) vz[i] = sV[tz * n + i];
    const T* cz = sb + lc * S + ty * n;  // + kx n^2 + iz
    const bool shell = ty == P || tz == P;
#pragma unroll
    for (int kx = 0; kx < n; ++kx) {
      T acc = T(0);
#pragma unroll
      for (int i = 0; i < n; ++i) acc += vz[i] * cz[kx * n2 + i];
      const double m = (double)acc;
      tot += m * m;
      if (kx == P || shell) top += m * m;
    }
  }
  if constexpr (L::spill) __syncthreads();  // every thread of the workgroup, active or not: the pairs reach into sb
  if (active) {
    part[2 * (lc * n2 + t)] = tot;  // sa is dead since the second barrier
    part[2 * (lc * n2 + t) + 1] = top;
  }
  __syncthreads();

  if (active && tz == 0) {  // the row over tz, in order, into the row's first slot (no other thread reads or writes this row)
    double* row = part + 2 * (lc * n2 + ty * n);
    tot = row[0], top = row[1];
#pragma unroll
    for (int j = 1; j < n; ++j) {
      tot += row[2 * j];
      top += row[2 * j + 1];
    }
    row[0] = tot;
    row[1] = top;
  }
  __syncthreads();

  if (lead) {
    const double* rows = part + 2 * (lc * n2);
    tot = rows[0], top = rows[1];
#pragma unroll
    for (int j = 1; j < n; ++j) {
      tot += rows[2 * j * n];
      top += rows[2 * j * n + 1];
    }
    double s = kSensorQuiet, r = 0.0;
    if (!(tot <= floor8) && top > 0.0) {
      s = log10(top / tot);
      if (s >= s0 + kappa)
        r = 1.0;
      else if (s > s0 - kappa)
        r = 0.5 * (1.0 + sin(1.5707963267948966 * (s - s0) / kappa));
    }
    const double e = fmax(r * e_max, hold * e_prev);
    eps[cell] = e;
    sensor[cell] = s;
    cc4[cell] = e == 0.0 ? c_base : (T)((double)c_base - e * (double)sc);  // a smooth cell keeps its constant bit for bit
  }
}

template <typename T, int P>
inline hipError_t launch_modal_sensor(const T* u, const int32_t* dofmap, const T* Vinv, const T* cc4_base, const T* scale,
                                      const double* eps_max, double* eps, double* sensor, T* cc4, int64_t ncell, double s0,
                                      double kappa, double floor, double hold, hipStream_t stream) {
  constexpr int CPB = default_cells_per_block(P, 256);
  if (ncell <= 0) return hipSuccess;
  const int64_t nblocks = (ncell + CPB - 1) / CPB;
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  constexpr int threads = col_block_threads<P, CPB>();
  hipLaunchKernelGGL((modal_sensor_kernel<T, P, CPB>), dim3((unsigned)nblocks), dim3(threads), 0, stream, u, dofmap, Vinv, cc4_base,
                     scale, eps_max, eps, sensor, cc4, ncell, s0, kappa, 8.0 * floor * floor, hold);
  return hipGetLastError();
}

}  // namespace fus
