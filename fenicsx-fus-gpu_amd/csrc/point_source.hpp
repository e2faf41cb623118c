// Point sources: the monopole term  q(t) delta(x - x_s)  of one RK4 stage.  Its weak form adds, for a point p in cell c with the 1-D
// Lagrange rows (Lx, Ly, Lz) of its reference coordinates,
//   y[dofmap[c][i n^2 + j n + k]] += g_p(t) Lx[i] Ly[j] Lz[k]
// which is the TRANSPOSE of probe_eval_kernel (probe.hpp): the same tables (``cells``: row of ``dofmap`` per point, ``dofmap``: the rows
// of the distinct cells, ``w[p][3][n]``), built by the same host set-up (sensors.sensor_setup).  The waveform is the array source's
// (source_array.hpp: SourceStage, source_window) with per-POINT amplitude, phase and delay, s = t - tau_p:
//   g_p(t) = a_p A Env(s) cos(w0 s + phi_p)          Env = W(s) (continuous wave, D = 0)  or  W(s) W(D - s) (burst)
// fp64 time arithmetic for fp32 fields too, the angle through sincospi, the value rounded to T once, before the add.
//
// One thread per (point, i, j): a row of n adds along z, the fastest index of the dofmap row.  The outer two loops of the probe are the
// thread index here, so the registers hold one row whatever the degree (the probe's rolled outer loops, transposed).  Several points may
// share a cell or a dof, and next to a halo the launch runs WHILE the interior stiffness launch adds into the same y: float atomics,
// never load + store, as the facet kernels (mass.hpp, source_array.hpp).  A point before its start or after its burst (Env == 0) and a
// zero weight (a point on a node: one-hot rows) issue no atomic; a cell index outside [0, ncells) is skipped, never dereferenced.
// Point counts are 1 to a few thousand: the launch is launch-bound.  No LDS, no scratch, at most 64 VGPRs (tests/test_point_sources.py).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "source_array.hpp"

namespace fus {

constexpr int kPointSourceThreads = 256;

template <typename T, int P>
__global__ void __launch_bounds__(kPointSourceThreads, 8)
    point_source_kernel(T* __restrict__ y, const int32_t* __restrict__ cells, const int32_t* __restrict__ dofmap, const T* __restrict__ w,
                        int64_t npts, int64_t ncells, const double* __restrict__ amp, const double* __restrict__ phase,
                        const double* __restrict__ delay, SourceStage st) {
  constexpr int n = P + 1;
  const int64_t idx = (int64_t)blockIdx.x * kPointSourceThreads + threadIdx.x;
  if (idx >= npts * (n * n)) return;
  const int64_t p = idx / (n * n);
  const int ij = (int)(idx - p * (n * n));
  const int64_t c = cells[p];
  if (c < 0 || c >= ncells) return;  // a point the host did not locate (cannot happen through PointSources)
  const double s = st.t - delay[p];
  double env, denv;
  source_window(s, st.f0, st.alpha, env, denv);
  if (st.D > 0.0) {
    double w2, dw2;
    source_window(st.D - s, st.f0, st.alpha, w2, dw2);
    env *= w2;
  }
  if (env == 0.0) return;
  double sn, cs;
  sincospi(2.0 * st.f0 * s + phase[p] * M_1_PI, &sn, &cs);
  const T* lx = w + p * (3 * n);
  const T* ly = lx + n;
  const T* lz = ly + n;
  const double g = (amp[p] * st.A * env * cs) * ((double)lx[ij / n] * (double)ly[ij % n]);
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
inline hipError_t launch_point_source(T* y, const int32_t* cells, const int32_t* dofmap, const T* w, int64_t npts, int64_t ncells,
                                      const double* amp, const double* phase, const double* delay, const SourceStage& st,
                                      hipStream_t stream) {
  if (npts <= 0) return hipSuccess;
  constexpr int n = P + 1;
  const int64_t nblocks = (npts * (n * n) + kPointSourceThreads - 1) / kPointSourceThreads;
  hipLaunchKernelGGL((point_source_kernel<T, P>), dim3((unsigned)nblocks), dim3(kPointSourceThreads), 0, stream, y, cells, dofmap, w, npts,
                     ncells, amp, phase, delay, st);
  return hipGetLastError();
}

}  // namespace fus
