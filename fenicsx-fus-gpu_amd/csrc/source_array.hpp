// Phased-array sources: the source-facet term of one RK4 stage with a per-element amplitude, phase and delay.
//
// ``facet_terms_kernel`` (mass.hpp) drives every source facet with one scalar (g(t), dg/dt).  Here each source facet f
// belongs to an element e = eid[f] in [0, E) (or -1: inactive), and with s = t - tau_e
//   g_e(t)  = a_e A Env(s) cos(w0 s + phi_e)
//   W(s)    = 0 (s <= 0),  0.5 (1 - cos(pi f0 s / alpha)) (0 < s < alpha T),  1 (s >= alpha T)      T = 1 / f0
//   Env(s)  = W(s) (continuous wave, D = 0)  or  W(s) W(D - s) (tone burst of duration D)
//   dg_e/dt = its analytic derivative
// so that, per stage,
//   set A:  y[dmA[f][i]] += (g_e(f) cA1[f] + dg_e(f) cA2[f]) detJA[f][i]        (cA2 may be null: linear solver)
//   set B:  y[dmB[f][i]] += xB[dmB[f][i]] cB[f] detJB[f][i]                      (the absorbing term, as facet_terms_kernel)
// A one-element array with a = 1, phi = 0, tau = 0, D = 0 is today's source (linear_solver.source_value,
// nonlinear_solver.source_values) for every t >= 0.
//
// The time arithmetic is fp64 for fp32 fields too (w0 t reaches ~1e3 rad); the facet value is rounded to T once,
// before the add.  The angles go through sincospi (cos(w0 s + phi) = cospi(2 f0 s + phi / pi)): its reduction is exact
// and cheap, where fp64 sin / cos carry a Payne-Hanek path for large arguments (82 VGPRs, 5 waves per SIMD).  Every entry
// re-evaluates its element's value: a few thousand source facets are launch-bound, not ALU-bound.  The kernel is held to
// 64 VGPRs (8 waves per SIMD, no scratch; tests/test_sources.py): next to a halo it is a boundary term that runs WHILE the
// interior stiffness launch holds the CUs and adds into the same y -- hence float atomics, never load + store.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fus {

// the stage block, fp64: what fus_facet_source_array_* copy into the kernel arguments and the _dev variants read from
// device memory (a captured hipGraph is replayed with new times by rewriting it)
struct SourceStage {
  double t;      // stage time
  double w0;     // angular frequency 2 pi f0
  double A;      // source constant (p0 w0 / c0 linear, 2 p0 w0 / c0 Westervelt)
  double f0;     // frequency of the ramp
  double alpha;  // ramp length in periods
  double D;      // burst duration; 0 = continuous wave
};
constexpr int kSourceStageWords = 6;

// W(s) and W'(s), the expressions of linear_solver.source_value / nonlinear_solver.source_values
__device__ inline void source_window(double s, double f0, double alpha, double& w, double& dw) {
  if (s <= 0.0) {
    w = 0.0;
    dw = 0.0;
  } else if (s < (1.0 / f0) * alpha) {
    double sn, cs;
    sincospi(f0 * s / alpha, &sn, &cs);
    w = 0.5 * (1.0 - cs);
    dw = 0.5 * M_PI * f0 / alpha * sn;
  } else {
    w = 1.0;
    dw = 0.0;
  }
}

template <typename T>
__global__ void __launch_bounds__(256, 8)
    facet_source_array_kernel(T* __restrict__ y, const T* __restrict__ cA1, const T* __restrict__ cA2,
                              const T* __restrict__ detJA, const int32_t* __restrict__ dmA, const int32_t* __restrict__ eid,
                              int64_t totalA, const double* __restrict__ amp, const double* __restrict__ phase,
                              const double* __restrict__ delay, const T* __restrict__ xB, const T* __restrict__ cB,
                              const T* __restrict__ detJB, const int32_t* __restrict__ dmB, int64_t totalB, int N,
                              SourceStage st, const double* __restrict__ sdev) {
  if (sdev != nullptr) {
    st.t = sdev[0];
    st.w0 = sdev[1];
    st.A = sdev[2];
    st.f0 = sdev[3];
    st.alpha = sdev[4];
    st.D = sdev[5];
  }
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < totalA + totalB; idx += stride) {
    if (idx < totalA) {
      const int64_t f = idx / N;
      const int e = eid[f];
      if (e < 0) continue;  // inactive facet
      const double s = st.t - delay[e];
      double env, denv;
      source_window(s, st.f0, st.alpha, env, denv);
      if (st.D > 0.0) {
        double w2, dw2;
        source_window(st.D - s, st.f0, st.alpha, w2, dw2);
        denv = denv * w2 - env * dw2;
        env *= w2;
      }
      if (env == 0.0 && denv == 0.0) continue;
      double sn, cs;
      sincospi(2.0 * st.f0 * s + phase[e] * M_1_PI, &sn, &cs);
      const double a = amp[e] * st.A;
      double c = (env * a * cs) * (double)cA1[f];
      if (cA2 != nullptr) c += (denv * a * cs - env * a * st.w0 * sn) * (double)cA2[f];
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
inline hipError_t launch_facet_source_array(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA, const int32_t* eid,
                                            int64_t nentA, const double* amp, const double* phase, const double* delay, const T* xB,
                                            const T* cB, const T* detJB, const int32_t* dmB, int64_t nentB, int N, const SourceStage& st,
                                            const double* sdev, hipStream_t stream) {
  const int64_t total = (nentA + nentB) * (int64_t)N;
  if (total <= 0) return hipSuccess;
  int64_t nblocks = (total + 255) / 256;
  if (nblocks > 4096) nblocks = 4096;
  hipLaunchKernelGGL((facet_source_array_kernel<T>), dim3((unsigned)nblocks), dim3(256), 0, stream, y, cA1, cA2, detJA, dmA, eid,
                     nentA * (int64_t)N, amp, phase, delay, xB, cB, detJB, dmB, nentB * (int64_t)N, N, st, sdev);
  return hipGetLastError();
}

}  // namespace fus
