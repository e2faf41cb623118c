// Pennes bioheat: the streaming kernel between two stiffness applies of an explicit RK4 stage (fus_bioheat_stage_*).
//
// With GLL collocation M(rho C) dT/dt = -K(k) T - M(w_b rho_b C_b)(T - T_a) + g(t) M(1) q is, per owned dof d,
//     dT/dt = minv[d] b[d] - pr[d] (T[d] - T_a) + g(t) s[d]          b = -K(k) T  (the stiffness apply with the coefficient -k)
// with minv = 1 / M(rho C) 1, pr = M(w_b rho_b C_b) 1 minv, s = M(1) 1 q minv formed once at set-up (bioheat.py).  Dofs held at
// their initial value carry minv = pr = s = 0: no branch here.  One elementwise launch per stage evaluates
//     k = minv b - pr (Tn - T_a) + gate s            Tn = the vector the operator was applied to (T0 itself in the first stage)
// and, with bw = b_i dt and aw = a_{i+1} dt of the classical RK4 tableau,
//   0 FIRST    reads b minv T0 [pr] [s],                      writes acc Tn b:   acc = T0 + bw k ;  Tn = T0 + aw k
//   1 MIDDLE   reads b minv T0 Tn acc [pr] [s],               writes acc Tn b:   acc += bw k     ;  Tn = T0 + aw k
//   2 LAST     reads b minv Tn acc [pr] [s] [cem43] [tmax],   writes T0 b [cem43] [tmax]:   T0 = acc + bw k, then from the new T0
//                  cem43 += (dt / 60) R^(43 - T0)   R = 0.5 for T0 >= 43, 0.25 below   (minutes, always double)
//                  tmax   = max(tmax, T0)
// The dose rule is the one of k-Wave's kWaveDiffusion (once per step, from the step's end temperature).  R^(43 - T) is
// exp2((43 - T) log2 R) in double for an fp32 field too; log2 R is -1 or -2 exactly.  A null pr, s, cem43 or tmax switches the term
// off (uniform over the launch); ``init`` on LAST WRITES cem43 and tmax instead of updating them, as the monitors' first record.
//
// Access shape: ld_chunk / st_chunk of vecops.hpp on the device (one 16-byte access per thread and array, 32-bit offsets from uniform
// bases), stream_shape.hpp on the host (alignment, grid, a launch per 2^27 dofs, the streaming policy): grid-strided over at most
// 2048 workgroups, a scalar tail, and the scalar kernel (W = 1) where an operand is not 16-byte aligned.  LAST of an fp32 field takes 2 dofs per thread (8-byte accesses of the field, one 16-byte access
// of the double dose: launch_bioheat_stage).  LAST is a kernel of its own (template parameter): with the three kinds in one kernel
// the aligned fp64 instantiation needs 103 scalar registers and loses its eighth wave per SIMD.  Updates run over [0, nlocal), b is
// re-zeroed over [0, ntotal) (owned + ghosts: the next apply adds into it).  vector_stream decides non-temporal
// access.  A dof belongs to one thread: no atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vecops.hpp"

namespace fus {

enum { kBioheatFirst = 0, kBioheatMiddle = 1, kBioheatLast = 2 };

template <typename T>
struct BioheatStageArgs {
  T bw, aw, gate, Ta;
  double dt60;  // dt / 60: the step in minutes
  const T *minv, *pr, *s;
  T *b, *T0, *Tn, *acc;
  double* cem43;
  T* tmax;
  int kind, init;
};

// W consecutive owned dofs from ``i``
template <typename T, int W, int NT, bool LAST>
__device__ __forceinline__ void bioheat_group(uint32_t i, const BioheatStageArgs<T>& a) {
  const bool PR = a.pr != nullptr, SRC = a.s != nullptr;  // uniform
  const int kind = LAST ? (int)kBioheatLast : a.kind;
  T rb[W], rm[W], r0[W], rn[W], ra[W], rp[W], rs[W];
#pragma unroll
  for (int k = 0; k < W; ++k) r0[k] = rn[k] = ra[k] = rp[k] = rs[k] = T(0);
  ld_chunk<T, W, NT>(a.b, i, rb);
  ld_chunk<T, W, NT>(a.minv, i, rm);
  if (kind != kBioheatLast) ld_chunk<T, W, NT>(a.T0, i, r0);
  if (kind != kBioheatFirst) {
    ld_chunk<T, W, NT>(a.Tn, i, rn);
    ld_chunk<T, W, NT>(a.acc, i, ra);
  }
  if (PR) ld_chunk<T, W, NT>(a.pr, i, rp);
  if (SRC) ld_chunk<T, W, NT>(a.s, i, rs);
  T o1[W], o2[W];  // FIRST / MIDDLE: acc, Tn; LAST: T0
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const T tn = kind == kBioheatFirst ? r0[k] : rn[k];
    T kk = rm[k] * rb[k];
    if (PR) kk -= rp[k] * (tn - a.Ta);
    if (SRC) kk += a.gate * rs[k];
    o1[k] = (kind == kBioheatFirst ? r0[k] : ra[k]) + a.bw * kk;
    o2[k] = r0[k] + a.aw * kk;
  }
  T z[W];
#pragma unroll
  for (int k = 0; k < W; ++k) z[k] = T(0);
  st_chunk<T, W, NT>(a.b, i, z);
  if constexpr (!LAST) {
    st_chunk<T, W, NT>(a.acc, i, o1);
    st_chunk<T, W, NT>(a.Tn, i, o2);
  } else {
    st_chunk<T, W, NT>(a.T0, i, o1);
    if (a.tmax != nullptr) {
      T mx[W];
#pragma unroll
      for (int k = 0; k < W; ++k) mx[k] = o1[k];
      if (!a.init) ld_chunk<T, W, NT>(a.tmax, i, mx);
#pragma unroll
      for (int k = 0; k < W; ++k) mx[k] = o1[k] > mx[k] ? o1[k] : mx[k];
      st_chunk<T, W, NT>(a.tmax, i, mx);
    }
    if (a.cem43 != nullptr) {
      constexpr int D = W == 1 ? 1 : 2;  // dofs per 16-byte access of the double dose
#pragma unroll
      for (int h = 0; h < W; h += D) {
        double c[D];
#pragma unroll
        for (int k = 0; k < D; ++k) c[k] = 0.0;
        if (!a.init) ld_chunk<double, D, NT>(a.cem43, i + h, c);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double t = (double)o1[h + k];
          c[k] += a.dt60 * exp2((43.0 - t) * (t >= 43.0 ? -1.0 : -2.0));
        }
        st_chunk<double, D, NT>(a.cem43, i + h, c);
      }
    }
  }
}

// ``nlocal`` <= ``ntotal`` < 2^27 + 1 of this launch's piece (launch_bioheat_stage splits)
template <typename T, int W, int NT, bool LAST>
__global__ void __launch_bounds__(256) bioheat_stage_kernel(BioheatStageArgs<T> a, uint32_t nlocal, uint32_t ntotal) {
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const uint32_t sweep = gridDim.x * 256 * W;
  const uint32_t nv = nlocal - nlocal % W;
  for (uint32_t i = gid * W; i < nv; i += sweep) bioheat_group<T, W, NT, LAST>(i, a);
  if constexpr (W > 1) {  // the last nlocal % W owned dofs
    if (nv + gid < nlocal) bioheat_group<T, 1, 0, LAST>(nv + gid, a);
  }
  // the ghost block of b: scalar up to the next multiple of W, 16-byte stores, a scalar tail
  uint32_t g0 = nlocal;
  if constexpr (W > 1) {
    g0 = nlocal + (W - nlocal % W) % W;
    if (g0 > ntotal) g0 = ntotal;
    if (nlocal + gid < g0) a.b[nlocal + gid] = T(0);
  }
  const uint32_t gv = g0 + (ntotal - g0) / W * W;
  T z[W];
#pragma unroll
  for (int k = 0; k < W; ++k) z[k] = T(0);
  for (uint32_t i = g0 + gid * W; i < gv; i += sweep) st_chunk<T, W, NT>(a.b, i, z);
  if constexpr (W > 1) {
    if (gv + gid < ntotal) a.b[gv + gid] = T(0);
  }
}

// kind in [0, 2], 0 <= nlocal <= ntotal, the required pointers non-null: checked by the entry point (fus_gpu.hip)
template <typename T>
inline hipError_t launch_bioheat_stage(T bw, T aw, int kind, T gate, T Ta, double dt, const T* minv, const T* pr, const T* s, T* b, T* T0,
                                       T* Tn, T* acc, double* cem43, T* tmax, bool init, int64_t nlocal, int64_t ntotal,
                                       hipStream_t stream) {
  if (ntotal <= 0) return hipSuccess;
  constexpr int W = 16 / (int)sizeof(T);
  // LAST of an fp32 field: 2 dofs per thread, so that the double dose is ONE 16-byte access per lane, contiguous across the lanes
  // (with 4 dofs it is two accesses per lane at a 32-byte stride, each touching half of every cache line); the field arrays then
  // go in 8-byte accesses, still 512 contiguous bytes per wave and instruction.
  constexpr int WLAST = sizeof(T) == 4 ? 2 : W;
  if (kind != kBioheatLast) cem43 = nullptr, tmax = nullptr;
  const bool aligned = aligned16({minv, pr, s, b, T0, Tn, acc, cem43, tmax});
  const int nt = vector_stream(ntotal * (int64_t)sizeof(T));
  flag_dispatch(kind == kBioheatLast, [&](auto last) {  // one launch per kLaunchDofs dofs: the kernel's offsets are 32-bit
    constexpr bool LAST = decltype(last)::value;
    for_each_piece(ntotal, kLaunchDofs, [&](int64_t at, int64_t len) {
      const int64_t nloc = nlocal <= at ? 0 : (nlocal - at < len ? nlocal - at : len);
      const BioheatStageArgs<T> a{bw, aw, gate, Ta, dt / 60.0, minv + at, piece_of(pr, at), piece_of(s, at), b + at, T0 + at, Tn + at,
                                  acc + at, piece_of(cem43, at), piece_of(tmax, at), kind, (int)init};
      shape_dispatch<(LAST ? WLAST : W)>(aligned, nt, [&](auto w, auto t) {
        hipLaunchKernelGGL((bioheat_stage_kernel<T, decltype(w)::value, decltype(t)::value, LAST>),
                           dim3(stream_blocks(len, decltype(w)::value, kStreamGridCap)), dim3(256), 0, stream, a, (uint32_t)nloc, (uint32_t)len);
      });
    });
  });
  return hipGetLastError();
}

}  // namespace fus
