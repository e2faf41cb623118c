// Full-field monitors: streaming accumulators over the owned dofs after a recorded time step (fus_field_accumulate_*).
//
// The reference gets its last-period maps (peak pressures, harmonic amplitudes, the heat deposited) by copying the whole
// field to the host every step of its collection window and post-processing there (cuda/demo_nonlinear_bowl.py:662-680,
// cuda/demo_linear_piston.py).  Here one elementwise launch per recorded step updates, per owned dof d, any subset of
//     pmax[d] = max(pmax[d], u[d])    pmin[d] = min(pmin[d], u[d])               T        (comparisons only: bitwise the extrema)
//     usq[d] += u[d]^2                vsq[d] += v[d]^2                           double
//     hre[h][d] += u[d] coef[2h]      him[h][d] += u[d] coef[2h + 1]   h < H     double   (rows ``hstride`` doubles apart)
// with coef = this step's {cos(k w t), -sin(k w t)} in DEVICE memory (the factors of the point sensors, probe.hpp).  A null
// pointer switches an output off.  ``init`` WRITES the accumulators (pmax = pmin = u, usq = u^2, ...) instead of updating
// them: the first record of a window needs no fill launches and reads no stale accumulator.
//
// Access shape: ld_chunk / st_chunk of vecops.hpp on the device, stream_shape.hpp on the host (alignment, grid, pieces, the
// streaming policy).  One 16-byte access per thread and array (W = 2 doubles or 4 floats of the field; the
// double accumulators of an fp32 field are two 16-byte accesses, handled as two halves of 2 dofs so that the fp32 kernel holds
// no more accumulators in registers than the fp64 one: 8 waves per SIMD at H = 4 for both), grid-strided over at most 2048
// workgroups (one launch per 2^27 dofs), a scalar tail, and the scalar kernel (W = 1) for operands that are not 16-byte aligned.  Within a half every
// accumulator load is issued before the first FMA.  Streaming policy: vector_stream -- above 24 MB every access is
// non-temporal (nothing is re-read before ~1 GB of other data has passed, and a plain store would leave dirty lines in the
// memory-side cache that are written back while the next operator runs).  A dof belongs to one thread: no atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vecops.hpp"

namespace fus {

struct FieldAccumulators {
  double *usq, *vsq, *hre, *him;
  int64_t hstride;
};

// W consecutive dofs from ``i``; c = the 2H factors (uniform)
template <typename T, int H, int W, int NT>
__device__ __forceinline__ void field_accumulate_group(uint32_t i, const T* __restrict__ u, const T* __restrict__ v, T* pmax, T* pmin,
                                                       const FieldAccumulators& a, const double (&c)[2 * H + 1], bool init) {
  const bool PEAK = pmax != nullptr, USQ = a.usq != nullptr, VSQ = a.vsq != nullptr;  // uniform
  constexpr int D = W == 1 ? 1 : 2;  // dofs per 16-byte access of a double accumulator
  T ru[W], rv[W];
  ld_chunk<T, W, NT>(u, i, ru);
  if (VSQ) ld_chunk<T, W, NT>(v, i, rv);
#pragma unroll
  for (int s = 0; s < W; s += D) {
    const uint32_t j = i + s;
    T mx[W], mn[W];
    double sq[D], vq[D], re[H + 1][D], im[H + 1][D];
    // -- the identity of an ``init`` record, else every load of this half
#pragma unroll
    for (int k = 0; k < W; ++k) mx[k] = mn[k] = ru[k];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      sq[k] = vq[k] = 0.0;
#pragma unroll
      for (int h = 0; h < H; ++h) re[h][k] = im[h][k] = 0.0;
    }
    if (!init) {
      if (PEAK && s == 0) {
        ld_chunk<T, W, NT>(pmax, i, mx);
        ld_chunk<T, W, NT>(pmin, i, mn);
      }
      if (USQ) ld_chunk<double, D, NT>(a.usq, j, sq);
      if (VSQ) ld_chunk<double, D, NT>(a.vsq, j, vq);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        ld_chunk<double, D, NT>(a.hre + h * a.hstride, j, re[h]);
        ld_chunk<double, D, NT>(a.him + h * a.hstride, j, im[h]);
      }
    }
    // -- the updates
    if (PEAK && s == 0) {
#pragma unroll
      for (int k = 0; k < W; ++k) {
        mx[k] = ru[k] > mx[k] ? ru[k] : mx[k];
        mn[k] = ru[k] < mn[k] ? ru[k] : mn[k];
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double du = (double)ru[s + k];
      if (USQ) sq[k] = __builtin_fma(du, du, sq[k]);
      if (VSQ) {
        const double dv = (double)rv[s + k];
        vq[k] = __builtin_fma(dv, dv, vq[k]);
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
        re[h][k] = __builtin_fma(du, c[2 * h], re[h][k]);
        im[h][k] = __builtin_fma(du, c[2 * h + 1], im[h][k]);
      }
    }
    // -- the stores
    if (PEAK && s == 0) {
      st_chunk<T, W, NT>(pmax, i, mx);
      st_chunk<T, W, NT>(pmin, i, mn);
    }
    if (USQ) st_chunk<double, D, NT>(a.usq, j, sq);
    if (VSQ) st_chunk<double, D, NT>(a.vsq, j, vq);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      st_chunk<double, D, NT>(a.hre + h * a.hstride, j, re[h]);
      st_chunk<double, D, NT>(a.him + h * a.hstride, j, im[h]);
    }
  }
}

template <typename T, int H, int W, int NT>
__global__ void __launch_bounds__(256)
    field_accumulate_kernel(const T* __restrict__ u, const T* __restrict__ v, uint32_t n, T* pmax, T* pmin, FieldAccumulators a,
                            const double* __restrict__ coef, int init) {
  double c[2 * H + 1];  // uniform: loaded once per thread (scalar registers)
#pragma unroll
  for (int k = 0; k < 2 * H; ++k) c[k] = coef[k];
  c[2 * H] = 0.0;
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const uint32_t sweep = gridDim.x * 256 * W;
  const uint32_t nv = n - n % W;
  for (uint32_t i = gid * W; i < nv; i += sweep) field_accumulate_group<T, H, W, NT>(i, u, v, pmax, pmin, a, c, init != 0);
  if constexpr (W > 1) {  // the last n % W dofs
    if (nv + gid < n) field_accumulate_group<T, H, 1, 0>(nv + gid, u, v, pmax, pmin, a, c, init != 0);
  }
}

// H in [0, 4], hstride >= n when H > 0, pmax and pmin both or neither, v where vsq: checked by the entry point (fus_gpu.hip)
template <typename T>
inline hipError_t launch_field_accumulate(const T* u, const T* v, int64_t n, T* pmax, T* pmin, double* usq, double* vsq, double* hre,
                                          double* him, int64_t hstride, const double* coef, int H, bool init, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  constexpr int W = 16 / (int)sizeof(T);
  const bool aligned = aligned16({u, vsq ? v : nullptr, pmax, pmin, usq, vsq, H ? hre : nullptr, H ? him : nullptr}) &&
                       (H == 0 || (hstride & 1) == 0);  // every row of hre / him 16-byte aligned
  const int nt = vector_stream(n * (int64_t)sizeof(T));
  auto launch = [&](auto h) {  // one launch per kLaunchDofs dofs: the kernel's offsets are 32-bit
    for_each_piece(n, kLaunchDofs, [&](int64_t at, int64_t len) {
      const FieldAccumulators a{piece_of(usq, at), piece_of(vsq, at), H ? hre + at : hre, H ? him + at : him, hstride};
      shape_dispatch<W>(aligned, nt, [&](auto w, auto t) {
        hipLaunchKernelGGL((field_accumulate_kernel<T, decltype(h)::value, decltype(w)::value, decltype(t)::value>),
                           dim3(stream_blocks(len, decltype(w)::value, kStreamGridCap)), dim3(256), 0, stream, u + at, vsq ? v + at : v,
                           (uint32_t)len, piece_of(pmax, at), piece_of(pmin, at), a, coef, (int)init);
      });
    });
  };
  switch (H) {
    case 0: launch(std::integral_constant<int, 0>{}); break;
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace fus
