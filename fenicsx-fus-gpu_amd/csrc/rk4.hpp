// Fused RK4 stage vector kernel.
//
// Between two operator applications the reference launches, per stage, 12 streaming kernels
// (cuda/demo_linear_box.py:491-563: 5 copy, 4 axpy, 2 fill, 1 pointwise_divide = 216 B/dof).
// Everything after scatter_rev(b) of stage i and before scatter_fwd of stage i+1 is elementwise,
// so it is ONE kernel here (88-104 B/dof):
//     kv  = b * minv                       pointwise_divide(b, m, kv)   :556   (1/m precomputed, cf. the
//                                                                       "store 1/m" TODO cpp/common/Linear.hpp:216-218)
//     u  += bw * ku ;  v += bw * kv        axpy x2                      :562-563   bw = b_runge[i] dt
//     [new step: u0 = u ; v0 = v]          copy x2                      :491-492
//     un  = u0 + aw * ku                   copy + axpy                  :496,499    aw = a_runge[i+1] dt
//     vn  = v0 + aw * kv                   copy + axpy                  :497,500
//     ku  = vn                             copy (f0)                    :508  (ku doubles as v_n: same values)
//     b   = 0                              fill                         :541
// kv is never stored.  Updates run over the owned dofs [0, nlocal); b is zeroed over
// [0, ntotal) (owned + ghosts), ghost values of un / ku are refreshed by the forward scatter.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rk4_table.hpp"
#include "vecops.hpp"

namespace fus {

// The stage kinds (what ``kind`` -- the ABI's ``new_step`` -- computes, reads and writes, and the touch counts): rk4_table.hpp.
// W dofs per thread as ONE 16-byte access per array where the arrays are 16-byte aligned (W = 2 doubles / 4 floats), scalar
// otherwise.  NT (vectors far larger than the caches: stream_shape.hpp vector_stream): EVERY access non-temporal.  The loads: the
// pass re-reads nothing before ~1 GB of other data has gone through the caches.  The stores -- un, ku and b included, although
// the next kernel reads them: a line written with a plain store stays dirty in the memory-side Infinity Cache and is written
// back WHILE THE OPERATOR RUNS (its launch takes 251-272 us after a plain-store vector pass against 219-222 us after a busy
// wait or a read-only stream: profiles/r04i_interleave_probe.log); re-reading 82 MB of un from HBM is the cheaper side.
template <typename T, int W, int NT>
__global__ void __launch_bounds__(256)
    rk4_stage_kernel(T bw, T aw, int kind, const T* __restrict__ minv, T* __restrict__ b, T* __restrict__ u,
                     T* __restrict__ v, T* __restrict__ u0, T* __restrict__ v0, T* __restrict__ ku,
                     T* __restrict__ un, int64_t nlocal, int64_t ntotal) {
  const int64_t stride = (int64_t)gridDim.x * 256 * W;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W; i < ntotal; i += stride) {
    if (i + W <= nlocal) {
      T rb[W], rm[W], ru[W], rv[W], ru0[W], rv0[W], rku[W];
      ld_vec<T, W, NT>(b + i, rb);
      ld_vec<T, W, NT>(minv + i, rm);
      const Rk4Access a = rk4_access(kind);
      if (a.rd_u) ld_vec<T, W, NT>(u + i, ru);
      if (a.rd_v) ld_vec<T, W, NT>(v + i, rv);
      if (a.rd_0) {
        ld_vec<T, W, NT>(u0 + i, ru0);
        ld_vec<T, W, NT>(v0 + i, rv0);
      }
      if (a.rd_ku) ld_vec<T, W, NT>(ku + i, rku);
      T ou[W], ov[W], ou0[W], ov0[W], oun[W], oku[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const Rk4Out<T> o = rk4_update<T>(kind, bw, aw, Rk4In<T>{ru[k], rv[k], ru0[k], rv0[k], rku[k]}, rb[k] * rm[k]);
        ou[k] = o.u, ov[k] = o.v, ou0[k] = o.u0, ov0[k] = o.v0, oun[k] = o.un, oku[k] = o.ku;
      }
      if (a.wr_u) st_vec<T, W, NT>(u + i, ou);
      if (a.wr_v) st_vec<T, W, NT>(v + i, ov);
      if (a.wr_n) {
        st_vec<T, W, NT>(un + i, oun);
        st_vec<T, W, NT>(ku + i, oku);
      }
      if (a.wr_u0) st_vec<T, W, NT>(u0 + i, ou0);
      if (a.wr_v0) st_vec<T, W, NT>(v0 + i, ov0);
      T z[W];
#pragma unroll
      for (int k = 0; k < W; ++k) z[k] = T(0);
      st_vec<T, W, NT>(b + i, z);
    } else {  // the last owned dofs (nlocal not a multiple of W) and the ghost block of b
      for (int64_t j = i; j < i + W && j < ntotal; ++j) {
        if (j < nlocal) {
          const Rk4Access a = rk4_access(kind);
          const T kv = b[j] * minv[j];
          const Rk4In<T> in{a.rd_u ? u[j] : T(0), a.rd_v ? v[j] : T(0), a.rd_0 ? u0[j] : T(0), a.rd_0 ? v0[j] : T(0), a.rd_ku ? ku[j] : T(0)};
          const Rk4Out<T> o = rk4_update<T>(kind, bw, aw, in, kv);
          if (a.wr_u) u[j] = o.u;
          if (a.wr_v) v[j] = o.v;
          if (a.wr_n) un[j] = o.un, ku[j] = o.ku;
          if (a.wr_u0) u0[j] = o.u0;
          if (a.wr_v0) v0[j] = o.v0;
        }
        b[j] = T(0);
      }
    }
  }
}

template <typename T>
inline hipError_t launch_rk4_stage(T bw, T aw, int new_step, const T* minv, T* b, T* u, T* v, T* u0, T* v0, T* ku,
                                   T* un, int64_t nlocal, int64_t ntotal, hipStream_t stream) {
  if (ntotal <= 0) return hipSuccess;
  const bool aligned = aligned16({minv, b, u, v, u0, v0, ku, un});
  shape_dispatch<16 / (int)sizeof(T)>(aligned, vector_stream(ntotal * (int64_t)sizeof(T)), [&](auto w, auto nt) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL((rk4_stage_kernel<T, W, decltype(nt)::value>), dim3(stream_blocks(ntotal, W, kStageGridCap)), dim3(256), 0, stream, bw,
                       aw, new_step, minv, b, u, v, u0, v0, ku, un, nlocal, ntotal);
  });
  return hipGetLastError();
}

}  // namespace fus
