// Power-law absorption through relaxation mechanisms: the streaming pass of one RK4 stage (fus_relax_stage_*).
//
// Per owned dof and mechanism nu = 1..NR a memory variable obeys  xi_nu' = kappa_nu v - xi_nu / tau_nu , and every stiffness apply
// of the wave solvers acts on  ur = u_n + sum_nu xi_nu,n  in the place of u_n (relaxation.py).  The xi are advanced by the
// RK4 of (u, v); one elementwise launch per stage evaluates, per mechanism, the kind of relax_table.hpp (FIRST / MIDDLE / LAST: the
// three arrays xi0, xin, acc as in bioheat.hpp) with the slope  k = kappa_nu vn - xin_nu / tau_nu  and writes the NEXT stage's
//     ur = (u_base + aw_u vn) + sum_nu next_nu            u' = v: the next stage's u_n is u0 + a_{i+1} dt vn_i
// (after LAST: u_base = the new u0, aw_u = 0).  The state is mechanism-major, [NR][stride] per array: one base pointer and a stride
// for each of xi0, xin, acc and the per-dof weights, so the kernel holds at most 7 bases whatever NR is (bioheat_stage_kernel lost
// a wave per SIMD at nine); the row bases are uniform (scalar adds), the per-lane offset is the one 32-bit register of ld_chunk.
// A null ``kappa`` means one scalar weight per mechanism (a homogeneous medium: no per-dof vector is read).
//
// Access shape: that of bioheat.hpp -- ld_chunk / st_chunk, 16-byte accesses per lane, grid-strided over at most 2048 workgroups,
// a scalar tail, the scalar kernel (W = 1) where an operand or the stride does not allow 16-byte accesses, a launch per 2^27 dofs,
// vector_stream decides non-temporal access.  Only [0, nlocal) is touched (the ghost entries of ur come with the forward scatter).
// A dof belongs to one thread: no atomics, no LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "relax_table.hpp"
#include "vecops.hpp"

namespace fus {

template <typename T, int NR>
struct RelaxStageArgs {
  T bw, aw, aw_u;
  T itau[NR], kappa_s[NR];  // 1 / tau_nu; the scalar weights (read where ``kappa`` is null)
  const T* kappa;           // [NR][stride] per-dof weights, or null
  T *xi0, *xin, *acc;       // [NR][stride]
  const T *u_base, *vn;
  T* ur;
  int64_t stride;
  int kind;
};

// W consecutive owned dofs from ``i``
template <typename T, int NR, int W, int NT, bool PERDOF>
__device__ __forceinline__ void relax_group(uint32_t i, const RelaxStageArgs<T, NR>& a) {
  const RelaxAccess acs = relax_access(a.kind);  // uniform
  T ru[W], rv[W], sum[W];
  ld_chunk<T, W, NT>(a.u_base, i, ru);
  ld_chunk<T, W, NT>(a.vn, i, rv);
#pragma unroll
  for (int k = 0; k < W; ++k) sum[k] = ru[k] + a.aw_u * rv[k];
#pragma unroll
  for (int nu = 0; nu < NR; ++nu) {
    const int64_t row = nu * a.stride;
    T x0[W], xn[W], ac[W], kp[W];
#pragma unroll
    for (int k = 0; k < W; ++k) x0[k] = xn[k] = ac[k] = T(0), kp[k] = PERDOF ? T(0) : a.kappa_s[nu];
    if (acs.rd_x0) ld_chunk<T, W, NT>(a.xi0 + row, i, x0);
    if (acs.rd_xn) ld_chunk<T, W, NT>(a.xin + row, i, xn);
    if (acs.rd_acc) ld_chunk<T, W, NT>(a.acc + row, i, ac);
    if constexpr (PERDOF) ld_chunk<T, W, NT>(a.kappa + row, i, kp);
    T o0[W], on[W], oa[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const RelaxOut<T> o = relax_update<T>(a.kind, a.bw, a.aw, kp[k], a.itau[nu], rv[k], x0[k], xn[k], ac[k]);
      o0[k] = o.x0, on[k] = o.xn, oa[k] = o.acc;
      sum[k] += o.next;
    }
    if (acs.wr_x0) st_chunk<T, W, NT>(a.xi0 + row, i, o0);
    if (acs.wr_xn) st_chunk<T, W, NT>(a.xin + row, i, on);
    if (acs.wr_acc) st_chunk<T, W, NT>(a.acc + row, i, oa);
  }
  st_chunk<T, W, NT>(a.ur, i, sum);
}

// ``nlocal`` < 2^27 + 1 of this launch's piece (launch_relax_stage splits).  PERDOF (per-dof weights or one scalar per mechanism) is a
// template parameter: with both forms in one kernel the aligned fp64 NR = 4 build holds the weights' row bases AND the scalars, 106
// scalar registers, and loses its eighth wave per SIMD.
template <typename T, int NR, int W, int NT, bool PERDOF>
__global__ void __launch_bounds__(256) relax_stage_kernel(RelaxStageArgs<T, NR> a, uint32_t nlocal) {
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const uint32_t sweep = gridDim.x * 256 * W;
  const uint32_t nv = nlocal - nlocal % W;
  for (uint32_t i = gid * W; i < nv; i += sweep) relax_group<T, NR, W, NT, PERDOF>(i, a);
  if constexpr (W > 1) {  // the last nlocal % W owned dofs
    if (nv + gid < nlocal) relax_group<T, NR, 1, 0, PERDOF>(nv + gid, a);
  }
}

// kind in [0, 2], 1 <= NR <= 4, 0 <= nlocal <= stride, the required pointers non-null: checked by the entry point (fus_gpu.hip)
template <typename T, int NR>
inline hipError_t launch_relax_stage(T bw, T aw, T aw_u, int kind, const double* tau, const double* kappa_scalar, const T* kappa, T* xi0,
                                     T* xin, T* acc, int64_t stride, const T* u_base, const T* vn, T* ur, int64_t nlocal,
                                     hipStream_t stream) {
  if (nlocal <= 0) return hipSuccess;
  constexpr int W = 16 / (int)sizeof(T);
  // every row of the packed arrays must start 16-byte aligned for the wide form: the bases and the stride
  const bool aligned = aligned16({kappa, xi0, xin, acc, u_base, vn, ur}) && stride % W == 0;
  const int nt = vector_stream(nlocal * (int64_t)sizeof(T));
  for_each_piece(nlocal, kLaunchDofs, [&](int64_t at, int64_t len) {
    RelaxStageArgs<T, NR> a{};
    a.bw = bw, a.aw = aw, a.aw_u = aw_u;
    for (int nu = 0; nu < NR; ++nu) a.itau[nu] = (T)(1.0 / tau[nu]), a.kappa_s[nu] = kappa_scalar ? (T)kappa_scalar[nu] : T(0);
    a.kappa = piece_of(kappa, at), a.xi0 = xi0 + at, a.xin = xin + at, a.acc = acc + at;
    a.u_base = u_base + at, a.vn = vn + at, a.ur = ur + at, a.stride = stride, a.kind = kind;
    flag_dispatch(kappa != nullptr, [&](auto perdof) {
      shape_dispatch<W>(aligned, nt, [&](auto w, auto t) {
        hipLaunchKernelGGL((relax_stage_kernel<T, NR, decltype(w)::value, decltype(t)::value, decltype(perdof)::value>),
                           dim3(stream_blocks(len, decltype(w)::value, kStreamGridCap)), dim3(256), 0, stream, a, (uint32_t)len);
      });
    });
  });
  return hipGetLastError();
}

}  // namespace fus
