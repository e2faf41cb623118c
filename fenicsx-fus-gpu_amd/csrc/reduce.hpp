// Reductions over the owned dofs: the library's one kernel that returns sums and a maximum (fus_reduce_terms_*).
//
// One streaming pass over the first n entries yields four doubles,
//     out[0] = sum a0 b0 c0      out[1] = sum a1 b1 c1        (c taken as 1 when null; the sum is 0 when its a is null)
//     out[2] = max |x| over the FINITE entries of x            (0 when there are none, or x is null)
//     out[3] = the number of non-finite entries of x
// which is what an energy record (v.Mv, u.Ku, max|u|), a weighted dot product of a Lanczos recurrence and a field guard each need.
// A null pointer switches a term off through a uniform branch (as in field_monitor.hpp); the inputs are only read and may alias.
// Products and sums are formed in double for float fields too (a b of two floats is then exact).  A NaN or Inf in a sum operand
// simply propagates into that sum: out[2] and out[3] are how it is found.
//
// Access shape: that of the other streaming kernels -- ld_chunk of vecops.hpp, W = 16 / sizeof(T) entries per thread and array, the
// scalar build (W = 1) for operands that are not 16-byte aligned, grid-strided over at most kStreamGridCap workgroups of 256 with a
// scalar tail, one launch per kLaunchDofs entries, non-temporal loads above kStreamBytes (there are no stores: vector_stream's
// "stores only" answer is the cached build).
//
// Reduction: a fixed order, no float atomics, no counters.  A thread adds its products serially; a wave is reduced with __shfl_down
// over its 64 lanes, the four waves of a block through LDS, and the block's four partials go to row blockIdx of a workspace the caller
// provides.  A second launch of ONE workgroup (reduce_finish_kernel) has each thread add its rows in index order, runs the same tree
// and stores out[0..3]; the rows of every piece of a large vector go through that one launch.  The grid is a function of n, the
// alignment and the streaming mode only, so two calls on the same data are bitwise equal, and a captured graph replays with no state
// to reset (the in-launch "last block reduces" form keeps a counter that every call would have to re-initialise).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vecops.hpp"

namespace fus {

constexpr int kReduceSlots = 4;  // doubles per workspace row and per result

struct ReduceAcc {
  double s0, s1, mx, bad;
};

// the entries [i, i + K) of every term that is switched on
template <typename T, int K, int NT>
__device__ __forceinline__ void reduce_group(uint32_t i, const T* a0, const T* b0, const T* c0, const T* a1, const T* b1, const T* c1,
                                             const T* x, ReduceAcc& r) {
  if (a0 != nullptr) {  // (uniform, as the branches below)
    T ra[K], rb[K];
    ld_chunk<T, K, NT>(a0, i, ra);
    ld_chunk<T, K, NT>(b0, i, rb);
    double t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = (double)ra[k] * (double)rb[k];
    if (c0 != nullptr) {
      T rc[K];
      ld_chunk<T, K, NT>(c0, i, rc);
#pragma unroll
      for (int k = 0; k < K; ++k) t[k] *= (double)rc[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) r.s0 += t[k];
  }
  if (a1 != nullptr) {
    T ra[K], rb[K];
    ld_chunk<T, K, NT>(a1, i, ra);
    ld_chunk<T, K, NT>(b1, i, rb);
    double t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = (double)ra[k] * (double)rb[k];
    if (c1 != nullptr) {
      T rc[K];
      ld_chunk<T, K, NT>(c1, i, rc);
#pragma unroll
      for (int k = 0; k < K; ++k) t[k] *= (double)rc[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) r.s1 += t[k];
  }
  if (x != nullptr) {
    T rx[K];
    ld_chunk<T, K, NT>(x, i, rx);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double ax = __builtin_fabs((double)rx[k]);
      if (ax <= 1.7976931348623157e308)  // finite (false for a NaN)
        r.mx = ax > r.mx ? ax : r.mx;
      else
        r.bad += 1.0;
    }
  }
}

// The tree every level shares: 64 lanes by __shfl_down, then the four waves of the block in wave order through LDS.  The block's
// result is valid in thread 0.
__device__ __forceinline__ void reduce_block(ReduceAcc& r) {
  __shared__ double part[4][kReduceSlots];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    r.s0 += __shfl_down(r.s0, off);
    r.s1 += __shfl_down(r.s1, off);
    const double m = __shfl_down(r.mx, off);
    r.mx = m > r.mx ? m : r.mx;
    r.bad += __shfl_down(r.bad, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = r.s0;
    part[wave][1] = r.s1;
    part[wave][2] = r.mx;
    part[wave][3] = r.bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      r.s0 += part[w][0];
      r.s1 += part[w][1];
      r.mx = part[w][2] > r.mx ? part[w][2] : r.mx;
      r.bad += part[w][3];
    }
  }
}

__device__ __forceinline__ void reduce_store(double* q, const ReduceAcc& r) {
  q[0] = r.s0;
  q[1] = r.s1;
  q[2] = r.mx;
  q[3] = r.bad;
}

template <typename T, int W, int NT>
__global__ void __launch_bounds__(256) reduce_terms_kernel(const T* a0, const T* b0, const T* c0, const T* a1, const T* b1, const T* c1,
                                                           const T* x, uint32_t n, double* rows) {
  ReduceAcc r{0.0, 0.0, 0.0, 0.0};
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const uint32_t sweep = gridDim.x * 256 * W;
  const uint32_t nv = n - n % W;
  for (uint32_t i = gid * W; i < nv; i += sweep) reduce_group<T, W, NT>(i, a0, b0, c0, a1, b1, c1, x, r);
  if constexpr (W > 1) {  // the last n % W entries
    if (nv + gid < n) reduce_group<T, 1, 0>(nv + gid, a0, b0, c0, a1, b1, c1, x, r);
  }
  reduce_block(r);
  if (threadIdx.x == 0) reduce_store(rows + (size_t)blockIdx.x * kReduceSlots, r);
}

// one workgroup: thread t adds the rows t, t + 256, ... in that order
__global__ void __launch_bounds__(256) reduce_finish_kernel(const double* __restrict__ rows, uint32_t nrows, double* __restrict__ out) {
  ReduceAcc r{0.0, 0.0, 0.0, 0.0};
  for (uint32_t i = threadIdx.x; i < nrows; i += 256) {
    const double* q = rows + (size_t)i * kReduceSlots;
    r.s0 += q[0];
    r.s1 += q[1];
    r.mx = q[2] > r.mx ? q[2] : r.mx;
    r.bad += q[3];
  }
  reduce_block(r);
  if (threadIdx.x == 0) reduce_store(out, r);
}

// rows of the workspace that an n-vector can need: those of the scalar build, piece by piece
inline int64_t reduce_rows(int64_t n) {
  int64_t rows = 0;
  for_each_piece(n, kLaunchDofs, [&](int64_t, int64_t len) { rows += stream_blocks(len, 1, kStreamGridCap); });
  return rows;
}

// a without b, n < 0, null out / workspace: refused by the entry point (abi_reduce.hip)
template <typename T>
inline hipError_t launch_reduce_terms(const T* a0, const T* b0, const T* c0, const T* a1, const T* b1, const T* c1, const T* x, int64_t n,
                                      double* out, double* rows, hipStream_t stream) {
  constexpr int W = 16 / (int)sizeof(T);
  if (!a0) b0 = c0 = nullptr;  // operands of a term that is off do not count for the alignment
  if (!a1) b1 = c1 = nullptr;
  const bool aligned = aligned16({a0, b0, c0, a1, b1, c1, x});
  const int nt = vector_stream(n * (int64_t)sizeof(T)) == 1 ? 1 : 0;
  uint32_t at_row = 0;
  for_each_piece(n, kLaunchDofs, [&](int64_t at, int64_t len) {
    shape_dispatch<W>(aligned, nt, [&](auto w, auto t) {
      constexpr int NT = decltype(t)::value == 1 ? 1 : 0;
      const unsigned blocks = stream_blocks(len, decltype(w)::value, kStreamGridCap);
      hipLaunchKernelGGL((reduce_terms_kernel<T, decltype(w)::value, NT>), dim3(blocks), dim3(256), 0, stream, piece_of(a0, at),
                         piece_of(b0, at), piece_of(c0, at), piece_of(a1, at), piece_of(b1, at), piece_of(c1, at), piece_of(x, at),
                         (uint32_t)len, rows + (size_t)at_row * kReduceSlots);
      at_row += blocks;
    });
  });
  hipLaunchKernelGGL(reduce_finish_kernel, dim3(1), dim3(256), 0, stream, rows, at_row, out);
  return hipGetLastError();
}

}  // namespace fus
