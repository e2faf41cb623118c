// Streaming vector kernels of the RK4 stage: axpy, copy, fill, pointwise_divide, square
// (cuda/operators.py:195-274, numba-cpu/operators.py:230-300).  HBM-bound: 16-byte accesses per
// lane when the operands allow it, grid capped at 8 workgroups per CU and grid-strided.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stream_shape.hpp"

namespace fus {

// Streaming policy (template parameter NT: 0 cached accesses, 1 non-temporal loads AND stores, 2 non-temporal stores only) and the
// host side of every launch: stream_shape.hpp.
template <int NT, typename V>
__device__ __forceinline__ V ld_stream(const V* p) {
  if constexpr (NT == 1)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}
template <int NT, typename V>
__device__ __forceinline__ void st_stream(V* p, V v) {
  if constexpr (NT != 0)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// K consecutive values of S at ``q`` as ONE access (K = 1: scalar; K * sizeof(S) = 16, or 8, otherwise), in registers as an array
template <typename S, int K, int NT>
__device__ __forceinline__ void ld_vec(const S* q, S (&r)[K]) {
  if constexpr (K == 1) {
    r[0] = ld_stream<NT>(q);
  } else {
    typedef S VN __attribute__((ext_vector_type(K)));  // native vector: what the non-temporal builtins take
    const VN t = ld_stream<NT>(reinterpret_cast<const VN*>(q));
    __builtin_memcpy(r, &t, sizeof(VN));
  }
}
template <typename S, int K, int NT>
__device__ __forceinline__ void st_vec(S* q, const S (&r)[K]) {
  if constexpr (K == 1) {
    st_stream<NT>(q, r[0]);
  } else {
    typedef S VN __attribute__((ext_vector_type(K)));
    VN t;
    __builtin_memcpy(&t, r, sizeof(VN));
    st_stream<NT>(reinterpret_cast<VN*>(q), t);
  }
}
// The same from element ``o`` of ``p``.  ``p`` is uniform and the byte offset is formed in 32 bits (a launch covers at most kLaunchDofs
// dofs, stream_shape.hpp), so the access is scalar base + one offset register that every array of the same element size shares: 64-bit
// per-lane addresses of up to 12 arrays would cost the H = 4 kernels of field_monitor.hpp their eighth wave per SIMD.
template <typename S, int K, int NT>
__device__ __forceinline__ void ld_chunk(const S* p, uint32_t o, S (&r)[K]) {
  uint32_t ob = o * (uint32_t)sizeof(S);
  asm volatile("" : "+v"(ob));
  ld_vec<S, K, NT>(reinterpret_cast<const S*>(reinterpret_cast<const char*>(p) + ob), r);
}
template <typename S, int K, int NT>
__device__ __forceinline__ void st_chunk(S* p, uint32_t o, const S (&r)[K]) {
  uint32_t ob = o * (uint32_t)sizeof(S);
  asm volatile("" : "+v"(ob));
  st_vec<S, K, NT>(reinterpret_cast<S*>(reinterpret_cast<char*>(p) + ob), r);
}

template <typename T>
struct OpAxpy {  // y = alpha x + y
  T alpha;
  __device__ __forceinline__ T operator()(T a, T b) const { return alpha * a + b; }
};
template <typename T>
struct OpScale {  // out = alpha a
  T alpha;
  __device__ __forceinline__ T operator()(T a, T) const { return alpha * a; }
};
template <typename T>
struct OpCopy {  // out = a
  __device__ __forceinline__ T operator()(T a, T) const { return a; }
};
template <typename T>
struct OpFill {  // out = alpha
  T alpha;
  __device__ __forceinline__ T operator()(T, T) const { return alpha; }
};
template <typename T>
struct OpDiv {  // out = a / b
  __device__ __forceinline__ T operator()(T a, T b) const { return a / b; }
};
template <typename T>
struct OpSquare {  // out = a * a
  __device__ __forceinline__ T operator()(T a, T) const { return a * a; }
};

// out[i] = op(a[i], b[i]);  USE_A / USE_B say which inputs are actually read.  NT: streaming (non-temporal) accesses.
template <typename T, typename Op, bool USE_A, bool USE_B, bool VEC, int NT>
__global__ void __launch_bounds__(256)
    ew_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, int64_t n, Op op) {
  constexpr int W = 16 / (int)sizeof(T);
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if constexpr (VEC) {
    const int64_t nv = n / W;
    for (int64_t i = gid; i < nv; i += stride) {
      T ra[W] = {}, rb[W] = {}, ro[W];
      if constexpr (USE_A) ld_vec<T, W, NT>(a + i * W, ra);
      if constexpr (USE_B) ld_vec<T, W, NT>(b + i * W, rb);
#pragma unroll
      for (int k = 0; k < W; ++k) ro[k] = op(ra[k], rb[k]);
      st_vec<T, W, NT>(out + i * W, ro);
    }
    const int64_t i = nv * W + gid;  // tail
    if (i < n) {
      T sa = T(0), sb = T(0);
      if constexpr (USE_A) sa = a[i];
      if constexpr (USE_B) sb = b[i];
      out[i] = op(sa, sb);
    }
  } else {
    for (int64_t i = gid; i < n; i += stride) {
      T sa = T(0), sb = T(0);
      if constexpr (USE_A) sa = ld_stream<NT>(a + i);
      if constexpr (USE_B) sb = ld_stream<NT>(b + i);
      st_stream<NT>(out + i, op(sa, sb));
    }
  }
}

// y[i] += w[i] * x[i]: the cell mass apply in CACHED-DIAGONAL form.  With GLL collocation the mass operator of
// numba-cpu/operators.py:19-68 is diagonal, M(c) x = (M(c) 1) (.) x, so a driver that applies the same M(c) many times
// assembles w = M(c) 1 once (one gather-scale-scatter apply) and applies 3 vector touches per dof afterwards instead of
// 47.6 B/dof of gather / scatter.  Opt-in (operators.diagonal_mass_operator), its own bytes contract.
template <typename T, bool VEC, int NT>
__global__ void __launch_bounds__(256) muladd_kernel(const T* __restrict__ w, const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  constexpr int W = 16 / (int)sizeof(T);
  typedef T VN __attribute__((ext_vector_type(W)));  // arithmetic on the native vector: with ld_vec's arrays fp32 loses its packed FMAs
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if constexpr (VEC) {
    const int64_t nv = n / W;
    const VN* wv = reinterpret_cast<const VN*>(w);
    const VN* xv = reinterpret_cast<const VN*>(x);
    VN* yv = reinterpret_cast<VN*>(y);
    for (int64_t i = gid; i < nv; i += stride) {
      const VN a = ld_stream<NT>(wv + i), b = ld_stream<NT>(xv + i);
      VN c = ld_stream<NT>(yv + i);
      c += a * b;  // element-wise
      st_stream<NT>(yv + i, c);
    }
    const int64_t i = nv * W + gid;
    if (i < n) y[i] += w[i] * x[i];
  } else {
    for (int64_t i = gid; i < n; i += stride) st_stream<NT>(y + i, ld_stream<NT>(y + i) + ld_stream<NT>(w + i) * ld_stream<NT>(x + i));
  }
}

// Both launchers: VEC where every operand that is read or written is 16-byte aligned, at most kStreamGridCap workgroups.
template <typename T>
inline hipError_t launch_muladd(const T* w, const T* x, T* y, int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  shape_dispatch<16 / (int)sizeof(T)>(aligned16({w, x, y}), vector_stream(n * (int64_t)sizeof(T)), [&](auto wd, auto nt) {
    constexpr int W = decltype(wd)::value;
    hipLaunchKernelGGL((muladd_kernel<T, (W > 1), decltype(nt)::value>), dim3(stream_blocks(n, W, kStreamGridCap)), dim3(256), 0, stream, w, x,
                       y, n);
  });
  return hipGetLastError();
}

template <typename T, typename Op, bool USE_A, bool USE_B>
inline hipError_t launch_ew(const T* a, const T* b, T* out, int64_t n, Op op, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const bool aligned = aligned16({out, USE_A ? a : nullptr, USE_B ? b : nullptr});
  shape_dispatch<16 / (int)sizeof(T)>(aligned, vector_stream(n * (int64_t)sizeof(T)), [&](auto wd, auto nt) {
    constexpr int W = decltype(wd)::value;
    hipLaunchKernelGGL((ew_kernel<T, Op, USE_A, USE_B, (W > 1), decltype(nt)::value>), dim3(stream_blocks(n, W, kStreamGridCap)), dim3(256), 0,
                       stream, a, b, out, n, op);
  });
  return hipGetLastError();
}

}  // namespace fus
