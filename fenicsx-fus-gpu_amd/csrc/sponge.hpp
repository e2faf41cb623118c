// Absorbing sponge layer: the damping term of  u'' + 2 sigma u' + sigma^2 u = (undamped right-hand side)  in one RK4 stage, as a SPARSE
// launch over the layer's dofs only.  With GLL collocation the mass is diagonal, so per owned dof j of the layer
//   y[idx[k]] -= cv[k] v[idx[k]] + cu[k] u[idx[k]]          cv = 2 sigma_j m_j,  cu = sigma_j^2 m_j,  j = idx[k]
// into the stage's right-hand side y = b before the vector pass divides by the mass (sponge.py forms the list; (u, v) are the
// stage's inputs).  The dense form -- two coefficient vectors read by every vector pass -- would cost every dof ~12 more touches
// per step, the 60-90 % outside the layer included; this one costs the layer's dofs 4 + 5 sizeof(T) bytes per stage and nothing else.
// One thread per list entry, grid-strided.  idx / cu / cv are streamed (read once per launch: non-temporal from vector_stream's
// threshold on their total size); u[idx], v[idx] are gathered (idx ascends, and on a box numbering the layer is a few long runs:
// consecutive lanes mostly read consecutive dofs).  The add is the hardware FP atomic, as the facet kernels' (mass.hpp): next to a
// halo this launch runs on the communicator's stream WHILE the interior cells add into the same y, where a plain load + store
// would lose adds.  No LDS, no scratch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stream_shape.hpp"
#include "vecops.hpp"

namespace fus {

template <typename T, int NT>
__global__ void __launch_bounds__(256)
    sponge_terms_kernel(T* __restrict__ y, const T* __restrict__ u, const T* __restrict__ v, const int32_t* __restrict__ idx,
                        const T* __restrict__ cu, const T* __restrict__ cv, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) {
    const int32_t j = ld_stream<NT>(idx + k);
    const T a = ld_stream<NT>(cv + k), b = ld_stream<NT>(cu + k);
    unsafeAtomicAdd(y + j, -(a * v[j] + b * u[j]));
  }
}

// n == 0: no launch.  At most kStreamGridCap workgroups, as the other streaming launchers.
template <typename T>
inline hipError_t launch_sponge_terms(T* y, const T* u, const T* v, const int32_t* idx, const T* cu, const T* cv, int64_t n,
                                      hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t list_bytes = n * (int64_t)(sizeof(int32_t) + 2 * sizeof(T));
  nt_dispatch(vector_stream(list_bytes), [&](auto nt) {
    hipLaunchKernelGGL((sponge_terms_kernel<T, decltype(nt)::value>), dim3(stream_blocks(n, 1, kStreamGridCap)), dim3(256), 0, stream, y, u,
                       v, idx, cu, cv, n);
  });
  return hipGetLastError();
}

}  // namespace fus
