// libfusgpu.so -- the reduction part of the C ABI (include/fus_gpu_reduce.h: fus_reduce_*) over reduce.hpp.  A translation unit of
// its own: it shares nothing with the operator entry points of fus_gpu.hip but the streaming policy (stream_shape.hpp).
#include "../../include/fus_gpu_reduce.h"

#include <hip/hip_runtime.h>

#include "reduce.hpp"

namespace {

template <typename T>
int reduce_terms(const T* a0, const T* b0, const T* c0, const T* a1, const T* b1, const T* c1, const T* x, int64_t n, double* out4,
                 void* workspace, void* stream) {
  if (n < 0 || !out4 || !workspace || (a0 && !b0) || (a1 && !b1)) return FUS_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(out4)) & 7u) return FUS_ERR_INVALID_ARGUMENT;
  const hipError_t e =
      fus::launch_reduce_terms<T>(a0, b0, c0, a1, b1, c1, x, n, out4, static_cast<double*>(workspace), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? FUS_OK : FUS_ERR_HIP_BASE - (int)e;
}

}  // namespace

extern "C" {

int64_t fus_reduce_workspace_bytes(int64_t n) {
  if (n < 0) return FUS_ERR_INVALID_ARGUMENT;
  const int64_t rows = fus::reduce_rows(n);
  return (rows > 0 ? rows : 1) * fus::kReduceSlots * (int64_t)sizeof(double);
}

int fus_reduce_terms_f64(const double* a0, const double* b0, const double* c0, const double* a1, const double* b1, const double* c1,
                         const double* x, int64_t n, double* out4, void* workspace, void* stream) {
  return reduce_terms<double>(a0, b0, c0, a1, b1, c1, x, n, out4, workspace, stream);
}
int fus_reduce_terms_f32(const float* a0, const float* b0, const float* c0, const float* a1, const float* b1, const float* c1,
                         const float* x, int64_t n, double* out4, void* workspace, void* stream) {
  return reduce_terms<float>(a0, b0, c0, a1, b1, c1, x, n, out4, workspace, stream);
}

}  // extern "C"
