/*
 * fus_gpu_reduce.h -- reductions over a vector, an extension of the C ABI of include/fus_gpu.h (same library, same conventions and
 * error codes, FUS_ABI_VERSION unchanged: the entry points are additions): sums of products, the largest finite magnitude and the
 * number of non-finite entries of the first n entries of device vectors, in one streaming pass (csrc/reduce.hpp).  The ctypes binding
 * derives from this header exactly as from fus_gpu.h (_lib.LATER).
 *
 *   out4[0] = sum_i a0[i] b0[i] c0[i]      c0 null: taken as 1;  a0 null: the sum is 0 and b0, c0 are not read
 *   out4[1] = sum_i a1[i] b1[i] c1[i]      the same rules
 *   out4[2] = max_i |x[i]| over the FINITE entries of x;  0 when there are none or x is null
 *   out4[3] = the number of entries of x that are NaN or +-Inf, as a double
 *
 * All pointers but ``stream`` are DEVICE memory.  The inputs are only read and may alias each other.  Products and sums are formed in
 * double for float inputs too.  A NaN or Inf in an operand of a sum propagates into that sum; out4[2] and out4[3] are how it is found.
 * The order of every addition is a function of n, of whether all operands are 16-byte aligned and of FUS_TUNE_VECTOR_STREAM only: two
 * calls on the same data give the same bits.  No atomics and no state between calls: a captured hipGraph replays as it stands.
 *
 * ``workspace``: at least fus_reduce_workspace_bytes(n) bytes, 8-byte aligned; its contents on entry do not matter, and calls that
 * may run at the same time need one each.  Two launches per call (one more per 2^27 entries); n == 0 still writes four zeros.
 * FUS_ERR_INVALID_ARGUMENT, and nothing launched: n < 0, a null (or not 8-byte aligned) out4 or workspace, an a without its b.
 */
#ifndef FUS_GPU_REDUCE_H
#define FUS_GPU_REDUCE_H

#include "fus_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace a call with this n needs (never 0); FUS_ERR_INVALID_ARGUMENT for n < 0 */
int64_t fus_reduce_workspace_bytes(int64_t n);

int fus_reduce_terms_f64(const double* a0, const double* b0, const double* c0, const double* a1, const double* b1, const double* c1,
                         const double* x, int64_t n, double* out4, void* workspace, void* stream);
int fus_reduce_terms_f32(const float* a0, const float* b0, const float* c0, const float* a1, const float* b1, const float* c1,
                         const float* x, int64_t n, double* out4, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FUS_GPU_REDUCE_H */
