/*
 * fus_gpu_relaxation.h -- power-law tissue absorption through relaxation mechanisms, an extension of the C ABI of include/fus_gpu.h
 * (same library, same conventions and error codes, FUS_ABI_VERSION unchanged: the entry points are additions).  fus_gpu.h declares the
 * ABI as it stood when its set of functions was pinned (tests/test_abi.py); additions are declared in a header of their own that
 * includes it, as fus_gpu_array.h.  The ctypes binding derives from this header exactly as from fus_gpu.h (_lib.ADDITIONS), and
 * include/fus_gpu.hpp includes it.
 */
#ifndef FUS_GPU_RELAXATION_H
#define FUS_GPU_RELAXATION_H

#include "fus_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FUS_RELAX_MAX_MECHANISMS 4

/*
 * Relaxation stage (csrc/relaxation.hpp): the streaming pass that advances the memory variables of NR = nr relaxation mechanisms
 * through one stage of the explicit RK4 step of the wave solvers,
 *   xi_nu' = kappa_nu v - xi_nu / tau_nu          nu < nr,  1 <= nr <= FUS_RELAX_MAX_MECHANISMS
 * and writes the vector the NEXT stage's stiffness applies act on,  ur = u_n + sum_nu xi_nu,n .  With the slope of the stage's inputs
 * k = kappa_nu vn - xin_nu / tau_nu  per owned dof, bw = b_i dt, aw = a_{i+1} dt.  ``kind``:
 *   0 FIRST   (xin of this stage is xi0 itself)  acc = xi0 + bw k ; xin = xi0 + aw k        next = xin
 *   1 MIDDLE                                     acc += bw k      ; xin = xi0 + aw k        next = xin
 *   2 LAST                                       xi0 = acc + bw k                           next = xi0
 *   ur = (u_base + aw_u vn) + sum_nu next_nu     u' = v: the next stage's u_n is u0 + aw_u vn (after LAST: u_base = the new u0, aw_u = 0)
 *   tau           double[nr]  HOST memory, copied into the launch: the relaxation times, each > 0
 *   kappa_scalar  double[nr]  HOST memory, copied into the launch: one weight per mechanism, read where ``kappa`` is NULL
 *   kappa         T[nr][stride]  per-dof weights (device), or NULL: a homogeneous medium reads no weight vector
 *   xi0 xin acc   T[nr][stride]  the state, mechanism-major (device); stride >= nlocal
 *   u_base vn     T[nlocal]      read;   ur  T[nlocal]  written (it may be neither u_base nor vn)
 * Only [0, nlocal) of every row is touched; 16-byte accesses where every pointer is 16-byte aligned and stride * sizeof(T) is a
 * multiple of 16, scalar accesses otherwise.  FUS_ERR_INVALID_ARGUMENT for nr outside 1..4, another kind, a negative size,
 * stride < nlocal, a tau <= 0, or a null tau, xi0, xin, acc, u_base, vn, ur (or kappa and kappa_scalar both null); nlocal == 0 is a
 * no-op.  Each dof is written by one thread: no atomics.  Every device argument is a fixed pointer and the rest are constants, so the
 * launch is captured with the step (hipGraph).  No reference counterpart (its only volume loss is the thermoviscous term).
 */
int fus_relax_stage_f64(double bw, double aw, double aw_u, int kind, int nr, const double* tau, const double* kappa_scalar,
                        const double* kappa, double* xi0, double* xin, double* acc, int64_t stride, const double* u_base,
                        const double* vn, double* ur, int64_t nlocal, void* stream);
int fus_relax_stage_f32(float bw, float aw, float aw_u, int kind, int nr, const double* tau, const double* kappa_scalar,
                        const float* kappa, float* xi0, float* xin, float* acc, int64_t stride, const float* u_base, const float* vn,
                        float* ur, int64_t nlocal, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FUS_GPU_RELAXATION_H */
