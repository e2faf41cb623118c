/*
 * fus_gpu_westervelt_nodal.h -- the Westervelt cell pass with NODAL material coefficients, an extension of the C ABI of
 * include/fus_gpu.h (same library, same conventions and error codes, FUS_ABI_VERSION unchanged: the entry points are additions).
 * Declared in a header of its own that includes fus_gpu.h, as every addition since the pinned sets; the ctypes binding derives from
 * this header exactly as from fus_gpu.h (_lib.LATER), and include/fus_gpu.hpp includes it.
 */
#ifndef FUS_GPU_WESTERVELT_NODAL_H
#define FUS_GPU_WESTERVELT_NODAL_H

#include "fus_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * b += sum_q B_q^T G_q ( c3 nodal3(x_q) grad u(x_q) + c4 nodal4(x_q) grad v(x_q) ), the geometric factor formed in the kernel from the
 * cell's 8 vertices (csrc/westervelt_geom_nodal.hpp): the stiffness part of the Westervelt cell pass with a coefficient per DOF on
 * each of its two inputs.  The GLL rule is collocated, so the coefficient at quadrature point q of a cell is nodal[dofmap[cell][q]]:
 * ``nodal3`` / ``nodal4`` are device vectors in the dof numbering of u (at least as long as the largest dof of the plan + 1; owned
 * and ghost dofs), gathered through the plan in the round trip of u and v.  No G array is read, and there is no mass part.
 *   c3, c4   T[ncell], a further factor per cell on each input (the solver passes -1)
 *   every other argument, the checks and their order: as fus_stiffness_apply_planned_geom_nodal_* (the same plan serves both); a
 *   null ``nodal3`` / ``nodal4`` is FUS_ERR_INVALID_ARGUMENT.
 * The result is the one two calls of fus_stiffness_apply_planned_geom_nodal_* give, (u, c3, nodal3) then (v, c4, nodal4), with one
 * plan read, one backward contraction and one atomic per distinct dof instead of two.
 */
int fus_westervelt_stiffness_apply_planned_geom_nodal_f64(const double* u, const double* v, const double* c3, const double* c4,
                                                          const double* nodal3, const double* nodal4, double* b, const double* x_g,
                                                          const int32_t* x_dofs, const double* pts, const double* wts,
                                                          const void* workspace, const double* dphi, int P, int64_t ncell, void* stream);
int fus_westervelt_stiffness_apply_planned_geom_nodal_f32(const float* u, const float* v, const float* c3, const float* c4,
                                                          const float* nodal3, const float* nodal4, float* b, const float* x_g,
                                                          const int32_t* x_dofs, const float* pts, const float* wts,
                                                          const void* workspace, const float* dphi, int P, int64_t ncell, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FUS_GPU_WESTERVELT_NODAL_H */
