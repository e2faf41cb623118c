/*
 * fus_gpu_nodal.h -- the stiffness apply with a NODAL material coefficient, an extension of the C ABI of include/fus_gpu.h (same
 * library, same conventions and error codes, FUS_ABI_VERSION unchanged: the entry points are additions).  fus_gpu.h, fus_gpu_array.h
 * and fus_gpu_relaxation.h keep their pinned sets of functions; this and every later addition is declared in a header of its own that
 * includes fus_gpu.h.  The ctypes binding derives from this header exactly as from fus_gpu.h (_lib.LATER), and include/fus_gpu.hpp
 * includes it.
 */
#ifndef FUS_GPU_NODAL_H
#define FUS_GPU_NODAL_H

#include "fus_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * y += K(cell_constants * nodal) x with the geometric factor formed in the kernel from the cell's 8 vertices
 * (csrc/stiffness_geom_nodal.hpp):  K = sum_q B_q^T (c_cell nodal(x_q) G_q) B_q.  The GLL rule is collocated, so the coefficient at
 * quadrature point q of a cell is nodal[dofmap[cell][q]]: ``nodal`` is a device vector in the dof numbering of x (at least as long as
 * the largest dof of the plan + 1; owned and ghost dofs), gathered through the plan in the round trip of x.  No G array is read.
 *   cell_constants   T[ncell], a further factor per cell (the linear solver passes -1)
 *   every other argument, the checks and their order: as fus_stiffness_apply_planned_geom_* (the same plan serves both); a null
 *   ``nodal`` is FUS_ERR_INVALID_ARGUMENT.
 * The operator is the one fus_stiffness_apply_planned_* computes from the pre-scaled array G'[c][q][:] = nodal[dofmap[c][q]] G[c][q][:].
 */
int fus_stiffness_apply_planned_geom_nodal_f64(const double* x, const double* cell_constants, const double* nodal, double* y,
                                               const double* x_g, const int32_t* x_dofs, const double* pts, const double* wts,
                                               const void* workspace, const double* dphi, int P, int64_t ncell, void* stream);
int fus_stiffness_apply_planned_geom_nodal_f32(const float* x, const float* cell_constants, const float* nodal, float* y,
                                               const float* x_g, const int32_t* x_dofs, const float* pts, const float* wts,
                                               const void* workspace, const float* dphi, int P, int64_t ncell, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FUS_GPU_NODAL_H */
