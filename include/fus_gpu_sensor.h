/*
 * fus_gpu_sensor.h -- shock capturing, an extension of the C ABI of include/fus_gpu.h (same library, same conventions and error
 * codes, FUS_ABI_VERSION unchanged: the entry points are additions): a smoothness sensor per cell that sets the cell's artificial
 * diffusivity (csrc/modal_sensor.hpp).  The ctypes binding derives from this header exactly as from fus_gpu.h (_lib.LATER).
 *
 * Per cell e of a degree-P spectral hexahedron mesh, with n = P + 1 and the cell's n^3 values of u gathered through ``dofmap``
 * ([ncell, n^3] int32, local dof l = ix n^2 + iy n + iz as everywhere):
 *
 *   modes    = (Vinv x Vinv x Vinv) u_e         Vinv: the n x n table, row-major [mode, node], in the type of u: the inverse of
 *                                               V[j][k] = sqrt((2k + 1) / 2) P_k(2 x_j - 1) at the 1-D nodes x_j in the order the
 *                                               dofmap numbers them.  The modes are then orthonormal on the reference cell [-1, 1]^3.
 *   tot      = sum of modes^2                   over all n^3 modes
 *   top      = sum of modes^2                   over the modes with an index equal to P in any of the three directions
 *   quiet    = tot <= 8 floor^2                 the reference cell has measure 8: the cell's rms against ``floor``
 *   s        = log10(top / tot)
 *   r        = 0 if quiet or s <= s0 - kappa;  1 if s >= s0 + kappa;  else (1 + sin(pi (s - s0) / (2 kappa))) / 2
 *   eps[e]   = max(r eps_max[e], hold eps[e])   eps[e] on the right: the value the array holds on entry
 *   sensor[e]= s, or FUS_SENSOR_QUIET where the cell is quiet or top is not positive (log10 of a ratio of doubles is above -650);
 *              an infinity is never written
 *   cc4[e]   = cc4_base[e] - eps[e] scale[e]    formed in double, stored in the type of u; where eps[e] == 0 the store is
 *              cc4_base[e] bit for bit
 *
 * All pointers but ``stream`` are DEVICE memory.  u, Vinv, cc4_base, scale and cc4 have the type of the suffix; eps_max, eps and
 * sensor are double.  cc4 must not alias cc4_base or scale.  The transform runs in the type of u, the squares and every sum of them in
 * double.  Every sum has a fixed order and there is no atomic operation: two calls on the same data give the same bits, and a captured
 * hipGraph replays the launch as it stands.  One launch; u is only read.
 *
 * FUS_ERR_INVALID_ARGUMENT, and nothing launched: ncell < 0, a null pointer (checked for ncell > 0), kappa not > 0, floor not >= 0,
 * hold outside [0, 1], a NaN among the four scalars.  FUS_ERR_UNSUPPORTED_DEGREE: P outside FUS_MIN_DEGREE .. FUS_MAX_DEGREE.
 * ncell == 0 launches nothing and is FUS_OK.
 */
#ifndef FUS_GPU_SENSOR_H
#define FUS_GPU_SENSOR_H

#include "fus_gpu.h"

#define FUS_SENSOR_QUIET (-1000)

#ifdef __cplusplus
extern "C" {
#endif

int fus_modal_sensor_f64(const double* u, const int32_t* dofmap, const double* Vinv, const double* cc4_base, const double* scale,
                         const double* eps_max, double* eps, double* sensor, double* cc4, int P, int64_t ncell, double s0, double kappa,
                         double floor, double hold, void* stream);
int fus_modal_sensor_f32(const float* u, const int32_t* dofmap, const float* Vinv, const float* cc4_base, const float* scale,
                         const double* eps_max, double* eps, double* sensor, float* cc4, int P, int64_t ncell, double s0, double kappa,
                         double floor, double hold, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FUS_GPU_SENSOR_H */
