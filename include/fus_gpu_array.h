/*
 * fus_gpu_array.h -- the listening side of a transducer array, an extension of the C ABI of include/fus_gpu.h (same library, same
 * conventions and error codes, FUS_ABI_VERSION unchanged: the entry points are additions): point sources inside the volume and what
 * each array element receives.  fus_gpu.h declares the ABI as it stood when its set of functions was pinned
 * (tests/test_abi.py); additions are declared in a header of their own that includes it.  The ctypes binding derives from this header
 * exactly as from fus_gpu.h (_lib.EXTENSIONS), and include/fus_gpu.hpp includes it.
 */
#ifndef FUS_GPU_ARRAY_H
#define FUS_GPU_ARRAY_H

#include "fus_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Point sources (csrc/point_source.hpp): the monopole term q(t) delta(x - x_s) of one RK4 stage, the TRANSPOSE of fus_probe_eval_*
 * over the same tables (cells, dofmap, weights: see there).  With the stage block {t, w0, A, f0, alpha, D} of
 * fus_facet_source_array_* (fp64, HOST memory, copied into the launch) and s = t - delay[p]:
 *   g_p = amplitude[p] A Env(s) cos(w0 s + phase[p])                 (W, Env: as fus_facet_source_array_*)
 *   y[dofmap[c][i n^2 + j n + k]] += g_p Lx[i] Ly[j] Lz[k]           c = cells[p]; evaluated in fp64, rounded to T once
 *   amplitude / phase / delay   double[npts]  (device)
 * The adds are float atomics (points may share dofs, and the launch may run next to a stiffness apply into the same y).  A point
 * with Env == 0 (before its start, after its burst) adds nothing; a cell index outside [0, ncells) is skipped.  npts == 0 is a
 * no-op; f0 > 0, alpha > 0, D >= 0 are checked.  The reference has no counterpart: all its sources are boundary facets.
 */
int fus_point_source_f64(double* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const double* weights,
                         int P, const double* amplitude, const double* phase, const double* delay, const double* stage, void* stream);
int fus_point_source_f32(float* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const float* weights,
                         int P, const double* amplitude, const double* phase, const double* delay, const double* stage, void* stream);

/*
 * Element receivers (csrc/element_receive.hpp): the surface integral of ``u`` over each element of a transducer array,
 *   S_e = sum_{k in [offsets[e], offsets[e + 1])} wgt[k] u[dof[k]]        e < nelem
 *   dof      int32[offsets[nelem]]   the facet-dof entries of the receiving facets, sorted by element (NOT checked, as dofmaps are not)
 *   wgt      T[offsets[nelem]]       their scaled facet detJ (the quadrature weights of the integral)
 *   offsets  int64[nelem + 1]        ascending; an element without entries writes 0
 * summed in double in a fixed order (one workgroup per element, no atomics: two runs give the same bits), rounded to T, and applied to
 * every output whose pointer is non-null:
 *   rec      T[capacity][nelem]      row ``slot`` = S (slot in [0, capacity))
 *   hre / him    double[H][nelem]    += S coef[2h] / += S coef[2h + 1]; coef double[2H] in DEVICE memory (H >= 1)
 * Nothing is normalised: the area of an element is sum wgt, and the partial integrals and areas of partitioned ranks add.
 * nelem == 0 is a no-op.  The reference has no counterpart.
 */
int fus_element_receive_f64(const double* u, const int32_t* dof, const double* wgt, const int64_t* offsets, int64_t nelem, double* rec,
                            int64_t capacity, int slot, double* hre, double* him, const double* coef, int H, void* stream);
int fus_element_receive_f32(const float* u, const int32_t* dof, const float* wgt, const int64_t* offsets, int64_t nelem, float* rec,
                            int64_t capacity, int slot, double* hre, double* him, const double* coef, int H, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FUS_GPU_ARRAY_H */
