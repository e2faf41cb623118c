/*
 * fus_gpu_waveform.h -- sampled source waveforms, an extension of the C ABI of include/fus_gpu.h (same library, same conventions and
 * error codes, FUS_ABI_VERSION unchanged: the entry points are additions): the source-facet term and the point-source term of one RK4
 * stage with an arbitrary signal per element / point, interpolated in the kernel from a table in device memory
 * (csrc/source_wave.hpp).  The ctypes binding derives from this header exactly as from fus_gpu.h (_lib.LATER).
 *
 * The table, ``table``: double[nrows][nt][2] in DEVICE memory, 16-byte aligned; row r holds per sample k the value w_r and the
 * derivative dw_r/ds at s_k = t0 + k dt, interleaved.  nrows >= 1, nt >= 2, dt > 0 and finite, t0 finite.  The interpolant is the
 * cubic Hermite of value and derivative on each interval (C1, exact at the nodes), evaluated in fp64 for fp32 fields too:
 *   x = (s - t0) / dt;  x < 0, x > nt - 1 or x not a number: nothing is contributed (the waveform is zero outside its samples)
 *   k = min(floor(x), nt - 2), th = x - k, with the usual basis functions h00, h10, h01, h11 of th
 *   w = h00 w_k + h10 dt d_k + h01 w_{k+1} + h11 dt d_{k+1},   dw = its analytic derivative in s
 * The stage block ``stage`` is the fp64 block {t, w0, A, f0, alpha, D} of fus_facet_source_array_*, of which only t and A are read.
 */
#ifndef FUS_GPU_WAVEFORM_H
#define FUS_GPU_WAVEFORM_H

#include "fus_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Source facets (facet_source_wave_kernel): fus_facet_source_array_* with the element value read from the table.  With
 * e = element_of_facet[f] (-1: inactive), r = row_of_element[e] (outside [0, nrows): a silent element) and s = t - delay[e]:
 *   set A:  y[dmA[f][i]] += amplitude[e] A (w_r(s) cA1[f] + dw_r(s) cA2[f]) detJA[f][i]      (cA2 may be null)
 *   set B:  y[dmB[f][i]] += xB[dmB[f][i]] cB[f] detJB[f][i]                                  (as fus_facet_source_array_*)
 *   amplitude / delay   double[nelem]   (device)        row_of_element   int32[nelem]   (device)
 * in ONE launch, with float atomics; the facet value is rounded to T once.  ``stage`` is in HOST memory (copied into the launch);
 * the _dev variants read it from DEVICE memory (a captured hipGraph replays with new stage times).  nentA + nentB == 0 is a no-op.
 */
int fus_facet_source_wave_f64(double* y, const double* cA1, const double* cA2, const double* detJA, const int32_t* dmA,
                              const int32_t* element_of_facet, int64_t nentA, const double* amplitude, const double* delay,
                              const int32_t* row_of_element, int64_t nelem, const double* table, int64_t nrows, int64_t nt, double t0,
                              double dt, const double* xB, const double* cB, const double* detJB, const int32_t* dmB, int64_t nentB,
                              int N, const double* stage, void* stream);
int fus_facet_source_wave_f32(float* y, const float* cA1, const float* cA2, const float* detJA, const int32_t* dmA,
                              const int32_t* element_of_facet, int64_t nentA, const double* amplitude, const double* delay,
                              const int32_t* row_of_element, int64_t nelem, const double* table, int64_t nrows, int64_t nt, double t0,
                              double dt, const float* xB, const float* cB, const float* detJB, const int32_t* dmB, int64_t nentB, int N,
                              const double* stage, void* stream);
int fus_facet_source_wave_dev_f64(double* y, const double* cA1, const double* cA2, const double* detJA, const int32_t* dmA,
                                  const int32_t* element_of_facet, int64_t nentA, const double* amplitude, const double* delay,
                                  const int32_t* row_of_element, int64_t nelem, const double* table, int64_t nrows, int64_t nt,
                                  double t0, double dt, const double* xB, const double* cB, const double* detJB, const int32_t* dmB,
                                  int64_t nentB, int N, const double* stage_dev, void* stream);
int fus_facet_source_wave_dev_f32(float* y, const float* cA1, const float* cA2, const float* detJA, const int32_t* dmA,
                                  const int32_t* element_of_facet, int64_t nentA, const double* amplitude, const double* delay,
                                  const int32_t* row_of_element, int64_t nelem, const double* table, int64_t nrows, int64_t nt,
                                  double t0, double dt, const float* xB, const float* cB, const float* detJB, const int32_t* dmB,
                                  int64_t nentB, int N, const double* stage_dev, void* stream);

/*
 * Point sources (point_source_wave_kernel): fus_point_source_* (include/fus_gpu_array.h: the same tables cells / dofmap / weights)
 * with the point value read from the table.  With r = row_of_point[p] (outside [0, nrows): a silent point) and s = t - delay[p]:
 *   y[dofmap[c][i n^2 + j n + k]] += amplitude[p] A w_r(s) Lx[i] Ly[j] Lz[k]         c = cells[p]
 *   amplitude / delay   double[npts]   (device)        row_of_point   int32[npts]   (device)
 * ``stage`` is in HOST memory.  A zero value or weight adds nothing; a cell index outside [0, ncells) is skipped.  npts == 0 is a no-op.
 */
int fus_point_source_wave_f64(double* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells,
                              const double* weights, int P, const double* amplitude, const double* delay, const int32_t* row_of_point,
                              const double* table, int64_t nrows, int64_t nt, double t0, double dt, const double* stage, void* stream);
int fus_point_source_wave_f32(float* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const float* weights,
                              int P, const double* amplitude, const double* delay, const int32_t* row_of_point, const double* table,
                              int64_t nrows, int64_t nt, double t0, double dt, const double* stage, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FUS_GPU_WAVEFORM_H */
