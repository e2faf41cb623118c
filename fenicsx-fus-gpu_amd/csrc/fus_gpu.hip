// libfusgpu.so -- C ABI (include/fus_gpu.h) over the CDNA4 kernels in this directory: every entry point but the communicator and halo
// exchange (abi_halo.hip).  Each typed entry point is a template here or in a dispatch_*.hip, which holds every check and the launch;
// its _f64 / _f32 twins are one-line forwards stamped by FUS_TYPED at the end of this file.
// Build: see Makefile (hipcc --offload-arch=gfx950).
#include "../../include/fus_gpu.h"
#include "../../include/fus_gpu_array.h"
#include "../../include/fus_gpu_relaxation.h"
#include "../../include/fus_gpu_nodal.h"
#include "../../include/fus_gpu_westervelt_nodal.h"
#include "../../include/fus_gpu_waveform.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "bioheat.hpp"
#include "element_receive.hpp"
#include "field_monitor.hpp"
#include "fus_dispatch.hpp"
#include "geometry.hpp"
#include "halo.hpp"
#include "mass.hpp"
#include "mass_gather.hpp"
#include "plan_build.hpp"
#include "point_source.hpp"
#include "probe.hpp"
#include "relaxation.hpp"
#include "rk4.hpp"
#include "source_array.hpp"
#include "source_wave.hpp"
#include "sponge.hpp"
#include "stiffness.hpp"
#include "vecops.hpp"
#include "westervelt.hpp"

using namespace fus_abi;

namespace {

// what was built in which workspace: batch plans, transposed gather plans of the atomic-free mass apply and their static companions
PlanRegistry<fus::GatherHeader> g_registry;

template <typename T, int P>
hipError_t stiffness_dispatch_variant(const T* x, const T* cc, T* y, const T* G, const int32_t* dofmap,
                                      const T* dphi, int64_t ncell, hipStream_t s) {
  const int variant = g_stiffness_variant.load(std::memory_order_relaxed);
  const int remap = g_xcd_remap.load(std::memory_order_relaxed);
  constexpr int CPB256 = fus::default_cells_per_block(P, 256);
  constexpr int CPB128 = fus::default_cells_per_block(P, 128);
  switch (variant) {
    case 1:  // ~128-thread workgroups
      return fus::launch_stiffness_col<T, P, CPB128>(x, cc, y, G, dofmap, dphi, ncell, remap, s);
    default:  // ~256-thread workgroups
      return fus::launch_stiffness_col<T, P, CPB256>(x, cc, y, G, dofmap, dphi, ncell, remap, s);
  }
}

template <typename T>
int stiffness_apply(const T* x, const T* cc, T* y, const T* G, const int32_t* dofmap, const T* dphi, int P,
                    int64_t ncell, void* stream) {
  if (ncell < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  if (ncell == 0) return FUS_OK;
  if (!x || !cc || !y || !G || !dofmap || !dphi) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(G, 2 * sizeof(T)) || misaligned(x, sizeof(T)) || misaligned(y, sizeof(T)) ||
      misaligned(dofmap, sizeof(int32_t)))
    return FUS_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipErrorInvalidValue;
  degree_dispatch(P, [&](auto p) { e = stiffness_dispatch_variant<T, decltype(p)::value>(x, cc, y, G, dofmap, dphi, ncell, s); });
  return hip_rc(e);
}

template <typename T>
int mass_apply(const T* x, const T* consts, T* y, const T* detJ, const int32_t* dofmap, int N, int64_t nent,
               void* stream) {
  if (nent < 0 || N < 1) return FUS_ERR_INVALID_ARGUMENT;
  if (nent == 0) return FUS_OK;
  if (!x || !consts || !y || !detJ || !dofmap) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_mass<T>(x, consts, y, detJ, dofmap, N, nent, static_cast<hipStream_t>(stream)));
}

template <typename T, typename Op, bool UA, bool UB>
int ew(const T* a, const T* b, T* out, int64_t n, Op op, void* stream) {
  if (n < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (n == 0) return FUS_OK;
  if (!out || (UA && !a) || (UB && !b)) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_ew<T, Op, UA, UB>(a, b, out, n, op, static_cast<hipStream_t>(stream)));
}

template <typename T, int MODE>
int halo(const T* in, T* out, const int64_t* index, int64_t count, int64_t offset, void* stream) {
  if (count < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (count == 0) return FUS_OK;
  if (!in || !out || !index) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_halo<T, MODE>(in, out, index, count, offset, static_cast<hipStream_t>(stream)));
}

template <typename T>
int muladd(const T* w, const T* x, T* y, int64_t n, void* stream) {
  if (n < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (n == 0) return FUS_OK;
  if (!w || !x || !y) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_muladd<T>(w, x, y, n, static_cast<hipStream_t>(stream)));
}

template <typename T>
int mass_apply_planned(const T* x, const T* consts, T* y, const T* detJ, const void* ws, int N, int epb,
                              int64_t nent, void* stream) {
  if (nent < 0 || N < 2 || epb < 1 || (int64_t)N * epb > fus::kPlanMaxEntries) return FUS_ERR_INVALID_ARGUMENT;
  if (nent == 0) return FUS_OK;
  if (!x || !consts || !y || !detJ || !ws || misaligned(ws, 256)) return FUS_ERR_INVALID_ARGUMENT;
  bool ord = false, excl = false;
  bool rp = true;
  if (!plan_check(ws, N, epb, nent, &ord, &excl, &rp)) return FUS_ERR_PLAN_MISMATCH;
  return hip_rc(fus::launch_mass_plan<T>(x, consts, y, detJ, ws, N, epb, nent, static_cast<hipStream_t>(stream), ord, plan_use_runs<T>(N, rp), excl));
}

// a transposed gather plan at ``ws`` for exactly this shape, copied out
bool gather_check(const void* ws, int N, int64_t nent, fus::GatherHeader* h) {
  return g_registry.get(ws, h) && h->N == N && h->nent == nent;
}

template <typename T>
int mass_apply_gather(const T* x, const T* c, T* y, const T* detJ, const void* ws, int N, int64_t nent, void* stream) {
  if (nent < 0 || N < 1) return FUS_ERR_INVALID_ARGUMENT;
  fus::GatherHeader h{};
  if (!gather_check(ws, N, nent, &h)) return FUS_ERR_PLAN_MISMATCH;
  if (nent == 0) return FUS_OK;
  if (!x || !c || !y || !detJ) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_mass_gather<T>(x, c, y, detJ, ws, h, static_cast<hipStream_t>(stream),
                                           g_mass_variant.load(std::memory_order_relaxed)));
}

template <typename T>
int mass_gather_static_build(const void* ws, const T* detJ, void* sws, int64_t sws_bytes, void* stream) {
  fus::GatherHeader h{};
  if (!g_registry.get(ws, &h)) return FUS_ERR_PLAN_MISMATCH;
  if (!sws || misaligned(sws, 256) || (h.nent > 0 && !detJ)) return FUS_ERR_INVALID_ARGUMENT;
  if (sws_bytes < fus::gather_static_bytes(h.nent, (int)h.N, h.nent * h.N, (int)sizeof(T))) return FUS_ERR_INVALID_ARGUMENT;
  int too_wide = 0;
  const hipError_t e = fus::gather_static_build<T>(ws, h, detJ, sws, static_cast<hipStream_t>(stream), &too_wide);
  if (e != hipSuccess) return hip_rc(e);
  if (too_wide) return FUS_ERR_UNSUPPORTED_ENTITY;
  g_registry.put(sws, GatherStaticInfo{ws, (int)sizeof(T)});
  return FUS_OK;
}

template <typename T>
int mass_apply_gather_static(const T* x, const T* c, T* y, const void* ws, const void* sws, int N, int64_t nent, void* stream) {
  if (nent < 0 || N < 1) return FUS_ERR_INVALID_ARGUMENT;
  fus::GatherHeader h{};
  GatherStaticInfo st{};
  if (!gather_check(ws, N, nent, &h)) return FUS_ERR_PLAN_MISMATCH;
  if (!g_registry.get(sws, &st) || st.plan != ws || st.elem_bytes != (int)sizeof(T)) return FUS_ERR_PLAN_MISMATCH;
  if (nent == 0) return FUS_OK;
  if (!x || !c || !y) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_mass_gather_static<T>(x, c, y, ws, h, const_cast<void*>(sws), static_cast<hipStream_t>(stream),
                                                  g_mass_variant.load(std::memory_order_relaxed)));
}

// the transposed plan of ``dofmap`` (of its rows in ``row_set`` == ``which``, if given) into a workspace the caller has checked
int gather_plan_build(const int32_t* dofmap, int N, int64_t nent, int64_t ndofs, const uint8_t* row_set, int which, void* workspace,
                      void* stream) {
  if (nent > 0 && !dofmap) return FUS_ERR_INVALID_ARGUMENT;
  fus::GatherHeader h{};
  int bad = 0;
  const hipError_t e = fus::gather_plan_build(dofmap, N, nent, ndofs, workspace, static_cast<hipStream_t>(stream), &h, &bad, row_set, which);
  if (e != hipSuccess) return hip_rc(e);
  if (bad) return FUS_ERR_UNSUPPORTED_ENTITY;
  g_registry.put(workspace, h);
  return FUS_OK;
}

// point sensors (csrc/probe.hpp): every check before any device work; npts == 0 is a no-op
template <typename T>
int probe_eval(const T* u, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights, int P, T* rec,
               int64_t capacity, int slot, double* pmax, double* pmin, double* hre, double* him, const double* coef, int H,
               void* stream) {
  if (npts < 0 || ncells < 0 || capacity < 0 || H < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  if (npts == 0) return FUS_OK;
  if (!u || !cells || !dofmap || !weights) return FUS_ERR_INVALID_ARGUMENT;
  if (rec && (slot < 0 || slot >= capacity)) return FUS_ERR_INVALID_ARGUMENT;
  if ((hre || him || H > 0) && (!hre || !him || !coef || H < 1)) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(u, sizeof(T)) || misaligned(weights, sizeof(T)) || misaligned(cells, sizeof(int32_t)) ||
      misaligned(dofmap, sizeof(int32_t)))
    return FUS_ERR_INVALID_ARGUMENT;
  T* row = rec ? rec + (int64_t)slot * npts : nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipErrorInvalidValue;
  degree_dispatch(P, [&](auto p) {
    e = fus::launch_probe_eval<T, decltype(p)::value>(u, cells, dofmap, weights, npts, ncells, row, pmax, pmin, hre, him, coef, H, s);
  });
  return hip_rc(e);
}

// point sources (csrc/point_source.hpp), the transpose of probe_eval: every check before any device work; npts == 0 is a no-op.
// ``stage``: the fp64 block {t, w0, A, f0, alpha, D} in host memory, copied into the launch.
template <typename T>
int point_source(T* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights, int P,
                 const double* amp, const double* phase, const double* delay, const double* stage, void* stream) {
  if (npts < 0 || ncells < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  if (npts == 0) return FUS_OK;
  if (!y || !cells || !dofmap || !weights || !amp || !phase || !delay || !stage) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(y, sizeof(T)) || misaligned(weights, sizeof(T)) || misaligned(cells, sizeof(int32_t)) ||
      misaligned(dofmap, sizeof(int32_t)) || misaligned(stage, sizeof(double)) || misaligned(amp, sizeof(double)) ||
      misaligned(phase, sizeof(double)) || misaligned(delay, sizeof(double)))
    return FUS_ERR_INVALID_ARGUMENT;
  const fus::SourceStage st{stage[0], stage[1], stage[2], stage[3], stage[4], stage[5]};
  // a NaN fails every comparison: f0 and alpha must be positive, D zero (continuous wave) or positive
  if (!(st.f0 > 0.0) || !(st.alpha > 0.0) || !(st.D >= 0.0)) return FUS_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipErrorInvalidValue;
  degree_dispatch(P, [&](auto p) {
    e = fus::launch_point_source<T, decltype(p)::value>(y, cells, dofmap, weights, npts, ncells, amp, phase, delay, st, s);
  });
  return hip_rc(e);
}

// element receivers (csrc/element_receive.hpp): every check before any device work; nelem == 0 is a no-op
template <typename T>
int element_receive(const T* u, const int32_t* dof, const T* wgt, const int64_t* offsets, int64_t nelem, T* rec, int64_t capacity,
                    int slot, double* hre, double* him, const double* coef, int H, void* stream) {
  if (nelem < 0 || capacity < 0 || H < 0 || nelem > 0x7fffffffLL) return FUS_ERR_INVALID_ARGUMENT;
  if (nelem == 0) return FUS_OK;
  if (!u || !dof || !wgt || !offsets) return FUS_ERR_INVALID_ARGUMENT;
  if (rec && (slot < 0 || slot >= capacity)) return FUS_ERR_INVALID_ARGUMENT;
  if ((hre || him || H > 0) && (!hre || !him || !coef || H < 1)) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(u, sizeof(T)) || misaligned(wgt, sizeof(T)) || misaligned(rec, sizeof(T)) || misaligned(dof, sizeof(int32_t)) ||
      misaligned(offsets, sizeof(int64_t)) || misaligned(hre, sizeof(double)) || misaligned(him, sizeof(double)) ||
      misaligned(coef, sizeof(double)))
    return FUS_ERR_INVALID_ARGUMENT;
  T* row = rec ? rec + (int64_t)slot * nelem : nullptr;
  return hip_rc(fus::launch_element_receive<T>(u, dof, wgt, offsets, nelem, row, hre, him, coef, H, static_cast<hipStream_t>(stream)));
}

// full-field monitors (csrc/field_monitor.hpp): every check before any device work; n == 0 or no output requested is a no-op
template <typename T>
int field_accumulate(const T* u, const T* v, int64_t n, T* pmax, T* pmin, double* usq, double* vsq, double* hre, double* him,
                     int64_t hstride, const double* coef, int H, int init, void* stream) {
  if (n < 0 || H < 0 || H > 4) return FUS_ERR_INVALID_ARGUMENT;
  if (H > 0 && (!hre || !him || !coef || hstride < n)) return FUS_ERR_INVALID_ARGUMENT;
  if ((vsq && !v) || (!pmax != !pmin)) return FUS_ERR_INVALID_ARGUMENT;
  if (n == 0 || (!pmax && !usq && !vsq && H == 0)) return FUS_OK;
  if (!u) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(u, sizeof(T)) || misaligned(v, sizeof(T)) || misaligned(pmax, sizeof(T)) || misaligned(pmin, sizeof(T)) ||
      misaligned(usq, sizeof(double)) || misaligned(vsq, sizeof(double)) || misaligned(hre, sizeof(double)) ||
      misaligned(him, sizeof(double)) || misaligned(coef, sizeof(double)))
    return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_field_accumulate<T>(u, v, n, pmax, pmin, usq, vsq, hre, him, hstride, coef, H, init != 0,
                                                static_cast<hipStream_t>(stream)));
}

// phased-array source facets (csrc/source_array.hpp): every check before any device work; nA + nB == 0 is a no-op.
// ``stage``: the fp64 block {t, w0, A, f0, alpha, D} in host memory (copied into the launch) or, with ``dev``, in device memory.
template <typename T>
int facet_source_array(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA, const int32_t* eid, int64_t nA,
                       const double* amp, const double* phase, const double* delay, int64_t E, const T* xB, const T* cB, const T* detJB,
                       const int32_t* dmB, int64_t nB, int N, const double* stage, bool dev, void* stream) {
  if (nA < 0 || nB < 0 || E < 0 || N < 1) return FUS_ERR_INVALID_ARGUMENT;
  if (nA == 0 && nB == 0) return FUS_OK;
  if (!y || !stage) return FUS_ERR_INVALID_ARGUMENT;
  if (nA > 0 && (E < 1 || !cA1 || !detJA || !dmA || !eid || !amp || !phase || !delay)) return FUS_ERR_INVALID_ARGUMENT;
  if (nB > 0 && (!xB || !cB || !detJB || !dmB)) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(y, sizeof(T)) || misaligned(stage, sizeof(double)) || misaligned(amp, sizeof(double)) ||
      misaligned(phase, sizeof(double)) || misaligned(delay, sizeof(double)) || misaligned(eid, sizeof(int32_t)))
    return FUS_ERR_INVALID_ARGUMENT;
  fus::SourceStage st{0.0, 0.0, 0.0, 1.0, 1.0, 0.0};
  if (!dev) {
    st = fus::SourceStage{stage[0], stage[1], stage[2], stage[3], stage[4], stage[5]};
    // a NaN fails every comparison: f0 and alpha must be positive, D zero (continuous wave) or positive
    if (!(st.f0 > 0.0) || !(st.alpha > 0.0) || !(st.D >= 0.0)) return FUS_ERR_INVALID_ARGUMENT;
  }
  return hip_rc(fus::launch_facet_source_array<T>(y, cA1, cA2, detJA, dmA, eid, nA, amp, phase, delay, xB, cB, detJB, dmB, nB, N, st,
                                                  dev ? stage : nullptr, static_cast<hipStream_t>(stream)));
}

// sampled waveforms (csrc/source_wave.hpp): the table of a launch, checked before any device work
inline bool wave_table_ok(const double* table, int64_t R, int64_t Nt, double t0, double dt) {
  // a NaN fails every comparison: dt must be positive and finite, t0 finite
  return table && R >= 1 && Nt >= 2 && dt > 0.0 && dt <= 1.7976931348623157e308 && t0 >= -1.7976931348623157e308 &&
         t0 <= 1.7976931348623157e308 && !misaligned(table, 16);
}

// point sources with a sampled waveform (csrc/source_wave.hpp): point_source with the value read from the table
template <typename T>
int point_source_wave(T* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights, int P,
                      const double* amp, const double* delay, const int32_t* row_of, const double* table, int64_t R, int64_t Nt,
                      double t0, double dt, const double* stage, void* stream) {
  if (npts < 0 || ncells < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  if (npts == 0) return FUS_OK;
  if (!y || !cells || !dofmap || !weights || !amp || !delay || !row_of || !stage) return FUS_ERR_INVALID_ARGUMENT;
  if (!wave_table_ok(table, R, Nt, t0, dt)) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(y, sizeof(T)) || misaligned(weights, sizeof(T)) || misaligned(cells, sizeof(int32_t)) ||
      misaligned(dofmap, sizeof(int32_t)) || misaligned(row_of, sizeof(int32_t)) || misaligned(stage, sizeof(double)) ||
      misaligned(amp, sizeof(double)) || misaligned(delay, sizeof(double)))
    return FUS_ERR_INVALID_ARGUMENT;
  const fus::SourceStage st{stage[0], stage[1], stage[2], stage[3], stage[4], stage[5]};
  const fus::WaveTable wt{table, R, Nt, t0, dt};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipErrorInvalidValue;
  degree_dispatch(P, [&](auto p) {
    e = fus::launch_point_source_wave<T, decltype(p)::value>(y, cells, dofmap, weights, npts, ncells, amp, delay, row_of, wt, st, s);
  });
  return hip_rc(e);
}

// source facets with a sampled waveform (csrc/source_wave.hpp): facet_source_array with the element value read from the table
template <typename T>
int facet_source_wave(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA, const int32_t* eid, int64_t nA,
                      const double* amp, const double* delay, const int32_t* row_of, int64_t E, const double* table, int64_t R,
                      int64_t Nt, double t0, double dt, const T* xB, const T* cB, const T* detJB, const int32_t* dmB, int64_t nB, int N,
                      const double* stage, bool dev, void* stream) {
  if (nA < 0 || nB < 0 || E < 0 || N < 1) return FUS_ERR_INVALID_ARGUMENT;
  if (nA == 0 && nB == 0) return FUS_OK;
  if (!y || !stage) return FUS_ERR_INVALID_ARGUMENT;
  if (nA > 0 && (E < 1 || !cA1 || !detJA || !dmA || !eid || !amp || !delay || !row_of || !wave_table_ok(table, R, Nt, t0, dt)))
    return FUS_ERR_INVALID_ARGUMENT;
  if (nB > 0 && (!xB || !cB || !detJB || !dmB)) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(y, sizeof(T)) || misaligned(stage, sizeof(double)) || misaligned(amp, sizeof(double)) ||
      misaligned(delay, sizeof(double)) || misaligned(eid, sizeof(int32_t)) || misaligned(row_of, sizeof(int32_t)))
    return FUS_ERR_INVALID_ARGUMENT;
  fus::SourceStage st{0.0, 0.0, 0.0, 1.0, 1.0, 0.0};
  if (!dev) st = fus::SourceStage{stage[0], stage[1], stage[2], stage[3], stage[4], stage[5]};
  // without set A the table is not read: R = 0 makes every row a silent one
  const fus::WaveTable wt{table, nA > 0 ? R : 0, Nt, t0, dt};
  return hip_rc(fus::launch_facet_source_wave<T>(y, cA1, cA2, detJA, dmA, eid, nA, amp, delay, row_of, wt, xB, cB, detJB, dmB, nB, N, st,
                                                 dev ? stage : nullptr, static_cast<hipStream_t>(stream)));
}

// boundary facet terms (csrc/mass.hpp); the two scalars by value or, with ``dev``, from device memory
template <typename T>
int facet_terms(T* y, const T* cA1, T sA1, const T* cA2, T sA2, const T* scalars, bool dev, const T* detJA, const int32_t* dmA, int64_t nentA,
                const T* xB, const T* cB, const T* detJB, const int32_t* dmB, int64_t nentB, int N, void* stream) {
  if (nentA < 0 || nentB < 0 || N < 1 || !y || (dev && !scalars)) return FUS_ERR_INVALID_ARGUMENT;
  if (nentA > 0 && (!cA1 || !detJA || !dmA)) return FUS_ERR_INVALID_ARGUMENT;
  if (nentB > 0 && (!xB || !cB || !detJB || !dmB)) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_facet_terms<T>(y, cA1, sA1, cA2, sA2, detJA, dmA, nentA, xB, cB, detJB, dmB, nentB, N,
                                           static_cast<hipStream_t>(stream), dev ? scalars : nullptr));
}

// sponge-layer damping terms of a stage (csrc/sponge.hpp): every check before any device work; n == 0 is a no-op
template <typename T>
int sponge_terms(T* y, const T* u, const T* v, const int32_t* idx, const T* cu, const T* cv, int64_t n, void* stream) {
  if (n < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (n == 0) return FUS_OK;
  if (!y || !u || !v || !idx || !cu || !cv) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(y, sizeof(T)) || misaligned(u, sizeof(T)) || misaligned(v, sizeof(T)) || misaligned(idx, sizeof(int32_t)) ||
      misaligned(cu, sizeof(T)) || misaligned(cv, sizeof(T)))
    return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_sponge_terms<T>(y, u, v, idx, cu, cv, n, static_cast<hipStream_t>(stream)));
}

template <typename T>
int geometry_factors(const T* x_g, const int32_t* x_dofs, const T* dphi, const T* weights, int nq, int64_t ncell, T* G, T* detJ, void* stream) {
  if (ncell < 0 || nq < 1) return FUS_ERR_INVALID_ARGUMENT;
  if (ncell == 0) return FUS_OK;
  if (!x_g || !x_dofs || !dphi || !weights || (!G && !detJ)) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_geometry<T>(x_g, x_dofs, dphi, weights, nq, ncell, G, detJ, static_cast<hipStream_t>(stream)));
}

template <typename T>
int facet_jacobian(const T* x_g, const int32_t* x_dofs, const int32_t* boundary_data, const T* dphi_f, const T* weights, int nqf,
                   int64_t nfacets, T* detJ_f, void* stream) {
  if (nfacets < 0 || nqf < 1) return FUS_ERR_INVALID_ARGUMENT;
  if (nfacets == 0) return FUS_OK;
  if (!x_g || !x_dofs || !boundary_data || !dphi_f || !weights || !detJ_f) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_facet_geometry<T>(x_g, x_dofs, boundary_data, dphi_f, weights, nqf, nfacets, detJ_f,
                                              static_cast<hipStream_t>(stream)));
}

// RK4 stages (csrc/rk4.hpp, westervelt.hpp): ntotal == 0 is a no-op; the lean kinds 4..7 of ``new_step`` exist for stage and stage_nl2 only
template <typename T>
int rk4_stage(T bw, T aw, int new_step, const T* minv, T* b, T* u, T* v, T* u0, T* v0, T* ku, T* un, int64_t nlocal, int64_t ntotal,
              void* stream) {
  if (nlocal < 0 || ntotal < nlocal) return FUS_ERR_INVALID_ARGUMENT;
  if (ntotal == 0) return FUS_OK;
  if (!minv || !b || !u || !v || !u0 || !v0 || !ku || !un) return FUS_ERR_INVALID_ARGUMENT;
  if (new_step < 0 || new_step > 7) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_rk4_stage<T>(bw, aw, new_step, minv, b, u, v, u0, v0, ku, un, nlocal, ntotal, static_cast<hipStream_t>(stream)));
}

template <typename T>
int rk4_stage_nl(T bw, T aw, int new_step, const T* m0, T* m, T* b, T* u, T* v, T* u0, T* v0, T* ku, T* un, int64_t nlocal, int64_t ntotal,
                 void* stream) {
  if (nlocal < 0 || ntotal < nlocal) return FUS_ERR_INVALID_ARGUMENT;
  if (ntotal == 0) return FUS_OK;
  if (!m0 || !m || !b || !u || !v || !u0 || !v0 || !ku || !un) return FUS_ERR_INVALID_ARGUMENT;
  if (new_step < 0 || new_step > 3) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_rk4_stage_nl<T>(bw, aw, new_step, m0, m, b, u, v, u0, v0, ku, un, nlocal, ntotal,
                                            static_cast<hipStream_t>(stream)));
}

template <typename T>
int rk4_stage_nl2(T bw, T aw, int new_step, const T* m0, const T* w2, const T* w5, T* b, T* u, T* v, T* u0, T* v0, T* ku, T* un, T kappa,
                  T* w, int64_t nlocal, int64_t ntotal, void* stream) {
  if (nlocal < 0 || ntotal < nlocal) return FUS_ERR_INVALID_ARGUMENT;
  if (ntotal == 0) return FUS_OK;
  if (!m0 || !w2 || !w5 || !b || !u || !v || !u0 || !v0 || !ku || !un) return FUS_ERR_INVALID_ARGUMENT;
  if (new_step < 0 || new_step > 7) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_rk4_stage_nl2<T>(bw, aw, new_step, m0, w2, w5, b, u, v, u0, v0, ku, un, kappa, w, nlocal, ntotal,
                                             static_cast<hipStream_t>(stream)));
}

// Pennes bioheat stage (csrc/bioheat.hpp): every check before any device work; ntotal == 0 is a no-op
template <typename T>
int bioheat_stage(T bw, T aw, int kind, T gate, T t_a, double dt, const T* minv, const T* pr, const T* s, T* b, T* T0, T* Tn, T* acc,
                  double* cem43, T* tmax, int init, int64_t nlocal, int64_t ntotal, void* stream) {
  if (nlocal < 0 || ntotal < nlocal) return FUS_ERR_INVALID_ARGUMENT;
  if (kind < 0 || kind > 2) return FUS_ERR_INVALID_ARGUMENT;
  if (ntotal == 0) return FUS_OK;
  if (!minv || !b || !T0 || !Tn || !acc) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(minv, sizeof(T)) || misaligned(pr, sizeof(T)) || misaligned(s, sizeof(T)) || misaligned(b, sizeof(T)) ||
      misaligned(T0, sizeof(T)) || misaligned(Tn, sizeof(T)) || misaligned(acc, sizeof(T)) || misaligned(cem43, sizeof(double)) ||
      misaligned(tmax, sizeof(T)))
    return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::launch_bioheat_stage<T>(bw, aw, kind, gate, t_a, dt, minv, pr, s, b, T0, Tn, acc, cem43, tmax, init != 0, nlocal, ntotal,
                                             static_cast<hipStream_t>(stream)));
}

// relaxation stage (csrc/relaxation.hpp): every check before any device work; nlocal == 0 is a no-op
template <typename T>
int relax_stage(T bw, T aw, T aw_u, int kind, int nr, const double* tau, const double* kappa_scalar, const T* kappa, T* xi0, T* xin, T* acc,
                int64_t stride, const T* u_base, const T* vn, T* ur, int64_t nlocal, void* stream) {
  if (nlocal < 0 || stride < nlocal) return FUS_ERR_INVALID_ARGUMENT;
  if (kind < 0 || kind > 2 || nr < 1 || nr > FUS_RELAX_MAX_MECHANISMS) return FUS_ERR_INVALID_ARGUMENT;
  if (nlocal == 0) return FUS_OK;
  if (!tau || (!kappa && !kappa_scalar) || !xi0 || !xin || !acc || !u_base || !vn || !ur) return FUS_ERR_INVALID_ARGUMENT;
  for (int nu = 0; nu < nr; ++nu)
    if (!(tau[nu] > 0.0)) return FUS_ERR_INVALID_ARGUMENT;
  if (misaligned(kappa, sizeof(T)) || misaligned(xi0, sizeof(T)) || misaligned(xin, sizeof(T)) || misaligned(acc, sizeof(T)) ||
      misaligned(u_base, sizeof(T)) || misaligned(vn, sizeof(T)) || misaligned(ur, sizeof(T)))
    return FUS_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipErrorInvalidValue;
  switch (nr) {
    case 1: e = fus::launch_relax_stage<T, 1>(bw, aw, aw_u, kind, tau, kappa_scalar, kappa, xi0, xin, acc, stride, u_base, vn, ur, nlocal, s); break;
    case 2: e = fus::launch_relax_stage<T, 2>(bw, aw, aw_u, kind, tau, kappa_scalar, kappa, xi0, xin, acc, stride, u_base, vn, ur, nlocal, s); break;
    case 3: e = fus::launch_relax_stage<T, 3>(bw, aw, aw_u, kind, tau, kappa_scalar, kappa, xi0, xin, acc, stride, u_base, vn, ur, nlocal, s); break;
    default: e = fus::launch_relax_stage<T, 4>(bw, aw, aw_u, kind, tau, kappa_scalar, kappa, xi0, xin, acc, stride, u_base, vn, ur, nlocal, s); break;
  }
  return hip_rc(e);
}

}  // namespace

bool fus_abi::plan_check(const void* ws, int N, int epb, int64_t nent, bool* ordered, bool* exclusive, bool* runs_pay) {
  PlanInfo p;
  if (!g_registry.get(ws, &p) || p.N != N || p.epb != epb || p.nent != nent) return false;
  *ordered = p.ordered;
  if (exclusive) *exclusive = p.exclusive;
  if (runs_pay) *runs_pay = p.runs_pay;
  return true;
}

int fus_abi::plan_rows_stride(const void* ws) {
  PlanInfo p;
  return (g_registry.get(ws, &p) && p.rows_consecutive) ? p.run_stride : 0;
}

int fus_abi::plan_sweep_flip(const void* ws) { return g_registry.flip_sweep(ws); }

extern "C" {

int fus_abi_version(void) { return FUS_ABI_VERSION; }

#ifndef FUS_SOURCE_HASH
#define FUS_SOURCE_HASH "unknown"
#endif
const char* fus_source_hash(void) { return FUS_SOURCE_HASH; }

const char* fus_error_string(int code) {
  switch (code) {
    case FUS_OK: return "ok";
    case FUS_ERR_INVALID_ARGUMENT: return "invalid argument (null pointer, negative size or misaligned buffer)";
    case FUS_ERR_UNSUPPORTED_DEGREE: return "unsupported polynomial degree";
    case FUS_ERR_UNSUPPORTED_ENTITY: return "unsupported entity size";
    case FUS_ERR_NO_DEVICE: return "no HIP device";
    case FUS_ERR_PLAN_MISMATCH:
      return "workspace holds no plan built through this library for this (degree / entity size, entity count)";
    case FUS_ERR_COMM: return "communicator / RCCL failure (see fus_comm_last_error)";
    default:
      if (code <= FUS_ERR_HIP_BASE) return hipGetErrorString((hipError_t)(FUS_ERR_HIP_BASE - code));
      return "unknown error";
  }
}

int fus_device_info(int device, char* name, int* compute_units, int64_t* hbm_bytes, int* lds_bytes_per_cu) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return FUS_ERR_NO_DEVICE;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) return FUS_ERR_NO_DEVICE;
  if (name) {
    std::snprintf(name, 256, "%s (%s)", p.name, p.gcnArchName);
  }
  if (compute_units) *compute_units = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)p.maxSharedMemoryPerMultiProcessor;
  return FUS_OK;
}

int fus_set_tuning(int key, int value) {
  switch (key) {
    case FUS_TUNE_STIFFNESS_VARIANT: g_stiffness_variant = value; return FUS_OK;
    case FUS_TUNE_XCD_REMAP: g_xcd_remap = value ? 1 : 0; return FUS_OK;
    case FUS_TUNE_MASS_VARIANT: g_mass_variant = value; return FUS_OK;
    case FUS_TUNE_PLAN_VARIANT: g_plan_variant = value; return FUS_OK;
    case FUS_TUNE_PLAN_RUNS: g_plan_runs = value; return FUS_OK;
    case FUS_TUNE_PLAN_ROWS: g_plan_rows = value ? 1 : 0; return FUS_OK;
    case FUS_TUNE_PLAN_XCD_GROUP:
      if (!plan_xcd_group_valid(value)) return FUS_ERR_INVALID_ARGUMENT;
      g_plan_xcd_group = value;
      return FUS_OK;
    case FUS_TUNE_PLAN_SWEEP:
      if (!plan_sweep_valid(value)) return FUS_ERR_INVALID_ARGUMENT;
      g_plan_sweep = value;
      return FUS_OK;
    case FUS_TUNE_VECTOR_STREAM:
      if (value < 0 || value > 4) return FUS_ERR_INVALID_ARGUMENT;
      fus::vector_stream_mode() = value;
      return FUS_OK;
  }
  return FUS_ERR_INVALID_ARGUMENT;
}

int fus_get_tuning(int key) {
  switch (key) {
    case FUS_TUNE_STIFFNESS_VARIANT: return g_stiffness_variant;
    case FUS_TUNE_XCD_REMAP: return g_xcd_remap;
    case FUS_TUNE_MASS_VARIANT: return g_mass_variant;
    case FUS_TUNE_PLAN_VARIANT: return g_plan_variant;
    case FUS_TUNE_PLAN_RUNS: return g_plan_runs;
    case FUS_TUNE_PLAN_ROWS: return g_plan_rows;
    case FUS_TUNE_PLAN_XCD_GROUP: return g_plan_xcd_group;
    case FUS_TUNE_PLAN_SWEEP: return g_plan_sweep;
    case FUS_TUNE_VECTOR_STREAM: return fus::vector_stream_mode();
  }
  return FUS_ERR_INVALID_ARGUMENT;
}

int64_t fus_stiffness_plan_bytes(int P, int64_t ncell) {
  if (ncell < 0) return FUS_ERR_INVALID_ARGUMENT;
  return plan_bytes(P, ncell);
}

int fus_stiffness_plan_build(const int32_t* dofmap, int P, int64_t ncell, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  return fus_plan_build_ordered(dofmap, nullptr, (P + 1) * (P + 1) * (P + 1), fus::cells_per_batch(P), ncell, workspace,
                                workspace_bytes, stream);
}

int fus_plan_entities_per_batch(int N) {
  if (N < 1 || N > fus::kPlanMaxEntries) return FUS_ERR_UNSUPPORTED_ENTITY;
  // cells (N = n^3): the stiffness kernel's batch size, so one plan serves both operators
  for (int P = FUS_MIN_DEGREE; P <= FUS_MAX_DEGREE; ++P)
    if ((P + 1) * (P + 1) * (P + 1) == N) return fus::cells_per_batch(P);
  const int epb = 1280 / N;  // ~5 entries per thread of a 256-thread workgroup
  return epb > 0 ? epb : 1;
}

int64_t fus_plan_bytes(int N, int entities_per_batch, int64_t nent) {
  if (N < 1 || entities_per_batch < 1 || nent < 0 || (int64_t)N * entities_per_batch > fus::kPlanMaxEntries)
    return FUS_ERR_INVALID_ARGUMENT;
  return fus::plan_view_generic(nullptr, N, entities_per_batch, nent).bytes;
}

int fus_plan_build(const int32_t* dofmap, int N, int entities_per_batch, int64_t nent, void* workspace,
                   int64_t workspace_bytes, void* stream) {
  return fus_plan_build_ordered(dofmap, nullptr, N, entities_per_batch, nent, workspace, workspace_bytes, stream);
}

int fus_plan_release(const void* workspace) {
  g_registry.release(workspace);
  return FUS_OK;
}

int64_t fus_mass_gather_plan_bytes(int N, int64_t nent, int64_t ndofs) {
  if (N < 1 || N > 2048 || nent < 0 || ndofs < 0 || nent * (int64_t)N > (int64_t)INT32_MAX) return FUS_ERR_INVALID_ARGUMENT;
  fus::GatherHeader h{};
  fus::gather_layout(nent, N, ndofs, &h);
  return h.bytes;
}

int fus_mass_gather_plan_build(const int32_t* dofmap, int N, int64_t nent, int64_t ndofs, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  const int64_t need = fus_mass_gather_plan_bytes(N, nent, ndofs);
  if (need < 0) return (int)need;
  if (!workspace || misaligned(workspace, 256) || workspace_bytes < need) return FUS_ERR_INVALID_ARGUMENT;
  return gather_plan_build(dofmap, N, nent, ndofs, nullptr, 0, workspace, stream);
}

int fus_mass_gather_plan_build_rows(const int32_t* dofmap, int N, int64_t nent, int64_t ndofs, const uint8_t* row_set, int which,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  const int64_t need = fus_mass_gather_plan_bytes(N, nent, ndofs);
  if (need < 0) return (int)need;
  if (!workspace || misaligned(workspace, 256) || workspace_bytes < need || !row_set || which < 0 || which > 255)
    return FUS_ERR_INVALID_ARGUMENT;
  if (ndofs >= 0x7fffffffLL) return FUS_ERR_INVALID_ARGUMENT;  // the sentinel key of the dropped rows is ndofs itself
  return gather_plan_build(dofmap, N, nent, ndofs, row_set, which, workspace, stream);
}

int fus_mass_gather_plan_info(const void* workspace, int64_t* out4) {
  if (!workspace || !out4) return FUS_ERR_INVALID_ARGUMENT;
  fus::GatherHeader h{};
  if (!g_registry.get(workspace, &h)) return FUS_ERR_PLAN_MISMATCH;
  out4[0] = h.nrows;
  out4[1] = h.dense;
  out4[2] = h.max_len;
  out4[3] = h.bytes;
  return FUS_OK;
}

int64_t fus_mass_gather_static_bytes(int N, int64_t nent, int elem_bytes) {
  if (N < 1 || nent < 0 || (elem_bytes != 4 && elem_bytes != 8)) return FUS_ERR_INVALID_ARGUMENT;
  if (nent * (int64_t)N >= (int64_t)1 << 31) return FUS_ERR_INVALID_ARGUMENT;
  return fus::gather_static_bytes(nent, N, nent * (int64_t)N, elem_bytes);
}

int fus_plan_build_ordered(const int32_t* dofmap, const int32_t* entity_order, int N, int entities_per_batch,
                           int64_t nent, void* workspace, int64_t workspace_bytes, void* stream) {
  const int64_t need = fus_plan_bytes(N, entities_per_batch, nent);
  if (need < 0) return (int)need;
  if (!workspace || misaligned(workspace, 256) || workspace_bytes < need) return FUS_ERR_INVALID_ARGUMENT;
  if (nent > 0 && !dofmap) return FUS_ERR_INVALID_ARGUMENT;
  if (nent > 0) {
    const hipError_t e = fus::launch_plan_build_generic(dofmap, N, entities_per_batch, nent, workspace,
                                                        static_cast<hipStream_t>(stream), plan_allow_runs(N), entity_order);
    if (e != hipSuccess) return hip_rc(e);
  }
  int64_t nbatch = 0, with_runs = 0;
  bool rows = false;
  int run_stride = 0;
  if (nent > 0) {
    const hipError_t e = fus::plan_run_batches(workspace, static_cast<hipStream_t>(stream), &with_runs, &rows, &run_stride);
    if (e != hipSuccess) return hip_rc(e);
    nbatch = (nent + entities_per_batch - 1) / entities_per_batch;
  }
  g_registry.put(workspace, PlanInfo{N, entities_per_batch, nent, entity_order != nullptr, false, 2 * with_runs >= nbatch, nbatch, with_runs,
                                     rows, fus::plan_row_len(N) > 0 ? run_stride : 0});
  return FUS_OK;
}

int fus_plan_encoding(const void* workspace, int64_t* batches, int64_t* batches_with_runs, int* reads_runs_f64, int* reads_runs_f32) {
  PlanInfo p;
  if (!g_registry.get(workspace, &p)) return FUS_ERR_PLAN_MISMATCH;
  if (batches) *batches = p.nbatch;
  if (batches_with_runs) *batches_with_runs = p.with_runs;
  if (reads_runs_f64) *reads_runs_f64 = plan_use_runs<double>(p.N, p.runs_pay) ? 1 : 0;
  if (reads_runs_f32) *reads_runs_f32 = plan_use_runs<float>(p.N, p.runs_pay) ? 1 : 0;
  return FUS_OK;
}

int fus_plan_mark_exclusive(void* workspace, int N, int entities_per_batch, int64_t nent, int32_t* dof_use_count,
                            int64_t ndofs, void* stream) {
  if (!workspace || !dof_use_count || ndofs < 0) return FUS_ERR_INVALID_ARGUMENT;
  bool ord = false;
  if (!plan_check(workspace, N, entities_per_batch, nent, &ord)) return FUS_ERR_PLAN_MISMATCH;
  const hipError_t e = fus::launch_plan_mark_exclusive(workspace, N, entities_per_batch, nent, dof_use_count, ndofs,
                                                       static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_rc(e);
  g_registry.mark_exclusive(workspace);
  return FUS_OK;
}

// The typed entry points: a prototype and a forward each.
#define FUS_TYPED(T, SUF)                                                                                                                  \
  int fus_stiffness_apply_##SUF(const T* x, const T* cc, T* y, const T* G, const int32_t* dofmap, const T* dphi, int P, int64_t ncell,     \
                                void* s) {                                                                                                 \
    return stiffness_apply<T>(x, cc, y, G, dofmap, dphi, P, ncell, s);                                                                     \
  }                                                                                                                                        \
  int fus_stiffness_apply_planned_##SUF(const T* x, const T* cc, T* y, const T* G, const void* ws, const T* dphi, int P, int64_t ncell,    \
                                        void* s) {                                                                                         \
    return stiffness_apply_planned<T>(x, cc, y, G, ws, dphi, P, ncell, s);                                                                 \
  }                                                                                                                                        \
  int fus_stiffness_apply_planned_affine_##SUF(const T* x, const T* cc, T* y, const T* G, const T* wratio, const void* ws, const T* dphi,  \
                                               int P, int64_t ncell, void* s) {                                                            \
    return stiffness_apply_planned_affine<T>(x, cc, y, G, wratio, ws, dphi, P, ncell, s);                                                  \
  }                                                                                                                                        \
  int fus_stiffness_apply_planned_geom_##SUF(const T* x, const T* cc, T* y, const T* x_g, const int32_t* x_dofs, const T* pts,             \
                                             const T* wts, const void* ws, const T* dphi, int P, int64_t ncell, void* s) {                 \
    return stiffness_apply_planned_geom<T>(x, cc, y, x_g, x_dofs, pts, wts, ws, dphi, P, ncell, s);                                        \
  }                                                                                                                                        \
  int fus_stiffness_apply_planned_geom_nodal_##SUF(const T* x, const T* cc, const T* nodal, T* y, const T* x_g, const int32_t* x_dofs,    \
                                                   const T* pts, const T* wts, const void* ws, const T* dphi, int P, int64_t ncell,        \
                                                   void* s) {                                                                              \
    return stiffness_apply_planned_geom_nodal<T>(x, cc, nodal, y, x_g, x_dofs, pts, wts, ws, dphi, P, ncell, s);                           \
  }                                                                                                                                        \
  int fus_gradient_apply_planned_geom_##SUF(const T* x, const T* cc, T* y, int64_t ystride, const T* x_g, const int32_t* x_dofs,           \
                                            const T* pts, const T* wts, const void* ws, const T* dphi, int P, int64_t ncell, void* s) {    \
    return gradient_apply_planned_geom<T>(x, cc, y, ystride, x_g, x_dofs, pts, wts, ws, dphi, P, ncell, s);                                \
  }                                                                                                                                        \
  int fus_westervelt_cell_apply_planned_##SUF(const T* u, const T* v, const T* c2, const T* c3, const T* c4, const T* c5, T* b, T* m,      \
                                              const T* G, const T* detJ, const void* ws, const T* dphi, int P, int64_t ncell, void* s) {   \
    return westervelt_cell<T>(u, v, c2, c3, c4, c5, b, m, G, detJ, ws, dphi, P, ncell, s);                                                 \
  }                                                                                                                                        \
  int fus_westervelt_cell_apply_planned_geom_##SUF(const T* u, const T* v, const T* c2, const T* c3, const T* c4, const T* c5, T* b, T* m, \
                                                   const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts, const void* ws,        \
                                                   const T* dphi, int P, int64_t ncell, void* s) {                                         \
    return westervelt_cell_geom<T>(u, v, c2, c3, c4, c5, b, m, x_g, x_dofs, pts, wts, ws, dphi, P, ncell, s);                              \
  }                                                                                                                                        \
  int fus_westervelt_stiffness_apply_planned_geom_nodal_##SUF(const T* u, const T* v, const T* c3, const T* c4, const T* nodal3,           \
                                                              const T* nodal4, T* b, const T* x_g, const int32_t* x_dofs, const T* pts,    \
                                                              const T* wts, const void* ws, const T* dphi, int P, int64_t ncell,           \
                                                              void* s) {                                                                   \
    return westervelt_stiffness_apply_planned_geom_nodal<T>(u, v, c3, c4, nodal3, nodal4, b, x_g, x_dofs, pts, wts, ws, dphi, P, ncell,    \
                                                            s);                                                                            \
  }                                                                                                                                        \
  int fus_mass_apply_##SUF(const T* x, const T* c, T* y, const T* detJ, const int32_t* dofmap, int N, int64_t nent, void* s) {             \
    return mass_apply<T>(x, c, y, detJ, dofmap, N, nent, s);                                                                               \
  }                                                                                                                                        \
  int fus_mass_apply_planned_##SUF(const T* x, const T* c, T* y, const T* detJ, const void* ws, int N, int epb, int64_t nent, void* s) {   \
    return mass_apply_planned<T>(x, c, y, detJ, ws, N, epb, nent, s);                                                                      \
  }                                                                                                                                        \
  int fus_mass_apply_gather_##SUF(const T* x, const T* c, T* y, const T* detJ, const void* ws, int N, int64_t nent, void* s) {             \
    return mass_apply_gather<T>(x, c, y, detJ, ws, N, nent, s);                                                                            \
  }                                                                                                                                        \
  int fus_mass_gather_static_build_##SUF(const void* ws, const T* detJ, void* sws, int64_t sws_bytes, void* s) {                           \
    return mass_gather_static_build<T>(ws, detJ, sws, sws_bytes, s);                                                                       \
  }                                                                                                                                        \
  int fus_mass_apply_gather_static_##SUF(const T* x, const T* c, T* y, const void* ws, const void* sws, int N, int64_t nent, void* s) {    \
    return mass_apply_gather_static<T>(x, c, y, ws, sws, N, nent, s);                                                                      \
  }                                                                                                                                        \
  int fus_facet_terms_##SUF(T* y, const T* cA1, T sA1, const T* cA2, T sA2, const T* detJA, const int32_t* dmA, int64_t nentA,             \
                            const T* xB, const T* cB, const T* detJB, const int32_t* dmB, int64_t nentB, int N, void* s) {                 \
    return facet_terms<T>(y, cA1, sA1, cA2, sA2, nullptr, false, detJA, dmA, nentA, xB, cB, detJB, dmB, nentB, N, s);                      \
  }                                                                                                                                        \
  int fus_facet_terms_dev_##SUF(T* y, const T* cA1, const T* cA2, const T* scalars, const T* detJA, const int32_t* dmA, int64_t nentA,     \
                                const T* xB, const T* cB, const T* detJB, const int32_t* dmB, int64_t nentB, int N, void* s) {             \
    return facet_terms<T>(y, cA1, T(0), cA2, T(0), scalars, true, detJA, dmA, nentA, xB, cB, detJB, dmB, nentB, N, s);                     \
  }                                                                                                                                        \
  int fus_facet_source_array_##SUF(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA, const int32_t* element_of_facet,  \
                                   int64_t nentA, const double* amplitude, const double* phase, const double* delay, int64_t nelem,        \
                                   const T* xB, const T* cB, const T* detJB, const int32_t* dmB, int64_t nentB, int N,                     \
                                   const double* stage, void* s) {                                                                         \
    return facet_source_array<T>(y, cA1, cA2, detJA, dmA, element_of_facet, nentA, amplitude, phase, delay, nelem, xB, cB, detJB, dmB,     \
                             nentB, N, stage, false, s);                                                                                   \
  }                                                                                                                                        \
  int fus_facet_source_array_dev_##SUF(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA,                               \
                                       const int32_t* element_of_facet, int64_t nentA, const double* amplitude, const double* phase,       \
                                       const double* delay, int64_t nelem, const T* xB, const T* cB, const T* detJB, const int32_t* dmB,   \
                                       int64_t nentB, int N, const double* stage_dev, void* s) {                                           \
    return facet_source_array<T>(y, cA1, cA2, detJA, dmA, element_of_facet, nentA, amplitude, phase, delay, nelem, xB, cB, detJB, dmB,     \
                             nentB, N, stage_dev, true, s);                                                                                \
  }                                                                                                                                        \
  int fus_geometry_factors_##SUF(const T* x_g, const int32_t* x_dofs, const T* dphi, const T* weights, int nq, int64_t ncell, T* G,        \
                                 T* detJ, void* s) {                                                                                       \
    return geometry_factors<T>(x_g, x_dofs, dphi, weights, nq, ncell, G, detJ, s);                                                         \
  }                                                                                                                                        \
  int fus_facet_jacobian_##SUF(const T* x_g, const int32_t* x_dofs, const int32_t* boundary_data, const T* dphi_f, const T* weights,       \
                               int nqf, int64_t nfacets, T* detJ_f, void* s) {                                                             \
    return facet_jacobian<T>(x_g, x_dofs, boundary_data, dphi_f, weights, nqf, nfacets, detJ_f, s);                                        \
  }                                                                                                                                        \
  int fus_axpy_##SUF(T alpha, const T* x, T* y, int64_t n, void* s) {                                                                      \
    return ew<T, fus::OpAxpy<T>, true, true>(x, y, y, n, fus::OpAxpy<T>{alpha}, s);                                                        \
  }                                                                                                                                        \
  int fus_scale_##SUF(T alpha, const T* a, T* b, int64_t n, void* s) {                                                                     \
    return ew<T, fus::OpScale<T>, true, false>(a, nullptr, b, n, fus::OpScale<T>{alpha}, s);                                               \
  }                                                                                                                                        \
  int fus_copy_##SUF(const T* a, T* b, int64_t n, void* s) {                                                                               \
    return ew<T, fus::OpCopy<T>, true, false>(a, nullptr, b, n, fus::OpCopy<T>{}, s);                                                      \
  }                                                                                                                                        \
  int fus_fill_##SUF(T alpha, T* x, int64_t n, void* s) {                                                                                  \
    return ew<T, fus::OpFill<T>, false, false>(nullptr, nullptr, x, n, fus::OpFill<T>{alpha}, s);                                          \
  }                                                                                                                                        \
  int fus_pointwise_divide_##SUF(const T* a, const T* b, T* c, int64_t n, void* s) {                                                       \
    return ew<T, fus::OpDiv<T>, true, true>(a, b, c, n, fus::OpDiv<T>{}, s);                                                               \
  }                                                                                                                                        \
  int fus_square_##SUF(const T* a, T* b, int64_t n, void* s) {                                                                             \
    return ew<T, fus::OpSquare<T>, true, false>(a, nullptr, b, n, fus::OpSquare<T>{}, s);                                                  \
  }                                                                                                                                        \
  int fus_muladd_##SUF(const T* w, const T* x, T* y, int64_t n, void* s) {                                                                 \
    return muladd<T>(w, x, y, n, s);                                                                                                       \
  }                                                                                                                                        \
  int fus_pack_fwd_##SUF(const T* in, T* out, const int64_t* idx, int64_t cnt, void* s) {                                                  \
    return halo<T, fus::PACK>(in, out, idx, cnt, 0, s);                                                                                    \
  }                                                                                                                                        \
  int fus_unpack_fwd_##SUF(const T* in, T* out, const int64_t* idx, int64_t cnt, int64_t N, void* s) {                                     \
    return halo<T, fus::UNPACK_SET>(in, out, idx, cnt, N, s);                                                                              \
  }                                                                                                                                        \
  int fus_pack_rev_##SUF(const T* in, T* out, const int64_t* idx, int64_t cnt, int64_t N, void* s) {                                       \
    return halo<T, fus::PACK>(in, out, idx, cnt, N, s);                                                                                    \
  }                                                                                                                                        \
  int fus_unpack_rev_##SUF(const T* in, T* out, const int64_t* idx, int64_t cnt, void* s) {                                                \
    return halo<T, fus::UNPACK_ADD>(in, out, idx, cnt, 0, s);                                                                              \
  }                                                                                                                                        \
  int fus_rk4_stage_##SUF(T bw, T aw, int new_step, const T* minv, T* b, T* u, T* v, T* u0, T* v0, T* ku, T* un, int64_t nlocal,           \
                          int64_t ntotal, void* s) {                                                                                       \
    return rk4_stage<T>(bw, aw, new_step, minv, b, u, v, u0, v0, ku, un, nlocal, ntotal, s);                                               \
  }                                                                                                                                        \
  int fus_rk4_stage_nl_##SUF(T bw, T aw, int new_step, const T* m0, T* m, T* b, T* u, T* v, T* u0, T* v0, T* ku, T* un, int64_t nlocal,    \
                             int64_t ntotal, void* s) {                                                                                    \
    return rk4_stage_nl<T>(bw, aw, new_step, m0, m, b, u, v, u0, v0, ku, un, nlocal, ntotal, s);                                           \
  }                                                                                                                                        \
  int fus_rk4_stage_nl2_##SUF(T bw, T aw, int new_step, const T* m0, const T* w2, const T* w5, T* b, T* u, T* v, T* u0, T* v0, T* ku,      \
                              T* un, T kappa, T* w, int64_t nlocal, int64_t ntotal, void* s) {                                             \
    return rk4_stage_nl2<T>(bw, aw, new_step, m0, w2, w5, b, u, v, u0, v0, ku, un, kappa, w, nlocal, ntotal, s);                           \
  }                                                                                                                                        \
  int fus_sponge_terms_##SUF(T* y, const T* u, const T* v, const int32_t* idx, const T* cu, const T* cv, int64_t n, void* s) {            \
    return sponge_terms<T>(y, u, v, idx, cu, cv, n, s);                                                                                    \
  }                                                                                                                                        \
  int fus_bioheat_stage_##SUF(T bw, T aw, int kind, T gate, T t_a, double dt, const T* minv, const T* pr, const T* src, T* b, T* T0,       \
                              T* Tn, T* acc, double* cem43, T* tmax, int init, int64_t nlocal, int64_t ntotal, void* s) {                  \
    return bioheat_stage<T>(bw, aw, kind, gate, t_a, dt, minv, pr, src, b, T0, Tn, acc, cem43, tmax, init, nlocal, ntotal, s);             \
  }                                                                                                                                        \
  int fus_relax_stage_##SUF(T bw, T aw, T aw_u, int kind, int nr, const double* tau, const double* kappa_scalar, const T* kappa, T* xi0,    \
                            T* xin, T* acc, int64_t stride, const T* u_base, const T* vn, T* ur, int64_t nlocal, void* s) {                \
    return relax_stage<T>(bw, aw, aw_u, kind, nr, tau, kappa_scalar, kappa, xi0, xin, acc, stride, u_base, vn, ur, nlocal, s);             \
  }                                                                                                                                        \
  int fus_probe_eval_##SUF(const T* u, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights, int P, \
                           T* rec, int64_t capacity, int slot, double* pmax, double* pmin, double* hre, double* him, const double* coef,   \
                           int H, void* s) {                                                                                               \
    return probe_eval<T>(u, cells, npts, dofmap, ncells, weights, P, rec, capacity, slot, pmax, pmin, hre, him, coef, H, s);               \
  }                                                                                                                                        \
  int fus_point_source_##SUF(T* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights, int P,     \
                             const double* amplitude, const double* phase, const double* delay, const double* stage, void* s) {            \
    return point_source<T>(y, cells, npts, dofmap, ncells, weights, P, amplitude, phase, delay, stage, s);                                 \
  }                                                                                                                                        \
  int fus_element_receive_##SUF(const T* u, const int32_t* dof, const T* wgt, const int64_t* offsets, int64_t nelem, T* rec,               \
                                int64_t capacity, int slot, double* hre, double* him, const double* coef, int H, void* s) {                \
    return element_receive<T>(u, dof, wgt, offsets, nelem, rec, capacity, slot, hre, him, coef, H, s);                                     \
  }                                                                                                                                        \
  int fus_field_accumulate_##SUF(const T* u, const T* v, int64_t n, T* pmax, T* pmin, double* usq, double* vsq, double* hre, double* him,  \
                                 int64_t hstride, const double* coef, int H, int init, void* s) {                                          \
    return field_accumulate<T>(u, v, n, pmax, pmin, usq, vsq, hre, him, hstride, coef, H, init, s);                                        \
  }
FUS_TYPED(double, f64)
FUS_TYPED(float, f32)
#undef FUS_TYPED

// include/fus_gpu_waveform.h
#define FUS_WAVE(T, SUF)                                                                                                                   \
  int fus_facet_source_wave_##SUF(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA, const int32_t* element_of_facet,   \
                                  int64_t nentA, const double* amplitude, const double* delay, const int32_t* row_of_element,              \
                                  int64_t nelem, const double* table, int64_t nrows, int64_t nt, double t0, double dt, const T* xB,        \
                                  const T* cB, const T* detJB, const int32_t* dmB, int64_t nentB, int N, const double* stage, void* s) {   \
    return facet_source_wave<T>(y, cA1, cA2, detJA, dmA, element_of_facet, nentA, amplitude, delay, row_of_element, nelem, table, nrows,   \
                                nt, t0, dt, xB, cB, detJB, dmB, nentB, N, stage, false, s);                                                \
  }                                                                                                                                        \
  int fus_facet_source_wave_dev_##SUF(T* y, const T* cA1, const T* cA2, const T* detJA, const int32_t* dmA,                                \
                                      const int32_t* element_of_facet, int64_t nentA, const double* amplitude, const double* delay,        \
                                      const int32_t* row_of_element, int64_t nelem, const double* table, int64_t nrows, int64_t nt,        \
                                      double t0, double dt, const T* xB, const T* cB, const T* detJB, const int32_t* dmB, int64_t nentB,   \
                                      int N, const double* stage_dev, void* s) {                                                           \
    return facet_source_wave<T>(y, cA1, cA2, detJA, dmA, element_of_facet, nentA, amplitude, delay, row_of_element, nelem, table, nrows,   \
                                nt, t0, dt, xB, cB, detJB, dmB, nentB, N, stage_dev, true, s);                                             \
  }                                                                                                                                        \
  int fus_point_source_wave_##SUF(T* y, const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights,       \
                                  int P, const double* amplitude, const double* delay, const int32_t* row_of_point, const double* table,   \
                                  int64_t nrows, int64_t nt, double t0, double dt, const double* stage, void* s) {                         \
    return point_source_wave<T>(y, cells, npts, dofmap, ncells, weights, P, amplitude, delay, row_of_point, table, nrows, nt, t0, dt,      \
                                stage, s);                                                                                                 \
  }
FUS_WAVE(double, f64)
FUS_WAVE(float, f32)
#undef FUS_WAVE

}  // extern "C"
