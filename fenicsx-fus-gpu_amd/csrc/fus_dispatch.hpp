// State and helpers shared by the translation units of libfusgpu.so (C ABI: include/fus_gpu.h).  The library is several objects so
// that the planned cell operators -- by far the most kernel instantiations: 10 degrees x builds x (ORDERED, RUNS) x 2 scalar types --
// compile in parallel (Makefile); everything here is ``inline`` (one instance in the linked library).
#pragma once
#include "../../include/fus_gpu.h"

#include <hip/hip_runtime.h>

#include <atomic>

#include "plan.hpp"
#include "plan_registry.hpp"
#include "plan_sweep.hpp"

namespace fus_abi {

inline std::atomic<int> g_stiffness_variant{0};
// 1 = every XCD walks one contiguous eighth of the batches (plan-free kernel and the two general-G planned kernels).  Slower on MI355X:
// it does cut the x re-fetches (fetch bytes 1147.5 -> 1064.1 MB per launch at config 3) and is still 11 % slower, 245.9 against 221.9 us
// (profiles/xcd_group_probe.log; 0.2582 against 0.2313 ms on the first planned kernel, profiles/r01b_ab_variants.log)
inline std::atomic<int> g_xcd_remap{0};
inline std::atomic<int> g_mass_variant{0};
inline std::atomic<int> g_plan_runs{1};  // 0 never, 1 auto, 2 always

// Run-length coded dof lists (8 bytes per run of consecutive dofs instead of 4 per dof; expanded in LDS by
// the apply kernels): the builder decides per batch (a list that does not compress stays raw).
inline int plan_allow_runs(int ndof_per_entity) {
  (void)ndof_per_entity;
  return g_plan_runs.load(std::memory_order_relaxed) != 0;
}
// which encoding of the dof lists a launch reads (the plan holds both).  ``runs_pay``: at least half of the plan's batches carry a
// run table -- a numbering whose lists do not compress (Morton, a graph reordering) makes a run-coded launch read every list one round
// trip late, behind a wasted speculative read of the table (+2..3 %, profiles/r05y_numbering.log)
template <typename T>
inline bool plan_use_runs(int ndof_per_entity, bool runs_pay = true) {
  const int mode = g_plan_runs.load(std::memory_order_relaxed);
  if (mode == 1 && !runs_pay) return false;
  // auto: fp64 always (+4..6 % at every degree); fp32 up to P = 8, i.e. wherever the preamble reads the run words speculatively and
  // issues its loads by every thread (plan.hpp: +7..12 % at P = 2, 4, 5, 6, +7 % at P = 7, +3 % at P = 8; P = 9, 10 keep the raw
  // lists).  Before that the fp32 limit was P = 4 (-12 % at P = 6 then): profiles/r05x_ab_run_tables.log,
  // r05x_ab_run_tables_fp32_p78.log; r02o_ab_run_tables.log, r02y_ab_fp32.log for the earlier kernels
  return mode == 2 || (mode == 1 && (sizeof(T) == 8 || ndof_per_entity <= 729));
}
inline std::atomic<int> g_plan_variant{-1};  // -1 = auto
// fp64 general-G apply: 1 (default) = a run-coded launch of a plan whose rows are all consecutive reads one slot per local ROW and the
// compact run tables (stiffness_plan_rows_kernel); 0 = never (the A/B knob: the launch then runs stiffness_plan_kernel)
inline std::atomic<int> g_plan_rows{1};
// general-G planned apply, both kernels: g consecutive batches per XCD label (stiffness.hpp: group_block).  -1 = auto (the table in
// stiffness_apply_planned), 0 = off, a power of two from 2 to 256 = g.  g_xcd_remap = 1 wins over it.
inline std::atomic<int> g_plan_xcd_group{-1};
inline bool plan_xcd_group_valid(int v) { return v == -1 || v == 0 || (v >= 2 && v <= 256 && (v & (v - 1)) == 0); }
// general-G planned apply, both kernels: the direction in which a launch walks its batches (plan_sweep.hpp).  -1 = auto, 0 = upwards,
// 1 = every launch of a plan the other way than the one before it, 2 = downwards
inline std::atomic<int> g_plan_sweep{plan_sweep_initial()};

// The one workspace registry of the library (plan_registry.hpp) is defined in fus_gpu.hip, where the header type of the gather plans is
// complete.  true if ``ws`` holds a batch plan for exactly this shape; ``ordered`` out
bool plan_check(const void* ws, int N, int epb, int64_t nent, bool* ordered, bool* exclusive = nullptr, bool* runs_pay = nullptr);

// runs per batch of the compact run tables if the plan at ``ws`` says that its rows are consecutive, else 0
int plan_rows_stride(const void* ws);

// flips the sweep parity of the batch plan at ``ws`` (one bit per workspace, under the registry's mutex) and returns the value before
// the flip: 0, 1, 0, ...
int plan_sweep_flip(const void* ws);

// Is this general-G launch a downward one?  Host state only: no device allocation, no synchronisation, no global counter.  Every plan
// has its own parity, so the sub-launches of a halo apply, which own separate plans, alternate independently.  Under stream capture the
// flip happens at capture time and the direction is baked into the node: a captured step with an EVEN number of general-G applies on a
// plan (RK4: four) ends where it began and alternates consistently across replays; an odd number repeats the last direction at the
// seam between two replays and merely loses the gain on that pair.
template <typename T>
inline bool plan_sweep_down(const void* ws, int P, int64_t ncell) {
  const int knob = g_plan_sweep.load(std::memory_order_relaxed);
  if (plan_sweep_alternates(knob, P, (int)sizeof(T), ncell)) return plan_sweep_flip(ws) == 1;
  return knob == 2;
}

inline int hip_rc(hipError_t e) { return e == hipSuccess ? FUS_OK : FUS_ERR_HIP_BASE - (int)e; }

inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// The one switch from the runtime degree to code compiled per degree: K is a generic lambda taking std::integral_constant<int, P>
// (as plan_dispatch, plan.hpp, takes its two booleans).  false, and K not called, for a degree outside the supported range.
static_assert(FUS_MIN_DEGREE == 1 && FUS_MAX_DEGREE == 10, "degree_dispatch lists the supported degrees");
template <typename K>
inline bool degree_dispatch(int P, K&& k) {
  switch (P) {
    case 1: k(std::integral_constant<int, 1>{}); return true;
    case 2: k(std::integral_constant<int, 2>{}); return true;
    case 3: k(std::integral_constant<int, 3>{}); return true;
    case 4: k(std::integral_constant<int, 4>{}); return true;
    case 5: k(std::integral_constant<int, 5>{}); return true;
    case 6: k(std::integral_constant<int, 6>{}); return true;
    case 7: k(std::integral_constant<int, 7>{}); return true;
    case 8: k(std::integral_constant<int, 8>{}); return true;
    case 9: k(std::integral_constant<int, 9>{}); return true;
    case 10: k(std::integral_constant<int, 10>{}); return true;
  }
  return false;
}

inline int64_t plan_bytes(int P, int64_t ncell) {
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  return fus::plan_view(nullptr, P, fus::cells_per_batch(P), ncell).bytes;
}

// What the entry points of the planned cell operators check and decide in common, in the order of their error codes: negative cell count,
// degree, the empty mesh (FUS_OK before any pointer is looked at), the entry's own arguments (``args_ok``: its null pointers and the
// alignment of its G) and the workspace, the plan of the workspace; then which list encoding the launch reads (plan_use_runs) and the
// degree.  ``launch`` is a generic lambda (std::integral_constant<int, P>, bool ordered, bool use_runs) -> hipError_t.
template <typename T, typename L>
int planned_cell_entry(bool args_ok, const void* ws, int P, int64_t ncell, L&& launch) {
  if (ncell < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  if (ncell == 0) return FUS_OK;
  if (!args_ok || !ws || misaligned(ws, 256)) return FUS_ERR_INVALID_ARGUMENT;
  const int Nd = (P + 1) * (P + 1) * (P + 1);
  bool ord = false, rp = true;
  if (!plan_check(ws, Nd, fus::cells_per_batch(P), ncell, &ord, nullptr, &rp)) return FUS_ERR_PLAN_MISMATCH;
  const bool use_runs = plan_use_runs<T>(Nd, rp);
  hipError_t e = hipErrorInvalidValue;
  degree_dispatch(P, [&](auto p) { e = launch(p, ord, use_runs); });
  return hip_rc(e);
}

// ---- the planned cell operators: defined and explicitly instantiated (one object per operator family and scalar type, compiled in
// parallel: Makefile) in dispatch_stiffness_plan.hip, dispatch_geometry.hip and dispatch_westervelt.hip
template <typename T>
int stiffness_apply_planned(const T* x, const T* cc, T* y, const T* G, const void* ws, const T* dphi, int P, int64_t ncell, void* stream);
template <typename T>
int stiffness_apply_planned_affine(const T* x, const T* cc, T* y, const T* G, const T* wratio, const void* ws, const T* dphi, int P,
                                   int64_t ncell, void* stream);
template <typename T>
int stiffness_apply_planned_geom(const T* x, const T* cc, T* y, const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts,
                                 const void* ws, const T* dphi, int P, int64_t ncell, void* stream);
template <typename T>
int stiffness_apply_planned_geom_nodal(const T* x, const T* cc, const T* nodal, T* y, const T* x_g, const int32_t* x_dofs, const T* pts,
                                       const T* wts, const void* ws, const T* dphi, int P, int64_t ncell, void* stream);  // dispatch_stiffness_nodal.hip
template <typename T>
int westervelt_stiffness_apply_planned_geom_nodal(const T* u, const T* v, const T* c3, const T* c4, const T* nodal3, const T* nodal4, T* b,
                                                  const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts, const void* ws,
                                                  const T* dphi, int P, int64_t ncell, void* stream);  // dispatch_westervelt_nodal.hip
template <typename T>
int westervelt_cell(const T* u, const T* v, const T* c2, const T* c3, const T* c4, const T* c5, T* b, T* m, const T* G, const T* detJ,
                    const void* ws, const T* dphi, int P, int64_t ncell, void* stream);
template <typename T>
int westervelt_cell_geom(const T* u, const T* v, const T* c2, const T* c3, const T* c4, const T* c5, T* b, T* m, const T* x_g,
                         const int32_t* x_dofs, const T* pts, const T* wts, const void* ws, const T* dphi, int P, int64_t ncell,
                         void* stream);
template <typename T>
int gradient_apply_planned_geom(const T* x, const T* cc, T* y, int64_t ystride, const T* x_g, const int32_t* x_dofs, const T* pts,
                                const T* wts, const void* ws, const T* dphi, int P, int64_t ncell, void* stream);  // dispatch_gradient.hip

}  // namespace fus_abi
