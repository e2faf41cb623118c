// libfusgpu.so: the general-G planned stiffness apply (fus_stiffness_apply_planned_*): validation + dispatch over degree and build.
// Compiled once per scalar type (-DFUS_INST_T=double|float), see Makefile and fus_dispatch.hpp.
#include "fus_dispatch.hpp"
#include "stiffness_plan.hpp"

#ifndef FUS_INST_T  // the Makefile builds both; a bare ``hipcc -c`` of this file checks the fp64 instances
#define FUS_INST_T double
#endif

namespace fus_abi {

// fp32 build with 5 waves per SIMD (only instantiated for float)
template <typename T, int P>
hipError_t launch_plan_f32_5w(const T* x, const T* cc, T* y, const T* G, const void* ws, const T* dphi, int64_t ncell,
                              int remap, hipStream_t s, bool ord, bool runs) {
  if constexpr (sizeof(T) == 4 && P <= 4)
    return fus::launch_stiffness_plan<T, P, false, true, 5>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, runs);
  else
    return fus::launch_stiffness_plan<T, P, false, true, 1>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, runs);
}

// Degrees whose fp64 auto build also ships as stiffness_plan_rows_kernel (one slot per local row, compact run tables): those where
// the rows build has no scratch and the occupancy of its stiffness_plan_kernel twin (tests/test_plan_rows_isa.py).
template <int P>
constexpr bool plan_rows_ships() {
  return P >= 2 && P <= 8;
}
// the auto build of degree P (the table in stiffness_apply_planned) as a rows launch
template <typename T, int P>
hipError_t launch_plan_rows_auto(const T* x, const T* cc, T* y, const T* G, const void* ws, const T* dphi, int64_t ncell, int remap,
                                 hipStream_t s, bool ord, int run_stride) {
  if constexpr (P <= 3)
    return fus::launch_stiffness_plan_rows<T, P, false, true, 1>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, run_stride);
  else if constexpr (P <= 5)
    return fus::launch_stiffness_plan_rows<T, P, true, true, 1>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, run_stride);
  else
    return fus::launch_stiffness_plan_rows<T, P, true, (P != 8), fus::plan_ring_min_waves<P>(), fus::plan_g_ring<P>()>(
        x, cc, y, G, ws, dphi, ncell, remap, s, ord, run_stride);
}

// Group size of the batch placement (stiffness.hpp: group_block) for degree P: the knob, or in auto the size measured per degree and
// scalar type at ~10 M dofs with tools/ab_xcd_group.py (profiles/ab_xcd_group.log: three runs on MI355X boxes, the arms alternating in one
// process).  A degree has a size only where that size passed the bar of docs/history.md 3.2 (median below the natural order's by more
// than three times the larger spread) in at least two of the three runs and was slower in none: fp64 P = 4 g = 32 (+0.5 / +1.5 ... 1.8 /
// +1.1 ... 1.8 %), fp64 P = 8 g = 16 (+1.3 ... 1.5 %), fp32 P = 3 g = 16 (+2.3 ... 2.5 %).  0 = natural order: fp64 P = 3, 5 gain 0.4 ... 1.9 %
// with g = 32 but pass in one run only, P = 2, 6, 7 gain nothing or lose from g = 16 up, the other fp32 degrees stay inside the bar.
template <typename T, int P>
int plan_xcd_group() {
  const int g = g_plan_xcd_group.load(std::memory_order_relaxed);
  if (g >= 0) return g;
  constexpr int auto_f64[11] = {0, 0, 0, 0, 32, 0, 0, 0, 16, 0, 0};
  constexpr int auto_f32[11] = {0, 0, 0, 16, 0, 0, 0, 0, 0, 0, 0};
  return sizeof(T) == 8 ? auto_f64[P] : auto_f32[P];
}

template <typename T>
int stiffness_apply_planned(const T* x, const T* cc, T* y, const T* G, const void* ws, const T* dphi, int P,
                            int64_t ncell, void* stream) {
  const bool args_ok = x && cc && y && G && dphi && !misaligned(G, 2 * sizeof(T));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int chunks = g_xcd_remap.load(std::memory_order_relaxed);
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    // placement of the batches on the XCDs, carried in the kernels' xcd_remap argument (stiffness.hpp: place_batch)
    // ... and the direction of the sweep in its flag bit (fus_dispatch.hpp: plan_sweep_down flips the plan's parity when it alternates)
    const int remap = (chunks ? 1 : plan_xcd_group<T, PP>()) | (plan_sweep_down<T>(ws, PP, ncell) ? fus::kPlaceReverse : 0);
    // Builds (profiles/r01d_ab_alias_by_degree.log, r02*_ab_*.log; pinned by tests/test_resource_usage.py):
    //   0  three LDS cubes + own x/y buffer           (P <= 3)
    //   1  LDS-aliased, whole G slab issued up front  (P = 4, 5: 4 workgroups per CU at P = 4)
    //   2  LDS-aliased, ring of G slabs               (P >= 6: registers are the binding limit there; P = 8 also
    //                                                  drops the LDS padding to fit a third workgroup per CU)
    //   30 fp32, registers allow 5 waves per SIMD     (fp32, P <= 4)
    int pv = g_plan_variant.load(std::memory_order_relaxed);
    if constexpr (sizeof(T) == 8 && plan_rows_ships<PP>()) {
      // auto build, run-coded launch, a plan whose header says rows_consecutive: the same build reading one slot per row
      if (pv < 0 && runs && g_plan_rows.load(std::memory_order_relaxed) != 0) {
        const int run_stride = plan_rows_stride(ws);
        if (run_stride > 0) return launch_plan_rows_auto<T, PP>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, run_stride);
      }
    }
    if (pv < 0) {
      if (sizeof(T) == 4)
        pv = (PP <= 4) ? 30 : 1;  // fp32: registers are not the limit, the whole G slab up front wins (r02y_ab_fp32.log)
      else {
        // measured per degree at ~10 M dofs (profiles/r02a_ab_builds_and_slp.log, r02b_ab_isolated_and_degrees.log,
        // r02h_ab_degrees_3_9_10.log, r02r_ab_degrees_8_9_10.log): the ring wins where it buys a workgroup per CU
        constexpr int best[11] = {0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2};
        pv = best[PP];
      }
    }
    switch (pv) {
      case 1: return fus::launch_stiffness_plan<T, PP, true, true, 1>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, runs);
      case 2:
        return fus::launch_stiffness_plan<T, PP, true, (PP != 8), fus::plan_ring_min_waves<PP>(), fus::plan_g_ring<PP>()>(
            x, cc, y, G, ws, dphi, ncell, remap, s, ord, runs);
      case 30: return launch_plan_f32_5w<T, PP>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, runs);
      default: return fus::launch_stiffness_plan<T, PP, false, true, 1>(x, cc, y, G, ws, dphi, ncell, remap, s, ord, runs);
    }
  });
}

template int stiffness_apply_planned<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);

}  // namespace fus_abi
