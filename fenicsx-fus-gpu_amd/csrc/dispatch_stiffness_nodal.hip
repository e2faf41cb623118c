// libfusgpu.so: the planned stiffness apply with a nodal coefficient and the geometry formed in the kernel: validation + dispatch over
// degree.  Compiled once per scalar type (-DFUS_INST_T=double|float), see Makefile and fus_dispatch.hpp.
#include "fus_dispatch.hpp"
#include "stiffness_geom_nodal.hpp"

#ifndef FUS_INST_T  // the Makefile builds both; a bare ``hipcc -c`` of this file checks the fp64 instances
#define FUS_INST_T double
#endif

namespace fus_abi {

// The (ORDERED, RUNS) shapes, the cells per batch, the LDS aliasing and the flux form per degree are those of the per-cell kernel
// (dispatch_geometry.hip: stiffness_apply_planned_geom).
template <typename T>
int stiffness_apply_planned_geom_nodal(const T* x, const T* cc, const T* nodal, T* y, const T* x_g, const int32_t* x_dofs, const T* pts,
                                       const T* wts, const void* ws, const T* dphi, int P, int64_t ncell, void* stream) {
  const bool args_ok = x && cc && nodal && y && x_g && x_dofs && pts && wts && dphi;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    return fus::launch_stiffness_plan_geom_nodal<T, PP, (PP >= 4), true, fus::nodal_min_waves<T, PP>(), fus::nodal_factors_in_registers<T, PP>()>(
        x, cc, nodal, y, x_g, x_dofs, pts, wts, ws, dphi, ncell, s, ord, runs);
  });
}

template int stiffness_apply_planned_geom_nodal<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, const FUS_INST_T*, const int32_t*, const FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);

}  // namespace fus_abi
