// libfusgpu.so: the Westervelt cell pass with nodal coefficients and the geometry formed in the kernel: validation + dispatch over
// degree.  Compiled once per scalar type (-DFUS_INST_T=double|float), see Makefile and fus_dispatch.hpp.
#include "fus_dispatch.hpp"
#include "westervelt_geom_nodal.hpp"

#ifndef FUS_INST_T  // the Makefile builds both; a bare ``hipcc -c`` of this file checks the fp64 instances
#define FUS_INST_T double
#endif

namespace fus_abi {

// The (ORDERED, RUNS) shapes and the cells per batch are those of the other planned cell kernels with in-kernel geometry
// (dispatch_westervelt.hip: westervelt_cell_geom; dispatch_stiffness_nodal.hip).
template <typename T>
int westervelt_stiffness_apply_planned_geom_nodal(const T* u, const T* v, const T* c3, const T* c4, const T* nodal3, const T* nodal4, T* b,
                                                  const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts, const void* ws,
                                                  const T* dphi, int P, int64_t ncell, void* stream) {
  const bool args_ok = u && v && c3 && c4 && nodal3 && nodal4 && b && x_g && x_dofs && pts && wts && dphi;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    return fus::launch_westervelt_cell_geom_nodal<T, PP>(u, v, c3, c4, nodal3, nodal4, b, x_g, x_dofs, pts, wts, ws, dphi, ncell, s, ord, runs);
  });
}

template int westervelt_stiffness_apply_planned_geom_nodal<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, const FUS_INST_T*, const int32_t*, const FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);

}  // namespace fus_abi
