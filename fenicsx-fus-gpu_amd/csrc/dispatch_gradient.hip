// libfusgpu.so: the planned weak gradient with in-kernel geometry: validation + dispatch over degree.
// Compiled once per scalar type (-DFUS_INST_T=double|float), see Makefile and fus_dispatch.hpp.
#include "fus_dispatch.hpp"
#include "gradient_geom.hpp"

#ifndef FUS_INST_T  // the Makefile builds both; a bare ``hipcc -c`` of this file checks the fp64 instances
#define FUS_INST_T double
#endif

namespace fus_abi {

template <typename T>
int gradient_apply_planned_geom(const T* x, const T* cc, T* y, int64_t ystride, const T* x_g, const int32_t* x_dofs, const T* pts,
                                const T* wts, const void* ws, const T* dphi, int P, int64_t ncell, void* stream) {
  const bool args_ok = x && cc && y && ystride >= 0 && x_g && x_dofs && pts && wts && dphi;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    return fus::launch_gradient_plan_geom<T, PP>(x, cc, y, ystride, x_g, x_dofs, pts, wts, ws, dphi, ncell, s, ord, runs);
  });
}

template int gradient_apply_planned_geom<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, int64_t, const FUS_INST_T*, const int32_t*, const FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);

}  // namespace fus_abi
