// libfusgpu.so: the affine and the in-kernel-geometry planned stiffness applies: validation + dispatch over degree.
// Compiled once per scalar type (-DFUS_INST_T=double|float), see Makefile and fus_dispatch.hpp.
#include "fus_dispatch.hpp"
#include "stiffness_affine.hpp"
#include "stiffness_geom.hpp"

#ifndef FUS_INST_T  // the Makefile builds both; a bare ``hipcc -c`` of this file checks the fp64 instances
#define FUS_INST_T double
#endif

namespace fus_abi {

template <typename T>
int stiffness_apply_planned_affine(const T* x, const T* cc, T* y, const T* G, const T* wratio, const void* ws,
                                   const T* dphi, int P, int64_t ncell, void* stream) {
  const bool args_ok = x && cc && y && G && wratio && dphi && !misaligned(G, 2 * sizeof(T));
  hipStream_t s = static_cast<hipStream_t>(stream);
  // P <= 4: unpadded LDS + 5 waves per SIMD (+8 %, profiles/r01f_affine_fast_path.log); above, registers do
  // not allow 5 waves without spilling: padded build, compiler's own allocation
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    return fus::launch_stiffness_plan_affine<T, PP, true, (PP > 4), (PP <= 4 ? 5 : 1)>(x, cc, y, G, wratio, ws, dphi, ncell, s, ord, runs);
  });
}

template <typename T>
int stiffness_apply_planned_geom(const T* x, const T* cc, T* y, const T* x_g, const int32_t* x_dofs, const T* pts,
                                 const T* wts, const void* ws, const T* dphi, int P, int64_t ncell, void* stream) {
  const bool args_ok = x && cc && y && x_g && x_dofs && pts && wts && dphi;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    return fus::launch_stiffness_plan_geom<T, PP, (PP >= 4), true, fus::geom_min_waves<T, PP>(), fus::geom_factors_in_registers<T, PP>()>(
        x, cc, y, x_g, x_dofs, pts, wts, ws, dphi, ncell, s, ord, runs);
  });
}

template int stiffness_apply_planned_affine<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);
template int stiffness_apply_planned_geom<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, const FUS_INST_T*, const int32_t*, const FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);

}  // namespace fus_abi
