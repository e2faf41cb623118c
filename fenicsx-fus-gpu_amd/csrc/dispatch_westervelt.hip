// libfusgpu.so: the fused Westervelt cell passes (general G and in-kernel geometry): validation + dispatch over degree.
// Compiled once per scalar type (-DFUS_INST_T=double|float), see Makefile and fus_dispatch.hpp.
#include "fus_dispatch.hpp"
#include "westervelt.hpp"
#include "westervelt_geom.hpp"

#ifndef FUS_INST_T  // the Makefile builds both; a bare ``hipcc -c`` of this file checks the fp64 instances
#define FUS_INST_T double
#endif

namespace fus_abi {

template <typename T>
int westervelt_cell(const T* u, const T* v, const T* c2, const T* c3, const T* c4, const T* c5, T* b, T* m, const T* G,
                    const T* detJ, const void* ws, const T* dphi, int P, int64_t ncell, void* stream) {
  const bool mass = c2 || c5 || m || detJ;  // all four or none: none = the stiffness part alone
  const bool args_ok = u && v && c3 && c4 && b && G && dphi && (!mass || (c2 && c5 && m && detJ)) && !misaligned(G, 2 * sizeof(T));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    return mass ? fus::launch_westervelt_cell<T, PP, true>(u, v, c2, c3, c4, c5, b, m, G, detJ, ws, dphi, ncell, s, ord, runs)
                : fus::launch_westervelt_cell<T, PP, false>(u, v, c2, c3, c4, c5, b, m, G, detJ, ws, dphi, ncell, s, ord, runs);
  });
}

template <typename T>
int westervelt_cell_geom(const T* u, const T* v, const T* c2, const T* c3, const T* c4, const T* c5, T* b, T* m,
                         const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts, const void* ws, const T* dphi,
                         int P, int64_t ncell, void* stream) {
  const bool mass = c2 || c5 || m;
  const bool args_ok = u && v && c3 && c4 && b && x_g && x_dofs && pts && wts && dphi && (!mass || (c2 && c5 && m));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return planned_cell_entry<T>(args_ok, ws, P, ncell, [&](auto p, bool ord, bool runs) {
    constexpr int PP = decltype(p)::value;
    return mass ? fus::launch_westervelt_cell_geom<T, PP, true>(u, v, c2, c3, c4, c5, b, m, x_g, x_dofs, pts, wts, ws, dphi, ncell, s, ord, runs)
                : fus::launch_westervelt_cell_geom<T, PP, false>(u, v, c2, c3, c4, c5, b, m, x_g, x_dofs, pts, wts, ws, dphi, ncell, s, ord, runs);
  });
}

template int westervelt_cell<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);
template int westervelt_cell_geom<FUS_INST_T>(const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, const FUS_INST_T*, FUS_INST_T*, FUS_INST_T*, const FUS_INST_T*, const int32_t*, const FUS_INST_T*, const FUS_INST_T*, const void*, const FUS_INST_T*, int, int64_t, void*);

}  // namespace fus_abi
