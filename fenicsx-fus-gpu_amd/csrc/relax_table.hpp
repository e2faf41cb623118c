// The stage kinds of the relaxation pass (relaxation.hpp), once, free of HIP (any C++17 host compiler, like rk4_table.hpp;
// tests/host/relax_table_check.cpp checks it without a GPU): what a kind computes for one memory variable (relax_update), which of
// its three arrays it reads and writes (relax_access), and how many vector touches a pass is (relax_touches: counted from the flags).
//
// A memory variable obeys  xi' = kappa v - xi / tau  and is advanced by the classical RK4 of (u, v): with the slope of the stage's
// inputs  k = kappa vn - xin / tau,  bw = b_i dt and aw = a_{i+1} dt,
//   0 FIRST    (xin of this stage is xi0 itself)   reads xi0,            writes acc xin:   acc = xi0 + bw k ;  xin = xi0 + aw k
//   1 MIDDLE                                       reads xi0 xin acc,    writes acc xin:   acc += bw k      ;  xin = xi0 + aw k
//   2 LAST                                         reads xin acc,        writes xi0:       xi0 = acc + bw k
// the three kinds of bioheat_stage_kernel.  ``next`` is the variable the NEXT stiffness apply sees (the new xin; after LAST the new
// xi0): the pass sums it into ur = u_n + sum_nu xi_nu.
#pragma once

#if defined(__HIPCC__)
#define FUS_RELAX_TABLE_FN __host__ __device__ __forceinline__
#else
#define FUS_RELAX_TABLE_FN inline
#endif

namespace fus {

enum { kRelaxFirst = 0, kRelaxMiddle = 1, kRelaxLast = 2 };
constexpr int kRelaxMaxMechanisms = 4;

// which of a mechanism's three arrays a kind reads / writes
struct RelaxAccess {
  bool rd_x0, rd_xn, rd_acc, wr_x0, wr_xn, wr_acc;
};
FUS_RELAX_TABLE_FN constexpr RelaxAccess relax_access(int kind) {
  switch (kind) {
    case kRelaxFirst: return {true, false, false, false, true, true};
    case kRelaxLast: return {false, true, true, true, false, false};
    default: return {true, true, true, false, true, true};  // MIDDLE
  }
}
// vector touches of one pass over ``nr`` mechanisms: u_base and vn read, ur written; per mechanism the flagged arrays and, with
// per-dof weights, its row of kappa
FUS_RELAX_TABLE_FN constexpr int relax_touches(int kind, int nr, bool per_dof_weights) {
  const RelaxAccess a = relax_access(kind);
  return 3 + nr * (a.rd_x0 + a.rd_xn + a.rd_acc + a.wr_x0 + a.wr_xn + a.wr_acc + (per_dof_weights ? 1 : 0));
}
// touches of the four passes of one step (FIRST, MIDDLE, MIDDLE, LAST)
FUS_RELAX_TABLE_FN constexpr int relax_step_touches(int nr, bool per_dof_weights) {
  return relax_touches(kRelaxFirst, nr, per_dof_weights) + 2 * relax_touches(kRelaxMiddle, nr, per_dof_weights) +
         relax_touches(kRelaxLast, nr, per_dof_weights);
}

template <typename T>
struct RelaxOut {
  T x0, xn, acc, next;  // what the flags of relax_access say is written, and the variable the next stage sees
};
// one memory variable of one dof (all operands in registers); vn: the stage's v_n; itau = 1 / tau
template <typename T>
FUS_RELAX_TABLE_FN RelaxOut<T> relax_update(int kind, T bw, T aw, T kappa, T itau, T vn, T x0, T xn, T acc) {
  RelaxOut<T> o{};
  const T xs = kind == kRelaxFirst ? x0 : xn;  // the stage's input
  const T k = kappa * vn - xs * itau;
  if (kind == kRelaxLast) {
    o.x0 = acc + bw * k;
    o.next = o.x0;
  } else {
    o.acc = (kind == kRelaxFirst ? x0 : acc) + bw * k;
    o.xn = x0 + aw * k;
    o.next = o.xn;
  }
  return o;
}

}  // namespace fus

#undef FUS_RELAX_TABLE_FN
