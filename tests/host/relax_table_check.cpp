// csrc/relax_table.hpp on the host (no HIP, no GPU): the three kinds of the relaxation pass against the classical RK4 of
//   xi' = kappa v - xi / tau        (v given at the four stage times)
// written out as its textbook sequence, the access flags against what relax_update reads and writes, and the touch counts of DESIGN 3.13.
// Build with -ffp-contract=off: "the same operations in the same order" is then exact.
#include <cmath>
#include <cstdio>

#include "../../fenicsx-fus-gpu_amd/csrc/relax_table.hpp"

using namespace fus;

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                               \
    }                                                        \
  } while (0)

template <typename T>
static void step_against_textbook() {
  const T A[4] = {T(0), T(0.5), T(0.5), T(1)}, B[4] = {T(1) / 6, T(1) / 3, T(1) / 3, T(1) / 6};
  const T dt = T(0.37), kappa = T(0.8), tau = T(1.3), itau = T(1) / tau;
  T xi_tab = T(0.25), xi_ref = T(0.25);
  for (int step = 0; step < 5; ++step) {
    T vn[4];
    for (int i = 0; i < 4; ++i) vn[i] = std::sin(T(0.7) * (step + A[i]) + T(0.1) * i);  // any four stage values
    // textbook: xn_i = x0 + a_i dt k_{i-1}; k_i = kappa vn_i - xn_i / tau; x += b_i dt k_i
    T x = xi_ref, k = T(0);
    const T x0 = xi_ref;
    for (int i = 0; i < 4; ++i) {
      const T xn = i == 0 ? x0 : x0 + (A[i] * dt) * k;
      k = kappa * vn[i] - xn * itau;
      x = x + (B[i] * dt) * k;
    }
    xi_ref = x;
    // the table: FIRST, MIDDLE, MIDDLE, LAST over the arrays (xi0, xin, acc); poison what a kind may not read
    T a0 = xi_tab, an = T(NAN), ac = T(NAN);
    for (int i = 0; i < 4; ++i) {
      const int kind = i == 0 ? kRelaxFirst : i == 3 ? kRelaxLast : kRelaxMiddle;
      const RelaxAccess f = relax_access(kind);
      const RelaxOut<T> o = relax_update<T>(kind, B[i] * dt, i == 3 ? T(0) : A[i + 1] * dt, kappa, itau, vn[i], f.rd_x0 ? a0 : T(NAN),
                                            f.rd_xn ? an : T(NAN), f.rd_acc ? ac : T(NAN));
      CHECK(!std::isnan(o.next));
      if (f.wr_x0) a0 = o.x0;
      if (f.wr_xn) an = o.xn;
      if (f.wr_acc) ac = o.acc;
      CHECK(o.next == (kind == kRelaxLast ? a0 : an));  // what the next stiffness apply sees
    }
    xi_tab = a0;
    CHECK(xi_tab == xi_ref);  // the same operations in the same order
  }
  CHECK(xi_tab != T(0.25));
}

int main() {
  step_against_textbook<double>();
  step_against_textbook<float>();
  // flags: FIRST reads xi0 alone and writes acc, xin; MIDDLE reads all three; LAST reads xin, acc and writes xi0
  const RelaxAccess f = relax_access(kRelaxFirst), m = relax_access(kRelaxMiddle), l = relax_access(kRelaxLast);
  CHECK(f.rd_x0 && !f.rd_xn && !f.rd_acc && !f.wr_x0 && f.wr_xn && f.wr_acc);
  CHECK(m.rd_x0 && m.rd_xn && m.rd_acc && !m.wr_x0 && m.wr_xn && m.wr_acc);
  CHECK(!l.rd_x0 && l.rd_xn && l.rd_acc && l.wr_x0 && !l.wr_xn && !l.wr_acc);
  // touches: 3 + NR (3 | 5 | 3), one more per mechanism with per-dof weights; a step is 12 + 16 NR (+ 4 NR)
  for (int nr = 1; nr <= kRelaxMaxMechanisms; ++nr) {
    CHECK(relax_touches(kRelaxFirst, nr, false) == 3 + 3 * nr);
    CHECK(relax_touches(kRelaxMiddle, nr, false) == 3 + 5 * nr);
    CHECK(relax_touches(kRelaxLast, nr, false) == 3 + 3 * nr);
    CHECK(relax_touches(kRelaxMiddle, nr, true) == 3 + 6 * nr);
    CHECK(relax_step_touches(nr, false) == 12 + 16 * nr);
    CHECK(relax_step_touches(nr, true) == 12 + 20 * nr);
  }
  static_assert(relax_step_touches(2, false) == 44, "constexpr");
  if (fails) return 1;
  std::printf("RELAX_TABLE_OK\n");
  return 0;
}
