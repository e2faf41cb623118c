// Stand-alone check of csrc/rk4_table.hpp (host-only: any C++17 compiler, no HIP, no GPU), for double and float.  Build with
// -ffp-contract=off: "the same operations in the same order" is then exact on the host.
//   (a) kinds 2, 0, 0, 3 run one step bitwise as the reference's sequence of copies, axpys and one divide (the list at the top of
//       csrc/rk4.hpp), written out as plain loops; a step that ends with the legacy kind 1 and aw = 0 gives the same (u0, v0) and leaves
//       un == u0, ku == v0.  The same with the Westervelt kv against the reference's m = m0 + w2 u_n, b += w5 v_n^2.
//   (b) the lean kinds 4, 5, 6, 7 against (a): u and the un entering the last stage bitwise, v and ku to 1e-14 / 1e-6 of the largest
//       magnitude (the bound of test_lean_rk4_stage_kinds_equal_the_reference_sequence).
//   (c) the access flags against the arithmetic, for both access descriptions: what the flags call unread is poisoned with NaN, what
//       they call written must come out finite.  This catches a read or write flag that is missing; a read flag too many (a vector
//       loaded and never used) shows only in (d).  The per-dof loads and stores of the kernels (rk4.hpp) are not run here: the GPU test
//       test_rk4_stage_kinds_equal_the_numpy_table does that.
//   (d) the touch counts derived from the flags: the figures of DESIGN.md and benchlib/roofline.py.
// tests/test_rk4_table_host.py builds and runs it; it is also the program to build with -fsanitize=address,undefined.
// Prints RK4_TABLE_OK and exits 0.
#include "../../fenicsx-fus-gpu_amd/csrc/rk4_table.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace fus;

static int failures = 0;
#define CHECK(cond) \
  if (!(cond)) std::printf("FAILED line %d: %s\n", __LINE__, #cond), ++failures

constexpr int N = 307;  // dofs

// fixed-seed generator: uniform in (-1, 1), never 0
struct Lcg {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(s >> 11) + 0.5) / 4503599627370496.0 - 1.0;
  }
};
template <typename T>
using Vec = std::vector<T>;
template <typename T>
static Vec<T> random_vec(Lcg& g, double scale = 1.0, double shift = 0.0) {
  Vec<T> x(N);
  for (T& e : x) e = (T)(shift + scale * g.next());
  return x;
}
template <typename T>
static Vec<T> poison() {
  return Vec<T>(N, std::numeric_limits<T>::quiet_NaN());
}
template <typename T>
static bool bitwise_equal(const Vec<T>& a, const Vec<T>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}
template <typename T>
static bool all_finite(const Vec<T>& a) {
  for (T e : a)
    if (!std::isfinite(e)) return false;
  return true;
}
template <typename T>
static double max_abs(const Vec<T>& a) {
  double m = 0;
  for (T e : a) m = std::fabs((double)e) > m ? std::fabs((double)e) : m;
  return m;
}
template <typename T>
static double max_diff(const Vec<T>& a, const Vec<T>& b) {
  double m = 0;
  for (int j = 0; j < N; ++j) m = std::fabs((double)a[j] - (double)b[j]) > m ? std::fabs((double)a[j] - (double)b[j]) : m;
  return m;
}

template <typename T>
struct State {
  Vec<T> b, u, v, u0, v0, ku, un, w;
};
template <typename T>
struct Mass {
  Vec<T> minv, m0, w2, w5;
};

// One vector pass as the kernels make it, except that EVERY input is loaded: what the flags call unread is poisoned by the caller.
template <typename T>
static void pass(int kind, T bw, T aw, bool westervelt, bool with_w, T kappa, const Mass<T>& m, State<T>& s) {
  for (int j = 0; j < N; ++j) {
    const Rk4In<T> in{s.u[j], s.v[j], s.u0[j], s.v0[j], s.ku[j]};
    const Rk4WesterveltAccess wa = rk4_westervelt_access(kind, with_w);
    const Rk4Access a = westervelt ? Rk4Access(wa) : rk4_access(kind);
    const bool start = rk4_stage_inputs_are_start(kind);
    const T kv = westervelt ? rk4_westervelt_kv(s.b[j], m.w5[j], m.m0[j], m.w2[j], start ? in.u0 : s.un[j], start ? in.v0 : in.ku)
                            : s.b[j] * m.minv[j];
    const Rk4Out<T> o = rk4_update<T>(kind, bw, aw, in, kv);
    if (a.wr_u) s.u[j] = o.u;
    if (a.wr_v) s.v[j] = o.v;
    if (a.wr_n) s.un[j] = o.un, s.ku[j] = o.ku;
    if (a.wr_u0) s.u0[j] = o.u0;
    if (a.wr_v0) s.v0[j] = o.v0;
    if (westervelt && wa.wr_w) s.w[j] = rk4_next_combined(kind, kappa, in, o);
    s.b[j] = T(0);
  }
}

template <typename T>
struct Problem {
  Vec<T> u_start, v_start, rhs[4];
  Mass<T> m;
  T bw[4], aw[4];  // b_i dt, a_{i+1} dt
};
template <typename T>
static Problem<T> problem() {
  Lcg g;
  Problem<T> p;
  p.u_start = random_vec<T>(g), p.v_start = random_vec<T>(g);
  for (auto& r : p.rhs) r = random_vec<T>(g);
  p.m = {random_vec<T>(g, 0.5, 1.5), random_vec<T>(g, 0.5, 4.5), random_vec<T>(g, 0.01), random_vec<T>(g)};
  const T dt = (T)0.37, B[4] = {T(1) / 6, T(1) / 3, T(1) / 3, T(1) / 6}, A[5] = {T(0), T(0.5), T(0.5), T(1), T(0)};
  for (int i = 0; i < 4; ++i) p.bw[i] = B[i] * dt, p.aw[i] = A[i + 1] * dt;
  return p;
}

// the solution after the step, the last stage's inputs, and the (un, ku) left behind
template <typename T>
struct Step {
  Vec<T> u, v, un4, ku4, un_end, ku_end;
};
// one step through the table; every vector but (u0, v0) starts poisoned: a kind may read only what an earlier pass wrote
template <typename T>
static Step<T> table_step(const Problem<T>& p, const int (&kinds)[4], bool lean, bool westervelt) {
  State<T> s{poison<T>(), poison<T>(), poison<T>(), p.u_start, p.v_start, poison<T>(), poison<T>(), poison<T>()};
  Step<T> r;
  for (int i = 0; i < 4; ++i) {
    s.b = p.rhs[i];
    if (i == 3) r.un4 = s.un, r.ku4 = s.ku;
    pass<T>(kinds[i], lean ? p.bw[0] : p.bw[i], lean ? p.aw[0] : p.aw[i], westervelt, false, T(0), p.m, s);
    CHECK(max_abs(s.b) == 0.0);
  }
  r.u = s.u0, r.v = s.v0, r.un_end = s.un, r.ku_end = s.ku;
  return r;
}
// The reference's sequence: copies, axpys, one divide per stage (1 / m precomputed in the linear solver: a product), as loops.
template <typename T>
static Step<T> reference_step(const Problem<T>& p, bool westervelt) {
  Vec<T> u = p.u_start, v = p.v_start, u0(N), v0(N), un(N), vn(N), ku(N, T(0)), kv(N, T(0)), b(N), mm(N);
  Step<T> r;
  const T a_dt[4] = {T(0), p.aw[0], p.aw[1], p.aw[2]};
  for (int j = 0; j < N; ++j) u0[j] = u[j];  // copy
  for (int j = 0; j < N; ++j) v0[j] = v[j];  // copy
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < N; ++j) un[j] = u0[j];              // copy
    for (int j = 0; j < N; ++j) vn[j] = v0[j];              // copy
    for (int j = 0; j < N; ++j) un[j] += a_dt[i] * ku[j];   // axpy
    for (int j = 0; j < N; ++j) vn[j] += a_dt[i] * kv[j];   // axpy
    for (int j = 0; j < N; ++j) ku[j] = vn[j];              // copy (f0)
    if (i == 3) r.un4 = un, r.ku4 = ku;
    for (int j = 0; j < N; ++j) b[j] = p.rhs[i][j];         // the operator's part
    if (westervelt) {
      for (int j = 0; j < N; ++j) mm[j] = p.m.m0[j] + p.m.w2[j] * un[j];       // m = m0 + M(c2) u_n
      for (int j = 0; j < N; ++j) b[j] = b[j] + p.m.w5[j] * vn[j] * vn[j];     // b += M(c5) v_n^2
      for (int j = 0; j < N; ++j) kv[j] = b[j] / mm[j];                        // pointwise_divide
    } else {
      for (int j = 0; j < N; ++j) kv[j] = b[j] * p.m.minv[j];                  // pointwise_divide
    }
    for (int j = 0; j < N; ++j) u[j] += p.bw[i] * ku[j];    // axpy
    for (int j = 0; j < N; ++j) v[j] += p.bw[i] * kv[j];    // axpy
  }
  r.u = u, r.v = v;
  return r;
}

template <typename T>
static void steps(double tol) {
  const Problem<T> p = problem<T>();
  for (int westervelt = 0; westervelt < 2; ++westervelt) {
    // (a)
    const Step<T> ref = reference_step<T>(p, westervelt != 0);
    const Step<T> tab = table_step<T>(p, {2, 0, 0, 3}, false, westervelt != 0);
    CHECK(all_finite(ref.u) && all_finite(ref.v));
    CHECK(bitwise_equal(tab.u, ref.u));
    CHECK(bitwise_equal(tab.v, ref.v));
    CHECK(bitwise_equal(tab.un4, ref.un4) && bitwise_equal(tab.ku4, ref.ku4));
    Problem<T> q = p;
    q.aw[3] = T(0);
    const Step<T> legacy = table_step<T>(q, {2, 0, 0, 1}, false, westervelt != 0);
    CHECK(bitwise_equal(legacy.u, tab.u) && bitwise_equal(legacy.v, tab.v));
    CHECK(bitwise_equal(legacy.un_end, legacy.u) && bitwise_equal(legacy.ku_end, legacy.v));
    // (b)
    const Step<T> lean = table_step<T>(p, {4, 5, 6, 7}, true, westervelt != 0);
    if (!westervelt) {  // (the Westervelt pass feeds un and ku back into kv: its u differs with v's rounding from the second stage on)
      CHECK(bitwise_equal(lean.u, tab.u));
      CHECK(bitwise_equal(lean.un4, tab.un4));
    }
    CHECK(max_diff(lean.u, tab.u) <= tol * max_abs(tab.u));
    CHECK(max_diff(lean.un4, tab.un4) <= tol * max_abs(tab.un4));
    CHECK(max_diff(lean.v, tab.v) <= tol * max_abs(tab.v));
    CHECK(max_diff(lean.ku4, tab.ku4) <= tol * max_abs(tab.ku4));
  }
}

// (c)
template <typename T>
static void access_consistency() {
  Lcg g;
  const Mass<T> m{random_vec<T>(g, 0.5, 1.5), random_vec<T>(g, 0.5, 4.5), random_vec<T>(g, 0.01), random_vec<T>(g)};
  for (int kind = 0; kind < 8; ++kind)
    for (int mode = 0; mode < 3; ++mode) {  // linear, Westervelt, Westervelt with w
      const bool westervelt = mode > 0, with_w = mode == 2;
      const Rk4WesterveltAccess wa = rk4_westervelt_access(kind, with_w);
      const Rk4Access a = westervelt ? Rk4Access(wa) : rk4_access(kind);
      State<T> s{random_vec<T>(g), random_vec<T>(g), random_vec<T>(g), random_vec<T>(g), random_vec<T>(g), random_vec<T>(g), random_vec<T>(g), poison<T>()};
      if (!a.rd_u) s.u = poison<T>();
      if (!a.rd_v) s.v = poison<T>();
      if (!a.rd_0 && !(westervelt && wa.rd_u0)) s.u0 = poison<T>();
      if (!a.rd_0) s.v0 = poison<T>();
      if (!a.rd_ku) s.ku = poison<T>();
      if (!(westervelt && wa.rd_un)) s.un = poison<T>();
      pass<T>(kind, T(0.3), T(0.7), westervelt, with_w, T(0.25), m, s);
      if (a.wr_u) CHECK(all_finite(s.u));
      if (a.wr_v) CHECK(all_finite(s.v));
      if (a.wr_n) CHECK(all_finite(s.un) && all_finite(s.ku));
      if (a.wr_u0) CHECK(all_finite(s.u0));
      if (a.wr_v0) CHECK(all_finite(s.v0));
      CHECK(wa.wr_w == with_w);
      if (with_w) CHECK(all_finite(s.w));
      CHECK(max_abs(s.b) == 0.0);
    }
}

// (d)
static void touches() {
  static_assert(rk4_touches(0) == 12 && rk4_westervelt_touches(7, true) == 11, "the counts are constant expressions");
  const int linear[8] = {12, 12, 9, 8, 7, 10, 12, 5}, westervelt[8] = {15, 15, 11, 11, 9, 13, 15, 9};
  for (int kind = 0; kind < 8; ++kind) {
    CHECK(rk4_touches(kind) == linear[kind]);
    CHECK(rk4_westervelt_touches(kind, false) == westervelt[kind]);
    CHECK(rk4_westervelt_touches(kind, true) == westervelt[kind] + 1 + (kind == 7));  // w written; LAST' reads u0 for it
    CHECK(rk4_stage_inputs_are_start(kind) == (kind == 2 || kind == 4));
  }
  CHECK(rk4_touches(2) + rk4_touches(0) + rk4_touches(0) + rk4_touches(3) == 41);
  CHECK(rk4_touches(4) + rk4_touches(5) + rk4_touches(6) + rk4_touches(7) == 34);
  auto w = [](int kind) { return rk4_westervelt_touches(kind, false); };
  CHECK(w(2) + w(0) + w(0) + w(3) == 52);
  CHECK(w(4) + w(5) + w(6) + w(7) == 46);
}

int main() {
  steps<double>(1e-14);
  steps<float>(1e-6);
  access_consistency<double>();
  access_consistency<float>();
  touches();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("RK4_TABLE_OK\n");
  return 0;
}
