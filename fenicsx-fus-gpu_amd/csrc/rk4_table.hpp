// The stage kinds of the fused RK4 vector pass, once, free of HIP (any C++17 host compiler, like stream_shape.hpp and halo_layout.hpp;
// tests/host/rk4_table_check.cpp checks it without a GPU): what a kind computes (rk4_update), which vectors it reads and writes
// (rk4_access; rk4_westervelt_access for the pass that forms kv from the stage's inputs), and how many vector touches that is
// (rk4_touches, rk4_westervelt_touches: counted from the access flags).  rk4_stage_kernel (rk4.hpp) runs it.  The two Westervelt
// kernels (westervelt.hpp) compute the same kinds, differing in how they form kv and in their access shape, but still from their own
// inline statement: the Westervelt part at the end of this header describes them and is not called by them.
#pragma once

#if defined(__HIPCC__)
#define FUS_RK4_TABLE_FN __host__ __device__ __forceinline__
#else
#define FUS_RK4_TABLE_FN inline
#endif

namespace fus {

// ``kind`` (the ABI's ``new_step`` argument):
//   0 MIDDLE   stages 2, 3:  reads b minv ku u v u0 v0, writes u v un ku b            (12 vector touches)
//   1 legacy   last stage that also materialises the next step's stage inputs
//              (u0 = u, v0 = v, un = u, ku = v): reads 5, writes 7
//   2 FIRST    stage 1 of a step whose inputs ARE (u0, v0) -- the driver hands u0 / v0 to the operator
//              instead of copies of them: reads b minv u0 v0, writes u v un ku b        (9 touches)
//   3 LAST     stage 4: the new solution goes straight to u0 / v0, nothing else is materialised:
//              reads b minv ku u v, writes u0 v0 b                                      (8 touches)
// A step run as FIRST, MIDDLE, MIDDLE, LAST moves 41 vector touches instead of 48 with the same
// arithmetic in the same order (bitwise the same u, v).
//
// LEAN kinds 4, 5, 6, 7 (round 6; one per stage of a step, used as a set; bw = b_runge[0] dt = dt / 6, aw = a_runge[1] dt = dt / 2, the
// other coefficients are their exact doubles): 34 touches.  The floor argument: b must be complete before kv = b / m, so
// every pass reads b, minv and re-zeroes b (3); passes 1-3 must write the next stage's (un, vn) (2) and need (u0, v0) for them (2);
// passes 2, 3 read vn of their own stage (1): 26.  What is left is the traffic of the two accumulators (15 of the 41), and it shrinks because
//   * u's increments are the vn's, each KNOWN ONE PASS EARLY (vn_{i+1} is formed in pass i): pass 2 writes u0 + b1 v0 + b2 vn2 + b3 vn3,
//     pass 3 adds b4 vn4 and writes the NEW u straight into u0 (u0 is dead once un4 has been formed) -- pass 4 does not touch u at all;
//   * pass 1 writes neither accumulator: pass 2 reads u0, v0, vn2 anyway and re-derives u0 + b1 v0 and b1 kv1 = (vn2 - v0) b1 / a2 (a
//     first-order difference scaled by b1 / a2 = 1 / 3: absolute error eps |v0| / 3, the size of v's own rounding).
//   4 FIRST'   reads b minv u0 v0,            writes un ku b            (7)
//   5 SECOND'  reads b minv u0 v0 ku,         writes u v un ku b        (10)   u = accumulator INCLUDING b3 vn3
//   6 THIRD'   reads b minv u0 v0 ku u v,     writes u0 v un ku b       (12)   u0 = new u
//   7 LAST'    reads b minv v,                writes v0 b               (5)    v0 = new v
// u is formed with the reference's operations in the reference's order (bitwise the same); v differs from the sequence above in the
// rounding of b1 kv1 only.  Deriving more (v's accumulator in pass 3 from un and u0) would divide a difference of u's by dt twice:
// not done.

// one dof of the stage (all operands in registers)
template <typename T>
struct Rk4In {
  T u, v, u0, v0, ku;
};
template <typename T>
struct Rk4Out {
  T u, v, u0, v0, un, ku;
};
// which vectors a stage kind reads / writes (b and the mass operand are always read, b is always re-zeroed); rd_0: u0 AND v0,
// wr_n: un AND ku
struct Rk4Access {
  bool rd_u, rd_v, rd_0, rd_ku, wr_u, wr_v, wr_n, wr_u0, wr_v0;
};
FUS_RK4_TABLE_FN constexpr Rk4Access rk4_access(int kind) {
  switch (kind) {
    case 1: return {true, true, false, true, true, true, true, true, true};
    case 2: return {false, false, true, false, true, true, true, false, false};
    case 3: return {true, true, false, true, false, false, false, true, true};
    case 4: return {false, false, true, false, false, false, true, false, false};
    case 5: return {false, false, true, true, true, true, true, false, false};
    case 6: return {true, true, true, true, false, true, true, true, false};
    case 7: return {false, true, false, false, false, false, false, false, true};
    default: return {true, true, true, true, true, true, true, false, false};  // 0 MIDDLE
  }
}
// vector touches of one pass: b read + zeroed, the mass operand(s), the flagged reads and writes
FUS_RK4_TABLE_FN constexpr int rk4_touches(const Rk4Access& a, int mass_operands) {
  return 2 + mass_operands + a.rd_u + a.rd_v + 2 * a.rd_0 + a.rd_ku + a.wr_u + a.wr_v + 2 * a.wr_n + a.wr_u0 + a.wr_v0;
}
FUS_RK4_TABLE_FN constexpr int rk4_touches(int kind) { return rk4_touches(rk4_access(kind), 1); }  // the linear pass: minv

// The arithmetic of the table above.  kv = (M^-1 b) of this stage, the one thing the passes differ in: b * minv in rk4_stage_kernel,
// which calls this; (b + w5 vn^2) / (m0 + w2 un) and b / m in the two Westervelt kernels, which do not yet (see the end of this header).
template <typename T>
FUS_RK4_TABLE_FN Rk4Out<T> rk4_update(int kind, T bw, T aw, const Rk4In<T>& in, T kv) {
  Rk4Out<T> o{};
  if (kind >= 4) {  // LEAN set: bw = dt / 6, aw = dt / 2
    const T b2 = bw + bw, a4 = aw + aw;
    if (kind == 4) {
      o.un = in.u0 + aw * in.v0;
      o.ku = in.v0 + aw * kv;
    } else if (kind == 5) {
      const T vn2 = in.ku, vn3 = in.v0 + aw * kv;
      o.v = (in.v0 + (vn2 - in.v0) * (bw / aw)) + b2 * kv;
      o.u = ((in.u0 + bw * in.v0) + b2 * vn2) + b2 * vn3;
      o.un = in.u0 + aw * vn2;
      o.ku = vn3;
    } else if (kind == 6) {
      const T vn3 = in.ku, vn4 = in.v0 + a4 * kv;
      o.v = in.v + b2 * kv;
      o.u0 = in.u + bw * vn4;
      o.un = in.u0 + a4 * vn3;
      o.ku = vn4;
    } else {
      o.v0 = in.v + bw * kv;
    }
    return o;
  }
  if (kind == 2) {  // FIRST: u == u0, v == v0, ku == v0
    o.u = in.u0 + bw * in.v0;
    o.v = in.v0 + bw * kv;
    o.un = in.u0 + aw * in.v0;
    o.ku = in.v0 + aw * kv;
  } else if (kind == 3) {  // LAST
    o.u0 = in.u + bw * in.ku;
    o.v0 = in.v + bw * kv;
  } else {
    o.u = in.u + bw * in.ku;
    o.v = in.v + bw * kv;
    const T u0i = kind == 1 ? o.u : in.u0, v0i = kind == 1 ? o.v : in.v0;
    o.u0 = u0i;
    o.v0 = v0i;
    o.un = u0i + aw * in.ku;
    o.ku = v0i + aw * kv;
  }
  return o;
}

// ---- the Westervelt pass (rk4_stage_nl2_kernel): the lumped mass and one source term depend on the stage's inputs (u_n, v_n).
// A DESCRIPTION NO KERNEL CALLS YET: rk4_stage_nl2_kernel and rk4_stage_nl_kernel state the same kinds inline (westervelt.hpp says
// why).  Everything from here to the end of the namespace is used by tests/host/rk4_table_check.cpp alone, which checks it against the
// reference's sequence and the touch counts the roofline uses; what ties the kernels to the same statement is
// test_rk4_stage_kinds_equal_the_numpy_table (numpy, every kind, on the GPU).  A change to the Westervelt stage scheme has to be
// made in westervelt.hpp AND here.
// Are the stage's inputs the step's start (u0, v0) -- the FIRST kinds -- or the (un, ku) the pass before wrote?
FUS_RK4_TABLE_FN constexpr bool rk4_stage_inputs_are_start(int kind) { return kind == 2 || kind == 4; }
// kv = (b + M(c5) v_n^2) / (m0 + M(c2) u_n) with the two mass operators as their diagonals w5, w2 (westervelt.hpp)
template <typename T>
FUS_RK4_TABLE_FN T rk4_westervelt_kv(T b, T w5, T m0, T w2, T un, T vn) {
  return (b + w5 * vn * vn) / (m0 + w2 * un);
}
// The inputs (u_n', v_n') of the NEXT stage, for the optional output w = u_n' + kappa v_n': what this pass wrote to (un, ku); after a
// LAST pass the new (u0, v0); after LAST' the u0 that pass 3 wrote (read back: this pass does not have it) and the new v0.
enum Rk4Next { kRk4NextStage, kRk4NextStart, kRk4NextKeptU0 };
FUS_RK4_TABLE_FN constexpr Rk4Next rk4_next_inputs(int kind) { return kind == 3 ? kRk4NextStart : kind == 7 ? kRk4NextKeptU0 : kRk4NextStage; }
template <typename T>
FUS_RK4_TABLE_FN T rk4_next_combined(int kind, T kappa, const Rk4In<T>& in, const Rk4Out<T>& o) {
  const Rk4Next nx = rk4_next_inputs(kind);
  const T un_new = nx == kRk4NextStage ? o.un : nx == kRk4NextStart ? o.u0 : in.u0;
  const T vn_new = nx == kRk4NextStage ? o.ku : o.v0;
  return un_new + kappa * vn_new;
}
// rk4_access plus what the pass reads for its kv -- un wherever the inputs are (un, ku), and then ku too (LAST' alone does not
// read it otherwise) -- and for w: u0 alone where the next inputs keep it
struct Rk4WesterveltAccess : Rk4Access {
  bool rd_un, rd_u0, wr_w;
};
FUS_RK4_TABLE_FN constexpr Rk4WesterveltAccess rk4_westervelt_access(int kind, bool with_w) {
  const bool chained = !rk4_stage_inputs_are_start(kind);
  Rk4WesterveltAccess a{rk4_access(kind), chained, false, with_w};
  a.rd_ku = a.rd_ku || chained;
  a.rd_u0 = with_w && rk4_next_inputs(kind) == kRk4NextKeptU0 && !a.rd_0;
  return a;
}
// b read + zeroed, m0 w2 w5, the flags
FUS_RK4_TABLE_FN constexpr int rk4_westervelt_touches(int kind, bool with_w) {
  const Rk4WesterveltAccess a = rk4_westervelt_access(kind, with_w);
  return rk4_touches(a, 3) + a.rd_un + a.rd_u0 + a.wr_w;
}

}  // namespace fus

#undef FUS_RK4_TABLE_FN
