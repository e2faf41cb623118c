// The host-side shape of a streaming (elementwise) launch, free of HIP (any C++17 host compiler, like halo_layout.hpp;
// tests/host/stream_shape_check.cpp checks it without a GPU): which access flavour (vector_stream), whether every operand allows
// 16-byte accesses (aligned16), how many workgroups (stream_blocks), which pieces (for_each_piece), and the step from these runtime
// values to template arguments (shape_dispatch).  A launcher is its argument checks, these, and one generic lambda with its launch.
#pragma once

#include <stdint.h>

#include <initializer_list>
#include <type_traits>

namespace fus {

// Streaming accesses.  A vector kernel on operands far larger than the caches re-reads nothing it touches, and -- what
// matters -- every line it WRITES with a plain store stays dirty in the 256 MB memory-side Infinity Cache and is written
// back while the NEXT kernel runs: the headline apply takes 219-222 us after nothing / a busy wait / a 1 GiB read-only
// stream, 287 us after a 1 GiB fill, 263 us after a 1 GiB copy, 251-272 us after the RK4 vector pass
// (tools/interleave_probe.py, profiles/r04i_interleave_probe.log).  Non-temporal stores go to memory without lingering.
// Loads too: most of these kernels update in place (u += ..., y += w x), and a non-temporal store to a line the kernel's own
// plain load has just brought into the cache hits there and leaves it dirty all the same -- fused RK4 step on one box: cached
// 1.621 ms, non-temporal stores only 1.569, loads and stores 1.484 (profiles/r04k_ab_vector_stream_policy.log).
// Kernel template parameter NT: 0 cached accesses, 1 non-temporal loads AND stores, 2 non-temporal stores only.
// mode (fus_set_tuning FUS_TUNE_VECTOR_STREAM): 0 never; 1 auto = loads and stores for operands > kStreamBytes (default);
// 2 always loads and stores; 3 auto, stores only; 4 always, stores only
constexpr int64_t kStreamBytes = 24ll << 20;
inline int& vector_stream_mode() {
  static int m = 1;
  return m;
}
inline int vector_stream(int64_t operand_bytes) {
  const int m = vector_stream_mode();
  const bool on = m == 2 || m == 4 || ((m == 1 || m == 3) && operand_bytes > kStreamBytes);
  return !on ? 0 : (m >= 3 ? 2 : 1);
}

// Most workgroups (of 256 threads) of a grid-strided streaming launch: 8 per CU of the 256 CUs, a full complement of waves
// (vecops.hpp, field_monitor.hpp, bioheat.hpp).  The fused RK4 stages (rk4.hpp, westervelt.hpp) take twice that; neither
// docs/history.md nor a log under profiles/ records a measurement of one cap against the other, so each kernel keeps the one it
// was tuned and benchmarked with.
constexpr int64_t kStreamGridCap = 2048, kStageGridCap = 4096;

// do all of these pointers allow 16-byte accesses?  A null pointer (an operand that is switched off) does not count.
inline bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15u) == 0;
}

// workgroups of 256 threads for ``len`` elements, ``width`` per thread, grid-strided above ``cap``
inline unsigned stream_blocks(int64_t len, int width, int64_t cap) {
  const int64_t nblocks = ((len + width - 1) / width + 255) / 256;
  return (unsigned)(nblocks < cap ? nblocks : cap);
}

// Most dofs of one launch of a kernel that forms 32-bit byte offsets (vecops.hpp ld_chunk).  A multiple of every access width:
// the pieces keep the alignment of the whole.
constexpr int64_t kLaunchDofs = 1ll << 27;
// f(at, len) for [0, n) in pieces of at most ``piece``
template <typename F>
inline void for_each_piece(int64_t n, int64_t piece, F&& f) {
  for (int64_t at = 0; at < n; at += piece) f(at, n - at < piece ? n - at : piece);
}
// an optional operand of the piece at ``at``: null stays null
template <typename P>
inline P* piece_of(P* p, int64_t at) {
  return p ? p + at : p;
}

// The switches from a runtime value to code compiled per value (as degree_dispatch, fus_dispatch.hpp): f is a generic lambda that
// reads its tag as decltype(t)::value.  nt: vector_stream's 0 | 1 | 2, anything else the cached build.  aligned: W dofs per thread
// (one 16-byte access per array) or the scalar kernel.
template <typename F>
inline void nt_dispatch(int nt, F&& f) {
  if (nt == 1)
    f(std::integral_constant<int, 1>{});
  else if (nt == 2)
    f(std::integral_constant<int, 2>{});
  else
    f(std::integral_constant<int, 0>{});
}
template <int W, typename F>
inline void width_dispatch(bool aligned, F&& f) {
  if (aligned)
    f(std::integral_constant<int, W>{});
  else
    f(std::integral_constant<int, 1>{});
}
// a yes / no that a kernel is compiled for (bioheat's LAST, the gather's DENSE): std::true_type or std::false_type
template <typename F>
inline void flag_dispatch(bool on, F&& f) {
  if (on)
    f(std::true_type{});
  else
    f(std::false_type{});
}
// width and nt: f(width tag, nt tag)
template <int W, typename F>
inline void shape_dispatch(bool aligned, int nt, F&& f) {
  width_dispatch<W>(aligned, [&](auto w) { nt_dispatch(nt, [&](auto t) { f(w, t); }); });
}

}  // namespace fus
