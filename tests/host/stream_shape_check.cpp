// Stand-alone check of csrc/stream_shape.hpp (host-only: any C++17 compiler, no HIP, no GPU): the streaming policy, the alignment
// rule, the grid rule, the pieces of a launch and the tag dispatchers, against literals worked out from the formulas the launchers
// carried before they shared this header.  tests/test_stream_shape_host.py builds and runs it; it is also the program to build with
// -fsanitize=address,undefined.  Prints STREAM_SHAPE_OK and exits 0.
#include "../../fenicsx-fus-gpu_amd/csrc/stream_shape.hpp"

#include <cstdio>
#include <utility>
#include <vector>

using namespace fus;

static int failures = 0;
#define CHECK(cond) \
  if (!(cond)) std::printf("FAILED line %d: %s\n", __LINE__, #cond), ++failures

// ---------------------------------------------------------------------------------------------- vector_stream
static void policy() {
  CHECK(kStreamBytes == 25165824);  // 24 MiB
  CHECK(vector_stream_mode() == 1);  // the default: auto, loads and stores
  // mode: 0 never; 1 auto, loads and stores; 2 always, loads and stores; 3 auto, stores only; 4 always, stores only
  const int at_limit[5] = {0, 0, 1, 0, 2};  // exactly 24 MiB: the auto modes are off
  const int above[5] = {0, 1, 1, 2, 2};     // one byte more
  for (int m = 0; m < 5; ++m) {
    vector_stream_mode() = m;
    CHECK(vector_stream(25165824) == at_limit[m]);
    CHECK(vector_stream(25165825) == above[m]);
    CHECK(vector_stream(0) == (m == 2 ? 1 : m == 4 ? 2 : 0));
  }
  vector_stream_mode() = 1;
}

// ---------------------------------------------------------------------------------------------- aligned16
static void alignment() {
  alignas(16) static char buf[64];
  const void* none = nullptr;
  CHECK(aligned16({}));
  CHECK(aligned16({none, none, none}));  // every operand switched off
  CHECK(aligned16({buf, buf + 16, buf + 48}));
  CHECK(!aligned16({buf, buf + 8, buf + 32}));  // one pointer at + 8
  CHECK(!aligned16({buf + 4}));
  CHECK(aligned16({buf, none, buf + 32}));  // a null pointer among aligned ones does not count
  CHECK(!aligned16({none, buf + 8}));
}

// ---------------------------------------------------------------------------------------------- stream_blocks
static void grid() {
  CHECK(kStreamGridCap == 2048 && kStageGridCap == 4096);
  // work = aligned ? ceil(n / W) : n;  blocks = min(cap, ceil(work / 256))
  CHECK(stream_blocks(1000, 2, 2048) == 2);  // fp64 aligned: 500 threads
  CHECK(stream_blocks(1000, 1, 2048) == 4);  // fp64 unaligned: 1000 threads
  CHECK(stream_blocks(513, 4, 2048) == 1);   // fp32 aligned: 129 chunks
  CHECK(stream_blocks(513, 2, 2048) == 2);   // LAST of an fp32 bioheat field, 2 dofs per thread: 257 threads
  CHECK(stream_blocks(1, 1, 2048) == 1 && stream_blocks(1, 2, 2048) == 1 && stream_blocks(1, 4, 4096) == 1);
  CHECK(stream_blocks(512, 2, 2048) == 1 && stream_blocks(514, 2, 2048) == 2);  // 256 threads, 257 threads
  CHECK(stream_blocks(10218313, 2, 4096) == 4096);  // config 3: 5 109 157 threads = 19 958 blocks uncapped
  CHECK(stream_blocks(10218313, 2, 2048) == 2048);
  CHECK(stream_blocks(1048576, 2, 2048) == 2048);  // 524 288 threads: exactly the cap
  CHECK(stream_blocks(1048576, 2, 4096) == 2048);
  CHECK(stream_blocks(1048064, 2, 2048) == 2047);  // 524 032 threads: one block below it
  CHECK(stream_blocks(1048066, 2, 2048) == 2048);  // 524 033 threads
  CHECK(stream_blocks(int64_t(1) << 27, 1, 4096) == 4096);
  CHECK(stream_blocks((int64_t(1) << 40) + 3, 1, 4096) == 4096);  // no 32-bit intermediate
}

// ---------------------------------------------------------------------------------------------- for_each_piece, piece_of
using Pieces = std::vector<std::pair<int64_t, int64_t>>;
static Pieces pieces(int64_t n, int64_t piece) {
  Pieces got;
  for_each_piece(n, piece, [&](int64_t at, int64_t len) { got.emplace_back(at, len); });
  return got;
}
static void splitting() {
  CHECK(pieces(0, 8).empty());
  CHECK(pieces(-3, 8).empty());
  CHECK((pieces(1, 8) == Pieces{{0, 1}}));
  CHECK((pieces(8, 8) == Pieces{{0, 8}}));
  CHECK((pieces(9, 8) == Pieces{{0, 8}, {8, 1}}));
  CHECK((pieces(21, 8) == Pieces{{0, 8}, {8, 8}, {16, 5}}));
  CHECK(kLaunchDofs == 134217728);  // 2^27 dofs: the byte offsets of a double array stay below 2^30
  CHECK(kLaunchDofs % 4 == 0);      // the pieces keep a 16-byte alignment for doubles and floats
  CHECK((pieces(134217728, kLaunchDofs) == Pieces{{0, 134217728}}));
  CHECK((pieces(134217733, kLaunchDofs) == Pieces{{0, 134217728}, {134217728, 5}}));
  double field[32];
  double* off = nullptr;
  CHECK(piece_of(field, 8) == field + 8 && piece_of(field, 0) == field);
  CHECK(piece_of(off, 8) == nullptr);  // an operand that is switched off stays off in every piece
}

// ---------------------------------------------------------------------------------------------- the tag dispatchers
static void dispatch() {
  for (int nt = -2; nt <= 9; ++nt) {
    int got = -1, calls = 0;
    nt_dispatch(nt, [&](auto t) { got = decltype(t)::value, ++calls; });
    CHECK(calls == 1 && got == (nt == 1 ? 1 : nt == 2 ? 2 : 0));  // outside 0..2: the cached build
  }
  for (int aligned = 0; aligned < 2; ++aligned) {
    int got = -1, calls = 0;
    width_dispatch<4>(aligned != 0, [&](auto w) { got = decltype(w)::value, ++calls; });
    CHECK(calls == 1 && got == (aligned ? 4 : 1));
    got = -1;
    width_dispatch<2>(aligned != 0, [&](auto w) { got = decltype(w)::value; });
    CHECK(got == (aligned ? 2 : 1));
    bool flag = !aligned;
    calls = 0;
    flag_dispatch(aligned != 0, [&](auto f) { flag = decltype(f)::value, ++calls; });
    CHECK(calls == 1 && flag == (aligned != 0));
    for (int nt = 0; nt < 4; ++nt) {
      int w_got = -1, nt_got = -1;
      calls = 0;
      shape_dispatch<4>(aligned != 0, nt, [&](auto w, auto t) { w_got = decltype(w)::value, nt_got = decltype(t)::value, ++calls; });
      CHECK(calls == 1 && w_got == (aligned ? 4 : 1) && nt_got == (nt == 3 ? 0 : nt));
    }
  }
}

int main() {
  policy();
  alignment();
  grid();
  splitting();
  dispatch();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("STREAM_SHAPE_OK\n");
  return 0;
}
