// Stand-alone check of the sweep parity of csrc/plan_registry.hpp (flip_sweep) and of the rules of csrc/plan_sweep.hpp (host-only: any
// C++17 compiler, no HIP).  tests/test_sweep_placement.py builds and runs it; it is also the program to build with
// -fsanitize=address,undefined or -fsanitize=thread.  Prints PLAN_SWEEP_OK and exits 0.
#include "../../fenicsx-fus-gpu_amd/csrc/plan_registry.hpp"
#include "../../fenicsx-fus-gpu_amd/csrc/plan_sweep.hpp"

#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

using fus_abi::GatherStaticInfo;
using fus_abi::PlanInfo;

struct Gather {  // stands in for fus::GatherHeader
  int64_t nent, N;
};
using Registry = fus_abi::PlanRegistry<Gather>;

static int failures = 0;
#define CHECK(cond) \
  if (!(cond)) std::printf("FAILED line %d: %s\n", __LINE__, #cond), ++failures

static const void* addr(uintptr_t a) { return reinterpret_cast<const void*>(a * 256); }

static void parity() {
  Registry r;
  CHECK(r.flip_sweep(addr(1)) == -1);  // nothing there
  PlanInfo in;
  in.N = 125, in.epb = 10, in.nent = 2744, in.nbatch = 275;
  r.put(addr(1), in);
  r.put(addr(2), in);
  // the value BEFORE the flip: 0, 1, 0, ...
  for (int i = 0; i < 6; ++i) CHECK(r.flip_sweep(addr(1)) == i % 2);
  // per workspace: the plan at another address has not moved
  CHECK(r.flip_sweep(addr(2)) == 0 && r.flip_sweep(addr(1)) == 0 && r.flip_sweep(addr(2)) == 1 && r.flip_sweep(addr(2)) == 0);
  CHECK(r.flip_sweep(addr(1)) == 1 && r.flip_sweep(addr(1)) == 0);
  // ... and the record is otherwise what was put; marking it exclusive keeps the parity
  PlanInfo p;
  CHECK(r.flip_sweep(addr(1)) == 1 && r.flip_sweep(addr(1)) == 0);  // the bit is set now: the next alternating launch walks downwards
  CHECK(r.mark_exclusive(addr(1)) && r.get(addr(1), &p) && p.exclusive && p.sweep_down && p.N == 125 && p.nbatch == 275);
  CHECK(r.flip_sweep(addr(1)) == 1);
  // a rebuild at the same address starts upwards again
  CHECK(r.flip_sweep(addr(1)) == 0);
  r.put(addr(1), in);
  CHECK(r.get(addr(1), &p) && !p.sweep_down && r.flip_sweep(addr(1)) == 0 && r.flip_sweep(addr(1)) == 1);
  // release forgets it; a new plan at the address starts upwards
  CHECK(r.flip_sweep(addr(1)) == 0);
  r.release(addr(1));
  CHECK(r.flip_sweep(addr(1)) == -1);
  r.put(addr(1), in);
  CHECK(r.flip_sweep(addr(1)) == 0);
  // the other kinds of record have no parity
  r.put(addr(3), Gather{7, 8});
  r.put(addr(4), GatherStaticInfo{addr(3), 8});
  CHECK(r.flip_sweep(addr(3)) == -1 && r.flip_sweep(addr(4)) == -1);
  r.put(addr(2), Gather{1, 1});  // a batch plan replaced by another kind
  CHECK(r.flip_sweep(addr(2)) == -1);
}

// Threads on their own plans each see 0, 1, 0, ...; on one shared plan the flips are a total order: as many 0s as 1s come back.
static void threads() {
  Registry r;
  constexpr int kThreads = 8, kRounds = 2000;
  r.put(addr(50), PlanInfo{});
  std::atomic<int> bad{0}, ones{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < kThreads; ++t)
    pool.emplace_back([&r, &bad, &ones, t] {
      const void* own = addr(100 + t);
      r.put(own, PlanInfo{});
      for (int i = 0; i < kRounds; ++i) {
        if (r.flip_sweep(own) != i % 2) ++bad;
        const int v = r.flip_sweep(addr(50));
        if (v != 0 && v != 1) ++bad;
        ones += v;
      }
      r.release(own);
    });
  for (auto& th : pool) th.join();
  CHECK(bad.load() == 0 && ones.load() == kThreads * kRounds / 2);
}

static void rules() {
  using namespace fus_abi;
  for (int v : {-1, 0, 1, 2}) CHECK(plan_sweep_valid(v));
  for (int v : {-2, 3, 4, 16, 65536, -65536}) CHECK(!plan_sweep_valid(v));
  // the bytes of benchlib/roofline.py: P = 4 fp64 8044 per cell, config 3 (54^3 cells) 1 266 640 416 per launch
  CHECK(stiffness_bytes_per_cell(4, 8) == 8044 && stiffness_bytes_per_cell(4, 8) * 157464 == 1266640416LL);
  CHECK(stiffness_bytes_per_cell(2, 4) == 6 * 27 * 4 + 4 * 27 + 3 * 4 * 8 + 4);
  CHECK(kMemorySideCacheBytes == 268435456LL);
  // the threshold at P = 4 fp64: 268435456 / 8044 = 33370.9...
  CHECK(!plan_sweep_exceeds_cache(4, 8, 33370) && plan_sweep_exceeds_cache(4, 8, 33371));
  CHECK(!plan_sweep_exceeds_cache(4, 8, 27000) && plan_sweep_exceeds_cache(4, 8, 157464));  // 30^3: 217 MB, resident; config 3
  CHECK(stiffness_bytes_per_cell(10, 8) == 93220 && !plan_sweep_exceeds_cache(10, 8, 2879) && plan_sweep_exceeds_cache(10, 8, 2880));
  // which launches take their direction from the parity: knob 1 all, knob 0 / 2 none, auto by the byte rule (if auto alternates at all)
  for (int64_t ncell : {int64_t(1), int64_t(2744), int64_t(157464)}) {
    CHECK(plan_sweep_alternates(1, 4, 8, ncell) && !plan_sweep_alternates(0, 4, 8, ncell) && !plan_sweep_alternates(2, 4, 8, ncell));
    CHECK(plan_sweep_alternates(-1, 4, 8, ncell) == (kPlanSweepAutoAlternates && ncell > 33370));
  }
}

int main() {
  parity();
  threads();
  rules();
  if (failures) return 1;
  std::printf("PLAN_SWEEP_OK\n");
  return 0;
}
