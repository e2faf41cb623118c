// Stand-alone check of csrc/plan_registry.hpp (host-only: any C++17 compiler, no HIP).  tests/test_plan_registry.py builds and runs it;
// it is also the program to build with -fsanitize=address,undefined or -fsanitize=thread.  Prints PLAN_REGISTRY_OK and exits 0.
#include "../../fenicsx-fus-gpu_amd/csrc/plan_registry.hpp"

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

template <typename R>
static bool has(const Registry& r, const void* ws) {
  R out{};
  return r.get(ws, &out);
}

static void each_kind() {
  Registry r;
  PlanInfo p;
  Gather g{};
  GatherStaticInfo s{};
  CHECK(!r.get(addr(1), &p) && !r.get(addr(1), &g) && !r.get(addr(1), &s));
  PlanInfo in;
  in.N = 27, in.epb = 8, in.nent = 5, in.ordered = true, in.nbatch = 1;
  r.put(addr(1), in);
  r.put(addr(2), Gather{7, 8});
  r.put(addr(3), GatherStaticInfo{addr(2), 8});
  CHECK(r.get(addr(1), &p) && p.N == 27 && p.epb == 8 && p.nent == 5 && p.ordered && !p.exclusive && p.nbatch == 1);
  CHECK(r.get(addr(2), &g) && g.nent == 7 && g.N == 8);
  CHECK(r.get(addr(3), &s) && s.plan == addr(2) && s.elem_bytes == 8);
  // a record answers to its own kind only, and a failed look-up leaves ``out`` alone
  p.N = -1;
  CHECK(!r.get(addr(2), &p) && p.N == -1 && !has<Gather>(r, addr(1)) && !has<GatherStaticInfo>(r, addr(1)) && !has<PlanInfo>(r, addr(3)));
  CHECK(r.mark_exclusive(addr(1)) && r.get(addr(1), &p) && p.exclusive && p.N == 27);
  CHECK(!r.mark_exclusive(addr(2)) && !r.mark_exclusive(addr(9)));
  r.release(addr(1));
  CHECK(!has<PlanInfo>(r, addr(1)) && has<Gather>(r, addr(2)) && has<GatherStaticInfo>(r, addr(3)));
  r.release(addr(3));  // a companion on its own: its plan stays
  CHECK(!has<GatherStaticInfo>(r, addr(3)) && has<Gather>(r, addr(2)));
  r.release(addr(2));
  CHECK(!has<Gather>(r, addr(2)));
  r.release(addr(2));  // twice, and an address never seen: no error
  r.release(addr(77));
}

static void replacement_and_companions() {
  Registry r;
  r.put(addr(1), PlanInfo{});
  r.put(addr(1), Gather{3, 4});  // kind B at the address of kind A: A is gone
  CHECK(!has<PlanInfo>(r, addr(1)) && has<Gather>(r, addr(1)) && !r.mark_exclusive(addr(1)));
  r.put(addr(2), GatherStaticInfo{addr(1), 4});
  r.put(addr(3), GatherStaticInfo{addr(1), 8});
  r.put(addr(4), Gather{1, 1});
  r.put(addr(5), GatherStaticInfo{addr(4), 8});
  r.put(addr(1), PlanInfo{});  // back to kind A: the gather plan is gone, its companions no longer find it
  CHECK(has<PlanInfo>(r, addr(1)) && !has<Gather>(r, addr(1)) && has<GatherStaticInfo>(r, addr(2)));
  r.release(addr(1));  // the companions of a released address go with it, those of another plan stay
  CHECK(!has<PlanInfo>(r, addr(1)) && !has<GatherStaticInfo>(r, addr(2)) && !has<GatherStaticInfo>(r, addr(3)));
  CHECK(has<Gather>(r, addr(4)) && has<GatherStaticInfo>(r, addr(5)));
  r.put(addr(5), PlanInfo{});  // a companion replaced by another kind
  r.release(addr(4));
  CHECK(has<PlanInfo>(r, addr(5)) && !has<Gather>(r, addr(4)));
}

// Threads on disjoint addresses see exactly their own records; on one shared address every look-up sees a whole record of one thread or
// none, never a mixture.
static void threads() {
  Registry r;
  constexpr int kThreads = 8, kRounds = 2000;
  std::atomic<int> bad{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < kThreads; ++t)
    pool.emplace_back([&r, &bad, t] {
      const void* own = addr(100 + t);
      const void* companion = addr(200 + t);
      const void* shared = addr(50);
      for (int i = 0; i < kRounds; ++i) {
        PlanInfo p;
        Gather g{};
        GatherStaticInfo s{};
        PlanInfo mine;
        mine.N = t, mine.epb = t, mine.nent = i;
        r.put(own, mine);
        if (!r.get(own, &p) || p.N != t || p.epb != t || p.nent != i || !r.mark_exclusive(own)) ++bad;
        r.put(own, Gather{i, t});
        r.put(companion, GatherStaticInfo{own, t});
        if (r.get(own, &p) || !r.get(own, &g) || g.nent != i || g.N != t || !r.get(companion, &s) || s.plan != own) ++bad;
        r.release(own);
        if (r.get(own, &g) || r.get(companion, &s)) ++bad;
        if (t % 2)
          r.put(shared, Gather{t, t});
        else
          r.put(shared, PlanInfo{t, t, t});
        if (r.get(shared, &g) && g.nent != g.N) ++bad;
        if (r.get(shared, &p) && (p.N != p.epb || p.N != p.nent)) ++bad;
        r.mark_exclusive(shared);
        if (i % 3 == 0) r.release(shared);
      }
    });
  for (auto& th : pool) th.join();
  CHECK(bad.load() == 0);
  r.release(addr(50));
  CHECK(!has<PlanInfo>(r, addr(50)) && !has<Gather>(r, addr(50)));
}

int main() {
  each_kind();
  replacement_and_companions();
  threads();
  if (failures) return 1;
  std::printf("PLAN_REGISTRY_OK\n");
  return 0;
}
