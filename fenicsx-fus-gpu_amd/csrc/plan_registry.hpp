// Host mirror of what was built through this library in caller-owned workspaces, keyed by workspace address: ONE map, ONE mutex.  An entry
// point looks the record of ITS kind up before any kernel indexes the workspace (a workspace that holds something else would be gathered /
// scattered out of bounds).  A build REPLACES whatever kind was registered at its address.  Host-only (no HIP include): the record of the
// transposed gather plan is a template parameter, because fus::GatherHeader lives with its kernels in mass_gather.hpp; the library's one
// instance is in fus_gpu.hip, tests/host/plan_registry_check.cpp exercises this header alone.
#pragma once
#include <cstdint>
#include <iterator>
#include <mutex>
#include <unordered_map>
#include <variant>

namespace fus_abi {

// batch plan (fus_plan_build*): the shape it was built for, whether it carries a cell order, and its list encodings
struct PlanInfo {
  int N = 0, epb = 0;
  int64_t nent = 0;
  bool ordered = false;
  bool exclusive = false;  // fus_plan_mark_exclusive has run: the plan carries exclusive-dof marks
  bool runs_pay = true;    // at least half of the batches carry a run table (plan_use_runs)
  int64_t nbatch = 0, with_runs = 0;
  bool rows_consecutive = false;  // the header's word: every local row of every cell is consecutive dof numbers (plan.hpp: rowbase)
  int run_stride = 0;             // runs per batch of the compact copy of the run tables (plan.hpp: runs_c); 0: the plan has none
  bool sweep_down = false;        // the next alternating general-G apply on this plan walks its batches downwards (flip_sweep)
};

// static companion of a transposed gather plan (detJ in row order), keyed by its own workspace address
struct GatherStaticInfo {
  const void* plan;
  int elem_bytes;
};

template <typename Gather>
class PlanRegistry {
 public:
  // registers ``r`` at ``ws``; a record of any kind that was there is gone
  template <typename R>
  void put(const void* ws, const R& r) {
    std::lock_guard<std::mutex> lk(mu_);
    map_.insert_or_assign(ws, Record{r});
  }
  // copies the record of kind R at ``ws`` out; false if there is none or it is of another kind
  template <typename R>
  bool get(const void* ws, R* out) const {
    std::lock_guard<std::mutex> lk(mu_);
    const auto it = map_.find(ws);
    const R* r = it == map_.end() ? nullptr : std::get_if<R>(&it->second);
    if (r) *out = *r;
    return r != nullptr;
  }
  // sets the exclusive mark of the batch plan at ``ws``; false if there is none
  bool mark_exclusive(const void* ws) {
    std::lock_guard<std::mutex> lk(mu_);
    const auto it = map_.find(ws);
    PlanInfo* p = it == map_.end() ? nullptr : std::get_if<PlanInfo>(&it->second);
    if (p) p->exclusive = true;
    return p != nullptr;
  }
  // flips the sweep direction of the batch plan at ``ws`` and returns the one from BEFORE the flip (0 upwards, 1 downwards: 0, 1, 0, ...
  // per workspace; a build at the address starts at 0 again); -1 if there is no batch plan
  int flip_sweep(const void* ws) {
    std::lock_guard<std::mutex> lk(mu_);
    const auto it = map_.find(ws);
    PlanInfo* p = it == map_.end() ? nullptr : std::get_if<PlanInfo>(&it->second);
    if (!p) return -1;
    const bool was = p->sweep_down;
    p->sweep_down = !was;
    return was ? 1 : 0;
  }
  // forgets ``ws`` and every static companion of the plan at ``ws``; an unknown address is no error
  void release(const void* ws) {
    std::lock_guard<std::mutex> lk(mu_);
    map_.erase(ws);
    for (auto it = map_.begin(); it != map_.end();) {
      const GatherStaticInfo* s = std::get_if<GatherStaticInfo>(&it->second);
      it = (s && s->plan == ws) ? map_.erase(it) : std::next(it);
    }
  }

 private:
  using Record = std::variant<PlanInfo, Gather, GatherStaticInfo>;
  mutable std::mutex mu_;
  std::unordered_map<const void*, Record> map_;
};

}  // namespace fus_abi
