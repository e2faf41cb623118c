// Sweep direction of the general-G planned stiffness apply (knob FUS_TUNE_PLAN_SWEEP; the map: stiffness.hpp, mirror_block; the parity:
// plan_registry.hpp, flip_sweep; DESIGN 3.1, "sweep direction"): the rules, as pure host functions.  Host-only (no HIP include):
// tests/test_sweep_placement.py compiles them into a program of its own.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace fus_abi {

// knob values: -1 auto, 0 always upwards, 1 alternate on every launch of a plan, 2 always downwards
inline bool plan_sweep_valid(int v) { return v >= -1 && v <= 2; }

// the knob's value at load: the environment variable FUS_TUNE_PLAN_SWEEP if it holds a valid value, else auto
inline int plan_sweep_initial() {
  const char* v = std::getenv("FUS_TUNE_PLAN_SWEEP");
  if (!v || !*v) return -1;
  char* end = nullptr;
  const long k = std::strtol(v, &end, 10);
  return (*end == '\0' && k >= -1 && k <= 2) ? (int)k : -1;
}

// Algorithmic HBM bytes per cell of the general-G apply (benchlib/roofline.py: stiffness_bytes_per_cell):
// G + dofmap + x once + y read-modify-write + the cell constant.  P = 4 fp64: 8044.
inline int64_t stiffness_bytes_per_cell(int P, int elem_bytes) {
  const int64_t nd = (int64_t)(P + 1) * (P + 1) * (P + 1), p3 = (int64_t)P * P * P, T = elem_bytes;
  return 6 * nd * T + 4 * nd + T * p3 + 2 * T * p3 + T;
}

// the memory-side cache of the MI355X (Infinity Cache)
constexpr int64_t kMemorySideCacheBytes = int64_t(256) << 20;

// A launch whose algorithmic bytes fit the memory-side cache finds everything resident in either direction.
inline bool plan_sweep_exceeds_cache(int P, int elem_bytes, int64_t ncell) {
  return stiffness_bytes_per_cell(P, elem_bytes) * ncell > kMemorySideCacheBytes;
}

// What auto does with a launch that exceeds the cache: alternate (true) or stay upwards.  One rule for all degrees and types.
constexpr bool kPlanSweepAutoAlternates = true;

// Does this launch take its direction from the plan's parity (and flip it)?  knob 1: always; auto: by the byte rule.
inline bool plan_sweep_alternates(int knob, int P, int elem_bytes, int64_t ncell) {
  return knob == 1 || (knob < 0 && kPlanSweepAutoAlternates && plan_sweep_exceeds_cache(P, elem_bytes, ncell));
}

}  // namespace fus_abi
