// The communicator behind fus_comm_*: its high-priority stream(s) and the event-free fork / join between a caller's
// stream and them.  Nothing here knows what a halo is; the transports (halo_rccl.hpp, halo_local.hpp, halo_peer.hpp)
// hang their state on it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "flag_wait.hpp"    // stream_flag_wait
#include "halo_layout.hpp"  // the status words
#include "plan.hpp"         // LaunchSignal

struct ncclComm;  // RCCL's, opaque (halo_rccl.hpp)

namespace fus {

struct Halo;
struct LocalWorld;

struct Comm {
  enum Kind { RCCL = 0, LOCAL = 1, PEER = 2 } kind = RCCL;
  int rank = 0, nranks = 1, device = 0;
  ncclComm* nccl = nullptr;
  std::shared_ptr<LocalWorld> world;
  hipStream_t stream = nullptr;   // high priority: small exchange kernels between big operator kernels
  hipStream_t stream2 = nullptr;  // PEER: the receive kernels' stream (sends never queue behind a waiting receive)
  std::vector<Halo*> halos;       // the live halo objects: the communicator outlives them (comm_health)
  // event-free fork / join between a caller's stream and ``stream`` (comm_fork_join below)
  uint64_t* sync_words = nullptr;  // device: [0] fork flag, [1] join flag, [2..] status (ST_TIMEOUTS, ST_DEAD)
  uint64_t sync_seq[2] = {0, 0};
  uint64_t sync_budget = 0;
  // One sequence flag per direction: consecutive forks / joins of a communicator must come from ONE caller stream (two
  // streams forking alternately would let the later stream's signal satisfy the earlier wait).  Enforced: a fork from
  // another stream is accepted only when the communicator's stream has drained.
  hipStream_t caller_stream = nullptr;
  bool caller_stream_set = false;
  // PEER: fork / join folded into the exchange kernels (fus_comm_fork_lazy / fus_comm_arm_join)
  uint64_t gate_pending = 0;      // fork sequence number no kernel of the communicator's stream waits for yet
  bool join_armed = false;        // the last receive kernel of the next begin / begin_group publishes the join flag
  Halo* join_halo = nullptr;      // ... that is this halo's, in direction join_dir
  int join_dir = 0;
  uint64_t join_inflight = 0;     // join sequence number a posted receive kernel will publish
  std::string last_error;
};

// ``return -1`` with the communicator's last_error set, for the int-returning host functions of the halo layer
#define FUS_H(c_, e_)                                                                                \
  do {                                                                                               \
    if (hipError_t _e = (e_); _e != hipSuccess) return (c_)->last_error = hipGetErrorString(_e), -1; \
  } while (0)

// what a device-side wait may spin before it gives up, in ticks of the device's wall clock (FUS_IPC_SPIN_SECONDS, default 20 s)
inline uint64_t spin_budget_ticks(int device) {
  int khz = 100000;
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device);
  double seconds = 20.0;
  if (const char* v = std::getenv("FUS_IPC_SPIN_SECONDS")) seconds = std::atof(v) > 0 ? std::atof(v) : seconds;
  return (uint64_t)(seconds * 1e3 * khz);
}

inline hipError_t comm_make_stream(Comm* c) {
  int lo = 0, hi = 0;
  hipError_t e = hipGetDevice(&c->device);
  if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi = numerically lowest = highest priority
  if (e != hipSuccess) return e;
  if (const char* pr = std::getenv("FUS_COMM_PRIORITY")) {  // experiments: "normal" / "low" instead of the highest
    if (!std::strcmp(pr, "normal")) hi = 0;
    if (!std::strcmp(pr, "low")) hi = lo;
  }
  e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi);
  if (e == hipSuccess && c->kind == Comm::PEER) {
    // One stream by default: send, receive and -- when the host puts them there (fus_comm_stream) -- the boundary-cell
    // kernels between a forward and a reverse exchange follow each other in stream order, with no event edge between
    // them.  FUS_IPC_TWO_STREAMS=1: receive kernels on a stream of their own.
    const char* two = std::getenv("FUS_IPC_TWO_STREAMS");
    if (two && two[0] == '1')
      e = hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, hi);
    else
      c->stream2 = c->stream;
  }
  return e;
}

// (called at creation too: the first fork of a time loop must not synchronise the device)
inline hipError_t comm_sync_init(Comm* c) {
  if (c->sync_words) return hipSuccess;
  hipError_t e = hipMalloc(&c->sync_words, (2 + ST_WORDS) * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemset(c->sync_words, 0, (2 + ST_WORDS) * sizeof(uint64_t));
  c->sync_budget = spin_budget_ticks(c->device);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

// ------------------------------------------------------------------------------------ fork / join without events
// Ordering a side stream after the caller's stream with an event costs the caller's stream 7 us per fork next to
// chip-filling launches (the record is a marker with a cache write-back between the caller's kernels), the join
// another 3-4 us (profiles/r03g_forkjoin.log).  A one-thread kernel in the caller's stream costs 2.4 us.  So:
//   fork   caller's stream: signal kernel (flag = seq: runs when everything before it in that stream has completed);
//          communicator's stream: a one-wave kernel that waits (bounded) for flag >= seq -- what follows it in that
//          stream starts after it, by stream order;
//   join   the same with the roles exchanged.
// Data written before the signal kernel is visible after the wait kernel for the reason two consecutive kernels of one
// stream see each other's data: every kernel ends with a release and starts with an acquire at device scope.
__global__ void stream_signal_kernel(uint64_t* flag, uint64_t seq) {
  __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void stream_wait_kernel(const uint64_t* flag, uint64_t seq, uint64_t* status, uint64_t budget) {
  if (threadIdx.x == 0) stream_flag_wait(flag, seq, status, budget);
}

// ``stream`` waits (bounded) until flag ``which`` (0 fork, 1 join) of the communicator has reached ``seq``
inline hipError_t comm_launch_wait(Comm* c, hipStream_t stream, int which, uint64_t seq) {
  hipLaunchKernelGGL(stream_wait_kernel, dim3(1), dim3(64), 0, stream, c->sync_words + which, seq, c->sync_words + 2, c->sync_budget);
  return hipGetLastError();
}

// the wait of a lazily posted fork that no send kernel took over: a wait kernel on the communicator's stream after all
inline hipError_t comm_flush_gate(Comm* c) {
  if (!c->gate_pending) return hipSuccess;
  return comm_launch_wait(c, c->stream, 0, std::exchange(c->gate_pending, 0));
}

// a fork signal that was attached to "the next planned operator launch" and has not been carried by one: publish it with
// a signal kernel after all (no launch came: an empty cell range, a plan-free kernel)
inline hipError_t comm_flush_attached(Comm* c) {
  if (!c->sync_words) return hipSuccess;
  hipStream_t st = nullptr;
  const LaunchSignal s = take_launch_signal_of(c->sync_words + 0, &st);
  if (!s.flag) return hipSuccess;
  hipLaunchKernelGGL(stream_signal_kernel, dim3(1), dim3(1), 0, st, s.flag, s.seq);
  return hipGetLastError();
}

// which: 0 fork (``stream`` -> communicator's stream), 1 join (communicator's stream -> ``stream``)
// lazy (fork, PEER): no wait kernel; the first send kernel of the next exchange posted on the communicator's stream waits for
// the flag itself (halo_peer.hpp halo_ipc_post) -- one kernel less in the exchange chain.
// attach (fork): no signal kernel; the NEXT PLANNED OPERATOR LAUNCH on ``stream`` publishes the flag when its first workgroup
// starts (plan.hpp LaunchSignal) -- 2.4 us less on the caller's stream.  Flushed by the next fork / join if no launch came.
// *misuse: the single-caller-stream contract was violated (nothing was launched; last_error says what).
inline hipError_t comm_fork_join(Comm* c, hipStream_t stream, int which, bool lazy, bool* misuse, bool attach = false) {
  *misuse = false;
  if (stream == c->stream) return hipSuccess;
  hipError_t e = comm_sync_init(c);
  if (e != hipSuccess) return e;
  if (c->caller_stream_set && stream != c->caller_stream) {
    // another caller stream: fine once everything forked so far has run (no wait kernel is pending on either side)
    if (which == 1 || hipStreamQuery(c->stream) != hipSuccess) {
      (void)hipGetLastError();
      c->last_error = which == 1 ? "fus_comm_join: called with a different stream than the fus_comm_fork before it"
                                 : "fus_comm_fork: consecutive forks of a communicator must come from one caller stream (the communicator's stream "
                                   "still has work forked from another stream; synchronise it before changing the caller stream)";
      *misuse = true;
      return hipSuccess;
    }
  }
  if (which == 0) {
    c->caller_stream = stream;
    c->caller_stream_set = true;
  }
  e = comm_flush_attached(c);
  if (e == hipSuccess) e = comm_flush_gate(c);
  if (e != hipSuccess) return e;
  // a receive kernel already on the communicator's stream publishes the flag
  if (which == 1 && c->join_inflight) return comm_launch_wait(c, stream, 1, std::exchange(c->join_inflight, 0));
  if (which == 1) {
    c->join_armed = false;  // armed, but no receive kernel took it (no neighbours on that side)
    c->join_halo = nullptr;
  }
  const uint64_t seq = ++c->sync_seq[which];
  hipStream_t from = which == 0 ? stream : c->stream, to = which == 0 ? c->stream : stream;
  if (which == 0 && attach) {
    const LaunchSignal old = post_launch_signal(stream, c->sync_words + 0, seq);
    if (old.flag) hipLaunchKernelGGL(stream_signal_kernel, dim3(1), dim3(1), 0, stream, old.flag, old.seq);  // another communicator's
  } else {
    hipLaunchKernelGGL(stream_signal_kernel, dim3(1), dim3(1), 0, from, c->sync_words + which, seq);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (which == 0 && lazy && c->kind == Comm::PEER && c->stream2 == c->stream) {
    c->gate_pending = seq;
    return hipSuccess;
  }
  return comm_launch_wait(c, to, which, seq);
}

// PEER: the last receive kernel of the NEXT fus_halo_*_begin / *_begin_group of this communicator also publishes the join
// flag, so that the fus_comm_join that follows launches only the wait kernel on the caller's stream.  That exchange must be
// the last thing enqueued on the communicator's stream before the join.  Without a receive kernel to carry it (no
// neighbours on that side, receive kernels on a stream of their own) the join falls back to its signal kernel.
inline hipError_t comm_arm_join(Comm* c) {
  hipError_t e = comm_sync_init(c);
  if (e != hipSuccess) return e;
  if (c->kind == Comm::PEER && c->stream2 == c->stream) {
    c->join_armed = true;
    c->join_halo = nullptr;
  }
  return hipSuccess;
}

}  // namespace fus
