// The halo object behind fus_halo_*: the plan (halo_layout.hpp), its message buffers and events, the per-transport
// state, and the two stages the packed transports (RCCL, LOCAL) share: pack before the messages move, unpack after.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "comm_sync.hpp"
#include "halo.hpp"
#include "halo_layout.hpp"

namespace fus {

struct IpcRole {  // PEER: device tables of one kernel role (send or recv) over one side
  IpcChunk* chunks = nullptr;
  IpcPeer* peers = nullptr;
  unsigned* counters = nullptr;
  int nchunks = 0, nnbr = 0;
  std::vector<IpcPeer> host_peers;
};

struct IpcState : IpcArena {  // PEER: my arena (fine-grained device memory: flags, forward and reverse receive buffer) + what posts into it
  uint64_t* status = nullptr;  // ST_WORDS words, ordinary device memory
  bool connected = false;
  std::vector<void*> opened;  // peer arenas mapped with hipIpcOpenMemHandle
  IpcRole send_fwd, recv_fwd, send_rev, recv_rev;
  uint64_t seq[2] = {0, 0};
  // A receive kernel that waits occupies its hardware queue, and one process has only a few of them (4 by default) for
  // all its streams.  One process per rank: every rank's send precedes its receive, no cycle.  Several ranks in ONE
  // process (tests): rank A's waiting receive can sit in front of rank B's send in a shared queue.  There the receive
  // kernel is posted by *_end, under the in-process contract of the LOCAL transport (every rank's *_begin before any
  // rank's *_end), so it never waits for a send that has not been queued.
  bool defer_recv = false;
  uint64_t pending[2] = {0, 0};
  uint64_t budget = 0;
  hipEvent_t ev_sent = nullptr;
  bool sent_recorded = false, done_recorded = false;  // the events of the exchange in flight were recorded (caller not on the comm stream)
  unsigned* join_counter = nullptr;  // workgroups of a receive kernel that have finished (ipc_kernel_done)
  int memory_kind = 0;  // 0 fine-grained, 1 uncached, 2 ordinary
  int fenced = 0;       // FUS_IPC_FENCED=1 at creation: system-scope release / acquire around the flags (ipc_release_system)
};

struct Halo : HaloPlan {
  Comm* comm = nullptr;
  int eb = 8;  // element bytes
  char* buf_owner = nullptr;  // owners-side message buffer (forward: recv, reverse: send), owners.total elements
  char* buf_ghost = nullptr;  // ghosts-side message buffer (forward: send, reverse: recv), ghosts.total elements
  hipEvent_t ev_ready = nullptr, ev_done = nullptr;
  // LOCAL transport state
  int index = 0;                    // creation index within the rank (pairs halo objects across ranks)
  hipEvent_t ev_packed = nullptr;   // my message is complete in cur_send
  hipEvent_t ev_pulled = nullptr;   // my copies out of the peers' buffers have executed
  bool pulled_valid = false;
  const char* cur_send = nullptr;   // where my outgoing message lives for the exchange in flight
  int cur_dir = 0;                  // 0 forward, 1 reverse
  IpcState ipc;                     // PEER transport state
};

constexpr int kHaloGroupMax = 8;  // vectors of one begin_group: the ABI's bound, and the transports' per-group arrays

inline void side_free(Side& s) {
  if (s.idx_d) (void)hipFree(s.idx_d);
  s.idx_d = nullptr;
}

inline hipError_t side_init(Side& s, int nn, const int32_t* ranks, const int64_t* sizes, const int64_t* idx,
                            hipStream_t stream) {
  s.ranks.assign(ranks, ranks + nn);
  s.counts.assign(sizes, sizes + nn);
  s.offsets.assign(nn + 1, 0);
  for (int i = 0; i < nn; ++i) s.offsets[i + 1] = s.offsets[i] + s.counts[i];
  s.total = s.offsets[nn];
  if (s.total == 0) return hipSuccess;
  const hipError_t e = hipMalloc(&s.idx_d, s.total * sizeof(int64_t));
  return e != hipSuccess ? e : hipMemcpyAsync(s.idx_d, idx, s.total * sizeof(int64_t), hipMemcpyHostToDevice, stream);
}

// f(T()) with T the element type of ``eb`` bytes
template <typename F>
inline auto by_elem(int eb, F f) {
  return eb == 8 ? f(double()) : f(float());
}

// ------------------------------------------------------------------------------------ packed transports: pack / unpack
// where the message of an end lives: the contiguous ghost block of the vector itself, or the side's message buffer
inline char* halo_message(const Halo* h, const ExchangeEnd& e, char* vec) {
  return e.gather ? (e.side == &h->owners ? h->buf_owner : h->buf_ghost) : vec + e.offset * h->eb;
}

// the one launch (all neighbours) that packs a sending end's message or unpacks a receiving end's; none for the ghost block
inline hipError_t halo_stage(const Halo* h, const ExchangeEnd& e, char* vec, hipStream_t s) {
  if (!e.gather) return hipSuccess;
  char* msg = halo_message(h, e, vec);
  return by_elem(h->eb, [&](auto t) {
    using T = decltype(t);
    const int64_t n = e.side->total;
    switch (e.mode) {
      case PACK: return launch_halo<T, PACK>((const T*)vec, (T*)msg, e.idx, n, e.offset, s);
      case UNPACK_SET: return launch_halo<T, UNPACK_SET>((const T*)msg, (T*)vec, e.idx, n, e.offset, s);
      default: return launch_halo<T, UNPACK_ADD>((const T*)msg, (T*)vec, e.idx, n, e.offset, s);
    }
  });
}

}  // namespace fus
