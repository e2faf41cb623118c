// LOCAL transport of the halo exchange: all ranks live in ONE process (tests on a one-GPU box, or one process driving
// several GPUs).  *_begin packs and records "packed"; *_end, on the receiver's communicator stream, pulls each message
// out of the peer's buffer with hipMemcpyAsync, ordered by events, and unpacks.  Host-side contract: every rank's
// *_begin of an exchange is called before any rank's *_end of it.
#pragma once

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "halo_object.hpp"

namespace fus {

struct LocalWorld {  // the ranks of one process
  int nranks = 0;
  std::vector<std::vector<Halo*>> halos;  // [rank][creation index]
};

inline std::mutex& local_worlds_mutex() {
  static std::mutex m;
  return m;
}

inline std::map<int, std::weak_ptr<LocalWorld>>& local_worlds() {  // guarded by local_worlds_mutex()
  static std::map<int, std::weak_ptr<LocalWorld>> m;
  return m;
}

// the halo object of ``rank`` that pairs with ``h`` (same creation index), or nullptr
inline Halo* local_peer(const Halo* h, int rank) {
  const auto& peers = h->comm->world->halos[rank];
  return h->index < (int)peers.size() ? peers[h->index] : nullptr;
}

// Receiver side: pull every incoming segment out of the peer's current message.
inline int halo_pull_local(Halo* h, const Side& rside, char* recvbuf, int dir) {
  Comm* c = h->comm;
  for (size_t i = 0; i < rside.ranks.size(); ++i) {
    if (rside.counts[i] == 0) continue;
    Halo* p = local_peer(h, rside.ranks[i]);
    if (!p) FUS_H(c, hipErrorInvalidValue);
    if (!p->cur_send || p->cur_dir != dir) FUS_H(c, hipErrorNotReady);  // the peer's *_begin has not been called
    // my segment inside the peer's outgoing message: the peer's send side lists me as a neighbour
    const Side& ps = *exchange_ends(*p, dir).send.side;
    int64_t poff = -1;
    for (size_t k = 0; k < ps.ranks.size(); ++k)
      if (ps.ranks[k] == c->rank) {
        if (ps.counts[k] != rside.counts[i]) FUS_H(c, hipErrorInvalidValue);
        poff = ps.offsets[k];
      }
    if (poff < 0) FUS_H(c, hipErrorInvalidValue);
    FUS_H(c, hipStreamWaitEvent(c->stream, p->ev_packed, 0));
    FUS_H(c, hipMemcpyAsync(recvbuf + rside.offsets[i] * h->eb, p->cur_send + poff * h->eb, rside.counts[i] * h->eb,
                            hipMemcpyDeviceToDevice, c->stream));
  }
  const hipError_t e = hipEventRecord(h->ev_pulled, c->stream);
  h->pulled_valid = true;
  FUS_H(c, e);
  return 0;
}

// Sender side: before overwriting my message buffer, wait until the peers that read the previous message out of it
// have done so.
inline int halo_wait_readers_local(Halo* h, const Side& sside) {
  for (size_t i = 0; i < sside.ranks.size(); ++i)
    if (const Halo* p = local_peer(h, sside.ranks[i]); p && p->pulled_valid)
      FUS_H(h->comm, hipStreamWaitEvent(h->comm->stream, p->ev_pulled, 0));
  return 0;
}

inline int local_begin_group(Comm* c, Halo* const* hs, void* const* buffers, int nh, int dir) {
  for (int k = 0; k < nh; ++k) {
    const ExchangeEnd send = exchange_ends(*hs[k], dir).send;
    char* vec = static_cast<char*>(buffers[k]);
    if (halo_wait_readers_local(hs[k], *send.side) != 0) return -1;
    FUS_H(c, halo_stage(hs[k], send, vec, c->stream));
    hs[k]->cur_send = halo_message(hs[k], send, vec);
    hs[k]->cur_dir = dir;
  }
  for (int k = 0; k < nh; ++k) FUS_H(c, hipEventRecord(hs[k]->ev_packed, c->stream));
  return 0;
}

// pull, unpack, "done" on the communicator's stream (the caller's stream then waits for the event: halo_end)
inline int local_end(Comm* c, Halo* h, char* vec, int dir) {
  const ExchangeEnd recv = exchange_ends(*h, dir).recv;
  if (halo_pull_local(h, *recv.side, halo_message(h, recv, vec), dir) != 0) return -1;
  FUS_H(c, halo_stage(h, recv, vec, c->stream));
  FUS_H(c, hipEventRecord(h->ev_done, c->stream));
  return 0;
}

}  // namespace fus
