// Ghost-dof halo exchange behind the C ABI (fus_halo_{create,forward,reverse,destroy}): the switch over the
// three transports.
//
// Replaces the closures of cuda/scatterer.py:104-188 (scatter_reverse) and :191-277 (scatter_forward), which per neighbour
// launch one pack kernel, device-synchronise, post MPI Isend/Irecv on device pointers, wait, launch one unpack kernel and
// synchronise again, and the C++ driver's scatter calls (cpp/common/Linear.hpp:120,193,196,212).
//
// MI355X form: the library owns one HIGH-PRIORITY stream per communicator (comm_sync.hpp); an exchange is
//   [caller's stream: event "vector ready"]
//   comm stream: wait -> the transport's work (RCCL halo_rccl.hpp | LOCAL halo_local.hpp | PEER halo_peer.hpp) -> event "done"
//   [caller's stream: wait "done"]                                     <- fus_halo_*_end
// so between begin and end the caller's stream is free for interior-cell kernels.  What each end of an exchange packs,
// unpacks or moves as it lies in the vector: halo_layout.hpp exchange_ends.
#pragma once

#include <cstring>

#include "halo_local.hpp"
#include "halo_object.hpp"
#include "halo_peer.hpp"
#include "halo_rccl.hpp"

namespace fus {

// Failed device-side waits of EVERY halo object of the communicator plus of its fork / join kernels (0 = healthy): what a
// time loop checks before it trusts its result.  Synchronises the communicator's streams (one small copy per halo).
inline int comm_health(Comm* c, int64_t* failures, int64_t* detail3 = nullptr) {
  int64_t d[3] = {0, 0, 0};  // time-outs of halo waits, poisoned flags read, time-outs of fork / join waits
  hipError_t e = hipDeviceSynchronize();  // exchange kernels may have run on the communicator's stream(s) or on a caller's
  if (e == hipSuccess && c->sync_words) {
    uint64_t w = 0;
    e = hipMemcpy(&w, c->sync_words + 2 + ST_TIMEOUTS, sizeof w, hipMemcpyDeviceToHost);
    d[2] = (int64_t)w;
  }
  if (e == hipSuccess && c->kind == Comm::PEER)
    for (Halo* h : c->halos) {
      uint64_t w[ST_WORDS] = {0};
      if (!h->ipc.status) continue;
      e = hipMemcpy(w, h->ipc.status, sizeof w, hipMemcpyDeviceToHost);
      if (e != hipSuccess) break;
      d[0] += (int64_t)w[ST_TIMEOUTS];
      d[1] += (int64_t)w[ST_POISONED];
    }
  *failures = d[0] + d[1] + d[2];
  FUS_H(c, e);
  if (detail3) std::memcpy(detail3, d, sizeof d);
  return 0;
}

inline bool halo_has_neighbours(const Halo* h) { return h->owners.total > 0 || h->ghosts.total > 0; }

// Begin ``nh`` <= kHaloGroupMax exchanges (one per vector, halos of ONE communicator) as one unit: one event edge from the
// caller's stream, then every vector's messages.
inline int halo_begin_group(Halo* const* hs, void* const* buffers, int nh, hipStream_t stream, int dir) {
  if (nh <= 0) return 0;
  Comm* c = hs[0]->comm;
  bool any = false;
  for (int k = 0; k < nh; ++k) {
    if (hs[k]->comm != c) {
      c->last_error = "halo group: the halos belong to different communicators";
      return -1;
    }
    any = any || halo_has_neighbours(hs[k]);
  }
  if (!any) return 0;  // no neighbours: nothing to order, nothing to move
  if (nh > kHaloGroupMax) {
    c->last_error = "halo group: at most 8 vectors";
    return -1;
  }
  if (c->kind == Comm::PEER) return peer_begin_group(c, hs, buffers, nh, stream, dir);
  FUS_H(c, hipEventRecord(hs[0]->ev_ready, stream));
  FUS_H(c, hipStreamWaitEvent(c->stream, hs[0]->ev_ready, 0));
  return c->kind == Comm::LOCAL ? local_begin_group(c, hs, buffers, nh, dir) : rccl_begin_group(c, hs, buffers, nh, dir);
}

inline int halo_begin(Halo* h, void* buffer, hipStream_t stream, int dir) { return halo_begin_group(&h, &buffer, 1, stream, dir); }

inline int halo_end(Halo* h, void* buffer, hipStream_t stream, int dir) {
  Comm* c = h->comm;
  if (!halo_has_neighbours(h)) return 0;
  char* vec = static_cast<char*>(buffer);
  bool done = false;  // RCCL: everything was enqueued by begin
  if (c->kind == Comm::PEER && peer_end(c, h, vec, stream, dir, &done) != 0) return -1;
  if (c->kind == Comm::LOCAL && local_end(c, h, vec, dir) != 0) return -1;
  if (!done) FUS_H(c, hipStreamWaitEvent(stream, h->ev_done, 0));
  return 0;
}

// begin + end of ONE exchange in one call (scatter_forward(buffer) / scatter_reverse(buffer) of the reference's closures called alone:
// set-up exchanges, u_sol(with_ghosts), the non-overlapped stage): the transport's inline form where it has one (PEER), else begin; end.
inline int halo_exchange(Halo* h, void* buffer, hipStream_t stream, int dir) {
  if (!halo_has_neighbours(h)) return 0;
  if (h->comm->kind == Comm::PEER) return peer_exchange_inline(h, static_cast<char*>(buffer), stream, dir);
  const int rc = halo_begin(h, buffer, stream, dir);
  return rc != 0 ? rc : halo_end(h, buffer, stream, dir);
}

}  // namespace fus
