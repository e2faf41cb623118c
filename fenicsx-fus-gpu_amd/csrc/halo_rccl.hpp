// RCCL transport of the halo exchange: librccl.so.1 resolved with dlopen at first use (libfusgpu.so itself has no
// link-time dependency on it: the operator kernels load on any ROCm box).  Bootstrap = 128-byte unique id from rank 0,
// broadcast by whatever the host already has (MPI_Bcast in the reference's drivers, torch.distributed here); one
// process per GPU.  *_begin enqueues the whole exchange on the communicator's stream -- pack (ONE launch for all neighbours)
// -> one ncclGroup of ncclSend / ncclRecv per neighbour (RCCL over xGMI: a neighbour all-to-all-v, no host sync) -> unpack
// (one launch) -> event "done" -- so not even the pack / unpack launches sit between begin and end.
#pragma once

#include <dlfcn.h>

#include <string>

#include "halo_object.hpp"

// The few RCCL declarations the dlopen'ed entry points need (rccl/rccl.h is not required to build the library).
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct {
  char internal[128];
} ncclUniqueId;
typedef int ncclResult_t;    // ncclSuccess == 0
typedef int ncclDataType_t;  // ncclFloat32 == 7, ncclFloat64 == 8 (nccl.h, stable since NCCL 2.0)
}
constexpr ncclResult_t ncclSuccess = 0;
constexpr ncclDataType_t ncclFloat32 = 7, ncclFloat64 = 8;

namespace fus {

struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;

  bool load() {
    if (handle) return true;
    // a process that already holds an RCCL (torch does) gets that one: same SONAME
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (handle) break;
    }
    if (!handle) {
      error = std::string("cannot load librccl.so.1: ") + dlerror();
      return false;
    }
#define FUS_SYM(field, sym)                                          \
  field = reinterpret_cast<decltype(field)>(dlsym(handle, sym));     \
  if (!field) {                                                      \
    error = std::string("librccl lacks ") + sym;                     \
    handle = nullptr;                                                \
    return false;                                                    \
  }
    FUS_SYM(GetUniqueId, "ncclGetUniqueId")
    FUS_SYM(CommInitRank, "ncclCommInitRank")
    FUS_SYM(CommDestroy, "ncclCommDestroy")
    FUS_SYM(GroupStart, "ncclGroupStart")
    FUS_SYM(GroupEnd, "ncclGroupEnd")
    FUS_SYM(Send, "ncclSend")
    FUS_SYM(Recv, "ncclRecv")
    FUS_SYM(GetErrorString, "ncclGetErrorString")
#undef FUS_SYM
    return true;
  }
};

inline RcclApi& rccl() {
  static RcclApi api;
  return api;
}

// Post the receives and sends of one exchange (inside an open ncclGroup): the segments of the receiving end into its
// message, those of the sending end out of its message.
inline ncclResult_t halo_post_rccl(Halo* h, const ExchangeEnds& x, char* vec) {
  Comm* c = h->comm;
  RcclApi& api = rccl();
  const Side &sside = *x.send.side, &rside = *x.recv.side;
  const char* sendbuf = halo_message(h, x.send, vec);
  char* recvbuf = halo_message(h, x.recv, vec);
  const ncclDataType_t dt = h->eb == 8 ? ncclFloat64 : ncclFloat32;
  ncclResult_t r = ncclSuccess;
  for (size_t i = 0; r == ncclSuccess && i < rside.ranks.size(); ++i)
    if (rside.counts[i] > 0)
      r = api.Recv(recvbuf + rside.offsets[i] * h->eb, (size_t)rside.counts[i], dt, rside.ranks[i], c->nccl, c->stream);
  for (size_t i = 0; r == ncclSuccess && i < sside.ranks.size(); ++i)
    if (sside.counts[i] > 0)
      r = api.Send(sendbuf + sside.offsets[i] * h->eb, (size_t)sside.counts[i], dt, sside.ranks[i], c->nccl, c->stream);
  return r;
}

// Begin ``nh`` exchanges as one unit; in the ONE ncclGroup two messages to the same peer are matched in issue order, which
// is the same on both sides.  The RK4 stage forward-scatters two vectors (u_n, v_n): one RCCL launch instead of two.
inline int rccl_begin_group(Comm* c, Halo* const* hs, void* const* buffers, int nh, int dir) {
  ExchangeEnds x[kHaloGroupMax];
  for (int k = 0; k < nh; ++k) {
    x[k] = exchange_ends(*hs[k], dir);
    FUS_H(c, halo_stage(hs[k], x[k].send, static_cast<char*>(buffers[k]), c->stream));
  }
  RcclApi& api = rccl();
  ncclResult_t r = api.GroupStart();
  for (int k = 0; r == ncclSuccess && k < nh; ++k) r = halo_post_rccl(hs[k], x[k], static_cast<char*>(buffers[k]));
  const ncclResult_t r2 = api.GroupEnd();
  if (r == ncclSuccess) r = r2;
  if (r != ncclSuccess) {
    c->last_error = std::string("RCCL: ") + api.GetErrorString(r);
    return -1;
  }
  for (int k = 0; k < nh; ++k) {
    FUS_H(c, halo_stage(hs[k], x[k].recv, static_cast<char*>(buffers[k]), c->stream));
    FUS_H(c, hipEventRecord(hs[k]->ev_done, c->stream));
  }
  return 0;
}

}  // namespace fus
