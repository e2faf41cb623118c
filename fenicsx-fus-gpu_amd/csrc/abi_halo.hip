// libfusgpu.so -- the communicator and halo-exchange part of the C ABI (include/fus_gpu.h: fus_comm_*, fus_halo_*) over halo_comm.hpp.
// A translation unit of its own: it shares nothing with the operator entry points of fus_gpu.hip but hip_rc.
#include "../../include/fus_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "fus_dispatch.hpp"
#include "halo_comm.hpp"

using namespace fus_abi;

extern "C" {

struct fus_comm {
  fus::Comm c;
};
struct fus_halo {
  fus::Halo h;
};

static std::string g_comm_error;  // errors that happen before a communicator exists

int fus_comm_unique_id(void* id) {
  if (!id) return FUS_ERR_INVALID_ARGUMENT;
  fus::RcclApi& api = fus::rccl();
  if (!api.load()) {
    g_comm_error = api.error;
    return FUS_ERR_COMM;
  }
  ncclUniqueId uid;
  static_assert(sizeof(uid) == FUS_UNIQUE_ID_BYTES, "unique id size");
  const ncclResult_t r = api.GetUniqueId(&uid);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclGetUniqueId: ") + api.GetErrorString(r);
    return FUS_ERR_COMM;
  }
  std::memcpy(id, &uid, sizeof(uid));
  return FUS_OK;
}

int fus_comm_create(const void* id, int nranks, int rank, fus_comm_t* out) {
  if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks) return FUS_ERR_INVALID_ARGUMENT;
  fus::RcclApi& api = fus::rccl();
  if (!api.load()) {
    g_comm_error = api.error;
    return FUS_ERR_COMM;
  }
  auto* c = new fus_comm;
  c->c.kind = fus::Comm::RCCL;
  c->c.rank = rank;
  c->c.nranks = nranks;
  hipError_t e = fus::comm_make_stream_and_sync(&c->c);
  if (e != hipSuccess) {
    delete c;
    return hip_rc(e);
  }
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  const ncclResult_t r = api.CommInitRank(&c->c.nccl, nranks, uid, rank);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclCommInitRank: ") + api.GetErrorString(r);
    (void)hipStreamDestroy(c->c.stream);
    delete c;
    return FUS_ERR_COMM;
  }
  *out = c;
  return FUS_OK;
}

int fus_comm_create_peer(int nranks, int rank, fus_comm_t* out) {
  if (!out || nranks < 1 || rank < 0 || rank >= nranks) return FUS_ERR_INVALID_ARGUMENT;
  auto* c = new fus_comm;
  c->c.kind = fus::Comm::PEER;
  c->c.rank = rank;
  c->c.nranks = nranks;
  hipError_t e = fus::comm_make_stream_and_sync(&c->c);
  if (e != hipSuccess) {
    if (c->c.stream) (void)hipStreamDestroy(c->c.stream);
    delete c;
    return hip_rc(e);
  }
  *out = c;
  return FUS_OK;
}

int fus_comm_create_local(int world_id, int nranks, int rank, fus_comm_t* out) {
  if (!out || nranks < 1 || rank < 0 || rank >= nranks) return FUS_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(fus::local_worlds_mutex());
  auto& worlds = fus::local_worlds();
  std::shared_ptr<fus::LocalWorld> w = worlds[world_id].lock();
  if (!w) {
    w = std::make_shared<fus::LocalWorld>();
    w->nranks = nranks;
    w->halos.resize(nranks);
    worlds[world_id] = w;
  }
  if (w->nranks != nranks) return FUS_ERR_INVALID_ARGUMENT;
  auto* c = new fus_comm;
  c->c.kind = fus::Comm::LOCAL;
  c->c.rank = rank;
  c->c.nranks = nranks;
  c->c.world = w;
  hipError_t e = fus::comm_make_stream_and_sync(&c->c);
  if (e != hipSuccess) {
    delete c;
    return hip_rc(e);
  }
  *out = c;
  return FUS_OK;
}

int fus_comm_rank(fus_comm_t comm) { return comm ? comm->c.rank : FUS_ERR_INVALID_ARGUMENT; }
int fus_comm_size(fus_comm_t comm) { return comm ? comm->c.nranks : FUS_ERR_INVALID_ARGUMENT; }
void* fus_comm_stream(fus_comm_t comm) { return comm ? comm->c.stream : nullptr; }

static int comm_fork_join_rc(fus_comm_t comm, void* stream, int which, bool lazy, bool attach = false) {
  if (!comm) return FUS_ERR_INVALID_ARGUMENT;
  bool misuse = false;
  const hipError_t e = fus::comm_fork_join(&comm->c, static_cast<hipStream_t>(stream), which, lazy, &misuse, attach);
  return misuse ? FUS_ERR_INVALID_ARGUMENT : hip_rc(e);
}
int fus_comm_fork(fus_comm_t comm, void* stream) { return comm_fork_join_rc(comm, stream, 0, false); }
int fus_comm_fork_lazy(fus_comm_t comm, void* stream) { return comm_fork_join_rc(comm, stream, 0, true); }
int fus_comm_fork_ex(fus_comm_t comm, void* stream, int flags) {
  if (flags & ~(FUS_FORK_LAZY | FUS_FORK_ATTACH)) return FUS_ERR_INVALID_ARGUMENT;
  return comm_fork_join_rc(comm, stream, 0, (flags & FUS_FORK_LAZY) != 0, (flags & FUS_FORK_ATTACH) != 0);
}
int fus_comm_fork_flush(fus_comm_t comm) {
  if (!comm) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::comm_flush_attached(&comm->c));
}
int fus_comm_join(fus_comm_t comm, void* stream) { return comm_fork_join_rc(comm, stream, 1, false); }
int fus_comm_arm_join(fus_comm_t comm) {
  if (!comm) return FUS_ERR_INVALID_ARGUMENT;
  return hip_rc(fus::comm_arm_join(&comm->c));
}
int fus_comm_health(fus_comm_t comm, int64_t* failures) {
  if (!comm || !failures) return FUS_ERR_INVALID_ARGUMENT;
  return fus::comm_health(&comm->c, failures) == 0 ? FUS_OK : FUS_ERR_COMM;
}
int fus_comm_health_detail(fus_comm_t comm, int64_t* out3) {
  if (!comm || !out3) return FUS_ERR_INVALID_ARGUMENT;
  int64_t total = 0;
  return fus::comm_health(&comm->c, &total, out3) == 0 ? FUS_OK : FUS_ERR_COMM;
}
int fus_comm_sync_timeouts(fus_comm_t comm, int64_t* out) {
  if (!comm || !out) return FUS_ERR_INVALID_ARGUMENT;
  *out = 0;
  if (!comm->c.sync_words) return FUS_OK;
  uint64_t w = 0;
  hipError_t e = hipStreamSynchronize(comm->c.stream);
  if (e == hipSuccess) e = hipMemcpy(&w, comm->c.sync_words + 2 + fus::ST_TIMEOUTS, sizeof w, hipMemcpyDeviceToHost);
  *out = (int64_t)w;
  return hip_rc(e);
}

const char* fus_comm_last_error(fus_comm_t comm) {
  return comm ? comm->c.last_error.c_str() : g_comm_error.c_str();
}

int fus_comm_destroy(fus_comm_t comm) {
  if (!comm) return FUS_OK;
  if (comm->c.nhalos > 0) {  // a halo holds a pointer to its communicator: destroy the halos first
    comm->c.last_error = "fus_comm_destroy: " + std::to_string(comm->c.nhalos) + " halo object(s) of this communicator are still alive";
    return FUS_ERR_COMM;
  }
  (void)fus::comm_flush_attached(&comm->c);  // a fork signal still waiting for a launch to carry it must not outlive its flag
  if (comm->c.stream) (void)hipStreamSynchronize(comm->c.stream);
  if (comm->c.stream2) (void)hipStreamSynchronize(comm->c.stream2);
  if (comm->c.nccl) (void)fus::rccl().CommDestroy(comm->c.nccl);
  if (comm->c.stream2 && comm->c.stream2 != comm->c.stream) (void)hipStreamDestroy(comm->c.stream2);
  if (comm->c.stream) (void)hipStreamDestroy(comm->c.stream);
  if (comm->c.sync_words) (void)hipFree(comm->c.sync_words);
  delete comm;
  return FUS_OK;
}

int fus_halo_create(fus_comm_t comm, int elem_bytes, int64_t nlocal, int64_t nghost, int n_owner_ranks,
                    const int32_t* owner_ranks, const int64_t* owner_sizes, const int64_t* owners_idx,
                    int n_ghost_ranks, const int32_t* ghost_ranks, const int64_t* ghost_sizes,
                    const int64_t* ghosts_idx, fus_halo_t* out) {
  if (!comm || !out || (elem_bytes != 4 && elem_bytes != 8) || nlocal < 0 || nghost < 0 || n_owner_ranks < 0 ||
      n_ghost_ranks < 0)
    return FUS_ERR_INVALID_ARGUMENT;
  if ((n_owner_ranks > 0 && (!owner_ranks || !owner_sizes)) || (n_ghost_ranks > 0 && (!ghost_ranks || !ghost_sizes)))
    return FUS_ERR_INVALID_ARGUMENT;
  int64_t no = 0, ng = 0;
  for (int i = 0; i < n_owner_ranks; ++i) {
    if (owner_sizes[i] < 0 || owner_ranks[i] < 0 || owner_ranks[i] >= comm->c.nranks) return FUS_ERR_INVALID_ARGUMENT;
    no += owner_sizes[i];
  }
  for (int i = 0; i < n_ghost_ranks; ++i) {
    if (ghost_sizes[i] < 0 || ghost_ranks[i] < 0 || ghost_ranks[i] >= comm->c.nranks) return FUS_ERR_INVALID_ARGUMENT;
    ng += ghost_sizes[i];
  }
  if (no > nghost || (no > 0 && !owners_idx) || (ng > 0 && !ghosts_idx)) return FUS_ERR_INVALID_ARGUMENT;
  // out-of-range indices would fault in the pack / unpack kernels: check them here, once
  bool direct = no > 0;
  for (int64_t i = 0; i < no; ++i) {
    if (owners_idx[i] < 0 || owners_idx[i] >= nghost) return FUS_ERR_INVALID_ARGUMENT;
    if (owners_idx[i] != i) direct = false;
  }
  for (int64_t i = 0; i < ng; ++i)
    if (ghosts_idx[i] < 0 || ghosts_idx[i] >= nlocal) return FUS_ERR_INVALID_ARGUMENT;
  auto* hh = new fus_halo;
  fus::Halo& h = hh->h;
  h.comm = &comm->c;
  h.eb = elem_bytes;
  h.nlocal = nlocal;
  h.nghost = nghost;
  h.direct = direct;
  ++comm->c.nhalos;
  comm->c.halos.push_back(&h);
  const bool peer = comm->c.kind == fus::Comm::PEER;
  hipError_t e = fus::side_init(h.owners, n_owner_ranks, owner_ranks, owner_sizes, owners_idx, comm->c.stream);
  if (e == hipSuccess) e = fus::side_init(h.ghosts, n_ghost_ranks, ghost_ranks, ghost_sizes, ghosts_idx, comm->c.stream);
  if (e == hipSuccess && no > 0 && !peer) e = hipMalloc(&h.buf_owner, no * elem_bytes);
  if (e == hipSuccess && ng > 0 && !peer) e = hipMalloc(&h.buf_ghost, ng * elem_bytes);
  if (e == hipSuccess && peer) e = fus::halo_ipc_create(&h);
  for (hipEvent_t* ev : {&h.ev_ready, &h.ev_done, &h.ev_packed, &h.ev_pulled})
    if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipStreamSynchronize(comm->c.stream);  // the index lists came from host arrays the caller may free
  if (e != hipSuccess) {
    fus_halo_destroy(hh);
    return hip_rc(e);
  }
  if (comm->c.kind == fus::Comm::LOCAL) {
    std::lock_guard<std::mutex> lock(fus::local_worlds_mutex());
    auto& mine = comm->c.world->halos[comm->c.rank];
    h.index = (int)mine.size();
    mine.push_back(&h);
  }
  *out = hh;
  return FUS_OK;
}

int fus_halo_destroy(fus_halo_t halo) {
  if (!halo) return FUS_OK;
  fus::Halo& h = halo->h;
  if (h.comm && h.comm->stream) (void)hipStreamSynchronize(h.comm->stream);
  if (h.comm && h.comm->stream2) (void)hipStreamSynchronize(h.comm->stream2);
  if (h.comm && h.comm->kind == fus::Comm::LOCAL && h.comm->world) {
    std::lock_guard<std::mutex> lock(fus::local_worlds_mutex());
    auto& mine = h.comm->world->halos[h.comm->rank];
    if (h.index < (int)mine.size() && mine[h.index] == &h) mine[h.index] = nullptr;
  }
  if (h.comm) {
    --h.comm->nhalos;
    auto& hv = h.comm->halos;
    hv.erase(std::remove(hv.begin(), hv.end(), &h), hv.end());
    if (h.comm->join_halo == &h) {
      h.comm->join_halo = nullptr;
      h.comm->join_armed = false;
    }
  }
  fus::halo_ipc_free(&h);
  fus::side_free(h.owners);
  fus::side_free(h.ghosts);
  if (h.buf_owner) (void)hipFree(h.buf_owner);
  if (h.buf_ghost) (void)hipFree(h.buf_ghost);
  for (hipEvent_t ev : {h.ev_ready, h.ev_done, h.ev_packed, h.ev_pulled})
    if (ev) (void)hipEventDestroy(ev);
  delete halo;
  return FUS_OK;
}

int fus_halo_is_direct(fus_halo_t halo) { return halo ? (halo->h.direct ? 1 : 0) : FUS_ERR_INVALID_ARGUMENT; }

int64_t fus_halo_ipc_blob_bytes(fus_halo_t halo) {
  if (!halo || halo->h.comm->kind != fus::Comm::PEER) return FUS_ERR_INVALID_ARGUMENT;
  return fus::halo_ipc_blob_bytes(&halo->h);
}
int fus_halo_ipc_export(fus_halo_t halo, void* blob) {
  if (!halo || !blob || halo->h.comm->kind != fus::Comm::PEER) return FUS_ERR_INVALID_ARGUMENT;
  return fus::halo_ipc_export(&halo->h, blob) == 0 ? FUS_OK : FUS_ERR_COMM;
}
int fus_halo_ipc_connect(fus_halo_t halo, int nblobs, const void* const* blobs) {
  if (!halo || nblobs < 0 || (nblobs > 0 && !blobs) || halo->h.comm->kind != fus::Comm::PEER) return FUS_ERR_INVALID_ARGUMENT;
  return fus::halo_ipc_connect(&halo->h, nblobs, blobs) == 0 ? FUS_OK : FUS_ERR_COMM;
}
int fus_halo_ipc_status(fus_halo_t halo, int64_t* out8) {
  if (!halo || !out8 || halo->h.comm->kind != fus::Comm::PEER) return FUS_ERR_INVALID_ARGUMENT;
  return fus::halo_ipc_status(&halo->h, out8) == 0 ? FUS_OK : FUS_ERR_COMM;
}

static int halo_op(int (*fn)(fus::Halo*, void*, hipStream_t, int), fus_halo_t halo, void* buffer, void* stream, int dir) {
  if (!halo || !buffer) return FUS_ERR_INVALID_ARGUMENT;
  return fn(&halo->h, buffer, static_cast<hipStream_t>(stream), dir) == 0 ? FUS_OK : FUS_ERR_COMM;
}
int fus_halo_forward_begin(fus_halo_t halo, void* buffer, void* stream) { return halo_op(fus::halo_begin, halo, buffer, stream, 0); }
int fus_halo_forward_end(fus_halo_t halo, void* buffer, void* stream) { return halo_op(fus::halo_end, halo, buffer, stream, 0); }
int fus_halo_reverse_begin(fus_halo_t halo, void* buffer, void* stream) { return halo_op(fus::halo_begin, halo, buffer, stream, 1); }
int fus_halo_reverse_end(fus_halo_t halo, void* buffer, void* stream) { return halo_op(fus::halo_end, halo, buffer, stream, 1); }

static int halo_group_rc(const fus_halo_t* halos, void* const* buffers, int n, void* stream, int dir) {
  if (n < 0 || n > 8 || (n > 0 && (!halos || !buffers))) return FUS_ERR_INVALID_ARGUMENT;
  fus::Halo* hs[8];
  for (int k = 0; k < n; ++k) {
    if (!halos[k] || !buffers[k]) return FUS_ERR_INVALID_ARGUMENT;
    hs[k] = &halos[k]->h;
  }
  return fus::halo_begin_group(hs, buffers, n, static_cast<hipStream_t>(stream), dir) == 0 ? FUS_OK : FUS_ERR_COMM;
}
int fus_halo_forward_begin_group(const fus_halo_t* halos, void* const* buffers, int n, void* stream) {
  return halo_group_rc(halos, buffers, n, stream, 0);
}
int fus_halo_reverse_begin_group(const fus_halo_t* halos, void* const* buffers, int n, void* stream) {
  return halo_group_rc(halos, buffers, n, stream, 1);
}

int fus_halo_forward(fus_halo_t halo, void* buffer, void* stream) {
  if (!halo || !buffer) return FUS_ERR_INVALID_ARGUMENT;
  const int r = fus::halo_exchange_inline(&halo->h, buffer, static_cast<hipStream_t>(stream), 0);  // PEER: on the caller's stream
  if (r <= 0) return r == 0 ? FUS_OK : FUS_ERR_COMM;
  const int rc = fus_halo_forward_begin(halo, buffer, stream);
  return rc != FUS_OK ? rc : fus_halo_forward_end(halo, buffer, stream);
}
int fus_halo_reverse(fus_halo_t halo, void* buffer, void* stream) {
  if (!halo || !buffer) return FUS_ERR_INVALID_ARGUMENT;
  const int r = fus::halo_exchange_inline(&halo->h, buffer, static_cast<hipStream_t>(stream), 1);
  if (r <= 0) return r == 0 ? FUS_OK : FUS_ERR_COMM;
  const int rc = fus_halo_reverse_begin(halo, buffer, stream);
  return rc != FUS_OK ? rc : fus_halo_reverse_end(halo, buffer, stream);
}

}  // extern "C"
