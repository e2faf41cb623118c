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

static bool rccl_loaded() {
  if (!fus::rccl().load()) g_comm_error = fus::rccl().error;
  return fus::rccl().handle != nullptr;
}

int fus_comm_unique_id(void* id) {
  if (!id) return FUS_ERR_INVALID_ARGUMENT;
  if (!rccl_loaded()) return FUS_ERR_COMM;
  fus::RcclApi& api = fus::rccl();
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

// Release whatever of a communicator exists: both streams (drained first), the fork / join words, the RCCL communicator.
// fus_comm_destroy and every failure path of the creators end here.
static void comm_release(fus_comm* comm) {
  fus::Comm& c = comm->c;
  (void)fus::comm_flush_attached(&c);  // a fork signal still waiting for a launch to carry it must not outlive its flag
  if (c.stream) (void)hipStreamSynchronize(c.stream);
  if (c.stream2) (void)hipStreamSynchronize(c.stream2);
  if (c.nccl) (void)fus::rccl().CommDestroy(c.nccl);
  if (c.stream2 && c.stream2 != c.stream) (void)hipStreamDestroy(c.stream2);
  if (c.stream) (void)hipStreamDestroy(c.stream);
  if (c.sync_words) (void)hipFree(c.sync_words);
  delete comm;
}

// *out: a communicator of ``kind`` with its stream(s) and fork / join words; on failure nothing is left behind or written
static int comm_new(fus::Comm::Kind kind, int nranks, int rank, fus_comm** out) {
  auto* c = new fus_comm;
  c->c.kind = kind;
  c->c.rank = rank;
  c->c.nranks = nranks;
  hipError_t e = fus::comm_make_stream(&c->c);
  if (e == hipSuccess) e = fus::comm_sync_init(&c->c);
  if (e == hipSuccess) *out = c;
  else comm_release(c);
  return hip_rc(e);
}

int fus_comm_create(const void* id, int nranks, int rank, fus_comm_t* out) {
  if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks) return FUS_ERR_INVALID_ARGUMENT;
  if (!rccl_loaded()) return FUS_ERR_COMM;
  fus::RcclApi& api = fus::rccl();
  fus_comm* c = nullptr;
  if (const int rc = comm_new(fus::Comm::RCCL, nranks, rank, &c); rc != FUS_OK) return rc;
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  const ncclResult_t r = api.CommInitRank(&c->c.nccl, nranks, uid, rank);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclCommInitRank: ") + api.GetErrorString(r);
    c->c.nccl = nullptr;
    comm_release(c);
    return FUS_ERR_COMM;
  }
  *out = c;
  return FUS_OK;
}

int fus_comm_create_peer(int nranks, int rank, fus_comm_t* out) {
  if (!out || nranks < 1 || rank < 0 || rank >= nranks) return FUS_ERR_INVALID_ARGUMENT;
  return comm_new(fus::Comm::PEER, nranks, rank, out);
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
  const int rc = comm_new(fus::Comm::LOCAL, nranks, rank, out);
  if (rc == FUS_OK) (*out)->c.world = w;
  return rc;
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
int fus_comm_fork_flush(fus_comm_t comm) { return comm ? hip_rc(fus::comm_flush_attached(&comm->c)) : FUS_ERR_INVALID_ARGUMENT; }
int fus_comm_join(fus_comm_t comm, void* stream) { return comm_fork_join_rc(comm, stream, 1, false); }
int fus_comm_arm_join(fus_comm_t comm) { return comm ? hip_rc(fus::comm_arm_join(&comm->c)) : FUS_ERR_INVALID_ARGUMENT; }
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

const char* fus_comm_last_error(fus_comm_t comm) { return comm ? comm->c.last_error.c_str() : g_comm_error.c_str(); }

int fus_comm_destroy(fus_comm_t comm) {
  if (!comm) return FUS_OK;
  if (!comm->c.halos.empty()) {  // a halo holds a pointer to its communicator: destroy the halos first
    comm->c.last_error = "fus_comm_destroy: " + std::to_string(comm->c.halos.size()) + " halo object(s) of this communicator are still alive";
    return FUS_ERR_COMM;
  }
  comm_release(comm);
  return FUS_OK;
}

// Elements of one side of a plan, or -1: no rank or size list, a negative size, a neighbour rank outside the communicator, no index list,
// an index outside [0, bound) (it would fault in the pack / unpack kernels: checked here, once).  *identity: idx[i] == i, side not empty.
static int64_t side_check(int n, const int32_t* ranks, const int64_t* sizes, int nranks, const int64_t* idx, int64_t bound,
                          bool* identity) {
  int64_t total = 0;
  if (n > 0 && (!ranks || !sizes)) return -1;
  for (int i = 0; i < n; ++i) {
    if (sizes[i] < 0 || ranks[i] < 0 || ranks[i] >= nranks) return -1;
    total += sizes[i];
  }
  if (total > 0 && !idx) return -1;
  *identity = total > 0;
  for (int64_t i = 0; i < total; ++i) {
    if (idx[i] < 0 || idx[i] >= bound) return -1;
    if (idx[i] != i) *identity = false;
  }
  return total;
}

int fus_halo_create(fus_comm_t comm, int elem_bytes, int64_t nlocal, int64_t nghost, int n_owner_ranks,
                    const int32_t* owner_ranks, const int64_t* owner_sizes, const int64_t* owners_idx,
                    int n_ghost_ranks, const int32_t* ghost_ranks, const int64_t* ghost_sizes,
                    const int64_t* ghosts_idx, fus_halo_t* out) {
  if (!comm || !out || (elem_bytes != 4 && elem_bytes != 8) || nlocal < 0 || nghost < 0 || n_owner_ranks < 0 ||
      n_ghost_ranks < 0)
    return FUS_ERR_INVALID_ARGUMENT;
  bool direct = false, unused = false;
  const int64_t no = side_check(n_owner_ranks, owner_ranks, owner_sizes, comm->c.nranks, owners_idx, nghost, &direct);
  const int64_t ng = side_check(n_ghost_ranks, ghost_ranks, ghost_sizes, comm->c.nranks, ghosts_idx, nlocal, &unused);
  if (no < 0 || ng < 0 || no > nghost) return FUS_ERR_INVALID_ARGUMENT;
  auto* hh = new fus_halo;
  fus::Halo& h = hh->h;
  h.comm = &comm->c;
  h.eb = elem_bytes;
  h.nlocal = nlocal;
  h.nghost = nghost;
  h.direct = direct;
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
  fus::Comm& c = *h.comm;  // (set before anything of a halo can fail)
  if (c.stream) (void)hipStreamSynchronize(c.stream);
  if (c.stream2) (void)hipStreamSynchronize(c.stream2);
  if (c.kind == fus::Comm::LOCAL && c.world) {
    std::lock_guard<std::mutex> lock(fus::local_worlds_mutex());
    auto& mine = c.world->halos[c.rank];
    if (h.index < (int)mine.size() && mine[h.index] == &h) mine[h.index] = nullptr;
  }
  c.halos.erase(std::remove(c.halos.begin(), c.halos.end(), &h), c.halos.end());
  if (c.join_halo == &h) {
    c.join_halo = nullptr;
    c.join_armed = false;
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
  if (n < 0 || n > fus::kHaloGroupMax || (n > 0 && (!halos || !buffers))) return FUS_ERR_INVALID_ARGUMENT;
  fus::Halo* hs[fus::kHaloGroupMax];
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

int fus_halo_forward(fus_halo_t halo, void* buffer, void* stream) { return halo_op(fus::halo_exchange, halo, buffer, stream, 0); }
int fus_halo_reverse(fus_halo_t halo, void* buffer, void* stream) { return halo_op(fus::halo_exchange, halo, buffer, stream, 1); }

}  // extern "C"
