// PEER transport of the halo exchange, host side (the kernels and the protocol: halo_ipc.hpp; the arena layout and the
// wiring arithmetic: halo_layout.hpp).  The neighbours' receive arenas are mapped once (HIP IPC handles exchanged by the
// host's bootstrap channel); an exchange is then one send and one receive kernel per rank.
#pragma once

#include <strings.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "halo_ipc.hpp"
#include "halo_object.hpp"

namespace fus {

constexpr uint32_t kIpcMagic = 0x46555349u;  // "FUSI"
constexpr int32_t kIpcBlobVersion = 3;

// Identity of THIS process, drawn once: a pid alone does not identify an address space (ranks in different PID namespaces
// -- one container per rank -- can share a pid, and the importer would then dereference a foreign virtual address).
struct IpcProcessToken {
  uint64_t w[2];
};
inline const IpcProcessToken& ipc_process_token() {
  static const IpcProcessToken tok = [] {
    IpcProcessToken t{{0, 0}};
    if (FILE* f = std::fopen("/dev/urandom", "rb")) {
      if (std::fread(&t, sizeof t, 1, f) != 1) t = IpcProcessToken{{0, 0}};
      std::fclose(f);
    }
    if (!t.w[0] && !t.w[1]) {  // no /dev/urandom: pid + a high-resolution clock + an address of this image
      t.w[0] = ((uint64_t)getpid() << 32) ^ (uint64_t)(uintptr_t)&ipc_process_token;
      t.w[1] = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
    }
    t.w[0] |= 1;  // never all-zero
    return t;
  }();
  return tok;
}

struct IpcBlobHeader {
  uint32_t magic;
  int32_t version;
  int32_t rank;
  int32_t elem_bytes;
  IpcProcessToken token;  // of the exporting process
  char pci_bus_id[32];  // of the exporter's device: ordinals are process-local (HIP_VISIBLE_DEVICES per rank)
  IpcArena arena;  // layout, and the base in the exporting process (used directly when importer == exporter process)
  hipIpcMemHandle_t handle;
  int32_t n_owner, n_ghost;
  // followed by n_owner x (int64 rank, count, offset), then n_ghost x the same
};

// A process that drives several ranks maps a neighbour's arena once, however many of its ranks border that neighbour
// (opening one HIP IPC handle twice in a process is not portable): process-wide table, reference counted.
struct IpcOpened {
  hipIpcMemHandle_t handle;
  void* ptr;
  int refs;
  std::vector<int> importers;  // devices of this process that may dereference ``ptr``
};
struct IpcOpenedTable {
  std::mutex mutex;  // guards ``rows``
  std::vector<IpcOpened> rows;
};
inline IpcOpenedTable& ipc_opened_table() {
  static IpcOpenedTable t;
  return t;
}
// ``importer``: the device whose kernels will use the mapping (the communicator's); ``exporter``: the device the arena lives on,
// as an ordinal of THIS process (-1: not visible here).  hipIpcMemLazyEnablePeerAccess enables peer access for the device that
// is current at the first open only: a second rank of this process on ANOTHER device that borders the same neighbour gets
// the cached pointer and must have peer access to the exporter enabled for itself, or its send / receive kernel faults
// (ADVICE r4).
inline hipError_t ipc_open_shared(const hipIpcMemHandle_t& handle, int importer, int exporter, void** out) {
  std::lock_guard<std::mutex> lock(ipc_opened_table().mutex);
  for (IpcOpened& o : ipc_opened_table().rows)
    if (!std::memcmp(&o.handle, &handle, sizeof handle)) {
      bool known = false;
      for (int d : o.importers) known = known || d == importer;
      if (!known) {
        if (exporter >= 0 && exporter != importer) {
          int cur = -1;
          hipError_t e = hipGetDevice(&cur);
          if (e == hipSuccess && cur != importer) e = hipSetDevice(importer);
          if (e == hipSuccess) {
            e = hipDeviceEnablePeerAccess(exporter, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) {
              (void)hipGetLastError();
              e = hipSuccess;
            }
          }
          if (cur >= 0 && cur != importer) (void)hipSetDevice(cur);
          if (e != hipSuccess) return e;
        }
        o.importers.push_back(importer);
      }
      ++o.refs;
      *out = o.ptr;
      return hipSuccess;
    }
  void* p = nullptr;
  const hipError_t e = hipIpcOpenMemHandle(&p, handle, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) return e;
  ipc_opened_table().rows.push_back(IpcOpened{handle, p, 1, {importer}});
  *out = p;
  return hipSuccess;
}
inline void ipc_close_shared(void* p) {
  std::lock_guard<std::mutex> lock(ipc_opened_table().mutex);
  auto& t = ipc_opened_table().rows;
  for (size_t i = 0; i < t.size(); ++i)
    if (t[i].ptr == p) {
      if (--t[i].refs == 0) {
        (void)hipIpcCloseMemHandle(p);
        t.erase(t.begin() + (long)i);
      }
      return;
    }
}

inline void ipc_role_free(IpcRole& r) {
  if (r.chunks) (void)hipFree(r.chunks);
  if (r.peers) (void)hipFree(r.peers);
  if (r.counters) (void)hipFree(r.counters);
  r = IpcRole();
}

// chunk table of one side on the device: every neighbour's segment cut into pieces of ipc_chunk() elements
inline hipError_t ipc_role_init(IpcRole& r, const Side& s) {
  const std::vector<IpcChunk> ch = ipc_cut_chunks(s.counts, s.offsets, ipc_chunk(), r.host_peers);
  r.nnbr = (int)s.counts.size();
  r.nchunks = (int)ch.size();
  if (r.nchunks == 0) return hipSuccess;
  hipError_t e = hipMalloc(&r.chunks, ch.size() * sizeof(IpcChunk));
  if (e == hipSuccess) e = hipMemcpy(r.chunks, ch.data(), ch.size() * sizeof(IpcChunk), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&r.peers, r.nnbr * sizeof(IpcPeer));
  if (e == hipSuccess) e = hipMalloc(&r.counters, r.nnbr * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(r.counters, 0, r.nnbr * sizeof(unsigned));
  return e;
}

inline hipError_t ipc_arena_alloc(IpcState& st) {  // st.arena_bytes of it, zeroed
  // Arena memory: UNCACHED device memory first (what RCCL gives its own peer-to-peer flag / LL buffers on gfx942 / gfx950;
  // every access of the exchange kernels bypasses the caches anyway, and nothing else may ever find a stale line of it),
  // then fine-grained, then ordinary memory.  FUS_IPC_MEMORY = uncached | finegrained | coarse picks the first choice
  // (all three export / open through HIP IPC and pass the two-process probe: profiles/r03a_ipc_probe.log).
  const char* force = std::getenv("FUS_IPC_MEMORY");
  const int first = force ? (!std::strcmp(force, "finegrained") ? 0 : !std::strcmp(force, "coarse") ? 2 : 1) : 1;
  hipError_t e = hipErrorOutOfMemory;
  for (const int kind : {first, first == 1 ? 0 : 1, first == 2 ? 0 : 2}) {  // the first choice, then the other two
    void* p = nullptr;
    e = kind == 0   ? hipExtMallocWithFlags(&p, st.arena_bytes, hipDeviceMallocFinegrained)
        : kind == 1 ? hipExtMallocWithFlags(&p, st.arena_bytes, hipDeviceMallocUncached)
                    : hipMalloc(&p, st.arena_bytes);
    if (e == hipSuccess) {
      st.arena = static_cast<char*>(p);
      st.memory_kind = kind;
      break;
    }
    (void)hipGetLastError();
  }
  return e != hipSuccess ? e : hipMemset(st.arena, 0, st.arena_bytes);
}

inline void halo_ipc_free(Halo* h) {
  IpcState& st = h->ipc;
  for (void* p : st.opened) ipc_close_shared(p);
  st.opened.clear();
  for (IpcRole* r : {&st.send_fwd, &st.recv_fwd, &st.send_rev, &st.recv_rev}) ipc_role_free(*r);
  if (st.arena) (void)hipFree(st.arena);
  if (st.status) (void)hipFree(st.status);
  if (st.ev_sent) (void)hipEventDestroy(st.ev_sent);
  if (st.join_counter) (void)hipFree(st.join_counter);
  st = IpcState();
}

inline hipError_t halo_ipc_create(Halo* h) {
  IpcState& st = h->ipc;
  static_cast<IpcArena&>(st) = ipc_arena_layout(*h, h->eb);
  hipError_t e = ipc_arena_alloc(st);
  if (e == hipSuccess) e = hipMalloc(&st.status, ST_WORDS * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemset(st.status, 0, ST_WORDS * sizeof(uint64_t));
  if (e == hipSuccess) e = ipc_role_init(st.send_fwd, h->ghosts);
  if (e == hipSuccess) e = ipc_role_init(st.recv_rev, h->ghosts);
  if (e == hipSuccess) e = ipc_role_init(st.recv_fwd, h->owners);
  if (e == hipSuccess) e = ipc_role_init(st.send_rev, h->owners);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&st.ev_sent, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&st.join_counter, sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(st.join_counter, 0, sizeof(unsigned));
  st.budget = spin_budget_ticks(h->comm->device);
  if (const char* v = std::getenv("FUS_IPC_FENCED")) st.fenced = std::atoi(v) != 0 ? 1 : 0;
  if (e == hipSuccess) e = hipDeviceSynchronize();  // arena zeroed before its handle can reach a peer
  return e;
}

inline int64_t halo_ipc_blob_bytes(const Halo* h) {
  return (int64_t)sizeof(IpcBlobHeader) + 3 * (int64_t)sizeof(int64_t) * (int64_t)(h->owners.ranks.size() + h->ghosts.ranks.size());
}

inline int halo_ipc_export(Halo* h, void* blob) {
  Comm* c = h->comm;
  IpcState& st = h->ipc;
  IpcBlobHeader hd;
  std::memset(static_cast<void*>(&hd), 0, sizeof hd);
  hd.magic = kIpcMagic;
  hd.version = kIpcBlobVersion;
  hd.rank = c->rank;
  hd.elem_bytes = h->eb;
  hd.token = ipc_process_token();
  if (hipDeviceGetPCIBusId(hd.pci_bus_id, (int)sizeof hd.pci_bus_id, c->device) != hipSuccess) {
    (void)hipGetLastError();
    hd.pci_bus_id[0] = 0;
  }
  hd.pci_bus_id[sizeof hd.pci_bus_id - 1] = 0;
  hd.arena = st;  // (sliced: the layout and my base address)
  hd.n_owner = (int32_t)h->owners.ranks.size();
  hd.n_ghost = (int32_t)h->ghosts.ranks.size();
  const hipError_t e = hipIpcGetMemHandle(&hd.handle, st.arena);
  if (e != hipSuccess) {
    c->last_error = std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e);
    return -1;
  }
  char* out = static_cast<char*>(blob);
  std::memcpy(out, &hd, sizeof hd);
  int64_t* t = reinterpret_cast<int64_t*>(out + sizeof hd);
  for (const Side* s : {&h->owners, &h->ghosts})
    for (size_t k = 0; k < s->ranks.size(); ++k) {
      *t++ = s->ranks[k];
      *t++ = s->counts[k];
      *t++ = s->offsets[k];
    }
  return 0;
}

// The arena behind a neighbour's blob as THIS process addresses it (nullptr: last_error says why): the exporter's own
// pointer inside one address space, else the handle opened through the process-wide table.
inline char* ipc_map_arena(Halo* h, const IpcBlobHeader& hd) {
  Comm* c = h->comm;
  const IpcProcessToken& me = ipc_process_token();
  if (hd.token.w[0] == me.w[0] && hd.token.w[1] == me.w[1]) {  // same address space (in-process ranks, self-neighbour)
    if (hd.rank != c->rank) h->ipc.defer_recv = true;
    return hd.arena.arena;
  }
  // another process (normally another GPU): refuse up front what would otherwise fault inside a kernel.  The
  // exporter's device is identified by its PCI bus id -- ordinals are process-local -- and looked up among the
  // devices visible HERE; one that is not visible here cannot be checked and is left to hipIpcOpenMemHandle.
  int ndev = 0, can = 1, peer_dev = -1;
  if (hd.pci_bus_id[0] && hipGetDeviceCount(&ndev) == hipSuccess)
    for (int d = 0; d < ndev && peer_dev < 0; ++d) {
      char id[32] = {0};
      if (hipDeviceGetPCIBusId(id, (int)sizeof id, d) == hipSuccess && !strcasecmp(id, hd.pci_bus_id)) peer_dev = d;
    }
  if (peer_dev >= 0 && peer_dev != c->device && hipDeviceCanAccessPeer(&can, c->device, peer_dev) == hipSuccess && !can) {
    c->last_error = "device " + std::to_string(c->device) + " has no peer access to device " + std::string(hd.pci_bus_id) +
                    " (rank " + std::to_string(hd.rank) + ")";
    return nullptr;
  }
  (void)hipGetLastError();
  void* p = nullptr;
  const hipError_t e = ipc_open_shared(hd.handle, c->device, peer_dev, &p);
  if (e != hipSuccess) {
    c->last_error = "hipIpcOpenMemHandle (rank " + std::to_string(hd.rank) + "): " + hipGetErrorString(e);
    return nullptr;
  }
  h->ipc.opened.push_back(p);
  return static_cast<char*>(p);
}

// ``blobs``: what fus_halo_ipc_export produced on the other ranks for THE SAME halo (same creation order), any order,
// at least one per neighbour rank (extra ones are ignored).  Parses them, maps the neighbours' arenas, wires every
// neighbour slot of the owners side and of the ghosts side (ipc_wire_slot) and uploads the device tables.
inline int halo_ipc_connect(Halo* h, int nblobs, const void* const* blobs) {
  Comm* c = h->comm;
  IpcState& st = h->ipc;
  if (st.connected) {
    c->last_error = "halo already connected";
    return -1;
  }
  std::map<int, const IpcBlobHeader*> from;  // by exporting rank
  for (int b = 0; b < nblobs; ++b) {
    if (!blobs[b]) continue;
    const auto* hd = static_cast<const IpcBlobHeader*>(blobs[b]);
    if (hd->magic != kIpcMagic || hd->version != kIpcBlobVersion || hd->elem_bytes != h->eb || hd->rank < 0 || hd->rank >= c->nranks) {
      c->last_error = "halo connect: malformed or mismatching blob";
      return -1;
    }
    from[hd->rank] = hd;
  }
  std::map<int, char*> arenas;  // a neighbour's arena is mapped once, whichever sides list it
  // owners side (my ghosts' owners): I receive forward, send reverse; ghosts side (ranks ghosting my dofs): the opposite.
  // The neighbour lists me on its OTHER side.
  for (const bool owners_side : {true, false}) {
    const Side& s = owners_side ? h->owners : h->ghosts;
    IpcRole &send = owners_side ? st.send_rev : st.send_fwd, &recv = owners_side ? st.recv_fwd : st.recv_rev;
    for (size_t i = 0; i < s.ranks.size(); ++i) {
      if (s.counts[i] == 0) continue;
      const int rank = s.ranks[i];
      if (!from.count(rank)) {
        c->last_error = "halo connect: no blob from neighbour rank " + std::to_string(rank);
        return -1;
      }
      const IpcBlobHeader* hd = from[rank];
      char*& pa = arenas[rank];
      if (!pa && !(pa = ipc_map_arena(h, *hd))) return -1;
      IpcArena theirs = hd->arena;
      theirs.arena = pa;
      const int64_t* triples = reinterpret_cast<const int64_t*>(hd + 1) + (owners_side ? 3 * hd->n_owner : 0);
      if (!ipc_wire_slot(owners_side, s.counts[i], (int)i, c->rank, st, triples, owners_side ? hd->n_ghost : hd->n_owner, theirs,
                         h->eb, send.host_peers[i], recv.host_peers[i])) {
        c->last_error = "halo connect: rank " + std::to_string(rank) + " does not list this rank with the same count";
        return -1;
      }
    }
  }
  for (IpcRole* r : {&st.send_fwd, &st.recv_fwd, &st.send_rev, &st.recv_rev})
    if (r->nchunks > 0) FUS_H(c, hipMemcpy(r->peers, r->host_peers.data(), r->nnbr * sizeof(IpcPeer), hipMemcpyHostToDevice));
  st.connected = true;
  return 0;
}

inline bool halo_ipc_connected(Halo* h) {
  if (!h->ipc.connected) h->comm->last_error = "halo not connected: exchange the blobs of fus_halo_ipc_export and call fus_halo_ipc_connect first";
  return h->ipc.connected;
}

// One exchange kernel over the chunks of ``r`` on stream ``s``; ``extra``: the send kernel's gate, the receive kernel's join.
template <typename T, typename K, typename X>
inline hipError_t ipc_launch(K kernel, const IpcRole& r, hipStream_t s, char* vec, const ExchangeEnd& end, const IpcState& st, uint64_t seq,
                             X extra) {
  hipLaunchKernelGGL(kernel, dim3(r.nchunks), dim3(ipc_threads()), 0, s, reinterpret_cast<T*>(vec), end.idx, end.offset, r.chunks,
                     r.peers, r.counters, st.status, seq, st.budget, extra, st.fenced);
  return hipGetLastError();
}

// ``on_stream``: the caller enqueues on the communicator's own stream (HaloApply's concurrent schedule): stream order is
// all the ordering there is, and no event is recorded (an event record is a marker with a cache write-back between the
// exchange kernels).  ``inline_mode``: both kernels on ``run_on``, the caller's own stream (may be the null stream).
inline int halo_ipc_post_recv(Halo* h, char* vecp, int dir, uint64_t seq, bool on_stream, bool inline_mode = false,
                              hipStream_t run_on = nullptr) {
  Comm* c = h->comm;
  IpcState& st = h->ipc;
  hipStream_t rs = inline_mode ? run_on : c->stream2;
  const IpcRole& rr = dir == 0 ? st.recv_fwd : st.recv_rev;
  IpcJoin join{nullptr, 0, st.join_counter};
  if (c->join_armed && c->join_halo == h && c->join_dir == dir) {
    c->join_armed = false;
    c->join_halo = nullptr;
    if (rr.nchunks > 0 && c->stream2 == c->stream && !inline_mode) {  // this kernel is the last of the chain: it publishes the join flag
      join.flag = c->sync_words + 1;
      join.seq = ++c->sync_seq[1];
      c->join_inflight = join.seq;
    }
  }
  if (rr.nchunks > 0) {
    const ExchangeEnd end = exchange_ends(*h, dir).recv;
    FUS_H(c, by_elem(h->eb, [&](auto t) {
      using T = decltype(t);
      if (end.mode == UNPACK_ADD) return ipc_launch<T>(ipc_recv_kernel<T, UNPACK_ADD, true>, rr, rs, vecp, end, st, seq, join);
      if (end.gather) return ipc_launch<T>(ipc_recv_kernel<T, UNPACK_SET, true>, rr, rs, vecp, end, st, seq, join);
      return ipc_launch<T>(ipc_recv_kernel<T, UNPACK_SET, false>, rr, rs, vecp, end, st, seq, join);  // the ghost block, grouped by owner
    }));
  }
  st.done_recorded = !on_stream;
  if (!on_stream) FUS_H(c, hipEventRecord(h->ev_done, rs));
  return 0;
}

// the receive kernel a *_begin left to *_end (ranks of ONE process, IpcState::defer_recv), if one is pending
inline int halo_ipc_post_deferred(Halo* h, char* vec, int dir, bool on_stream, bool inline_mode = false, hipStream_t run_on = nullptr) {
  if (!h->ipc.defer_recv || !h->ipc.pending[dir]) return 0;
  return halo_ipc_post_recv(h, vec, dir, std::exchange(h->ipc.pending[dir], 0), on_stream, inline_mode, run_on);
}

inline int halo_ipc_post(Halo* h, char* vecp, int dir, bool on_stream, bool inline_mode = false, hipStream_t run_on = nullptr) {
  Comm* c = h->comm;
  IpcState& st = h->ipc;
  hipStream_t ss = inline_mode ? run_on : c->stream;
  const uint64_t seq = ++st.seq[dir];
  const IpcRole& sr = dir == 0 ? st.send_fwd : st.send_rev;
  // a lazily posted fork: the first send kernel on the communicator's stream waits for the fork flag itself; where there
  // is none to carry the wait (no neighbours on this side), a wait kernel does
  IpcGate gate{nullptr, 0, nullptr};
  if (c->gate_pending && !inline_mode) {
    if (sr.nchunks > 0) {
      gate = IpcGate{c->sync_words + 0, c->gate_pending, c->sync_words + 2};
      c->gate_pending = 0;
    } else {
      FUS_H(c, comm_flush_gate(c));
    }
  }
  if (sr.nchunks > 0) {
    const ExchangeEnd end = exchange_ends(*h, dir).send;
    FUS_H(c, by_elem(h->eb, [&](auto t) {
      using T = decltype(t);
      // forward: owned entries listed in ghosts.idx -> the ghosting ranks; reverse: permuted ghosts, or the ghost block as it is -> owners
      return end.gather ? ipc_launch<T>(ipc_send_kernel<T, true>, sr, ss, vecp, end, st, seq, gate)
                        : ipc_launch<T>(ipc_send_kernel<T, false>, sr, ss, vecp, end, st, seq, gate);
    }));
  }
  st.sent_recorded = !on_stream;
  if (!on_stream) FUS_H(c, hipEventRecord(st.ev_sent, ss));
  if (st.defer_recv) {  // ranks of ONE process: the receive kernel is posted by *_end (see IpcState::defer_recv)
    st.pending[dir] = seq;
    return 0;
  }
  return halo_ipc_post_recv(h, vecp, dir, seq, on_stream, inline_mode, run_on);
}

// failures seen by this halo's kernels (0 = healthy); synchronises the communicator's streams
//   out8 = {failed waits (time-outs + poisoned flags read), forward exchanges posted, reverse exchanges posted, arena
//           memory kind, time-outs, poisoned flags read (a neighbour's halo had failed), dead (0 / 1), fenced (0 / 1)}
inline int halo_ipc_status(Halo* h, int64_t* out8) {
  Comm* c = h->comm;
  uint64_t w[ST_WORDS] = {0};
  // the whole device: a stand-alone exchange runs its kernels on the CALLER's stream (peer_exchange_inline), not on the
  // communicator's
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(w, h->ipc.status, sizeof w, hipMemcpyDeviceToHost);
  FUS_H(c, e);
  const uint64_t out[8] = {w[ST_TIMEOUTS] + w[ST_POISONED], h->ipc.seq[0], h->ipc.seq[1], (uint64_t)h->ipc.memory_kind,
                           w[ST_TIMEOUTS], w[ST_POISONED], w[ST_DEAD], (uint64_t)h->ipc.fenced};
  std::memcpy(out8, out, sizeof out);
  return 0;
}

// the caller may BE on the communicator's stream (HaloApply's concurrent schedule): then stream order is all there is
inline bool peer_on_stream(const Comm* c, hipStream_t stream) { return stream == c->stream && stream == c->stream2; }

inline int peer_begin_group(Comm* c, Halo* const* hs, void* const* buffers, int nh, hipStream_t stream, int dir) {
  for (int k = 0; k < nh; ++k)
    if (!halo_ipc_connected(hs[k])) return -1;
  const bool on_stream = peer_on_stream(c, stream);
  if (!on_stream) {
    FUS_H(c, comm_flush_gate(c));
    FUS_H(c, hipEventRecord(hs[0]->ev_ready, stream));
    if (stream != c->stream) FUS_H(c, hipStreamWaitEvent(c->stream, hs[0]->ev_ready, 0));
    if (stream != c->stream2 && c->stream2 != c->stream) FUS_H(c, hipStreamWaitEvent(c->stream2, hs[0]->ev_ready, 0));
  }
  if (c->join_armed && !c->join_halo) {  // fus_comm_arm_join: the last receive kernel of THIS call carries the join
    c->join_halo = hs[nh - 1];
    c->join_dir = dir;
  }
  for (int k = 0; k < nh; ++k)
    if (halo_ipc_post(hs[k], static_cast<char*>(buffers[k]), dir, on_stream) != 0) return -1;
  return 0;
}

// *done: the caller's stream is ordered after the exchange already; else it still has to wait for the "done" event
inline int peer_end(Comm* c, Halo* h, char* vec, hipStream_t stream, int dir, bool* done) {
  const bool on_stream = peer_on_stream(c, stream);
  if (halo_ipc_post_deferred(h, vec, dir, on_stream) != 0) return -1;
  *done = true;
  if (on_stream) return 0;  // the caller is on the exchange kernels' stream: already ordered
  // begin was called on the communicator's stream, end from elsewhere: the events were not recorded then -- now is as good
  if (!h->ipc.sent_recorded) FUS_H(c, hipEventRecord(h->ipc.ev_sent, c->stream));
  if (!h->ipc.done_recorded) FUS_H(c, hipEventRecord(h->ev_done, c->stream2));
  h->ipc.sent_recorded = h->ipc.done_recorded = true;
  if (stream != c->stream) FUS_H(c, hipStreamWaitEvent(stream, h->ipc.ev_sent, 0));  // the send kernel has read the vector
  *done = stream == c->stream2;
  return 0;
}

// begin + end of ONE exchange in one call: both kernels run on the CALLER's stream, in stream order with what precedes and
// follows them -- no event edge to the communicator's stream and back (a stand-alone exchange has nothing to overlap with;
// profiles/r04l_scatter_alone.log).  A receive that was deferred (ranks of one process) is posted here too, so a host
// driving several ranks calls begin / end separately instead.
inline int peer_exchange_inline(Halo* h, char* vec, hipStream_t stream, int dir) {
  if (!halo_ipc_connected(h) || halo_ipc_post(h, vec, dir, true, true, stream) != 0) return -1;
  return halo_ipc_post_deferred(h, vec, dir, true, true, stream);
}

}  // namespace fus
