// The arithmetic of the halo exchange, free of HIP (any C++17 host compiler, like plan_registry.hpp; tests/host/halo_layout_check.cpp
// checks it without a GPU): the exchange rule -- what direction and ``direct`` decide for the two ends of an exchange (exchange_ends) --
// and the PEER arenas: their layout, the cutting of segments into chunks, the wiring of flags and segments between two ranks.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace fus {

enum HaloMode { PACK = 0, UNPACK_SET = 1, UNPACK_ADD = 2 };

// ------------------------------------------------------------------------------------ halo plan
struct Side {  // one side of the plan: per-neighbour ranks / counts / offsets + device index list
  std::vector<int> ranks;
  std::vector<int64_t> counts, offsets;
  int64_t total = 0;
  int64_t* idx_d = nullptr;  // concatenated index lists on the device
};

struct HaloPlan {
  int64_t nlocal = 0, nghost = 0;
  Side owners;          // my ghosts grouped by owning rank: indices into the ghost block
  Side ghosts;          // my owned dofs ghosted elsewhere, grouped by ghosting rank: local indices
  bool direct = false;  // ghosts numbered owner by owner: the ghost block is the owners-side message
};

// ------------------------------------------------------------------------------------ the exchange rule
// dir 0: forward (owners -> ghosts, overwrite)   cuda/scatterer.py:191-277
// dir 1: reverse (ghosts -> owners, add)         cuda/scatterer.py:104-188
// Element i of an end's message is vec[idx[i] + offset] where the end goes through its index list (``gather``), else
// vec[offset + i]: the contiguous ghost block, which needs no pack / unpack launch and no message buffer.
struct ExchangeEnd {
  const Side* side;
  const int64_t* idx;  // the side's device index list (also handed to the kernels of an end that does not gather)
  int64_t offset;      // elements
  bool gather;
  int mode;            // send: PACK; receive: UNPACK_SET (forward) or UNPACK_ADD (reverse)
};
struct ExchangeEnds { ExchangeEnd send, recv; };
// The ghosts side always gathers through ghosts.idx at offset 0; the owners side works at offset nlocal, through owners.idx unless
// ``direct``.  Forward sends the ghosts side and SETs the owners side, reverse sends the owners side and ADDs into the ghosts side.
inline ExchangeEnds exchange_ends(const HaloPlan& p, int dir) {
  const ExchangeEnd ghosts{&p.ghosts, p.ghosts.idx_d, 0, true, dir == 0 ? PACK : UNPACK_ADD};
  const ExchangeEnd owners{&p.owners, p.owners.idx_d, p.nlocal, !p.direct, dir == 0 ? UNPACK_SET : PACK};
  return dir == 0 ? ExchangeEnds{ghosts, owners} : ExchangeEnds{owners, ghosts};
}

// ------------------------------------------------------------------------------------ PEER arena layout
constexpr int kIpcFlagStride = 64;  // bytes between two flags: one flag per 64-byte line

// flag kinds inside an arena; slot = index of the neighbour in the owners-side (kinds 0, 1) or ghosts-side (2, 3) list
enum IpcFlag { ARRIVED_FWD = 0, CREDIT_REV = 1, ARRIVED_REV = 2, CREDIT_FWD = 3 };
enum IpcStatus { ST_TIMEOUTS = 0, ST_DEAD = 1, ST_POISONED = 2, ST_WORDS = 8 };

struct IpcChunk {
  int32_t nbr;    // neighbour slot on the side the kernel walks
  int32_t count;  // elements in this chunk
  int64_t start;  // element offset inside the side's concatenated index list
};

struct IpcPeer {       // one per neighbour slot and kernel role, in device memory
  char* data;          // send: my segment inside the neighbour's receive buffer (mapped); recv: my receive buffer
  uint64_t* flag_out;  // send: neighbour's "arrived" flag (mapped);  recv: neighbour's credit flag (mapped)
  uint64_t* flag_in;   // send: my credit flag;                         recv: my "arrived" flag
  int64_t seg_off;     // first element of the neighbour's segment in my concatenated list
  int32_t nchunks;     // workgroups of this neighbour's segment
  int32_t pad_;
};

inline int64_t ipc_align(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// [flags: 4 kinds x nmax slots x 64 B][forward receive buffer: owners.total][reverse receive buffer: ghosts.total]
struct IpcArena {
  char* arena = nullptr;  // its base, in the address space of whoever dereferences it
  int64_t arena_bytes = 0, off_flags = 0, off_recv_fwd = 0, off_recv_rev = 0;
  int nmax = 1;  // flag slots per kind
};

inline IpcArena ipc_arena_layout(const HaloPlan& p, int eb) {
  IpcArena a;
  a.nmax = (int)std::max<size_t>(1, std::max(p.owners.ranks.size(), p.ghosts.ranks.size()));
  a.off_recv_fwd = ipc_align(4ll * a.nmax * kIpcFlagStride, 256);
  a.off_recv_rev = ipc_align(a.off_recv_fwd + p.owners.total * eb, 256);
  a.arena_bytes = ipc_align(a.off_recv_rev + p.ghosts.total * eb, 256) + 256;
  return a;
}

inline uint64_t* ipc_flag_ptr(const IpcArena& a, int kind, int slot) {
  return reinterpret_cast<uint64_t*>(a.arena + a.off_flags + ((int64_t)kind * a.nmax + slot) * kIpcFlagStride);
}

// chunk table of one side: every neighbour's segment cut into pieces of ``chunk`` elements; peers[k] gets its offset and chunk count
inline std::vector<IpcChunk> ipc_cut_chunks(const std::vector<int64_t>& counts, const std::vector<int64_t>& offsets, int chunk,
                                            std::vector<IpcPeer>& peers) {
  std::vector<IpcChunk> ch;
  peers.assign(counts.size(), IpcPeer());
  for (int k = 0; k < (int)counts.size(); ++k) {
    int n = 0;
    for (int64_t s = 0; s < counts[k]; s += chunk, ++n)
      ch.push_back(IpcChunk{k, (int32_t)std::min<int64_t>(chunk, counts[k] - s), offsets[k] + s});
    peers[k].nchunks = n;
    peers[k].seg_off = offsets[k];
  }
  return ch;
}

// Wire neighbour slot ``slot`` of one of my sides: over a slot of my OWNERS side (my ghosts' owners) I receive forward and send reverse,
// over a slot of my GHOSTS side (ranks ghosting my dofs) I send forward and receive reverse.  ``theirs``: the neighbour's arena as I see
// it; ``triples``: the (rank, count, offset) list it exported for its OTHER side, which must list ``my_rank`` with the same count (else
// false, nothing written).  A sender stores at the receiver's offset and publishes "arrived" in the receiver's arena; credit returns.
inline bool ipc_wire_slot(bool owners_side, int64_t count, int slot, int my_rank, const IpcArena& mine, const int64_t* triples,
                          int ntriples, const IpcArena& theirs, int eb, IpcPeer& send, IpcPeer& recv) {
  int ts = -1;
  for (int k = 0; k < ntriples && ts < 0; ++k)
    if (triples[3 * k] == my_rank) ts = k;
  if (ts < 0 || triples[3 * ts + 1] != count) return false;
  const int rdir = owners_side ? 0 : 1, sdir = 1 - rdir;  // the direction I receive / send in over this slot
  auto arrived = [](int dir) { return dir == 0 ? ARRIVED_FWD : ARRIVED_REV; };
  auto credit = [](int dir) { return dir == 0 ? CREDIT_FWD : CREDIT_REV; };
  auto recv_buf = [](const IpcArena& a, int dir) { return a.arena + (dir == 0 ? a.off_recv_fwd : a.off_recv_rev); };
  recv.data = recv_buf(mine, rdir);
  recv.flag_in = ipc_flag_ptr(mine, arrived(rdir), slot);
  recv.flag_out = ipc_flag_ptr(theirs, credit(rdir), ts);
  send.data = recv_buf(theirs, sdir) + triples[3 * ts + 2] * eb;
  send.flag_out = ipc_flag_ptr(theirs, arrived(sdir), ts);
  send.flag_in = ipc_flag_ptr(mine, credit(sdir), slot);
  return true;
}

}  // namespace fus
