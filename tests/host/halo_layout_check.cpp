// Stand-alone check of csrc/halo_layout.hpp (host-only: any C++17 compiler, no HIP, no GPU): the exchange rule, the chunk tables and the
// wiring of PEER arenas, flags and segments on fake arenas (plain host buffers).  tests/test_halo_layout_host.py builds and runs it; it
// is also the program to build with -fsanitize=address,undefined.  Prints HALO_LAYOUT_OK and exits 0.
#include "../../fenicsx-fus-gpu_amd/csrc/halo_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>

using namespace fus;

static int failures = 0;
#define CHECK(cond) \
  if (!(cond)) std::printf("FAILED line %d: %s\n", __LINE__, #cond), ++failures

// ---------------------------------------------------------------------------------------------- the exchange rule
static void exchange_rule() {
  HaloPlan p;
  p.nlocal = 1000;
  int64_t oi = 0, gi = 0;  // stand in for the device index lists: only their addresses matter
  p.owners.idx_d = &oi;
  p.ghosts.idx_d = &gi;
  enum Which { OWNERS, GHOSTS };
  struct End {
    Which side;
    int64_t offset;
    bool gather;
    int mode;
  };
  struct Row {
    int dir;
    bool direct;
    End send, recv;
  };
  // forward sends the ghosts side gathered through ghosts.idx at offset 0 and receives the owners side with SET at offset nlocal,
  // through owners.idx unless direct; reverse sends the owners side at offset nlocal, through owners.idx unless direct, and receives
  // the ghosts side with ADD through ghosts.idx at offset 0, always
  const Row table[4] = {
      {0, false, {GHOSTS, 0, true, PACK}, {OWNERS, 1000, true, UNPACK_SET}},
      {0, true, {GHOSTS, 0, true, PACK}, {OWNERS, 1000, false, UNPACK_SET}},
      {1, false, {OWNERS, 1000, true, PACK}, {GHOSTS, 0, true, UNPACK_ADD}},
      {1, true, {OWNERS, 1000, false, PACK}, {GHOSTS, 0, true, UNPACK_ADD}},
  };
  for (const Row& row : table) {
    p.direct = row.direct;
    const ExchangeEnds x = exchange_ends(p, row.dir);
    const ExchangeEnd* got[2] = {&x.send, &x.recv};
    const End* want[2] = {&row.send, &row.recv};
    for (int e = 0; e < 2; ++e) {
      CHECK(got[e]->side == (want[e]->side == OWNERS ? &p.owners : &p.ghosts));
      CHECK(got[e]->idx == (want[e]->side == OWNERS ? &oi : &gi));
      CHECK(got[e]->offset == want[e]->offset && got[e]->gather == want[e]->gather && got[e]->mode == want[e]->mode);
    }
  }
}

// ---------------------------------------------------------------------------------------------- chunk tables
static void chunk_tables() {
  const int c = 64;
  const std::vector<int64_t> counts = {0, 1, c, c + 1, 3 * c - 1};
  const int want_chunks[5] = {0, 1, 1, 2, 3};
  std::vector<int64_t> offsets(1, 10);  // the first segment need not start at 0
  for (int64_t n : counts) offsets.push_back(offsets.back() + n);
  std::vector<IpcPeer> peers;
  const std::vector<IpcChunk> ch = ipc_cut_chunks(counts, offsets, c, peers);
  CHECK(peers.size() == counts.size() && ch.size() == 7);
  size_t at = 0;
  for (int k = 0; k < (int)counts.size(); ++k) {
    CHECK(peers[k].nchunks == want_chunks[k] && peers[k].seg_off == offsets[k]);
    int64_t next = offsets[k];  // contiguous, in order, covering exactly [offset, offset + count)
    for (int n = 0; n < want_chunks[k] && at < ch.size(); ++n, ++at) {
      CHECK(ch[at].nbr == k && ch[at].start == next && ch[at].count >= 1 && ch[at].count <= c);
      next += ch[at].count;
    }
    CHECK(next == offsets[k] + counts[k]);
  }
  CHECK(at == ch.size());
}

// ---------------------------------------------------------------------------------------------- wiring
struct Rank {
  HaloPlan plan;
  IpcArena arena;
  std::vector<int64_t> triples[2];  // exported (rank, count, offset): [0] owners side, [1] ghosts side
  std::vector<IpcPeer> recv_fwd, send_rev, send_fwd, recv_rev;
};

// ``ghosted[{q, r}]``: how many dofs of rank r rank q ghosts (the entry is listed on both sides even when it is 0)
static void wiring(int nranks, const std::map<std::pair<int, int>, int64_t>& ghosted, int eb) {
  std::vector<Rank> w(nranks);
  for (const auto& [qr, n] : ghosted) {
    Side &o = w[qr.first].plan.owners, &g = w[qr.second].plan.ghosts;
    o.ranks.push_back(qr.second), o.counts.push_back(n);
    g.ranks.push_back(qr.first), g.counts.push_back(n);
  }
  for (Rank& r : w) {
    for (Side* s : {&r.plan.owners, &r.plan.ghosts}) {
      s->offsets.assign(1, 0);
      for (int64_t n : s->counts) s->offsets.push_back(s->offsets.back() + n);
      s->total = s->offsets.back();
      std::vector<int64_t>& t = r.triples[s == &r.plan.ghosts];
      for (size_t k = 0; k < s->ranks.size(); ++k) t.insert(t.end(), {s->ranks[k], s->counts[k], s->offsets[k]});
    }
    r.arena = ipc_arena_layout(r.plan, eb);
    r.arena.arena = static_cast<char*>(std::aligned_alloc(256, (size_t)r.arena.arena_bytes));
    r.recv_fwd.resize(r.plan.owners.ranks.size()), r.send_rev.resize(r.plan.owners.ranks.size());
    r.send_fwd.resize(r.plan.ghosts.ranks.size()), r.recv_rev.resize(r.plan.ghosts.ranks.size());
  }
  for (int q = 0; q < nranks; ++q)
    for (const bool owners_side : {true, false}) {
      const Side& s = owners_side ? w[q].plan.owners : w[q].plan.ghosts;
      for (size_t i = 0; i < s.ranks.size(); ++i) {
        if (s.counts[i] == 0) continue;  // what halo_ipc_connect does: a zero-count neighbour is not wired
        const Rank& nb = w[s.ranks[i]];
        const std::vector<int64_t>& t = nb.triples[owners_side ? 1 : 0];
        CHECK(ipc_wire_slot(owners_side, s.counts[i], (int)i, q, w[q].arena, t.data(), (int)t.size() / 3, nb.arena, eb,
                            owners_side ? w[q].send_rev[i] : w[q].send_fwd[i], owners_side ? w[q].recv_fwd[i] : w[q].recv_rev[i]));
        IpcPeer a{}, b{};  // another count than the neighbour lists: refused, nothing written
        CHECK(!ipc_wire_slot(owners_side, s.counts[i] + 1, (int)i, q, w[q].arena, t.data(), (int)t.size() / 3, nb.arena, eb, a, b));
        CHECK(!a.data && !a.flag_in && !a.flag_out && !b.data && !b.flag_in && !b.flag_out);
      }
    }
  std::vector<std::set<const uint64_t*>> flags(nranks);  // every flag address in use, by the arena it must lie in
  size_t nflags = 0;
  auto slot_of = [](const Side& s, int rank) {
    for (size_t k = 0; k < s.ranks.size(); ++k)
      if (s.ranks[k] == rank) return (int)k;
    return -1;
  };
  for (const auto& [qr, n] : ghosted) {
    if (n == 0) continue;
    const int q = qr.first, r = qr.second;  // q ghosts n dofs of r
    const int i = slot_of(w[q].plan.owners, r), j = slot_of(w[r].plan.ghosts, q);
    // forward: r sends, q receives; reverse: q sends, r receives
    const IpcPeer* sender[2] = {&w[r].send_fwd[j], &w[q].send_rev[i]};
    const IpcPeer* receiver[2] = {&w[q].recv_fwd[i], &w[r].recv_rev[j]};
    const char* recv_buf[2] = {w[q].arena.arena + w[q].arena.off_recv_fwd, w[r].arena.arena + w[r].arena.off_recv_rev};
    const int64_t seg_off[2] = {w[q].plan.owners.offsets[i], w[r].plan.ghosts.offsets[j]};  // the RECEIVER's segment for that sender
    const int arena_of_receiver[2] = {q, r}, arena_of_sender[2] = {r, q};
    for (int dir = 0; dir < 2; ++dir) {
      CHECK(receiver[dir]->data == recv_buf[dir]);
      CHECK(sender[dir]->data == recv_buf[dir] + seg_off[dir] * eb);
      CHECK(sender[dir]->flag_out == receiver[dir]->flag_in);  // arrived
      CHECK(receiver[dir]->flag_out == sender[dir]->flag_in);  // credit
      flags[arena_of_receiver[dir]].insert(receiver[dir]->flag_in);
      flags[arena_of_sender[dir]].insert(sender[dir]->flag_in);
      nflags += 2;
    }
  }
  size_t distinct = 0;
  for (int q = 0; q < nranks; ++q) {
    const IpcArena& a = w[q].arena;
    const char *fwd0 = a.arena + a.off_recv_fwd, *fwd1 = fwd0 + w[q].plan.owners.total * eb;
    const char *rev0 = a.arena + a.off_recv_rev, *rev1 = rev0 + w[q].plan.ghosts.total * eb;
    CHECK(fwd1 <= rev0 && rev1 <= a.arena + a.arena_bytes);
    CHECK((uintptr_t)fwd0 % 256 == 0 && (uintptr_t)rev0 % 256 == 0);
    for (const uint64_t* f : flags[q]) {
      const int64_t at = reinterpret_cast<const char*>(f) - (a.arena + a.off_flags);
      CHECK(at >= 0 && at % kIpcFlagStride == 0 && at < 4ll * a.nmax * kIpcFlagStride);      // one per 64-byte line of the flag region
      CHECK(reinterpret_cast<const char*>(f + 1) <= fwd0 && a.off_flags + at + 8 <= a.off_recv_fwd);  // in front of both receive buffers
    }
    distinct += flags[q].size();
  }
  CHECK(distinct == nflags);  // no two roles share a flag
  for (Rank& r : w) std::free(r.arena.arena);
}

int main() {
  exchange_rule();
  chunk_tables();
  for (const int eb : {8, 4}) {
    // a line of three ranks, rank 1 borders both others, unequal counts; rank 0 lists rank 2 (and rank 2 rank 0) with no dofs
    wiring(3, {{{0, 1}, 5}, {{1, 0}, 3}, {{1, 2}, 130}, {{2, 1}, 7}, {{0, 2}, 0}}, eb);
    wiring(1, {{{0, 0}, 9}}, eb);  // a one-rank world that is its own neighbour
    // a star: four flag slots per kind on rank 0, so that the flag region ends exactly where the first receive buffer starts
    wiring(5, {{{0, 1}, 2}, {{0, 2}, 3}, {{0, 3}, 4}, {{0, 4}, 5}, {{1, 0}, 6}, {{2, 0}, 7}, {{3, 0}, 8}, {{4, 0}, 70}}, eb);
  }
  if (failures) return 1;
  std::printf("HALO_LAYOUT_OK\n");
  return 0;
}
