// PEER transport of the ghost-dof halo exchange: no RCCL kernel, no copy engine call, no host in the loop.
//
// This file is the device code; the host side (arenas, chunk tables, blobs, posting) is halo_peer.hpp.
//
// Why (profiles/r02z_overlap_probe.log, r03a_*): RCCL's send/recv kernel needs 264 VGPRs per lane and is not scheduled
// next to an operator launch that holds every vector register of every CU, so an exchange posted "under" interior cells
// ran after them (+41..46 us per apply).  hipMemcpyAsync into peer-mapped memory costs 150 us per hop on this runtime
// (r03a_ipc_probe.log).  What does run next to the operator is a kernel of a few registers.  So each rank maps its
// neighbours' receive arenas once (hipIpcGetMemHandle / hipIpcOpenMemHandle: xGMI stores between GPUs, plain stores
// inside one GPU), and an exchange is two small kernels per rank:
//
//   send  (workgroup = up to 8192 message elements of ONE neighbour): wait until that neighbour has consumed the previous
//         message (credit flag in MY arena), gather the elements from the vector and store them straight into the
//         neighbour's receive buffer (write-through stores), wait for their acknowledgement; the last workgroup of a
//         neighbour's segment publishes the exchange's sequence number in the neighbour's "arrived" flag;
//   recv  wait (bounded) for the "arrived" flag of the chunk's neighbour in MY arena, read the chunk with system-scope
//         loads, store (forward) or atomically add (reverse) it into the vector; the last workgroup of a segment
//         returns the credit to the sender's arena.
//
// Flags carry sequence numbers (exchange 1, 2, ...), so nothing depends on the order in which the processes' hosts
// issue their calls, and the hosts never synchronise with each other after the one-off exchange of the arena handles.
// The arenas are uncached device memory (what RCCL's own peer-to-peer flag buffers are on this architecture), so a reader
// never sees a stale cache line.
//
// Host-side contract (the one MPI's non-blocking collectives and RCCL have too): ALL RANKS POST THE EXCHANGES OF A
// COMMUNICATOR IN THE SAME ORDER.  Send and receive kernels share the communicator's one stream by default, so rank A
// posting (halo 1, halo 2) while rank B posts (halo 2, halo 1) is a cycle: A's receive 1 waits for B's send 1, which is
// queued behind B's receive 2, which waits for A's send 2, queued behind A's receive 1.  (FUS_IPC_TWO_STREAMS=1 puts the
// receive kernels on a stream of their own -- a send never waits for remote data -- at the price of an event edge per
// exchange; the drivers of this repository post in program order on every rank and do not need it.)
//
// Every wait is bounded (FUS_IPC_SPIN_SECONDS, default 20 s of the device's wall clock) and A FAILED EXCHANGE IS LOUD ON
// BOTH SIDES: on a time-out the kernel records it in the halo's status words, stops waiting for the rest of the run,
// drains -- and every flag this halo publishes from then on carries the POISON bit (bit 63).  A neighbour that reads a
// poisoned flag does not consume the arena (stale data), counts it (ST_POISONED), becomes dead itself and poisons what it
// publishes: the failure reaches every rank connected to the one that timed out within a few exchanges, and
// fus_halo_ipc_status() != 0 there.  The solvers / demos / C++ host check it at the end of every rk4() call and raise.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "flag_wait.hpp"    // stream_flag_wait: the fork flag, waited for by the first send kernel of an apply itself
#include "halo.hpp"
#include "halo_layout.hpp"  // IpcChunk, IpcPeer, the flag and status words

namespace fus {

// Workgroup shape of the exchange kernels (FUS_IPC_THREADS x FUS_IPC_CHUNK message elements per workgroup), measured
// next to the config-3 operator launch with config-4 messages (profiles/r03f_sweep.log, exposed cost of both exchanges
// of an apply): 64..512 threads with 512..4096 elements all cost the same 11-13 us; 256-element workgroups cost 22 (too
// many), 1024-thread workgroups 50 (a workgroup that needs 16 wave slots of one CU at once waits long for them next to
// an operator that fills every CU).  Default 256 x 1024: the footprint of the operator workgroup it displaces.
constexpr int kIpcMaxThreads = 1024;
constexpr int kIpcEpt = 8;  // elements per thread at most: all loads issued before the first store
inline int ipc_env_int(const char* name, int dflt, int lo, int hi) {
  const char* v = std::getenv(name);
  const int x = v ? std::atoi(v) : dflt;
  return x < lo ? lo : (x > hi ? hi : x);
}
// workgroup size and message elements per workgroup of the exchange kernels (chunk <= threads * kIpcEpt)
inline int ipc_threads() {
  static const int t = ipc_env_int("FUS_IPC_THREADS", 256, 64, kIpcMaxThreads) / 64 * 64;
  return t;
}
inline int ipc_chunk() {
  static const int c = ipc_env_int("FUS_IPC_CHUNK", 1024, 64, ipc_threads() * kIpcEpt);
  return c;
}
constexpr uint64_t kIpcPoison = 1ull << 63;  // in a flag: the publisher's halo has failed (time-out here or upstream)

// Memory ordering without fences.  A release / acquire fence at agent or system scope is an L2 write-back / invalidate on
// gfx942 / gfx950 (buffer_wbl2 / buffer_inv): issued by every workgroup of an exchange next to an operator launch whose
// scatter-adds keep the L2 full of dirty lines it cost +75 us per exchange (profiles/r03b_overlap.log).  Instead every
// access to an arena is a RELAXED SYSTEM-SCOPE atomic -- a write-through store / cache-bypassing load (sc0 sc1) on memory
// that is fine-grained anyway -- and the order "data before flag" is kept by waiting for the stores' acknowledgements
// (s_waitcnt vmcnt(0)) before the workgroup barrier that precedes the flag store; on the reader's side the data loads
// are issued after the barrier that follows the flag load.
__device__ inline uint64_t ipc_load_flag(const uint64_t* f) {
  return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ inline void ipc_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// FENCED variant of the same protocol (FUS_IPC_FENCED=1 when the halo object is created; bench.py's ladder tries it as "peer:fenced" after
// a PEER transport that came up but failed the run's halo check ON DATA): the conservatively ordered form of the microarchitecture
// guide's hand-off -- producer: every storing wave's s_waitcnt vmcnt(0), the workgroup barrier, then ONE lane's SYSTEM-scope release
// (L2 write-back) + s_waitcnt vmcnt(0) before the relaxed flag store; consumer: ONE relaxed poll, then ONE lane's system-scope acquire
// (cache invalidate) + s_waitcnt vmcnt(0) before the workgroup barrier that precedes the data loads.  The fence-free default rests on
// every arena access being a write-through / cache-bypassing system-scope atomic on uncached memory; should that not hold between two
// DIFFERENT devices (never run on this pool: one GPU per box), this rung costs two fences per workgroup instead of RCCL's 40 us per apply.
__device__ inline void ipc_release_system() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the compiler may drop the wait behind buffer_wbl2 when it thinks the scoreboard empty)
}
__device__ inline void ipc_acquire_system() {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate completes asynchronously: hold the barrier until it has
}

// Wait until *flag >= want.  Bounded: gives up after ``budget`` wall-clock ticks, or at once if an earlier wait of this
// halo has already failed.  A poisoned flag (the publisher's halo is dead) ends the wait at once, is counted and kills this
// halo too.  Returns 1 only if the data behind the flag may be consumed.
__device__ inline int ipc_wait(const uint64_t* flag, uint64_t want, uint64_t* status, uint64_t budget) {
  uint64_t v = ipc_load_flag(flag);
  if (!(v & kIpcPoison) && v >= want) return 1;
  const uint64_t t0 = wall_clock64();
  for (;;) {
    if (v & kIpcPoison) {
      atomicAdd((unsigned long long*)&status[ST_POISONED], 1ull);
      __hip_atomic_store(&status[ST_DEAD], (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return 0;
    }
    if (v >= want) return 1;
    if (__hip_atomic_load(&status[ST_DEAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0;
    __builtin_amdgcn_s_sleep(4);
    if (wall_clock64() - t0 > budget) {
      atomicAdd((unsigned long long*)&status[ST_TIMEOUTS], 1ull);
      __hip_atomic_store(&status[ST_DEAD], (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return 0;
    }
    v = ipc_load_flag(flag);
  }
}

// last workgroup of a neighbour's segment publishes ``seq`` in ``flag_out`` -- poisoned if this halo has failed
__device__ inline void ipc_segment_done(unsigned* counter, int nchunks, uint64_t* flag_out, uint64_t seq, const uint64_t* status) {
  const unsigned done = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (done == (unsigned)nchunks - 1u) {  // every other workgroup's stores were acknowledged before it counted itself
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t dead = __hip_atomic_load(&status[ST_DEAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(flag_out, dead ? (seq | kIpcPoison) : seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// A kernel's last workgroup publishes ``seq`` in a flag of THIS device: the join flag of the communicator, folded into the
// last receive kernel of an apply instead of a signal kernel of its own.  Every workgroup has waited for its own stores /
// atomics (s_waitcnt vmcnt(0)) before it counts itself.
struct IpcJoin {
  uint64_t* flag;     // nullptr: nothing to publish
  uint64_t seq;
  unsigned* counter;  // zero between launches
};
__device__ inline void ipc_kernel_done(const IpcJoin& j) {
  if (!j.flag) return;
  const unsigned done = __hip_atomic_fetch_add(j.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (done == gridDim.x - 1u) {
    __hip_atomic_store(j.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(j.flag, j.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct IpcGate {
  const uint64_t* flag;  // nullptr: no gate
  uint64_t seq;
  uint64_t* status;      // the communicator's fork / join status words
};

template <typename T>
__device__ inline T ipc_load_elem(const T* p);
template <typename T>
__device__ inline void ipc_store_elem(T* p, T v);
template <>
__device__ inline void ipc_store_elem<double>(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<uint64_t*>(p), (uint64_t)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <>
__device__ inline void ipc_store_elem<float>(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<uint32_t*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <>
__device__ inline double ipc_load_elem<double>(const double* p) {
  const uint64_t u = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return __longlong_as_double((long long)u);
}
template <>
__device__ inline float ipc_load_elem<float>(const float* p) {
  const uint32_t u = __hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return __uint_as_float(u);
}

// an empty, unconditional use of loaded values (keeps their loads where they were issued)
template <typename V, int N>
__device__ __forceinline__ void ipc_pin(V (&a)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) asm volatile("" : "+v"(a[k]));
}

// GATHER: element i of the message is vec[index[i] + offset]; otherwise vec[offset + i] (ghosts numbered owner by owner)
template <typename T, bool GATHER>
__global__ void __launch_bounds__(kIpcMaxThreads)
    ipc_send_kernel(const T* __restrict__ vec, const int64_t* __restrict__ index, int64_t offset,
                    const IpcChunk* __restrict__ chunks, const IpcPeer* __restrict__ peers, unsigned* counters,
                    uint64_t* status, uint64_t seq, uint64_t budget, IpcGate gate, int fenced) {
  const IpcChunk c = chunks[blockIdx.x];
  const IpcPeer p = peers[c.nbr];
  __shared__ int ok;
  if (threadIdx.x == 0) {
    if (gate.flag) stream_flag_wait(gate.flag, gate.seq, gate.status, budget);  // the caller's stream has produced the vector
    ok = ipc_wait(p.flag_in, seq - 1, status, budget);                       // the neighbour has consumed message seq-1
  }
  __syncthreads();
  if (ok) {
    T* dst = reinterpret_cast<T*>(p.data) + (c.start - p.seg_off);
    // Two round trips for the whole chunk -- every index, then every value -- not two per element: the loads are issued by every
    // thread with a clamped element (a thread beyond the chunk re-reads its first element) instead of under ``e < count``, where the
    // compiler waits for each index inside its own block (16 serial round trips for 8 elements per thread; the same rule as the
    // preamble of the planned kernels, plan.hpp)
    int64_t src[kIpcEpt];
    T v[kIpcEpt];
    if (c.count > 0) {  // block-uniform
#pragma unroll
      for (int k = 0; k < kIpcEpt; ++k) {
        const int e = (int)threadIdx.x + k * (int)blockDim.x;
        const int64_t i = c.start + (e < c.count ? e : 0);
        src[k] = GATHER ? index[i] : i;
      }
#pragma unroll
      for (int k = 0; k < kIpcEpt; ++k) v[k] = vec[src[k] + offset];
      ipc_pin(v);  // (an empty use: the compiler would sink each load into the block of its store again)
#pragma unroll
      for (int k = 0; k < kIpcEpt; ++k) {
        const int e = (int)threadIdx.x + k * (int)blockDim.x;
        if (e < c.count) ipc_store_elem<T>(dst + e, v[k]);
      }
    }
  }
  ipc_stores_done();  // my stores have reached the neighbour's memory before the flag can
  __syncthreads();
  if (threadIdx.x == 0) {
    if (fenced) ipc_release_system();
    ipc_segment_done(&counters[c.nbr], p.nchunks, p.flag_out, seq, status);
  }
}

// MODE: UNPACK_SET (forward: ghosts overwritten) or UNPACK_ADD (reverse: partial sums added into the owners' entries)
template <typename T, int MODE, bool GATHER>
__global__ void __launch_bounds__(kIpcMaxThreads)
    ipc_recv_kernel(T* __restrict__ vec, const int64_t* __restrict__ index, int64_t offset,
                    const IpcChunk* __restrict__ chunks, const IpcPeer* __restrict__ peers, unsigned* counters,
                    uint64_t* status, uint64_t seq, uint64_t budget, IpcJoin join, int fenced) {
  const IpcChunk c = chunks[blockIdx.x];
  const IpcPeer p = peers[c.nbr];
  __shared__ int ok;
  if (threadIdx.x == 0) {
    ok = ipc_wait(p.flag_in, seq, status, budget);  // the neighbour's message seq is complete
    if (fenced) ipc_acquire_system();
  }
  __syncthreads();
  if (ok) {
    const T* src = reinterpret_cast<const T*>(p.data);
    T v[kIpcEpt];
    int64_t j[kIpcEpt];
    if (c.count > 0) {  // block-uniform; loads by every thread with a clamped element: one round trip for the chunk (see ipc_send_kernel)
#pragma unroll
      for (int k = 0; k < kIpcEpt; ++k) {
        const int e = (int)threadIdx.x + k * (int)blockDim.x;
        const int64_t i = c.start + (e < c.count ? e : 0);
        v[k] = ipc_load_elem<T>(src + i);
        j[k] = GATHER ? index[i] : i;
      }
      ipc_pin(j);
#pragma unroll
      for (int k = 0; k < kIpcEpt; ++k) {
        const int e = (int)threadIdx.x + k * (int)blockDim.x;
        if (e < c.count) {
          if constexpr (MODE == UNPACK_SET)
            vec[j[k] + offset] = v[k];
          else
            unsafeAtomicAdd(vec + j[k] + offset, v[k]);
        }
      }
    }
  }
  if (join.flag) ipc_stores_done();  // my stores / adds into the vector have been performed before the join flag can say so
  __syncthreads();                   // every load of this chunk has been consumed
  if (threadIdx.x == 0) {
    ipc_segment_done(&counters[c.nbr], p.nchunks, p.flag_out, seq, status);
    ipc_kernel_done(join);
  }
}

}  // namespace fus
