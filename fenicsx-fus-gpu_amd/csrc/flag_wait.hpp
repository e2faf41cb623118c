// The bounded wait for a sequence flag of THIS device, shared by the fork / join wait kernel (comm_sync.hpp) and the
// first send kernel of an apply, which waits for the fork flag itself (halo_ipc.hpp).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "halo_layout.hpp"  // the status words

namespace fus {

// wait for *flag >= seq at agent scope, by one thread; a time-out is counted in ``status`` and ends every later wait at once
__device__ inline void stream_flag_wait(const uint64_t* flag, uint64_t seq, uint64_t* status, uint64_t budget) {
  if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= seq) return;
  if (__hip_atomic_load(&status[ST_DEAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const uint64_t t0 = wall_clock64();
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < seq) {
    __builtin_amdgcn_s_sleep(2);
    if (wall_clock64() - t0 > budget) {
      atomicAdd((unsigned long long*)&status[ST_TIMEOUTS], 1ull);
      __hip_atomic_store(&status[ST_DEAD], (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
}

}  // namespace fus
