// shine_arrive.hpp — the one hand-off between workgroups inside a launch: "every workgroup leaves a partial in a workspace, the
// last one to arrive sums them" (the loss sums of shine_loss_modes.hip, the metric sums of shine_eval.hip, both ticket levels of
// the semantic head's weight gradients, shine_sem_head.hpp).
//
// Contract of arrive_last(counter, expected, verdict):
//   - who may call: every thread of a workgroup, in block-uniform control flow; `expected` workgroups call it on `counter`.
//   - returns, to every thread of the workgroup alike, whether this workgroup is the last of the `expected` to arrive.
//   - published: every global store that any thread of a workgroup issued before its call is visible to every thread of the last
//     arriver after the call returns true — wherever the two workgroups ran (the eight XCDs' L2s are not coherent with each
//     other, a CU's L1 is never refreshed by another CU's stores).  Both sides use plain vector accesses at per-lane addresses:
//     a block-uniform load may take the scalar cache, which the acquire does not invalidate.
//   - *counter is zero before the first arrival and is not reset here: a caller whose workspace is to stay zero stores 0 from the
//     last arriver (nobody else touches the counter any more), or its entry point clears the word in front of every launch.
//   - `verdict`: one LDS word of the caller's that no thread reads or writes around the call.
//   - it never waits for another workgroup: nothing spins, so no workgroup needs to be resident with another.
//
// The order of the steps is the point.  Release: every wave drains its own stores, the barrier gathers the waves, ONE lane
// writes the L2 back (agent-scope release) and waits for that write-back itself — the compiler may fold the fence's own wait
// away — before it takes the ticket.  Acquire: ONE lane of the last arriver invalidates the CU's L1, waits, and the barrier holds
// the other waves' loads behind it.
#pragma once
#include <hip/hip_runtime.h>

namespace shine {

__device__ __forceinline__ bool arrive_last(unsigned* counter, unsigned expected, unsigned* verdict) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *verdict = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == expected - 1;
  }
  __syncthreads();
  if (!*verdict) return false;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  return true;
}

}  // namespace shine
