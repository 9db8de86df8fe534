// handover.hpp — the inter-workgroup hand-over of k_pconv_coop (pconv_coop.hip) and k_dconv_block (dconv_block.hip): several
// workgroups store partial results, the one that arrives LAST at a counter reads them all and finishes the block.  No
// workgroup ever waits for another one: nothing spins.  (An extension: the reference sums with CAS atomics instead,
// cl_conv_kernels.h:102-118, cl_dconv.cpp:32-43.)  tools/check_isa.py --handover audits the compiled form of both kernels.
#pragma once
#include "cpx.hpp"

namespace clfa {

// Hand-over protocol (MI355X_MICROARCH.md, "Valid forms"): slices stored with agent-scope (sc1) stores, every
// storing wave s_waitcnt vmcnt(0), workgroup barrier, ONE lane's agent-scope atomic add on the channel's counter;
// the workgroup whose add returns S - 1 reads every slice with agent-scope (sc1) loads after its own barrier.
// The hand-overs are written for gfx950's memory pipeline (sc1 stores write through, vmcnt counts stores, sc1 loads
// are served past the CU's L1): another target needs the C++ release / acquire forms instead.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "handover.hpp: the inter-workgroup hand-overs are gfx950-specific (see MI355X_MICROARCH.md, 'Valid forms')"
#endif
// The form without an acquire is the one MI355X_MICROARCH.md measured ("Valid forms": sc1 stores, every storing wave's
// vmcnt(0), barrier, one lane's agent-scope add; the workgroup whose add came last loads with sc1 loads) — for launches of
// at most ONE workgroup per CU.  A launch with more workgroups than CUs (acquire != 0, set by the launcher) is outside
// that table: there the arriving lane of the last workgroup runs the documented consumer form as well — one agent-scope
// acquire (buffer_inv sc1) and its wait, in front of the barrier that releases the other waves' loads.
__device__ __forceinline__ void handover_acquire(int acquire) {
  if (acquire) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}
// The arriving lane's add carries the C++ model's release as well: the hand-written form above
// orders the slice stores in hardware, but nothing in it tells hipcc that they must stay above the add — with the
// release a future compiler cannot sink a slice store below the counter.  On gfx950 it costs a buffer_wbl2 sc1 and a wait
// in ONE lane after the barrier (profiles/handover_release_r05.txt).
__device__ __forceinline__ unsigned handover_arrive(unsigned *counter) {
  return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(cpx *p, cpx v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ cpx ld_agent(const cpx *p) {
  return __builtin_bit_cast(cpx, __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_agent_f(float *p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_agent_f(const float *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace clfa
