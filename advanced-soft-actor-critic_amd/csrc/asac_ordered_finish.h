// The ordered cross-workgroup finish: every workgroup of a launch PUBLISHES partial sums in a workspace and ARRIVES at a counter;
// the last one to arrive COLLECTS the partials in workgroup order (a fixed order and no float atomics: equal inputs give equal
// bits), writes the result and RESETS the counter for the next launch.  This header is the only place that exchange is written.
//
// Why relaxed accesses and a wait are enough on gfx950.  The chip has eight XCDs whose L2s are not coherent with each other, and
// a CU's L1 is never refreshed by another CU's stores.  A relaxed agent-scope atomic store or load is a `global_store` /
// `global_load ... sc1`: the store is written through to the memory all XCDs share, the load passes L1 and any L2 copy.
// `s_waitcnt vmcnt(0)` returns once the wave's stores are acknowledged from there, and the barrier puts every wave's wait in
// front of the workgroup's one `fetch_add`, performed at that same level.  The workgroup that reads nb - 1 from the counter
// thus knows that every other workgroup's partials arrived before its add did; its own loads are issued after that answer (they
// depend on it through LDS and a barrier) and no stale line or scalar cache can serve them, as none is a plain load.  Hence the
// rule: EVERYTHING the last arriver reads from another workgroup is stored by finish_publish and loaded by finish_load /
// finish_sum_in_order, through pointers without `__restrict__`.  The wait is the asm statement with its "memory" clobber:
// the compiler keeps the stores in front of it and the add behind, which `__builtin_amdgcn_s_waitcnt` does not promise.
//
// Why no release or acquire fence (`__threadfence()` is both).  An agent-scope release writes back EVERY dirty line of the
// XCD's L2 — in these kernels the gradient the same launch is streaming out (NOTES.md, "An agent-scope RELEASE writes back
// the XCD's whole L2") — which costs microseconds per workgroup, more when all 256 threads issue it; an acquire invalidates an
// L1 that no load here goes through.  Neither repairs a plain store or load of an exchanged word.
//
// State.  Only the counter word must be ZERO before the first launch on a workspace; every launch leaves it zero (hipGraph
// replays included: the reset is part of the kernel).  The partial slots need no initial value: each launch rewrites all nb
// of them before the counter reaches nb.  One workspace per concurrently running launch.  Nothing here waits for another
// workgroup — no loop polls — so nothing can spin, whatever the dispatch order or residency.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asac {

// publish: one partial to its slot (wider values: one store per float)
__device__ __forceinline__ void finish_publish(float* slot, float v) { __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float finish_load(float* slot) { return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// reset: by ONE lane of the last arriver, after its collection
__device__ __forceinline__ void finish_reset(unsigned int* counter) { __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// arrive: called by EVERY thread of the workgroup after its finish_publish calls; true in every thread of the last workgroup
// (`expected`: how many workgroups arrive at this counter — the grid's x extent unless the caller says otherwise)
__device__ __forceinline__ bool finish_arrive(unsigned int* counter, unsigned int expected) {
    __shared__ bool last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // every wave: its own stores have arrived
    __syncthreads();
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == expected - 1;
    __syncthreads();
    return last;
}
__device__ __forceinline__ bool finish_arrive(unsigned int* counter) { return finish_arrive(counter, gridDim.x); }

// two-level arrival, for launches of many short workgroups that publish NOTHING and only need to know who is last (the draw
// counter of asac_dropout.h: a workgroup's part is a LOAD it has already waited for).  Arrivals at one word are served one
// after the other by the memory side (about 30 ns each, csrc/image.hip) — and so are arrivals at different words of one
// 128-byte line — so workgroup g arrives at leaf word g % n_leaves (n_leaves a power of two; the words `leaf_stride` uint32
// apart: 32 or more puts each in a line of its own); the last one at a leaf resets it and arrives at the root; the last one
// there resets the root.
// Called by ONE lane of the workgroup, behind its own wait; true in the launch's last arriver.  Both levels end a launch
// zero, as above, and nothing waits for another workgroup.
__device__ __forceinline__ bool finish_arrive_two_level(unsigned int* leaves, unsigned int n_leaves, unsigned int leaf_stride,
                                                        unsigned int* root) {
    const unsigned int nb = gridDim.x, leaf = blockIdx.x & (n_leaves - 1);
    const unsigned int at_leaf = nb / n_leaves + (leaf < (nb & (n_leaves - 1)) ? 1u : 0u);      // workgroups g < nb with g % n_leaves == leaf
    unsigned int* const mine = leaves + leaf * leaf_stride;
    if (__hip_atomic_fetch_add(mine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != at_leaf - 1) return false;
    finish_reset(mine);
    const unsigned int used_leaves = nb < n_leaves ? nb : n_leaves;
    if (__hip_atomic_fetch_add(root, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != used_leaves - 1) return false;
    finish_reset(root);
    return true;
}

// collect: base[0] + base[stride] + .. + base[(count - 1) * stride], added in that order by the calling lane; sixteen loads
// requested at a time (one by one, each add waits for its own trip to memory; indices beyond `count` re-read the last slot: a
// valid address, the value is not added)
__device__ __forceinline__ float finish_sum_in_order(float* base, int64_t stride, int count) {
    float s = 0.f;
    for (int b0 = 0; b0 < count; b0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = finish_load(base + (int64_t)min(b0 + u, count - 1) * stride);
#pragma unroll
        for (int u = 0; u < 16; ++u) s += b0 + u < count ? v[u] : 0.f;
    }
    return s;
}

}  // namespace asac
