// Dropout draws decided on the device: the one contract every kernel that drops elements shares, so that a mask is never
// stored — the backward regenerates the forward's from the call counter the forward used — and a captured launch draws
// afresh on every replay (a host draw would be baked into the graph).
//
// A draw is a function of (seed, instance id, call counter, element) and of nothing else: not of the grid, not of which
// wave or lane asks.  One Philox4x32-10 block serves FOUR neighbouring elements (the four a lane holds in one f32x4):
//   counter words  (index, (kDropTag << 28) | (instance & 0x0FFFFFFF), call counter lo, call counter hi)
//   key            the seed (lo, hi)
//   element e      block index e >> 2, word e & 3;  KEPT iff word >= thr
//   thr            floor(p * 2^32), formed in float64 on the host  (P(dropped) = thr / 2^32; p in (0, 1) -> thr < 2^32)
//   kept elements are multiplied by s = float32(1 / (1 - p)), the quotient formed in double precision (ATen's `dropout`)
// Tags 0..4 of the second word belong to csrc/image.hip, 5 (kDropTag, dropout_factors4 below) to the attention weights of
// csrc/attn_mh.hip, 6..9 to the dense stacks of csrc/rows_proj.hip (its row_factors4): there element (row r, feature f) of a
// [rows][E] tensor uses block index r * (E / 4) + (f >> 2), word f & 3 — 6 / 7 / 8 the q / k / v stack with r = b * L + t, the
// position in the FULL window (a draw does not depend on how many newest positions a job covers), 9 the output block with r
// the flat row; rows * E < 2^34.  Every drawing launch SITE owns a state (one state per concurrently running launch).
// tests/dense_dropout_ref.py restates that layout.  The instance ids come from the one counter of
// algorithm/utils/image_transforms.py, so no two modules of a process share a stream.
// tests/attn_dropout_ref.py restates this in NumPy.
//
// The call counter is device state of the module instance (an int64 behind `state`), advanced by the launch itself:
// see dropout_counter_begin below.
#pragma once
#include "asac_noise.h"
#include "asac_ordered_finish.h"

namespace asac {

constexpr uint32_t kDropTag = 5u;
constexpr int kDropLeaves = 32;                       // arrival words in front of the root (a power of two)
// A module's draw state, in int64 words: [0] the call counter, [16] the root arrival word, [32 + 16 g] leaf arrival word g
// (the first 32 bits of each) — every word that is arrived at in a 128-byte line of its own.  Measured (NOTES.md, "Attention
// dropout"): with the 32 leaves side by side in one line the forward launch of 1 024 workgroups cost 6.1 - 7.7 us more than
// the launch without dropout, hardly less than with ONE word (11 - 12 us); a line each, 1.0 - 3.1 us.
constexpr int kDropLine = 16;
constexpr int kDropStateWords = 2 * kDropLine + kDropLeaves * kDropLine;

struct DropDraw {
    uint64_t seed;
    uint64_t counter;
    uint32_t instance;
    uint32_t thr;
    float scale;
};

// the factors (0 or s) of elements 4 * block .. 4 * block + 3
__device__ __forceinline__ void dropout_factors4(const DropDraw& d, uint32_t block, float f[4]) {
    const Philox x = philox4x32_10(block, (kDropTag << 28) | (d.instance & 0x0FFFFFFFu), (uint32_t)d.counter,
                                   (uint32_t)(d.counter >> 32), (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
#pragma unroll
    for (int r = 0; r < 4; ++r) f[r] = x.c[r] >= d.thr ? d.scale : 0.f;
}

// The counter exchange of a drawing launch, by ONE lane of every workgroup, in two steps so that other work can stand
// between them: read the call counter (one load past the caches) ...
__device__ __forceinline__ int64_t dropout_counter_load(int64_t* state) {
    return __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... and, once the value `c` has come back, arrive.  Workgroup 0 records it in `used` (what the backward launch reads, and
// what tests ask for); the last arriver stores c + 1 (`advance`: not under the measurement repeat knob, whose repetitions
// draw alike) — by then every workgroup holds its copy.  Nothing waits for another workgroup.
__device__ __forceinline__ void dropout_counter_arrive(int64_t* state, int64_t* used, int64_t c, bool advance) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the value is here before the arrival leaves
    if (blockIdx.x == 0) *used = c;
    unsigned int* const root = reinterpret_cast<unsigned int*>(state + kDropLine);
    unsigned int* const leaves = reinterpret_cast<unsigned int*>(state + 2 * kDropLine);
    if (finish_arrive_two_level(leaves, kDropLeaves, 2 * kDropLine, root)) {
        if (advance) __hip_atomic_store(state, c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace asac
