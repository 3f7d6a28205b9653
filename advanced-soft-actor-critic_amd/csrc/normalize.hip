// Observation normalization for gfx950 (`use_normalization`, reference sac_base.py:302-336, 766-781): the whitening of
// every observation of a call as ONE launch, and the running statistics' update over an episode as ONE launch.  C ABI in
// include/asac_hip.h.  Both are memory-bound; every store is a plain vector store.
//
// Whiten.  The work is flattened over (job, row, unit) as in gather.hip, unit = 16 bytes where the job's D, pitches and
// pointers allow it, else 4: consecutive lanes touch consecutive addresses whatever D is.  mean / variance (<= 21 168 floats
// for an 84 x 84 x 3 frame) come through the read-only path; `step` is one scalar load.  Nothing of the statistics is in the
// launch's arguments but their addresses.
//
// Update.  A workgroup owns kNormCols consecutive columns of one job and all T rows of them: thread (c, g) of the 64 x 4
// workgroup reads column c of the rows t = g (mod 4) — a wave reads 64 consecutive elements of a row — and keeps 16
// accumulators, one per LOGICAL row lane l = t mod 64 = g + 4 k.  The 64 lane partials of a column are then combined by
// the tree p[l] += p[l + off], off = 32 .. 1: offsets 32 .. 4 inside the thread (k + 8, + 4, + 2, + 1), offsets 2 and 1
// through LDS.  The mean's sum first, the variance's in a second walk over the rows (it needs mean').  The old `step` is
// read by every workgroup before it arrives at the counter; the last arriver writes step + T (asac_ordered_finish.h).
#include "asac_common.h"
#include "asac_ordered_finish.h"

namespace asac {

constexpr int kNormBlock = 256;
constexpr int kNormCols = 64;                               // columns of a workgroup of the update
constexpr int kNormGroups = kNormBlock / kNormCols;         // row groups g of a workgroup
constexpr int kNormAcc = ASAC_NORM_ROW_LANES / kNormGroups; // accumulators (logical lanes) of a thread
static_assert(kNormGroups == 4 && kNormAcc == 16, "the tree below is written for 64 lanes = 4 groups x 16");

struct WhitenJobDev {
    const float* src;
    float* dst;
    const float* mean;
    const float* variance;
    int64_t src_pitch, dst_pitch;     // elements
    uint32_t units_per_row;
    uint32_t total_units;
    uint32_t first_block;
    int32_t vec;                      // 1: 16-byte units
};

struct WhitenLaunch {
    WhitenJobDev job[ASAC_NORM_MAX_OBS];
    const int32_t* step;
    int32_t n_jobs;
};

// torch.clamp(v, -5, 5): NaN stays NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float whiten1(float x, float mean, float variance, float count) {
    const float v = (x - mean) / sqrtf(variance / count);
    return v < -5.f ? -5.f : (v > 5.f ? 5.f : v);
}

__global__ __launch_bounds__(kNormBlock) void k_obs_whiten(const WhitenLaunch by_value) {
    const ASAC_KARG WhitenLaunch& m = *static_cast<const ASAC_KARG WhitenLaunch*>(kernarg_base());
    int q = 0;
    for (int i = 1; i < m.n_jobs; ++i)
        if (blockIdx.x >= m.job[i].first_block) q = i;
    const WhitenJobDev j = karg_copy(&m.job[q]);
    const uint32_t u = (blockIdx.x - j.first_block) * kNormBlock + threadIdx.x;
    if (u >= j.total_units) return;
    // (int32 `step + 1` as torch forms it — wrapping — then rounded to float by the promotion of the division)
    const float count = (float)(int32_t)((uint32_t)*m.step + 1u);
    const uint32_t row = u / j.units_per_row, c = u - row * j.units_per_row;
    if (j.vec) {
        const float4 x = *reinterpret_cast<const float4*>(j.src + (int64_t)row * j.src_pitch + 4 * (int64_t)c);
        const float4 mu = __ldg(reinterpret_cast<const float4*>(j.mean) + c);
        const float4 var = __ldg(reinterpret_cast<const float4*>(j.variance) + c);
        float4 y;
        y.x = whiten1(x.x, mu.x, var.x, count);
        y.y = whiten1(x.y, mu.y, var.y, count);
        y.z = whiten1(x.z, mu.z, var.z, count);
        y.w = whiten1(x.w, mu.w, var.w, count);
        *reinterpret_cast<float4*>(j.dst + (int64_t)row * j.dst_pitch + 4 * (int64_t)c) = y;
    } else {
        const float x = j.src[(int64_t)row * j.src_pitch + c];
        j.dst[(int64_t)row * j.dst_pitch + c] = whiten1(x, __ldg(j.mean + c), __ldg(j.variance + c), count);
    }
}

struct NormJobDev {
    const void* x;
    float* mean;
    float* variance;
    int64_t D, pitch;
    int32_t dtype;
    uint32_t first_block;
};

struct NormLaunch {
    NormJobDev job[ASAC_NORM_MAX_OBS];
    int32_t* step;
    unsigned int* counter;
    int32_t n_jobs, T;
    int32_t commit;                   // 0: a repetition of the measurement knob — everything but the stores
};

template <bool U8>
__device__ __forceinline__ float norm_load(const void* x, int64_t i) {
    return U8 ? (float)static_cast<const uint8_t*>(x)[i] : static_cast<const float*>(x)[i];
}

// the tree's offsets 32 .. 4 (inside the thread), then 2 and 1 (the four groups of a column through LDS); valid where g == 0
__device__ __forceinline__ float norm_tree(float (&acc)[kNormAcc], float (*s_part)[kNormCols], int c, int g) {
#pragma unroll
    for (int off = kNormAcc / 2; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < off; ++k) acc[k] += acc[k + off];
    s_part[g][c] = acc[0];
    __syncthreads();
    const float r = (s_part[0][c] + s_part[2][c]) + (s_part[1][c] + s_part[3][c]);
    __syncthreads();
    return r;
}

template <bool U8>
__device__ __forceinline__ void norm_columns(const NormJobDev& j, int T, float count, bool commit, int64_t col, int c, int g,
                                             float (*s_part)[kNormCols]) {
    const bool live = col < j.D;
    const float mean = live ? j.mean[col] : 0.f;
    float acc[kNormAcc];
#pragma unroll
    for (int k = 0; k < kNormAcc; ++k) acc[k] = 0.f;
    for (int t0 = 0; t0 < T; t0 += ASAC_NORM_ROW_LANES) {
#pragma unroll
        for (int k = 0; k < kNormAcc; ++k) {
            const int t = t0 + g + kNormGroups * k;
            if (live && t < T) acc[k] += (norm_load<U8>(j.x, (int64_t)t * j.pitch + col) - mean) / count;
        }
    }
    const float new_mean = mean + norm_tree(acc, s_part, c, g);      // (every group forms it: same LDS words, same order)
#pragma unroll
    for (int k = 0; k < kNormAcc; ++k) acc[k] = 0.f;
    for (int t0 = 0; t0 < T; t0 += ASAC_NORM_ROW_LANES) {
#pragma unroll
        for (int k = 0; k < kNormAcc; ++k) {
            const int t = t0 + g + kNormGroups * k;
            if (live && t < T) {
                const float x = norm_load<U8>(j.x, (int64_t)t * j.pitch + col);
                acc[k] += (x - new_mean) * (x - mean);
            }
        }
    }
    const float sum_v = norm_tree(acc, s_part, c, g);
    if (live && g == 0 && commit) {
        j.variance[col] = j.variance[col] + sum_v;
        j.mean[col] = new_mean;
    }
}

__global__ __launch_bounds__(kNormBlock) void k_normalizer_update(const NormLaunch by_value) {
    const ASAC_KARG NormLaunch& m = *static_cast<const ASAC_KARG NormLaunch*>(kernarg_base());
    __shared__ float s_part[kNormGroups][kNormCols];
    int q = 0;
    for (int i = 1; i < m.n_jobs; ++i)
        if (blockIdx.x >= m.job[i].first_block) q = i;
    const NormJobDev j = karg_copy(&m.job[q]);
    const int c = threadIdx.x & (kNormCols - 1), g = threadIdx.x / kNormCols;
    const int64_t col = (int64_t)(blockIdx.x - j.first_block) * kNormCols + c;
    // the OLD step: an agent-scope load (no scalar cache), its value is in every term below, so every workgroup has it
    // before it arrives
    const int32_t step = __hip_atomic_load(m.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t new_step = (int32_t)((uint32_t)step + (uint32_t)m.T);
    const float count = (float)new_step;
    if (j.dtype == ASAC_NORM_U8) norm_columns<true>(j, m.T, count, m.commit != 0, col, c, g, s_part);
    else norm_columns<false>(j, m.T, count, m.commit != 0, col, c, g, s_part);
    if (finish_arrive(m.counter) && threadIdx.x == 0) {
        if (m.commit) __hip_atomic_store(m.step, new_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        finish_reset(m.counter);
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace asac

using namespace asac;

extern "C" {

int asac_normalizer_row_lanes(void) { return ASAC_NORM_ROW_LANES; }

int asac_obs_whiten(const asac_whiten_job_t* jobs_host, int n_jobs, const int32_t* step, void* stream) {
    if (!jobs_host || n_jobs <= 0 || n_jobs > ASAC_NORM_MAX_OBS || !step) return bad_arg("asac_obs_whiten");
    WhitenLaunch m{};
    m.step = step;
    m.n_jobs = n_jobs;
    uint64_t blocks = 0;
    for (int q = 0; q < n_jobs; ++q) {
        const asac_whiten_job_t& h = jobs_host[q];
        WhitenJobDev& d = m.job[q];
        if (!h.src || !h.dst || !h.mean || !h.variance || h.D <= 0 || h.rows <= 0 || h.src_row_pitch < 0 ||
            h.dst_row_pitch < 0)
            return bad_arg("asac_obs_whiten: job");
        d.src_pitch = h.src_row_pitch ? h.src_row_pitch : h.D;
        d.dst_pitch = h.dst_row_pitch ? h.dst_row_pitch : h.D;
        if (d.src_pitch < h.D || d.dst_pitch < h.D) return bad_arg("asac_obs_whiten: pitch");
        if (h.rows * h.D >= (int64_t)1 << 31) return bad_arg("asac_obs_whiten: size");
        // in place (same rows), or apart: the extents [first element, one past the last) must not meet
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(h.src), d0 = reinterpret_cast<uintptr_t>(h.dst);
        const uintptr_t s1 = s0 + 4 * (uintptr_t)((h.rows - 1) * d.src_pitch + h.D);
        const uintptr_t d1 = d0 + 4 * (uintptr_t)((h.rows - 1) * d.dst_pitch + h.D);
        if (s0 == d0 ? d.src_pitch != d.dst_pitch : (s0 < d1 && d0 < s1)) return bad_arg("asac_obs_whiten: overlap");
        if ((s0 | d0 | reinterpret_cast<uintptr_t>(h.mean) | reinterpret_cast<uintptr_t>(h.variance)) & 3)
            return bad_arg("asac_obs_whiten: alignment");
        d.src = h.src;
        d.dst = h.dst;
        d.mean = h.mean;
        d.variance = h.variance;
        d.vec = h.D % 4 == 0 && d.src_pitch % 4 == 0 && d.dst_pitch % 4 == 0 && aligned16(h.src) && aligned16(h.dst) &&
                aligned16(h.mean) && aligned16(h.variance);
        d.units_per_row = (uint32_t)(d.vec ? h.D / 4 : h.D);
        d.total_units = (uint32_t)(h.rows * d.units_per_row);
        d.first_block = (uint32_t)blocks;
        blocks += (d.total_units + (uint64_t)kNormBlock - 1) / kNormBlock;
    }
    if (blocks == 0 || blocks > 0x7fffffffull) return bad_arg("asac_obs_whiten: grid");
    ASAC_LAUNCH(k_obs_whiten, dim3((unsigned)blocks), dim3(kNormBlock), 0, as_stream(stream), m);
    return finish_launch("asac_obs_whiten");
}

int asac_normalizer_update(const asac_normalizer_job_t* jobs_host, int n_jobs, int T, int32_t* step,
                           unsigned int* counter, void* stream) {
    if (!jobs_host || n_jobs <= 0 || n_jobs > ASAC_NORM_MAX_OBS || T <= 0 || !step || !counter)
        return bad_arg("asac_normalizer_update");
    NormLaunch m{};
    m.step = step;
    m.counter = counter;
    m.n_jobs = n_jobs;
    m.T = T;
    uint64_t blocks = 0;
    for (int q = 0; q < n_jobs; ++q) {
        const asac_normalizer_job_t& h = jobs_host[q];
        NormJobDev& d = m.job[q];
        if (!h.x || !h.mean || !h.variance || h.D <= 0 || h.x_row_pitch < 0 ||
            (h.dtype != ASAC_NORM_F32 && h.dtype != ASAC_NORM_U8))
            return bad_arg("asac_normalizer_update: job");
        d.pitch = h.x_row_pitch ? h.x_row_pitch : h.D;
        if (d.pitch < h.D) return bad_arg("asac_normalizer_update: pitch");
        if ((reinterpret_cast<uintptr_t>(h.mean) | reinterpret_cast<uintptr_t>(h.variance) |
             (h.dtype == ASAC_NORM_F32 ? reinterpret_cast<uintptr_t>(h.x) : 0)) & 3)
            return bad_arg("asac_normalizer_update: alignment");
        d.x = h.x;
        d.mean = h.mean;
        d.variance = h.variance;
        d.D = h.D;
        d.dtype = h.dtype;
        d.first_block = (uint32_t)blocks;
        blocks += (uint64_t)((h.D + kNormCols - 1) / kNormCols);
    }
    if (blocks == 0 || blocks > 0x7fffffffull) return bad_arg("asac_normalizer_update: grid");
    // (under the measurement repeat knob the statistics and the step advance in the first repetition only: an episode
    // counts once)
    for (int rep = 0; rep < g_launch_repeat; ++rep) {
        m.commit = rep == 0;
        hipLaunchKernelGGL(k_normalizer_update, dim3((unsigned)blocks), dim3(kNormBlock), 0, as_stream(stream), m);
    }
    return finish_launch("asac_normalizer_update");
}

}  // extern "C"
