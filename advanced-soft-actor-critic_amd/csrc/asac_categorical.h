// Per-row pieces of the branched categorical policy (reference nn_models/policy.py: one OneHotCategorical per discrete
// action branch, concatenated), under every kernel over a categorical head: the rows of asac_discrete_rows.h (discrete.hip,
// hybrid.hip, dqn.hip), asac_dqn.h, act.hip, drnd.hip.  ONE implementation: a value two kernels both form (p at the step's
// state in the policy step and in the temperature step) has the same bits in both.
//   p  = softmax(z)           = exp(z - max) / sum_j exp(z_j - max)        (torch softmax)
//   lp = z - logsumexp(z)     = z - (log(sum_j exp(z_j - max)) + max)      (torch logsumexp)
//   cl(p) = log(max(p, 1e-8))                                              (sac_base.py: torch.log(probs.clamp(min=1e-8)))
//   H  = -sum_j p_j lp_j                                                   (torch Categorical.entropy)
// Sums run over the branch's entries in index order by one lane (those of CatSum's comment compensated).
// Accurate expf / logf, -ffp-contract=off.
#pragma once
#include "asac_common.h"
#include "asac_vtrace.h"

#include <cmath>

namespace asac {

constexpr float kCatProbFloor = 1e-8f;

// the branch table of a launch: K sizes, D = their sum (by value in the kernel arguments)
__host__ __device__ __forceinline__ bool cat_branches_ok(const asac_branches_t& br) {
    if (br.K <= 0 || br.K > ASAC_DISCRETE_MAX_BRANCHES || br.D <= 0 || br.D > ASAC_DISCRETE_MAX_WIDTH) return false;
    int d = 0;
    for (int k = 0; k < br.K; ++k) {
        if (br.size[k] <= 0) return false;
        d += br.size[k];
    }
    return d == br.D;
}

struct CatStats {
    float m, sum, lse;       // max_j z_j, sum_j exp(z_j - m), log(sum) + m
};

// z[0..s): the logits of one branch of one row (stride 1; LDS or global)
__device__ __forceinline__ CatStats cat_stats(const float* z, int s) {
    CatStats st;
    float m = z[0];
    for (int j = 1; j < s; ++j) m = fmaxf(m, z[j]);
    float sum = 0.f;
    for (int j = 0; j < s; ++j) sum += expf(z[j] - m);
    st.m = m, st.sum = sum, st.lse = logf(sum) + m;
    return st;
}
// ... rebuilt from (m, sum) kept by the caller
__device__ __forceinline__ CatStats cat_stats_from(float m, float sum) {
    CatStats st;
    st.m = m, st.sum = sum, st.lse = logf(sum) + m;
    return st;
}

__device__ __forceinline__ float cat_prob(float z, const CatStats& st) { return expf(z - st.m) / st.sum; }
__device__ __forceinline__ float cat_logp(float z, const CatStats& st) { return z - st.lse; }
__device__ __forceinline__ float cat_cl(float p) { return logf(fmaxf(p, kCatProbFloor)); }
// d cl(p) / d p * p: 1 where the clamp passes the gradient (torch: p >= min), else 0
__device__ __forceinline__ float cat_cl_open(float p) { return p >= kCatProbFloor ? 1.f : 0.f; }

// a running float32 sum that carries its rounding error along (Kahan; nothing here is compiled with fast-math, so the
// compensation survives).  For the sums over up to 64 entries, 64 steps or 8 members whose plain running error shows at
// the limits: the branch sums the policy step's gradient cancels against a term of their own size afterwards (lp_i + H_k,
// g_i - S_k), V over a row's entries, the rows' loss terms, the members' mean, the DQN-like target's reward sum
struct CatSum {
    float s = 0.f, c = 0.f;
    __device__ __forceinline__ void add(float t) {
        const float y = t - c;
        const float u = s + y;
        c = (u - s) - y;
        s = u;
    }
};

__device__ __forceinline__ float cat_entropy(const float* z, int s, const CatStats& st) {
    CatSum h;
    for (int j = 0; j < s; ++j) h.add(cat_prob(z[j], st) * cat_logp(z[j], st));
    return -h.s;
}

// index drawn from a branch of s entries with probabilities p[0..s) by the inverse CDF on one uniform u in [0, 1):
// #{i < s - 1 : c_i <= u}, c the running float32 sum in index order (drnd.hip's candidates, act.hip's sampled action)
__device__ __forceinline__ int inverse_cdf(const float* p, int s, float u) {
    float c = 0.f;
    int idx = 0;
    for (int i = 0; i < s - 1; ++i) {
        c += p[i];
        idx += c <= u ? 1 : 0;
    }
    return idx;
}

// mean over the members of a device-resident subset of element `off` of each member's tensor (the members are separate
// tensors of one shape: a pointer table instead of a stack).  Every member's load is requested before the first add
// (members beyond the real ones re-read the last real one: a valid address, the value is not added); sum in subset order
// (compensated: CatSum), one division (torch mean).  `tab`: the table read in place from the kernel-argument segment.
__device__ __forceinline__ float cat_member_mean(const ASAC_KARG asac_members_t& tab, const int32_t* subset, int Es,
                                                 int64_t off) {
    float v[ASAC_DISCRETE_MAX_MEMBERS];
#pragma unroll
    for (int e = 0; e < ASAC_DISCRETE_MAX_MEMBERS; ++e) v[e] = tab.base[member(subset, min(e, Es - 1))][off];
    CatSum s;
#pragma unroll
    for (int e = 0; e < ASAC_DISCRETE_MAX_MEMBERS; ++e)
        if (e < Es) s.add(v[e]);
    return s.s / (float)Es;
}

// ... the minimum over the subset instead (the option's target, option_base.py:337-338): the same loads, fminf in subset
// order (torch min(0)); of one member it is that member's value, as the mean is
__device__ __forceinline__ float cat_member_min(const ASAC_KARG asac_members_t& tab, const int32_t* subset, int Es,
                                                int64_t off) {
    float v[ASAC_DISCRETE_MAX_MEMBERS];
#pragma unroll
    for (int e = 0; e < ASAC_DISCRETE_MAX_MEMBERS; ++e) v[e] = tab.base[member(subset, min(e, Es - 1))][off];
    float m = v[0];
#pragma unroll
    for (int e = 1; e < ASAC_DISCRETE_MAX_MEMBERS; ++e)
        if (e < Es) m = fminf(m, v[e]);
    return m;
}

constexpr int kDiscThreads = 256;

// sum_j a[j] * q[j] over a row of D entries: loads in groups of four requested together (indices beyond D re-read the last
// entry: a valid address, the product is not added), added in index order
__device__ __forceinline__ float disc_dot(const float* a, const float* q, int D) {
    float s = 0.f;
    for (int j0 = 0; j0 < D; j0 += 4) {
        float av[4], qv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = min(j0 + u, D - 1);
            av[u] = a[j], qv[u] = q[j];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j0 + u < D) s += av[u] * qv[u];
    }
    return s;
}

// the fixed-order tree over a workgroup's 256 lane partials (k_q_loss's), valid in lane 0
__device__ __forceinline__ float disc_tree_sum(float* red, float part) {
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = kDiscThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// the host checks of the entry points built on these pieces (discrete.hip, dqn.hip), written once per kind of argument
inline bool members_ok(const asac_members_t* m) {
    if (!m || m->E <= 0 || m->E > ASAC_DISCRETE_MAX_MEMBERS) return false;
    for (int e = 0; e < m->E; ++e)
        if (!m->base[e]) return false;
    return true;
}
inline bool reduction_rows_ok(int B) { return B > 0 && B <= ASAC_DISCRETE_MAX_ROWS; }

}  // namespace asac
