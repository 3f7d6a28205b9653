// The rows every launch over a branched categorical head is made of, written ONCE: discrete.hip (both instantiations of
// its return), hybrid.hip and dqn.hip call these, so what two launches both form (d_y, p, the Q step's gradient row) has
// the same bits in both by construction.  Built on asac_categorical.h (branch softmax, subset statistics, the tree).
//   return     disc_return_carve / disc_return_stage (phase 0) / disc_return_values (phase 1) / disc_return_online_q,
//              and the host side: disc_return_args_ok, disc_return_geometry
//   losses     disc_q_grad_row, disc_policy_row (both passes), disc_alpha_row
// The argument blocks arrive as POINTERS into the kernel-argument segment and are re-bound to a reference inside.  A
// reference PARAMETER is inlined as `dereferenceable`, which lets the compiler hoist the block's scalar loads to the top
// of the kernel — what ASAC_KARG (asac_common.h) is there to prevent (NOTES.md: figures).
#pragma once
#include "asac_categorical.h"

namespace asac {

__host__ __device__ __forceinline__ int disc_round4(int v) { return (v + 3) & ~3; }

// ------------------------------------------------------------------------------------------------------------------------
// the return: a workgroup of R rows, T = n + 1 window positions each, P = R * T
struct DiscReturnGeom {
    int32_t R, Dp, pitch, seg;       // rows per workgroup, LDS pitch of a position's entries, of a row's steps, scan lanes
};

struct DiscReturnLds {
    float *z, *qn, *qx;              // [P][Dp] logits; the statistic over subset_n / subset_next of the target members' values
    float *a, *mu;                   // [P][Dp] stored action, mu * stored action      (importance sampling only)
    float *vn, *vx, *lpa, *mup;      // [P] V with subset_n / subset_next, pi(stored action), prod_j (mu_j a_j, zeros -> 1)
    float* rest;                     // the kernel's own arrays
};
// LDS floats of the carve (every part a multiple of four floats) ...
__host__ __device__ __forceinline__ int disc_return_carve_floats(int P, int Dp, bool is) {
    return (is ? 5 : 3) * disc_round4(P * Dp) + 4 * disc_round4(P);
}
// ... and the carve
__device__ __forceinline__ DiscReturnLds disc_return_carve(float* lds, int P, int Dp, bool is) {
    const int NE = disc_round4(P * Dp), NP = disc_round4(P);
    DiscReturnLds s;
    s.z = lds, s.qn = s.z + NE, s.qx = s.qn + NE;
    s.a = s.qx + NE, s.mu = s.a + (is ? NE : 0);
    s.vn = s.mu + (is ? NE : 0), s.vx = s.vn + NP, s.lpa = s.vx + NP, s.mup = s.lpa + NP;
    s.rest = s.mup + NP;
    return s;
}

// phase 0, all lanes, coalesced over (row, position, j): logits, the two subset statistics of the target members' values
// (kMin: the minimum, else the mean) and, under importance sampling, the stored action and mu * action -> LDS; each
// element's loads are requested together.  The caller's barrier follows.
template <bool kMin>
__device__ __forceinline__ void disc_return_stage(const ASAC_KARG asac_vtrace_args_t* ap,
                                                  const ASAC_KARG asac_discrete_return_t* xp, const DiscReturnLds& s,
                                                  int row0, int R, int Dp) {
    const ASAC_KARG asac_vtrace_args_t& a = *ap;
    const ASAC_KARG asac_discrete_return_t& x = *xp;
    const int n = a.n, T = n + 1, D = x.branches.D, B = a.B, P = R * T, Es = a.E_sample;
    const bool is = a.use_n_step_is != 0;
    for (int idx = threadIdx.x; idx < P * D; idx += kDiscThreads) {
        const int pos = idx / D, j = idx - pos * D;
        const int r = pos / T, t = pos - r * T;
        const int b = row0 + r;
        if (b >= B) continue;
        const int64_t qoff = (int64_t)b * x.q_target.stride_b + (int64_t)t * x.q_target.stride_t + j;
        const float z = x.logits[(int64_t)b * x.logits_stride_b + (int64_t)t * x.logits_stride_t + j];
        float av = 0.f, mv = 0.f;
        if (is && t < n) {
            av = x.action[(int64_t)b * x.action_stride_b + (int64_t)t * x.action_stride_t + j];
            mv = a.mu_prob[(int64_t)b * a.mu_stride_b + (int64_t)t * a.mu_stride_t + j];
        }
        const float qn = kMin ? cat_member_min(x.q_target, a.subset_n, Es, qoff)
                              : cat_member_mean(x.q_target, a.subset_n, Es, qoff);
        const float qx = kMin ? cat_member_min(x.q_target, a.subset_next, Es, qoff)
                              : cat_member_mean(x.q_target, a.subset_next, Es, qoff);
        const int o = pos * Dp + j;
        s.z[o] = z, s.qn[o] = qn, s.qx[o] = qx;
        if (is) s.a[o] = av, s.mu[o] = mv * av;
    }
}

// phase 1, one lane per window position: branch softmax, V with subset_n and with subset_next, pi(stored action),
// prod mu.  kOption: per entry of the next position the termination mix (1 - beta) (Qx_j - c_j) + beta vbar
// (option_base.py:349-351), beta / vbar the [P] arrays of the step INTO the position
template <bool kOption>
__device__ __forceinline__ void disc_return_values(const ASAC_KARG asac_vtrace_args_t* ap,
                                                   const ASAC_KARG asac_discrete_return_t* xp, const DiscReturnLds& s,
                                                   int row0, int R, int Dp, const float* s_beta = nullptr,
                                                   const float* s_vbar = nullptr) {
    const ASAC_KARG asac_vtrace_args_t& a = *ap;
    const ASAC_KARG asac_discrete_return_t& x = *xp;
    const int T = a.n + 1, K = x.branches.K, P = R * T, tid = threadIdx.x;
    const bool is = a.use_n_step_is != 0;
    const float alpha = expf(*a.log_alpha);
    if (tid >= P || row0 + tid / T >= a.B) return;
    const int pos = tid;
    CatSum vn, vx;
    double lpa = 0.;                 // sum_k log pi_k(stored action), see below
    float mu = 1.f;
    const float beta = kOption ? s_beta[pos] : 0.f, vbar = kOption ? s_vbar[pos] : 0.f;
    int j0 = 0;
    for (int k = 0; k < K; ++k) {
        const int sz = x.branches.size[k];
        const int o0 = pos * Dp + j0;
        const CatStats cs = cat_stats(s.z + o0, sz);
        int arg = 0;
        float amax = is ? s.a[o0] : 0.f;
        for (int j = 0; j < sz; ++j) {
            const float p = cat_prob(s.z[o0 + j], cs);
            const float c = alpha * cat_cl(p);
            vn.add(p * (s.qn[o0 + j] - c));
            if (kOption)
                vx.add(p * ((1.f - beta) * (s.qx[o0 + j] - c) + beta * vbar));
            else
                vx.add(p * (s.qx[o0 + j] - c));
            if (is) {
                const float av = s.a[o0 + j];
                if (av > amax) amax = av, arg = j;             // the first maximum (torch max(-1)[1])
                const float m = s.mu[o0 + j];
                mu *= (m == 0.f) ? 1.f : m;
            }
        }
        if (is) lpa += ((double)s.z[o0 + arg] - (double)cs.m) - log((double)cs.sum);
        j0 += sz;
    }
    s.vn[pos] = vn.s / (float)K, s.vx[pos] = vx.s / (float)K;
    // pi(stored action) = exp(sum_k lp_k).  Over eight branches the sum reaches -13 and below, where float32 steps are
    // 1e-6, and exp turns the sum's rounding into that RELATIVE error of an unclamped ratio: the K terms (one per
    // position, from the branch's float32 max and sum) are formed and added in double, and pi is rounded once
    s.lpa[pos] = (float)exp(lpa), s.mup[pos] = mu;
}

// (1/K) sum_j a_j q_e[b, j] of the Eon online members at the step's state (TD error variant) -> s_qs [R][8]
__device__ __forceinline__ void disc_return_online_q(const ASAC_KARG asac_discrete_return_t* xp, float* s_qs, int row0,
                                                     int R, int B, int Eon) {
    const ASAC_KARG asac_discrete_return_t& x = *xp;
    for (int i = threadIdx.x; i < R * Eon; i += kDiscThreads) {
        const int r = i / Eon, e = i - r * Eon, b = row0 + r;
        if (b >= B) continue;
        const float s = disc_dot(x.action + (int64_t)b * x.action_stride_b,
                                 x.q_online.base[e] + (int64_t)b * x.q_online.stride_b, x.branches.D);
        s_qs[r * ASAC_DISCRETE_MAX_MEMBERS + e] = s / (float)x.branches.K;
    }
}

// the host checks of a categorical return's blocks (everything but the sign of B)
inline bool disc_return_args_ok(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host) {
    if (!args_host || !job_host) return false;
    const asac_vtrace_args_t& h = *args_host;
    const asac_discrete_return_t& x = *job_host;
    if (h.n <= 0 || h.n > ASAC_DISCRETE_MAX_STEPS || !h.y_out || !h.reward || !h.done || !h.last_mask ||
        !h.padding_mask || !h.gamma_ratio || !h.log_alpha || !x.logits || !cat_branches_ok(x.branches) ||
        !members_ok(&x.q_target) || h.E_sample <= 0 || h.E_sample > x.q_target.E)
        return false;
    if (h.use_n_step_is && (!h.mu_prob || !h.lambda_ratio || !x.action)) return false;
    if (h.td_error_out && (!members_ok(&x.q_online) || !x.action)) return false;
    return true;
}

// the launch geometry of kKernel, whose workgroup of R rows needs lds_floats(R, T, Dp, pitch) floats of LDS: rows per
// workgroup (one lane per window position, a few rounds of phase 0 at most, 64 KB), odd pitches (conflict-free
// position-per-lane / row-per-lane reads), the scan lanes; one row of a long, wide window under importance sampling
// (<= 88 KB) raises the kernel's limit to 96 KB, once per kernel.  0, or the error already recorded under `where`
template <auto kKernel, typename LdsFloats>
int disc_return_geometry(int B, int n, int D, LdsFloats lds_floats, const char* where, DiscReturnGeom* g,
                         size_t* lds_bytes) {
    const int T = n + 1;
    g->Dp = D | 1;
    g->pitch = (n + 1) | 1;
    int R = kDiscThreads / T;
    if (R > 2048 / (T * D)) R = 2048 / (T * D);
    if (R > B) R = B;
    if (R < 1) R = 1;
    while (R > 1 && (size_t)lds_floats(R, T, g->Dp, g->pitch) * sizeof(float) > 64 * 1024) --R;
    g->R = R;
    g->seg = vtrace_scan_lanes(B, n);
    const size_t lds = (size_t)lds_floats(R, T, g->Dp, g->pitch) * sizeof(float);
    if (lds > 64 * 1024) {
        static bool raised = false;               // (one flag per kernel)
        if (!raised) {
            hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            if (err != hipSuccess) {
                set_error(err, where);
                return (int)err;
            }
            raised = true;
        }
        if (lds > 96 * 1024) return bad_arg(where);
    }
    *lds_bytes = lds;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// the Q step's gradient row: d (diff^2 w / B) / d q[j], q entering through (1/K) sum_j a_j q_j
__device__ __forceinline__ void disc_q_grad_row(float diff, float wv, const float* act, float* g, int B, int D, int K) {
    const float gq = 2.f * diff * wv / (float)B / (float)K;
    for (int j = 0; j < D; ++j) g[j] = gq * act[j];
}

// ------------------------------------------------------------------------------------------------------------------------
// the policy step's row, part of the kernel's argument block (read in place: a subset pointer handed on by value stays
// live across both passes and costs scratch)
struct DiscPolicyRows {
    asac_branches_t br;
    asac_members_t q;                // the online members' head outputs
    const float *logits, *mu;
    const int32_t* subset;
    int64_t logits_stride, mu_stride, grad_stride;
    float *grad, *probs;             // probs (optional): p [B, D] contiguous
    float penalty;
    int32_t Es;
};
// a lane's per-branch (max, sum exp, sum_j p_j g_j, H_k) of the row it is on, kept between its two passes
struct DiscPolicyKeep {
    float m[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads], sum[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads];
    float S[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads], H[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads];
};

struct DiscRowTerm {
    float term, h_pi;                // the row's addend to the launch's sum; the row's entropy (1/K) sum_k H_k
};

// row b by one lane: the pass that forms the row's loss term and entropy (both returned), then the pass that writes
// its gradient p_i (g_i - S_k) + (lambda / K) (H_mu - H_pi) p_i (lp_i + H_k), over B (and p)
__device__ __forceinline__ DiscRowTerm disc_policy_row(const ASAC_KARG DiscPolicyRows* xp, DiscPolicyKeep& keep, int b,
                                                       int B, float alpha) {
    const ASAC_KARG DiscPolicyRows& x = *xp;
    const int K = x.br.K, Es = x.Es, tid = threadIdx.x;
    const float* z = x.logits + (int64_t)b * x.logits_stride;
    const float* mu = x.mu + (int64_t)b * x.mu_stride;
    const int64_t qrow = (int64_t)b * x.q.stride_b;
    CatSum main_sum, h_mu_sum;
    float h_pi = 0.f;
    int j0 = 0;
    for (int k = 0; k < K; ++k) {
        const int s = x.br.size[k];
        const CatStats cs = cat_stats(z + j0, s);
        CatSum Sk;
        for (int j = 0; j < s; ++j) {
            const float p = cat_prob(z[j0 + j], cs);
            const float c = alpha * cat_cl(p);
            const float qbar = cat_member_mean(x.q, x.subset, Es, qrow + j0 + j);
            const float g = (c - qbar + alpha * cat_cl_open(p)) / (float)K;
            main_sum.add(p * (c - qbar));
            Sk.add(p * g);
            const float m = mu[j0 + j];
            h_mu_sum.add(m * cat_cl(m));
        }
        const float H = cat_entropy(z + j0, s, cs), S = Sk.s;
        h_pi += H;
        keep.m[k * kDiscThreads + tid] = cs.m, keep.sum[k * kDiscThreads + tid] = cs.sum;
        keep.S[k * kDiscThreads + tid] = S, keep.H[k * kDiscThreads + tid] = H;
        j0 += s;
    }
    const float main = main_sum.s / (float)K;
    const float h_mu = -h_mu_sum.s / (float)K;
    h_pi = h_pi / (float)K;
    const float dh = h_mu - h_pi;
    const DiscRowTerm out = {main + x.penalty * (dh * dh / 2.f), h_pi};
    const float coef = x.penalty / (float)K * dh;
    float* grad = x.grad + (int64_t)b * x.grad_stride;
    j0 = 0;
    for (int k = 0; k < K; ++k) {
        const int s = x.br.size[k];
        const CatStats cs = cat_stats_from(keep.m[k * kDiscThreads + tid], keep.sum[k * kDiscThreads + tid]);
        const float S = keep.S[k * kDiscThreads + tid], H = keep.H[k * kDiscThreads + tid];
        for (int j = 0; j < s; ++j) {
            const float zz = z[j0 + j];
            const float p = cat_prob(zz, cs), lp = cat_logp(zz, cs);
            const float c = alpha * cat_cl(p);
            const float qbar = cat_member_mean(x.q, x.subset, Es, qrow + j0 + j);
            const float g = (c - qbar + alpha * cat_cl_open(p)) / (float)K;
            grad[j0 + j] = (p * (g - S) + coef * (p * (lp + H))) / (float)B;
            if (x.probs) x.probs[(int64_t)b * x.br.D + j0 + j] = p;
        }
        j0 += s;
    }
    return out;
}

// ------------------------------------------------------------------------------------------------------------------------
// the temperature step's row: (1/K) sum_j p_j (-cl(p_j) - target_j) and (want_h, else 0) the row's entropy; optionally
// p -> probs[0..D)
__device__ __forceinline__ DiscRowTerm disc_alpha_row(const ASAC_KARG asac_branches_t* brp, const float* z,
                                                      const float* target, float* probs, bool want_h) {
    const ASAC_KARG asac_branches_t& br = *brp;
    const int K = br.K;
    CatSum row;
    float h = 0.f;
    int j0 = 0;
    for (int k = 0; k < K; ++k) {
        const int s = br.size[k];
        const CatStats cs = cat_stats(z + j0, s);
        for (int j = 0; j < s; ++j) {
            const float p = cat_prob(z[j0 + j], cs);
            row.add(p * (-cat_cl(p) - target[j0 + j]));
            if (probs) probs[j0 + j] = p;
        }
        if (want_h) h += cat_entropy(z + j0, s, cs);
        j0 += s;
    }
    return {row.s / (float)K, h / (float)K};
}

}  // namespace asac
