// The DQN-like discrete learner's per-row target (reference sac_base.py get_dqn_like_d_y 1194-1242, called from _get_y
// 1363-1382): ONE implementation, called by the return's launch and by the Q step's loss launch (dqn.hip), so the y both
// write has the same bits.
//   L    = the last t in [0, n) with !(last | pad); n - 1 where there is none (get_last_false_indexes on an all-True row)
//   j*_k = the LOWEST index of the maximum of eval[subset_n[i]][b, L, branch k]                     (torch.argmax)
//   v_i  = (1/K) sum_k target[subset_next[i]][b, L + 1, j*_k];   the two subsets pair by position i
//   y    = sum_t gamma_ratio[t] reward[b, t] + gamma^(L+1) min_i v_i (done[b, L] ? 0 : 1)
// Loads: the row's steps in one uniform loop; then, four columns of a branch at a time, the eval and the target values of
// ALL members of the pair of subsets are requested together at clamped indices (columns beyond the branch re-read its last
// one, member slots beyond E_sample re-read the last real member: valid addresses) and selected afterwards — no load sits
// under a lane condition.  The running (maximum, target value at it) per member lives in registers: M is the compile-time
// number of member slots (2 or 8), every array index a constant after unrolling.
#pragma once
#include "asac_categorical.h"

namespace asac {

struct DqnDev {
    asac_vtrace_args_t a;
    asac_dqn_job_t x;
};

template <int M>
__device__ __forceinline__ float dqn_row_target(const ASAC_KARG asac_vtrace_args_t& a, const ASAC_KARG asac_dqn_job_t& x,
                                                int b) {
    const int n = a.n, K = x.branches.K, Es = a.E_sample;
    // the row's steps: L, done at L, gamma^(L+1), the discounted reward sum in index order (compensated)
    int L = -1;
    bool done_at = false, done_t = false;
    CatSum g;
    double gp = 1., gp_at = 1.;        // gamma^(t+1), exact to float after the rounding below
    const int64_t m0 = (int64_t)b * a.mask_stride;
    const float* rw = a.reward + (int64_t)b * a.reward_stride;
    for (int t = 0; t < n; ++t) {
        const bool gone = a.last_mask[m0 + t] | a.padding_mask[m0 + t];
        done_t = a.done[m0 + t];
        g.add(a.gamma_ratio[t] * rw[t]);
        gp *= (double)a.gamma;
        if (!gone) L = t, done_at = done_t, gp_at = gp;
    }
    if (L < 0) L = n - 1, done_at = done_t, gp_at = gp;

    const int64_t eoff = (int64_t)b * x.q_eval.stride_b + (int64_t)L * x.q_eval.stride_t;
    const int64_t toff = (int64_t)b * x.q_target.stride_b + (int64_t)(L + 1) * x.q_target.stride_t;
    const float *pe[M], *pt[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const int ii = min(i, Es - 1);
        pe[i] = x.q_eval.base[member(a.subset_n, ii)] + eoff;
        pt[i] = x.q_target.base[member(a.subset_next, ii)] + toff;
    }
    float best[M], at[M], acc[M];
#pragma unroll
    for (int i = 0; i < M; ++i) best[i] = 0.f, at[i] = 0.f, acc[i] = 0.f;
    int j0 = 0;
    for (int k = 0; k < K; ++k) {
        const int s = x.branches.size[k];
        for (int c0 = 0; c0 < s; c0 += 4) {
            float ev[M][4], tv[M][4];
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + min(c0 + u, s - 1);
                    ev[i][u] = pe[i][j], tv[i][u] = pt[i][j];
                }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool first = c0 + u == 0, in = c0 + u < s;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const bool take = in && (first || ev[i][u] > best[i]);      // strictly greater: the first maximum
                    best[i] = take ? ev[i][u] : best[i];
                    at[i] = take ? tv[i][u] : at[i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < M; ++i) acc[i] += at[i];
        j0 += s;
    }
    float v = acc[0] / (float)K;
#pragma unroll
    for (int i = 1; i < M; ++i)
        if (i < Es) v = fminf(v, acc[i] / (float)K);
    return g.s + (float)gp_at * v * (done_at ? 0.f : 1.f);
}

// (1/K) sum_j a[b, j] q_e[b, j] of online member e at the step's state
__device__ __forceinline__ float dqn_stored_q(const ASAC_KARG asac_dqn_job_t& x, int e, int b) {
    return disc_dot(x.action + (int64_t)b * x.action_stride, x.q_online.base[e] + (int64_t)b * x.q_online.stride_b,
                    x.branches.D) / (float)x.branches.K;
}

}  // namespace asac
