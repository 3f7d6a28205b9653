// Pure-discrete, policy-based SAC: the learner's row-wise arithmetic around the networks, one launch per item
// (reference sac_base.py: _get_y 1383-1421 + _v_trace 1244-1295, _train_rep_q 1533-1538 / 1563-1568, _train_policy
// 1858-1880 / 1903, _train_alpha 1924-1929 / 1944, _get_td_error 2219-2244).  The per-row categorical pieces are
// asac_categorical.h's, the return's step arithmetic and row scan asac_vtrace.h's.
//
//   asac_discrete_return            many workgroups of R rows, no exchange between them:
//       phase 0  all lanes, coalesced over (row, position, j): logits, the two subset means of the target members' values
//                (and, under importance sampling, the stored action and mu * action) -> LDS; each element's loads are
//                requested together; the step's reward / masks / ratios are requested before that
//       phase 1  one lane per window position: branch softmax, V with subset_n and with subset_next, log pi(stored action),
//                prod mu
//       phase 2  one lane per step: ratio, vtrace_step_finish_v;   phase 3  one lane per row: vtrace_scan_row, y, TD error
//   asac_option_discrete_return     the same kernel's second instantiation (OptionBase._get_y's policy-based discrete
//       branch, option_base.py:287, 333-373): the MINIMUM over each subset instead of the mean, and per entry of positions
//       1..n the termination mix (1 - beta_t) (Qx_j - c_j) + beta_t vbar_t, vbar = asac_option.h's option_mean.  A step's
//       beta and its options' values are requested with the step's reward and masks (at clamped indexes, by every lane)
//       and handed to position t + 1 through LDS.  The plain instantiation's arithmetic and order are what they were
//   asac_discrete_q_loss_grad       one workgroup per member
//   asac_discrete_policy_loss_grad  one workgroup; a lane keeps its row's per-branch (max, sum, sum p g, H) in LDS between
//                                   the pass that forms the row's loss and entropies and the pass that writes its gradient
//   asac_discrete_alpha_grad        one workgroup
// Batch means: lane partial (rows tid, tid + 256, ..) -> the tree of k_q_loss (returns.hip) -> one division by B.  No float
// atomics: equal inputs give equal bits.  The argument blocks (branch table, member pointers) are read in place from the
// kernel-argument segment (asac_common.h ASAC_KARG): a lane-dependent member index is an ordinary load, not a private copy.
#include "asac_common.h"
#include "asac_vtrace.h"
#include "asac_categorical.h"
#include "asac_option.h"

namespace asac {

// ------------------------------------------------------------------------------------------------------------------------
struct DiscReturnDev {
    asac_vtrace_args_t a;
    asac_discrete_return_t x;
    int32_t R, Dp, pitch, seg;       // rows per workgroup, LDS pitch of a position's entries, of a row's steps, scan lanes
    // the option's termination mix (kOption only): beta [B, n], the options' values [B, n, O], strides in floats
    const float *beta, *v_options;
    int64_t beta_sb, beta_st, v_sb, v_st, v_so;
    int32_t O;
};

__host__ __device__ __forceinline__ int disc_round4(int v) { return (v + 3) & ~3; }
// LDS floats of a workgroup of R rows (every part a multiple of four floats)
// (`option`: plus the two [P] arrays of the termination mix)
__host__ __device__ __forceinline__ int disc_return_lds_floats(int R, int T, int Dp, int pitch, bool is,
                                                               bool option = false) {
    const int P = R * T;
    return (is ? 5 : 3) * disc_round4(P * Dp) + (option ? 6 : 4) * disc_round4(P) + 2 * disc_round4(R * pitch) +
           disc_round4(R * ASAC_DISCRETE_MAX_MEMBERS);
}

template <bool kOption>
__global__ __launch_bounds__(kDiscThreads) void k_discrete_return(const DiscReturnDev by_value) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ASAC_KARG DiscReturnDev& v = *static_cast<const ASAC_KARG DiscReturnDev*>(kernarg_base());
    const ASAC_KARG asac_vtrace_args_t& a = v.a;
    const ASAC_KARG asac_discrete_return_t& x = v.x;
    const int n = a.n, T = n + 1, R = v.R, D = x.branches.D, K = x.branches.K, Dp = v.Dp, pitch = v.pitch;
    const int B = a.B, P = R * T;
    const bool is = a.use_n_step_is != 0;
    const int NE = disc_round4(P * Dp), NP = disc_round4(P), NS = disc_round4(R * pitch);
    float* s_z = lds;                    // [P][Dp] logits
    float* s_qn = s_z + NE;              // [P][Dp] mean over subset_n of the target members' values
    float* s_qx = s_qn + NE;             // [P][Dp] ... over subset_next
    float* s_a = s_qx + NE;              // [P][Dp] stored action            (importance sampling only)
    float* s_mu = s_a + (is ? NE : 0);   // [P][Dp] mu * stored action       (importance sampling only)
    float* s_vn = s_mu + (is ? NE : 0);  // [P] V with subset_n
    float* s_vx = s_vn + NP;             // [P] V with subset_next
    float* s_lpa = s_vx + NP;            // [P] log pi(stored action)
    float* s_mup = s_lpa + NP;           // [P] prod_j (mu_j a_j, zeros -> 1)
    float* s_d = s_mup + NP;             // [R][pitch] per-step term d_t
    float* s_c = s_d + NS;               // [R][pitch] trace-cutting factor c_t
    float* s_qs = s_c + NS;              // [R][8] the online members' value of the stored action at t = 0
    float* s_beta = s_qs + disc_round4(R * ASAC_DISCRETE_MAX_MEMBERS);   // [P] beta of the step INTO the position (kOption)
    float* s_vbar = s_beta + NP;         // [P] mean over the options at that step                                 (kOption)
    const int row0 = blockIdx.x * R;
    const int tid = threadIdx.x;

    // the step (row, t) this lane finishes in phase 2 (R * n <= R * T <= 256): its loads are requested first
    VtraceStepRaw raw{};
    const int sr = tid / n, st = tid - sr * n;
    const bool have_step = tid < R * n && row0 + sr < B;
    if (have_step) {
        const int b = row0 + sr;
        const int64_t mi = (int64_t)b * a.mask_stride + st;
        const bool done = a.done[mi];
        raw.reward = a.reward[(int64_t)b * a.reward_stride + st];
        raw.gamma_ratio = a.gamma_ratio[st];
        const bool gone = a.last_mask[mi] | a.padding_mask[mi];
        raw.lambda_ratio = is ? a.lambda_ratio[st] : 1.f;
        raw.g = done ? 0.f : a.gamma;                      // gamma * ~done
        raw.keep = gone ? 0.f : 1.f;                       // ~(last | pad)
        raw.ratio = 1.f;
    }
    if (kOption) {
        // the step's beta and option values: loaded by EVERY lane at clamped indexes, kept by the lanes that have a step;
        // step t mixes into position t + 1 (position 0 of a row is never a next position: an exact 0 there)
        const int b = min(row0 + sr, B - 1);
        const float beta = v.beta[(int64_t)b * v.beta_sb + (int64_t)st * v.beta_st];
        const float vbar = option_mean(v.v_options + (int64_t)b * v.v_sb + (int64_t)st * v.v_st, v.v_so, v.O);
        if (have_step) {
            const int pos = sr * T + st;
            s_beta[pos + 1] = beta, s_vbar[pos + 1] = vbar;
            if (st == 0) s_beta[pos] = 0.f, s_vbar[pos] = 0.f;
        }
    }

    // phase 0
    const int Es = a.E_sample;
    for (int idx = tid; idx < P * D; idx += kDiscThreads) {
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
        const float qn = kOption ? cat_member_min(x.q_target, a.subset_n, Es, qoff)
                                 : cat_member_mean(x.q_target, a.subset_n, Es, qoff);
        const float qx = kOption ? cat_member_min(x.q_target, a.subset_next, Es, qoff)
                                 : cat_member_mean(x.q_target, a.subset_next, Es, qoff);
        const int o = pos * Dp + j;
        s_z[o] = z, s_qn[o] = qn, s_qx[o] = qx;
        if (is) s_a[o] = av, s_mu[o] = mv * av;
    }
    __syncthreads();

    // phase 1
    const float alpha = expf(*a.log_alpha);
    if (tid < P && row0 + tid / T < B) {
        const int pos = tid;
        float vn = 0.f, vx = 0.f, lpa = 0.f, mu = 1.f;
        const float beta = kOption ? s_beta[pos] : 0.f, vbar = kOption ? s_vbar[pos] : 0.f;
        int j0 = 0;
        for (int k = 0; k < K; ++k) {
            const int s = x.branches.size[k];
            const int o0 = pos * Dp + j0;
            const CatStats cs = cat_stats(s_z + o0, s);
            int arg = 0;
            float amax = is ? s_a[o0] : 0.f;
            for (int j = 0; j < s; ++j) {
                const float p = cat_prob(s_z[o0 + j], cs);
                const float c = alpha * cat_cl(p);
                vn += p * (s_qn[o0 + j] - c);
                if (kOption)
                    vx += p * ((1.f - beta) * (s_qx[o0 + j] - c) + beta * vbar);      // option_base.py:349-351
                else
                    vx += p * (s_qx[o0 + j] - c);
                if (is) {
                    const float av = s_a[o0 + j];
                    if (av > amax) amax = av, arg = j;             // the first maximum (torch max(-1)[1])
                    const float m = s_mu[o0 + j];
                    mu *= (m == 0.f) ? 1.f : m;
                }
            }
            if (is) lpa += cat_logp(s_z[o0 + arg], cs);
            j0 += s;
        }
        s_vn[pos] = vn / (float)K, s_vx[pos] = vx / (float)K;
        s_lpa[pos] = lpa, s_mup[pos] = mu;
    }
    // (1/K) sum_j a_j q_e[b, j] of the online members at the step's state (TD error variant)
    const int Eon = a.td_error_out ? x.q_online.E : 0;
    for (int i = tid; i < R * Eon; i += kDiscThreads) {
        const int r = i / Eon, e = i - r * Eon, b = row0 + r;
        if (b >= B) continue;
        const float s = disc_dot(x.action + (int64_t)b * x.action_stride_b,
                                 x.q_online.base[e] + (int64_t)b * x.q_online.stride_b, D);
        s_qs[r * ASAC_DISCRETE_MAX_MEMBERS + e] = s / (float)K;
    }
    __syncthreads();

    // phase 2
    if (have_step) {
        const int pos = sr * T + st;
        if (is) raw.ratio = expf(s_lpa[pos]) / fmaxf(s_mup[pos], 1e-8f);
        float d, c;
        vtrace_step_finish_v(a, raw, s_vn[pos], s_vx[pos + 1], &d, &c);
        s_d[sr * pitch + st] = d;
        s_c[sr * pitch + st] = c;
    }
    __syncthreads();

    // phase 3
    if (tid >= R || row0 + tid >= B) return;
    const int b = row0 + tid;
    const float y = s_vn[tid * T] + vtrace_scan_row(s_d + tid * pitch, s_c + tid * pitch, n, v.seg);
    a.y_out[b] = y;
    if (Eon) {
        float s = 0.f;
        for (int e = 0; e < Eon; ++e) s += fabsf(s_qs[tid * ASAC_DISCRETE_MAX_MEMBERS + e] - y);
        a.td_error_out[b] = s / (float)Eon;
    }
}

// the host side both instantiations share: the checks (everything but the sign of B) ...
static bool discrete_return_args_ok(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host) {
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

// ... and the launch geometry (`v`: the option's fields already set, the rest filled here)
template <bool kOption>
static int discrete_return_launch(const asac_vtrace_args_t& h, const asac_discrete_return_t& x, DiscReturnDev& v,
                                  const char* where, void* stream) {
    v.a = h;
    v.x = x;
    if (!h.td_error_out) v.x.q_online.E = 0;
    const int T = h.n + 1, D = x.branches.D;
    const bool is = h.use_n_step_is != 0;
    v.Dp = D | 1;                                 // odd pitches: conflict-free position-per-lane / row-per-lane reads
    v.pitch = (h.n + 1) | 1;
    // rows per workgroup: one lane per window position, a few rounds of phase 0 at most, and the LDS they need
    int R = kDiscThreads / T;
    if (R > 2048 / (T * D)) R = 2048 / (T * D);
    if (R > h.B) R = h.B;
    if (R < 1) R = 1;
    while (R > 1 && (size_t)disc_return_lds_floats(R, T, v.Dp, v.pitch, is, kOption) * sizeof(float) > 64 * 1024) --R;
    v.R = R;
    v.seg = vtrace_scan_lanes(h.B, h.n);
    const size_t lds = (size_t)disc_return_lds_floats(R, T, v.Dp, v.pitch, is, kOption) * sizeof(float);
    if (lds > 64 * 1024) {                        // one row of a long, wide window under importance sampling (<= 88 KB)
        static bool raised = false;               // (one flag per instantiation)
        if (!raised) {
            hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_discrete_return<kOption>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            if (err != hipSuccess) {
                set_error(err, where);
                return (int)err;
            }
            raised = true;
        }
        if (lds > 96 * 1024) return bad_arg(where);
    }
    const int blocks = (h.B + R - 1) / R;
    ASAC_LAUNCH(k_discrete_return<kOption>, dim3((unsigned)blocks), dim3(kDiscThreads), lds, as_stream(stream), v);
    return finish_launch(where);
}

// ------------------------------------------------------------------------------------------------------------------------
struct DiscQLossDev {
    asac_branches_t br;
    asac_members_t q;
    const float *action, *y, *w;
    int64_t action_stride, y_stride, w_stride;
    float *loss, *grad;
    int32_t B;
};

__global__ __launch_bounds__(kDiscThreads) void k_discrete_q_loss(const DiscQLossDev by_value) {
    __shared__ float red[kDiscThreads];
    const ASAC_KARG DiscQLossDev& x = *static_cast<const ASAC_KARG DiscQLossDev*>(kernarg_base());
    const int e = blockIdx.x, B = x.B, D = x.br.D, K = x.br.K;
    const float* qe = x.q.base[e];
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += kDiscThreads) {
        const float* act = x.action + (int64_t)b * x.action_stride;
        const float yv = x.y[(int64_t)b * x.y_stride];
        const float wv = x.w ? x.w[(int64_t)b * x.w_stride] : 1.f;
        const float qs = disc_dot(act, qe + (int64_t)b * x.q.stride_b, D) / (float)K;
        const float diff = qs - yv;
        part += diff * diff * wv;
        const float gq = 2.f * diff * wv / (float)B / (float)K;
        float* g = x.grad + ((int64_t)e * B + b) * D;
        for (int j = 0; j < D; ++j) g[j] = gq * act[j];
    }
    const float total = disc_tree_sum(red, part);
    if (threadIdx.x == 0) x.loss[e] = total / (float)B;
}

// ------------------------------------------------------------------------------------------------------------------------
struct DiscPolicyDev {
    asac_branches_t br;
    asac_members_t q;
    const float *logits, *mu, *log_alpha;
    const int32_t* subset;
    int64_t logits_stride, mu_stride, grad_stride;
    float *loss, *grad, *entropy, *probs, *row_entropy;
    float penalty;
    int32_t B, Es;
};

__global__ __launch_bounds__(kDiscThreads) void k_discrete_policy_loss(const DiscPolicyDev by_value) {
    // a lane's per-branch (max, sum exp, sum_j p_j g_j, H_k) of the row it is on, kept between its two passes
    __shared__ float s_m[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads], s_sum[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads];
    __shared__ float s_S[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads], s_H[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads];
    __shared__ float red[kDiscThreads];
    const ASAC_KARG DiscPolicyDev& x = *static_cast<const ASAC_KARG DiscPolicyDev*>(kernarg_base());
    const int B = x.B, D = x.br.D, K = x.br.K, Es = x.Es, tid = threadIdx.x;
    const float alpha = expf(*x.log_alpha);
    float part = 0.f, ent = 0.f;
    for (int b = tid; b < B; b += kDiscThreads) {
        const float* z = x.logits + (int64_t)b * x.logits_stride;
        const float* mu = x.mu + (int64_t)b * x.mu_stride;
        const int64_t qrow = (int64_t)b * x.q.stride_b;
        float main = 0.f, h_mu = 0.f, h_pi = 0.f;
        int j0 = 0;
        for (int k = 0; k < K; ++k) {
            const int s = x.br.size[k];
            const CatStats cs = cat_stats(z + j0, s);
            float S = 0.f;
            for (int j = 0; j < s; ++j) {
                const float p = cat_prob(z[j0 + j], cs);
                const float c = alpha * cat_cl(p);
                const float qbar = cat_member_mean(x.q, x.subset, Es, qrow + j0 + j);
                const float g = (c - qbar + alpha * cat_cl_open(p)) / (float)K;
                main += p * (c - qbar);
                S += p * g;
                const float m = mu[j0 + j];
                h_mu += m * cat_cl(m);
            }
            const float H = cat_entropy(z + j0, s, cs);
            h_pi += H;
            s_m[k * kDiscThreads + tid] = cs.m, s_sum[k * kDiscThreads + tid] = cs.sum;
            s_S[k * kDiscThreads + tid] = S, s_H[k * kDiscThreads + tid] = H;
            j0 += s;
        }
        main = main / (float)K;
        h_mu = -h_mu / (float)K;
        h_pi = h_pi / (float)K;
        const float dh = h_mu - h_pi;
        part += main + x.penalty * (dh * dh / 2.f);
        ent += h_pi;
        if (x.row_entropy) x.row_entropy[b] = h_pi;
        // the row's gradient: p_i (g_i - S_k) + (lambda / K) (H_mu - H_pi) p_i (lp_i + H_k), over B
        const float coef = x.penalty / (float)K * dh;
        float* grad = x.grad + (int64_t)b * x.grad_stride;
        j0 = 0;
        for (int k = 0; k < K; ++k) {
            const int s = x.br.size[k];
            const CatStats cs = cat_stats_from(s_m[k * kDiscThreads + tid], s_sum[k * kDiscThreads + tid]);
            const float S = s_S[k * kDiscThreads + tid], H = s_H[k * kDiscThreads + tid];
            for (int j = 0; j < s; ++j) {
                const float zz = z[j0 + j];
                const float p = cat_prob(zz, cs), lp = cat_logp(zz, cs);
                const float c = alpha * cat_cl(p);
                const float qbar = cat_member_mean(x.q, x.subset, Es, qrow + j0 + j);
                const float g = (c - qbar + alpha * cat_cl_open(p)) / (float)K;
                grad[j0 + j] = (p * (g - S) + coef * (p * (lp + H))) / (float)B;
                if (x.probs) x.probs[(int64_t)b * D + j0 + j] = p;
            }
            j0 += s;
        }
    }
    const float loss = disc_tree_sum(red, part);
    __syncthreads();
    const float entropy = disc_tree_sum(red, ent);
    if (tid == 0) {
        *x.loss = loss / (float)B;
        *x.entropy = entropy / (float)B;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct DiscAlphaDev {
    asac_branches_t br;
    const float *logits, *target;
    int64_t logits_stride;
    float *slot, *probs, *row_entropy;
    int32_t B;
};

__global__ __launch_bounds__(kDiscThreads) void k_discrete_alpha_grad(const DiscAlphaDev by_value) {
    __shared__ float red[kDiscThreads];
    const ASAC_KARG DiscAlphaDev& x = *static_cast<const ASAC_KARG DiscAlphaDev*>(kernarg_base());
    const int B = x.B, D = x.br.D, K = x.br.K;
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += kDiscThreads) {
        const float* z = x.logits + (int64_t)b * x.logits_stride;
        float row = 0.f, h_pi = 0.f;
        int j0 = 0;
        for (int k = 0; k < K; ++k) {
            const int s = x.br.size[k];
            const CatStats cs = cat_stats(z + j0, s);
            for (int j = 0; j < s; ++j) {
                const float p = cat_prob(z[j0 + j], cs);
                row += p * (-cat_cl(p) - x.target[j0 + j]);
                if (x.probs) x.probs[(int64_t)b * D + j0 + j] = p;
            }
            if (x.row_entropy) h_pi += cat_entropy(z + j0, s, cs);
            j0 += s;
        }
        part += row / (float)K;
        if (x.row_entropy) x.row_entropy[b] = h_pi / (float)K;
    }
    const float total = disc_tree_sum(red, part);
    if (threadIdx.x == 0) *x.slot = total / (float)B;
}

}  // namespace asac

using namespace asac;

extern "C" {

int asac_discrete_return(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host, void* stream) {
    if (!discrete_return_args_ok(args_host, job_host) || args_host->B <= 0)
        return bad_arg("asac_discrete_return");
    DiscReturnDev v{};
    return discrete_return_launch<false>(*args_host, *job_host, v, "asac_discrete_return", stream);
}

int asac_option_discrete_return(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host,
                                const float* beta, int64_t beta_stride_b, int64_t beta_stride_t,
                                const float* v_options, int64_t v_stride_b, int64_t v_stride_t, int64_t v_stride_o,
                                int num_options, void* stream) {
    if (!discrete_return_args_ok(args_host, job_host) || args_host->B < 0 || !beta ||
        !v_options || num_options <= 0 || num_options > ASAC_OPTION_MAX_OPTIONS)
        return bad_arg("asac_option_discrete_return");
    if (args_host->B == 0) return 0;
    DiscReturnDev v{};
    v.beta = beta, v.v_options = v_options;
    v.beta_sb = beta_stride_b, v.beta_st = beta_stride_t;
    v.v_sb = v_stride_b, v.v_st = v_stride_t, v.v_so = v_stride_o;
    v.O = num_options;
    return discrete_return_launch<true>(*args_host, *job_host, v, "asac_option_discrete_return", stream);
}

int asac_discrete_q_loss_grad(const asac_branches_t* branches, const asac_members_t* q, const float* action,
                              int64_t action_stride, const float* y, int64_t y_stride, const float* w, int64_t w_stride,
                              int B, float* loss_out, float* grad_q, void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !members_ok(q) || !action || !y || !loss_out || !grad_q ||
        !reduction_rows_ok(B))
        return bad_arg("asac_discrete_q_loss_grad");
    DiscQLossDev x{};
    x.br = *branches, x.q = *q;
    x.action = action, x.y = y, x.w = w;
    x.action_stride = action_stride, x.y_stride = y_stride, x.w_stride = w_stride;
    x.loss = loss_out, x.grad = grad_q, x.B = B;
    ASAC_LAUNCH(k_discrete_q_loss, dim3((unsigned)q->E), dim3(kDiscThreads), 0, as_stream(stream), x);
    return finish_launch("asac_discrete_q_loss_grad");
}

int asac_discrete_policy_loss_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                                   const asac_members_t* q, const int32_t* subset, int E_sample, const float* mu,
                                   int64_t mu_stride, const float* log_alpha, float entropy_penalty, int B,
                                   float* loss_out, float* grad_logits, int64_t grad_stride, float* entropy_out,
                                   float* probs_out, float* row_entropy_out, void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !logits || !members_ok(q) || E_sample <= 0 || E_sample > q->E ||
        !mu || !log_alpha || !loss_out || !grad_logits || !entropy_out || !reduction_rows_ok(B))
        return bad_arg("asac_discrete_policy_loss_grad");
    DiscPolicyDev x{};
    x.br = *branches, x.q = *q;
    x.logits = logits, x.mu = mu, x.log_alpha = log_alpha, x.subset = subset;
    x.logits_stride = logits_stride, x.mu_stride = mu_stride, x.grad_stride = grad_stride;
    x.loss = loss_out, x.grad = grad_logits, x.entropy = entropy_out, x.probs = probs_out, x.row_entropy = row_entropy_out;
    x.penalty = entropy_penalty, x.B = B, x.Es = E_sample;
    ASAC_LAUNCH(k_discrete_policy_loss, dim3(1), dim3(kDiscThreads), 0, as_stream(stream), x);
    return finish_launch("asac_discrete_policy_loss_grad");
}

int asac_discrete_alpha_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                             const float* target, int B, float* grad_slot, float* probs_out, float* row_entropy_out,
                             void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !logits || !target || !grad_slot || !reduction_rows_ok(B))
        return bad_arg("asac_discrete_alpha_grad");
    DiscAlphaDev x{};
    x.br = *branches;
    x.logits = logits, x.target = target, x.logits_stride = logits_stride;
    x.slot = grad_slot, x.probs = probs_out, x.row_entropy = row_entropy_out, x.B = B;
    ASAC_LAUNCH(k_discrete_alpha_grad, dim3(1), dim3(kDiscThreads), 0, as_stream(stream), x);
    return finish_launch("asac_discrete_alpha_grad");
}

}  // extern "C"
