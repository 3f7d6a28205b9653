// Pure-discrete, policy-based SAC: the learner's row-wise arithmetic around the networks, one launch per item
// (reference sac_base.py: _get_y 1383-1421 + _v_trace 1244-1295, _train_rep_q 1533-1538 / 1563-1568, _train_policy
// 1858-1880 / 1903, _train_alpha 1924-1929 / 1944, _get_td_error 2219-2244).  The rows themselves are
// asac_discrete_rows.h's, shared with hybrid.hip and dqn.hip; the return's step arithmetic and row scan asac_vtrace.h's.
// This file holds what is its own: the argument blocks, the step's loads, phases 2 and 3 and the reductions.
//
//   asac_discrete_return            many workgroups of R rows, no exchange between them:
//       the step's reward / masks / ratios are requested first
//       phase 0  disc_return_stage   phase 1  disc_return_values (and disc_return_online_q)
//       phase 2  one lane per step: ratio, vtrace_step_finish_v;   phase 3  one lane per row: vtrace_scan_row, y, TD error
//   asac_option_discrete_return     the same kernel's second instantiation (OptionBase._get_y's policy-based discrete
//       branch, option_base.py:287, 333-373): the MINIMUM over each subset instead of the mean, and per entry of positions
//       1..n the termination mix (1 - beta_t) (Qx_j - c_j) + beta_t vbar_t, vbar = asac_option.h's option_mean.  A step's
//       beta and its options' values are requested with the step's reward and masks (at clamped indexes, by every lane)
//       and handed to position t + 1 through LDS
//   asac_discrete_q_loss_grad       one workgroup per member
//   asac_discrete_policy_loss_grad  one workgroup; a lane keeps its row's per-branch (max, sum, sum p g, H) in LDS between
//                                   the pass that forms the row's loss and entropies and the pass that writes its gradient
//   asac_discrete_alpha_grad        one workgroup
// Batch means: lane partial (rows tid, tid + 256, ..) -> the tree of k_q_loss (returns.hip) -> one division by B.  No float
// atomics: equal inputs give equal bits.  The argument blocks (branch table, member pointers) are read in place from the
// kernel-argument segment (asac_common.h ASAC_KARG): a lane-dependent member index is an ordinary load, not a private copy.
#include "asac_discrete_rows.h"
#include "asac_option.h"

namespace asac {

// ------------------------------------------------------------------------------------------------------------------------
struct DiscReturnDev {
    asac_vtrace_args_t a;
    asac_discrete_return_t x;
    DiscReturnGeom g;
    // the option's termination mix (kOption only): beta [B, n], the options' values [B, n, O], strides in floats
    const float *beta, *v_options;
    int64_t beta_sb, beta_st, v_sb, v_st, v_so;
    int32_t O;
};

// LDS floats of a workgroup of R rows: the carve, the two [R][pitch] step arrays, the online members' [R][8]
// (`option`: plus the two [P] arrays of the termination mix)
__host__ __device__ __forceinline__ int disc_return_lds_floats(int R, int T, int Dp, int pitch, bool is, bool option) {
    return disc_return_carve_floats(R * T, Dp, is) + 2 * disc_round4(R * pitch) +
           disc_round4(R * ASAC_DISCRETE_MAX_MEMBERS) + (option ? 2 : 0) * disc_round4(R * T);
}

template <bool kOption>
__global__ __launch_bounds__(kDiscThreads) void k_discrete_return(const DiscReturnDev by_value) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ASAC_KARG DiscReturnDev& v = *static_cast<const ASAC_KARG DiscReturnDev*>(kernarg_base());
    const ASAC_KARG asac_vtrace_args_t& a = v.a;
    const ASAC_KARG asac_discrete_return_t& x = v.x;
    const int n = a.n, T = n + 1, R = v.g.R, Dp = v.g.Dp, pitch = v.g.pitch;
    const int B = a.B, P = R * T;
    const bool is = a.use_n_step_is != 0;
    const int NP = disc_round4(P), NS = disc_round4(R * pitch);
    const DiscReturnLds s = disc_return_carve(lds, P, Dp, is);
    float* s_d = s.rest;                 // [R][pitch] per-step term d_t
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

    disc_return_stage<kOption>(&v.a, &v.x, s, row0, R, Dp);                          // phase 0
    __syncthreads();
    disc_return_values<kOption>(&v.a, &v.x, s, row0, R, Dp, s_beta, s_vbar);         // phase 1
    const int Eon = a.td_error_out ? x.q_online.E : 0;
    disc_return_online_q(&v.x, s_qs, row0, R, B, Eon);
    __syncthreads();

    // phase 2
    if (have_step) {
        const int pos = sr * T + st;
        if (is) raw.ratio = s.lpa[pos] / fmaxf(s.mup[pos], 1e-8f);
        float d, c;
        vtrace_step_finish_v(a, raw, s.vn[pos], s.vx[pos + 1], &d, &c);
        s_d[sr * pitch + st] = d;
        s_c[sr * pitch + st] = c;
    }
    __syncthreads();

    // phase 3
    if (tid >= R || row0 + tid >= B) return;
    const int b = row0 + tid;
    const float y = s.vn[tid * T] + vtrace_scan_row(s_d + tid * pitch, s_c + tid * pitch, n, v.g.seg);
    a.y_out[b] = y;
    if (Eon) {
        float sum = 0.f;
        for (int e = 0; e < Eon; ++e) sum += fabsf(s_qs[tid * ASAC_DISCRETE_MAX_MEMBERS + e] - y);
        a.td_error_out[b] = sum / (float)Eon;
    }
}

// the host side both instantiations share (`v`: the option's fields already set, the rest filled here)
template <bool kOption>
static int discrete_return_launch(const asac_vtrace_args_t& h, const asac_discrete_return_t& x, DiscReturnDev& v,
                                  const char* where, void* stream) {
    v.a = h;
    v.x = x;
    if (!h.td_error_out) v.x.q_online.E = 0;
    const bool is = h.use_n_step_is != 0;
    size_t lds;
    const int err = disc_return_geometry<k_discrete_return<kOption>>(
        h.B, h.n, x.branches.D,
        [is](int R, int T, int Dp, int pitch) { return disc_return_lds_floats(R, T, Dp, pitch, is, kOption); }, where,
        &v.g, &lds);
    if (err) return err;
    const int blocks = (h.B + v.g.R - 1) / v.g.R;
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
        disc_q_grad_row(diff, wv, act, x.grad + ((int64_t)e * B + b) * D, B, D, K);
    }
    const float total = disc_tree_sum(red, part);
    if (threadIdx.x == 0) x.loss[e] = total / (float)B;
}

// ------------------------------------------------------------------------------------------------------------------------
struct DiscPolicyDev {
    DiscPolicyRows rows;
    const float* log_alpha;
    float *loss, *entropy, *row_entropy;
    int32_t B;
};

__global__ __launch_bounds__(kDiscThreads) void k_discrete_policy_loss(const DiscPolicyDev by_value) {
    __shared__ DiscPolicyKeep keep;
    __shared__ float red[kDiscThreads];
    const ASAC_KARG DiscPolicyDev& x = *static_cast<const ASAC_KARG DiscPolicyDev*>(kernarg_base());
    const int B = x.B, tid = threadIdx.x;
    const float alpha = expf(*x.log_alpha);
    float part = 0.f, ent = 0.f;
    for (int b = tid; b < B; b += kDiscThreads) {
        const DiscRowTerm r = disc_policy_row(&x.rows, keep, b, B, alpha);
        part += r.term;
        ent += r.h_pi;
        if (x.row_entropy) x.row_entropy[b] = r.h_pi;
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
    const int B = x.B, D = x.br.D;
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += kDiscThreads) {
        const DiscRowTerm r = disc_alpha_row(&x.br, x.logits + (int64_t)b * x.logits_stride, x.target,
                                             x.probs ? x.probs + (int64_t)b * D : nullptr, x.row_entropy != nullptr);
        part += r.term;
        if (x.row_entropy) x.row_entropy[b] = r.h_pi;
    }
    const float total = disc_tree_sum(red, part);
    if (threadIdx.x == 0) *x.slot = total / (float)B;
}

}  // namespace asac

using namespace asac;

extern "C" {

int asac_discrete_return(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host, void* stream) {
    if (!disc_return_args_ok(args_host, job_host) || args_host->B <= 0)
        return bad_arg("asac_discrete_return");
    DiscReturnDev v{};
    return discrete_return_launch<false>(*args_host, *job_host, v, "asac_discrete_return", stream);
}

int asac_option_discrete_return(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host,
                                const float* beta, int64_t beta_stride_b, int64_t beta_stride_t,
                                const float* v_options, int64_t v_stride_b, int64_t v_stride_t, int64_t v_stride_o,
                                int num_options, void* stream) {
    if (!disc_return_args_ok(args_host, job_host) || args_host->B < 0 || !beta ||
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
    DiscPolicyRows& r = x.rows;
    r.br = *branches, r.q = *q;
    r.logits = logits, r.mu = mu, r.subset = subset;
    r.logits_stride = logits_stride, r.mu_stride = mu_stride, r.grad_stride = grad_stride;
    r.grad = grad_logits, r.probs = probs_out, r.penalty = entropy_penalty, r.Es = E_sample;
    x.log_alpha = log_alpha, x.loss = loss_out, x.entropy = entropy_out, x.row_entropy = row_entropy_out, x.B = B;
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
