// Hybrid action spaces (d_action_sizes set AND c_action_size > 0), policy-based SAC: the learner's row-wise arithmetic
// around the networks, one launch per item (reference sac_base.py: _get_y 1383-1464 + _v_trace 1244-1295, _train_rep_q
// 1533-1568, _train_policy 1858-1903, _train_alpha 1924-1944, _get_td_error 2219-2244).  The reference's hybrid loss, TD
// error and temperature loss each sum a discrete and a continuous term per row, so each launch here forms both heads'
// quantities.  Nothing of either head's arithmetic is written here: the discrete rows are asac_discrete_rows.h's (the
// functions discrete.hip calls), the continuous leg is asac_vtrace.h's (step load / finish, row scan) and asac_common.h's
// (clipped_q_loss_row, policy_loss_row).  This file holds the argument blocks, how the two legs share a lane, and the sums.
//
//   asac_hybrid_return            the categorical return's workgroup of R rows (disc_return_stage / disc_return_values,
//       the calls of k_discrete_return's plain instantiation) with a continuous leg: the lane that owns step (row, t) loads
//       the step ONCE with vtrace_step_load on the continuous block — reward, masks and ratios serve both scans, the two
//       blocks agree on them — and finishes it twice; the lane that owns a row scans twice (vtrace_scan_row, the `seg` rule
//       of k_td_update).  d_y has the bits of asac_discrete_return, c_y those of asac_vtrace_return_min
//   asac_hybrid_q_loss_grad       one workgroup per member: disc_q_grad_row and clipped_q_loss_row
//   asac_hybrid_policy_loss_grad  one workgroup: disc_policy_row and policy_loss_row
//   asac_hybrid_alpha_grad        one workgroup, both temperature slots: disc_alpha_row and k_alpha_grad's line
// Batch means: lane partial (rows tid, tid + 256, ..) -> the tree of k_q_loss -> one division by B.  No float atomics: equal
// inputs give equal bits.  Argument blocks are read in place from the kernel-argument segment (asac_common.h ASAC_KARG).
#include "asac_discrete_rows.h"

namespace asac {

// ------------------------------------------------------------------------------------------------------------------------
struct HybridReturnDev {
    asac_vtrace_args_t d, c;         // the discrete and the continuous return's blocks
    asac_discrete_return_t x;
    float* td;                       // the summed TD error (NULL: none)
    DiscReturnGeom g;
};

// LDS floats of a workgroup of R rows: the carve, the two [R][pitch] step arrays of each leg, the online members' [R][8]
// and the continuous leg's [R] V(s_0)
__host__ __device__ __forceinline__ int hybrid_return_lds_floats(int R, int T, int Dp, int pitch, bool is) {
    return disc_return_carve_floats(R * T, Dp, is) + 4 * disc_round4(R * pitch) +
           disc_round4(R * ASAC_DISCRETE_MAX_MEMBERS) + disc_round4(R);
}

__global__ __launch_bounds__(kDiscThreads) void k_hybrid_return(const HybridReturnDev by_value) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ASAC_KARG HybridReturnDev& v = *static_cast<const ASAC_KARG HybridReturnDev*>(kernarg_base());
    const ASAC_KARG asac_vtrace_args_t& a = v.d;
    const ASAC_KARG asac_vtrace_args_t& ca = v.c;
    const ASAC_KARG asac_discrete_return_t& x = v.x;
    const int n = a.n, T = n + 1, R = v.g.R, Dp = v.g.Dp, pitch = v.g.pitch;
    const int B = a.B, P = R * T;
    const bool is = a.use_n_step_is != 0;
    const int NS = disc_round4(R * pitch);
    const DiscReturnLds s = disc_return_carve(lds, P, Dp, is);
    float* s_d = s.rest;                 // [R][pitch] per-step term d_t, discrete
    float* s_c = s_d + NS;               // [R][pitch] trace-cutting factor c_t, discrete
    float* s_dc = s_c + NS;              // [R][pitch] d_t, continuous
    float* s_cc = s_dc + NS;             // [R][pitch] c_t, continuous
    float* s_qs = s_cc + NS;             // [R][8] the online members' discrete value of the stored action at t = 0
    float* s_v0 = s_qs + disc_round4(R * ASAC_DISCRETE_MAX_MEMBERS);     // [R] the continuous V(s_0)
    const int row0 = blockIdx.x * R;
    const int tid = threadIdx.x;

    // the step (row, t) this lane finishes in phase 2 (R * n <= R * T <= 256): ONE load of it, on the continuous block —
    // reward, masks and ratios are the discrete block's too (the host refuses blocks that differ in them)
    VtraceStepRaw craw{};
    const int sr = tid / n, st = tid - sr * n;
    const bool have_step = tid < R * n && row0 + sr < B;
    if (have_step) craw = vtrace_step_load(ca, row0 + sr, st);

    disc_return_stage<false>(&v.d, &v.x, s, row0, R, Dp);        // phase 0
    __syncthreads();
    disc_return_values<false>(&v.d, &v.x, s, row0, R, Dp);       // phase 1
    const int Eon = v.td ? x.q_online.E : 0;
    disc_return_online_q(&v.x, s_qs, row0, R, B, Eon);
    __syncthreads();

    // phase 2: the step finished twice
    if (have_step) {
        const int pos = sr * T + st;
        VtraceStepRaw draw = craw;           // reward, g, keep and the two ratios of the step; its own pi / mu ratio
        draw.ratio = is ? s.lpa[pos] / fmaxf(s.mup[pos], 1e-8f) : 1.f;
        float d, c;
        vtrace_step_finish_v(a, draw, s.vn[pos], s.vx[pos + 1], &d, &c);
        s_d[sr * pitch + st] = d;
        s_c[sr * pitch + st] = c;
        const float v_t = vtrace_step_finish(ca, craw, expf(*ca.log_alpha), &d, &c);
        if (st == 0) s_v0[sr] = v_t;
        s_dc[sr * pitch + st] = d;
        s_cc[sr * pitch + st] = c;
    }
    __syncthreads();

    // phase 3: the row scanned twice
    if (tid >= R || row0 + tid >= B) return;
    const int b = row0 + tid;
    const float dy = s.vn[tid * T] + vtrace_scan_row(s_d + tid * pitch, s_c + tid * pitch, n, v.g.seg);
    const float cy = s_v0[tid] + vtrace_scan_row(s_dc + tid * pitch, s_cc + tid * pitch, n, v.g.seg);
    a.y_out[b] = dy;
    ca.y_out[b] = cy;
    if (Eon) {      // mean_e (|qs_e - d_y| + |c_q_e - c_y|): per member the discrete addend first, members in order
        float sum = 0.f;
        for (int e = 0; e < Eon; ++e)
            sum += fabsf(s_qs[tid * ASAC_DISCRETE_MAX_MEMBERS + e] - dy) + fabsf(ca.q_online[(int64_t)e * B + b] - cy);
        v.td[b] = sum / (float)Eon;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct HybridQLossDev {
    asac_branches_t br;
    asac_members_t q;
    const float *action, *cq, *tq, *dy, *cy, *w;
    int64_t action_stride, dy_stride, cy_stride, w_stride;
    float *loss, *grad_qd, *grad_cq;
    float clip_eps;
    int32_t B;
};

__global__ __launch_bounds__(kDiscThreads) void k_hybrid_q_loss(const HybridQLossDev by_value) {
    __shared__ float red[kDiscThreads];
    const ASAC_KARG HybridQLossDev& x = *static_cast<const ASAC_KARG HybridQLossDev*>(kernarg_base());
    const int e = blockIdx.x, B = x.B, D = x.br.D, K = x.br.K;
    const float* qe = x.q.base[e];
    const float inv_b = 1.f / (float)B;                 // (k_q_loss's scaling of the continuous gradient)
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += kDiscThreads) {
        const float* act = x.action + (int64_t)b * x.action_stride;
        const float dyv = x.dy[(int64_t)b * x.dy_stride], cyv = x.cy[(int64_t)b * x.cy_stride];
        const float wv = x.w ? x.w[(int64_t)b * x.w_stride] : 1.f;
        const float cqv = x.cq[(int64_t)e * B + b], tqv = x.tq[(int64_t)e * B + b];
        const float qs = disc_dot(act, qe + (int64_t)b * x.q.stride_b, D) / (float)K;
        const float diff = qs - dyv;
        disc_q_grad_row(diff, wv, act, x.grad_qd + ((int64_t)e * B + b) * D, B, D, K);
        // the continuous term, unweighted (the row's two terms are added, then weighted), and its gradient, weighted as
        // clipped_q_loss_row weights it
        float gc;
        const float lc = clipped_q_loss_row(cqv, tqv, cyv, 1.f, x.clip_eps, &gc);
        x.grad_cq[(int64_t)e * B + b] = inv_b * (wv * gc);
        part += (diff * diff + lc) * wv;
    }
    const float total = disc_tree_sum(red, part);
    if (threadIdx.x == 0) x.loss[e] = total / (float)B;
}

// ------------------------------------------------------------------------------------------------------------------------
struct HybridPolicyDev {
    DiscPolicyRows rows;             // (q: the online members' discrete head outputs at the stored continuous action)
    const float *log_d_alpha, *log_c_alpha, *logp, *cq, *scale;
    const int32_t* subset_c;
    int64_t scale_stride;
    float *loss, *grad_logp, *grad_cq, *d_entropy, *c_entropy;
    int32_t B, E, Es, A;
};

__global__ __launch_bounds__(kDiscThreads) void k_hybrid_policy_loss(const HybridPolicyDev by_value) {
    __shared__ DiscPolicyKeep keep;
    __shared__ float red[kDiscThreads];
    const ASAC_KARG HybridPolicyDev& x = *static_cast<const ASAC_KARG HybridPolicyDev*>(kernarg_base());
    const int B = x.B, E = x.E, Es = x.Es, A = x.A, tid = threadIdx.x;
    const float alpha = expf(*x.log_d_alpha), c_alpha = expf(*x.log_c_alpha);
    const float inv_b = 1.f / (float)B;                 // (k_policy_loss's scaling of the continuous gradients)
    float part = 0.f, ent = 0.f, c_ent = 0.f;
    for (int b = tid; b < B; b += kDiscThreads) {
        const DiscRowTerm r = disc_policy_row(&x.rows, keep, b, B, alpha);
        ent += r.h_pi;
        part += r.term + policy_loss_row(x.logp, x.cq, x.subset_c, E, Es, B, b, c_alpha, inv_b, x.grad_logp, x.grad_cq);
        for (int d = 0; d < A; ++d) c_ent += logf(x.scale[(int64_t)b * x.scale_stride + d]) + 1.4189385332046727f;
    }
    const float loss = disc_tree_sum(red, part);
    __syncthreads();
    const float entropy = disc_tree_sum(red, ent);
    __syncthreads();
    const float c_entropy = disc_tree_sum(red, c_ent);
    if (tid == 0) {
        *x.loss = loss / (float)B;
        *x.d_entropy = entropy / (float)B;
        *x.c_entropy = c_entropy / (float)B;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct HybridAlphaDev {
    asac_branches_t br;
    const float *logits, *target_d, *logp;
    int64_t logits_stride;
    float* slots;                    // [log_d_alpha, log_c_alpha]
    float target_c;
    int32_t B;
};

__global__ __launch_bounds__(kDiscThreads) void k_hybrid_alpha_grad(const HybridAlphaDev by_value) {
    __shared__ float red[kDiscThreads];
    const ASAC_KARG HybridAlphaDev& x = *static_cast<const ASAC_KARG HybridAlphaDev*>(kernarg_base());
    const int B = x.B;
    float part = 0.f, c_part = 0.f;
    for (int b = threadIdx.x; b < B; b += kDiscThreads) {
        part += disc_alpha_row(&x.br, x.logits + (int64_t)b * x.logits_stride, x.target_d, nullptr, false).term;
        c_part += -x.logp[b] - x.target_c;      // (k_alpha_grad's)
    }
    const float total = disc_tree_sum(red, part);
    __syncthreads();
    const float c_total = disc_tree_sum(red, c_part);
    if (threadIdx.x == 0) {
        x.slots[0] = total / (float)B;
        x.slots[1] = c_total / (float)B;
    }
}

// the blocks of one hybrid return: the discrete one as asac_discrete_return takes it, the same step data in both, and the
// continuous one complete for its own launch
static bool hybrid_return_args_ok(const asac_vtrace_args_t* d_host, const asac_vtrace_args_t* c_host,
                                  const asac_discrete_return_t* job_host, const float* td) {
    if (!disc_return_args_ok(d_host, job_host) || !c_host || d_host->B < 0) return false;
    const asac_vtrace_args_t &d = *d_host, &c = *c_host;
    const asac_discrete_return_t& x = *job_host;
    if (c.B != d.B || c.n != d.n || c.reward != d.reward || c.reward_stride != d.reward_stride || c.done != d.done ||
        c.last_mask != d.last_mask || c.padding_mask != d.padding_mask || c.mask_stride != d.mask_stride ||
        c.gamma_ratio != d.gamma_ratio || c.lambda_ratio != d.lambda_ratio || c.gamma != d.gamma || c.v_rho != d.v_rho ||
        c.v_c != d.v_c || (c.use_n_step_is != 0) != (d.use_n_step_is != 0))
        return false;
    if (!c.y_out || c.y_out == d.y_out || !c.q || !c.logp || !c.log_alpha || c.E_sample <= 0 ||
        c.E_sample > x.q_target.E || c.A <= 0 || c.A > ASAC_MAX_ACTION)
        return false;
    if (c.use_n_step_is && (!c.mu_prob || !c.pi_prob)) return false;
    if (d.td_error_out || c.td_error_out) return false;
    if (td && (!members_ok(&x.q_online) || !x.action || !c.q_online || c.E_online != x.q_online.E)) return false;
    return true;
}

}  // namespace asac

using namespace asac;

extern "C" {

int asac_hybrid_return(const asac_vtrace_args_t* d_args, const asac_vtrace_args_t* c_args,
                       const asac_discrete_return_t* job, float* td_error_out, void* stream) {
    const char* where = "asac_hybrid_return";
    if (!hybrid_return_args_ok(d_args, c_args, job, td_error_out)) return bad_arg(where);
    const asac_vtrace_args_t& h = *d_args;
    if (h.B == 0) return 0;
    HybridReturnDev v{};
    v.d = h, v.c = *c_args, v.x = *job;
    v.td = td_error_out;
    if (!td_error_out) v.x.q_online.E = 0;
    const bool is = h.use_n_step_is != 0;
    size_t lds;
    const int err = disc_return_geometry<k_hybrid_return>(
        h.B, h.n, job->branches.D,
        [is](int R, int T, int Dp, int pitch) { return hybrid_return_lds_floats(R, T, Dp, pitch, is); }, where, &v.g, &lds);
    if (err) return err;
    const int blocks = (h.B + v.g.R - 1) / v.g.R;
    ASAC_LAUNCH(k_hybrid_return, dim3((unsigned)blocks), dim3(kDiscThreads), lds, as_stream(stream), v);
    return finish_launch(where);
}

int asac_hybrid_q_loss_grad(const asac_branches_t* branches, const asac_members_t* q_d, const float* action,
                            int64_t action_stride, const float* cq, const float* tq, const float* d_y, int64_t d_y_stride,
                            const float* c_y, int64_t c_y_stride, const float* w, int64_t w_stride, int B, float clip_eps,
                            float* loss_out, float* grad_qd, float* grad_cq, void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !members_ok(q_d) || !action || !cq || !tq || !d_y || !c_y ||
        !loss_out || !grad_qd || !grad_cq || !(clip_eps > 0.f) || B < 0 || B > ASAC_DISCRETE_MAX_ROWS)
        return bad_arg("asac_hybrid_q_loss_grad");
    if (B == 0) return 0;
    HybridQLossDev x{};
    x.br = *branches, x.q = *q_d;
    x.action = action, x.cq = cq, x.tq = tq, x.dy = d_y, x.cy = c_y, x.w = w;
    x.action_stride = action_stride, x.dy_stride = d_y_stride, x.cy_stride = c_y_stride, x.w_stride = w_stride;
    x.loss = loss_out, x.grad_qd = grad_qd, x.grad_cq = grad_cq, x.clip_eps = clip_eps, x.B = B;
    ASAC_LAUNCH(k_hybrid_q_loss, dim3((unsigned)q_d->E), dim3(kDiscThreads), 0, as_stream(stream), x);
    return finish_launch("asac_hybrid_q_loss_grad");
}

int asac_hybrid_policy_loss_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                                 const asac_members_t* q_d, const int32_t* subset_d, const float* mu, int64_t mu_stride,
                                 const float* log_d_alpha, float entropy_penalty, const float* logp, const float* cq,
                                 const int32_t* subset_c, int E_sample, const float* log_c_alpha, const float* scale,
                                 int64_t scale_stride, int A, int B, float* loss_out, float* grad_logits,
                                 int64_t grad_stride, float* grad_logp, float* grad_cq, float* d_entropy_out,
                                 float* c_entropy_out, void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !logits || !members_ok(q_d) || E_sample <= 0 || E_sample > q_d->E ||
        !mu || !log_d_alpha || !logp || !cq || !log_c_alpha || !scale || A <= 0 || A > ASAC_MAX_ACTION ||
        scale_stride < A || !loss_out || !grad_logits || !grad_logp || !grad_cq || !d_entropy_out || !c_entropy_out ||
        B < 0 || B > ASAC_DISCRETE_MAX_ROWS)
        return bad_arg("asac_hybrid_policy_loss_grad");
    if (B == 0) return 0;
    HybridPolicyDev x{};
    DiscPolicyRows& r = x.rows;
    r.br = *branches, r.q = *q_d;
    r.logits = logits, r.mu = mu, r.subset = subset_d;
    r.logits_stride = logits_stride, r.mu_stride = mu_stride, r.grad_stride = grad_stride;
    r.grad = grad_logits, r.penalty = entropy_penalty, r.Es = E_sample;
    x.log_d_alpha = log_d_alpha, x.log_c_alpha = log_c_alpha;
    x.logp = logp, x.cq = cq, x.scale = scale, x.subset_c = subset_c, x.scale_stride = scale_stride;
    x.loss = loss_out, x.grad_logp = grad_logp, x.grad_cq = grad_cq;
    x.d_entropy = d_entropy_out, x.c_entropy = c_entropy_out;
    x.B = B, x.E = q_d->E, x.Es = E_sample, x.A = A;
    ASAC_LAUNCH(k_hybrid_policy_loss, dim3(1), dim3(kDiscThreads), 0, as_stream(stream), x);
    return finish_launch("asac_hybrid_policy_loss_grad");
}

int asac_hybrid_alpha_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                           const float* target_d, const float* logp, float target_c, int B, float* grad_slots,
                           void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !logits || !target_d || !logp || !grad_slots || B < 0 ||
        B > ASAC_DISCRETE_MAX_ROWS)
        return bad_arg("asac_hybrid_alpha_grad");
    if (B == 0) return 0;
    HybridAlphaDev x{};
    x.br = *branches;
    x.logits = logits, x.target_d = target_d, x.logp = logp, x.logits_stride = logits_stride;
    x.slots = grad_slots, x.target_c = target_c, x.B = B;
    ASAC_LAUNCH(k_hybrid_alpha_grad, dim3(1), dim3(kDiscThreads), 0, as_stream(stream), x);
    return finish_launch("asac_hybrid_alpha_grad");
}

}  // extern "C"
