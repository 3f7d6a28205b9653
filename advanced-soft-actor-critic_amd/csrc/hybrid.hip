// Hybrid action spaces (d_action_sizes set AND c_action_size > 0), policy-based SAC: the learner's row-wise arithmetic
// around the networks, one launch per item (reference sac_base.py: _get_y 1383-1464 + _v_trace 1244-1295, _train_rep_q
// 1533-1568, _train_policy 1858-1903, _train_alpha 1924-1944, _get_td_error 2219-2244).  The reference's hybrid loss, TD
// error and temperature loss each sum a discrete and a continuous term per row, so each launch here forms both heads'
// quantities.  The pieces are the shared ones: asac_categorical.h (branch softmax, subset means, the reduction tree),
// asac_vtrace.h (step load / finish, row scan), asac_common.h (the clipped Q loss of one row).
//
//   asac_hybrid_return            k_discrete_return's workgroup of R rows (discrete.hip: phases 0 and 1 are its plain
//       instantiation's, operation for operation) with a continuous leg: the lane that owns step (row, t) loads the step ONCE
//       with vtrace_step_load on the continuous block — reward, masks and ratios serve both scans, the two blocks agree on
//       them — and finishes it twice; the lane that owns a row scans twice (vtrace_scan_row, the `seg` rule of
//       k_td_update).  d_y has the bits of asac_discrete_return, c_y those of asac_vtrace_return_min
//   asac_hybrid_q_loss_grad       one workgroup per member
//   asac_hybrid_policy_loss_grad  one workgroup; the discrete row term is k_discrete_policy_loss's, the continuous one
//                                 k_policy_loss's (returns.hip)
//   asac_hybrid_alpha_grad        one workgroup, both temperature slots
// Batch means: lane partial (rows tid, tid + 256, ..) -> the tree of k_q_loss -> one division by B.  No float atomics: equal
// inputs give equal bits.  Argument blocks are read in place from the kernel-argument segment (asac_common.h ASAC_KARG).
#include "asac_common.h"
#include "asac_vtrace.h"
#include "asac_categorical.h"

namespace asac {

// ------------------------------------------------------------------------------------------------------------------------
struct HybridReturnDev {
    asac_vtrace_args_t d, c;         // the discrete and the continuous return's blocks
    asac_discrete_return_t x;
    float* td;                       // the summed TD error (NULL: none)
    int32_t R, Dp, pitch, seg;       // rows per workgroup, LDS pitch of a position's entries, of a row's steps, scan lanes
};

__host__ __device__ __forceinline__ int hyb_round4(int v) { return (v + 3) & ~3; }
// LDS floats of a workgroup of R rows (every part a multiple of four floats): k_discrete_return's, then the continuous
// leg's two [R][pitch] step arrays and its [R] V(s_0)
__host__ __device__ __forceinline__ int hybrid_return_lds_floats(int R, int T, int Dp, int pitch, bool is) {
    const int P = R * T;
    return (is ? 5 : 3) * hyb_round4(P * Dp) + 4 * hyb_round4(P) + 4 * hyb_round4(R * pitch) +
           hyb_round4(R * ASAC_DISCRETE_MAX_MEMBERS) + hyb_round4(R);
}

__global__ __launch_bounds__(kDiscThreads) void k_hybrid_return(const HybridReturnDev by_value) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ASAC_KARG HybridReturnDev& v = *static_cast<const ASAC_KARG HybridReturnDev*>(kernarg_base());
    const ASAC_KARG asac_vtrace_args_t& a = v.d;
    const ASAC_KARG asac_vtrace_args_t& ca = v.c;
    const ASAC_KARG asac_discrete_return_t& x = v.x;
    const int n = a.n, T = n + 1, R = v.R, D = x.branches.D, K = x.branches.K, Dp = v.Dp, pitch = v.pitch;
    const int B = a.B, P = R * T;
    const bool is = a.use_n_step_is != 0;
    const int NE = hyb_round4(P * Dp), NP = hyb_round4(P), NS = hyb_round4(R * pitch);
    float* s_z = lds;                    // [P][Dp] logits
    float* s_qn = s_z + NE;              // [P][Dp] mean over subset_n of the target members' values
    float* s_qx = s_qn + NE;             // [P][Dp] ... over subset_next
    float* s_a = s_qx + NE;              // [P][Dp] stored action            (importance sampling only)
    float* s_mu = s_a + (is ? NE : 0);   // [P][Dp] mu * stored action       (importance sampling only)
    float* s_vn = s_mu + (is ? NE : 0);  // [P] V with subset_n
    float* s_vx = s_vn + NP;             // [P] V with subset_next
    float* s_lpa = s_vx + NP;            // [P] log pi(stored action)
    float* s_mup = s_lpa + NP;           // [P] prod_j (mu_j a_j, zeros -> 1)
    float* s_d = s_mup + NP;             // [R][pitch] per-step term d_t, discrete
    float* s_c = s_d + NS;               // [R][pitch] trace-cutting factor c_t, discrete
    float* s_dc = s_c + NS;              // [R][pitch] d_t, continuous
    float* s_cc = s_dc + NS;             // [R][pitch] c_t, continuous
    float* s_qs = s_cc + NS;             // [R][8] the online members' discrete value of the stored action at t = 0
    float* s_v0 = s_qs + hyb_round4(R * ASAC_DISCRETE_MAX_MEMBERS);      // [R] the continuous V(s_0)
    const int row0 = blockIdx.x * R;
    const int tid = threadIdx.x;

    // the step (row, t) this lane finishes in phase 2 (R * n <= R * T <= 256): ONE load of it, on the continuous block —
    // reward, masks and ratios are the discrete block's too (the host refuses blocks that differ in them)
    VtraceStepRaw craw{};
    const int sr = tid / n, st = tid - sr * n;
    const bool have_step = tid < R * n && row0 + sr < B;
    if (have_step) craw = vtrace_step_load(ca, row0 + sr, st);

    // phase 0 (k_discrete_return<false>'s)
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
        const float qn = cat_member_mean(x.q_target, a.subset_n, Es, qoff);
        const float qx = cat_member_mean(x.q_target, a.subset_next, Es, qoff);
        const int o = pos * Dp + j;
        s_z[o] = z, s_qn[o] = qn, s_qx[o] = qx;
        if (is) s_a[o] = av, s_mu[o] = mv * av;
    }
    __syncthreads();

    // phase 1 (k_discrete_return<false>'s)
    const float alpha = expf(*a.log_alpha);
    if (tid < P && row0 + tid / T < B) {
        const int pos = tid;
        float vn = 0.f, vx = 0.f, lpa = 0.f, mu = 1.f;
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
    const int Eon = v.td ? x.q_online.E : 0;
    for (int i = tid; i < R * Eon; i += kDiscThreads) {
        const int r = i / Eon, e = i - r * Eon, b = row0 + r;
        if (b >= B) continue;
        const float s = disc_dot(x.action + (int64_t)b * x.action_stride_b,
                                 x.q_online.base[e] + (int64_t)b * x.q_online.stride_b, D);
        s_qs[r * ASAC_DISCRETE_MAX_MEMBERS + e] = s / (float)K;
    }
    __syncthreads();

    // phase 2: the step finished twice
    if (have_step) {
        const int pos = sr * T + st;
        VtraceStepRaw draw = craw;           // reward, g, keep and the two ratios of the step; its own pi / mu ratio
        draw.ratio = is ? expf(s_lpa[pos]) / fmaxf(s_mup[pos], 1e-8f) : 1.f;
        float d, c;
        vtrace_step_finish_v(a, draw, s_vn[pos], s_vx[pos + 1], &d, &c);
        s_d[sr * pitch + st] = d;
        s_c[sr * pitch + st] = c;
        // vtrace_step_finish (asac_vtrace.h) on the continuous block
        const float c_alpha = expf(*ca.log_alpha);
        const float v_t = craw.m0 - c_alpha * craw.lp0, v_next = craw.m1 - c_alpha * craw.lp1;
        vtrace_step_finish_v(ca, craw, v_t, v_next, &d, &c);
        if (st == 0) s_v0[sr] = v_t;
        s_dc[sr * pitch + st] = d;
        s_cc[sr * pitch + st] = c;
    }
    __syncthreads();

    // phase 3: the row scanned twice
    if (tid >= R || row0 + tid >= B) return;
    const int b = row0 + tid;
    const float dy = s_vn[tid * T] + vtrace_scan_row(s_d + tid * pitch, s_c + tid * pitch, n, v.seg);
    const float cy = s_v0[tid] + vtrace_scan_row(s_dc + tid * pitch, s_cc + tid * pitch, n, v.seg);
    a.y_out[b] = dy;
    ca.y_out[b] = cy;
    if (Eon) {      // mean_e (|qs_e - d_y| + |c_q_e - c_y|): per member the discrete addend first, members in order
        float s = 0.f;
        for (int e = 0; e < Eon; ++e)
            s += fabsf(s_qs[tid * ASAC_DISCRETE_MAX_MEMBERS + e] - dy) + fabsf(ca.q_online[(int64_t)e * B + b] - cy);
        v.td[b] = s / (float)Eon;
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
        // the discrete term and its gradient (k_discrete_q_loss's)
        const float qs = disc_dot(act, qe + (int64_t)b * x.q.stride_b, D) / (float)K;
        const float diff = qs - dyv;
        const float gq = 2.f * diff * wv / (float)B / (float)K;
        float* g = x.grad_qd + ((int64_t)e * B + b) * D;
        for (int j = 0; j < D; ++j) g[j] = gq * act[j];
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
    asac_branches_t br;
    asac_members_t q;                // the online members' discrete head outputs at the stored continuous action
    const float *logits, *mu, *log_d_alpha, *log_c_alpha, *logp, *cq, *scale;
    const int32_t *subset_d, *subset_c;
    int64_t logits_stride, mu_stride, grad_stride, scale_stride;
    float *loss, *grad_logits, *grad_logp, *grad_cq, *d_entropy, *c_entropy;
    float penalty;
    int32_t B, E, Es, A;
};

__global__ __launch_bounds__(kDiscThreads) void k_hybrid_policy_loss(const HybridPolicyDev by_value) {
    // a lane's per-branch (max, sum exp, sum_j p_j g_j, H_k) of the row it is on, kept between its two passes
    __shared__ float s_m[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads], s_sum[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads];
    __shared__ float s_S[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads], s_H[ASAC_DISCRETE_MAX_BRANCHES * kDiscThreads];
    __shared__ float red[kDiscThreads];
    const ASAC_KARG HybridPolicyDev& x = *static_cast<const ASAC_KARG HybridPolicyDev*>(kernarg_base());
    const int B = x.B, K = x.br.K, E = x.E, Es = x.Es, A = x.A, tid = threadIdx.x;
    const float alpha = expf(*x.log_d_alpha), c_alpha = expf(*x.log_c_alpha);
    const float inv_b = 1.f / (float)B;                 // (k_policy_loss's scaling of the continuous gradients)
    float part = 0.f, ent = 0.f, c_ent = 0.f;
    for (int b = tid; b < B; b += kDiscThreads) {
        // the discrete row term and its gradient (k_discrete_policy_loss's)
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
                const float qbar = cat_member_mean(x.q, x.subset_d, Es, qrow + j0 + j);
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
        const float row_d = main + x.penalty * (dh * dh / 2.f);
        ent += h_pi;
        const float coef = x.penalty / (float)K * dh;
        float* grad = x.grad_logits + (int64_t)b * x.grad_stride;
        j0 = 0;
        for (int k = 0; k < K; ++k) {
            const int s = x.br.size[k];
            const CatStats cs = cat_stats_from(s_m[k * kDiscThreads + tid], s_sum[k * kDiscThreads + tid]);
            const float S = s_S[k * kDiscThreads + tid], H = s_H[k * kDiscThreads + tid];
            for (int j = 0; j < s; ++j) {
                const float zz = z[j0 + j];
                const float p = cat_prob(zz, cs), lp = cat_logp(zz, cs);
                const float c = alpha * cat_cl(p);
                const float qbar = cat_member_mean(x.q, x.subset_d, Es, qrow + j0 + j);
                const float g = (c - qbar + alpha * cat_cl_open(p)) / (float)K;
                grad[j0 + j] = (p * (g - S) + coef * (p * (lp + H))) / (float)B;
            }
            j0 += s;
        }
        // the continuous row term and its gradients (k_policy_loss's)
        int best = x.subset_c ? x.subset_c[0] : 0;
        float m = x.cq[(int64_t)best * B + b];
        for (int k = 1; k < Es; ++k) {
            const int e = x.subset_c ? x.subset_c[k] : k;
            const float val = x.cq[(int64_t)e * B + b];
            if (val < m) {
                m = val;
                best = e;
            }
        }
        for (int e = 0; e < E; ++e) x.grad_cq[(int64_t)e * B + b] = (e == best) ? -inv_b : 0.f;
        x.grad_logp[b] = c_alpha * inv_b;
        part += row_d + (c_alpha * x.logp[b] - m);
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
    const int B = x.B, K = x.br.K;
    float part = 0.f, c_part = 0.f;
    for (int b = threadIdx.x; b < B; b += kDiscThreads) {
        const float* z = x.logits + (int64_t)b * x.logits_stride;
        float row = 0.f;
        int j0 = 0;
        for (int k = 0; k < K; ++k) {      // (k_discrete_alpha_grad's)
            const int s = x.br.size[k];
            const CatStats cs = cat_stats(z + j0, s);
            for (int j = 0; j < s; ++j) {
                const float p = cat_prob(z[j0 + j], cs);
                row += p * (-cat_cl(p) - x.target_d[j0 + j]);
            }
            j0 += s;
        }
        part += row / (float)K;
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

// the blocks of one hybrid return: each complete for its own launch, and the same step data in both
static bool hybrid_return_args_ok(const asac_vtrace_args_t* d_host, const asac_vtrace_args_t* c_host,
                                  const asac_discrete_return_t* job_host, const float* td) {
    if (!d_host || !c_host || !job_host) return false;
    const asac_vtrace_args_t &d = *d_host, &c = *c_host;
    const asac_discrete_return_t& x = *job_host;
    if (d.B < 0 || d.n <= 0 || d.n > ASAC_DISCRETE_MAX_STEPS || !d.y_out || !d.reward || !d.done || !d.last_mask ||
        !d.padding_mask || !d.gamma_ratio || !d.log_alpha || !x.logits || !cat_branches_ok(x.branches) ||
        !members_ok(&x.q_target) || d.E_sample <= 0 || d.E_sample > x.q_target.E)
        return false;
    if (d.use_n_step_is && (!d.mu_prob || !d.lambda_ratio || !x.action)) return false;
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
    const int T = h.n + 1, D = job->branches.D;
    const bool is = h.use_n_step_is != 0;
    v.Dp = D | 1;                                 // odd pitches: conflict-free position-per-lane / row-per-lane reads
    v.pitch = (h.n + 1) | 1;
    // rows per workgroup (asac_discrete_return's rule): one lane per window position, a few rounds of phase 0 at most,
    // and the LDS they need
    int R = kDiscThreads / T;
    if (R > 2048 / (T * D)) R = 2048 / (T * D);
    if (R > h.B) R = h.B;
    if (R < 1) R = 1;
    while (R > 1 && (size_t)hybrid_return_lds_floats(R, T, v.Dp, v.pitch, is) * sizeof(float) > 64 * 1024) --R;
    v.R = R;
    v.seg = vtrace_scan_lanes(h.B, h.n);
    const size_t lds = (size_t)hybrid_return_lds_floats(R, T, v.Dp, v.pitch, is) * sizeof(float);
    if (lds > 64 * 1024) {                        // one row of a long, wide window under importance sampling (<= 88 KB)
        static bool raised = false;
        if (!raised) {
            hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_hybrid_return),
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
    x.br = *branches, x.q = *q_d;
    x.logits = logits, x.mu = mu, x.log_d_alpha = log_d_alpha, x.log_c_alpha = log_c_alpha;
    x.logp = logp, x.cq = cq, x.scale = scale, x.subset_d = subset_d, x.subset_c = subset_c;
    x.logits_stride = logits_stride, x.mu_stride = mu_stride, x.grad_stride = grad_stride, x.scale_stride = scale_stride;
    x.loss = loss_out, x.grad_logits = grad_logits, x.grad_logp = grad_logp, x.grad_cq = grad_cq;
    x.d_entropy = d_entropy_out, x.c_entropy = c_entropy_out;
    x.penalty = entropy_penalty, x.B = B, x.E = q_d->E, x.Es = E_sample, x.A = A;
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
