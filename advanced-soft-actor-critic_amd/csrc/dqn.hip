// Pure-discrete, DQN-like learner (d_action_sizes set, c_action_size == 0, discrete_dqn_like): the arithmetic around the
// critics, three launches (reference sac_base.py: get_dqn_like_d_y 1194-1242 + _get_y 1363-1382, _train_rep_q 1533-1538 /
// 1563-1568, _get_td_error 2219-2244, _choose_action 904-930 without RND).  The per-row target is asac_dqn.h's, the loss
// launch's gradient row asac_discrete_rows.h's (the one asac_discrete_q_loss_grad writes).
//
//   asac_dqn_return       one lane per row, workgroups of 64 rows, no exchange between them: y (and the TD error)
//   asac_dqn_q_loss_grad  one workgroup per online member: each forms its rows' y itself (row-local, kept in registers),
//                         then the member's loss and d loss / d (head outputs); workgroup 0 also stores y.  No workgroup
//                         waits for another; lane partial (rows tid, tid + 256, ..) -> the tree of k_q_loss -> one division
//   asac_dqn_act          one lane per row: greedy one-hot per branch from the first critic's heads, epsilon-random rows
//                         from uniforms drawn by the caller
// No float atomics: equal inputs give equal bits.  The argument blocks are read in place from the kernel-argument segment.
#include "asac_discrete_rows.h"
#include "asac_dqn.h"

namespace asac {

constexpr int kDqnRows = 64;          // rows (= lanes) of a workgroup of the row-per-lane kernels

template <int M>
__global__ __launch_bounds__(kDqnRows) void k_dqn_return(const DqnDev by_value) {
    const ASAC_KARG DqnDev& v = *static_cast<const ASAC_KARG DqnDev*>(kernarg_base());
    const int b = blockIdx.x * kDqnRows + threadIdx.x;
    if (b >= v.a.B) return;
    const float y = dqn_row_target<M>(v.a, v.x, b);
    v.a.y_out[b] = y;
    const int Eon = v.x.q_online.E;             // 0: no TD error asked for
    if (Eon) {
        float s = 0.f;
        for (int e = 0; e < Eon; ++e) s += fabsf(dqn_stored_q(v.x, e, b) - y);
        v.a.td_error_out[b] = s / (float)Eon;
    }
}

struct DqnLossDev {
    DqnDev d;
    const float* w;
    int64_t w_stride;
    float *loss, *grad;
};

template <int M>
__global__ __launch_bounds__(kDiscThreads) void k_dqn_q_loss(const DqnLossDev by_value) {
    __shared__ float red[kDiscThreads];
    const ASAC_KARG DqnLossDev& v = *static_cast<const ASAC_KARG DqnLossDev*>(kernarg_base());
    const ASAC_KARG asac_dqn_job_t& x = v.d.x;
    const int e = blockIdx.x, B = v.d.a.B, D = x.branches.D, K = x.branches.K;
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += kDiscThreads) {
        const float y = dqn_row_target<M>(v.d.a, x, b);
        if (e == 0 && v.d.a.y_out) v.d.a.y_out[b] = y;
        const float wv = v.w ? v.w[(int64_t)b * v.w_stride] : 1.f;
        const float diff = dqn_stored_q(x, e, b) - y;
        part += diff * diff * wv;
        disc_q_grad_row(diff, wv, x.action + (int64_t)b * x.action_stride, v.grad + ((int64_t)e * B + b) * D, B, D, K);
    }
    const float total = disc_tree_sum(red, part);
    if (threadIdx.x == 0) v.loss[e] = total / (float)B;
}

struct DqnActDev {
    asac_branches_t br;
    const float *q, *u;
    int64_t q_stride, u_stride, action_stride;
    float* action;
    float epsilon;
    int32_t B;
};

__global__ __launch_bounds__(kDqnRows) void k_dqn_act(const DqnActDev by_value) {
    const ASAC_KARG DqnActDev& x = *static_cast<const ASAC_KARG DqnActDev*>(kernarg_base());
    const int b = blockIdx.x * kDqnRows + threadIdx.x;
    if (b >= x.B) return;
    const int K = x.br.K;
    const float* q = x.q + (int64_t)b * x.q_stride;
    const float* u = x.u ? x.u + (int64_t)b * x.u_stride : q;      // (q: a valid address where no uniforms are given)
    float* out = x.action + (int64_t)b * x.action_stride;
    const bool random = x.u != nullptr && u[0] < x.epsilon;
    int j0 = 0;
    for (int k = 0; k < K; ++k) {
        const int s = x.br.size[k];
        const float uk = x.u ? u[1 + k] : 0.f;
        int arg = 0;
        float best = 0.f;
        for (int c0 = 0; c0 < s; c0 += 4) {
            float qv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = q[j0 + min(c0 + i, s - 1)];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool take = c0 + i < s && (c0 + i == 0 || qv[i] > best);     // the first maximum
                best = take ? qv[i] : best;
                arg = take ? c0 + i : arg;
            }
        }
        const int pick = random ? min((int)floorf(uk * (float)s), s - 1) : arg;
        for (int j = 0; j < s; ++j) out[j0 + j] = j == pick ? 1.f : 0.f;
        j0 += s;
    }
}

static bool dqn_args_ok(const asac_vtrace_args_t* a, const asac_dqn_job_t* x) {
    if (!a || !x) return false;
    if (a->B < 0 || a->n <= 0 || a->n > ASAC_DISCRETE_MAX_STEPS || !a->reward || !a->done || !a->last_mask ||
        !a->padding_mask || !a->gamma_ratio)
        return false;
    return cat_branches_ok(x->branches) && members_ok(&x->q_eval) && members_ok(&x->q_target) &&
           x->q_eval.E == x->q_target.E && a->E_sample > 0 && a->E_sample <= x->q_target.E;
}

}  // namespace asac

using namespace asac;

extern "C" {

int asac_dqn_return(const asac_vtrace_args_t* args_host, const asac_dqn_job_t* job_host, void* stream) {
    if (!dqn_args_ok(args_host, job_host) || !args_host->y_out) return bad_arg("asac_dqn_return");
    if (args_host->td_error_out && (!members_ok(&job_host->q_online) || !job_host->action))
        return bad_arg("asac_dqn_return: td error");
    DqnDev v{};
    v.a = *args_host;
    v.x = *job_host;
    if (!v.a.td_error_out) v.x.q_online.E = 0;
    if (v.a.B == 0) return 0;
    const dim3 grid((unsigned)((v.a.B + kDqnRows - 1) / kDqnRows));
    if (v.a.E_sample <= 2) {
        ASAC_LAUNCH(k_dqn_return<2>, grid, dim3(kDqnRows), 0, as_stream(stream), v);
    } else {
        ASAC_LAUNCH(k_dqn_return<ASAC_DISCRETE_MAX_MEMBERS>, grid, dim3(kDqnRows), 0, as_stream(stream), v);
    }
    return finish_launch("asac_dqn_return");
}

int asac_dqn_q_loss_grad(const asac_vtrace_args_t* args_host, const asac_dqn_job_t* job_host, const float* w,
                         int64_t w_stride, float* loss_out, float* grad_q, void* stream) {
    if (!dqn_args_ok(args_host, job_host) || !members_ok(&job_host->q_online) || !job_host->action || !loss_out ||
        !grad_q || args_host->B > ASAC_DISCRETE_MAX_ROWS)
        return bad_arg("asac_dqn_q_loss_grad");
    DqnLossDev v{};
    v.d.a = *args_host;
    v.d.x = *job_host;
    v.w = w, v.w_stride = w_stride, v.loss = loss_out, v.grad = grad_q;
    if (v.d.a.B == 0) return 0;
    const dim3 grid((unsigned)job_host->q_online.E);
    if (v.d.a.E_sample <= 2) {
        ASAC_LAUNCH(k_dqn_q_loss<2>, grid, dim3(kDiscThreads), 0, as_stream(stream), v);
    } else {
        ASAC_LAUNCH(k_dqn_q_loss<ASAC_DISCRETE_MAX_MEMBERS>, grid, dim3(kDiscThreads), 0, as_stream(stream), v);
    }
    return finish_launch("asac_dqn_q_loss_grad");
}

int asac_dqn_act(const asac_branches_t* branches, const float* q, int64_t q_stride, const float* u, int64_t u_stride,
                 float epsilon, float* action_out, int64_t action_stride, int B, void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !q || !action_out || B < 0) return bad_arg("asac_dqn_act");
    if (B == 0) return 0;
    DqnActDev x{};
    x.br = *branches;
    x.q = q, x.u = u, x.q_stride = q_stride, x.u_stride = u_stride, x.action_stride = action_stride;
    x.action = action_out, x.epsilon = epsilon, x.B = B;
    ASAC_LAUNCH(k_dqn_act, dim3((unsigned)((B + kDqnRows - 1) / kDqnRows)), dim3(kDqnRows), 0, as_stream(stream), x);
    return finish_launch("asac_dqn_act");
}

}  // extern "C"
