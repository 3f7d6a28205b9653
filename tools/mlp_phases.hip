// Phase timeline of the fused MLP backward (workgroup (0,0), 100 MHz wall clock): includes the library source with
// ASAC_MLP_STAMPS, drives it through its C ABI at the train step's shapes (N = 256 rows, E = 2 stock Q networks /
// the stock policy) and prints the time between stamps, averaged over launches.  The policy -> sample -> critics forward
// runs at the step's N = 1 280 rows, E = 2, A = 2, S = 6 with all three side jobs on, on plain rows and on ring-addressed
// rows; its side waves (threads 256, 320, 384) stamp the end of their two steps.  The one-launch policy step is stamped
// three times: with the action given, with the action sampled inside the launch, and with the action given and the
// policy's forward loaded from a saved tile (the headline step's form; the saved values are zeros here: timing only).
// The Q-loss backward is also stamped in the form that makes its own n-step return (n = 4, the headline step's launch) and
// in that form LOADING the critics' forward (no stamps 20..24: the recompute is not in that instantiation; the row between
// stamps 1 and 2 is the return's scan).  The forward is stamped again with the stored pair's
// extra job, without and with the critic-forward rider's workgroups beside the chain (workgroup 0 is a chain workgroup).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -Iadvanced-soft-actor-critic_amd/csrc \
//         tools/mlp_phases.hip -o tools/mlp_phases
#define ASAC_MLP_STAMPS 1
#include "../advanced-soft-actor-critic_amd/csrc/mlp.hip"

#include <cstdio>
#include <vector>

namespace asac {
int g_launch_repeat = 1;
void set_error(hipError_t e, const char* where) { printf("error %s at %s\n", hipGetErrorString(e), where); }
}  // namespace asac

static asac_mlp_desc_t stock(int in0, int in1, int heads0, int heads1, int transform) {
    asac_mlp_desc_t d{};
    d.in0 = in0; d.in1 = in1; d.n_blocks = 3;
    int off = 0, K = in0 + in1;
    for (int l = 0; l < 3; ++l) {
        d.width[l] = 64; d.residual[l] = l > 0;
        d.w_off[l] = off; off += 64 * K;
        d.b_off[l] = off; off += 64;
        K = 64;
    }
    d.head_cols[0] = heads0; d.head_cols[1] = heads1;
    d.head_w_off[0] = off; off += heads0 * 64;
    d.head_b_off[0] = off; off += heads0;
    if (heads1) { d.head_w_off[1] = off; off += heads1 * 64; d.head_b_off[1] = off; off += heads1; }
    d.head_transform = transform;
    return d;
}

int main() {
    const int N = 256, E = 2, A = 2, S = 6;
    const int64_t stride = 9216;
    std::vector<float> h(E * stride);
    for (size_t i = 0; i < h.size(); ++i) h[i] = 0.05f * (float)((int)(i * 2654435761u >> 20) % 21 - 10) / 10.f;
    float *params, *x0, *x1, *tq, *y, *ws, *grad, *loss, *eps, *ga, *la, *g1, *qt;
    hipMalloc(&params, h.size() * 4); hipMemcpy(params, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    hipMalloc(&x0, N * 8 * 4); hipMalloc(&x1, N * A * 4); hipMalloc(&tq, E * N * 4); hipMalloc(&y, N * 4);
    hipMalloc(&eps, N * A * 4); hipMalloc(&ga, E * N * A * 4); hipMalloc(&la, 4); hipMalloc(&g1, E * N * A * 4); hipMalloc(&qt, E * N * 4);
    hipMemset(x0, 0, N * 8 * 4); hipMemset(x1, 0, N * A * 4); hipMemset(tq, 0, E * N * 4); hipMemset(y, 0, N * 4);
    hipMemset(eps, 0, N * A * 4); hipMemset(ga, 0, E * N * A * 4); hipMemset(la, 0, 4); hipMemset(qt, 0, E * N * 4);
    const int64_t wsn = asac_mlp_backward_workspace(stride, E, N);
    hipMalloc(&ws, wsn * 4); hipMalloc(&grad, E * stride * 4); hipMalloc(&loss, E * 4);
    const asac_mlp_desc_t dq = stock(S, A, 1, 0, 0), dp = stock(S, 0, A, A, 1);
    asac_mlp_job_t jq{}, jp{};          // the critics on (x0 | x1), the policy on x0
    jq.desc = &dq, jq.params = params, jq.member_stride = stride, jq.E = E, jq.N = N;
    jq.x0 = x0, jq.x0_row_stride = S, jq.x1 = x1, jq.x1_row_stride = A;
    jp = jq, jp.desc = &dp, jp.E = 1, jp.x1 = nullptr, jp.x1_row_stride = 0;
    // the return target of the two `_return` modes: n = 4 steps, no importance ratios (zeros: timing only)
    const int n_ret = 4;
    float *rq, *rlogp, *rrew, *rratio;
    uint8_t* rmask;
    hipMalloc(&rq, E * N * (n_ret + 1) * 4); hipMemset(rq, 0, E * N * (n_ret + 1) * 4);
    hipMalloc(&rlogp, N * (n_ret + 1) * 4); hipMemset(rlogp, 0, N * (n_ret + 1) * 4);
    hipMalloc(&rrew, N * n_ret * 4); hipMemset(rrew, 0, N * n_ret * 4);
    hipMalloc(&rratio, n_ret * 4); hipMemset(rratio, 0, n_ret * 4);
    hipMalloc(&rmask, N * n_ret); hipMemset(rmask, 0, N * n_ret);
    asac_vtrace_args_t ret{};
    ret.q = rq, ret.q_stride_e = (int64_t)N * (n_ret + 1), ret.q_stride_b = n_ret + 1, ret.q_stride_t = 1, ret.E_sample = E;
    ret.logp = rlogp, ret.log_alpha = la, ret.reward = rrew, ret.reward_stride = n_ret;
    ret.done = rmask, ret.last_mask = rmask, ret.padding_mask = rmask, ret.mask_stride = n_ret;
    ret.gamma_ratio = rratio, ret.lambda_ratio = rratio, ret.gamma = 0.99f, ret.v_rho = 1.f, ret.v_c = 1.f;
    ret.B = N, ret.n = n_ret, ret.y_out = y;
    float* csaved = nullptr;
    hipMalloc(&csaved, asac_critic_forward_save_floats(N, E) * 4); hipMemset(csaved, 0, asac_critic_forward_save_floats(N, E) * 4);
    for (int mode = 0; mode < 5; ++mode) {
        double acc[24] = {0};
        const int reps = 200;
        int bad = 0;
        for (int r = 0; r < reps; ++r) {
            if (mode == 0)
                asac_mlp_backward_qloss(&jq, tq, y, nullptr, 0.2f, loss, nullptr, grad, ws, ASAC_MLP_REDUCE_DEFER, nullptr);
            else if (mode == 1)
                asac_mlp_backward_policy_q(&jq, qt, nullptr, E, g1, nullptr);
            else if (mode == 3)
                bad |= asac_mlp_backward_qloss_return(&jq, tq, &ret, nullptr, 0.2f, loss, nullptr, grad, ws, ASAC_MLP_REDUCE_DEFER, nullptr);
            else if (mode == 4)
                bad |= asac_mlp_backward_qloss_return_loaded(&jq, tq, &ret, nullptr, 0.2f, loss, grad, ws, ASAC_MLP_REDUCE_DEFER, csaved, nullptr);
            else
                asac_mlp_backward_policy_sample(&jp, eps, ga, E, la, grad, ws, ASAC_MLP_REDUCE_DEFER, nullptr);
            hipDeviceSynchronize();
            unsigned long long st[32];
            hipMemcpyFromSymbol(st, HIP_SYMBOL(asac::g_mlp_stamps), sizeof st);
            static const int idx[] = {0, 1, 2, 3, 4, 6, 7, 8, 10};
            for (int i = 1; i < 9; ++i) acc[i] += (double)(st[idx[i]] - st[idx[i - 1]]) / 100.0;
            acc[0] += (double)(st[10] - st[0]) / 100.0;
            acc[10] += (double)(st[16] - st[4]) / 100.0;
            acc[11] += (double)(st[17] - st[16]) / 100.0;
            acc[12] += (double)(st[18] - st[17]) / 100.0;
            acc[13] += (double)(st[6] - st[18]) / 100.0;
            if (mode != 4)
                for (int i = 0; i < 4; ++i) acc[14 + i] += (double)(st[21 + i] - st[20 + i]) / 100.0;
        }
        static const char* names[] = {"", "staging", "recompute", "loss / head mode", "head grads + g", "reverse L3", "reverse L2",
                                      "reverse L1", "input grads / end"};
        printf("%s: workgroup (0,0) total %.2f us%s\n",
               mode == 0 ? "backward_qloss" : mode == 1 ? "backward_policy_q" : mode == 2 ? "backward_policy_sample"
               : mode == 3 ? "backward_qloss_return" : "backward_qloss_return_loaded", acc[0] / reps, bad ? "  [the launch was refused]" : "");
        for (int i = 1; i < 9; ++i)
            printf("   %-18s %6.2f us\n", mode == 4 && i == 2 ? "return scan" : names[i], acc[i] / reps);
        if (mode != 4)
        printf("   recompute layer 2 in detail: gemm %.2f, gelu %.2f, LDS write %.2f, barrier %.2f\n", acc[14] / reps, acc[15] / reps,
               acc[16] / reps, acc[17] / reps);
        if (mode != 1)
            printf("   reverse L3 in detail: delta tile + barriers %.2f, grad_weight %.2f, grad_bias %.2f, dX gemm %.2f\n",
                   acc[10] / reps, acc[11] / reps, acc[12] / reps, acc[13] / reps);
    }
    // ---- the one-launch policy step and the one-launch policy -> sample -> critics forward ----------------------------
    {
        float *act, *qout, *lsout, *aout, *lpout, *prob, *a2, *lp2, *eps5, *x5, *q5;
        const int T = 5, N5 = N * T;
        hipMalloc(&act, N * A * 4); hipMemset(act, 0, N * A * 4); hipMalloc(&qout, E * N * 4);
        hipMalloc(&x5, N5 * 8 * 4); hipMemset(x5, 0, N5 * 8 * 4); hipMalloc(&eps5, N5 * A * 4); hipMemset(eps5, 0, N5 * A * 4);
        hipMalloc(&lsout, N5 * 2 * A * 4); hipMalloc(&aout, N5 * A * 4); hipMalloc(&lpout, N5 * 4); hipMalloc(&prob, N5 * A * 4);
        hipMalloc(&a2, N * A * 4); hipMalloc(&lp2, N * 4); hipMalloc(&q5, E * N5 * 4);
        const int reps = 200;
        // (form 1: the action sampled inside the launch, as the headline step issues it — the policy's first run on the tile
        // and the sampling lie between stamps 0 and 1, with the staging)
        // (form 2: the action given and the policy's forward LOADED from the tile an earlier launch saved — no stamp 7: the
        // forward and the head product are not in that instantiation; the row between stamps 6 and 8 is the fragments' LDS reads)
        float* saved = nullptr;
        if (hipMalloc(&saved, asac_policy_forward_save_floats(N) * 4) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
        hipMemset(saved, 0, asac_policy_forward_save_floats(N) * 4);
        for (int form = 0; form < 3; ++form) {
        double acc[16] = {0};
        for (int r = 0; r < reps; ++r) {
            if (form == 2)
                asac_policy_step_fused_loaded(&dq, params, stride, &dp, params, stride, x0, S, N, act, eps, la, nullptr, saved, qout,
                                              grad, ws, ASAC_MLP_REDUCE_DEFER, nullptr);
            else
            asac_policy_step_fused(&dq, params, stride, &dp, params, stride, x0, S, N, form ? nullptr : act, eps, la, nullptr, qout,
                                   form ? a2 : nullptr, form ? lp2 : nullptr, form ? lsout : nullptr, grad, ws, ASAC_MLP_REDUCE_DEFER, nullptr);
            hipDeviceSynchronize();
            unsigned long long st[32];
            hipMemcpyFromSymbol(st, HIP_SYMBOL(asac::g_mlp_stamps), sizeof st);
            if (form == 2) st[7] = st[6];
            for (int i = 1; i <= 13; ++i) acc[i] += (double)(st[i] - st[i - 1]) / 100.0;
            acc[0] += (double)(st[13] - st[0]) / 100.0;
        }
        static const char* names[] = {"", "staging", "critics forward", "critic heads", "dq", "critics backward", "policy -> LDS",
                                      "policy forward", "policy head", "sampling backward", "head grads + g", "reverse L3",
                                      "reverse L2", "reverse L1"};
        printf("policy_step_fused%s: workgroup 0 total %.2f us\n",
               form == 2 ? " (policy forward loaded)" : form ? " (action sampled inside)" : "", acc[0] / reps);
        for (int i = 1; i <= 13; ++i) {
            if (form == 2 && i == 7) continue;       // (no forward in the loaded form)
            printf("   %-18s %6.2f us\n", i == 1 && form == 1 ? "staging + sampling" : form == 2 && i == 8 ? "fragment reads" : names[i], acc[i] / reps);
        }
        }
        hipFree(saved);
        asac_pi_q_job_t job{};
        job.pi.desc = &dp; job.pi.params = params; job.pi.member_stride = stride; job.pi.x0 = x5; job.pi.x0_row_stride = S;
        job.pi.N = N5; job.pi.out = lsout; job.pi.E = 1;
        job.q = job.pi; job.q.desc = &dq; job.q.E = E; job.q.out = q5;
        job.sample.eps = eps5; job.sample.a_tanh_out = aout; job.sample.logp_out = lpout; job.sample.rows = N5; job.sample.A = A;
        job.sample.T = T; job.sample.action = aout; job.sample.action_stride_b = T * A; job.sample.action_stride_t = A;
        job.sample.prob_out = prob; job.sample.prob_stride_b = T * A; job.sample.prob_stride_t = A;
        job.eps2 = eps; job.t2 = 0; job.a2_out = a2; job.logp2_out = lp2;
        // ... and the same launch with ring-addressed rows (k_pi_sample_q_ring): a full ring of one long episode, the
        // batch's ids spread over it (every window row valid: the addressing is what is timed, not the padding)
        const int C = 4096;
        std::vector<int64_t> h_ids(N);
        std::vector<int32_t> h_index(C);
        for (int i = 0; i < N; ++i) h_ids[i] = (int64_t)((i * 2654435761u) % (unsigned)(C - T)) + C;
        for (int i = 0; i < C; ++i) h_index[i] = i;
        int64_t* ids;
        int32_t* index_ring;
        float *obs_ring, *act_ring;
        hipMalloc(&ids, N * 8); hipMemcpy(ids, h_ids.data(), N * 8, hipMemcpyHostToDevice);
        hipMalloc(&index_ring, C * 4); hipMemcpy(index_ring, h_index.data(), C * 4, hipMemcpyHostToDevice);
        hipMalloc(&obs_ring, C * S * 4); hipMemset(obs_ring, 0, C * S * 4);
        hipMalloc(&act_ring, C * A * 4); hipMemset(act_ring, 0, C * A * 4);
        asac_pi_q_job_t rjob = job;
        rjob.ring.ids = ids; rjob.ring.index_ring = index_ring; rjob.ring.capacity = C; rjob.ring.prev_n = 0; rjob.ring.L = T;
        rjob.ring.j0 = 0; rjob.ring.x_j0 = -1;
        rjob.ring.x0.src = obs_ring; rjob.ring.x0.row_bytes = S * 4; rjob.ring.x0.pad_mode = ASAC_PAD_KEEP;
        rjob.ring.action.src = act_ring; rjob.ring.action.row_bytes = A * 4; rjob.ring.action.pad_mode = ASAC_PAD_WORD;
        // forms 2..5: with the target critics on the stored pair as extra job 0 (ring rows: read through the ring, window row
        // 0), without (2, 4) and with (3, 5) the critic-forward rider on 32 further workgroups
        float* xq;
        hipMalloc(&xq, E * N * 4);
        asac_mlp_job_t jx = jq;
        jx.out = xq;
        asac_pi_q_job_t rjob_x = rjob;
        rjob_x.ring.x_j0 = 0; rjob_x.ring.x_action_offset = 0;
        for (int form = 0; form < 6; ++form) {
            double acc2[10] = {0}, side[6] = {0};
            int bad = 0;
            const bool ringf = form == 1 || form >= 4;
            for (int r = 0; r < reps; ++r) {
                if (form < 2)
                    bad |= asac_policy_sample_q_forward(form ? &rjob : &job, nullptr, 0, nullptr, 0, nullptr);
                else if (form == 2 || form == 4)
                    bad |= asac_policy_sample_q_forward(ringf ? &rjob_x : &job, &jx, 1, nullptr, 0, nullptr);
                else
                    bad |= asac_policy_sample_q_forward_saving(ringf ? &rjob_x : &job, &jx, 1, nullptr, 0, &jq, csaved, nullptr);
                hipDeviceSynchronize();
                unsigned long long st[32];
                hipMemcpyFromSymbol(st, HIP_SYMBOL(asac::g_mlp_stamps), sizeof st);
                for (int i = 1; i <= 7; ++i) acc2[i] += (double)(st[i] - st[i - 1]) / 100.0;
                acc2[0] += (double)(st[7] - st[0]) / 100.0;
                acc2[8] += (double)(st[8] - st[5]) / 100.0;
                for (int i = 0; i < 6; ++i) side[i] += (double)((long long)(st[9 + i] - st[3])) / 100.0;
            }
            // (a single-tile workgroup: "sampling" is the action alone, "actions -> tile" is empty, and the critic's first
            // layer ends at the barrier that also waits for the side waves to retire)
            static const char* names2[] = {"", "staging", "policy forward", "policy head", "sampling", "actions -> tile",
                                           "critic forward", "critic head"};
            printf("policy_sample_q_forward%s%s: workgroup 0 total %.2f us%s\n", ringf ? " (ring rows)" : "",
                   form < 2 ? "" : (form & 1) ? " + stored pair + critic-forward rider" : " + stored pair", acc2[0] / reps,
                   bad ? "  [the launch was refused]" : "");
            for (int i = 1; i <= 7; ++i) printf("   %-18s %6.2f us\n", names2[i], acc2[i] / reps);
            printf("   critic forward, first layer up to its barrier: %.2f us\n", acc2[8] / reps);
            printf("   side waves after the head's barrier (log-probability | stored actions | second sample): terms by"
                   " %.2f | %.2f | %.2f us, sums and stores by %.2f | %.2f | %.2f us\n", side[0] / reps, side[1] / reps,
                   side[2] / reps, side[3] / reps, side[4] / reps, side[5] / reps);
        }
    }
    return 0;
}
