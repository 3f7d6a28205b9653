// Acting of a policy-based learner (reference sac_base.py: _choose_action 931-966, _random_action 858-880; operators.py
// squash_correction_prob 17-19): the policy's head outputs and the caller's draws -> (action, prob), ONE launch for
// discrete branches, continuous actions or both, sampled or deterministic, with or without action_noise.
//
//   asac_act_policy  one lane per row, workgroups of 64 rows, no exchange between them (acting batches are the number
//                    of agents: a launch-latency kernel).  A row reads its D logits, its 2A head values and its draws,
//                    and writes D + A actions and D + A probabilities.
// The branch softmax is asac_categorical.h's, the inverse CDF the one asac_drnd_pick uses, the squashed Gaussian and its
// density asac_squash.h's, the head bounding the one the fused policy forward applies: a value another launch of the library
// also forms has the same bits here.  Accurate expf / logf / tanhf / atanhf, -ffp-contract=off (the one fused multiply-add,
// in the noise level, is asked for by name: torch.linspace forms it that way).  No float atomics.
#include "asac_categorical.h"
#include "asac_common.h"
#include "asac_squash.h"

namespace asac {

constexpr int kActRows = 64;          // rows (= lanes) of a workgroup

// torch.linspace(lo, hi, B)[b] in float32 (ATen RangeFactories: the two halves count from their own end)
__device__ __forceinline__ float act_noise_level(float lo, float hi, int b, int B) {
    if (B == 1) return lo;
    const float step = (hi - lo) / (float)(B - 1);
    return b < B / 2 ? fmaf(step, (float)b, lo) : fmaf(-step, (float)(B - 1 - b), hi);
}

__global__ __launch_bounds__(kActRows) void k_act_policy(const asac_act_job_t by_value) {
    const ASAC_KARG asac_act_job_t& x = *static_cast<const ASAC_KARG asac_act_job_t*>(kernarg_base());
    const int b = blockIdx.x * kActRows + threadIdx.x;
    if (b >= x.B) return;
    const int K = x.branches.K, D = K ? x.branches.D : 0, A = x.A;
    const bool det = x.deterministic != 0, noisy = x.use_noise != 0;
    const float level = noisy ? act_noise_level(x.noise_lo, x.noise_hi, b, x.B) : 0.f;
    float* act = x.action_out + (int64_t)b * x.action_stride;
    float* prob = x.prob_out + (int64_t)b * x.prob_stride;

    if (K) {
        const float* z = x.logits + (int64_t)b * x.logits_stride;
        // u columns: [K sampling: !det] [gate, K index: noisy]
        const float* u = x.u ? x.u + (int64_t)b * x.u_stride : z;       // (z: a valid address where there are no uniforms)
        const int gate = det ? 0 : K;
        const bool random = noisy && u[gate] < level;
        int j0 = 0;
        for (int k = 0; k < K; ++k) {
            const int s = x.branches.size[k];
            const CatStats st = cat_stats(z + j0, s);
            int arg = 0, last = 0;
            float best = 0.f;
            for (int j = 0; j < s; ++j) {
                const float zj = z[j0 + j], pj = cat_prob(zj, st);
                prob[j0 + j] = pj;
                const bool take = j == 0 || zj > best;                  // the first maximum (sample_deter's argmax)
                best = take ? zj : best;
                arg = take ? j : arg;
                last = pj > 0.f ? j : last;
            }
            int pick = arg;
            if (!det) pick = min(inverse_cdf(prob + j0, s, u[k]), last);      // (this lane's own stores, read back)
            if (random) pick = min((int)floorf(u[gate + 1 + k] * (float)s), s - 1);
            for (int j = 0; j < s; ++j) act[j0 + j] = j == pick ? 1.f : 0.f;
            j0 += s;
        }
    }

    if (A) {
        const float* lrow = x.loc + (int64_t)b * x.ls_row_stride;
        const float* srow = x.scale + (int64_t)b * x.ls_row_stride;
        // eps columns: [A sampling: !det] [A noise: noisy]
        const float* e = x.eps ? x.eps + (int64_t)b * x.eps_stride : lrow;
        const float* en = e + (det ? 0 : A);
        const bool raw = x.head_raw != 0;
        float l[ASAC_ACT_MAX_CONT], sc[ASAC_ACT_MAX_CONT], xs[ASAC_ACT_MAX_CONT];
        float jac = 1.f;
#pragma unroll
        for (int d = 0; d < ASAC_ACT_MAX_CONT; ++d) {
            if (d < A) {
                const float lv = lrow[d], sv = srow[d];
                l[d] = raw ? gauss_head_value(true, lv) : lv;
                sc[d] = raw ? gauss_head_value(false, sv) : sv;
                float a = det ? tanhf(l[d]) : tanhf(l[d] + e[d] * sc[d]);
                if (noisy) a = tanhf(atanhf(a) + en[d] * level);
                act[D + d] = a;
                xs[d] = atanhf(fminf(fmaxf(a, -0.999f), 0.999f));
                jac *= squash_jac(xs[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < ASAC_ACT_MAX_CONT; ++d)
            if (d < A) prob[D + d] = expf(normal_log_prob(xs[d], l[d], sc[d])) / jac;
    }
}

static bool act_sizes_ok(const asac_branches_t* br, int A) {
    const bool disc = br && br->K != 0;
    if (disc && !cat_branches_ok(*br)) return false;
    if (A < 0 || A > ASAC_ACT_MAX_CONT) return false;
    return disc || A > 0;
}

}  // namespace asac

using namespace asac;

extern "C" {

int asac_act_sizes_ok(const asac_branches_t* branches, int A) { return act_sizes_ok(branches, A) ? 1 : 0; }

int asac_act_policy(const asac_act_job_t* job_host, void* stream) {
    if (!job_host) return bad_arg("asac_act_policy");
    const asac_act_job_t& x = *job_host;
    if (!act_sizes_ok(&x.branches, x.A) || !x.action_out || !x.prob_out || x.B < 0) return bad_arg("asac_act_policy");
    const bool disc = x.branches.K != 0, det = x.deterministic != 0, noisy = x.use_noise != 0;
    if (disc && !x.logits) return bad_arg("asac_act_policy: logits");
    if (x.A && (!x.loc || !x.scale)) return bad_arg("asac_act_policy: loc / scale");
    if ((!det || noisy) && ((disc && !x.u) || (x.A && !x.eps))) return bad_arg("asac_act_policy: draws");
    if (noisy && !(x.noise_lo >= 0.f && x.noise_lo <= x.noise_hi)) return bad_arg("asac_act_policy: noise");
    if (x.B == 0) return 0;
    ASAC_LAUNCH(k_act_policy, dim3((unsigned)((x.B + kActRows - 1) / kActRows)), dim3(kActRows), 0, as_stream(stream), x);
    return finish_launch("asac_act_policy");
}

}  // extern "C"
