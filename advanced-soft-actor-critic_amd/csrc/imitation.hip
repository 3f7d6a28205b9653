// Behaviour-cloning loss of ImitationBase (reference algorithm/imitation_base.py:57-59):
//   loss = mean(-Normal(loc, scale).log_prob(a) - entropy_coef * Normal(loc, scale).entropy())
// over the first t_valid rows of one padded episode, value and gradients from ONE launch.  With `raw_head` the inputs are
// the stock policy's raw head outputs (mean | logstd): the launch applies the head (reference nn_models/policy.py:169,
// loc = 5 tanh(m / 5), scale = exp(clamp(s, -20, 0.5))) itself and the gradients are with respect to the raw values.
//
// The sum has a fixed order: lane partial (elements in index order) -> wave (xor butterfly) -> workgroup (waves in order)
// -> the last workgroup to arrive adds the workgroups' sums in workgroup order (asac_ordered_finish.h).  The arrival
// counter is an integer; no float atomics, so two launches on the same input give the same bits.  -ffp-contract=off.
#include "asac_common.h"
#include "asac_ordered_finish.h"
#include "asac_squash.h"

namespace asac {

constexpr int kBcThreads = 256, kBcPerLane = 4, kBcMaxBlocks = ASAC_BC_MAX_BLOCKS;
constexpr float kNormalEntropyConst = 0.5f + kLogSqrt2Pi;      // 1/2 + 1/2 log(2 pi)

struct BcArgs {
    const float *loc, *scale;        // rows `ld_in` floats apart (the halves of one [Tp, 2A] buffer, or two [Tp, A])
    const float* action;             // rows `a_stride` floats apart, the continuous part starts at column a_off
    const int32_t* t_valid;          // device: rows [0, t_valid) count
    float *loss, *dloc, *dscale;     // gradient rows `ld_out` floats apart
    float* partial;                  // [kBcMaxBlocks] workgroup sums
    unsigned int* counter;           // arrivals: zero before the first launch, left zero by every launch
    int64_t ld_in, ld_out, a_stride;
    int32_t a_off, Tp, A, raw_head;
    float entropy_coef;
};

__global__ __launch_bounds__(kBcThreads) void k_bc_loss_grad(const BcArgs a) {
    const int tid = threadIdx.x;
    const int A = a.A, n = a.Tp * A;                      // (n < 2^31 checked by the host)
    int tv = *a.t_valid;
    tv = tv < 0 ? 0 : (tv > a.Tp ? a.Tp : tv);
    const float inv = tv > 0 ? 1.f / ((float)tv * (float)A) : 0.f;
    const int stride = gridDim.x * kBcThreads;

    float s = 0.f;
    for (int i0 = blockIdx.x * kBcThreads + tid; i0 < n; i0 += kBcPerLane * stride) {
        float lv[kBcPerLane], sv[kBcPerLane], av[kBcPerLane];
#pragma unroll
        for (int u = 0; u < kBcPerLane; ++u) {            // the loads of a lane's elements requested together
            const int i = min(i0 + u * stride, n - 1);
            const int row = i / A, d = i - row * A;
            lv[u] = a.loc[row * a.ld_in + d];
            sv[u] = a.scale[row * a.ld_in + d];
            av[u] = a.action[row * a.a_stride + a.a_off + d];
        }
#pragma unroll
        for (int u = 0; u < kBcPerLane; ++u) {
            const int i = i0 + u * stride;
            if (i >= n) continue;
            const int row = i / A, d = i - row * A;
            float gl = 0.f, gs = 0.f;
            if (row < tv) {
                float loc = lv[u], scale = sv[u], dl_dm = 1.f, ds_dr = 1.f;
                if (a.raw_head) {
                    const float t = tanhf(lv[u] / 5.f);
                    loc = t * 5.f;
                    dl_dm = 1.f - t * t;
                    const bool open = sv[u] >= -20.f && sv[u] <= 0.5f;
                    scale = expf(fminf(fmaxf(sv[u], -20.f), 0.5f));
                    ds_dr = open ? scale : 0.f;
                }
                const float z = (av[u] - loc) / scale;
                const float entropy = kNormalEntropyConst + logf(scale);
                s += -normal_log_prob(av[u], loc, scale) - a.entropy_coef * entropy;
                gl = (-z / scale) * inv * dl_dm;
                gs = ((1.f - a.entropy_coef - z * z) / scale) * inv * ds_dr;
            }
            a.dloc[row * a.ld_out + d] = gl;              // rows >= t_valid: exact zeros
            a.dscale[row * a.ld_out + d] = gs;
        }
    }
    s = block_sum_waves<kBcThreads>(s);
    if (tid == 0) finish_publish(a.partial + blockIdx.x, s);
    if (!finish_arrive(a.counter) || tid != 0) return;
    const float v = finish_sum_in_order(a.partial, 1, (int)gridDim.x);
    *a.loss = tv > 0 ? v / ((float)tv * (float)A) : 0.f;          // torch.mean: the sum over the count
    finish_reset(a.counter);
}

}  // namespace asac

using namespace asac;

extern "C" {

int64_t asac_bc_loss_grad_workspace(void) { return kBcMaxBlocks + 4; }     // workgroup sums + the arrival counter's block

int asac_bc_loss_grad(const float* loc, const float* scale, int64_t ld_in, const float* action, int64_t action_stride,
                      int action_offset, const int32_t* t_valid, int Tp, int A, float entropy_coef, int raw_head,
                      float* loss, float* dloc, float* dscale, int64_t ld_out, float* workspace, void* stream) {
    if (!loc || !scale || !action || !t_valid || !loss || !dloc || !dscale || !workspace || Tp <= 0 || A <= 0 ||
        (int64_t)Tp * A > ASAC_BC_MAX_ELEMENTS || ld_in < A || ld_out < A || action_offset < 0 ||
        action_stride < (int64_t)action_offset + A)
        return bad_arg("asac_bc_loss_grad");
    BcArgs a;
    a.loc = loc, a.scale = scale, a.action = action, a.t_valid = t_valid;
    a.loss = loss, a.dloc = dloc, a.dscale = dscale;
    a.partial = workspace, a.counter = reinterpret_cast<unsigned int*>(workspace + kBcMaxBlocks);
    a.ld_in = ld_in, a.ld_out = ld_out, a.a_stride = action_stride;
    a.a_off = action_offset, a.Tp = Tp, a.A = A, a.raw_head = raw_head ? 1 : 0;
    a.entropy_coef = entropy_coef;
    const int64_t n = (int64_t)Tp * A;
    const int64_t want = (n + kBcThreads * kBcPerLane - 1) / (kBcThreads * kBcPerLane);
    const unsigned blocks = (unsigned)(want < kBcMaxBlocks ? want : kBcMaxBlocks);
    ASAC_LAUNCH(k_bc_loss_grad, dim3(blocks), dim3(kBcThreads), 0, as_stream(stream), a);
    return finish_launch("asac_bc_loss_grad");
}

}  // extern "C"
