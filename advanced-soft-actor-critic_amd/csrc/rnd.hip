// Random network distillation with continuous actions on the stock stacks (reference sac_base.py: _train_rnd 1978-2025,
// rnd_sample_c_action 829-856 inside _choose_action): two launches; the stacks' device code is asac_rnd.h's.
//
//   asac_rnd_distill  a workgroup per tile of 16 (state | action) rows: the frozen target and the predictor over the tile, the
//                     masked squared error and the cotangents at both pre-activations of the predictor, all row-local; the
//                     workgroups' loss sums meet in workgroup order (asac_ordered_finish.h).  The weight and bias gradients are
//                     products over ALL rows: csrc/xty.hip's, on the dense buffers this launch leaves.
//   asac_rnd_pick     a workgroup per group of WHOLE batch entries (max(1, 64 / k) of them, <= 64 candidate rows = up to four
//                     tiles, run one after the other against the staged weights): the k squashed candidates of every entry,
//                     both stacks on [state | candidate], the squared distillation error per candidate summed in a fixed order
//                     through LDS, then one lane per entry takes the first maximum and scores the chosen action under the
//                     policy.  An entry is decided inside one workgroup: nothing is exchanged between workgroups.
// Both stage the two stacks side by side (in = 128: 101 KB of weights, one workgroup a CU; the headline in = 8: 45 KB).
// No float atomics: equal inputs give equal bits.
#include "asac_common.h"
#include "asac_ordered_finish.h"
#include "asac_rnd.h"
#include "asac_squash.h"

namespace asac {
namespace rnd {

struct DistillDev {
    const float *state, *action;
    int64_t s_sb, s_st, a_sb, a_st;
    const uint8_t* mask;
    int64_t m_sb, m_st;
    StackDev pred, targ;
    int32_t S, A, n, N, r1, r2;
    float *x_cat, *h1, *gz1, *gz2, *loss, *partial;
    unsigned int* counter;
};

__global__ __launch_bounds__(kThreads) void k_rnd_distill(const DistillDev v) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int in = v.S + v.A, inp = pad16(in), p1 = inp + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const StackLds sp = stack_carve(lds, in), st = stack_carve(lds + stack_floats(in), in);
    float* xt = lds + 2 * stack_floats(in);       // [16][p1]
    float* ht = xt + kTile * p1;                  // [16][68] hidden tile
    float* gt = ht + kTile * kPitch;              // [16][68] cotangent at z2
    stack_stage(v.targ, st, in);
    stack_stage(v.pred, sp, in);
    const int row0 = blockIdx.x * kTile;
    for (int i = tid; i < kTile * inp; i += kThreads) {
        const int r = i / inp, c = i - r * inp, row = row0 + r;
        float x = 0.f;
        if (row < v.N && c < in) {
            const int b = row / v.n, t = row - b * v.n;
            x = c < v.S ? v.state[b * v.s_sb + t * v.s_st + c] : v.action[b * v.a_sb + t * v.a_st + (c - v.S)];
            v.x_cat[(int64_t)row * in + c] = x;
        }
        xt[r * p1 + c] = x;
    }
    // this lane's row: padded rows (and the rows beyond N of the last tile) contribute nothing
    const int r = lane & 15, row = row0 + r, col = 16 * wave + 4 * (lane >> 4);
    bool dead = row >= v.N;
    if (!dead && v.mask) {
        const int b = row / v.n, t = row - b * v.n;
        dead = v.mask[b * v.m_sb + t * v.m_st] != 0;
    }
    __syncthreads();
    const StackOut T = stack_forward(st, xt, ht, in, v.r1 != 0, v.r2 != 0, wave, lane);
    const StackOut P = stack_forward(sp, xt, ht, in, v.r1 != 0, v.r2 != 0, wave, lane);
    const float scale = 2.f / (float)(v.N * kWidth);
    f32x4 g, gz2;
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float d = dead ? 0.f : P.p[i] - T.p[i];
        part += d * d;
        g[i] = d * scale;
        gz2[i] = g[i] * P.d2[i];
    }
    st4(gt + r * kPitch + col, gz2);
    if (row < v.N) {
        st4(v.h1 + (int64_t)row * kWidth + col, P.h1);
        st4(v.gz2 + (int64_t)row * kWidth + col, gz2);
    }
    __syncthreads();
    const f32x4 back = layer_backward(sp.w2, gt, wave, lane);
    f32x4 gz1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float gh = v.r2 ? g[i] + back[i] : back[i];
        gz1[i] = gh * P.d1[i];
    }
    if (row < v.N) st4(v.gz1 + (int64_t)row * kWidth + col, gz1);
    // the loss: lanes -> wave -> workgroup in a fixed order, the workgroups' sums by the last one to arrive
    const float total = block_sum_waves<kThreads>(part);
    if (tid == 0) finish_publish(v.partial + blockIdx.x, total);
    if (!finish_arrive(v.counter) || tid != 0) return;
    *v.loss = finish_sum_in_order(v.partial, 1, (int)gridDim.x) / (float)(v.N * kWidth);
    finish_reset(v.counter);
}

struct PickDev {
    const float *state, *loc, *scale, *eps;
    int64_t s_stride, ls;
    StackDev pred, targ;
    int32_t S, A, k, batch, r1, r2;
    float *action, *prob, *err;
    int32_t* index;
};

constexpr int kPickRows = 64;            // candidate rows of a workgroup

__global__ __launch_bounds__(kThreads) void k_rnd_pick(const PickDev v) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = v.S, A = v.A, k = v.k, in = S + A, inp = pad16(in), p1 = inp + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const StackLds sp = stack_carve(lds, in), st = stack_carve(lds + stack_floats(in), in);
    float* xt = lds + 2 * stack_floats(in);       // [16][p1]
    float* ht = xt + kTile * p1;                  // [16][68]
    float* cand = ht + kTile * kPitch;            // [64][A] the candidates' squashed actions
    float* errs = cand + kPickRows * A;           // [64]    their errors
    float* errp = errs + kPickRows;               // [16][16] a tile's partial errors: (row, wave * 4 + lane group)
    stack_stage(v.targ, st, in);
    stack_stage(v.pred, sp, in);
    const int per = max(1, kPickRows / k), e0 = blockIdx.x * per, ne = min(per, v.batch - e0), rows = ne * k;
    for (int i = tid; i < rows * A; i += kThreads) {
        const int lr = i / A, d = i - lr * A, le = lr / k;
        const int64_t e = e0 + le;
        cand[i] = squashed_action(v.loc[e * v.ls + d], v.scale[e * v.ls + d], v.eps[((int64_t)e0 * k + lr) * A + d]);
    }
    for (int tile = 0; tile * kTile < rows; ++tile) {
        __syncthreads();                            // the candidates (first tile); the previous tile's xt and errp are read
        for (int i = tid; i < kTile * inp; i += kThreads) {
            const int r = i / inp, c = i - r * inp, lr = tile * kTile + r;
            float x = 0.f;
            if (lr < rows && c < in) x = c < S ? v.state[(int64_t)(e0 + lr / k) * v.s_stride + c] : cand[lr * A + (c - S)];
            xt[r * p1 + c] = x;
        }
        __syncthreads();
        const StackOut T = stack_forward(st, xt, ht, in, v.r1 != 0, v.r2 != 0, wave, lane);
        const StackOut P = stack_forward(sp, xt, ht, in, v.r1 != 0, v.r2 != 0, wave, lane);
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = P.p[i] - T.p[i];
            part += d * d;
        }
        errp[(lane & 15) * 16 + wave * 4 + (lane >> 4)] = part;
        __syncthreads();
        if (tid < kTile && tile * kTile + tid < rows) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) s += errp[tid * 16 + q];
            errs[tile * kTile + tid] = s;
        }
    }
    __syncthreads();
    if (v.err)
        for (int lr = tid; lr < rows; lr += kThreads) v.err[(int64_t)e0 * k + lr] = errs[lr];
    if (tid >= ne) return;
    // torch.argmax over the entry's candidates: the first maximum, NaN the largest value
    int best = 0;
    float bv = errs[tid * k];
    for (int j = 1; j < k; ++j) {
        const float x = errs[tid * k + j];
        const bool take = x > bv || (x != x && bv == bv);
        bv = take ? x : bv;
        best = take ? j : best;
    }
    const int64_t e = e0 + tid;
    if (v.index) v.index[e] = best;
    const float* a = cand + (tid * k + best) * A;
    for (int d = 0; d < A; ++d) v.action[e * A + d] = a[d];
    // the chosen action's density under (loc, scale): asac_squash_prob's own row function
    const StoredProb one{a, 1, 0, 0, 0, v.prob + e * A, 0, 0, 0};
    stored_action_prob(v.loc + e * v.ls, v.scale + e * v.ls, one, 0, A);
}

static size_t distill_lds(int in) { return sizeof(float) * (2 * stack_floats(in) + kTile * (pad16(in) + 4) + 2 * kTile * kPitch); }
static size_t pick_lds(int in, int A) {
    return sizeof(float) * (2 * stack_floats(in) + kTile * (pad16(in) + 4) + kTile * kPitch + kPickRows * A + kPickRows + 256);
}

static bool stack_ok(const asac_rnd_stack_t* s) {
    return s && s->w1 && s->b1 && s->w2 && s->b2 && aligned16(s->w1) && aligned16(s->b1) && aligned16(s->w2) && aligned16(s->b2);
}
// the residual flags a stack of these widths can have: the first block adds its input only at in == 64
static bool desc_ok(const asac_rnd_desc_t* d, int k) {
    return d && asac_rnd_supported(d->S, d->A, k) && (d->residual[0] == 0 || (d->residual[0] == 1 && d->S + d->A == kWidth)) &&
           (d->residual[1] == 0 || d->residual[1] == 1);
}
static StackDev stack_dev(const asac_rnd_stack_t& s) { return StackDev{s.w1, s.b1, s.w2, s.b2}; }

}  // namespace rnd
}  // namespace asac

using namespace asac;
using namespace asac::rnd;

extern "C" {

int asac_rnd_supported(int S, int A, int k) {
    return S > 0 && A > 0 && A <= ASAC_MAX_ACTION && S + A <= ASAC_RND_MAX_IN && k > 0 && k <= ASAC_RND_MAX_SAMPLES;
}

int64_t asac_rnd_distill_workspace(int64_t n_rows) {
    if (n_rows <= 0 || n_rows > ASAC_RND_MAX_ROWS) return -1;
    return (n_rows + kTile - 1) / kTile + 1;      // workgroup sums + arrival counter
}

int asac_rnd_distill(const asac_rnd_desc_t* desc, const asac_rnd_stack_t* predictor, const asac_rnd_stack_t* target,
                     const float* state, int64_t state_stride_b, int64_t state_stride_t, const float* action,
                     int64_t action_stride_b, int64_t action_stride_t, const uint8_t* padding_mask, int64_t mask_stride_b,
                     int64_t mask_stride_t, int B, int n, float* x_cat, float* h1, float* gz1, float* gz2, float* loss_out,
                     float* workspace, void* stream) {
    if (!desc_ok(desc, 1) || !stack_ok(predictor) || !stack_ok(target) || B < 0 || n <= 0) return bad_arg("asac_rnd_distill");
    if (B == 0) return 0;
    const int64_t N = (int64_t)B * n;
    if (N > ASAC_RND_MAX_ROWS || !state || !action || !x_cat || !h1 || !gz1 || !gz2 || !loss_out || !workspace ||
        !aligned16(x_cat) || !aligned16(h1) || !aligned16(gz1) || !aligned16(gz2))
        return bad_arg("asac_rnd_distill: rows / buffers");
    static bool lds_done = false;
    if (set_lds_limit((const void*)k_rnd_distill, distill_lds(kMaxIn), lds_done, "asac_rnd_distill: hipFuncSetAttribute")) return 1;
    const int64_t blocks = asac_rnd_distill_workspace(N) - 1;
    DistillDev v{};
    v.state = state, v.action = action, v.s_sb = state_stride_b, v.s_st = state_stride_t, v.a_sb = action_stride_b,
    v.a_st = action_stride_t;
    v.mask = padding_mask, v.m_sb = mask_stride_b, v.m_st = mask_stride_t;
    v.pred = stack_dev(*predictor), v.targ = stack_dev(*target);
    v.S = desc->S, v.A = desc->A, v.n = n, v.N = (int)N, v.r1 = desc->residual[0], v.r2 = desc->residual[1];
    v.x_cat = x_cat, v.h1 = h1, v.gz1 = gz1, v.gz2 = gz2, v.loss = loss_out, v.partial = workspace;
    v.counter = reinterpret_cast<unsigned int*>(workspace + blocks);
    ASAC_LAUNCH(k_rnd_distill, dim3((unsigned)blocks), dim3(kThreads), distill_lds(desc->S + desc->A), as_stream(stream), v);
    return finish_launch("asac_rnd_distill");
}

int asac_rnd_pick(const asac_rnd_desc_t* desc, const asac_rnd_stack_t* predictor, const asac_rnd_stack_t* target,
                  const float* state, int64_t state_stride, const float* loc, const float* scale, int64_t ls_row_stride,
                  const float* eps, int k, int batch, float* action_out, float* prob_out, float* err_out, int32_t* index_out,
                  void* stream) {
    if (!desc_ok(desc, k) || !stack_ok(predictor) || !stack_ok(target) || batch < 0) return bad_arg("asac_rnd_pick");
    if (batch == 0) return 0;
    if (!state || !loc || !scale || !eps || !action_out || !prob_out || (int64_t)batch * k > ASAC_RND_MAX_ROWS)
        return bad_arg("asac_rnd_pick: rows / buffers");
    static bool lds_done = false;
    if (set_lds_limit((const void*)k_rnd_pick, pick_lds(kMaxIn, ASAC_MAX_ACTION), lds_done, "asac_rnd_pick: hipFuncSetAttribute"))
        return 1;
    PickDev v{};
    v.state = state, v.loc = loc, v.scale = scale, v.eps = eps, v.s_stride = state_stride, v.ls = ls_row_stride;
    v.pred = stack_dev(*predictor), v.targ = stack_dev(*target);
    v.S = desc->S, v.A = desc->A, v.k = k, v.batch = batch, v.r1 = desc->residual[0], v.r2 = desc->residual[1];
    v.action = action_out, v.prob = prob_out, v.err = err_out, v.index = index_out;
    const int per = kPickRows / k > 1 ? kPickRows / k : 1;
    ASAC_LAUNCH(k_rnd_pick, dim3((unsigned)((batch + per - 1) / per)), dim3(kThreads), pick_lds(desc->S + desc->A, desc->A),
                as_stream(stream), v);
    return finish_launch("asac_rnd_pick");
}

}  // extern "C"
