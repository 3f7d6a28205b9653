// Random network distillation for a pure-discrete, policy-based learner (reference sac_base.py: _train_rnd 1997-2010,
// rnd_sample_d_action 793-826 and the probability at 957-961): ModelRND.d_dense_list is D = sum of the branch sizes independent
// stacks LinearLayers(S, 64, 2, None); a row's stored action is K concatenated one-hot vectors and SELECTS one member per
// branch.  Three launches; the stacks' device code is asac_rnd.h's (in = S, no action columns), the branch softmax is
// asac_categorical.h's.
//
//   asac_drnd_distill      a workgroup per tile of 16 rows.  It first finds, per (row, branch), the selected member (first
//                          non-zero element of the branch, its value the weight w) and flags the members any of its live rows
//                          selected; the others are skipped as a uniform branch.  Sweep 1 stages member m's target and
//                          predictor side by side and adds  d += w (P_m - T_m)  in the lane that holds (row, features) after
//                          every layer; sweep 2 stages the predictor again (the same bits: d sums over the branches, so the
//                          cotangent is known only after sweep 1) for h1, the GELU derivatives and the back-product through
//                          W2_m, and stores the compact records [N][K][64].  The loss meets in workgroup order.
//   asac_drnd_param_grads  grid (row chunk, member).  A workgroup walks its chunk 32 rows at a time, compacts the rows that
//                          selected its member (ballot prefix: ascending) and adds their outer products in that order; thread
//                          (feature f, quarter q) keeps 16 columns of dW2[f], every fourth column of dW1[f] and one bias sum
//                          in registers (fmaf chains over the rows).  One chunk: stored straight to the gradient views; more:
//                          published, and the member's last arriver adds the chunks in chunk order.  Every element of every
//                          member's four views is written (zeros where nobody selected it).
//   asac_drnd_pick         a workgroup per 16 batch entries: the entries ARE the rows of the tile (a member's output depends on
//                          the state alone), so both stacks of all D members run once per entry; ONE stack is staged at a
//                          time (the target's outputs wait in the lanes' registers) and the differences E_m = P_m - T_m are
//                          kept in LDS [D][16][64 + 1].  Candidate indices by the inverse CDF on the branch softmax, a
//                          candidate's error summed over f = 0..63 in that order by one lane, the first maximum by one lane
//                          per entry.  Nothing is exchanged between workgroups.
// No float atomics: equal inputs give equal bits.
#include "asac_categorical.h"
#include "asac_common.h"
#include "asac_ordered_finish.h"
#include "asac_rnd.h"

namespace asac {
namespace drnd {

using namespace asac::rnd;

constexpr int kMaxD = ASAC_DRND_MAX_MEMBERS, kMaxK = ASAC_DISCRETE_MAX_BRANCHES, kMaxCand = ASAC_RND_MAX_SAMPLES;
constexpr int kEPitch = kWidth + 1;      // floats between rows of the kept differences: lanes of different (member, entry) on different banks

__device__ __forceinline__ StackDev stack_dev(const asac_rnd_stack_t& s) { return StackDev{s.w1, s.b1, s.w2, s.b2}; }

// branch of member m and the first member of that branch
__device__ __forceinline__ void branch_of(const asac_branches_t& br, int m, int& j, int& first) {
    j = 0, first = 0;
    for (int b = 0; b < br.K; ++b) {
        if (m >= first + br.size[b]) first += br.size[b], j = b + 1;
        else break;
    }
}

struct DistillDev {
    const float *state, *action;
    int64_t s_sb, s_st, a_sb, a_st;
    const uint8_t* mask;
    int64_t m_sb, m_st;
    const asac_rnd_stack_t *pred, *targ;
    asac_branches_t br;
    int32_t S, n, N, r1, r2;
    int32_t* sel;
    float *x, *h1, *gz1, *gz2, *loss, *partial;
    unsigned int* counter;
};

__global__ __launch_bounds__(kThreads) void k_drnd_distill(const DistillDev v) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_sel[kTile * kMaxK];
    __shared__ float s_w[kTile * kMaxK];
    __shared__ int s_used[kMaxD];
    const int S = v.S, inp = pad16(S), p1 = inp + 4, K = v.br.K, D = v.br.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const StackLds sp = stack_carve(lds, S), st = stack_carve(lds + stack_floats(S), S);
    float* xt = lds + 2 * stack_floats(S);        // [16][p1]
    float* ht = xt + kTile * p1;                  // [16][68] hidden tile
    float* gt = ht + kTile * kPitch;              // [16][68] cotangent at z2
    const int row0 = blockIdx.x * kTile;
    if (tid < kMaxD) s_used[tid] = 0;
    for (int i = tid; i < kTile * inp; i += kThreads) {
        const int r = i / inp, c = i - r * inp, row = row0 + r;
        float x = 0.f;
        if (row < v.N && c < S) {
            const int b = row / v.n, t = row - b * v.n;
            x = v.state[b * v.s_sb + t * v.s_st + c];
            v.x[(int64_t)row * S + c] = x;
        }
        xt[r * p1 + c] = x;
    }
    __syncthreads();
    // the selection: one thread per (row, branch); padded rows and the rows beyond N select nothing
    if (tid < kTile * K) {
        const int r = tid / K, j = tid - r * K, row = row0 + r;
        int m = -1;
        float w = 0.f;
        if (row < v.N) {
            const int b = row / v.n, t = row - b * v.n;
            const bool dead = v.mask && v.mask[b * v.m_sb + t * v.m_st] != 0;
            if (!dead) {
                int first = 0;
                for (int q = 0; q < j; ++q) first += v.br.size[q];
                const float* a = v.action + b * v.a_sb + t * v.a_st + first;
                for (int i = 0; i < v.br.size[j]; ++i) {
                    const float ai = a[i];
                    if (ai != 0.f) {
                        m = first + i, w = ai;
                        break;
                    }
                }
            }
            v.sel[(int64_t)row * K + j] = m;
        }
        s_sel[r * K + j] = m, s_w[r * K + j] = w;
        if (m >= 0) s_used[m] = 1;
    }
    __syncthreads();
    // the records of the pairs that selected nothing: zeros
    for (int i = tid; i < kTile * K * (kWidth / 4); i += kThreads) {
        const int pair = i / (kWidth / 4), c = (i - pair * (kWidth / 4)) * 4, row = row0 + pair / K;
        if (row < v.N && s_sel[pair] < 0) {
            const int64_t o = ((int64_t)row0 * K + pair) * kWidth + c;
            st4(v.h1 + o, zero4()), st4(v.gz1 + o, zero4()), st4(v.gz2 + o, zero4());
        }
    }
    const int r = lane & 15, row = row0 + r, col = 16 * wave + 4 * (lane >> 4);
    f32x4 d = zero4();
    // sweep 1: d = sum over the row's branches of w (P_m - T_m)
    for (int m = 0; m < D; ++m) {
        if (!s_used[m]) continue;
        int j, first;
        branch_of(v.br, m, j, first);
        __syncthreads();                              // every wave is done with the stacks staged before
        stack_stage(stack_dev(v.targ[m]), st, S);
        stack_stage(stack_dev(v.pred[m]), sp, S);
        __syncthreads();
        const StackOut T = stack_forward(st, xt, ht, S, v.r1 != 0, v.r2 != 0, wave, lane);
        const StackOut P = stack_forward(sp, xt, ht, S, v.r1 != 0, v.r2 != 0, wave, lane);
        if (s_sel[r * K + j] == m) {
            const float w = s_w[r * K + j];
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] += w * (P.p[i] - T.p[i]);
        }
    }
    const float scale = 2.f / (float)(v.N * kWidth);
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) part += d[i] * d[i];
    // sweep 2: the predictor again, the cotangents at its two pre-activations
    for (int m = 0; m < D; ++m) {
        if (!s_used[m]) continue;
        int j, first;
        branch_of(v.br, m, j, first);
        __syncthreads();
        stack_stage(stack_dev(v.pred[m]), sp, S);
        __syncthreads();
        const StackOut P = stack_forward(sp, xt, ht, S, v.r1 != 0, v.r2 != 0, wave, lane);
        const bool has = s_sel[r * K + j] == m;
        const float w = s_w[r * K + j];
        f32x4 g, gz2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            g[i] = has ? (d[i] * scale) * w : 0.f;
            gz2[i] = has ? g[i] * P.d2[i] : 0.f;
        }
        st4(gt + r * kPitch + col, gz2);
        __syncthreads();
        const f32x4 back = layer_backward(sp.w2, gt, wave, lane);
        if (has && row < v.N) {
            f32x4 gz1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float gh = v.r2 ? g[i] + back[i] : back[i];
                gz1[i] = gh * P.d1[i];
            }
            const int64_t o = ((int64_t)row * K + j) * kWidth + col;
            st4(v.h1 + o, P.h1), st4(v.gz2 + o, gz2), st4(v.gz1 + o, gz1);
        }
    }
    __syncthreads();
    // the loss: lanes -> wave -> workgroup in a fixed order, the workgroups' sums by the last one to arrive
    const float total = block_sum_waves<kThreads>(part);
    if (tid == 0) finish_publish(v.partial + blockIdx.x, total);
    if (!finish_arrive(v.counter) || tid != 0) return;
    *v.loss = finish_sum_in_order(v.partial, 1, (int)gridDim.x) / (float)(v.N * kWidth);
    finish_reset(v.counter);
}

// ---------------------------------------------------------------------------------------------------------------------
struct GradDev {
    const int32_t* sel;
    const float *x, *h1, *gz1, *gz2;
    const asac_rnd_grads_t* grads;
    asac_branches_t br;
    int32_t S, N, chunk_rows;
    float* partial;                 // [chunks][D][P], P = 64 * 64 + 64 * S + 128
    unsigned int* counter;          // [D]
};

constexpr int kGradRows = 32;       // rows examined per pass (one ballot of wave 0); the pass's four tiles are 40 KB of LDS

__global__ __launch_bounds__(kThreads) void k_drnd_param_grads(const GradDev v) {
    __shared__ __attribute__((aligned(16))) float s_g2[kGradRows * kWidth], s_g1[kGradRows * kWidth], s_h[kGradRows * kWidth];
    __shared__ __attribute__((aligned(16))) float s_x[kGradRows * kMaxIn];
    __shared__ int s_rows[kGradRows];
    __shared__ int s_count;
    const int S = v.S, K = v.br.K, D = v.br.D, m = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const int tid = threadIdx.x, f = tid >> 2, q = tid & 3;
    int j, first;
    branch_of(v.br, m, j, first);
    float a2[16], a1[32], ab = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) a2[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) a1[i] = 0.f;
    const int r_begin = chunk * v.chunk_rows, r_end = min(v.N, r_begin + v.chunk_rows);
    for (int r0 = r_begin; r0 < r_end; r0 += kGradRows) {
        __syncthreads();                              // the previous pass's tiles are read
        if (tid < 64) {
            const int row = r0 + tid;
            const bool hit = tid < kGradRows && row < r_end && v.sel[(int64_t)row * K + j] == m;
            const unsigned long long bal = __ballot(hit);
            if (hit) s_rows[__popcll(bal & ((1ull << tid) - 1ull))] = row;
            if (tid == 0) s_count = __popcll(bal);
        }
        __syncthreads();
        const int cnt = s_count;
        if (cnt == 0) continue;
        for (int i = tid; i < cnt * (kWidth / 4); i += kThreads) {
            const int lr = i >> 4, c = (i & 15) * 4;
            const int64_t o = ((int64_t)s_rows[lr] * K + j) * kWidth + c;
            st4(s_g2 + lr * kWidth + c, ld4(v.gz2 + o));
            st4(s_g1 + lr * kWidth + c, ld4(v.gz1 + o));
            st4(s_h + lr * kWidth + c, ld4(v.h1 + o));
        }
        for (int i = tid; i < cnt * S; i += kThreads) {
            const int lr = i / S, c = i - lr * S;
            s_x[lr * kMaxIn + c] = v.x[(int64_t)s_rows[lr] * S + c];
        }
        __syncthreads();
        for (int lr = 0; lr < cnt; ++lr) {
            const float g2 = s_g2[lr * kWidth + f], g1 = s_g1[lr * kWidth + f];
            const float* hp = s_h + lr * kWidth + 16 * q;
            const float* xp = s_x + lr * kMaxIn + q;
#pragma unroll
            for (int i = 0; i < 16; ++i) a2[i] = __builtin_fmaf(g2, hp[i], a2[i]);
#pragma unroll
            for (int i = 0; i < 32; ++i)
                if (q + 4 * i < S) a1[i] = __builtin_fmaf(g1, xp[4 * i], a1[i]);
            ab += q == 0 ? g2 : (q == 1 ? g1 : 0.f);
        }
    }
    // this thread's elements: dW2[f][16 q + i], dW1[f][q + 4 i], db2[f] (q == 0), db1[f] (q == 1)
    const asac_rnd_grads_t gr = v.grads[m];
    if (nchunks == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) gr.w2[f * kWidth + 16 * q + i] = a2[i];
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if (q + 4 * i < S) gr.w1[f * S + q + 4 * i] = a1[i];
        if (q == 0) gr.b2[f] = ab;
        if (q == 1) gr.b1[f] = ab;
        return;
    }
    const int64_t P = kWidth * kWidth + kWidth * S + 2 * kWidth;
    float* mine = v.partial + ((int64_t)chunk * D + m) * P;
#pragma unroll
    for (int i = 0; i < 16; ++i) finish_publish(mine + f * kWidth + 16 * q + i, a2[i]);
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (q + 4 * i < S) finish_publish(mine + kWidth * kWidth + f * S + q + 4 * i, a1[i]);
    if (q < 2) finish_publish(mine + kWidth * kWidth + kWidth * S + (q == 0 ? 0 : kWidth) + f, ab);
    if (!finish_arrive(v.counter + m)) return;        // (the member's chunks are the grid's x extent)
    float* base = v.partial + (int64_t)m * P;
    const int64_t stride = (int64_t)D * P;
    for (int i = tid; i < kWidth * kWidth; i += kThreads) gr.w2[i] = finish_sum_in_order(base + i, stride, nchunks);
    for (int i = tid; i < kWidth * S; i += kThreads) gr.w1[i] = finish_sum_in_order(base + kWidth * kWidth + i, stride, nchunks);
    if (tid < kWidth) gr.b2[tid] = finish_sum_in_order(base + kWidth * kWidth + kWidth * S + tid, stride, nchunks);
    else if (tid < 2 * kWidth) gr.b1[tid - kWidth] = finish_sum_in_order(base + kWidth * kWidth + kWidth * S + tid, stride, nchunks);
    if (tid == 0) finish_reset(v.counter + m);
}

// ---------------------------------------------------------------------------------------------------------------------
struct PickDev {
    const float *state, *logits, *u;
    int64_t s_stride, l_stride;
    const asac_rnd_stack_t *pred, *targ;
    asac_branches_t br;
    int32_t S, k, batch, r1, r2;
    float *action, *prob, *err;
    int32_t *cand, *index;
};

__global__ __launch_bounds__(kThreads) void k_drnd_pick(const PickDev v) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float s_p[kTile * kMaxD];               // the branch softmax of the tile's entries
    __shared__ float s_err[kTile * kMaxCand];
    __shared__ unsigned char s_idx[kTile * kMaxCand * kMaxK];
    const int S = v.S, inp = pad16(S), p1 = inp + 4, K = v.br.K, D = v.br.D, k = v.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const StackLds sl = stack_carve(lds, S);
    float* xt = lds + stack_floats(S);            // [16][p1]
    float* ht = xt + kTile * p1;                  // [16][68]
    float* ed = ht + kTile * kPitch;              // [D][16][65] the members' differences
    const int e0 = blockIdx.x * kTile, ne = min(kTile, v.batch - e0);
    for (int i = tid; i < kTile * inp; i += kThreads) {
        const int r = i / inp, c = i - r * inp;
        xt[r * p1 + c] = (r < ne && c < S) ? v.state[(int64_t)(e0 + r) * v.s_stride + c] : 0.f;
    }
    // the branch softmax: one thread per (entry, branch), the bits of cat_prob
    if (tid < kTile * K) {
        const int r = tid / K, j = tid - r * K;
        if (r < ne) {
            int first = 0;
            for (int b = 0; b < j; ++b) first += v.br.size[b];
            const float* z = v.logits + (int64_t)(e0 + r) * v.l_stride + first;
            const int s = v.br.size[j];
            const CatStats cs = cat_stats(z, s);
            for (int i = 0; i < s; ++i) {
                const float p = cat_prob(z[i], cs);
                s_p[r * kMaxD + first + i] = p;
                v.prob[(int64_t)(e0 + r) * D + first + i] = p;
            }
        }
    }
    const int r = lane & 15, col = 16 * wave + 4 * (lane >> 4);
    for (int m = 0; m < D; ++m) {
        __syncthreads();                              // xt (first member); every wave is done with the stack staged before
        stack_stage(stack_dev(v.targ[m]), sl, S);
        __syncthreads();
        const StackOut T = stack_forward(sl, xt, ht, S, v.r1 != 0, v.r2 != 0, wave, lane);
        __syncthreads();
        stack_stage(stack_dev(v.pred[m]), sl, S);
        __syncthreads();
        const StackOut P = stack_forward(sl, xt, ht, S, v.r1 != 0, v.r2 != 0, wave, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) ed[(m * kTile + r) * kEPitch + col + i] = P.p[i] - T.p[i];
    }
    __syncthreads();
    // one lane per (entry, candidate): its index per branch, then its error over the 64 features in index order
    for (int pc = tid; pc < ne * k; pc += kThreads) {
        const int le = pc / k, c = pc - le * k;
        const float* u = v.u + ((int64_t)(e0 + le) * k + c) * K;
        const float* ep[kMaxK];
        int first = 0;
#pragma unroll
        for (int j = 0; j < kMaxK; ++j) {
            int idx = 0;
            if (j < K) {
                idx = inverse_cdf(s_p + le * kMaxD + first, v.br.size[j], u[j]);
                s_idx[(le * kMaxCand + c) * kMaxK + j] = (unsigned char)idx;
                if (v.cand) v.cand[((int64_t)(e0 + le) * k + c) * K + j] = idx;
            }
            ep[j] = ed + ((first + idx) * kTile + le) * kEPitch;
            if (j < K) first += v.br.size[j];
        }
        float err = 0.f;
        for (int f = 0; f < kWidth; ++f) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < kMaxK; ++j)
                if (j < K) s += ep[j][f];
            err += s * s;
        }
        s_err[le * kMaxCand + c] = err;
        if (v.err) v.err[(int64_t)(e0 + le) * k + c] = err;
    }
    __syncthreads();
    if (tid >= ne) return;
    // torch.argmax over the entry's candidates: the first maximum, NaN the largest value
    int best = 0;
    float bv = s_err[tid * kMaxCand];
    for (int c = 1; c < k; ++c) {
        const float x = s_err[tid * kMaxCand + c];
        const bool take = x > bv || (x != x && bv == bv);
        bv = take ? x : bv;
        best = take ? c : best;
    }
    const int64_t e = e0 + tid;
    if (v.index) v.index[e] = best;
    int first = 0;
    for (int j = 0; j < K; ++j) {
        const int idx = s_idx[(tid * kMaxCand + best) * kMaxK + j];
        for (int i = 0; i < v.br.size[j]; ++i) v.action[e * D + first + i] = i == idx ? 1.f : 0.f;
        first += v.br.size[j];
    }
}

static size_t distill_lds(int S) { return sizeof(float) * (2 * stack_floats(S) + kTile * (pad16(S) + 4) + 2 * kTile * kPitch); }
static size_t pick_lds(int S, int D) {
    return sizeof(float) * (stack_floats(S) + kTile * (pad16(S) + 4) + kTile * kPitch + D * kTile * kEPitch);
}

// the member tables are DEVICE memory: the host checks what it can see (the table pointers and the sizes); the learner's
// binding checks every member's four pointers when it builds the table (native.drnd_table)
static bool shape_ok(const asac_branches_t* br, int S, const int32_t* residual, int k) {
    return br && residual && cat_branches_ok(*br) && asac_drnd_supported(S, br->D, br->K, k) &&
           (residual[0] == 0 || (residual[0] == 1 && S == kWidth)) && (residual[1] == 0 || residual[1] == 1);
}

static int chunk_rows_of(int64_t N) {
    int64_t c = (N + 63) / 64;                   // at most 64 chunks
    c = (c + kGradRows - 1) / kGradRows * kGradRows;
    return (int)(c < 2 * kGradRows ? 2 * kGradRows : c);
}

}  // namespace drnd
}  // namespace asac

using namespace asac;
using namespace asac::drnd;

extern "C" {

int asac_drnd_supported(int S, int D, int K, int k) {
    return S > 0 && S <= ASAC_RND_MAX_IN && D > 0 && D <= ASAC_DRND_MAX_MEMBERS && K > 0 && K <= ASAC_DISCRETE_MAX_BRANCHES &&
           K <= D && k > 0 && k <= ASAC_RND_MAX_SAMPLES;
}

int64_t asac_drnd_distill_workspace(int64_t n_rows) {
    if (n_rows <= 0 || n_rows > ASAC_RND_MAX_ROWS) return -1;
    return (n_rows + kTile - 1) / kTile + 1;      // workgroup sums + arrival counter
}

int64_t asac_drnd_param_grads_workspace(int64_t n_rows, int S, int D) {
    if (n_rows <= 0 || n_rows > ASAC_RND_MAX_ROWS || S <= 0 || S > ASAC_RND_MAX_IN || D <= 0 || D > ASAC_DRND_MAX_MEMBERS) return -1;
    const int cr = chunk_rows_of(n_rows);
    const int64_t chunks = (n_rows + cr - 1) / cr, P = kWidth * kWidth + (int64_t)kWidth * S + 2 * kWidth;
    return (chunks > 1 ? chunks * D * P : 0) + ASAC_DRND_MAX_MEMBERS;      // partials + one arrival counter a member
}

int asac_drnd_distill(const asac_branches_t* branches, int S, const int32_t* residual, const asac_rnd_stack_t* predictors,
                      const asac_rnd_stack_t* targets, const float* state, int64_t state_stride_b, int64_t state_stride_t,
                      const float* action, int64_t action_stride_b, int64_t action_stride_t, const uint8_t* padding_mask,
                      int64_t mask_stride_b, int64_t mask_stride_t, int B, int n, int32_t* sel, float* x, float* h1, float* gz1,
                      float* gz2, float* loss_out, float* workspace, void* stream) {
    if (!shape_ok(branches, S, residual, 1) || !predictors || !targets || !aligned16(predictors) || !aligned16(targets) || B < 0 ||
        n <= 0)
        return bad_arg("asac_drnd_distill");
    if (B == 0) return 0;
    const int64_t N = (int64_t)B * n;
    if (N > ASAC_RND_MAX_ROWS || !state || !action || !sel || !x || !h1 || !gz1 || !gz2 || !loss_out || !workspace ||
        !aligned16(x) || !aligned16(h1) || !aligned16(gz1) || !aligned16(gz2))
        return bad_arg("asac_drnd_distill: rows / buffers");
    static bool lds_done = false;
    if (set_lds_limit((const void*)k_drnd_distill, distill_lds(kMaxIn), lds_done, "asac_drnd_distill: hipFuncSetAttribute")) return 1;
    const int64_t blocks = asac_drnd_distill_workspace(N) - 1;
    DistillDev v{};
    v.state = state, v.action = action, v.s_sb = state_stride_b, v.s_st = state_stride_t, v.a_sb = action_stride_b,
    v.a_st = action_stride_t;
    v.mask = padding_mask, v.m_sb = mask_stride_b, v.m_st = mask_stride_t;
    v.pred = predictors, v.targ = targets, v.br = *branches;
    v.S = S, v.n = n, v.N = (int)N, v.r1 = residual[0], v.r2 = residual[1];
    v.sel = sel, v.x = x, v.h1 = h1, v.gz1 = gz1, v.gz2 = gz2, v.loss = loss_out, v.partial = workspace;
    v.counter = reinterpret_cast<unsigned int*>(workspace + blocks);
    ASAC_LAUNCH(k_drnd_distill, dim3((unsigned)blocks), dim3(kThreads), distill_lds(S), as_stream(stream), v);
    return finish_launch("asac_drnd_distill");
}

int asac_drnd_param_grads(const asac_branches_t* branches, int S, const int32_t* sel, const float* x, const float* h1,
                          const float* gz1, const float* gz2, int64_t n_rows, const asac_rnd_grads_t* grads, float* workspace,
                          void* stream) {
    if (!branches || !cat_branches_ok(*branches) || !asac_drnd_supported(S, branches->D, branches->K, 1) || !grads ||
        !aligned16(grads) || n_rows < 0)
        return bad_arg("asac_drnd_param_grads");
    if (n_rows == 0) return 0;
    if (n_rows > ASAC_RND_MAX_ROWS || !sel || !x || !h1 || !gz1 || !gz2 || !workspace || !aligned16(x) || !aligned16(h1) ||
        !aligned16(gz1) || !aligned16(gz2))
        return bad_arg("asac_drnd_param_grads: rows / buffers");
    const int cr = chunk_rows_of(n_rows);
    const int64_t chunks = (n_rows + cr - 1) / cr;
    const int64_t words = asac_drnd_param_grads_workspace(n_rows, S, branches->D);
    GradDev v{};
    v.sel = sel, v.x = x, v.h1 = h1, v.gz1 = gz1, v.gz2 = gz2, v.grads = grads, v.br = *branches;
    v.S = S, v.N = (int)n_rows, v.chunk_rows = cr, v.partial = workspace;
    v.counter = reinterpret_cast<unsigned int*>(workspace + (words - ASAC_DRND_MAX_MEMBERS));
    ASAC_LAUNCH(k_drnd_param_grads, dim3((unsigned)chunks, (unsigned)branches->D), dim3(kThreads), 0, as_stream(stream), v);
    return finish_launch("asac_drnd_param_grads");
}

int asac_drnd_pick(const asac_branches_t* branches, int S, const int32_t* residual, const asac_rnd_stack_t* predictors,
                   const asac_rnd_stack_t* targets, const float* state, int64_t state_stride, const float* logits,
                   int64_t logits_stride, const float* u, int k, int batch, float* action_out, float* prob_out, float* err_out,
                   int32_t* cand_out, int32_t* index_out, void* stream) {
    if (!shape_ok(branches, S, residual, k) || !predictors || !targets || !aligned16(predictors) || !aligned16(targets) ||
        batch < 0)
        return bad_arg("asac_drnd_pick");
    if (batch == 0) return 0;
    if (!state || !logits || !u || !action_out || !prob_out || (int64_t)batch * k > ASAC_RND_MAX_ROWS)
        return bad_arg("asac_drnd_pick: rows / buffers");
    static bool lds_done = false;
    if (set_lds_limit((const void*)k_drnd_pick, pick_lds(kMaxIn, kMaxD), lds_done, "asac_drnd_pick: hipFuncSetAttribute")) return 1;
    PickDev v{};
    v.state = state, v.logits = logits, v.u = u, v.s_stride = state_stride, v.l_stride = logits_stride;
    v.pred = predictors, v.targ = targets, v.br = *branches;
    v.S = S, v.k = k, v.batch = batch, v.r1 = residual[0], v.r2 = residual[1];
    v.action = action_out, v.prob = prob_out, v.err = err_out, v.cand = cand_out, v.index = index_out;
    ASAC_LAUNCH(k_drnd_pick, dim3((unsigned)((batch + kTile - 1) / kTile)), dim3(kThreads), pick_lds(S, branches->D),
                as_stream(stream), v);
    return finish_launch("asac_drnd_pick");
}

}  // extern "C"
