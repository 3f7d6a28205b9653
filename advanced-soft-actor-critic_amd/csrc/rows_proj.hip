// The Linear layers AROUND the multi-head attention core (csrc/attn_mh.hip), over the rows of a batch of sampled windows, on
// f32 MFMA — `MultiheadAttention.forward` (reference algorithm/nn_models/layers/seq_layers.py:239-333) at the widths of the
// reference's environments (`EpisodeMultiheadAttention(64, …)`: envs/gym/toy_queue/nn_attn.py:28-45):
//   * q / k / v projections of one input as ONE launch (three nn.Linear(E, E): three library GEMMs of 9 216 x 64 x 64, each
//     at the launch floor), the query projected for the last `tail` positions of a window only (the episode blocks' cut query);
//     backward: the input gradient of the three as one launch (three GEMMs and two accumulations);
//   * the output ResBlock  y = (x + gelu(x W^T + b)) * row_scale  (LinearLayers(E, E, depth 1) + the dead-row / padded-row
//     factor: a GEMM and three elementwise launches), backward to grad_x and the pre-activation gradient (whose products
//     over the rows — weight and bias gradients — are csrc/xty.hip's);
//   * with a rotary position encoding (ROPE / ROPE2: `self.rope(query_index, key_index, q, k)` behind the projections), the
//     rotation of q and k as the epilogue of the projection launch and the un-rotation of their gradients as the prologue of
//     its backward (arithmetic: asac_rope.h — the bits of csrc/rope.hip behind / in front of the plain launches).
//
// A workgroup (4 waves) owns 16 rows; wave w the output feature tiles w, w + 4, ...  The ROWS are the N dimension of the
// MFMA (B operand = 16 bytes of a row's features, as they lie in memory), the weights the A operand: forward a weight row's
// 16 bytes, backward four strided words of a weight column; the result tile holds four consecutive features of a row per
// lane -> 16-byte stores.  Everything is L2-resident (weights 16 KB a matrix); the launches are latency, not bandwidth.
#include "asac_common.h"
#include "asac_dropout.h"
#include "asac_gelu.h"
#include "asac_rope.h"

namespace asac {
namespace rowsp {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kMaxJobs = 3;

#define RP_MF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 mfma4(const f32x4 a, const f32x4 b, f32x4 c) {
    c = RP_MF(a[0], b[0], c);
    c = RP_MF(a[1], b[1], c);
    c = RP_MF(a[2], b[2], c);
    c = RP_MF(a[3], b[3], c);
    return c;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

struct ProjArgs {
    const float* x; int64_t xs_b, xs_t;      // input rows x[b][t][E] (feature stride 1)
    int32_t B, L, J;
    const float* w[kMaxJobs];                // [E][E] (nn.Linear layout: out x in)
    const float* b[kMaxJobs];                // [E]
    int32_t tail[kMaxJobs];                  // job j covers positions t >= L - tail[j]; its rows are dense [B][tail[j]][E]
    float* y[kMaxJobs];
    const float* g[kMaxJobs];                // backward: gradients of y
    float* gx;                               // [B][L][E] dense
    // rotary kinds: jobs 0 and 1 (q, k) are rotated by the table row of ONE index array [B][L] (the query's: its newest entries)
    rope::Tables tab;
    rope::Index ix;
    float* gu[2];                            // backward: the un-rotated gradients of jobs 0 and 1, dense like g
};

// The draws of the `nn.Dropout` modules inside the dense stacks (the contract of asac_dropout.h): element (row r, feature f)
// is word f & 3 of Philox block r * (E / 4) + (f >> 2) — the four features a lane holds in one f32x4 are one block — under
// a tag of its own in the second counter word: 6 / 7 / 8 the q / k / v stack (r = b * L + t, the position in the FULL window:
// a draw does not depend on `tail`), 9 the output block (r the flat row).  Each launch owns a state (counter and arrival
// words) of the layout of asac_dropout.h; the backward reads the counter its forward left in `used`.
constexpr uint32_t kTagQkv = 6u, kTagOut = 9u;

struct DrawArgs {
    uint64_t seed; uint32_t instance, thr; float scale; int32_t advance;
    int64_t* state;                          // forward: the launch site's draw state
    int64_t* used;                           // forward: <- the counter drawn with; backward: read
    __device__ __forceinline__ DropDraw draw() const { return DropDraw{seed, 0, instance, thr, scale}; }
};

__device__ __forceinline__ f32x4 row_factors4(const DropDraw& d, uint32_t tag, uint32_t block) {
    const Philox p = philox4x32_10(block, (tag << 28) | (d.instance & 0x0FFFFFFFu), (uint32_t)d.counter,
                                   (uint32_t)(d.counter >> 32), (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
    f32x4 f;
#pragma unroll
    for (int r = 0; r < 4; ++r) f[r] = p.c[r] >= d.thr ? d.scale : 0.f;
    return f;
}

// the forward's counter exchange, by lane 0 of the LAST wave (the one with the fewest feature tiles): the load is issued first
// thing, so that it is in flight over the work that stands between draw_begin and draw_share ...
__device__ __forceinline__ DropDraw draw_begin(const DrawArgs& d) {
    DropDraw draw = d.draw();
    if (threadIdx.x == kThreads - 64) draw.counter = (uint64_t)dropout_counter_load(d.state);
    return draw;
}
// ... the value reaches the other waves through LDS (a workgroup barrier), and the arrival's trips run beside their products
__device__ __forceinline__ void draw_share(const DrawArgs& d, DropDraw& draw) {
    __shared__ uint32_t s_ctr[2];
    if (threadIdx.x == kThreads - 64) s_ctr[0] = (uint32_t)draw.counter, s_ctr[1] = (uint32_t)(draw.counter >> 32);
    __syncthreads();
    draw.counter = ((uint64_t)s_ctr[1] << 32) | s_ctr[0];
    if (threadIdx.x == kThreads - 64) dropout_counter_arrive(d.state, d.used, (int64_t)draw.counter, d.advance != 0);
}

struct ResArgs {
    const float* x; int64_t xs;              // [rows][E], row stride xs
    const float* w; const float* b;
    const float* scale;                      // [rows] or NULL
    int64_t rows;
    float* y; float* pre;                    // [rows][E]
    const float* gy; float* gx; float* gpre;
    DrawArgs d;                              // DROP
};

// the <= 3 dense stacks of one input: ResBlock(E, E) -> nn.Dropout(p) -> nn.Linear(E, E) each
struct DenseArgs {
    const float* x; int64_t xs_b, xs_t;      // input rows x[b][t][E] (feature stride 1)
    int32_t B, L, J;
    const float* w1[kMaxJobs]; const float* b1[kMaxJobs];      // the ResBlock's Linear
    const float* w2[kMaxJobs]; const float* b2[kMaxJobs];      // the Linear behind the dropout
    int32_t tail[kMaxJobs];                  // job j covers positions t >= L - tail[j]; its rows are dense [B][tail[j]][E]
    float* y[kMaxJobs]; float* pre[kMaxJobs]; float* h[kMaxJobs];
    const float* g[kMaxJobs];                // backward: gradients of y
    float* gx;                               // [B][L][E] dense
    float* gpre[kMaxJobs];
    DrawArgs d;
};

// four strided words of a weight column block: W[n0 + s][k] for s < 4
template <int E>
__device__ __forceinline__ f32x4 wcol4(const float* w, int n0, int k) {
    f32x4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = w[(n0 + s) * E + k];
    return v;
}

// KIND 0: the projections.  KIND ROPE: the lane's four consecutive features are two of the encoding's pairs.  KIND ROPE2: a wave
// takes the n-tiles nt and nt + EC / 2 together, so feature j and its partner j + E / 2 are in the same lane.
template <int EC, int KIND>
__global__ void __launch_bounds__(kThreads) k_rows_proj_fwd(const ProjArgs a) {
    constexpr int E = 16 * EC;
    constexpr int NP = KIND == rope::kRope2 ? 2 : 1, NT = EC / NP;
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const int64_t rows = (int64_t)a.B * a.L, row = (int64_t)blockIdx.x * 16 + x;
    const bool live = row < rows;
    const int64_t rc = live ? row : rows - 1;
    const int b = (int)(rc / a.L), t = (int)(rc - (int64_t)b * a.L);
    const float* xp = a.x + b * a.xs_b + t * a.xs_t + 4 * q;
    f32x4 xv[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) xv[c] = live ? ld4(xp + 16 * c) : zero4();
    const int64_t tr = KIND ? rope::table_row(a.ix, b, t, a.tab.T) * E + 4 * q : 0;
    // one job per workgroup (blockIdx.y): the launch is a dependent chain per wave (rows -> weights -> products -> store), not
    // bandwidth — three times the waves, a third of the chain each (10 -> 6 us at 9 216 rows x 64)
    for (int nt = wv; nt < NT; nt += kWaves) {
#pragma unroll
        for (int j = 0; j < kMaxJobs; ++j) {
            if (j != (int)blockIdx.y) continue;
            f32x4 acc[NP];
#pragma unroll
            for (int h = 0; h < NP; ++h) {
                const int n = nt + h * NT;
                const float* wp = a.w[j] + (16 * n + x) * E + 4 * q;
                f32x4 wa[EC];
#pragma unroll
                for (int c = 0; c < EC; ++c) wa[c] = ld4(wp + 16 * c);
                const f32x4 bias = ld4(a.b[j] + 16 * n + 4 * q);
                acc[h] = zero4();
#pragma unroll
                for (int c = 0; c < EC; ++c) acc[h] = mfma4(wa[c], xv[c], acc[h]);      // acc[r] = y[row x][16 n + 4 q + r]
                acc[h] += bias;
            }
            if (KIND == rope::kRope && j < 2) {
                const f32x4 cs = ld4(a.tab.t0 + tr + 16 * nt), v = acc[0];      // (c, s) of the pairs 8 nt + 2 q, + 1
                float y0, y1, y2, y3;
                rope::pair_fwd(v[0], v[1], cs[0], cs[1], y0, y1);
                rope::pair_fwd(v[2], v[3], cs[2], cs[3], y2, y3);
                acc[0] = (f32x4){y0, y1, y2, y3};
            }
            if (KIND == rope::kRope2 && j < 2) {
                const f32x4 cl = ld4(a.tab.t0 + tr + 16 * nt), sl = ld4(a.tab.t1 + tr + 16 * nt);
                const f32x4 ch = ld4(a.tab.t0 + tr + 16 * nt + E / 2), sh = ld4(a.tab.t1 + tr + 16 * nt + E / 2);
                const f32x4 vl = acc[0], vh = acc[NP - 1];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float yl, yh;
                    rope::half_fwd(vl[r], vh[r], cl[r], sl[r], ch[r], sh[r], yl, yh);
                    acc[0][r] = yl, acc[NP - 1][r] = yh;
                }
            }
            const int skip = a.L - a.tail[j];
#pragma unroll
            for (int h = 0; h < NP; ++h)
                if (live && t >= skip) st4(a.y[j] + ((int64_t)b * a.tail[j] + (t - skip)) * E + 16 * (nt + h * NT) + 4 * q, acc[h]);
        }
    }
}

// gx[row][k] = sum_j sum_n g_j[row][n] W_j[n][k]   (jobs in order, features in order)
// (rotary KIND: the gradients of jobs 0 and 1 are un-rotated as they are loaded and written to gu, one wave per tile)
template <int EC, int KIND>
__global__ void __launch_bounds__(kThreads) k_rows_proj_bwd(const ProjArgs a) {
    constexpr int E = 16 * EC;
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const int64_t rows = (int64_t)a.B * a.L, row = (int64_t)blockIdx.x * 16 + x;
    const bool live = row < rows;
    const int64_t rc = live ? row : rows - 1;
    const int b = (int)(rc / a.L), t = (int)(rc - (int64_t)b * a.L);
    const int64_t tr = KIND ? rope::table_row(a.ix, b, t, a.tab.T) * E + 4 * q : 0;
    f32x4 gv[kMaxJobs][EC];
#pragma unroll
    for (int j = 0; j < kMaxJobs; ++j) {
        if (j >= a.J) continue;
        const int skip = a.L - a.tail[j];
        const bool on = live && t >= skip;
        const int64_t at = ((int64_t)b * a.tail[j] + (on ? t - skip : 0)) * E + 4 * q;
        const float* gp = a.g[j] + at;
#pragma unroll
        for (int c = 0; c < EC; ++c) gv[j][c] = on ? ld4(gp + 16 * c) : zero4();
        if (KIND && j < 2) {
            if (KIND == rope::kRope) {
#pragma unroll
                for (int c = 0; c < EC; ++c) {
                    const f32x4 cs = ld4(a.tab.t0 + tr + 16 * c), v = gv[j][c];
                    float y0, y1, y2, y3;
                    rope::pair_bwd(v[0], v[1], cs[0], cs[1], y0, y1);
                    rope::pair_bwd(v[2], v[3], cs[2], cs[3], y2, y3);
                    gv[j][c] = (f32x4){y0, y1, y2, y3};
                }
            } else {
#pragma unroll
                for (int c = 0; c < EC / 2; ++c) {
                    const f32x4 cl = ld4(a.tab.t0 + tr + 16 * c), sl = ld4(a.tab.t1 + tr + 16 * c);
                    const f32x4 ch = ld4(a.tab.t0 + tr + 16 * c + E / 2), sh = ld4(a.tab.t1 + tr + 16 * c + E / 2);
                    const f32x4 vl = gv[j][c], vh = gv[j][c + EC / 2];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float yl, yh;
                        rope::half_bwd(vl[r], vh[r], cl[r], sl[r], ch[r], sh[r], yl, yh);
                        gv[j][c][r] = yl, gv[j][c + EC / 2][r] = yh;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < EC; ++c)
                if (on && (c & (kWaves - 1)) == wv) st4(a.gu[j] + at + 16 * c, gv[j][c]);
        }
    }
    for (int kt = wv; kt < EC; kt += kWaves) {
        f32x4 acc = zero4();
#pragma unroll
        for (int j = 0; j < kMaxJobs; ++j) {
            if (j >= a.J) continue;
#pragma unroll
            for (int c = 0; c < EC; ++c) acc = mfma4(wcol4<E>(a.w[j], 16 * c + 4 * q, 16 * kt + x), gv[j][c], acc);
        }
        if (live) st4(a.gx + row * E + 16 * kt + 4 * q, acc);
    }
}

// DROP: dropout behind the ResBlock, y = (x + gelu(x W^T + b)) (.) M s * row_scale — the `nn.Dropout` of the output stack
// (draws: row_factors4, tag kTagOut, r the flat row).  The counter exchange is done by lane 0 of the last wave, its load in
// flight beside the rows' loads.  The DROP = false instantiations keep their code.
template <int EC, bool DROP = false>
__global__ void __launch_bounds__(kThreads) k_rows_res_fwd(const ResArgs a) {
    constexpr int E = 16 * EC;
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    DropDraw draw{};
    if constexpr (DROP) draw = draw_begin(a.d);
    const int64_t row = (int64_t)blockIdx.x * 16 + x;
    const bool live = row < a.rows;
    const int64_t rc = live ? row : a.rows - 1;
    const float* xp = a.x + rc * a.xs + 4 * q;
    f32x4 xv[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) xv[c] = ld4(xp + 16 * c);
    const float s = a.scale ? a.scale[rc] : 1.f;
    if constexpr (DROP) draw_share(a.d, draw);
    for (int nt = wv; nt < EC; nt += kWaves) {
        const float* wp = a.w + (16 * nt + x) * E + 4 * q;
        f32x4 wa[EC];
#pragma unroll
        for (int c = 0; c < EC; ++c) wa[c] = ld4(wp + 16 * c);
        const f32x4 bias = ld4(a.b + 16 * nt + 4 * q), res = ld4(xp + 16 * nt);
        f32x4 acc = zero4();
#pragma unroll
        for (int c = 0; c < EC; ++c) acc = mfma4(wa[c], xv[c], acc);
        acc += bias;
        f32x4 y;
        if constexpr (DROP) {
            const f32x4 f = row_factors4(draw, kTagOut, (uint32_t)rc * (uint32_t)(E / 4) + (uint32_t)(4 * nt + q));
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = (gelu_f(acc[r]) + res[r]) * f[r] * s;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = (gelu_f(acc[r]) + res[r]) * s;
        }
        if (live) {
            st4(a.y + row * E + 16 * nt + 4 * q, y);
            st4(a.pre + row * E + 16 * nt + 4 * q, acc);
        }
    }
}

// g = gy * scale;  gpre = g * gelu'(pre);  gx = g + gpre W
// (DROP: g = gy * scale (.) M s, the mask regenerated from the counter the forward left in `used`)
template <int EC, bool DROP = false>
__global__ void __launch_bounds__(kThreads) k_rows_res_bwd(const ResArgs a) {
    constexpr int E = 16 * EC;
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + x;
    const bool live = row < a.rows;
    const int64_t rc = live ? row : a.rows - 1;
    const float s = a.scale ? a.scale[rc] : 1.f;
    const float* gyp = a.gy + rc * E + 4 * q;
    const float* prp = a.pre + rc * E + 4 * q;
    DropDraw draw{};
    if constexpr (DROP) draw = a.d.draw(), draw.counter = (uint64_t)*a.d.used;
    const uint32_t blk = (uint32_t)rc * (uint32_t)(E / 4) + (uint32_t)q;
    f32x4 gp[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) {
        f32x4 g = ld4(gyp + 16 * c) * s;
        const f32x4 z = ld4(prp + 16 * c);
        if constexpr (DROP) g *= row_factors4(draw, kTagOut, blk + (uint32_t)(4 * c));
#pragma unroll
        for (int r = 0; r < 4; ++r) gp[c][r] = live ? g[r] * gelu_grad(z[r]) : 0.f;
        if (live && (c & (kWaves - 1)) == wv) st4(a.gpre + row * E + 16 * c + 4 * q, gp[c]);
    }
    for (int kt = wv; kt < EC; kt += kWaves) {
        f32x4 acc = zero4();
#pragma unroll
        for (int c = 0; c < EC; ++c) acc = mfma4(wcol4<E>(a.w, 16 * c + 4 * q, 16 * kt + x), gp[c], acc);
        f32x4 g = ld4(gyp + 16 * kt) * s;
        if constexpr (DROP) g *= row_factors4(draw, kTagOut, blk + (uint32_t)(4 * kt));
        if (live) st4(a.gx + row * E + 16 * kt + 4 * q, g + acc);
    }
}

// The dense q / k / v stacks of one input, dropout included, as one launch:
//   pre_j = x W1_j^T + b1_j;  h_j = (x + gelu(pre_j)) (.) M_j s;  out_j = h_j W2_j^T + b2_j     over the rows t >= L - tail[j]
// A workgroup owns 16 rows and walks the jobs; wave w owns the feature tiles w, w + 4, ... of BOTH layers.  The dropped hidden
// rows change owner between the layers — every wave needs all features of the 16 rows as its B operand — through LDS behind
// ONE workgroup barrier: the first layer's sums of all jobs stay in registers until the call counter has come back (its load
// is issued first thing), then the epilogues of all jobs, the barrier, and the second layers.  A job none of whose rows lie in
// the workgroup's tile (the cut query) is skipped by all four waves alike.
template <int EC>
__global__ void __launch_bounds__(kThreads) k_rows_dense_drop_fwd(const DenseArgs a) {
    constexpr int E = 16 * EC, TPW = (EC + kWaves - 1) / kWaves, PP = E + 4;      // (pitch E + 4: conflict-free 16-byte reads)
    __shared__ __attribute__((aligned(16))) float s_h[kMaxJobs][16][PP];
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    DropDraw draw = draw_begin(a.d);
    const int64_t rows = (int64_t)a.B * a.L, row = (int64_t)blockIdx.x * 16 + x;
    const bool live = row < rows;
    const int64_t rc = live ? row : rows - 1;
    const int b = (int)(rc / a.L), t = (int)(rc - (int64_t)b * a.L);
    const float* xp = a.x + b * a.xs_b + t * a.xs_t + 4 * q;
    f32x4 xv[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) xv[c] = live ? ld4(xp + 16 * c) : zero4();
    bool on[kMaxJobs], any_on[kMaxJobs];
    int64_t at[kMaxJobs];
    f32x4 pre[kMaxJobs][TPW];
#pragma unroll
    for (int j = 0; j < kMaxJobs; ++j) {
        on[j] = any_on[j] = false, at[j] = 0;
        if (j >= a.J) continue;
        const int skip = a.L - a.tail[j];
        on[j] = live && t >= skip;
        any_on[j] = __any(on[j]) != 0;                      // (every wave holds the same 16 rows: alike in all four)
        at[j] = ((int64_t)b * a.tail[j] + (on[j] ? t - skip : 0)) * E + 4 * q;
        if (!any_on[j]) continue;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int nt = wv + i * kWaves;
            if (nt >= EC) continue;
            const float* wp = a.w1[j] + (16 * nt + x) * E + 4 * q;
            f32x4 wa[EC];
#pragma unroll
            for (int c = 0; c < EC; ++c) wa[c] = ld4(wp + 16 * c);
            const f32x4 bias = ld4(a.b1[j] + 16 * nt + 4 * q);
            f32x4 acc = zero4();
#pragma unroll
            for (int c = 0; c < EC; ++c) acc = mfma4(wa[c], xv[c], acc);
            pre[j][i] = acc + bias;
            if (on[j]) st4(a.pre[j] + at[j] + 16 * nt, pre[j][i]);
        }
    }
    draw_share(a.d, draw);
    const uint32_t blk = (uint32_t)rc * (uint32_t)(E / 4) + (uint32_t)q;
#pragma unroll
    for (int j = 0; j < kMaxJobs; ++j) {
        if (j >= a.J || !any_on[j]) continue;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int nt = wv + i * kWaves;
            if (nt >= EC) continue;
            const f32x4 f = row_factors4(draw, kTagQkv + (uint32_t)j, blk + (uint32_t)(4 * nt));
            const f32x4 res = live ? ld4(xp + 16 * nt) : zero4();
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = (gelu_f(pre[j][i][r]) + res[r]) * f[r];
            st4(&s_h[j][x][16 * nt + 4 * q], h);
            if (on[j]) st4(a.h[j] + at[j] + 16 * nt, h);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kMaxJobs; ++j) {
        if (j >= a.J || !any_on[j]) continue;
        f32x4 hv[EC];
#pragma unroll
        for (int c = 0; c < EC; ++c) hv[c] = ld4(&s_h[j][x][16 * c + 4 * q]);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int nt = wv + i * kWaves;
            if (nt >= EC) continue;
            const float* wp = a.w2[j] + (16 * nt + x) * E + 4 * q;
            f32x4 wa[EC];
#pragma unroll
            for (int c = 0; c < EC; ++c) wa[c] = ld4(wp + 16 * c);
            const f32x4 bias = ld4(a.b2[j] + 16 * nt + 4 * q);
            f32x4 acc = zero4();
#pragma unroll
            for (int c = 0; c < EC; ++c) acc = mfma4(wa[c], hv[c], acc);
            if (on[j]) st4(a.y[j] + at[j] + 16 * nt, acc + bias);
        }
    }
}

//   g_h_j = (g_out_j W2_j) (.) M_j s;  g_pre_j = g_h_j gelu'(pre_j);  gx = sum_j (g_h_j + g_pre_j W1_j)
// The tile of g_h a wave forms is the tile of gx it owns, so the residual term stays in its registers; the g_pre rows change
// owner through LDS as the hidden rows do in the forward.  The mask is regenerated from the counter in `used`.
template <int EC>
__global__ void __launch_bounds__(kThreads) k_rows_dense_drop_bwd(const DenseArgs a) {
    constexpr int E = 16 * EC, TPW = (EC + kWaves - 1) / kWaves, PP = E + 4;
    __shared__ __attribute__((aligned(16))) float s_g[kMaxJobs][16][PP];
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    DropDraw draw = a.d.draw();
    draw.counter = (uint64_t)*a.d.used;
    const int64_t rows = (int64_t)a.B * a.L, row = (int64_t)blockIdx.x * 16 + x;
    const bool live = row < rows;
    const int64_t rc = live ? row : rows - 1;
    const int b = (int)(rc / a.L), t = (int)(rc - (int64_t)b * a.L);
    const uint32_t blk = (uint32_t)rc * (uint32_t)(E / 4) + (uint32_t)q;
    bool any_on[kMaxJobs];
    f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = zero4();
#pragma unroll
    for (int j = 0; j < kMaxJobs; ++j) {
        any_on[j] = false;
        if (j >= a.J) continue;
        const int skip = a.L - a.tail[j];
        const bool on = live && t >= skip;
        any_on[j] = __any(on) != 0;
        if (!any_on[j]) continue;
        const int64_t at = ((int64_t)b * a.tail[j] + (on ? t - skip : 0)) * E + 4 * q;
        f32x4 gv[EC];
#pragma unroll
        for (int c = 0; c < EC; ++c) gv[c] = on ? ld4(a.g[j] + at + 16 * c) : zero4();
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int kt = wv + i * kWaves;
            if (kt >= EC) continue;
            const f32x4 z = ld4(a.pre[j] + at + 16 * kt);
            f32x4 gh = zero4();
#pragma unroll
            for (int c = 0; c < EC; ++c) gh = mfma4(wcol4<E>(a.w2[j], 16 * c + 4 * q, 16 * kt + x), gv[c], gh);
            gh *= row_factors4(draw, kTagQkv + (uint32_t)j, blk + (uint32_t)(4 * kt));
            f32x4 gp;
#pragma unroll
            for (int r = 0; r < 4; ++r) gp[r] = on ? gh[r] * gelu_grad(z[r]) : 0.f;
            acc[i] += gh;
            st4(&s_g[j][x][16 * kt + 4 * q], gp);
            if (on) st4(a.gpre[j] + at + 16 * kt, gp);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kMaxJobs; ++j) {
        if (j >= a.J || !any_on[j]) continue;
        f32x4 gpv[EC];
#pragma unroll
        for (int c = 0; c < EC; ++c) gpv[c] = ld4(&s_g[j][x][16 * c + 4 * q]);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int kt = wv + i * kWaves;
            if (kt >= EC) continue;
#pragma unroll
            for (int c = 0; c < EC; ++c) acc[i] = mfma4(wcol4<E>(a.w1[j], 16 * c + 4 * q, 16 * kt + x), gpv[c], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int kt = wv + i * kWaves;
        if (kt < EC && live) st4(a.gx + row * E + 16 * kt + 4 * q, acc[i]);
    }
}

struct AffineArgs {
    const float* x; int64_t xs;              // [rows][K], row stride xs
    const float* w; const float* b;          // [N][K], [N]
    int64_t rows;
    int32_t K, N;
    float* y;                                // [rows][N] dense
    float* pre;                              // GELU form: the pre-activation, saved for the backward
};

// y = x W^T + b for a NARROW input (K <= 64: observation ++ action in front of a recurrent layer — the input products
// `x W_ih^T + b_ih` of all steps, reference seq_layers.py:14-114 through nn.GRU) and a wide output (N = 3 H): the library
// GEMM takes 13-14 us for 20 736 x 8 -> 192; the work is writing 16 MB.  A workgroup owns 16 rows, its waves the output
// tiles w, w + 4, ...; the x tile (K / 4 scalars a lane) is the B operand of every tile.
template <int STEPS, bool GELU>      // k-steps of four: K <= 4 STEPS;  GELU: y = gelu(x W^T + b), the sum itself to `pre`
__global__ void __launch_bounds__(kThreads) k_rows_affine(const AffineArgs a) {
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + x;
    const bool live = row < a.rows;
    const float* xp = a.x + (live ? row : a.rows - 1) * a.xs;
    float xv[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int k = 4 * s + q;
        const float got = xp[min(k, a.K - 1)];
        xv[s] = k < a.K ? got : 0.f;
    }
    const int NT = a.N >> 4;
    // TB of the wave's tiles at a time: their weight operands requested together with the rows (one round trip), then the
    // products and the stores
    constexpr int TB = STEPS <= 4 ? 4 : 1;
    for (int nt0 = wv; nt0 < NT; nt0 += TB * kWaves) {
        float wq[TB][STEPS];
        f32x4 bias[TB];
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const int nt = min(nt0 + j * kWaves, NT - 1);
            const float* wp = a.w + (int64_t)(16 * nt + x) * a.K;
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int k = 4 * s + q;
                const float got = wp[min(k, a.K - 1)];
                wq[j][s] = k < a.K ? got : 0.f;
            }
            bias[j] = ld4(a.b + 16 * nt + 4 * q);
        }
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const int nt = nt0 + j * kWaves;
            f32x4 acc = zero4();
#pragma unroll
            for (int s = 0; s < STEPS; ++s) acc = RP_MF(wq[j][s], xv[s], acc);
            acc += bias[j];
            if (live && nt < NT) {
                if (GELU) {
                    st4(a.pre + row * a.N + 16 * nt + 4 * q, acc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = gelu_f(acc[r]);
                }
                st4(a.y + row * a.N + 16 * nt + 4 * q, acc);
            }
        }
    }
}

inline bool width_ok(int E) { return E == 32 || E == 64 || E == 128; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// the draws' host checks: thr = floor(p 2^32) >= 1 and scale = float32(1 / (1 - p)) >= 1, finite, are what a p in (0, 1) gives;
// the Philox block index r (E / 4) + (f >> 2) is 32 bits wide: rows E < 2^34
inline bool draw_args_ok(int64_t rows, int width, uint32_t thr, float scale) {
    return thr >= 1u && scale >= 1.f && std::isfinite(scale) && rows < ((int64_t)1 << 34) / width;
}

}  // namespace rowsp
}  // namespace asac

using namespace asac;
using namespace asac::rowsp;

#define RP_LAUNCH(kernel, E, grid, stream, args)                                                    \
    do {                                                                                            \
        if ((E) == 32) ASAC_LAUNCH(kernel<2>, grid, dim3(kThreads), 0, stream, args);               \
        else if ((E) == 64) ASAC_LAUNCH(kernel<4>, grid, dim3(kThreads), 0, stream, args);          \
        else ASAC_LAUNCH(kernel<8>, grid, dim3(kThreads), 0, stream, args);                         \
    } while (0)

#define RP_LAUNCH_KIND(kernel, KIND, E, grid, stream, args)                                         \
    do {                                                                                            \
        if ((E) == 32) ASAC_LAUNCH((kernel<2, KIND>), grid, dim3(kThreads), 0, stream, args);       \
        else if ((E) == 64) ASAC_LAUNCH((kernel<4, KIND>), grid, dim3(kThreads), 0, stream, args);  \
        else ASAC_LAUNCH((kernel<8, KIND>), grid, dim3(kThreads), 0, stream, args);                 \
    } while (0)

// the checks and the launch of the projections' forward, plain (kind 0) or with the rotation behind jobs 0 and 1
static int proj_forward(const char* what, int kind, const ProjArgs& rot, const float* x, int64_t x_stride_b, int64_t x_stride_t,
                        int batch, int window, int width, int n_jobs, const float* const* weights, const float* const* biases,
                        const int* tails, float* const* outs, void* stream) {
    if (!x || !weights || !biases || !tails || !outs || batch <= 0 || window <= 0 || !width_ok(width) || n_jobs < 1 ||
        n_jobs > kMaxJobs || !aligned16(x) || (x_stride_b & 3) || (x_stride_t & 3) || x_stride_t < width)
        return bad_arg(what);
    ProjArgs a = rot;
    a.x = x, a.xs_b = x_stride_b, a.xs_t = x_stride_t, a.B = batch, a.L = window, a.J = n_jobs;
    for (int j = 0; j < n_jobs; ++j) {
        if (!weights[j] || !biases[j] || !outs[j] || tails[j] < 1 || tails[j] > window || !aligned16(weights[j]) ||
            !aligned16(biases[j]) || !aligned16(outs[j]))
            return bad_arg(what);
        a.w[j] = weights[j], a.b[j] = biases[j], a.tail[j] = tails[j], a.y[j] = outs[j];
    }
    const dim3 grid((unsigned)(((int64_t)batch * window + 15) / 16), (unsigned)n_jobs);
    if (kind == rope::kRope) RP_LAUNCH_KIND(k_rows_proj_fwd, rope::kRope, width, grid, as_stream(stream), a);
    else if (kind == rope::kRope2) RP_LAUNCH_KIND(k_rows_proj_fwd, rope::kRope2, width, grid, as_stream(stream), a);
    else RP_LAUNCH_KIND(k_rows_proj_fwd, 0, width, grid, as_stream(stream), a);
    return finish_launch(what);
}

static int proj_backward(const char* what, int kind, const ProjArgs& rot, const float* const* grads, const int* tails, int n_jobs,
                         const float* const* weights, int batch, int window, int width, float* grad_x, void* stream) {
    if (!grads || !tails || !weights || !grad_x || batch <= 0 || window <= 0 || !width_ok(width) || n_jobs < 1 ||
        n_jobs > kMaxJobs || !aligned16(grad_x))
        return bad_arg(what);
    ProjArgs a = rot;
    a.B = batch, a.L = window, a.J = n_jobs, a.gx = grad_x;
    for (int j = 0; j < n_jobs; ++j) {
        if (!weights[j] || !grads[j] || tails[j] < 1 || tails[j] > window || !aligned16(grads[j])) return bad_arg(what);
        a.w[j] = weights[j], a.g[j] = grads[j], a.tail[j] = tails[j];
    }
    const dim3 grid((unsigned)(((int64_t)batch * window + 15) / 16));
    if (kind == rope::kRope) RP_LAUNCH_KIND(k_rows_proj_bwd, rope::kRope, width, grid, as_stream(stream), a);
    else if (kind == rope::kRope2) RP_LAUNCH_KIND(k_rows_proj_bwd, rope::kRope2, width, grid, as_stream(stream), a);
    else RP_LAUNCH_KIND(k_rows_proj_bwd, 0, width, grid, as_stream(stream), a);
    return finish_launch(what);
}

// the rotary operands both passes share: the kind's tables (read as 16-byte vectors) and the index array
static bool rope_operands(ProjArgs& a, int kind, const float* table0, const float* table1, int table_rows, const void* index,
                          int64_t index_stride_b, int64_t index_stride_t, int index_bytes) {
    if (!rope::kind_ok(kind) || !table0 || !aligned16(table0) || (kind == rope::kRope2 && (!table1 || !aligned16(table1))) ||
        table_rows < 1 || !index || (index_bytes != 4 && index_bytes != 8) || index_stride_b < 0 || index_stride_t < 0)
        return false;
    a.tab = rope::Tables{table0, table1, table_rows};
    a.ix = rope::Index{index, index_stride_b, index_stride_t, index_bytes};
    return true;
}

extern "C" {

int asac_rows_proj_supported(int width) { return width_ok(width); }

int asac_rows_proj_forward(const float* x, int64_t x_stride_b, int64_t x_stride_t, int batch, int window, int width, int n_jobs,
                           const float* const* weights, const float* const* biases, const int* tails, float* const* outs,
                           void* stream) {
    return proj_forward("asac_rows_proj_forward", 0, ProjArgs{}, x, x_stride_b, x_stride_t, batch, window, width, n_jobs, weights,
                        biases, tails, outs, stream);
}

int asac_rows_proj_backward(const float* const* grads, const int* tails, int n_jobs, const float* const* weights, int batch,
                            int window, int width, float* grad_x, void* stream) {
    return proj_backward("asac_rows_proj_backward", 0, ProjArgs{}, grads, tails, n_jobs, weights, batch, window, width, grad_x,
                         stream);
}

int asac_rows_proj_rope_forward(int kind, const float* table0, const float* table1, int table_rows, const void* index,
                                int64_t index_stride_b, int64_t index_stride_t, int index_bytes, const float* x,
                                int64_t x_stride_b, int64_t x_stride_t, int batch, int window, int width,
                                const float* const* weights, const float* const* biases, const int* tails, float* const* outs,
                                void* stream) {
    ProjArgs rot{};
    if (!rope_operands(rot, kind, table0, table1, table_rows, index, index_stride_b, index_stride_t, index_bytes))
        return bad_arg("asac_rows_proj_rope_forward");
    return proj_forward("asac_rows_proj_rope_forward", kind, rot, x, x_stride_b, x_stride_t, batch, window, width, kMaxJobs,
                        weights, biases, tails, outs, stream);
}

int asac_rows_proj_rope_backward(int kind, const float* table0, const float* table1, int table_rows, const void* index,
                                 int64_t index_stride_b, int64_t index_stride_t, int index_bytes, const float* const* grads,
                                 const int* tails, const float* const* weights, int batch, int window, int width, float* grad_x,
                                 float* const* grads_unrotated, void* stream) {
    ProjArgs rot{};
    if (!rope_operands(rot, kind, table0, table1, table_rows, index, index_stride_b, index_stride_t, index_bytes) ||
        !grads_unrotated || !grads_unrotated[0] || !grads_unrotated[1] || !aligned16(grads_unrotated[0]) ||
        !aligned16(grads_unrotated[1]))
        return bad_arg("asac_rows_proj_rope_backward");
    rot.gu[0] = grads_unrotated[0], rot.gu[1] = grads_unrotated[1];
    return proj_backward("asac_rows_proj_rope_backward", kind, rot, grads, tails, kMaxJobs, weights, batch, window, width, grad_x,
                         stream);
}

int asac_rows_resblock_forward(const float* x, int64_t x_row_stride, const float* weight, const float* bias,
                               const float* row_scale, int64_t rows, int width, float* y, float* pre, void* stream) {
    if (!x || !weight || !bias || !y || !pre || rows <= 0 || !width_ok(width) || x_row_stride < width || (x_row_stride & 3) ||
        !aligned16(x) || !aligned16(weight) || !aligned16(bias) || !aligned16(y) || !aligned16(pre))
        return bad_arg("asac_rows_resblock_forward");
    ResArgs a{};
    a.x = x, a.xs = x_row_stride, a.w = weight, a.b = bias, a.scale = row_scale, a.rows = rows, a.y = y, a.pre = pre;
    const dim3 grid((unsigned)((rows + 15) / 16));
    RP_LAUNCH(k_rows_res_fwd, width, grid, as_stream(stream), a);
    return finish_launch("asac_rows_resblock_forward");
}

int asac_rows_resblock_backward(const float* grad_y, const float* pre, const float* weight, const float* row_scale,
                                int64_t rows, int width, float* grad_x, float* grad_pre, void* stream) {
    if (!grad_y || !pre || !weight || !grad_x || !grad_pre || rows <= 0 || !width_ok(width) || !aligned16(grad_y) ||
        !aligned16(pre) || !aligned16(grad_x) || !aligned16(grad_pre))
        return bad_arg("asac_rows_resblock_backward");
    ResArgs a{};
    a.gy = grad_y, a.pre = const_cast<float*>(pre), a.w = weight, a.scale = row_scale, a.rows = rows, a.gx = grad_x, a.gpre = grad_pre;
    const dim3 grid((unsigned)((rows + 15) / 16));
    RP_LAUNCH(k_rows_res_bwd, width, grid, as_stream(stream), a);
    return finish_launch("asac_rows_resblock_backward");
}

int asac_rows_resblock_dropout_forward(const float* x, int64_t x_row_stride, const float* weight, const float* bias,
                                       const float* row_scale, int64_t rows, int width, float* y, float* pre, uint32_t thr,
                                       float scale, uint64_t seed, uint32_t instance, int64_t* state, int64_t* used, void* stream) {
    if (!x || !weight || !bias || !y || !pre || !state || !used || rows <= 0 || !width_ok(width) || x_row_stride < width ||
        (x_row_stride & 3) || !aligned16(x) || !aligned16(weight) || !aligned16(bias) || !aligned16(y) || !aligned16(pre) ||
        !draw_args_ok(rows, width, thr, scale))
        return bad_arg("asac_rows_resblock_dropout_forward");
    ResArgs a{};
    a.x = x, a.xs = x_row_stride, a.w = weight, a.b = bias, a.scale = row_scale, a.rows = rows, a.y = y, a.pre = pre;
    a.d = DrawArgs{seed, instance, thr, scale, 0, state, used};
    const dim3 grid((unsigned)((rows + 15) / 16));
    // under the measurement repeat knob only the last repetition advances the counter: all of them draw alike
    for (int rep = 0; rep < g_launch_repeat; ++rep) {
        a.d.advance = rep == g_launch_repeat - 1;
        if (width == 32) hipLaunchKernelGGL((k_rows_res_fwd<2, true>), grid, dim3(kThreads), 0, as_stream(stream), a);
        else if (width == 64) hipLaunchKernelGGL((k_rows_res_fwd<4, true>), grid, dim3(kThreads), 0, as_stream(stream), a);
        else hipLaunchKernelGGL((k_rows_res_fwd<8, true>), grid, dim3(kThreads), 0, as_stream(stream), a);
    }
    return finish_launch("asac_rows_resblock_dropout_forward");
}

int asac_rows_resblock_dropout_backward(const float* grad_y, const float* pre, const float* weight, const float* row_scale,
                                        int64_t rows, int width, float* grad_x, float* grad_pre, uint32_t thr, float scale,
                                        uint64_t seed, uint32_t instance, const int64_t* used, void* stream) {
    if (!grad_y || !pre || !weight || !grad_x || !grad_pre || !used || rows <= 0 || !width_ok(width) || !aligned16(grad_y) ||
        !aligned16(pre) || !aligned16(grad_x) || !aligned16(grad_pre) || !draw_args_ok(rows, width, thr, scale))
        return bad_arg("asac_rows_resblock_dropout_backward");
    ResArgs a{};
    a.gy = grad_y, a.pre = const_cast<float*>(pre), a.w = weight, a.scale = row_scale, a.rows = rows, a.gx = grad_x, a.gpre = grad_pre;
    a.d = DrawArgs{seed, instance, thr, scale, 0, nullptr, const_cast<int64_t*>(used)};
    const dim3 grid((unsigned)((rows + 15) / 16));
    RP_LAUNCH_KIND(k_rows_res_bwd, true, width, grid, as_stream(stream), a);
    return finish_launch("asac_rows_resblock_dropout_backward");
}

int asac_rows_dense_proj_dropout_forward(const float* x, int64_t x_stride_b, int64_t x_stride_t, int batch, int window, int width,
                                         int n_jobs, const float* const* weights1, const float* const* biases1,
                                         const float* const* weights2, const float* const* biases2, const int* tails,
                                         float* const* outs, float* const* pres, float* const* hiddens, uint32_t thr, float scale,
                                         uint64_t seed, uint32_t instance, int64_t* state, int64_t* used, void* stream) {
    const char* what = "asac_rows_dense_proj_dropout_forward";
    if (!x || !weights1 || !biases1 || !weights2 || !biases2 || !tails || !outs || !pres || !hiddens || !state || !used ||
        batch <= 0 || window <= 0 || !width_ok(width) || n_jobs < 1 || n_jobs > kMaxJobs || !aligned16(x) || (x_stride_b & 3) ||
        (x_stride_t & 3) || x_stride_t < width || !draw_args_ok((int64_t)batch * window, width, thr, scale))
        return bad_arg(what);
    DenseArgs a{};
    a.x = x, a.xs_b = x_stride_b, a.xs_t = x_stride_t, a.B = batch, a.L = window, a.J = n_jobs;
    for (int j = 0; j < n_jobs; ++j) {
        if (tails[j] < 1 || tails[j] > window) return bad_arg(what);
        for (const void* p : {(const void*)weights1[j], (const void*)biases1[j], (const void*)weights2[j], (const void*)biases2[j],
                              (const void*)outs[j], (const void*)pres[j], (const void*)hiddens[j]})
            if (!p || !aligned16(p)) return bad_arg(what);
        a.w1[j] = weights1[j], a.b1[j] = biases1[j], a.w2[j] = weights2[j], a.b2[j] = biases2[j], a.tail[j] = tails[j];
        a.y[j] = outs[j], a.pre[j] = pres[j], a.h[j] = hiddens[j];
    }
    a.d = DrawArgs{seed, instance, thr, scale, 0, state, used};
    const dim3 grid((unsigned)(((int64_t)batch * window + 15) / 16));
    for (int rep = 0; rep < g_launch_repeat; ++rep) {
        a.d.advance = rep == g_launch_repeat - 1;
        if (width == 32) hipLaunchKernelGGL(k_rows_dense_drop_fwd<2>, grid, dim3(kThreads), 0, as_stream(stream), a);
        else if (width == 64) hipLaunchKernelGGL(k_rows_dense_drop_fwd<4>, grid, dim3(kThreads), 0, as_stream(stream), a);
        else hipLaunchKernelGGL(k_rows_dense_drop_fwd<8>, grid, dim3(kThreads), 0, as_stream(stream), a);
    }
    return finish_launch(what);
}

int asac_rows_dense_proj_dropout_backward(const float* const* grads, const float* const* pres, const int* tails, int n_jobs,
                                          const float* const* weights1, const float* const* weights2, int batch, int window,
                                          int width, float* grad_x, float* const* grad_pres, uint32_t thr, float scale,
                                          uint64_t seed, uint32_t instance, const int64_t* used, void* stream) {
    const char* what = "asac_rows_dense_proj_dropout_backward";
    if (!grads || !pres || !tails || !weights1 || !weights2 || !grad_x || !grad_pres || !used || batch <= 0 || window <= 0 ||
        !width_ok(width) || n_jobs < 1 || n_jobs > kMaxJobs || !aligned16(grad_x) ||
        !draw_args_ok((int64_t)batch * window, width, thr, scale))
        return bad_arg(what);
    DenseArgs a{};
    a.B = batch, a.L = window, a.J = n_jobs, a.gx = grad_x;
    for (int j = 0; j < n_jobs; ++j) {
        if (tails[j] < 1 || tails[j] > window || !weights1[j] || !weights2[j]) return bad_arg(what);
        for (const void* p : {(const void*)grads[j], (const void*)pres[j], (const void*)grad_pres[j]})
            if (!p || !aligned16(p)) return bad_arg(what);
        a.w1[j] = weights1[j], a.w2[j] = weights2[j], a.tail[j] = tails[j];
        a.g[j] = grads[j], a.pre[j] = const_cast<float*>(pres[j]), a.gpre[j] = grad_pres[j];
    }
    a.d = DrawArgs{seed, instance, thr, scale, 0, nullptr, const_cast<int64_t*>(used)};
    const dim3 grid((unsigned)(((int64_t)batch * window + 15) / 16));
    RP_LAUNCH(k_rows_dense_drop_bwd, width, grid, as_stream(stream), a);
    return finish_launch(what);
}

int asac_rows_affine_supported(int K, int N) { return K >= 1 && K <= 64 && N >= 16 && N <= 1024 && (N & 15) == 0; }

static int affine_launch(const char* what, const float* x, int64_t x_row_stride, int K, const float* weight, const float* bias,
                         int64_t rows, int N, float* y, float* pre, void* stream) {
    if (!x || !weight || !bias || !y || rows <= 0 || !asac_rows_affine_supported(K, N) || x_row_stride < K || !aligned16(bias) ||
        !aligned16(y) || (pre && !aligned16(pre)))
        return bad_arg(what);
    AffineArgs a{};
    a.x = x, a.xs = x_row_stride, a.w = weight, a.b = bias, a.rows = rows, a.K = K, a.N = N, a.y = y, a.pre = pre;
    const dim3 grid((unsigned)((rows + 15) / 16));
    hipStream_t s = as_stream(stream);
    if (pre) {
        if (K <= 8) ASAC_LAUNCH((k_rows_affine<2, true>), grid, dim3(kThreads), 0, s, a);
        else if (K <= 16) ASAC_LAUNCH((k_rows_affine<4, true>), grid, dim3(kThreads), 0, s, a);
        else ASAC_LAUNCH((k_rows_affine<16, true>), grid, dim3(kThreads), 0, s, a);
    } else {
        if (K <= 8) ASAC_LAUNCH((k_rows_affine<2, false>), grid, dim3(kThreads), 0, s, a);
        else if (K <= 16) ASAC_LAUNCH((k_rows_affine<4, false>), grid, dim3(kThreads), 0, s, a);
        else ASAC_LAUNCH((k_rows_affine<16, false>), grid, dim3(kThreads), 0, s, a);
    }
    return finish_launch(what);
}

int asac_rows_affine_forward(const float* x, int64_t x_row_stride, int K, const float* weight, const float* bias, int64_t rows,
                             int N, float* y, void* stream) {
    return affine_launch("asac_rows_affine_forward", x, x_row_stride, K, weight, bias, rows, N, y, nullptr, stream);
}

int asac_rows_affine_gelu_forward(const float* x, int64_t x_row_stride, int K, const float* weight, const float* bias,
                                  int64_t rows, int N, float* y, float* pre, void* stream) {
    if (!pre) return bad_arg("asac_rows_affine_gelu_forward");
    return affine_launch("asac_rows_affine_gelu_forward", x, x_row_stride, K, weight, bias, rows, N, y, pre, stream);
}

}  // extern "C"
