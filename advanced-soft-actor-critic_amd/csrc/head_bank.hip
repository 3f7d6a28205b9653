// Head banks (reference nn_models: ModelQ.d_dense_list / ModelPolicy.d_dense_list): G groups of K independent stacks
// LinearLayers(S, W, depth, size_k) on the same rows — a critic ensemble's branch stacks, or a policy's.  The rows are few and
// the stacks small, so a pass is ONE grid over (tile of 16 rows, stack); the members are reached through a device table of
// per-stack parameter pointers, as csrc/drnd.hip reaches its members.
//
//   k_head_bank<false>   forward.  The tile's activations stay in two LDS tiles that take turns; ONE layer's weights are staged
//                        at a time (the stacks lie back to back in a flat buffer behind head biases of 3 or 2 floats, so
//                        nothing is assumed more than 4-byte aligned: a wave stages a row with dword loads, 256 consecutive
//                        bytes a request).  A layer is mfma_f32_16x16x4f32 with the weights as A and the rows as the N
//                        dimension (csrc/asac_rnd.h): wave w forms feature blocks w and w + 4, lane (g, r) ends with features
//                        16 fb + 4 g + {0..3} of row r after EVERY layer, so residuals and GELU derivatives never leave it.
//   k_head_bank<true>    backward, launch 1: the same forward (its layer outputs also go to records), then the cotangent
//                        chain back from the head through the re-staged weights (the transposed product reads W by columns);
//                        gz_l goes to records.  grad_x: every stack publishes gh_0 and the tile's last arriver adds the M
//                        stacks in ascending order.
//   k_head_bank_products backward, launch 2: grid (16 outputs, layer, stack).  dW[o][k] = sum_r gz[r][o] h[r][k] with the
//                        ROWS as the MFMA's k dimension, straight from the records (padded to whole tiles with zero
//                        cotangents: no row test in the loop); wave w holds input blocks w and w + 4, wave 0 also the bias
//                        (the same A against a B of ones).  The products run as mfma_f64_16x16x4f64 on the
//                        float32 records: exact products, float64 sums, ONE rounding where a gradient is stored — a float32
//                        chain over a few hundred rows loses to the tree sums of the library GEMMs it replaces.  One workgroup
//                        adds all the rows of its outputs in ascending order: nothing is exchanged.
// No float atomics: equal inputs give equal bits.
#include "asac_categorical.h"
#include "asac_common.h"
#include "asac_ordered_finish.h"
#include "asac_rnd.h"

namespace asac {
namespace head_bank {

using rnd::f32x4;
using rnd::ld4;
using rnd::mfma4;
using rnd::pad16;
using rnd::st4;
using rnd::zero4;

constexpr int kThreads = 256, kTile = 16, kMaxDepth = ASAC_HEAD_BANK_MAX_DEPTH, kMaxK = ASAC_DISCRETE_MAX_BRANCHES;
constexpr int kHeadPitch = ASAC_DISCRETE_MAX_WIDTH;       // floats between rows of the head's cotangent record

struct BankDev {
    const float* x;
    int64_t x_ss, x_st;
    const float* const* params;
    float* out;                     // forward
    const float* gout;              // backward ...
    float *gx, *xrec, *rec, *part;
    unsigned int* counter;
    int64_t stack_words;
    int32_t S, W, Wp, depth, K, D, N, T, npad;        // Wp: W padded to 64 or 128 with zero features
    int32_t res[kMaxDepth];
    int32_t size[kMaxK], off[kMaxK];
};

using f64x4 = __attribute__((ext_vector_type(4))) double;
#define ASAC_HB_MF64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// erf-form GELU and its derivative with the library's erff / expf (about one unit in the last place).  asac_gelu.h's
// gelu_parts carries the 1.5e-7 ABSOLUTE error of Abramowitz-Stegun 7.1.26, which at these stacks' few rows is larger than the
// float32 rounding of everything else in the pass and than what the float32 torch composition makes; here the
// transcendental is a handful of instructions beside a layer's products.
__device__ __forceinline__ void gelu_exact(float z, float& value, float& deriv) {
    const float cdf = 0.5f * (1.f + erff(z * 0.70710678118654752440f));
    value = z * cdf;
    deriv = fmaf(z * 0.39894228040143267794f, expf(-0.5f * (z * z)), cdf);
}

__host__ __device__ inline int pad_width(int W) { return W <= 64 ? 64 : 128; }
// (below, W is the PADDED width)
__host__ __device__ inline int pitch_of(int S, int W) { return (pad16(S) > W ? pad16(S) : W) + 4; }
// weights [W][pitch] | bias [128] | x tile and two activation tiles [16][pitch]
__host__ __device__ inline int lds_floats(int S, int W) { return W * pitch_of(S, W) + 128 + 3 * kTile * pitch_of(S, W); }

// one Linear, global -> LDS [rows_pad][P] (+ bias [rows_pad]), zeros in the padding: wave w takes rows w, w + 4, ..; a lane
// takes columns lane and lane + 64.  Dword loads: the matrix may start at any float.
__device__ __forceinline__ void stage(const float* gw, const float* gb, int rows, int cols, int rows_pad, int cols_pad,
                                      float* Wl, float* bl, int P) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll 4
    for (int r = wave; r < rows_pad; r += 4) {
        const float* src = gw + r * cols;
        for (int c = lane; c < cols_pad; c += 64) Wl[r * P + c] = (r < rows && c < cols) ? src[c] : 0.f;
    }
    if (tid < rows_pad) bl[tid] = tid < rows ? gb[tid] : 0.f;
}

// z[row r][16 fb + 4 g + i] = b[..] + sum_k W[16 fb + 4 g + i][k] X[r][k],  k < Kp (a multiple of 16)
__device__ __forceinline__ f32x4 fwd_block(const float* Wl, const float* X, const float* bl, int P, int Kp, int fb, int lane) {
    const int r = lane & 15, g = lane >> 4;
    const float* wp = Wl + (16 * fb + r) * P + 4 * g;
    const float* xp = X + r * P + 4 * g;
    // four accumulators take the blocks of 16 inputs in turn and meet in a tree: a chain is at most 32 inputs long (a sum's
    // rounding error grows with its chain), and no product waits for the one before it
    f32x4 c0 = zero4(), c1 = zero4(), c2 = zero4(), c3 = zero4();
    for (int k0 = 0; k0 < Kp; k0 += 64) {
        c0 = mfma4(ld4(wp + k0), ld4(xp + k0), c0);
        if (k0 + 16 < Kp) c1 = mfma4(ld4(wp + k0 + 16), ld4(xp + k0 + 16), c1);
        if (k0 + 32 < Kp) c2 = mfma4(ld4(wp + k0 + 32), ld4(xp + k0 + 32), c2);
        if (k0 + 48 < Kp) c3 = mfma4(ld4(wp + k0 + 48), ld4(xp + k0 + 48), c3);
    }
    return ((c0 + c1) + (c2 + c3)) + ld4(bl + 16 * fb + 4 * g);
}

// gh[row r][16 cb + 4 g + i] = sum_f G[r][f] W[f][16 cb + 4 g + i],  f < Fp (a multiple of 16)
__device__ __forceinline__ f32x4 bwd_block(const float* Wl, const float* G, int P, int Fp, int cb, int lane) {
    const int r = lane & 15, g = lane >> 4;
    const float* wp = Wl + (4 * g) * P + 16 * cb + r;
    const float* gp = G + r * P + 4 * g;
    f32x4 c[4] = {zero4(), zero4(), zero4(), zero4()};       // as in fwd_block: four chains, a tree
    for (int f0 = 0; f0 < Fp; f0 += 64) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (f0 + 16 * q < Fp) {
                f32x4 a;
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = wp[(f0 + 16 * q + i) * P];
                c[q] = mfma4(a, ld4(gp + f0 + 16 * q), c[q]);
            }
        }
    }
    return (c[0] + c[1]) + (c[2] + c[3]);
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void k_head_bank(const BankDev v) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g4 = 4 * (lane >> 4);
    const int S = v.S, W = v.W, Wp = v.Wp, Sp = pad16(S), P = pitch_of(S, Wp), depth = v.depth, N = v.N;
    const int m = blockIdx.y, grp = m / v.K, k = m - grp * v.K, sz = v.size[k], szp = pad16(sz), off = v.off[k];
    const int row0 = blockIdx.x * kTile, nfb = Wp / 64;
    float* Wl = lds;
    float* bl = Wl + Wp * P;
    float* xt = bl + 128;
    float* ha = xt + kTile * P;
    float* hb = ha + kTile * P;
    const float* const* rec = v.params + (int64_t)m * 2 * (depth + 1);
    float* srec = BWD ? v.rec + (int64_t)m * v.stack_words : nullptr;       // h_1 .. h_depth | gz_0 .. gz_{depth-1} | head gz
    const int64_t lw = (int64_t)v.npad * Wp;                                // floats of one [npad][Wp] record

    const int Xc = P - 4;                             // the tile's columns: zeros behind S (a residual first block reads Wp of them)
    for (int i = tid; i < kTile * Xc; i += kThreads) {
        const int rr = i / Xc, c = i - rr * Xc, row = row0 + rr;
        float xv = 0.f;
        if (row < N && c < S) {
            const int s = row / v.T, t = row - s * v.T;
            xv = v.x[s * v.x_ss + t * v.x_st + c];
        }
        xt[rr * P + c] = xv;
        if (BWD && m == 0 && c < Sp) v.xrec[(int64_t)row * Sp + c] = xv;
    }

    const float* in = xt;
    float* outT = ha;
    int Kp = Sp;
    f32x4 d[kMaxDepth][2];                            // gelu'(z_l) of this lane's (row, features)
#pragma unroll
    for (int l = 0; l < kMaxDepth; ++l) d[l][0] = d[l][1] = zero4();
#pragma unroll
    for (int l = 0; l < kMaxDepth; ++l) {
        if (l < depth) {
            stage(rec[2 * l], rec[2 * l + 1], W, l ? W : S, Wp, Kp, Wl, bl, P);
            __syncthreads();                          // the weights, and (first layer) the x tile
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j < nfb) {
                    const int c = 16 * (wave + 4 * j) + g4;
                    const f32x4 z = fwd_block(Wl, in, bl, P, Kp, wave + 4 * j, lane);
                    f32x4 h;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float val, der;
                        gelu_exact(z[i], val, der);
                        h[i] = val, d[l][j][i] = der;
                    }
                    if (v.res[l]) h = h + ld4(in + r * P + c);
                    st4(outT + r * P + c, h);
                    if (BWD) st4(srec + l * lw + (int64_t)(row0 + r) * Wp + c, h);      // h_{l+1}: the next layer's input
                }
            }
            __syncthreads();                          // every wave is done with the weights and the input tile
            in = outT;
            outT = outT == ha ? hb : ha;
            Kp = Wp;
        }
    }

    if (!BWD) {
        stage(rec[2 * depth], rec[2 * depth + 1], sz, W, szp, Wp, Wl, bl, P);
        __syncthreads();
        if (16 * wave < szp) {
            const f32x4 z = fwd_block(Wl, in, bl, P, Wp, wave, lane);
            const int row = row0 + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 16 * wave + g4 + i;
                if (row < N && c < sz) v.out[((int64_t)grp * N + row) * v.D + off + c] = z[i];
            }
        }
        return;
    }

    // ---- the cotangent chain.  Gt: the tile that is free (the other one holds h_depth, which the chain does not read)
    float* Gt = outT;
    float* hrec = srec + 2 * depth * lw;
    for (int i = tid; i < kTile * szp; i += kThreads) {
        const int rr = i / szp, c = i - rr * szp, row = row0 + rr;
        const float gv = (row < N && c < sz) ? v.gout[((int64_t)grp * N + row) * v.D + off + c] : 0.f;
        Gt[rr * P + c] = gv;
        hrec[(int64_t)row * kHeadPitch + c] = gv;
    }
    stage(rec[2 * depth], rec[2 * depth + 1], sz, W, szp, Wp, Wl, bl, P);
    __syncthreads();
    f32x4 gh[2] = {zero4(), zero4()};
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (j < nfb) gh[j] = bwd_block(Wl, Gt, P, szp, wave + 4 * j, lane);
#pragma unroll
    for (int l = kMaxDepth - 1; l >= 0; --l) {
        if (l < depth) {
            f32x4 gz[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) gz[j] = gh[j] * d[l][j];
            __syncthreads();                          // every wave is done with Gt and the weights staged before
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j < nfb) {
                    const int c = 16 * (wave + 4 * j) + g4;
                    st4(Gt + r * P + c, gz[j]);
                    st4(srec + (depth + l) * lw + (int64_t)(row0 + r) * Wp + c, gz[j]);
                }
            }
            if (l > 0 || v.gx) {
                const int cols = l ? W : S, colsp = l ? Wp : Sp;
                stage(rec[2 * l], rec[2 * l + 1], W, cols, Wp, colsp, Wl, bl, P);
                __syncthreads();
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    f32x4 t = zero4();
                    if (16 * (wave + 4 * j) < colsp) {
                        t = bwd_block(Wl, Gt, P, Wp, wave + 4 * j, lane);
                        if (v.res[l]) t = t + gh[j];
                    }
                    gh[j] = t;
                }
            }
        }
    }
    if (!v.gx) return;
    // gh: this stack's d / d x, columns 16 (wave + 4 j) + g4 + {0..3} of row r
    const int M = gridDim.y;
    if (M == 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 16 * (wave + 4 * j) + g4 + i, row = row0 + r;
                if (row < N && c < S) v.gx[(int64_t)row * S + c] = gh[j][i];
            }
        return;
    }
    float* mine = v.part + ((int64_t)m * v.npad + row0) * Sp;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 16 * (wave + 4 * j) + g4 + i;
            if (c < Sp) finish_publish(mine + r * Sp + c, gh[j][i]);
        }
    if (!finish_arrive(v.counter + blockIdx.x, (unsigned)M)) return;
    float* base = v.part + (int64_t)row0 * Sp;
    for (int i = tid; i < kTile * Sp; i += kThreads) {
        const int rr = i / Sp, c = i - rr * Sp, row = row0 + rr;
        if (row < N && c < S) v.gx[(int64_t)row * S + c] = finish_sum_in_order(base + rr * Sp + c, (int64_t)v.npad * Sp, M);
    }
    if (tid == 0) finish_reset(v.counter + blockIdx.x);
}

struct ProdDev {
    const float *xrec, *rec;
    float* const* grads;
    int64_t stack_words;
    int32_t S, W, Wp, depth, K, npad, accumulate;
    int32_t size[kMaxK];
};

__global__ __launch_bounds__(kThreads) void k_head_bank_products(const ProdDev v) {
    const int fb = blockIdx.x, l = blockIdx.y, m = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int W = v.W, Wp = v.Wp, S = v.S, depth = v.depth, npad = v.npad;
    const int outs = l < depth ? W : v.size[m % v.K];
    if (16 * fb >= outs) return;
    const int ins = l ? W : S, inp = l ? Wp : pad16(S);
    const int64_t lw = (int64_t)npad * Wp;
    const float* srec = v.rec + (int64_t)m * v.stack_words;
    const float* A = l < depth ? srec + (depth + l) * lw : srec + 2 * depth * lw;      // gz [npad][pa]
    const int pa = l < depth ? Wp : kHeadPitch;
    const float* B = l ? srec + (l - 1) * lw : v.xrec;                                 // h [npad][inp]
    const bool has0 = 16 * wave < inp, has1 = 16 * (wave + 4) < inp;
    const float* ap = A + (int64_t)g * pa + 16 * fb + r;
    const float* bp = B + (int64_t)g * inp + 16 * wave + r;
    f64x4 acc0 = {0., 0., 0., 0.}, acc1 = acc0, accb = acc0;
    for (int r0 = 0; r0 < npad; r0 += kTile) {        // (npad is whole tiles) a tile's twelve loads before its first product
        float a[4], b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t rb = r0 + 4 * u;
            a[u] = ap[rb * pa];
            b0[u] = has0 ? bp[rb * inp] : 0.f;
            b1[u] = has1 ? bp[rb * inp + 64] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = ASAC_HB_MF64((double)a[u], (double)b0[u], acc0);
            acc1 = ASAC_HB_MF64((double)a[u], (double)b1[u], acc1);
            if (wave == 0) accb = ASAC_HB_MF64((double)a[u], 1., accb);
        }
    }
    // lane (g, r), register i (the f64 form's map): dW[16 fb + g + 4 i][16 kb + r], kb = wave | wave + 4; wave 0, r == 0:
    // db[16 fb + g + 4 i].  One rounding, to float32, where the sum is stored.
    float* const* grec = v.grads + (int64_t)m * 2 * (depth + 1);
    float* gw = grec[2 * l];
    float* gb = grec[2 * l + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = 16 * fb + g + 4 * i;
        if (o >= outs) continue;
        const int c0 = 16 * wave + r, c1 = c0 + 64;
        if (c0 < ins) gw[o * ins + c0] = v.accumulate ? gw[o * ins + c0] + (float)acc0[i] : (float)acc0[i];
        if (c1 < ins) gw[o * ins + c1] = v.accumulate ? gw[o * ins + c1] + (float)acc1[i] : (float)acc1[i];
        if (wave == 0 && r == 0) gb[o] = v.accumulate ? gb[o] + (float)accb[i] : (float)accb[i];
    }
}

struct Layout {            // the backward workspace, in floats
    int64_t npad, tiles, xrec, stack_words, rec, part, counters, total;
};
static Layout layout_of(int64_t N, int S, int W_actual, int depth, int M) {
    Layout L;
    const int W = pad_width(W_actual);
    L.tiles = (N + kTile - 1) / kTile, L.npad = L.tiles * kTile;
    L.xrec = 0;
    L.rec = L.npad * pad16(S);
    L.stack_words = L.npad * (2 * (int64_t)depth * W + kHeadPitch);
    L.part = L.rec + M * L.stack_words;
    L.counters = L.part + (M > 1 ? M * L.npad * pad16(S) : 0);
    L.total = L.counters + (L.tiles + 3) / 4 * 4;
    return L;
}

static bool bank_ok(const asac_head_bank_t* b) {
    if (!b || !cat_branches_ok(b->branches)) return false;
    if (!asac_head_bank_supported(b->S, b->W, b->depth, b->branches.K, b->branches.D, b->G)) return false;
    for (int l = 0; l < b->depth; ++l)
        if (b->residual[l] != 0 && b->residual[l] != 1) return false;
    return b->residual[0] == 0 || b->S == b->W;
}

static void fill(BankDev& v, const asac_head_bank_t* b, const float* const* params, const float* x, int64_t ss, int64_t st,
                 int64_t N, int steps) {
    v.x = x, v.x_ss = ss, v.x_st = st, v.params = params;
    v.S = b->S, v.W = b->W, v.Wp = pad_width(b->W), v.depth = b->depth, v.K = b->branches.K, v.D = b->branches.D, v.N = (int)N, v.T = steps;
    for (int l = 0; l < kMaxDepth; ++l) v.res[l] = l < b->depth ? b->residual[l] : 0;
    int off = 0;
    for (int k = 0; k < b->branches.K; ++k) v.size[k] = b->branches.size[k], v.off[k] = off, off += b->branches.size[k];
}

}  // namespace head_bank
}  // namespace asac

using namespace asac;
using namespace asac::head_bank;

extern "C" {

int asac_head_bank_supported(int S, int W, int depth, int K, int D, int G) {
    return S > 0 && S <= ASAC_HEAD_BANK_MAX_IN && W > 0 && W <= ASAC_HEAD_BANK_MAX_WIDTH && depth >= 1 && depth <= ASAC_HEAD_BANK_MAX_DEPTH &&
           K > 0 && K <= ASAC_DISCRETE_MAX_BRANCHES && D >= K && D <= ASAC_DISCRETE_MAX_WIDTH && G > 0 &&
           G <= ASAC_HEAD_BANK_MAX_GROUPS && G * K <= ASAC_HEAD_BANK_MAX_STACKS;
}

int asac_head_bank_forward(const asac_head_bank_t* bank, const float* const* params, const float* x, int64_t x_stride_sample,
                           int64_t x_stride_step, int64_t samples, int steps, float* out, void* stream) {
    if (!bank_ok(bank) || !params || samples < 0 || steps <= 0 || samples * steps > ASAC_HEAD_BANK_MAX_ROWS)
        return bad_arg("asac_head_bank_forward");
    const int64_t N = samples * steps;
    if (N == 0) return 0;
    if (!x || !out) return bad_arg("asac_head_bank_forward: x / out");
    const size_t lds = sizeof(float) * lds_floats(bank->S, pad_width(bank->W));
    static bool lds_done = false;
    if (rnd::set_lds_limit((const void*)k_head_bank<false>, sizeof(float) * lds_floats(ASAC_HEAD_BANK_MAX_IN, ASAC_HEAD_BANK_MAX_WIDTH),
                           lds_done, "asac_head_bank_forward: hipFuncSetAttribute"))
        return 1;
    BankDev v{};
    fill(v, bank, params, x, x_stride_sample, x_stride_step, N, steps);
    v.out = out;
    const unsigned tiles = (unsigned)((N + kTile - 1) / kTile), M = (unsigned)(bank->G * bank->branches.K);
    ASAC_LAUNCH(k_head_bank<false>, dim3(tiles, M), dim3(kThreads), lds, as_stream(stream), v);
    return finish_launch("asac_head_bank_forward");
}

int64_t asac_head_bank_backward_workspace(int64_t n_rows, int S, int W, int depth, int D, int M) {
    if (n_rows <= 0 || n_rows > ASAC_HEAD_BANK_MAX_ROWS || S <= 0 || S > ASAC_HEAD_BANK_MAX_IN || W <= 0 || W > ASAC_HEAD_BANK_MAX_WIDTH ||
        depth < 1 || depth > ASAC_HEAD_BANK_MAX_DEPTH || D <= 0 || D > ASAC_DISCRETE_MAX_WIDTH || M <= 0 ||
        M > ASAC_HEAD_BANK_MAX_STACKS)
        return -1;
    return layout_of(n_rows, S, W, depth, M).total;
}

int asac_head_bank_backward(const asac_head_bank_t* bank, const float* const* params, float* const* grads, const float* x,
                            int64_t x_stride_sample, int64_t x_stride_step, int64_t samples, int steps, const float* grad_out,
                            float* grad_x, int accumulate, float* workspace, void* stream) {
    if (!bank_ok(bank) || !params || (!grads && !grad_x) || samples < 0 || steps <= 0 ||
        samples * steps > ASAC_HEAD_BANK_MAX_ROWS)
        return bad_arg("asac_head_bank_backward");
    const int64_t N = samples * steps;
    if (N == 0) return 0;
    if (!x || !grad_out || !workspace || !rnd::aligned16(workspace)) return bad_arg("asac_head_bank_backward: x / grad_out / workspace");
    const int M = bank->G * bank->branches.K;
    const Layout L = layout_of(N, bank->S, bank->W, bank->depth, M);
    const size_t lds = sizeof(float) * lds_floats(bank->S, pad_width(bank->W));
    static bool lds_done = false;
    if (rnd::set_lds_limit((const void*)k_head_bank<true>, sizeof(float) * lds_floats(ASAC_HEAD_BANK_MAX_IN, ASAC_HEAD_BANK_MAX_WIDTH),
                           lds_done, "asac_head_bank_backward: hipFuncSetAttribute"))
        return 1;
    BankDev v{};
    fill(v, bank, params, x, x_stride_sample, x_stride_step, N, steps);
    v.gout = grad_out, v.gx = grad_x, v.xrec = workspace + L.xrec, v.rec = workspace + L.rec, v.part = workspace + L.part;
    v.counter = reinterpret_cast<unsigned int*>(workspace + L.counters);
    v.stack_words = L.stack_words, v.npad = (int)L.npad;
    ASAC_LAUNCH(k_head_bank<true>, dim3((unsigned)L.tiles, (unsigned)M), dim3(kThreads), lds, as_stream(stream), v);
    if (int rc = finish_launch("asac_head_bank_backward")) return rc;
    if (!grads) return 0;
    ProdDev p{};
    p.xrec = v.xrec, p.rec = v.rec, p.grads = grads, p.stack_words = L.stack_words;
    p.S = bank->S, p.W = bank->W, p.Wp = pad_width(bank->W), p.depth = bank->depth, p.K = bank->branches.K, p.npad = (int)L.npad, p.accumulate = accumulate != 0;
    for (int k = 0; k < p.K; ++k) p.size[k] = bank->branches.size[k];
    ASAC_LAUNCH(k_head_bank_products, dim3(ASAC_HEAD_BANK_MAX_WIDTH / 16, (unsigned)(bank->depth + 1), (unsigned)M), dim3(kThreads), 0,
                as_stream(stream), p);
    return finish_launch("asac_head_bank_backward: products");
}

}  // extern "C"
