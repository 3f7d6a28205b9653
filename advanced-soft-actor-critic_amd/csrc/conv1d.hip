// One-launch 1-D convolution stack over rays (asac_conv1_forward / asac_conv1_backward, include/asac_hip.h):
//   Conv1d(C -> O1, k1, s1)  LeakyReLU  Conv1d(O1 -> O2, k2, s2)  LeakyReLU,  no padding, dilation 1, groups 1
// — the `default` stack of `Conv1dLayers` (nn_models/layers/image_layers.py), the reference's ray-sensor encoder.
//
// Layouts.  x [N][L][C] as stored (channels last), so the layer-1 patch of position p is the K1 = C k1 consecutive floats at
// p s1 C, position-major and channel-minor: patch index k = j C + c.  The staged weights are re-indexed to that order
// (w1s[o][j C + c] = w1[o][c][j]), the rays are not touched.  The layer-1 activations live in LDS as a1s[ray, position][A1S]
// (channel-minor, A1S >= O1 chosen so that the 16 positions of a tile start in different banks), the layer-2 patch index is
// k = j O1 + c at offset j A1S + c, and w2s[o][j O1 + c] = w2[o][c][j].  y [N][O2 L2] channel-major.
//
// Products: v_mfma_f32_16x16x4_f32, output channels = M (one tile for layer 1, up to two for layer 2), positions = N, the
// patch = K in steps of 4.  Operand lanes: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]; results
// C[row = 4 (lane >> 4) + i][col = lane & 15].  A position tile is 16 consecutive entries of the FLATTENED (ray, position)
// index over the workgroup's group of G rays: at L = 61 a ray has 14 / 6 positions and a tile spans rays.
//
// Backward (parameter gradients only; rays are data).  Per group: layer 1 again from the staged rays (the same function the
// forward runs, so the same instructions and bits),  dz2 = grad_y (y > 0 ? 1 : slope)  [O2][columns],  dW2 += dz2 patch2^T
// (K = columns), g2 = W2^T dz2 [columns][K2] to LDS, da1 = the col2im gather of g2 (position p receives (q, j) with
// q s2 + j = p, j ascending), dz1 = da1 (a1 > 0 ? 1 : slope), dW1 += dz1 patch1^T, and the bias sums as sliced row sums in a
// fixed order.  The accumulators stay in registers over the groups a workgroup walks; at the end it writes ONE slab of
// param_count floats (w1 | b1 | w2 | b2 in the nn.Conv1d layouts), and a second launch adds the slabs in workgroup order, 16
// slices then the slices: the arithmetic of asac_sum_partials_multi with slices = 16, so a deferred sum gives the same bits.
// Nothing depends on timing: equal inputs give equal bits.
//
// Rays beyond N in the last group: loaded at a clamped index (valid memory, finite values), their dz2 selected to zero, their
// outputs not stored (NOTES.md, "A load under a lane condition is a branch with its own wait").
#include "asac_common.h"

#include <cmath>

namespace asac {

constexpr int kC1Threads = 1024;         // 16 waves, four per SIMD: between the products the work is VALU and latency (measured
                                         // on the layer of tools/ray_bench.py, 256 / 512 / 1024 threads: 220 / 177 / 170 us at L = 400)
constexpr int kC1Waves = kC1Threads / 64;
constexpr size_t kC1LdsLimit = 160 * 1024;
constexpr int kC1FwdBlocks = 1024;      // forward: workgroups walk the groups with this stride
constexpr int kC1BwdBlocks = 256;       // backward: one slab per workgroup, one workgroup per CU
constexpr int kC1TargetCols = 192;      // layer-1 columns a group aims at (12 position tiles)
constexpr int kC1SumSlices = 16;
constexpr int kC1MaxOwn2 = 2;           // dW2 tiles per wave: up to 2 x 16 tiles over 16 waves

typedef float c1_f32x4 __attribute__((ext_vector_type(4)));

struct C1Dims {
    int L, C, O1, k1, s1, O2, k2, s2;
    float slope;
    int L1, L2, K1, K2, MT;             // MT: 16-row tiles of layer-2 channels (1 | 2)
    int G, cols1, cols2, cols1p, cols2p;        // columns of a group; ..p: rounded up to 16
    int W1S, W2S, A1S, K2S, D1S, D2S;   // LDS row strides
    int o_w1, o_b1, o_w2, o_b2, o_x, o_a1, fwd_total;
    int o_dz2, o_g2, o_dz1, o_red, bwd_total;
    // 1 / d in f32 for the index divisions of the hot loops (c1_div)
    float r_L1, r_L2, r_s2, r_cols1p, r_cols2p;
};

struct C1Args {
    C1Dims d;
    const float *x, *w1, *b1, *w2, *b2, *y_in, *gy;
    float* y;
    float* partial;
    int64_t N, n_groups;
};

// a row stride >= n with stride % 8 == 4: 16 rows x 4 consecutive floats then cover all 64 banks once
static inline int c1_stride4(int n) { return (n & 7) == 4 ? n : ((n + 7) & ~7) + 4; }

static bool c1_dims(const asac_conv1_desc_t& c, C1Dims& d) {
    if (c.length < 1 || c.channels < 1 || c.out1 < 1 || c.out2 < 1 || c.kernel1 < 1 || c.kernel2 < 1 || c.stride1 < 1 ||
        c.stride2 < 1)
        return false;
    if (!(c.negative_slope > 0.f) || !std::isfinite(c.negative_slope)) return false;
    if (c.out1 > 16 || c.out2 > 32 || c.length > (1 << 20) || c.channels > 64 || c.kernel1 > 64 || c.kernel2 > 256) return false;
    d.L = c.length; d.C = c.channels; d.O1 = c.out1; d.k1 = c.kernel1; d.s1 = c.stride1;
    d.O2 = c.out2; d.k2 = c.kernel2; d.s2 = c.stride2; d.slope = c.negative_slope;
    d.K1 = d.C * d.k1; d.K2 = d.O1 * d.k2;
    if ((d.K1 & 3) || (d.K2 & 3) || d.K1 > 64 || d.K2 > 256) return false;
    if (d.L < d.k1) return false;
    d.L1 = (d.L - d.k1) / d.s1 + 1;
    if (d.L1 < d.k2) return false;
    d.L2 = (d.L1 - d.k2) / d.s2 + 1;
    d.MT = (d.O2 + 15) / 16;
    d.W1S = c1_stride4(d.K1);
    d.W2S = c1_stride4(d.K2);
    d.K2S = d.K2 + 4;
    // a1s: 16 positions s2 A1S apart, 4 consecutive floats each -> (s2 A1S) % 8 == 4 where some A1S in O1 .. O1 + 7 gives it
    d.A1S = d.O1;
    for (int a = d.O1; a < d.O1 + 8; ++a)
        if (((int64_t)d.s2 * a) % 8 == 4) { d.A1S = a; break; }
    for (int G = (kC1TargetCols + d.L1 - 1) / d.L1; G >= 1; --G) {
        d.G = G;
        d.cols1 = G * d.L1; d.cols2 = G * d.L2;
        d.cols1p = (d.cols1 + 15) & ~15; d.cols2p = (d.cols2 + 15) & ~15;
        d.D1S = d.cols1p + 4; d.D2S = d.cols2p + 4;
        int64_t o = 0;
        auto take = [&](int64_t n) { int64_t at = o; o += (n + 3) & ~(int64_t)3; return at; };
        const int64_t o_w1 = take(16 * d.W1S), o_b1 = take(16), o_w2 = take((int64_t)d.MT * 16 * d.W2S), o_b2 = take(32);
        const int64_t o_x = take((int64_t)G * d.L * d.C), o_a1 = take((int64_t)d.cols1 * d.A1S);
        const int64_t fwd_total = o;
        const int64_t o_dz2 = take((int64_t)d.MT * 16 * d.D2S), o_g2 = take((int64_t)d.cols2p * d.K2S);
        const int64_t o_dz1 = take(16 * (int64_t)d.D1S), o_red = take(2 * kC1Threads);
        if ((size_t)o * sizeof(float) > kC1LdsLimit) continue;
        d.o_w1 = (int)o_w1; d.o_b1 = (int)o_b1; d.o_w2 = (int)o_w2; d.o_b2 = (int)o_b2; d.o_x = (int)o_x; d.o_a1 = (int)o_a1;
        d.fwd_total = (int)fwd_total;
        d.r_L1 = 1.f / (float)d.L1; d.r_L2 = 1.f / (float)d.L2; d.r_s2 = 1.f / (float)d.s2;
        d.r_cols1p = 1.f / (float)d.cols1p; d.r_cols2p = 1.f / (float)d.cols2p;
        d.o_dz2 = (int)o_dz2; d.o_g2 = (int)o_g2; d.o_dz1 = (int)o_dz1; d.o_red = (int)o_red; d.bwd_total = (int)o;
        return true;
    }
    return false;
}

static inline int c1_param_count(const C1Dims& d) { return d.O1 * d.K1 + d.O1 + d.O2 * d.K2 + d.O2; }

// t / d for 0 <= t < 2^20 with r = 1.f / d: (t + 0.5) / d lies at least 0.5 / d from an integer, the f32 product is off by
// less than 2^-22 of its value, which is < 0.5 / d while t < 2^20 — a few VALU instructions for the ~40 of an integer division.
// Every index divided here is below the LDS budget's 40 960 floats.
__device__ __forceinline__ int c1_div(int t, float r) { return (int)(((float)t + 0.5f) * r); }

__device__ __forceinline__ float c1_leaky(float z, float slope) { return z > 0.f ? z : z * slope; }

// the four parameter tensors, re-indexed to the patch order and zero-padded to whole tiles
__device__ __forceinline__ void c1_stage_weights(const C1Args& a, float* lds) {
    const C1Dims& d = a.d;
    float* w1s = lds + d.o_w1;
    for (int i = threadIdx.x; i < 16 * d.W1S; i += kC1Threads) {
        const int o = i / d.W1S, k = i - o * d.W1S;
        const bool ok = o < d.O1 && k < d.K1;
        const int j = k / d.C, c = k - j * d.C;
        const float v = a.w1[ok ? (o * d.C + c) * d.k1 + j : 0];
        w1s[i] = ok ? v : 0.f;
    }
    float* w2s = lds + d.o_w2;
    for (int i = threadIdx.x; i < d.MT * 16 * d.W2S; i += kC1Threads) {
        const int o = i / d.W2S, k = i - o * d.W2S;
        const bool ok = o < d.O2 && k < d.K2;
        const int j = k / d.O1, c = k - j * d.O1;
        const float v = a.w2[ok ? (o * d.O1 + c) * d.k2 + j : 0];
        w2s[i] = ok ? v : 0.f;
    }
    if (threadIdx.x < 16) {
        const float v = a.b1[min((int)threadIdx.x, d.O1 - 1)];
        lds[d.o_b1 + threadIdx.x] = (int)threadIdx.x < d.O1 ? v : 0.f;
    }
    if (threadIdx.x >= 64 && threadIdx.x < 96) {
        const int o = threadIdx.x - 64;
        const float v = a.b2 ? a.b2[min(o, d.O2 - 1)] : 0.f;
        lds[d.o_b2 + o] = o < d.O2 ? v : 0.f;
    }
}

// the rays of group `g` as stored; rays beyond N repeat the tensor's last floats (finite, never stored anywhere)
__device__ __forceinline__ void c1_stage_rays(const C1Args& a, float* lds, int64_t g) {
    const C1Dims& d = a.d;
    const int64_t ray = (int64_t)d.L * d.C, base = g * d.G * ray, last = a.N * ray - 1;
    float* xs = lds + d.o_x;
    const int n = d.G * (int)ray;
    for (int i = threadIdx.x; i < n; i += kC1Threads) xs[i] = a.x[min(base + i, last)];
}

// a1s <- LeakyReLU(W1 patch + b1) for the group's cols1 columns
__device__ __forceinline__ void c1_layer1(const C1Dims& d, float* lds, int wave, int lane) {
    const float* w1s = lds + d.o_w1;
    const float* b1s = lds + d.o_b1;
    const float* xs = lds + d.o_x;
    float* a1s = lds + d.o_a1;
    const int kq = lane >> 4, ln = lane & 15;
    const int tiles = (d.cols1 + 15) >> 4;
    const float* wp = w1s + ln * d.W1S + kq;
    for (int t = wave; t < tiles; t += kC1Waves) {
        const int col = t * 16 + ln, cc = min(col, d.cols1 - 1);
        const int r = c1_div(cc, d.r_L1), p = cc - r * d.L1;
        const float* xp = xs + (r * d.L + p * d.s1) * d.C + kq;
        c1_f32x4 acc;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = b1s[kq * 4 + i];
        for (int k0 = 0; k0 < d.K1; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[k0], xp[k0], acc, 0, 0, 0);
        if (col < d.cols1) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (kq * 4 + i < d.O1) a1s[col * d.A1S + kq * 4 + i] = c1_leaky(acc[i], d.slope);
        }
    }
}

__global__ __launch_bounds__(kC1Threads) void k_conv1_fwd(const C1Args a) {
    extern __shared__ float lds[];
    const C1Dims& d = a.d;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, ln = lane & 15;
    c1_stage_weights(a, lds);
    const float* w2s = lds + d.o_w2;
    const float* b2s = lds + d.o_b2;
    const float* a1s = lds + d.o_a1;
    const int tiles2 = (d.cols2 + 15) >> 4;
    const int64_t out = (int64_t)d.O2 * d.L2;
    for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        c1_stage_rays(a, lds, g);
        __syncthreads();
        c1_layer1(d, lds, wave, lane);
        __syncthreads();
        const float* wp = w2s + ln * d.W2S + kq;
        for (int t = wave; t < tiles2; t += kC1Waves) {
            const int col = t * 16 + ln, cc = min(col, d.cols2 - 1);
            const int r = c1_div(cc, d.r_L2), q = cc - r * d.L2;
            const float* ap = a1s + (r * d.L1 + q * d.s2) * d.A1S;
            int j = kq / d.O1, c = kq - j * d.O1;
            c1_f32x4 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc0[i] = b2s[kq * 4 + i];
                acc1[i] = b2s[16 + kq * 4 + i];
            }
            for (int k0 = 0; k0 < d.K2; k0 += 4) {
                const float b = ap[j * d.A1S + c];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[k0], b, acc0, 0, 0, 0);
                if (d.MT > 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[16 * d.W2S + k0], b, acc1, 0, 0, 0);
                c += 4;
                while (c >= d.O1) { c -= d.O1; ++j; }
            }
            const int64_t n = g * d.G + r;
            if (col < d.cols2 && n < a.N) {
                float* yp = a.y + n * out + q;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = kq * 4 + i;
                    if (o < d.O2) yp[(int64_t)o * d.L2] = c1_leaky(acc0[i], d.slope);
                    if (o + 16 < d.O2) yp[(int64_t)(o + 16) * d.L2] = c1_leaky(acc1[i], d.slope);
                }
            }
        }
        // (the next group's rays overwrite xs, which nobody reads after the barrier above; its layer 1 writes a1s only after
        // the barrier behind the staging, which every wave reaches after its layer-2 reads)
    }
}

// this thread's share of the row sums of src [rows][stride] over `cols` columns: row = tid % rows_pad, a contiguous slice of
// the columns per tid / rows_pad; red[tid] <- the share.  The caller adds red[row], red[rows_pad + row], .. in that order.
__device__ __forceinline__ void c1_row_sum_shares(const float* src, int stride, int rows_alloc, int rows_pad, int cols,
                                                  float* red) {
    const int row = threadIdx.x % rows_pad, part = threadIdx.x / rows_pad, parts = kC1Threads / rows_pad;
    const int per = (cols + parts - 1) / parts;
    const int lo = part * per, hi = min(lo + per, cols);
    float s = 0.f;
    if (row < rows_alloc)
        for (int c = lo; c < hi; ++c) s += src[row * stride + c];
    red[threadIdx.x] = s;
}

__global__ __launch_bounds__(kC1Threads) void k_conv1_bwd(const C1Args a) {
    extern __shared__ float lds[];
    const C1Dims& d = a.d;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, ln = lane & 15;
    c1_stage_weights(a, lds);
    const float* w2s = lds + d.o_w2;
    const float* xs = lds + d.o_x;
    const float* a1s = lds + d.o_a1;
    float* dz2s = lds + d.o_dz2;
    float* g2s = lds + d.o_g2;
    float* dz1s = lds + d.o_dz1;
    float* red = lds + d.o_red;
    const int64_t out = (int64_t)d.O2 * d.L2, out_last = a.N * out - 1;

    // dW2: tiles (nt over K2, m over the channel tiles), tile id nt MT + m, this wave owns ids wave, wave + kC1Waves, ..
    const int nt2 = (d.K2 + 15) >> 4, tiles_w2 = nt2 * d.MT;
    c1_f32x4 acc_w2[kC1MaxOwn2];
    int off2[kC1MaxOwn2];
#pragma unroll
    for (int u = 0; u < kC1MaxOwn2; ++u) {
        acc_w2[u] = c1_f32x4{0.f, 0.f, 0.f, 0.f};
        const int ti = wave + kC1Waves * u, nt = ti / d.MT;
        const int kk = min(nt * 16 + ln, d.K2 - 1);
        const int j = kk / d.O1;
        off2[u] = j * d.A1S + (kk - j * d.O1);
    }
    // dW1: one tile of 16 patch entries per wave (K1 <= 64)
    const int nt1 = (d.K1 + 15) >> 4;
    c1_f32x4 acc_w1 = c1_f32x4{0.f, 0.f, 0.f, 0.f};
    const int kk1 = min(wave * 16 + ln, d.K1 - 1);
    float db1 = 0.f, db2 = 0.f;         // threads < 16 / < 32

    for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        c1_stage_rays(a, lds, g);
        // dz2 [MT 16][cols2p] = grad_y (y > 0 ? 1 : slope); rows beyond O2, columns beyond cols2 and rays beyond N: zero
        for (int i = threadIdx.x; i < d.MT * 16 * d.cols2p; i += kC1Threads) {
            const int o = c1_div(i, d.r_cols2p), col = i - o * d.cols2p;
            const int r = c1_div(col, d.r_L2), q = col - r * d.L2;
            const int64_t n = g * d.G + r;
            const bool ok = o < d.O2 && col < d.cols2 && n < a.N;
            const int64_t at = min(n * out + (int64_t)o * d.L2 + q, out_last);
            const float yv = a.y_in[at], gv = a.gy[at];
            dz2s[o * d.D2S + col] = ok ? gv * (yv > 0.f ? 1.f : d.slope) : 0.f;
        }
        __syncthreads();
        c1_layer1(d, lds, wave, lane);
        __syncthreads();

        // dW2 += dz2 patch2^T over the group's columns
        for (int c0 = 0; c0 < d.cols2p; c0 += 4) {
            const int col = min(c0 + kq, d.cols2 - 1);
            const int r = c1_div(col, d.r_L2), q = col - r * d.L2;
            const float* ap = a1s + (r * d.L1 + q * d.s2) * d.A1S;
#pragma unroll
            for (int u = 0; u < kC1MaxOwn2; ++u) {
                const int ti = wave + kC1Waves * u;
                if (ti < tiles_w2) {
                    const int m = ti % d.MT;
                    const float av = dz2s[(m * 16 + ln) * d.D2S + c0 + kq];
                    acc_w2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ap[off2[u]], acc_w2[u], 0, 0, 0);
                }
            }
        }
        // g2 [cols2p][K2] = W2^T dz2
        {
            const int t2n = d.cols2p >> 4;
            for (int f = wave; f < nt2 * t2n; f += kC1Waves) {
                const int kt = f % nt2, t2 = f / nt2;
                const int kc = min(kt * 16 + ln, d.K2 - 1);
                c1_f32x4 acc = c1_f32x4{0.f, 0.f, 0.f, 0.f};
                for (int o0 = 0; o0 < d.MT * 16; o0 += 4)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2s[(o0 + kq) * d.W2S + kc], dz2s[(o0 + kq) * d.D2S + t2 * 16 + ln],
                                                               acc, 0, 0, 0);
                const int col = t2 * 16 + ln;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = kt * 16 + kq * 4 + i;
                    if (k < d.K2) g2s[col * d.K2S + k] = acc[i];
                }
            }
        }
        c1_row_sum_shares(dz2s, d.D2S, d.MT * 16, 32, d.cols2, red);
        __syncthreads();
        if (threadIdx.x < 32) {
            float s = 0.f;
            for (int part = 0; part < kC1Threads / 32; ++part) s += red[part * 32 + threadIdx.x];
            db2 += s;
        }
        // dz1 [16][cols1p] = (col2im gather of g2) (a1 > 0 ? 1 : slope); rows beyond O1 and columns beyond cols1: zero
        for (int i = threadIdx.x; i < 16 * d.cols1p; i += kC1Threads) {
            const int c = c1_div(i, d.r_cols1p), col = i - c * d.cols1p;
            float v = 0.f;
            if (c < d.O1 && col < d.cols1) {
                const int r = c1_div(col, d.r_L1), p = col - r * d.L1;
                float s = 0.f;
                for (int j = 0; j < d.k2; ++j) {
                    const int t = p - j;
                    if (t < 0) break;
                    const int q = c1_div(t, d.r_s2);
                    if (q * d.s2 == t && q < d.L2) s += g2s[(r * d.L2 + q) * d.K2S + j * d.O1 + c];
                }
                v = s * (a1s[col * d.A1S + c] > 0.f ? 1.f : d.slope);
            }
            dz1s[c * d.D1S + col] = v;
        }
        __syncthreads();
        // dW1 += dz1 patch1^T over the group's columns
        if (wave < nt1) {
            for (int c0 = 0; c0 < d.cols1p; c0 += 4) {
                const int col = min(c0 + kq, d.cols1 - 1);
                const int r = c1_div(col, d.r_L1), p = col - r * d.L1;
                const float bv = xs[(r * d.L + p * d.s1) * d.C + kk1];
                acc_w1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dz1s[ln * d.D1S + c0 + kq], bv, acc_w1, 0, 0, 0);
            }
        }
        c1_row_sum_shares(dz1s, d.D1S, 16, 16, d.cols1, red + kC1Threads);
        __syncthreads();
        if (threadIdx.x < 16) {
            float s = 0.f;
            for (int part = 0; part < kC1Threads / 16; ++part) s += red[kC1Threads + part * 16 + threadIdx.x];
            db1 += s;
        }
        // (the barrier above also ends this group's reads of xs, a1s, dz1s and g2s; the next group's first writes to dz2s
        // come after every wave's dW2 / g2 reads, which lie two barriers back)
    }

    // this workgroup's slab: w1 | b1 | w2 | b2 in the nn.Conv1d layouts
    float* slab = a.partial + (int64_t)blockIdx.x * (d.O1 * d.K1 + d.O1 + d.O2 * d.K2 + d.O2);
    if (wave < nt1) {
        const int kk = wave * 16 + ln;
        const int j = kk / d.C, ci = kk - j * d.C;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = kq * 4 + i;
            if (c < d.O1 && kk < d.K1) slab[(c * d.C + ci) * d.k1 + j] = acc_w1[i];
        }
    }
    if ((int)threadIdx.x < d.O1) slab[d.O1 * d.K1 + threadIdx.x] = db1;
    float* slab_w2 = slab + d.O1 * d.K1 + d.O1;
#pragma unroll
    for (int u = 0; u < kC1MaxOwn2; ++u) {
        const int ti = wave + kC1Waves * u;
        if (ti < tiles_w2) {
            const int m = ti % d.MT, nt = ti / d.MT;
            const int kk = nt * 16 + ln;
            const int j = kk / d.O1, c = kk - j * d.O1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = m * 16 + kq * 4 + i;
                if (o < d.O2 && kk < d.K2) slab_w2[(o * d.O1 + c) * d.k2 + j] = acc_w2[u][i];
            }
        }
    }
    if ((int)threadIdx.x < d.O2) slab_w2[d.O2 * d.K2 + threadIdx.x] = db2;
}

// sum of the workgroups' slabs in fixed order (64 parameters per workgroup, 16 slices of slabs, then the slices): the additions
// of asac_sum_partials_multi with slices = 16
__global__ __launch_bounds__(64 * kC1SumSlices) void k_conv1_sum_partials(const float* __restrict__ partial, int blocks,
                                                                          int n, float* __restrict__ out, int accumulate) {
    __shared__ float part[kC1SumSlices][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const int per = (blocks + kC1SumSlices - 1) / kC1SumSlices;
    const int lo = sl * per, hi = min(lo + per, blocks);
    float s = 0.f;
    if (i < n)
        for (int bk = lo; bk < hi; ++bk) s += partial[(int64_t)bk * n + i];
    part[sl][lane] = s;
    __syncthreads();
    if (sl != 0 || i >= n) return;
    s = 0.f;
#pragma unroll
    for (int w = 0; w < kC1SumSlices; ++w) s += part[w][lane];
    out[i] = accumulate ? out[i] + s : s;
}

static int c1_lds_limit(const void* fn, bool& done, const char* where) {
    if (done) return 0;
    hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kC1LdsLimit);
    if (err != hipSuccess) {
        set_error(err, where);
        return (int)err;
    }
    done = true;
    return 0;
}

static inline int64_t c1_groups(const C1Dims& d, int64_t N) { return (N + d.G - 1) / d.G; }

}  // namespace asac

using namespace asac;

extern "C" {

int asac_conv1_supported(const asac_conv1_desc_t* desc) {
    C1Dims d;
    return desc && c1_dims(*desc, d) ? 1 : 0;
}

int64_t asac_conv1_param_count(const asac_conv1_desc_t* desc) {
    C1Dims d;
    if (!desc || !c1_dims(*desc, d)) return -1;
    return c1_param_count(d);
}

int asac_conv1_backward_slabs(const asac_conv1_desc_t* desc, int64_t N) {
    C1Dims d;
    if (!desc || !c1_dims(*desc, d) || N <= 0) return -1;
    const int64_t groups = c1_groups(d, N);
    return (int)(groups < kC1BwdBlocks ? groups : kC1BwdBlocks);
}

int64_t asac_conv1_backward_workspace(const asac_conv1_desc_t* desc, int64_t N) {
    C1Dims d;
    if (!desc || !c1_dims(*desc, d) || N <= 0) return -1;
    return (int64_t)asac_conv1_backward_slabs(desc, N) * c1_param_count(d);
}

int asac_conv1_forward(const asac_conv1_desc_t* desc, const float* x, int64_t N, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* y, float* a1_out, void* stream) {
    C1Args a{};
    if (!desc || !c1_dims(*desc, a.d) || N <= 0 || !x || !w1 || !b1 || !w2 || !b2 || !y || a1_out)
        return bad_arg("asac_conv1_forward");
    a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.y = y;
    a.N = N;
    a.n_groups = c1_groups(a.d, N);
    static bool attr = false;
    if (int rc = c1_lds_limit(reinterpret_cast<const void*>(k_conv1_fwd), attr, "asac_conv1_forward")) return rc;
    const unsigned blocks = (unsigned)(a.n_groups < kC1FwdBlocks ? a.n_groups : kC1FwdBlocks);
    ASAC_LAUNCH(k_conv1_fwd, dim3(blocks), dim3(kC1Threads), (size_t)a.d.fwd_total * sizeof(float), as_stream(stream), a);
    return finish_launch("asac_conv1_forward");
}

int asac_conv1_backward(const asac_conv1_desc_t* desc, const float* x, int64_t N, const float* w1, const float* b1,
                        const float* w2, const float* y, const float* a1, const float* grad_y, float* grad_params,
                        int accumulate, float* workspace, void* stream) {
    C1Args a{};
    if (!desc || !c1_dims(*desc, a.d) || N <= 0 || !x || !w1 || !b1 || !w2 || !y || a1 || !grad_y || !grad_params ||
        !workspace || accumulate < 0 || accumulate > ASAC_CONV_SUM_DEFER)
        return bad_arg("asac_conv1_backward");
    a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = nullptr; a.y_in = y; a.gy = grad_y;
    a.partial = workspace;
    a.N = N;
    a.n_groups = c1_groups(a.d, N);
    static bool attr = false;
    if (int rc = c1_lds_limit(reinterpret_cast<const void*>(k_conv1_bwd), attr, "asac_conv1_backward")) return rc;
    const unsigned blocks = (unsigned)(a.n_groups < kC1BwdBlocks ? a.n_groups : kC1BwdBlocks);
    hipStream_t s = as_stream(stream);
    ASAC_LAUNCH(k_conv1_bwd, dim3(blocks), dim3(kC1Threads), (size_t)a.d.bwd_total * sizeof(float), s, a);
    const int n = c1_param_count(a.d);
    // launched once (not under the repeat knob: it may accumulate); ASAC_CONV_SUM_DEFER: left to asac_sum_partials_multi
    if (accumulate != ASAC_CONV_SUM_DEFER)
        hipLaunchKernelGGL(k_conv1_sum_partials, dim3((unsigned)((n + 63) / 64)), dim3(64 * kC1SumSlices), 0, s, workspace,
                           (int)blocks, n, grad_params, accumulate);
    return finish_launch("asac_conv1_backward");
}

}  // extern "C"
