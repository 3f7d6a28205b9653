// The gate an episode attention block puts BEHIND its attention (`EpisodeMultiheadAttentionBlock.forward`, reference
// algorithm/nn_models/layers/seq_layers.py:460-547, with the gate layers of 297-345), over the rows of a batch of sampled
// windows, with the padded-row factor folded in — ONE launch forward, ONE backward, next to csrc/rows_proj.hip:
//   x = the residual source [B][Lq][E] (the newest Lq positions of the block's input: read through its strides),
//   y = the attention output (dense), s = 1 - row_zero[b][t] (the caller's padded positions; NULL: 1)
//   * RESIDUAL   out = (x + y) s                                               (an add, a not, a cast and a multiply)
//   * OUTPUT     a = x W^T;  out = (x + sigmoid(a * y)) s                      (a GEMM and six elementwise launches)
//   * RECURRENT  r = sigmoid(x Wxr^T + y Wyr^T);  z = sigmoid(x Wxz^T + y Wyz^T + bz);  h = tanh(y Wyg^T + (r * x) Wxg^T)
//                out = ((1 - z) x + z h) s                                     (GTrXL: six GEMMs and ~a dozen elementwise)
// Backward: g = grad_out s, then
//   * RESIDUAL   grad_x = grad_y = g
//   * OUTPUT     p = sigmoid(a y);  d = g p (1 - p);  grad_y = d a;  grad_a = d y (dense: grad_a^T x is the weight gradient);
//                grad_x = g + grad_a W
//   * RECURRENT  dz_pre = g (h - x) z (1 - z);  dh_pre = g z (1 - h^2);  q = dh_pre Wxg;  dr_pre = q x r (1 - r);
//                grad_x = (g (1 - z) + q r) + (dr_pre Wxr + dz_pre Wxz);  grad_y = dr_pre Wyr + dz_pre Wyz + dh_pre Wyg;
//                dr_pre, dz_pre, dh_pre and r * x are written densely: the six weight gradients are their products over
//                the rows with x, y and r * x, the bias gradient the column sums of dz_pre (csrc/xty.hip).
// Order of the sums: a product runs over the input features in ascending blocks of 16 (inside a block: the MFMA's order), the
// lower and the upper half of the features in an accumulator each (E = 32: one), lower + upper; where several products feed
// one result, each is formed on its own and they are added in the order written above, left to right (the module's own
// association: dense_x(x) + dense_y(y)); the elementwise terms are added as bracketed above.  Independent accumulators are
// both the shorter rounding chain and the shorter dependent MFMA chain.
//
// A workgroup (4 waves) owns 16 rows, wave w the feature tiles w, w + 4, ...; the rows are the N dimension of the MFMA, the
// weights the A operand read where they lie (forward 16 bytes of a weight row, backward four strided words of a column), as
// in rows_proj.hip.  RECURRENT: the candidate needs the WHOLE row of r * x (backward: of dr_pre), of which a wave holds its
// own tiles only — the tile goes through LDS (16 rows x (E + 4) floats, the pad spreads the rows over the banks) behind one
// workgroup barrier.  Weights and rows are L2-resident; the launches are latency, not bandwidth.
#include "asac_common.h"

namespace asac {
namespace rowsg {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kResidual = 1, kOutput = 2, kRecurrent = 3;      // GATE.RESIDUAL / OUTPUT / RECURRENT
constexpr int kMaxW = 6, kMaxSaved = 3;

#define RG_MF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 mfma4(const f32x4 a, const f32x4 b, f32x4 c) {
    c = RG_MF(a[0], b[0], c);
    c = RG_MF(a[1], b[1], c);
    c = RG_MF(a[2], b[2], c);
    c = RG_MF(a[3], b[3], c);
    return c;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

struct GateArgs {
    const float* x; int64_t xs_b, xs_t;      // x[b][t][E] (feature stride 1)
    const float* y;                          // [B][L][E] dense
    const uint8_t* rz; int64_t rz_sb;        // [B][L] (position stride 1) or NULL
    int32_t B, L;
    const float* w[kMaxW];                   // [E][E] (nn.Linear layout: out x in)
    const float* bz;                         // [E]
    float* out;                              // forward
    float* sv[kMaxSaved];                    // forward: written (may be NULL); backward: read
    const float* go;                         // backward: gradient of out, dense
    float* gx; float* gy;                    // dense
    float* gp[kMaxSaved];                    // pre-activation gradients, dense
    float* rx;                               // r * x, dense
};

// four strided words of a weight column block: W[n0 + s][k] for s < 4
template <int E>
__device__ __forceinline__ f32x4 wcol4(const float* w, int n0, int k) {
    f32x4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = w[(n0 + s) * E + k];
    return v;
}

// (16 features of tile nt of) v W^T, v = the row operand held as EC chunks: the lower and the upper half of the input features
// in an accumulator each
template <int EC>
__device__ __forceinline__ f32x4 fwd_product(const float* w, int nt, int x, int q, const f32x4 (&v)[EC]) {
    constexpr int H = EC >= 4 ? EC / 2 : EC;
    const float* wp = w + (16 * nt + x) * (16 * EC) + 4 * q;
    f32x4 wa[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) wa[c] = ld4(wp + 16 * c);
    f32x4 lo = zero4(), hi = zero4();
#pragma unroll
    for (int c = 0; c < H; ++c) lo = mfma4(wa[c], v[c], lo);
#pragma unroll
    for (int c = H; c < EC; ++c) hi = mfma4(wa[c], v[c], hi);
    return H < EC ? lo + hi : lo;
}

// (16 features of tile kt of) v W, likewise
template <int EC>
__device__ __forceinline__ f32x4 bwd_product(const float* w, int kt, int x, int q, const f32x4 (&v)[EC]) {
    constexpr int H = EC >= 4 ? EC / 2 : EC;
    f32x4 lo = zero4(), hi = zero4();
#pragma unroll
    for (int c = 0; c < H; ++c) lo = mfma4(wcol4<16 * EC>(w, 16 * c + 4 * q, 16 * kt + x), v[c], lo);
#pragma unroll
    for (int c = H; c < EC; ++c) hi = mfma4(wcol4<16 * EC>(w, 16 * c + 4 * q, 16 * kt + x), v[c], hi);
    return H < EC ? lo + hi : lo;
}

struct RowPos {
    int64_t row, rc;      // the lane's row, and the row it reads (clamped: a lane past the end reads the last row, stores nothing)
    bool live;
    const float* xp;      // x row + 4 q
    float s;
};

__device__ __forceinline__ RowPos row_pos(const GateArgs& a, int x, int q) {
    RowPos p;
    const int64_t rows = (int64_t)a.B * a.L;
    p.row = (int64_t)blockIdx.x * 16 + x;
    p.live = p.row < rows;
    p.rc = p.live ? p.row : rows - 1;
    const int b = (int)(p.rc / a.L), t = (int)(p.rc - (int64_t)b * a.L);
    p.xp = a.x + b * a.xs_b + t * a.xs_t + 4 * q;
    p.s = (a.rz && a.rz[b * a.rz_sb + t]) ? 0.f : 1.f;
    return p;
}

// RESIDUAL, both passes: 16 rows x E / 4 vectors per workgroup
template <int EC, bool BWD>
__global__ void __launch_bounds__(kThreads) k_gate_residual(const GateArgs a) {
    constexpr int E = 16 * EC, V = E / 4;
    const int64_t rows = (int64_t)a.B * a.L;
    for (int i = threadIdx.x; i < 16 * V; i += kThreads) {
        const int64_t row = (int64_t)blockIdx.x * 16 + i / V;
        if (row >= rows) continue;
        const int col = 4 * (i % V);
        const int b = (int)(row / a.L), t = (int)(row - (int64_t)b * a.L);
        const float s = (a.rz && a.rz[b * a.rz_sb + t]) ? 0.f : 1.f;
        if (BWD) {
            const f32x4 g = ld4(a.go + row * E + col) * s;
            st4(a.gx + row * E + col, g);
            if (a.gy != a.gx) st4(a.gy + row * E + col, g);
        } else {
            st4(a.out + row * E + col, (ld4(a.x + b * a.xs_b + t * a.xs_t + col) + ld4(a.y + row * E + col)) * s);
        }
    }
}

template <int EC>
__global__ void __launch_bounds__(kThreads) k_gate_output_fwd(const GateArgs a) {
    constexpr int E = 16 * EC;
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const RowPos p = row_pos(a, x, q);
    f32x4 xv[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) xv[c] = ld4(p.xp + 16 * c);
    for (int nt = wv; nt < EC; nt += kWaves) {
        const f32x4 av = fwd_product<EC>(a.w[0], nt, x, q, xv);      // av[r] = a[row x][16 nt + 4 q + r]
        const f32x4 xt = ld4(p.xp + 16 * nt), yt = ld4(a.y + p.rc * E + 16 * nt + 4 * q);
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (xt[r] + sigmoid_f(av[r] * yt[r])) * p.s;
        if (p.live) {
            st4(a.out + p.row * E + 16 * nt + 4 * q, o);
            if (a.sv[0]) st4(a.sv[0] + p.row * E + 16 * nt + 4 * q, av);
        }
    }
}

template <int EC>
__global__ void __launch_bounds__(kThreads) k_gate_output_bwd(const GateArgs a) {
    constexpr int E = 16 * EC;
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const RowPos p = row_pos(a, x, q);
    const float* gop = a.go + p.rc * E + 4 * q;
    const float* ap = a.sv[0] + p.rc * E + 4 * q;
    const float* yp = a.y + p.rc * E + 4 * q;
    f32x4 ga[EC];      // grad_a of the lane's row, all features
#pragma unroll
    for (int c = 0; c < EC; ++c) {
        const f32x4 g = ld4(gop + 16 * c) * p.s, av = ld4(ap + 16 * c), yv = ld4(yp + 16 * c);
        f32x4 gy;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sg = sigmoid_f(av[r] * yv[r]);
            const float d = g[r] * (sg * (1.f - sg));
            gy[r] = d * av[r];
            ga[c][r] = d * yv[r];
        }
        if (p.live && (c & (kWaves - 1)) == wv) {
            st4(a.gy + p.row * E + 16 * c + 4 * q, gy);
            st4(a.gp[0] + p.row * E + 16 * c + 4 * q, ga[c]);
        }
    }
    for (int kt = wv; kt < EC; kt += kWaves) {
        const f32x4 acc = bwd_product<EC>(a.w[0], kt, x, q, ga);
        if (p.live) st4(a.gx + p.row * E + 16 * kt + 4 * q, ld4(gop + 16 * kt) * p.s + acc);
    }
}

template <int EC>
__global__ void __launch_bounds__(kThreads) k_gate_recurrent_fwd(const GateArgs a) {
    constexpr int E = 16 * EC, LS = E + 4, NT = (EC + kWaves - 1) / kWaves;
    __shared__ __attribute__((aligned(16))) float s_rx[16 * LS];
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const RowPos p = row_pos(a, x, q);
    f32x4 xv[EC], yv[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) xv[c] = ld4(p.xp + 16 * c), yv[c] = ld4(a.y + p.rc * E + 4 * q + 16 * c);
    f32x4 zt[NT], hp[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int nt = wv + kWaves * i;
        if (nt >= EC) continue;
        const f32x4 ar = fwd_product<EC>(a.w[0], nt, x, q, xv) + fwd_product<EC>(a.w[1], nt, x, q, yv);
        const f32x4 az = (fwd_product<EC>(a.w[2], nt, x, q, xv) + fwd_product<EC>(a.w[3], nt, x, q, yv)) + ld4(a.bz + 16 * nt + 4 * q);
        hp[i] = fwd_product<EC>(a.w[5], nt, x, q, yv);
        const f32x4 xt = ld4(p.xp + 16 * nt);
        f32x4 rt, rx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rt[r] = sigmoid_f(ar[r]);
            rx[r] = rt[r] * xt[r];
            zt[i][r] = sigmoid_f(az[r]);
        }
        st4(s_rx + x * LS + 16 * nt + 4 * q, rx);
        if (p.live && a.sv[0]) st4(a.sv[0] + p.row * E + 16 * nt + 4 * q, rt);
    }
    __syncthreads();      // the whole row of r * x, from the four waves' tiles
    f32x4 rxv[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) rxv[c] = ld4(s_rx + x * LS + 16 * c + 4 * q);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int nt = wv + kWaves * i;
        if (nt >= EC) continue;
        const f32x4 ah = hp[i] + fwd_product<EC>(a.w[4], nt, x, q, rxv);
        const f32x4 xt = ld4(p.xp + 16 * nt);
        f32x4 ht, o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ht[r] = tanhf(ah[r]);
            o[r] = ((1.f - zt[i][r]) * xt[r] + zt[i][r] * ht[r]) * p.s;
        }
        if (p.live) {
            st4(a.out + p.row * E + 16 * nt + 4 * q, o);
            if (a.sv[1]) st4(a.sv[1] + p.row * E + 16 * nt + 4 * q, zt[i]);
            if (a.sv[2]) st4(a.sv[2] + p.row * E + 16 * nt + 4 * q, ht);
        }
    }
}

template <int EC>
__global__ void __launch_bounds__(kThreads) k_gate_recurrent_bwd(const GateArgs a) {
    constexpr int E = 16 * EC, LS = E + 4, NT = (EC + kWaves - 1) / kWaves;
    __shared__ __attribute__((aligned(16))) float s_dr[16 * LS];
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, q = l >> 4, x = l & 15;
    const RowPos p = row_pos(a, x, q);
    const float* gop = a.go + p.rc * E + 4 * q;
    const float* rp = a.sv[0] + p.rc * E + 4 * q;
    const float* zp = a.sv[1] + p.rc * E + 4 * q;
    const float* hp = a.sv[2] + p.rc * E + 4 * q;
    f32x4 dz[EC], dh[EC];      // dz_pre, dh_pre of the lane's row, all features
#pragma unroll
    for (int c = 0; c < EC; ++c) {
        const f32x4 g = ld4(gop + 16 * c) * p.s, zv = ld4(zp + 16 * c), hv = ld4(hp + 16 * c), xc = ld4(p.xp + 16 * c);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dz[c][r] = (g[r] * (hv[r] - xc[r])) * (zv[r] * (1.f - zv[r]));
            dh[c][r] = (g[r] * zv[r]) * (1.f - hv[r] * hv[r]);
        }
        if (p.live && (c & (kWaves - 1)) == wv) {
            st4(a.gp[1] + p.row * E + 16 * c + 4 * q, dz[c]);
            st4(a.gp[2] + p.row * E + 16 * c + 4 * q, dh[c]);
        }
    }
    f32x4 part[NT];            // g (1 - z) + q r of the wave's tiles
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int kt = wv + kWaves * i;
        if (kt >= EC) continue;
        const f32x4 qv = bwd_product<EC>(a.w[4], kt, x, q, dh);      // qv[r] = (dh_pre Wxg)[row x][16 kt + 4 q + r]
        const f32x4 g = ld4(gop + 16 * kt) * p.s, rt = ld4(rp + 16 * kt), zv = ld4(zp + 16 * kt), xt = ld4(p.xp + 16 * kt);
        f32x4 dr, rx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dr[r] = (qv[r] * xt[r]) * (rt[r] * (1.f - rt[r]));
            rx[r] = rt[r] * xt[r];
            part[i][r] = g[r] * (1.f - zv[r]) + qv[r] * rt[r];
        }
        st4(s_dr + x * LS + 16 * kt + 4 * q, dr);
        if (p.live) {
            st4(a.gp[0] + p.row * E + 16 * kt + 4 * q, dr);
            st4(a.rx + p.row * E + 16 * kt + 4 * q, rx);
        }
    }
    __syncthreads();      // the whole row of dr_pre
    f32x4 dr[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) dr[c] = ld4(s_dr + x * LS + 16 * c + 4 * q);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int kt = wv + kWaves * i;
        if (kt >= EC) continue;
        const f32x4 ax = bwd_product<EC>(a.w[0], kt, x, q, dr) + bwd_product<EC>(a.w[2], kt, x, q, dz);
        const f32x4 ay = (bwd_product<EC>(a.w[1], kt, x, q, dr) + bwd_product<EC>(a.w[3], kt, x, q, dz)) +
                         bwd_product<EC>(a.w[5], kt, x, q, dh);
        if (p.live) {
            st4(a.gx + p.row * E + 16 * kt + 4 * q, part[i] + ax);
            st4(a.gy + p.row * E + 16 * kt + 4 * q, ay);
        }
    }
}

inline bool width_ok(int E) { return E == 32 || E == 64 || E == 128; }
inline bool kind_ok(int kind) { return kind == kResidual || kind == kOutput || kind == kRecurrent; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int n_weights(int kind) { return kind == kOutput ? 1 : kind == kRecurrent ? 6 : 0; }
inline int n_saved(int kind) { return kind == kOutput ? 1 : kind == kRecurrent ? 3 : 0; }

}  // namespace rowsg
}  // namespace asac

using namespace asac;
using namespace asac::rowsg;

#define RG_LAUNCH(kernel, E, grid, stream, args)                                                    \
    do {                                                                                            \
        if ((E) == 32) ASAC_LAUNCH(kernel<2>, grid, dim3(kThreads), 0, stream, args);               \
        else if ((E) == 64) ASAC_LAUNCH(kernel<4>, grid, dim3(kThreads), 0, stream, args);          \
        else ASAC_LAUNCH(kernel<8>, grid, dim3(kThreads), 0, stream, args);                         \
    } while (0)
#define RG_LAUNCH2(kernel, flag, E, grid, stream, args)                                             \
    do {                                                                                            \
        if ((E) == 32) ASAC_LAUNCH((kernel<2, flag>), grid, dim3(kThreads), 0, stream, args);       \
        else if ((E) == 64) ASAC_LAUNCH((kernel<4, flag>), grid, dim3(kThreads), 0, stream, args);  \
        else ASAC_LAUNCH((kernel<8, flag>), grid, dim3(kThreads), 0, stream, args);                 \
    } while (0)

// the checks both passes share: operands, strides, the kind's weights
static bool gate_common(GateArgs& a, int kind, const float* x, int64_t x_stride_b, int64_t x_stride_t, const float* y,
                        const uint8_t* row_zero, int64_t row_zero_stride_b, int batch, int window, int width,
                        const float* const* weights) {
    if (!kind_ok(kind) || !width_ok(width) || batch <= 0 || window <= 0 || !x || !y || !aligned16(x) || !aligned16(y) ||
        (x_stride_b & 3) || (x_stride_t & 3) || x_stride_t < width || x_stride_b < 0 || (row_zero && row_zero_stride_b < window))
        return false;
    if (n_weights(kind) && !weights) return false;
    a.x = x, a.xs_b = x_stride_b, a.xs_t = x_stride_t, a.y = y, a.rz = row_zero, a.rz_sb = row_zero_stride_b;
    a.B = batch, a.L = window;
    for (int j = 0; j < n_weights(kind); ++j) {
        if (!weights[j] || !aligned16(weights[j])) return false;
        a.w[j] = weights[j];
    }
    return true;
}

extern "C" {

int asac_rows_gate_supported(int kind, int width) { return kind_ok(kind) && width_ok(width); }

int asac_rows_gate_forward(int kind, const float* x, int64_t x_stride_b, int64_t x_stride_t, const float* y,
                           const uint8_t* row_zero, int64_t row_zero_stride_b, int batch, int window, int width,
                           const float* const* weights, const float* bias_z, float* out, float* const* saved, void* stream) {
    GateArgs a{};
    if (!gate_common(a, kind, x, x_stride_b, x_stride_t, y, row_zero, row_zero_stride_b, batch, window, width, weights) || !out ||
        !aligned16(out) || (kind == kRecurrent && (!bias_z || !aligned16(bias_z))))
        return bad_arg("asac_rows_gate_forward");
    a.bz = bias_z, a.out = out;
    for (int j = 0; saved && j < n_saved(kind); ++j) {
        if (!saved[j] || !aligned16(saved[j])) return bad_arg("asac_rows_gate_forward: saved");
        a.sv[j] = saved[j];
    }
    const dim3 grid((unsigned)(((int64_t)batch * window + 15) / 16));
    hipStream_t s = as_stream(stream);
    if (kind == kResidual) RG_LAUNCH2(k_gate_residual, false, width, grid, s, a);
    else if (kind == kOutput) RG_LAUNCH(k_gate_output_fwd, width, grid, s, a);
    else RG_LAUNCH(k_gate_recurrent_fwd, width, grid, s, a);
    return finish_launch("asac_rows_gate_forward");
}

int asac_rows_gate_backward(int kind, const float* grad_out, const float* x, int64_t x_stride_b, int64_t x_stride_t,
                            const float* y, const uint8_t* row_zero, int64_t row_zero_stride_b, int batch, int window, int width,
                            const float* const* weights, const float* const* saved, float* grad_x, float* grad_y,
                            float* const* grad_pre, float* rx, void* stream) {
    GateArgs a{};
    if (!gate_common(a, kind, x, x_stride_b, x_stride_t, y, row_zero, row_zero_stride_b, batch, window, width, weights) ||
        !grad_out || !grad_x || !grad_y || !aligned16(grad_out) || !aligned16(grad_x) || !aligned16(grad_y) ||
        (n_saved(kind) && (!saved || !grad_pre)) || (kind == kRecurrent && (!rx || !aligned16(rx))))
        return bad_arg("asac_rows_gate_backward");
    if (grad_x == grad_y && kind != kResidual) return bad_arg("asac_rows_gate_backward: grad_x is grad_y");
    a.go = grad_out, a.gx = grad_x, a.gy = grad_y, a.rx = rx;
    for (int j = 0; j < n_saved(kind); ++j) {
        if (!saved[j] || !grad_pre[j] || !aligned16(saved[j]) || !aligned16(grad_pre[j]))
            return bad_arg("asac_rows_gate_backward: saved");
        a.sv[j] = const_cast<float*>(saved[j]), a.gp[j] = grad_pre[j];
    }
    const dim3 grid((unsigned)(((int64_t)batch * window + 15) / 16));
    hipStream_t s = as_stream(stream);
    if (kind == kResidual) RG_LAUNCH2(k_gate_residual, true, width, grid, s, a);
    else if (kind == kOutput) RG_LAUNCH(k_gate_output_bwd, width, grid, s, a);
    else RG_LAUNCH(k_gate_recurrent_bwd, width, grid, s, a);
    return finish_launch("asac_rows_gate_backward");
}

}  // extern "C"
