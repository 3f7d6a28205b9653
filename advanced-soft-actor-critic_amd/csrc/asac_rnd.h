// Random network distillation, continuous actions (reference nn_models: ModelRND.c_dense = LinearLayers(S + A, 64, 2, None)):
// the device code both launches of csrc/rnd.hip share.  One "RND stack" is two GELU ResBlocks  in -> 64 -> 64  without an
// output Linear:
//   z1 = W1 x + b1,  h1 = gelu(z1) + r1 x,  z2 = W2 h1 + b2,  p = gelu(z2) + r2 h1        (r1 only where in == 64)
//
// A workgroup (4 waves) owns a tile of 16 rows.  Both stacks' weights are staged to LDS once per workgroup (16-byte loads, all
// of a stack issued before its first store), a layer is `__builtin_amdgcn_mfma_f32_16x16x4f32` with the WEIGHTS as the A
// operand and the ROWS as the N dimension: wave w forms output features [16 w, 16 w + 16), lane (g = lane >> 4, r = lane & 15)
// ends with features 16 w + 4 g + {0..3} of row r — four consecutive floats, 16-byte stores, and the SAME lane holds the
// same (row, features) after every layer, so residuals, GELU derivatives and the loss never leave its registers.  Both
// operands are 16-byte LDS reads (four consecutive k per lane); the pitches (width + 4 floats) keep rows 16-byte aligned
// and put the 16 rows a read instruction touches on different banks.  The input width is padded to a multiple of 16
// with zero columns on both operands.  Two accumulators take alternate blocks of 16 inputs (a dependent MFMA waits 40 cycles,
// an independent one issues after 32) and are added once: a fixed order, equal inputs give equal bits.
#pragma once
#include "asac_common.h"
#include "asac_gelu.h"

namespace asac {
namespace rnd {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kWidth = ASAC_RND_WIDTH, kMaxIn = ASAC_RND_MAX_IN;
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kTile = 16;                 // rows of a tile
constexpr int kPitch = kWidth + 4;        // floats between rows of a 64-wide LDS tile / matrix

#define ASAC_RND_MF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 mfma4(const f32x4 a, const f32x4 b, f32x4 c) {
    c = ASAC_RND_MF(a[0], b[0], c);
    c = ASAC_RND_MF(a[1], b[1], c);
    c = ASAC_RND_MF(a[2], b[2], c);
    c = ASAC_RND_MF(a[3], b[3], c);
    return c;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

struct StackDev {                          // one stack's parameters in device memory (nn.Linear layout: out x in)
    const float *w1, *b1, *w2, *b2;
};
struct StackLds {                          // ... and staged: w1 [64][in_pad + 4], w2 [64][68], b1 | b2 [128]
    float *w1, *w2, *b;
};

__host__ __device__ inline int pad16(int in) { return (in + 15) & ~15; }
__host__ __device__ inline int stack_floats(int in) { return kWidth * (pad16(in) + 4) + kWidth * kPitch + 2 * kWidth; }

__device__ __forceinline__ StackLds stack_carve(float* base, int in) {
    StackLds s;
    s.w1 = base;
    s.w2 = s.w1 + kWidth * (pad16(in) + 4);
    s.b = s.w2 + kWidth * kPitch;
    return s;
}

// one stack, global -> LDS.  The matrices are read as flat runs of 16-byte vectors (64 * in floats: a multiple of four
// whatever `in` is; the base is 16-byte aligned) and scattered to their pitched rows; up to 8 + 4 + 1 loads a lane, all
// requested before the first store (indices past the end re-read the last vector: a valid address, nothing is stored).
__device__ __forceinline__ void stack_stage(const StackDev& g, const StackLds& s, int in) {
    const int p1 = pad16(in) + 4, tid = threadIdx.x;
    const int n1 = kWidth * in / 4;                 // <= 2048
    const f32x4* g1 = reinterpret_cast<const f32x4*>(g.w1);
    const f32x4* g2 = reinterpret_cast<const f32x4*>(g.w2);
    f32x4 v1[8], v2[4], vb;
#pragma unroll
    for (int u = 0; u < 8; ++u) v1[u] = g1[min(tid + u * kThreads, n1 - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u) v2[u] = g2[tid + u * kThreads];      // 64 * 64 / 4 = 4 * kThreads vectors
    vb = reinterpret_cast<const f32x4*>(tid < 16 ? g.b1 : g.b2)[tid & 15];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = tid + u * kThreads;
        if (i < n1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int flat = 4 * i + e, r = flat / in, c = flat - r * in;
                s.w1[r * p1 + c] = v1[u][e];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid + u * kThreads, r = i >> 4, c = (i & 15) * 4;
        st4(s.w2 + r * kPitch + c, v2[u]);
    }
    if (tid < 32) st4(s.b + 4 * tid, vb);
    // the zero columns [in, in_pad) of the first matrix
    const int padc = pad16(in) - in;
    for (int i = tid; i < kWidth * padc; i += kThreads) {
        const int r = i / padc, c = in + (i - r * padc);
        s.w1[r * p1 + c] = 0.f;
    }
}

// z[row r][16 w + 4 g + i] = b[..] + sum_k W[16 w + 4 g + i][k] X[r][k],  K a multiple of 16; W [64][pw], X [16][px] in LDS
__device__ __forceinline__ f32x4 layer_forward(const float* W, int pw, const float* X, int px, const float* b, int K,
                                               int wave, int lane) {
    const int r = lane & 15, g = lane >> 4;
    const float* wp = W + (16 * wave + r) * pw + 4 * g;      // A: feature 16 w + r, inputs k0 + 4 g + {0..3}
    const float* xp = X + r * px + 4 * g;                    // B: row r, the same inputs
    f32x4 c0 = zero4(), c1 = zero4();
    for (int k0 = 0; k0 < K; k0 += 32) {
        c0 = mfma4(ld4(wp + k0), ld4(xp + k0), c0);
        if (k0 + 16 < K) c1 = mfma4(ld4(wp + k0 + 16), ld4(xp + k0 + 16), c1);
    }
    return (c0 + c1) + ld4(b + 16 * wave + 4 * g);
}

// gh[row r][16 w + 4 g + i] = sum_f G[r][f] W[f][16 w + 4 g + i]   (the transposed product: four strided words of a column)
__device__ __forceinline__ f32x4 layer_backward(const float* W /*[64][68]*/, const float* G /*[16][68]*/, int wave, int lane) {
    const int r = lane & 15, g = lane >> 4;
    const float* wp = W + (4 * g) * kPitch + 16 * wave + r;   // A: output column 16 w + r, features f0 + 4 g + {0..3}
    const float* gp = G + r * kPitch + 4 * g;                 // B: row r, the same features
    f32x4 c0 = zero4(), c1 = zero4();
#pragma unroll
    for (int f0 = 0; f0 < kWidth; f0 += 32) {
        f32x4 a0, a1;
#pragma unroll
        for (int i = 0; i < 4; ++i) a0[i] = wp[(f0 + i) * kPitch], a1[i] = wp[(f0 + 16 + i) * kPitch];
        c0 = mfma4(a0, ld4(gp + f0), c0);
        c1 = mfma4(a1, ld4(gp + f0 + 16), c1);
    }
    return c0 + c1;
}

struct StackOut {
    f32x4 p, h1, d1, d2;       // output, hidden activations, gelu'(z1), gelu'(z2): features 16 w + 4 g + {0..3} of row lane & 15
};

// One stack over the tile xt [16][in_pad + 4] (zero beyond `in`); ht [16][68] is the hidden tile it passes through.  Called
// by all 256 threads; the caller has a barrier between filling xt and this call.
__device__ __forceinline__ StackOut stack_forward(const StackLds& s, const float* xt, float* ht, int in, bool r1, bool r2,
                                                  int wave, int lane) {
    const int inp = pad16(in), p1 = inp + 4, r = lane & 15, c = 16 * wave + 4 * (lane >> 4);
    StackOut o;
    const f32x4 z1 = layer_forward(s.w1, p1, xt, p1, s.b, inp, wave, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v, d;
        gelu_parts(z1[i], v, d);
        o.h1[i] = v, o.d1[i] = d;
    }
    if (r1) o.h1 = o.h1 + ld4(xt + r * p1 + c);            // (in == 64: the tile's own columns)
    __syncthreads();                                          // every wave is done with the previous contents of ht
    st4(ht + r * kPitch + c, o.h1);
    __syncthreads();
    const f32x4 z2 = layer_forward(s.w2, kPitch, ht, kPitch, s.b + kWidth, kWidth, wave, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v, d;
        gelu_parts(z2[i], v, d);
        o.p[i] = v, o.d2[i] = d;
    }
    if (r2) o.p = o.p + o.h1;
    return o;
}

// a candidate action component: the per-element term of squash_sample_at (asac_squash.h) / squash_rows_block (returns.hip)
__device__ __forceinline__ float squashed_action(float loc, float scale, float eps) {
    const float x = loc + eps * scale;
    return tanhf(x);
}

// host side, shared by rnd.hip and drnd.hip: raise a kernel's dynamic LDS limit once; the alignment the 16-byte accesses need
inline int set_lds_limit(const void* fn, size_t bytes, bool& done, const char* where) {
    if (done) return 0;
    hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) {
        set_error(err, where);
        return (int)err;
    }
    done = true;
    return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace rnd
}  // namespace asac
