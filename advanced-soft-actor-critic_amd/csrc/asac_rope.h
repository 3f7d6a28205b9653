// The arithmetic of the rotary position encodings (reference nn_models/layers/seq_layers.py: `RotaryPositionalEncoding`,
// `RotaryPositionalEncoding2`), shared by the launch that rotates on its own (csrc/rope.hip) and the projection launch with the
// rotation as its epilogue (csrc/rows_proj.hip): both give the same bits.  Every result is two products and one sum, in the
// order written (-ffp-contract=off); sines and cosines come from the module's own tables.
#pragma once
#include "asac_common.h"

namespace asac {
namespace rope {

constexpr int kRope = 3, kRope2 = 4;      // POSITIONAL_ENCODING.ROPE / ROPE2

struct Tables {
    const float* t0;      // ROPE: freqs_cis as floats [T][E / 2][2] = (c, s);  ROPE2: cos_cached [T][E]
    const float* t1;      // ROPE2: sin_cached [T][E]
    int32_t T;
};

struct Index {
    const void* p;        // int32 / int64 [B][L] through its strides (in elements; a batch stride of 0: one row for all)
    int64_t sb, st;
    int32_t bytes;        // 4 / 8
};

inline bool kind_ok(int kind) { return kind == kRope || kind == kRope2; }

// the table row of position (b, t): index i reads row i, i < 0 row i + T (the module's `table[i]`); anything outside [-T, T)
// is clamped into the table (the values of such rows are unspecified, the reads stay inside)
__device__ __forceinline__ int64_t table_row(const Index& ix, int b, int t, int T) {
    const int64_t off = b * ix.sb + t * ix.st;
    int64_t i = ix.bytes == 8 ? static_cast<const int64_t*>(ix.p)[off] : (int64_t) static_cast<const int32_t*>(ix.p)[off];
    if (i < 0) i += T;
    return i < 0 ? 0 : (i >= T ? T - 1 : i);
}

// ROPE, the pair (2 i, 2 i + 1) with its (c, s)
__device__ __forceinline__ void pair_fwd(float x0, float x1, float c, float s, float& y0, float& y1) {
    y0 = x0 * c - x1 * s;
    y1 = x0 * s + x1 * c;
}
__device__ __forceinline__ void pair_bwd(float g0, float g1, float c, float s, float& x0, float& x1) {
    x0 = g0 * c + g1 * s;
    x1 = g1 * c - g0 * s;
}

// ROPE2, the features j < E / 2 (lo) and j + E / 2 (hi) with the table values at both
__device__ __forceinline__ void half_fwd(float xl, float xh, float cl, float sl, float ch, float sh, float& yl, float& yh) {
    yl = xl * cl + (-xh) * sl;
    yh = xh * ch + xl * sh;
}
__device__ __forceinline__ void half_bwd(float gl, float gh, float cl, float sl, float ch, float sh, float& xl, float& xh) {
    xl = gl * cl + gh * sh;
    xh = gh * ch - gl * sl;
}

}  // namespace rope
}  // namespace asac
