// The rotary position encodings of `MultiheadAttention.forward` (reference nn_models/layers/seq_layers.py:
// `self.rope(query_index, key_index, q, k)` with `RotaryPositionalEncoding` = ROPE, complex pairs of consecutive features, or
// `RotaryPositionalEncoding2` = ROPE2, feature j paired with j + E / 2) on their own: ONE launch rotates q [B][Lq][E] and
// k [B][Lk][E] into dense outputs (the module code: an index cast, a table gather, a complex product — or two products, a cat
// and an add — per tensor, and the autograd mirror of it), ONE launch un-rotates both gradients.  For what the projection launch
// with the rotation in its epilogue (csrc/rows_proj.hip) does not cover: projections with hidden layers, distinct query / key /
// value tensors, widths other than 32 / 64 / 128.  Arithmetic: asac_rope.h.
//
// A lane owns one pair of one row: it reads the row's index, the pair's table values and the two features, and writes two
// results.  Elementwise and tiny (a window batch is ~10^4 rows): the launch is latency, not bandwidth.
#include "asac_rope.h"

namespace asac {
namespace rope {

constexpr int kThreads = 256;

struct Side {
    const float* x; int64_t xs_b, xs_t;      // [B][L][E] (feature stride 1)
    Index ix;
    int32_t L;
    float* y;                                // [B][L][E] dense
};

struct RopeArgs {
    Tables tab;
    int32_t B, E;
    Side side[2];                            // q, k
};

template <int KIND, bool BWD>
__global__ void __launch_bounds__(kThreads) k_rope(const RopeArgs a) {
    const int H = a.E >> 1;
    const int64_t pairs_q = (int64_t)a.B * a.side[0].L * H, pairs = pairs_q + (int64_t)a.B * a.side[1].L * H;
    int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= pairs) return;
    const Side& s = a.side[p >= pairs_q];
    if (p >= pairs_q) p -= pairs_q;
    const int64_t row = p / H;
    const int i = (int)(p - row * H);
    const int b = (int)(row / s.L), t = (int)(row - (int64_t)b * s.L);
    const int64_t tr = table_row(s.ix, b, t, a.tab.T);
    const float* xp = s.x + b * s.xs_b + t * s.xs_t;
    float* yp = s.y + row * a.E;
    if (KIND == kRope) {
        const float c = a.tab.t0[tr * a.E + 2 * i], sn = a.tab.t0[tr * a.E + 2 * i + 1];
        float y0, y1;
        if (BWD) pair_bwd(xp[2 * i], xp[2 * i + 1], c, sn, y0, y1);
        else pair_fwd(xp[2 * i], xp[2 * i + 1], c, sn, y0, y1);
        yp[2 * i] = y0, yp[2 * i + 1] = y1;
    } else {
        const float* cs = a.tab.t0 + tr * a.E;
        const float* sn = a.tab.t1 + tr * a.E;
        float yl, yh;
        if (BWD) half_bwd(xp[i], xp[i + H], cs[i], sn[i], cs[i + H], sn[i + H], yl, yh);
        else half_fwd(xp[i], xp[i + H], cs[i], sn[i], cs[i + H], sn[i + H], yl, yh);
        yp[i] = yl, yp[i + H] = yh;
    }
}

inline bool width_ok(int E) { return E >= 2 && E <= 4096 && (E & 1) == 0; }

}  // namespace rope
}  // namespace asac

using namespace asac;
using namespace asac::rope;

template <bool BWD>
static int rope_launch(const char* what, int kind, const float* table0, const float* table1, int table_rows, int width, int batch,
                       const float* q, int64_t q_stride_b, int64_t q_stride_t, int q_len, const void* q_index,
                       int64_t q_index_stride_b, int64_t q_index_stride_t, const float* k, int64_t k_stride_b, int64_t k_stride_t,
                       int k_len, const void* k_index, int64_t k_index_stride_b, int64_t k_index_stride_t, int index_bytes,
                       float* out_q, float* out_k, void* stream) {
    if (!kind_ok(kind) || !width_ok(width) || !table0 || (kind == kRope2 && !table1) || table_rows < 1 || batch <= 0 || q_len <= 0 ||
        k_len <= 0 || !q || !k || !q_index || !k_index || !out_q || !out_k || (index_bytes != 4 && index_bytes != 8) ||
        q_stride_b < 0 || q_stride_t < 0 || k_stride_b < 0 || k_stride_t < 0 || q_index_stride_b < 0 || q_index_stride_t < 0 ||
        k_index_stride_b < 0 || k_index_stride_t < 0)
        return bad_arg(what);
    RopeArgs a{};
    a.tab = Tables{table0, table1, table_rows};
    a.B = batch, a.E = width;
    a.side[0] = Side{q, q_stride_b, q_stride_t, Index{q_index, q_index_stride_b, q_index_stride_t, index_bytes}, q_len, out_q};
    a.side[1] = Side{k, k_stride_b, k_stride_t, Index{k_index, k_index_stride_b, k_index_stride_t, index_bytes}, k_len, out_k};
    const int64_t pairs = (int64_t)batch * ((int64_t)q_len + k_len) * (width / 2);
    const dim3 grid((unsigned)((pairs + kThreads - 1) / kThreads));
    if (kind == kRope) ASAC_LAUNCH((k_rope<kRope, BWD>), grid, dim3(kThreads), 0, as_stream(stream), a);
    else ASAC_LAUNCH((k_rope<kRope2, BWD>), grid, dim3(kThreads), 0, as_stream(stream), a);
    return finish_launch(what);
}

extern "C" {

int asac_rope_supported(int kind, int width) { return kind_ok(kind) && width_ok(width); }

int asac_rope_forward(int kind, const float* table0, const float* table1, int table_rows, int width, int batch, const float* q,
                      int64_t q_stride_b, int64_t q_stride_t, int q_len, const void* q_index, int64_t q_index_stride_b,
                      int64_t q_index_stride_t, const float* k, int64_t k_stride_b, int64_t k_stride_t, int k_len,
                      const void* k_index, int64_t k_index_stride_b, int64_t k_index_stride_t, int index_bytes, float* out_q,
                      float* out_k, void* stream) {
    return rope_launch<false>("asac_rope_forward", kind, table0, table1, table_rows, width, batch, q, q_stride_b, q_stride_t, q_len,
                              q_index, q_index_stride_b, q_index_stride_t, k, k_stride_b, k_stride_t, k_len, k_index,
                              k_index_stride_b, k_index_stride_t, index_bytes, out_q, out_k, stream);
}

int asac_rope_backward(int kind, const float* table0, const float* table1, int table_rows, int width, int batch,
                       const float* grad_q, int64_t grad_q_stride_b, int64_t grad_q_stride_t, int q_len, const void* q_index,
                       int64_t q_index_stride_b, int64_t q_index_stride_t, const float* grad_k, int64_t grad_k_stride_b,
                       int64_t grad_k_stride_t, int k_len, const void* k_index, int64_t k_index_stride_b, int64_t k_index_stride_t,
                       int index_bytes, float* out_q, float* out_k, void* stream) {
    return rope_launch<true>("asac_rope_backward", kind, table0, table1, table_rows, width, batch, grad_q, grad_q_stride_b,
                             grad_q_stride_t, q_len, q_index, q_index_stride_b, q_index_stride_t, grad_k, grad_k_stride_b,
                             grad_k_stride_t, k_len, k_index, k_index_stride_b, k_index_stride_t, index_bytes, out_q, out_k, stream);
}

}  // extern "C"
