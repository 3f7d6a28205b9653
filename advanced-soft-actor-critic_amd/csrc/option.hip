// The option-critic's per-option learner (reference algorithm/oc/option_base.py): its two elementwise / scan pieces.
//
// asac_option_return — the n-step / V-trace return of OptionBase._get_y's continuous branch (option_base.py:287, 376-427)
// in ONE launch: asac_vtrace_return_min (returns.hip K4) with the termination mix in front of the scan,
//   V(s_t)   = min_{e in subset_n}    Q_e(s_t, a_t) - alpha logpi_t
//   V(s_t+1) = (1 - beta_t) * (min_{e in subset_next} Q_e(s_t+1, a_t+1) - alpha logpi_t+1) + beta_t * mean_o V_o(s_t+1)
// The step's loads and arithmetic are asac_vtrace.h's (vtrace_step_load, vtrace_step_finish_v), the scan has the segment
// order of k_vtrace_return_min: with beta == 0 everywhere the result has that kernel's bits.  n_vs, next_n_vs and the mean
// over the options live in registers / LDS only.
// Summation order of the option mean: o = 0, 1, .., O-1 by ONE lane, then one division by O.  Neighbouring lanes take
// neighbouring (row, t) items, so a wavefront's loads of one o cover a dense run of V when V is contiguous (O floats apart,
// O <= 16: every fetched line is used by the following o).
//
// asac_termination_loss_grad — compute_termination_grads behind the head's forward (option_base.py:695-703):
//   loss = mean_b(beta_b * (y_b - mean_o V_bo + terminal_entropy) * ~done_b * is_b),  d loss / d beta_b
// Summation order of the loss: lane partial (elements in index order) -> wave (xor butterfly) -> workgroup (waves in
// order) -> the last workgroup to arrive adds the workgroups' sums in workgroup order (asac_ordered_finish.h).  The
// arrival counter is an integer; no float atomics: equal inputs give equal bits.  -ffp-contract=off.
#include "asac_common.h"
#include "asac_option.h"
#include "asac_ordered_finish.h"
#include "asac_vtrace.h"

namespace asac {

struct OptionReturnDev {
    asac_vtrace_args_t a;
    const float* beta;               // [B, n]      element (b, t) at b * beta_sb + t * beta_st
    const float* v;                  // [B, n, O]   element (b, t, o) at b * v_sb + t * v_st + o * v_so
    int64_t beta_sb, beta_st, v_sb, v_st, v_so;
    int32_t O, R, pitch, seg;
};

__global__ __launch_bounds__(256) void k_option_return(const OptionReturnDev by_value) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // the argument block (40 fields) is read where it is used, not held in scalar registers (asac_common.h ASAC_KARG)
    const ASAC_KARG OptionReturnDev& v = *static_cast<const ASAC_KARG OptionReturnDev*>(kernarg_base());
    const ASAC_KARG asac_vtrace_args_t& a = v.a;
    const int n = a.n, R = v.R, pitch = v.pitch, SEG = v.seg;
    float* s_d = lds;                        // [R][pitch]  per-step term d_t
    float* s_c = s_d + R * pitch;            // [R][pitch]  trace-cutting factor c_t
    float* s_v0 = s_c + R * pitch;           // [R]         V(s_0)
    const int row0 = blockIdx.x * R;
    // the online critics' values of the row this lane will finish (TD error variant), requested first
    float q_on[4] = {0.f, 0.f, 0.f, 0.f};
    {
        const int r = threadIdx.x / SEG, b = row0 + r;
        if (a.td_error_out && r < R && b < a.B && threadIdx.x == r * SEG) {
#pragma unroll
            for (int j = 0; j < 4; ++j) q_on[j] = a.q_online[(int64_t)min(j, a.E_online - 1) * a.B + b];
        }
    }
    const float alpha = expf(*a.log_alpha);
    // phase 1: all lanes, coalesced over (row, t)
    for (int f = threadIdx.x; f < R * n; f += blockDim.x) {
        const int r = f / n, t = f - r * n;
        const int b = row0 + r;
        if (b >= a.B) continue;
        const VtraceStepRaw raw = vtrace_step_load(a, b, t);
        const float beta = v.beta[(int64_t)b * v.beta_sb + (int64_t)t * v.beta_st];
        const float vbar = option_mean(v.v + (int64_t)b * v.v_sb + (int64_t)t * v.v_st, v.v_so, v.O);
        float d, c;
        const float v_t = vtrace_step_finish_option(a, raw, alpha, beta, vbar, &d, &c);
        if (t == 0) s_v0[r] = v_t;
        s_d[r * pitch + t] = d;
        s_c[r * pitch + t] = c;
    }
    __syncthreads();

    // phase 2: k_vtrace_return_min's — SEG lanes per row, contiguous segments, combined as S_k + P_k * (rest)
    const int r = threadIdx.x / SEG, k = threadIdx.x - r * SEG;
    const int b = row0 + r;
    const bool valid = r < R && b < a.B;
    const int len = (n + SEG - 1) / SEG;
    const int t0 = min(n, k * len), t1 = min(n, t0 + len);
    float S = 0.f, P = 1.f;
    if (valid) {
        const float* d = s_d + r * pitch;
        const float* c = s_c + r * pitch;
        for (int t = t0; t < t1; ++t) {
            S += P * d[t];
            P *= c[t];
        }
    }
    for (int off = 1; off < SEG; off <<= 1) {
        const float S_hi = __shfl_down(S, off, 64), P_hi = __shfl_down(P, off, 64);
        S += P * S_hi;
        P *= P_hi;
    }
    if (!valid || k != 0) return;
    const float y = s_v0[r] + S;
    a.y_out[b] = y;
    if (a.td_error_out) {
        float s = 0.f;
        if (a.E_online <= 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < a.E_online) s += fabsf(q_on[e] - y);
        } else {
            for (int e = 0; e < a.E_online; ++e) s += fabsf(a.q_online[(int64_t)e * a.B + b] - y);
        }
        a.td_error_out[b] = s / (float)a.E_online;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
constexpr int kTermThreads = 256, kTermPerLane = 4, kTermMaxBlocks = ASAC_TERMINATION_MAX_BLOCKS;

struct TermArgs {
    const float *beta, *y, *v;       // [B] (beta_stride apart), [B] (y_stride apart), [B, O]
    const uint8_t* done;             // [B]
    const float* is;                 // [B] or NULL
    float *loss, *dbeta;             // f32[1], [B] contiguous
    float* partial;                  // [kTermMaxBlocks] workgroup sums
    unsigned int* counter;           // arrivals: zero before the first launch, left zero by every launch
    int64_t beta_stride, y_stride, v_sb, v_so, is_stride;
    int32_t B, O;
    float terminal_entropy;
};

__global__ __launch_bounds__(kTermThreads) void k_termination_loss_grad(const TermArgs a) {
    const int tid = threadIdx.x;
    const int B = a.B;
    const float inv = 1.f / (float)B;
    const int stride = gridDim.x * kTermThreads;
    float s = 0.f;
    for (int i0 = blockIdx.x * kTermThreads + tid; i0 < B; i0 += kTermPerLane * stride) {
        float bv[kTermPerLane], yv[kTermPerLane], wv[kTermPerLane];
        bool dn[kTermPerLane];
#pragma unroll
        for (int u = 0; u < kTermPerLane; ++u) {           // the scalar loads of a lane's rows requested together
            const int64_t i = min(i0 + u * stride, B - 1);
            bv[u] = a.beta[i * a.beta_stride];
            yv[u] = a.y[i * a.y_stride];
            dn[u] = a.done[i] != 0;
            wv[u] = a.is ? a.is[i * a.is_stride] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < kTermPerLane; ++u) {
            const int i = i0 + u * stride;
            if (i >= B) continue;
            const float vbar = option_mean(a.v + (int64_t)i * a.v_sb, a.v_so, a.O);
            const float adv = yv[u] - vbar + a.terminal_entropy;      // option_base.py:697
            float l = 0.f, g = 0.f;
            if (!dn[u]) {                                             // * ~done: exact zeros for finished rows
                l = bv[u] * adv;
                g = inv;
                if (a.is) l *= wv[u], g *= wv[u];
                g *= adv;
            }
            s += l;
            a.dbeta[i] = g;
        }
    }
    s = block_sum_waves<kTermThreads>(s);
    if (tid == 0) finish_publish(a.partial + blockIdx.x, s);
    if (!finish_arrive(a.counter) || tid != 0) return;
    *a.loss = finish_sum_in_order(a.partial, 1, (int)gridDim.x) / (float)B;      // torch.mean: the sum over the count
    finish_reset(a.counter);
}

}  // namespace asac

using namespace asac;

extern "C" {

int asac_option_return(const asac_vtrace_args_t* args_host, const float* beta, int64_t beta_stride_b,
                       int64_t beta_stride_t, const float* v_options, int64_t v_stride_b, int64_t v_stride_t,
                       int64_t v_stride_o, int num_options, void* stream) {
    if (!args_host) return bad_arg("asac_option_return");
    const asac_vtrace_args_t& h = *args_host;
    if (h.B <= 0 || h.n <= 0 || !h.y_out || !h.q || !h.logp || !h.log_alpha || h.E_sample <= 0 ||
        h.E_sample > ASAC_MAX_ENSEMBLE || !beta || !v_options || num_options <= 0 ||
        num_options > ASAC_OPTION_MAX_OPTIONS)
        return bad_arg("asac_option_return");
    if (h.use_n_step_is && (!h.mu_prob || !h.pi_prob || h.A <= 0)) return bad_arg("asac_option_return: is");
    if (h.td_error_out && (!h.q_online || h.E_online <= 0)) return bad_arg("asac_option_return: td error");
    OptionReturnDev v{};
    v.a = h;
    v.beta = beta, v.v = v_options;
    v.beta_sb = beta_stride_b, v.beta_st = beta_stride_t;
    v.v_sb = v_stride_b, v.v_st = v_stride_t, v.v_so = v_stride_o;
    v.O = num_options;
    v.pitch = (h.n + 1) | 1;                      // odd pitch: conflict-free row-per-lane reads
    // rows per workgroup and lanes per row: asac_vtrace_return_min's choice (the scan's association depends on it)
    const int64_t items = (int64_t)h.B * h.n;
    const bool huge = items >= (1 << 21) && h.n <= 8;
    int R = huge ? 256 : 64;
    if (items < (1 << 17))
        while (R > 1 && R * h.n > 512) R >>= 1;
    while (R > 1 && (size_t)(2 * R * v.pitch + R) * sizeof(float) > 64 * 1024) R >>= 1;
    v.R = R;
    v.seg = vtrace_scan_lanes(h.B, h.n);
    const size_t lds = (size_t)(2 * R * v.pitch + R) * sizeof(float);
    if (lds > 64 * 1024) return bad_arg("asac_option_return: n too large");
    const int blocks = (h.B + R - 1) / R;
    ASAC_LAUNCH(k_option_return, dim3((unsigned)blocks), dim3(256), lds, as_stream(stream), v);
    return finish_launch("asac_option_return");
}

int64_t asac_termination_loss_grad_workspace(void) { return kTermMaxBlocks + 4; }   // workgroup sums + the arrival counter

int asac_termination_loss_grad(const float* beta, int64_t beta_stride, const float* y, int64_t y_stride,
                               const float* v_options, int64_t v_stride_b, int64_t v_stride_o, int num_options,
                               const uint8_t* done, const float* priority_is, int64_t is_stride, float terminal_entropy,
                               int B, float* loss, float* dbeta, float* workspace, void* stream) {
    if (!beta || !y || !v_options || !done || !loss || !dbeta || !workspace || B <= 0 || num_options <= 0 ||
        num_options > ASAC_OPTION_MAX_OPTIONS || B > ASAC_TERMINATION_MAX_ROWS)
        return bad_arg("asac_termination_loss_grad");
    TermArgs a;
    a.beta = beta, a.y = y, a.v = v_options, a.done = done, a.is = priority_is;
    a.loss = loss, a.dbeta = dbeta;
    a.partial = workspace, a.counter = reinterpret_cast<unsigned int*>(workspace + kTermMaxBlocks);
    a.beta_stride = beta_stride, a.y_stride = y_stride, a.v_sb = v_stride_b, a.v_so = v_stride_o, a.is_stride = is_stride;
    a.B = B, a.O = num_options;
    a.terminal_entropy = terminal_entropy;
    const int64_t want = ((int64_t)B + kTermThreads * kTermPerLane - 1) / (kTermThreads * kTermPerLane);
    const unsigned blocks = (unsigned)(want < kTermMaxBlocks ? want : kTermMaxBlocks);
    ASAC_LAUNCH(k_termination_loss_grad, dim3(blocks), dim3(kTermThreads), 0, as_stream(stream), a);
    return finish_launch("asac_termination_loss_grad");
}

}  // extern "C"
