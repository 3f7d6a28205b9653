// Image augmentations of the siamese views (algorithm/utils/image_transforms.py) as ONE launch per call: Gaussian blur,
// brightness, crop + bilinear resize, salt-and-pepper and uniform noise, or a uniformly random choice among up to eight of
// them.  One workgroup per [H][W] plane (past 512 planes a workgroup takes several in turn): the plane is staged in LDS once
// (16-byte loads where the plane's address allows), the result leaves as whole rows.  The blur is separable (horizontal
// LDS -> LDS, vertical LDS -> global) with reflect INDEXING instead of a padded copy, and its weights are computed here from
// sigma, so a drawn sigma costs nothing.
//
// Everything random is decided on the device.  A module instance owns 16 bytes: an int64 draw counter and an arrival word.
// Every workgroup reads the counter at entry and derives the call's draws (which member, crop offsets, sigma or factor) from
// Philox4x32-10(seed, instance, counter): all workgroups get the same values without talking to each other.  The last
// workgroup to arrive (asac_ordered_finish.h) advances the counter — by then every other one has read it — and leaves the
// arrival word zero.  A captured launch therefore draws afresh on every replay; a host draw would be baked into the graph.
//
// The warps (nearest resized crop, elastic transform: asac_image_warp) are a second kernel with the same draw protocol, below.
#include "asac_common.h"
#include "asac_noise.h"
#include "asac_ordered_finish.h"

#include <cmath>

namespace asac {

constexpr int kImgThreads = 256;
// every workgroup arrives at ONE word: arrivals are served one after the other by the memory side (about 30 ns each on the
// MI355X), so the grid stops at what is resident at once (two workgroups on each of 256 CUs) and walks the planes
constexpr int kImgMaxGrid = 512;
constexpr int kImgBlurOutputs = 4;
constexpr int kImgWeights = 32;          // >= ASAC_IMAGE_MAX_KERNEL: the x taps, then the y taps
static_assert(ASAC_IMAGE_MAX_KERNEL <= kImgWeights, "tap table");
// two planes (the staged frame and the blur's horizontal pass) + the taps: two workgroups fit the CU's 160 KiB
static_assert(2 * (2 * ASAC_IMAGE_MAX_PLANE + 2 * kImgWeights + 4) * sizeof(float) <= 160 * 1024, "LDS budget");

struct ImageArgs {
    const float* x;
    float* y;
    int64_t* state;          // [0] the draw counter, [1] (its first word) the arrival counter; NULL: nothing is drawn
    double* drawn;           // counter, choice, top, left, sigma, factor (or NULL)
    uint64_t seed;
    uint32_t instance;
    int64_t planes;
    int32_t C, H, W, Ho, Wo, n_ops, advance;
    uint32_t magic_w, magic_wo;   // fastdiv_magic of W and Wo (0: divide)
    asac_image_op_t ops[ASAC_IMAGE_MAX_OPS];
};

// Philox counter words: (index, tag << 28 | instance, counter lo, counter hi); key: the seed
enum : uint32_t { kTagCall = 0u, kTagSaltPepper = 1u, kTagUniform = 2u };

__device__ __forceinline__ Philox image_philox(const uint64_t seed, uint32_t instance, uint64_t ctr, uint32_t tag, uint32_t index) {
    return philox4x32_10(index, (tag << 28) | (instance & 0x0FFFFFFFu), (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed,
                         (uint32_t)(seed >> 32));
}

__device__ __forceinline__ float image_u01(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }   // [0, 1), 24 bits

// torch's 'reflect' padding as an index (the edge sample is not repeated); one fold is enough while k / 2 < n
__device__ __forceinline__ int image_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

__device__ __forceinline__ float image_clamp01(float v) {   // NaN stays NaN, as torch.clamp keeps it
    v = v < 0.f ? 0.f : v;
    return v > 1.f ? 1.f : v;
}

// source coordinate of a destination index: bilinear, align_corners=False (negative coordinates clamp to 0)
__device__ __forceinline__ void image_source(int dst, float scale, int n_in, int* i0, int* i1, float* lambda) {
    float s = ((float)dst + 0.5f) * scale - 0.5f;
    s = s < 0.f ? 0.f : s;
    int lo = (int)s;
    lo = lo > n_in - 1 ? n_in - 1 : lo;
    *i0 = lo;
    *i1 = lo + 1 > n_in - 1 ? n_in - 1 : lo + 1;
    *lambda = s - (float)lo;
}

__global__ __launch_bounds__(kImgThreads) void k_image_augment(const ImageArgs by_value) {
    const ASAC_KARG ImageArgs& a = *static_cast<const ASAC_KARG ImageArgs*>(kernarg_base());
    __shared__ __attribute__((aligned(16))) float s_a[ASAC_IMAGE_MAX_PLANE];
    __shared__ __attribute__((aligned(16))) float s_b[ASAC_IMAGE_MAX_PLANE];
    __shared__ float s_w[2 * kImgWeights];
    __shared__ uint64_t s_ctr;
    const int tid = (int)threadIdx.x;
    const int H = a.H, W = a.W, HW = H * W, Ho = a.Ho, Wo = a.Wo, n_out = Ho * Wo;
    const uint32_t magic_w = a.magic_w, magic_wo = a.magic_wo;
    const int64_t planes = a.planes;
    int64_t* const state = a.state;
    const uint64_t seed = a.seed;
    const uint32_t instance = a.instance;

    // the call's counter: ONE load a workgroup (2 000 workgroups asking the memory side for the same word take longer than
    // the frames), in flight while the first plane is staged
    if (tid == 0) s_ctr = state ? (uint64_t)__hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;

    // what the call drew: set by every lane, alike, behind the first plane's barrier
    uint64_t ctr = 0;
    asac_image_op_t op{};
    float drawn_value = 0.f;
    int top = -1, left = -1;

    bool first = true;
    for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        // stage the plane
        const float* const src = a.x + plane * HW;
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const float4* const src4 = reinterpret_cast<const float4*>(src);
            float4* const s4 = reinterpret_cast<float4*>(s_a);
            const int n4 = HW >> 2;
            for (int i = tid; i < n4; i += kImgThreads) s4[i] = src4[i];
            for (int i = (n4 << 2) + tid; i < HW; i += kImgThreads) s_a[i] = src[i];
        } else {
            for (int i = tid; i < HW; i += kImgThreads) s_a[i] = src[i];
        }
        __syncthreads();
        float* const dst = a.y + plane * (int64_t)n_out;

        if (first) {
            ctr = s_ctr;
            const Philox d = image_philox(seed, instance, ctr, kTagCall, 0xFFFFFFFFu);
            const int n_ops = a.n_ops;
            const int choice = __builtin_amdgcn_readfirstlane(n_ops > 1 ? (int)__umulhi(d.c[0], (uint32_t)n_ops) : 0);
            op = karg_copy(&a.ops[choice]);
            const float u = image_u01(d.c[3]);
            drawn_value = op.hi > op.lo ? op.lo + u * (op.hi - op.lo) : op.lo;    // sigma | factor
            if (op.kind == ASAC_IMAGE_CROP_RESIZE) {
                top = op.top >= 0 ? op.top : (int)__umulhi(d.c[1], (uint32_t)(H - op.crop_h + 1));
                left = op.left >= 0 ? op.left : (int)__umulhi(d.c[2], (uint32_t)(W - op.crop_w + 1));
            }
            if (plane == 0 && tid == 0 && a.drawn) {
                double* const r = a.drawn;
                const double nan = __builtin_nan("");
                r[0] = (double)(int64_t)ctr;
                r[1] = (double)choice;
                r[2] = (double)top;
                r[3] = (double)left;
                r[4] = op.kind == ASAC_IMAGE_BLUR ? (double)drawn_value : nan;
                r[5] = op.kind == ASAC_IMAGE_BRIGHTNESS ? (double)drawn_value : nan;
            }
            if (op.kind == ASAC_IMAGE_BLUR) {
                // w_i = exp(-0.5 (x_i / sigma)^2), x = linspace(-(k - 1) / 2, (k - 1) / 2, k), normalised: one tap per lane
                const int kx = op.kx, ky = op.ky;
                const float sigma = drawn_value;
                if (tid < kx) {
                    const float t = ((float)tid - 0.5f * (float)(kx - 1)) / sigma;
                    s_w[tid] = expf(-0.5f * (t * t));
                } else if (tid >= kImgWeights && tid < kImgWeights + ky) {
                    const float t = ((float)(tid - kImgWeights) - 0.5f * (float)(ky - 1)) / sigma;
                    s_w[tid] = expf(-0.5f * (t * t));
                }
                __syncthreads();
                float sum_x = 0.f, sum_y = 0.f;
                for (int j = 0; j < kx; ++j) sum_x += s_w[j];
                for (int j = 0; j < ky; ++j) sum_y += s_w[kImgWeights + j];
                __syncthreads();
                if (tid < kx) s_w[tid] = s_w[tid] / sum_x;
                else if (tid >= kImgWeights && tid < kImgWeights + ky) s_w[tid] = s_w[tid] / sum_y;
                __syncthreads();
            }
            first = false;
        }

        const int kind = op.kind;
        if (kind == ASAC_IMAGE_BLUR) {
            // Four outputs a lane and trip: four independent chains of LDS reads (two waves on a SIMD hide little of one
            // chain's latency).  The taps sit in the lanes of one register — x taps in lanes 0..31, y taps in 32..63 — and
            // reach the sum through v_readlane: no LDS read per tap for a value every lane shares.
            const int kx = op.kx, ky = op.ky, rx = kx >> 1, ry = ky >> 1;
            const int taps = __float_as_int(s_w[tid & (2 * kImgWeights - 1)]);
            for (int i0 = tid; i0 < HW; i0 += kImgBlurOutputs * kImgThreads) {
                int at[kImgBlurOutputs], xx[kImgBlurOutputs];
                float acc[kImgBlurOutputs];
#pragma unroll
                for (int e = 0; e < kImgBlurOutputs; ++e) {
                    const int i = min(i0 + e * kImgThreads, HW - 1);        // (past the plane: a valid address, not stored)
                    const int yy = (int)fastdiv((uint32_t)i, (uint32_t)W, magic_w);
                    xx[e] = i - yy * W;
                    at[e] = yy * W;
                    acc[e] = 0.f;
                }
                for (int j = 0; j < kx; ++j) {
                    const float w = __int_as_float(__builtin_amdgcn_readlane(taps, j));
#pragma unroll
                    for (int e = 0; e < kImgBlurOutputs; ++e) acc[e] += w * s_a[at[e] + image_reflect(xx[e] + j - rx, W)];
                }
#pragma unroll
                for (int e = 0; e < kImgBlurOutputs; ++e)
                    if (i0 + e * kImgThreads < HW) s_b[i0 + e * kImgThreads] = acc[e];
            }
            __syncthreads();
            for (int i0 = tid; i0 < HW; i0 += kImgBlurOutputs * kImgThreads) {
                int yy[kImgBlurOutputs], xx[kImgBlurOutputs];
                float acc[kImgBlurOutputs];
#pragma unroll
                for (int e = 0; e < kImgBlurOutputs; ++e) {
                    const int i = min(i0 + e * kImgThreads, HW - 1);
                    yy[e] = (int)fastdiv((uint32_t)i, (uint32_t)W, magic_w);
                    xx[e] = i - yy[e] * W;
                    acc[e] = 0.f;
                }
                for (int j = 0; j < ky; ++j) {
                    const float w = __int_as_float(__builtin_amdgcn_readlane(taps, kImgWeights + j));
#pragma unroll
                    for (int e = 0; e < kImgBlurOutputs; ++e) acc[e] += w * s_b[image_reflect(yy[e] + j - ry, H) * W + xx[e]];
                }
#pragma unroll
                for (int e = 0; e < kImgBlurOutputs; ++e)
                    if (i0 + e * kImgThreads < HW) dst[i0 + e * kImgThreads] = acc[e];
            }
        } else if (kind == ASAC_IMAGE_CROP_RESIZE) {
            const int ch = op.crop_h, cw = op.crop_w;
            const float* const win = s_a + top * W + left;
            if (ch == Ho && cw == Wo) {              // a crop alone (or a resize to the same size): the window's bits
                for (int i = tid; i < n_out; i += kImgThreads) {
                    const int yy = (int)fastdiv((uint32_t)i, (uint32_t)Wo, magic_wo), xx = i - yy * Wo;
                    dst[i] = win[yy * W + xx];
                }
            } else {
                const float scale_h = (float)ch / (float)Ho, scale_w = (float)cw / (float)Wo;
                for (int i = tid; i < n_out; i += kImgThreads) {
                    const int yy = (int)fastdiv((uint32_t)i, (uint32_t)Wo, magic_wo), xx = i - yy * Wo;
                    int y0, y1, x0, x1;
                    float ly, lx;
                    image_source(yy, scale_h, ch, &y0, &y1, &ly);
                    image_source(xx, scale_w, cw, &x0, &x1, &lx);
                    const float hy = 1.f - ly, hx = 1.f - lx;
                    const float r0 = hx * win[y0 * W + x0] + lx * win[y0 * W + x1];
                    const float r1 = hx * win[y1 * W + x0] + lx * win[y1 * W + x1];
                    dst[i] = hy * r0 + ly * r1;
                }
            }
        } else {
            // the element-wise members, four pixels (one Philox block) per lane and trip
            const int groups = (HW + 3) >> 2;
            const bool dst_aligned = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
            // salt and pepper: the draw belongs to (frame, pixel) — every channel's plane sees the same one
            const int64_t draw_plane = kind == ASAC_IMAGE_SALT_PEPPER ? plane / a.C : plane;
            for (int g = tid; g < groups; g += kImgThreads) {
                const int base = g << 2;
                const int n = HW - base < 4 ? HW - base : 4;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = e < n ? s_a[base + e] : 0.f;
                if (kind == ASAC_IMAGE_BRIGHTNESS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = image_clamp01(v[e] * drawn_value);
                } else if (kind == ASAC_IMAGE_SALT_PEPPER || kind == ASAC_IMAGE_UNIFORM_NOISE) {
                    const Philox p = image_philox(seed, instance, ctr, kind == ASAC_IMAGE_SALT_PEPPER ? kTagSaltPepper : kTagUniform,
                                                  (uint32_t)(draw_plane * groups + g));
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float r = image_u01(p.c[e]);
                        if (kind == ASAC_IMAGE_SALT_PEPPER) {
                            // a: the amount, b / c: raise below b, lower above c (disjoint sets: transform.py `_salt_pepper`)
                            if (r < op.b) v[e] = image_clamp01(v[e] + op.a);
                            if (r > op.c) v[e] = image_clamp01(v[e] - op.a);
                        } else {
                            v[e] = image_clamp01(v[e] + r * op.b + op.a);      // a: mean, b: std (transform.py `GaussianNoise`)
                        }
                    }
                }
                if (n == 4 && dst_aligned) {
                    reinterpret_cast<float4*>(dst)[g] = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < n) dst[base + e] = v[e];
                }
            }
        }
        __syncthreads();                             // the next plane overwrites what this one read
    }

    // the arrival: this workgroup holds its copy of the counter, so whoever arrives last may advance it
    if (state) {
        unsigned int* const arrived = reinterpret_cast<unsigned int*>(state + 1);
        if (finish_arrive(arrived) && tid == 0) {
            if (a.advance) __hip_atomic_store(state, (int64_t)(s_ctr + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            finish_reset(arrived);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Warps: RandomResizedCrop and ElasticTransform with nearest sampling.  Every output pixel is one input pixel's bits (or
// zero), so the planes are not staged: a lane gathers straight from global memory.  What is staged is the elastic
// transform's displacement field, which all planes of a call share: every workgroup builds it in LDS from the call's Philox
// stream (noise, then two separable reflect-indexed blurs of up to 63 taps), turns it into one source index per pixel, and
// streams its planes through that table.  Building it again in every workgroup costs no launch, no workspace and no second
// reader of the counter; NOTES.md ("Image augmentation round") has the measurement.
// ---------------------------------------------------------------------------------------------------------------------
// sixteen waves: the field's blur is bound by instruction issue on the one CU that runs the workgroup, and the gather by loads
// in flight (NOTES.md, "Image augmentation round": 139 us a field with four waves at 84 x 84, 87 with sixteen)
constexpr int kWarpThreads = 1024;
constexpr int kWarpWeights = 64;         // > ASAC_IMAGE_WARP_MAX_KERNEL: one tap per lane of a wave
constexpr int kWarpTries = 10;           // torchvision's RandomResizedCrop.get_params
static_assert(ASAC_IMAGE_WARP_MAX_KERNEL < kWarpWeights, "tap table");
// the two fields and the blur's horizontal pass (later the index table), beside the static words: one workgroup on a CU
static_assert((3 * ASAC_IMAGE_MAX_PLANE + 2 * kWarpWeights + 8) * sizeof(float) <= 160 * 1024, "LDS budget");

struct WarpArgs {
    const float* x;
    float* y;
    int64_t* state;          // as ImageArgs
    double* drawn;           // counter, choice, top, left, height, width (or NULL)
    float* noise_out;        // [2][H][W] or NULL
    float* disp_out;         // [2][H][W] or NULL
    uint64_t seed;
    uint32_t instance;
    int64_t planes;
    int32_t H, W, Ho, Wo, n_ops, advance;
    uint32_t magic_w, magic_wo;
    float x_start, x_end, x_step, y_start, y_end, y_step;   // torch.linspace of the identity grid, as torch forms it
    asac_image_warp_op_t ops[ASAC_IMAGE_MAX_OPS];
};

enum : uint32_t { kTagField = 3u, kTagWindow = 4u };

// torch.linspace(start, end, n)[i] in float32: from the nearer end
__device__ __forceinline__ float warp_linspace(int i, int n, float start, float end, float step) {
    return i < n / 2 ? start + step * (float)i : end - step * (float)(n - i - 1);
}

// the normalised taps of one field's blur: k along x from sigma_x in w[0 .. k), along y from sigma_y in w[64 .. 64 + k)
__device__ __forceinline__ void warp_taps(float* w, int k, float sigma_x, float sigma_y, int tid) {
    if (tid < 2 * kWarpWeights) {
        const int j = tid & (kWarpWeights - 1);
        const float t = ((float)j - 0.5f * (float)(k - 1)) / (tid < kWarpWeights ? sigma_x : sigma_y);
        w[tid] = j < k ? expf(-0.5f * (t * t)) : 0.f;
    }
    __syncthreads();
    float sum_x = 0.f, sum_y = 0.f;
    for (int j = 0; j < k; ++j) {
        sum_x += w[j];
        sum_y += w[kWarpWeights + j];
    }
    __syncthreads();
    if (tid < 2 * kWarpWeights) w[tid] = w[tid] / (tid < kWarpWeights ? sum_x : sum_y);
    __syncthreads();
}

// One separable pass over an [H][W] plane in LDS.  A lane owns four outputs that are NEIGHBOURS ALONG THE BLUR: they share their
// source samples, so a trip computes one reflect index and one LDS read per sample (k + 3 of them) instead of per term (4 k) —
// the pass is bound by that index arithmetic, not by LDS.  Output e takes sample j with tap j - e; the taps sit in the lanes of
// one register.  The lanes of a wave make every trip together: `v_readlane` reads lanes that must not have left the loop.
// `along_x`: lines are rows, otherwise columns (neighbouring lanes then take neighbouring columns); out = (sum * mul) / div
__device__ __forceinline__ void warp_blur_pass(const float* src, float* dst, int H, int W, int k, float tap, bool along_x,
                                               float mul, float div, bool scale, int tid) {
    constexpr int E = kImgBlurOutputs;
    const int r = k >> 1;
    const int taps = __float_as_int(tap);
    const int n = along_x ? W : H, lines = along_x ? H : W;            // the extent along the blur, and across it
    const int per_line = (n + E - 1) / E, groups = per_line * lines;
    const int stride = along_x ? 1 : W;
    for (int base = 0; base < groups; base += kWarpThreads) {
        if (base + (tid & ~63) >= groups) break;                        // a whole wave past the plane leaves, as one
        const int g = min(base + tid, groups - 1);                      // (lanes past it: valid addresses, nothing stored)
        int line, p0;
        if (along_x) {
            line = g / per_line;
            p0 = (g - line * per_line) * E;
        } else {
            const int q = g / W;
            line = g - q * W;
            p0 = q * E;
        }
        const int origin = along_x ? line * W : line;
        float acc[E];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = 0.f;
        for (int j = 0; j < k + E - 1; ++j) {
            // (the samples past n - 1 + r belong to outputs past the line's end only: clamped, so that one fold stays enough)
            const float v = src[origin + image_reflect(min(p0 + j - r, n - 1 + r), n) * stride];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int t = j - e;                                    // (uniform: a scalar branch)
                const float w = t >= 0 && t < k ? __int_as_float(__builtin_amdgcn_readlane(taps, t)) : 0.f;
                acc[e] += w * v;
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (base + tid < groups && p0 + e < n) dst[origin + (p0 + e) * stride] = scale ? (acc[e] * mul) / div : acc[e];
    }
}

__global__ __launch_bounds__(kWarpThreads) void k_image_warp(const WarpArgs by_value) {
    const ASAC_KARG WarpArgs& a = *static_cast<const ASAC_KARG WarpArgs*>(kernarg_base());
    extern __shared__ __attribute__((aligned(16))) float s_field[];   // ELASTIC in the table: x field, y field, scratch
    __shared__ float s_w[2 * kWarpWeights];
    __shared__ uint64_t s_ctr;
    const int tid = (int)threadIdx.x;
    const int H = a.H, W = a.W, HW = H * W, Ho = a.Ho, Wo = a.Wo, n_out = Ho * Wo;
    const uint32_t magic_w = a.magic_w, magic_wo = a.magic_wo;
    const int64_t planes = a.planes;
    int64_t* const state = a.state;
    const uint64_t seed = a.seed;
    const uint32_t instance = a.instance;

    if (tid == 0) s_ctr = state ? (uint64_t)__hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    __syncthreads();
    const uint64_t ctr = s_ctr;

    // what the call drew: computed by every lane of every workgroup, alike
    const Philox d = image_philox(seed, instance, ctr, kTagCall, 0xFFFFFFFFu);
    const int n_ops = a.n_ops;
    const int choice = __builtin_amdgcn_readfirstlane(n_ops > 1 ? (int)__umulhi(d.c[0], (uint32_t)n_ops) : 0);
    const asac_image_warp_op_t op = karg_copy(&a.ops[choice]);
    const int kind = op.kind;
    int top = -1, left = -1, win_h = -1, win_w = -1;
    if (kind == ASAC_IMAGE_WARP_RESIZED_CROP) {
        const float area = (float)HW, log_lo = logf(op.ratio_lo), log_hi = logf(op.ratio_hi);
        bool found = false;
        for (int t = 0; t < kWarpTries && !found; t += 2) {          // one Philox block feeds two tries
            const Philox p = image_philox(seed, instance, ctr, kTagWindow, (uint32_t)(t >> 1));
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float target = area * (op.scale_lo + image_u01(p.c[2 * e]) * (op.scale_hi - op.scale_lo));
                const float aspect = expf(log_lo + image_u01(p.c[2 * e + 1]) * (log_hi - log_lo));
                const float fw = rintf(sqrtf(target * aspect)), fh = rintf(sqrtf(target / aspect));
                if (!found && fw > 0.f && fw <= (float)W && fh > 0.f && fh <= (float)H) {
                    found = true;
                    win_w = (int)fw;
                    win_h = (int)fh;
                }
            }
        }
        if (found) {
            top = (int)__umulhi(d.c[1], (uint32_t)(H - win_h + 1));
            left = (int)__umulhi(d.c[2], (uint32_t)(W - win_w + 1));
        } else {
            const float in_ratio = (float)W / (float)H;
            win_w = W;
            win_h = H;
            if (in_ratio < op.ratio_lo) win_h = (int)rintf((float)W / op.ratio_lo);
            else if (in_ratio > op.ratio_hi) win_w = (int)rintf((float)H * op.ratio_hi);
            win_h = max(1, min(win_h, H));                           // (the rule keeps them inside; rounding must not matter)
            win_w = max(1, min(win_w, W));
            top = (H - win_h) / 2;
            left = (W - win_w) / 2;
        }
    }
    if (blockIdx.x == 0 && tid == 0 && a.drawn) {
        double* const r = a.drawn;
        r[0] = (double)(int64_t)ctr;
        r[1] = (double)choice;
        r[2] = (double)top;
        r[3] = (double)left;
        r[4] = (double)win_h;
        r[5] = (double)win_w;
    }

    int* const s_index = reinterpret_cast<int*>(s_field + 2 * HW);   // ELASTIC: the source pixel of every pixel, -1: outside
    if (kind == ASAC_IMAGE_WARP_ELASTIC) {
        // the noise of both fields, four values a Philox block
        const int n_noise = 2 * HW, groups = (n_noise + 3) >> 2;
        float* const noise_out = blockIdx.x == 0 ? a.noise_out : nullptr;
        for (int g = tid; g < groups; g += kWarpThreads) {
            const Philox p = image_philox(seed, instance, ctr, kTagField, (uint32_t)g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = (g << 2) + e;
                if (i < n_noise) {
                    const float v = image_u01(p.c[e]) * 2.f - 1.f;
                    s_field[i] = v;
                    if (noise_out) noise_out[i] = v;
                }
            }
        }
        __syncthreads();
        float* const scratch = s_field + 2 * HW;
        for (int f = 0; f < 2; ++f) {
            const int k = f == 0 ? op.k0 : op.k1;
            warp_taps(s_w, k, op.sigma0, op.sigma1, tid);
            float* const field = s_field + f * HW;
            warp_blur_pass(field, scratch, H, W, k, s_w[tid & (kWarpWeights - 1)], true, 0.f, 1.f, false, tid);
            __syncthreads();
            // torchvision divides the x field by the frame's HEIGHT and the y field by its WIDTH
            warp_blur_pass(scratch, field, H, W, k, s_w[kWarpWeights + (tid & (kWarpWeights - 1))], false,
                           f == 0 ? op.alpha0 : op.alpha1, f == 0 ? (float)H : (float)W, true, tid);
            __syncthreads();
        }
        float* const disp_out = blockIdx.x == 0 ? a.disp_out : nullptr;
        for (int i = tid; i < HW; i += kWarpThreads) {
            const int yy = (int)fastdiv((uint32_t)i, (uint32_t)W, magic_w), xx = i - yy * W;
            const float dx = s_field[i], dy = s_field[HW + i];
            if (disp_out) {
                disp_out[i] = dx;
                disp_out[HW + i] = dy;
            }
            // grid_sample, align_corners=False, in torch's order of operations
            const float gx = warp_linspace(xx, W, a.x_start, a.x_end, a.x_step) + dx;
            const float gy = warp_linspace(yy, H, a.y_start, a.y_end, a.y_step) + dy;
            const float ix = rintf(((gx + 1.f) * (float)W - 1.f) / 2.f), iy = rintf(((gy + 1.f) * (float)H - 1.f) / 2.f);
            const bool inside = ix >= 0.f && ix < (float)W && iy >= 0.f && iy < (float)H;        // (false for NaN)
            s_index[i] = inside ? (int)iy * W + (int)ix : -1;
        }
        __syncthreads();
    }

    const float scale_h = (float)win_h / (float)Ho, scale_w = (float)win_w / (float)Wo;
    for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const float* const src = a.x + plane * HW;
        float* const dst = a.y + plane * (int64_t)n_out;
        if (kind == ASAC_IMAGE_WARP_ELASTIC) {
            for (int i = tid; i < HW; i += kWarpThreads) {
                const int at = s_index[i];
                dst[i] = at >= 0 ? src[at] : 0.f;
            }
        } else if (kind == ASAC_IMAGE_WARP_RESIZED_CROP) {
            const float* const win = src + top * W + left;
            for (int i = tid; i < n_out; i += kWarpThreads) {
                const int yy = (int)fastdiv((uint32_t)i, (uint32_t)Wo, magic_wo), xx = i - yy * Wo;
                const int sy = min((int)floorf((float)yy * scale_h), win_h - 1), sx = min((int)floorf((float)xx * scale_w), win_w - 1);
                dst[i] = win[sy * W + sx];
            }
        } else {
            for (int i = tid; i < HW; i += kWarpThreads) dst[i] = src[i];
        }
    }

    if (state) {
        unsigned int* const arrived = reinterpret_cast<unsigned int*>(state + 1);
        if (finish_arrive(arrived) && tid == 0) {
            if (a.advance) __hip_atomic_store(state, (int64_t)(s_ctr + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            finish_reset(arrived);
        }
    }
}

}  // namespace asac


using namespace asac;

extern "C" {

int asac_image_augment(const float* x, float* y, int64_t planes, int C, int H, int W, int Ho, int Wo, const asac_image_op_t* ops,
                       int n_ops, uint64_t seed, uint32_t instance, int64_t* state, double* drawn, void* stream) {
    if (!x || !y || !ops || planes < 1 || planes > 0x7FFFFFFF || C < 1 || planes % C != 0 || H < 1 || W < 1 || Ho < 1 || Wo < 1)
        return bad_arg("asac_image_augment");
    if (n_ops < 1 || n_ops > ASAC_IMAGE_MAX_OPS) return bad_arg("asac_image_augment: n_ops");
    if ((int64_t)H * W > ASAC_IMAGE_MAX_PLANE) return bad_arg("asac_image_augment: plane over ASAC_IMAGE_MAX_PLANE");
    if ((int64_t)Ho * Wo > 0x7FFFFFFF || planes * (((int64_t)H * W + 3) / 4) > 0xFFFFFFFFll)
        return bad_arg("asac_image_augment: size");
    bool draws = n_ops > 1;
    ImageArgs a{x, y, state, drawn, seed, instance, planes, C, H, W, Ho, Wo, n_ops, 0,
                fastdiv_magic((uint32_t)W, (uint64_t)H * W), fastdiv_magic((uint32_t)Wo, (uint64_t)Ho * Wo), {}};
    for (int i = 0; i < n_ops; ++i) {
        const asac_image_op_t& o = ops[i];
        const bool resizes = o.kind == ASAC_IMAGE_CROP_RESIZE;
        if (!resizes && (Ho != H || Wo != W)) return bad_arg("asac_image_augment: output size");
        switch (o.kind) {
        case ASAC_IMAGE_COPY:
            break;
        case ASAC_IMAGE_BLUR:
            if (o.kx < 1 || o.ky < 1 || !(o.kx & 1) || !(o.ky & 1) || o.kx > ASAC_IMAGE_MAX_KERNEL || o.ky > ASAC_IMAGE_MAX_KERNEL)
                return bad_arg("asac_image_augment: blur taps (odd, <= ASAC_IMAGE_MAX_KERNEL)");
            if (o.kx / 2 >= W || o.ky / 2 >= H) return bad_arg("asac_image_augment: blur radius reaches past the plane");
            if (!(o.lo > 0.f) || !(o.hi >= o.lo)) return bad_arg("asac_image_augment: sigma");
            draws |= o.hi > o.lo;
            break;
        case ASAC_IMAGE_BRIGHTNESS:
            if (!(o.lo >= 0.f) || !(o.hi >= o.lo)) return bad_arg("asac_image_augment: brightness");
            draws |= o.hi > o.lo;
            break;
        case ASAC_IMAGE_CROP_RESIZE:
            if (o.crop_h < 1 || o.crop_w < 1 || o.crop_h > H || o.crop_w > W || Ho < o.crop_h || Wo < o.crop_w)
                return bad_arg("asac_image_augment: crop window (the resize may not shrink it)");
            if (o.top > H - o.crop_h || o.left > W - o.crop_w) return bad_arg("asac_image_augment: crop offset");
            draws |= (o.top < 0 && o.crop_h < H) || (o.left < 0 && o.crop_w < W);
            break;
        case ASAC_IMAGE_SALT_PEPPER:
        case ASAC_IMAGE_UNIFORM_NOISE:
            draws = true;
            break;
        default:
            return bad_arg("asac_image_augment: op kind");
        }
        a.ops[i] = o;
    }
    if (draws && !state) return bad_arg("asac_image_augment: a drawing table needs its device state");
    // under the measurement repeat knob only the last repetition advances the counter: all of them draw alike
    for (int rep = 0; rep < g_launch_repeat; ++rep) {
        a.advance = rep == g_launch_repeat - 1;
        hipLaunchKernelGGL(k_image_augment, dim3((unsigned)(planes < kImgMaxGrid ? planes : kImgMaxGrid)), dim3(kImgThreads), 0,
                           as_stream(stream), a);
    }
    return finish_launch("asac_image_augment");
}

int asac_image_warp(const float* x, float* y, int64_t planes, int C, int H, int W, int Ho, int Wo,
                    const asac_image_warp_op_t* ops, int n_ops, uint64_t seed, uint32_t instance, int64_t* state, double* drawn,
                    float* noise_out, float* disp_out, void* stream) {
    if (!x || !y || !ops || planes < 1 || planes > 0x7FFFFFFF || C < 1 || planes % C != 0 || H < 1 || W < 1 || Ho < 1 || Wo < 1)
        return bad_arg("asac_image_warp");
    if (n_ops < 1 || n_ops > ASAC_IMAGE_MAX_OPS) return bad_arg("asac_image_warp: n_ops");
    if ((int64_t)H * W > ASAC_IMAGE_MAX_PLANE) return bad_arg("asac_image_warp: plane over ASAC_IMAGE_MAX_PLANE");
    if ((int64_t)Ho * Wo > 0x7FFFFFFF) return bad_arg("asac_image_warp: size");
    WarpArgs a{x, y, state, drawn, noise_out, disp_out, seed, instance, planes, H, W, Ho, Wo, n_ops, 0,
               fastdiv_magic((uint32_t)W, (uint64_t)H * W), fastdiv_magic((uint32_t)Wo, (uint64_t)Ho * Wo),
               0.f, 0.f, 0.f, 0.f, 0.f, 0.f, {}};
    // torch.linspace((1 - n) / n, (n - 1) / n, n) in float32: the ends are Python doubles, the step a float quotient
    a.x_start = (float)((double)(1 - W) / W), a.x_end = (float)((double)(W - 1) / W);
    a.y_start = (float)((double)(1 - H) / H), a.y_end = (float)((double)(H - 1) / H);
    a.x_step = W > 1 ? (a.x_end - a.x_start) / (float)(W - 1) : 0.f;
    a.y_step = H > 1 ? (a.y_end - a.y_start) / (float)(H - 1) : 0.f;
    bool draws = n_ops > 1, elastic = false;
    for (int i = 0; i < n_ops; ++i) {
        const asac_image_warp_op_t& o = ops[i];
        if (o.kind != ASAC_IMAGE_WARP_RESIZED_CROP && (Ho != H || Wo != W)) return bad_arg("asac_image_warp: output size");
        switch (o.kind) {
        case ASAC_IMAGE_WARP_COPY:
            break;
        case ASAC_IMAGE_WARP_RESIZED_CROP:
            if (!(o.scale_lo > 0.f) || !(o.scale_hi >= o.scale_lo) || !std::isfinite(o.scale_hi))
                return bad_arg("asac_image_warp: scale");
            if (!(o.ratio_lo > 0.f) || !(o.ratio_hi >= o.ratio_lo) || !std::isfinite(o.ratio_hi))
                return bad_arg("asac_image_warp: ratio");
            draws = true;
            break;
        case ASAC_IMAGE_WARP_ELASTIC:
            for (const int k : {o.k0, o.k1}) {
                if (k < 1 || !(k & 1) || k > ASAC_IMAGE_WARP_MAX_KERNEL)
                    return bad_arg("asac_image_warp: field taps (odd, <= ASAC_IMAGE_WARP_MAX_KERNEL)");
                if (k / 2 >= H || k / 2 >= W) return bad_arg("asac_image_warp: the field's blur reaches past the plane");
            }
            if (!(o.sigma0 > 0.f) || !(o.sigma1 > 0.f) || !std::isfinite(o.sigma0) || !std::isfinite(o.sigma1))
                return bad_arg("asac_image_warp: sigma");
            if (!std::isfinite(o.alpha0) || !std::isfinite(o.alpha1)) return bad_arg("asac_image_warp: alpha");
            draws = elastic = true;
            break;
        default:
            return bad_arg("asac_image_warp: op kind");
        }
        a.ops[i] = o;
    }
    if (draws && !state) return bad_arg("asac_image_warp: a drawing table needs its device state");
    // the field's LDS: 3 H W floats a workgroup.  A table with ELASTIC gets ONE workgroup per CU: building the field is bound by
    // instruction issue, so two workgroups on a CU each take twice as long over it (83 against 37 us at 30 x 30), and at
    // 84 x 84 a second one does not fit beside the first anyway
    const size_t lds = elastic ? (size_t)3 * H * W * sizeof(float) : 0;
    static bool lds_done = false;
    if (elastic && !lds_done) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_image_warp), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(3 * ASAC_IMAGE_MAX_PLANE * sizeof(float)));
        if (err != hipSuccess) {
            set_error(err, "asac_image_warp: hipFuncSetAttribute");
            return (int)err;
        }
        lds_done = true;
    }
    const int64_t cap = elastic ? kImgMaxGrid / 2 : kImgMaxGrid;
    for (int rep = 0; rep < g_launch_repeat; ++rep) {
        a.advance = rep == g_launch_repeat - 1;
        hipLaunchKernelGGL(k_image_warp, dim3((unsigned)(planes < cap ? planes : cap)), dim3(kWarpThreads), lds, as_stream(stream), a);
    }
    return finish_launch("asac_image_warp");
}

}  // extern "C"
