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

}  // extern "C"
