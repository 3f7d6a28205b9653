// Siamese representation losses (reference sac_base.py: _train_siamese_representation_learning 1633-1796), one launch each,
// loss AND gradients; the N x N logits, their labels and their cotangent live in registers only.
//
//   asac_siamese_atc_loss_grad   grid (column chunks, row tiles of 32).  A workgroup stages z = e W of its 32 rows in LDS and
//                                walks its chunk 64 target rows at a time (te staged in LDS, a wave per 16 of them).  Both
//                                products are v_mfma_f32_16x16x4_f32 and TRANSPOSED, so that the first one's result is the
//                                second one's B operand with no lane movement:
//                                    l^T[j][i]  = sum_k te[j][k] z[i][k]          (C: column i on the lane, rows j = 4 g + reg)
//                                    dz^T[c][i] = sum_j te[j][c] dl^T[j][i]       (k-step s: lane group g supplies j = 4 g + s)
//                                The label is a range test against [lo_i, lo_i + n), lo_i = (i / n) n divided ONCE per lane
//                                and workgroup.  Sums that cross workgroups are ordered (asac_ordered_finish.h), in two levels:
//                                the last chunk of a ROW TILE to arrive adds the tile's dz partials in chunk order, writes
//                                g_e = dz W^T for its rows and publishes e^T dz of the tile; the last row tile to arrive adds
//                                those in tile order into g_W, and the tiles' loss sums (each added in chunk order) in tile order.
//   asac_siamese_byol_loss_grad  a wave per group of 4 rows, at most 256 workgroups striding over the groups; the workgroups'
//                                loss sums meet in workgroup order.
// No float atomics: equal inputs give equal bits, whichever workgroup finishes last.
#include "asac_common.h"
#include "asac_ordered_finish.h"

namespace asac {
namespace siamese {

constexpr int kThreads = 256;
constexpr int kRows = 32;            // rows of e per workgroup (two MFMA tiles of 16)
constexpr int kCols = 64;            // rows of te per step (a wave each 16)
constexpr int kTargetGroups = 512;   // workgroups the (row tile x column chunk) grid aims for

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct AtcDev {
    const float *e, *te, *w, *pad;
    int32_t N, E, n, steps;          // steps: column steps of 64 per chunk
    float inv_n2;
    float *loss, *g_e, *g_w;
    float *dz_part, *gw_part, *loss_part, *tile_loss;
    unsigned int* counter;           // [row tiles] then the launch's
};

__host__ __device__ inline int row_tiles(int N) { return (N + kRows - 1) / kRows; }
// column chunks: enough workgroups to fill the chip at small N, whole steps of 64 columns each
inline int chunk_steps(int N) {
    const int steps = (N + kCols - 1) / kCols, rt = row_tiles(N);
    int chunks = (kTargetGroups + rt - 1) / rt;
    chunks = chunks < 1 ? 1 : (chunks > steps ? steps : chunks);
    return (steps + chunks - 1) / chunks;
}
inline int chunks_of(int N) {
    const int steps = (N + kCols - 1) / kCols, per = chunk_steps(N);
    return (steps + per - 1) / per;
}

// CB: 16-wide blocks of the encoder width (E <= 16 CB)
template <int CB>
__global__ __launch_bounds__(kThreads) void k_siamese_atc(const AtcDev v) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int P = CB * 16 + 1;                  // pitch: odd, the fragment reads of 16 rows hit 16 banks
    float* zs = lds;                                // [32][P]   z of the row tile, zero beyond E
    float* ts = lds + kRows * P;                    // [64][P]   te of the step, zero beyond E and beyond N
    float* red = ts;                                // [32][P]   after the walk: dz of the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, q = lane & 15;
    const int N = v.N, E = v.E, chunk = blockIdx.x, chunks = gridDim.x, tile = blockIdx.y;
    const int row0 = tile * kRows, kpad = (E + 3) & ~3;

    for (int i = tid; i < kRows * (P - 1); i += kThreads) {
        const int r = i / (P - 1), c = i - r * (P - 1), row = row0 + r;
        float z = 0.f;
        if (row < N && c < E) {
            const float* er = v.e + (int64_t)row * E;
            for (int k = 0; k < E; ++k) z = fmaf(er[k], v.w[k * E + c], z);
        }
        zs[r * P + c] = z;
    }
    // this lane's two rows (q and 16 + q of the tile): weight and label range
    float padw[2];
    int lo[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = row0 + 16 * r + q;
        padw[r] = row < N ? v.pad[row] : 0.f;
        lo[r] = row / v.n * v.n;
    }
    f32x4 dz[2][CB];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) dz[r][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float part = 0.f;

    for (int s = 0; s < v.steps; ++s) {
        const int col0 = (chunk * v.steps + s) * kCols;
        __syncthreads();                            // z (first step); the previous step's reads of ts
        for (int i = tid; i < kCols * (P - 1); i += kThreads) {
            const int r = i / (P - 1), c = i - r * (P - 1), col = col0 + r;
            ts[r * P + c] = (col < N && c < E) ? v.te[(int64_t)col * E + c] : 0.f;
        }
        __syncthreads();
        if (col0 + 16 * wave >= N) continue;        // (wave-uniform; the barriers above are reached by every wave)
        const float* tw = ts + 16 * wave * P;       // this wave's 16 target rows
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        for (int k0 = 0; k0 < kpad; k0 += 4) {
            const float a = tw[q * P + k0 + g];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, zs[q * P + k0 + g], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, zs[(16 + q) * P + k0 + g], acc[1], 0, 0, 0);
        }
        const int jcol = col0 + 16 * wave + 4 * g;  // this lane's target rows: jcol + reg
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int col = jcol + u;
                const float x = acc[r][u];
                const bool same = col >= lo[r] && col < lo[r] + v.n;
                const float t = expf(-fabsf(x)), inv = 1.f / (1.f + t);
                const float sig = x >= 0.f ? inv : t * inv;
                const float elem = fmaxf(x, 0.f) - (same ? x : 0.f) + log1pf(t);
                const bool real = col < N;
                part += real ? padw[r] * elem : 0.f;
                acc[r][u] = real ? padw[r] * (sig - (same ? 1.f : 0.f)) * v.inv_n2 : 0.f;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) {               // k-step u: lane group g supplies target row 4 g + u
            const float* trow = tw + (4 * g + u) * P + q;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const float a = trow[16 * cb];
                dz[0][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, acc[0][u], dz[0][cb], 0, 0, 0);
                dz[1][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, acc[1][u], dz[1][cb], 0, 0, 0);
            }
        }
    }
    // the four waves' dz, added in wave order in LDS: red[i][c]
    for (int w = 0; w < kThreads / 64; ++w) {
        __syncthreads();
        if (wave != w) continue;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float* at = red + (16 * r + q) * P + 16 * cb + 4 * g + u;
                    *at = w == 0 ? dz[r][cb][u] : *at + dz[r][cb][u];
                }
    }
    __syncthreads();
    float* mine = v.dz_part + ((int64_t)tile * chunks + chunk) * kRows * E;
    for (int i = tid; i < kRows * E; i += kThreads) finish_publish(mine + i, red[i / E * P + i % E]);
    const float total = block_sum_waves<kThreads>(part);
    if (tid == 0) finish_publish(v.loss_part + tile * chunks + chunk, total);
    if (!finish_arrive(v.counter + tile)) return;   // (a row tile's chunks are the grid's x extent)

    // the row tile's last chunk: dz of the tile in chunk order, its rows of g_e, its share of g_W
    float* tile_part = v.dz_part + (int64_t)tile * chunks * kRows * E;
    for (int i = tid; i < kRows * E; i += kThreads)
        red[i / E * P + i % E] = finish_sum_in_order(tile_part + i, (int64_t)kRows * E, chunks);
    __syncthreads();
    for (int i = tid; i < kRows * E; i += kThreads) {
        const int r = i / E, k = i - r * E, row = row0 + r;
        if (row >= N) continue;
        const float* wr = v.w + k * E;
        float acc = 0.f;
        for (int c = 0; c < E; ++c) acc = fmaf(red[r * P + c], wr[c], acc);
        v.g_e[(int64_t)row * E + k] = acc;
    }
    float* gw_mine = v.gw_part + (int64_t)tile * E * E;
    const int rows = min(kRows, N - row0);
    for (int i = tid; i < E * E; i += kThreads) {
        const int k = i / E, c = i - k * E;
        float acc = 0.f;
        for (int r = 0; r < rows; ++r) acc = fmaf(v.e[(int64_t)(row0 + r) * E + k], red[r * P + c], acc);
        finish_publish(gw_mine + i, acc);
    }
    if (tid == 0) {
        finish_publish(v.tile_loss + tile, finish_sum_in_order(v.loss_part + tile * chunks, 1, chunks));
        finish_reset(v.counter + tile);
    }
    if (!finish_arrive(v.counter + gridDim.y, gridDim.y)) return;

    // the launch's last row tile
    const int tiles = gridDim.y;
    for (int i = tid; i < E * E; i += kThreads) v.g_w[i] = finish_sum_in_order(v.gw_part + i, (int64_t)E * E, tiles);
    if (tid != 0) return;
    *v.loss = finish_sum_in_order(v.tile_loss, 1, tiles) * v.inv_n2;
    finish_reset(v.counter + tiles);
}

struct ByolDev {
    const float *pred, *target, *pad;
    int32_t N, P;
    float inv_n;
    float *loss, *g_pred, *partial;
    unsigned int* counter;
};

constexpr int kByolRows = 4;         // rows of a wave's group
constexpr int kByolMaxBlocks = ASAC_SIAMESE_BYOL_WORKSPACE_FLOATS - 1;
constexpr float kCosEps = 1e-8f;     // functional.cosine_similarity's default eps

// torch's cosine_similarity: (a / max(|a|, eps)) . (b / max(|b|, eps)); the clamp is applied outside autograd, so the
// gradient runs through |a| whether it was clamped or not (and is 0 through a zero norm)
__global__ __launch_bounds__(kThreads) void k_siamese_byol(const ByolDev v) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = v.P;
    const int groups = (v.N + kByolRows - 1) / kByolRows;
    float part = 0.f;                                // (equal in all lanes of a wave)
    for (int grp = blockIdx.x * (kThreads / 64) + wave; grp < groups; grp += gridDim.x * (kThreads / 64)) {
        for (int r = 0; r < kByolRows; ++r) {
            const int row = grp * kByolRows + r;
            if (row >= v.N) break;
            const float* a = v.pred + (int64_t)row * P;
            const float* b = v.target + (int64_t)row * P;
            float av[4], bv[4], aa = 0.f, bb = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = lane + 64 * u;
                av[u] = k < P ? a[k] : 0.f;
                bv[u] = k < P ? b[k] : 0.f;
                aa += av[u] * av[u];
                bb += bv[u] * bv[u];
            }
            const float na = sqrtf(wave_sum(aa)), nb = sqrtf(wave_sum(bb));
            const float ca = fmaxf(na, kCosEps), cb = fmaxf(nb, kCosEps);
            float dot = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bv[u] = bv[u] / cb;
                dot += av[u] / ca * bv[u];
            }
            dot = wave_sum(dot);                     // the row's cosine
            const float wgt = v.pad[row] * v.inv_n;
            part += v.pad[row] * dot;
            // d c / d a_k = b_k / (ca cb) - c a_k / (ca |a|): the difference is taken between numbers of size 1 (at P = 1 it
            // is exactly zero, as the derivative is)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = lane + 64 * u;
                const float unit = na > 0.f ? av[u] / na : 0.f;
                if (k < P) v.g_pred[(int64_t)row * P + k] = wgt * ((bv[u] - dot * unit) / ca);
            }
        }
    }
    __shared__ float s_wave[kThreads / 64];
    if (lane == 0) s_wave[wave] = part;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < kThreads / 64; ++w) t += s_wave[w];
        finish_publish(v.partial + blockIdx.x, t);
    }
    if (!finish_arrive(v.counter) || tid != 0) return;
    *v.loss = finish_sum_in_order(v.partial, 1, (int)gridDim.x) * v.inv_n;
    finish_reset(v.counter);
}

static bool atc_sizes_ok(int64_t N, int E, int n) {
    return E >= 1 && E <= ASAC_SIAMESE_MAX_WIDTH && n >= 1 && n <= ASAC_SIAMESE_MAX_BLOCK && N >= 1 && N <= ASAC_SIAMESE_MAX_ROWS &&
           N % n == 0;
}

}  // namespace siamese
}  // namespace asac

using namespace asac;
using namespace asac::siamese;

extern "C" {

int64_t asac_siamese_atc_workspace_floats(int64_t N, int E) {
    if (!atc_sizes_ok(N, E, 1)) return -1;
    const int64_t tiles = row_tiles((int)N), chunks = chunks_of((int)N);
    // dz partials, g_W partials, loss partials per (tile, chunk) and per tile, a counter per row tile and the launch's
    return tiles * chunks * kRows * E + tiles * E * E + tiles * chunks + tiles + tiles + 1;
}

int asac_siamese_atc_loss_grad(const float* e, const float* te, const float* w, const float* pad, int64_t N, int E, int n,
                               float* loss_out, float* g_e, float* g_w, float* workspace, void* stream) {
    if (!atc_sizes_ok(N, E, n) || !e || !te || !w || !pad || !loss_out || !g_e || !g_w || !workspace)
        return bad_arg("asac_siamese_atc_loss_grad");
    const int tiles = row_tiles((int)N), chunks = chunks_of((int)N);
    AtcDev v{};
    v.e = e, v.te = te, v.w = w, v.pad = pad;
    v.N = (int)N, v.E = E, v.n = n, v.steps = chunk_steps((int)N);
    v.inv_n2 = 1.f / ((float)N * (float)N);
    v.loss = loss_out, v.g_e = g_e, v.g_w = g_w;
    v.dz_part = workspace;
    v.gw_part = v.dz_part + (int64_t)tiles * chunks * kRows * E;
    v.loss_part = v.gw_part + (int64_t)tiles * E * E;
    v.tile_loss = v.loss_part + (int64_t)tiles * chunks;
    v.counter = reinterpret_cast<unsigned int*>(v.tile_loss + tiles);
    const dim3 grid((unsigned)chunks, (unsigned)tiles);
    const int cb = (E + 15) / 16;
    const size_t lds = sizeof(float) * (kRows + kCols);
    if (cb <= 1) ASAC_LAUNCH(k_siamese_atc<1>, grid, dim3(kThreads), lds * 17, as_stream(stream), v);
    else if (cb <= 2) ASAC_LAUNCH(k_siamese_atc<2>, grid, dim3(kThreads), lds * 33, as_stream(stream), v);
    else if (cb <= 4) ASAC_LAUNCH(k_siamese_atc<4>, grid, dim3(kThreads), lds * 65, as_stream(stream), v);
    else ASAC_LAUNCH(k_siamese_atc<8>, grid, dim3(kThreads), lds * 129, as_stream(stream), v);
    return finish_launch("asac_siamese_atc_loss_grad");
}

int asac_siamese_byol_loss_grad(const float* pred, const float* t_proj, const float* pad, int64_t N, int P, float* loss_out,
                                float* g_pred, float* workspace, void* stream) {
    if (N < 1 || N > ASAC_SIAMESE_BYOL_MAX_ROWS || P < 1 || P > ASAC_SIAMESE_BYOL_MAX_WIDTH || !pred || !t_proj || !pad ||
        !loss_out || !g_pred || !workspace)
        return bad_arg("asac_siamese_byol_loss_grad");
    ByolDev v{};
    v.pred = pred, v.target = t_proj, v.pad = pad, v.N = (int)N, v.P = P, v.inv_n = 1.f / (float)N;
    v.loss = loss_out, v.g_pred = g_pred, v.partial = workspace;
    const int64_t per = kByolRows * (kThreads / 64), want = (N + per - 1) / per;
    const int blocks = (int)(want < kByolMaxBlocks ? want : kByolMaxBlocks);
    v.counter = reinterpret_cast<unsigned int*>(workspace + kByolMaxBlocks);
    ASAC_LAUNCH(k_siamese_byol, dim3((unsigned)blocks), dim3(kThreads), 0, as_stream(stream), v);
    return finish_launch("asac_siamese_byol_loss_grad");
}

}  // extern "C"
