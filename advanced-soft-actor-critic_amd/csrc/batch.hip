// Episode batch queue for gfx950: the training mode without a replay buffer (reference algorithm/batch_buffer.py,
// utils/operators.py:105-206 `episode_to_batch`, sac_base.py:2496-2609 with use_replay_buffer=False), kept in HBM.
//
// Layout (algorithm/batch_buffer.py):
//   pool_k   [P, L, row_bytes_k]  one tensor per key, L = burn_in + n_step + 1: every live window stored once, padded
//   queue    i32[R, B]            pool slots of the queued batches (a ring of R = max_size + 1 rows)
//   head     i32[1]               absolute number of the next batch to pop (row head % R)
// The host planner decides every slot, queue row and head value; the device never decides anything.
//
//   asac_batch_put         one launch per episode: its surviving windows -> their pool slots (padded for every key),
//                          the new queue rows, the head as the host mirror computed it
//   asac_batch_pop_gather  one launch per step (captured): the B windows of queue[head % R] -> dense [B, L] batch
//                          tensors (uint8 / bool observations widened to f32 on the way)
// Work is flattened over (key, window, row, unit), unit = 16 / 4 / 1 bytes per key, like the replay gather (K3).
#include "asac_common.h"

namespace asac {

constexpr int kBatchBlock = 256;
constexpr int kBatchUnroll = 2;

struct BatchPutKeyDev {
    const uint8_t* src;        // episode rows [T] (src_stride bytes apart); NULL with ASAC_PAD_EMIT_MASK
    uint8_t* pool;             // [P, L, row_bytes]
    const uint8_t* pad_row;
    int64_t src_stride;
    int32_t row_bytes, pad_mode;
    uint32_t pad_word;
    int32_t unit_log2, units_per_row;
    uint32_t first_block;
};

struct BatchPutArgs {
    BatchPutKeyDev key[ASAC_MAX_GATHER_KEYS];
    int32_t n_keys, ep_len, burn_in, L, n_windows, pool_slots;
    const int32_t* win_start;      // [n_windows] first padded row of each window (episode row start - burn_in)
    const int32_t* win_slot;       // [n_windows] its pool slot
    const int32_t* queue_rows;     // [n_queue_rows]
    const int32_t* queue_slots;    // [n_queue_rows, B]
    int32_t n_queue_rows, batch, ring_rows;
    int32_t* queue;
    int32_t* head;
    int32_t new_head;
    uint32_t queue_block;          // the workgroup that writes the queue rows and the head
};

template <typename Unit>
__device__ __forceinline__ Unit put_pad(const BatchPutKeyDev& k, int w);
template <>
__device__ __forceinline__ uint4 put_pad<uint4>(const BatchPutKeyDev& k, int w) {
    if (k.pad_mode == ASAC_PAD_ROW) return reinterpret_cast<const uint4*>(k.pad_row)[w];
    uint32_t x = k.pad_word;
    if (k.pad_mode == ASAC_PAD_BYTE) x = (x & 0xff) * 0x01010101u;
    return make_uint4(x, x, x, x);
}
template <>
__device__ __forceinline__ uint32_t put_pad<uint32_t>(const BatchPutKeyDev& k, int w) {
    if (k.pad_mode == ASAC_PAD_ROW) return reinterpret_cast<const uint32_t*>(k.pad_row)[w];
    uint32_t x = k.pad_word;
    if (k.pad_mode == ASAC_PAD_BYTE) x = (x & 0xff) * 0x01010101u;
    return x;
}
template <>
__device__ __forceinline__ uint8_t put_pad<uint8_t>(const BatchPutKeyDev& k, int w) {
    if (k.pad_mode == ASAC_PAD_ROW) return k.pad_row[w];
    if (k.pad_mode == ASAC_PAD_WORD) return (uint8_t)(k.pad_word >> (8 * (w & 3)));
    return (uint8_t)(k.pad_word & 0xff);
}

// unit g of the key's [n_windows, L, units_per_row] destination: padded episode row start + j, or the padding value
template <typename Unit>
__device__ __forceinline__ void put_units(const BatchPutArgs& a, const BatchPutKeyDev& k, int64_t g0, int64_t total) {
    Unit val[kBatchUnroll];
    int64_t at[kBatchUnroll];
    bool live[kBatchUnroll];
#pragma unroll
    for (int r = 0; r < kBatchUnroll; ++r) {
        const int64_t g = g0 + (int64_t)r * kBatchBlock;
        live[r] = g < total;
        if (!live[r]) continue;
        const int64_t row = g / k.units_per_row;
        const int w = (int)(g - row * k.units_per_row);
        const int win = (int)(row / a.L);
        const int j = (int)(row - (int64_t)win * a.L);
        const int slot = a.win_slot[win];
        live[r] = (unsigned)slot < (unsigned)a.pool_slots;
        const int e = a.win_start[win] + j;            // episode row (negative / >= T: padding)
        at[r] = ((int64_t)slot * a.L + j) * k.row_bytes + (int64_t)w * (int)sizeof(Unit);
        val[r] = (e >= 0 && e < a.ep_len) ? reinterpret_cast<const Unit*>(k.src + (int64_t)e * k.src_stride)[w]
                                         : put_pad<Unit>(k, w);
    }
#pragma unroll
    for (int r = 0; r < kBatchUnroll; ++r)
        if (live[r]) *reinterpret_cast<Unit*>(k.pool + at[r]) = val[r];
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_put(const BatchPutArgs a) {
    if (blockIdx.x == a.queue_block) {
        // the new queue rows and the head (a vector store of the value the host mirror computed)
        const int64_t n = (int64_t)a.n_queue_rows * a.batch;
        for (int64_t i = threadIdx.x; i < n; i += kBatchBlock) {
            const int q = (int)(i / a.batch);
            const int b = (int)(i - (int64_t)q * a.batch);
            const int row = a.queue_rows[q];
            if ((unsigned)row < (unsigned)a.ring_rows) a.queue[(int64_t)row * a.batch + b] = a.queue_slots[i];
        }
        if (threadIdx.x == 0) a.head[0] = a.new_head;
        return;
    }
    int ki = 0;
#pragma unroll 1
    for (int q = 1; q < a.n_keys; ++q)
        if (blockIdx.x >= a.key[q].first_block) ki = q;
    const BatchPutKeyDev& k = a.key[ki];
    const int64_t rows = (int64_t)a.n_windows * a.L;
    const int64_t g0 = (int64_t)(blockIdx.x - k.first_block) * (kBatchBlock * kBatchUnroll) + threadIdx.x;
    if (k.pad_mode == ASAC_PAD_EMIT_MASK) {
        // padding_mask: 1 on the burn-in padding in FRONT of the episode only.  The reference builds the mask from
        // zeros_like of the already padded last_mask (operators.py:151-153), so its zero run covers the episode AND
        // burn_in + n_step - 1 rows behind it: no window reaches the trailing ones.
#pragma unroll
        for (int r = 0; r < kBatchUnroll; ++r) {
            const int64_t g = g0 + (int64_t)r * kBatchBlock;
            if (g >= rows) continue;
            const int win = (int)(g / a.L);
            const int j = (int)(g - (int64_t)win * a.L);
            const int slot = a.win_slot[win];
            if ((unsigned)slot >= (unsigned)a.pool_slots) continue;
            const int e = a.win_start[win] + j;
            k.pool[(int64_t)slot * a.L + j] = e < 0 ? 1 : 0;
        }
        return;
    }
    const int64_t total = rows * k.units_per_row;
    if (k.unit_log2 == 4) put_units<uint4>(a, k, g0, total);
    else if (k.unit_log2 == 2) put_units<uint32_t>(a, k, g0, total);
    else put_units<uint8_t>(a, k, g0, total);
}

struct BatchGatherKeyDev {
    const uint8_t* pool;       // [P, L, row_bytes]
    uint8_t* dst;              // [B, L, row_bytes] (f32: 4 x row_bytes with a conversion)
    int32_t row_bytes, convert, unit_log2, units_per_row;
    uint32_t first_block;
};

struct BatchGatherArgs {
    BatchGatherKeyDev key[ASAC_MAX_GATHER_KEYS];
    int32_t n_keys, batch, L, ring_rows, pool_slots;
    const int32_t* queue;
    const int32_t* head;
};

template <typename Unit>
__device__ __forceinline__ void pop_units(const BatchGatherArgs& a, const BatchGatherKeyDev& k, int row_slot_base,
                                          int64_t g0, int64_t total) {
    Unit val[kBatchUnroll];
    int64_t at[kBatchUnroll];
    bool live[kBatchUnroll];
#pragma unroll
    for (int r = 0; r < kBatchUnroll; ++r) {
        const int64_t g = g0 + (int64_t)r * kBatchBlock;
        live[r] = g < total;
        if (!live[r]) continue;
        const int64_t row = g / k.units_per_row;          // row of the destination [B, L]
        const int w = (int)(g - row * k.units_per_row);
        const int b = (int)(row / a.L);
        const int j = (int)(row - (int64_t)b * a.L);
        const int slot = a.queue[row_slot_base + b];
        live[r] = (unsigned)slot < (unsigned)a.pool_slots;
        at[r] = row * k.row_bytes + (int64_t)w * (int)sizeof(Unit);
        val[r] = live[r] ? reinterpret_cast<const Unit*>(k.pool + ((int64_t)slot * a.L + j) * k.row_bytes)[w] : Unit(0);
    }
#pragma unroll
    for (int r = 0; r < kBatchUnroll; ++r)
        if (live[r]) *reinterpret_cast<Unit*>(k.dst + at[r]) = val[r];
}

template <>
__device__ __forceinline__ void pop_units<uint4>(const BatchGatherArgs& a, const BatchGatherKeyDev& k, int row_slot_base,
                                                 int64_t g0, int64_t total) {
    uint4 val[kBatchUnroll];
    int64_t at[kBatchUnroll];
    bool live[kBatchUnroll];
#pragma unroll
    for (int r = 0; r < kBatchUnroll; ++r) {
        const int64_t g = g0 + (int64_t)r * kBatchBlock;
        live[r] = g < total;
        if (!live[r]) continue;
        const int64_t row = g / k.units_per_row;
        const int w = (int)(g - row * k.units_per_row);
        const int b = (int)(row / a.L);
        const int j = (int)(row - (int64_t)b * a.L);
        const int slot = a.queue[row_slot_base + b];
        live[r] = (unsigned)slot < (unsigned)a.pool_slots;
        at[r] = row * k.row_bytes + (int64_t)w * 16;
        val[r] = live[r] ? reinterpret_cast<const uint4*>(k.pool + ((int64_t)slot * a.L + j) * k.row_bytes)[w]
                         : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < kBatchUnroll; ++r)
        if (live[r]) *reinterpret_cast<uint4*>(k.dst + at[r]) = val[r];
}

// uint8 / bool -> f32: 4 source bytes -> one float4 (row_bytes % 4 == 0), else byte by byte (replay gather's rule)
__device__ __forceinline__ void pop_convert(const BatchGatherArgs& a, const BatchGatherKeyDev& k, int row_slot_base,
                                            int64_t g0, int64_t total) {
#pragma unroll
    for (int r = 0; r < kBatchUnroll; ++r) {
        const int64_t g = g0 + (int64_t)r * kBatchBlock;
        if (g >= total) continue;
        const int64_t row = g / k.units_per_row;
        const int w = (int)(g - row * k.units_per_row);
        const int b = (int)(row / a.L);
        const int j = (int)(row - (int64_t)b * a.L);
        const int slot = a.queue[row_slot_base + b];
        if ((unsigned)slot >= (unsigned)a.pool_slots) continue;
        const uint8_t* srow = k.pool + ((int64_t)slot * a.L + j) * k.row_bytes;
        float* drow = reinterpret_cast<float*>(k.dst + row * (int64_t)k.row_bytes * 4);
        if (k.unit_log2 == 2) {
            const uint32_t x = reinterpret_cast<const uint32_t*>(srow)[w];
            float4 o;
            if (k.convert == ASAC_CVT_U8_TO_F32_UNIT) {
                o = make_float4((float)(x & 0xff) / 255.f, (float)((x >> 8) & 0xff) / 255.f,
                                (float)((x >> 16) & 0xff) / 255.f, (float)(x >> 24) / 255.f);
            } else {
                o = make_float4((x & 0xff) ? 1.f : 0.f, ((x >> 8) & 0xff) ? 1.f : 0.f,
                                ((x >> 16) & 0xff) ? 1.f : 0.f, (x >> 24) ? 1.f : 0.f);
            }
            reinterpret_cast<float4*>(drow)[w] = o;
        } else {
            const uint8_t x = srow[w];
            drow[w] = (k.convert == ASAC_CVT_U8_TO_F32_UNIT) ? (float)x / 255.f : (x ? 1.f : 0.f);
        }
    }
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_pop_gather(const BatchGatherArgs a) {
    int ki = 0;
#pragma unroll 1
    for (int q = 1; q < a.n_keys; ++q)
        if (blockIdx.x >= a.key[q].first_block) ki = q;
    const BatchGatherKeyDev& k = a.key[ki];
    const int h = a.head[0];
    const int qrow = h < 0 ? 0 : h % a.ring_rows;
    const int base = qrow * a.batch;
    const int64_t total = (int64_t)a.batch * a.L * k.units_per_row;
    const int64_t g0 = (int64_t)(blockIdx.x - k.first_block) * (kBatchBlock * kBatchUnroll) + threadIdx.x;
    if (k.convert != ASAC_CVT_NONE) pop_convert(a, k, base, g0, total);
    else if (k.unit_log2 == 4) pop_units<uint4>(a, k, base, g0, total);
    else if (k.unit_log2 == 2) pop_units<uint32_t>(a, k, base, g0, total);
    else pop_units<uint8_t>(a, k, base, g0, total);
}

inline int unit_log2_of(uint64_t al) { return (al % 16 == 0) ? 4 : (al % 4 == 0) ? 2 : 0; }

}  // namespace asac

using namespace asac;

extern "C" {

int asac_batch_put(const asac_batch_put_key_t* keys_host, int n_keys, int ep_len, int burn_in, int L,
                   const int32_t* win_start, const int32_t* win_slot, int n_windows, int pool_slots,
                   const int32_t* queue_rows, const int32_t* queue_slots, int n_queue_rows, int batch,
                   int32_t* queue, int ring_rows, int32_t* head, int32_t new_head, void* stream) {
    if (n_keys <= 0 || n_keys > ASAC_MAX_GATHER_KEYS || !keys_host || ep_len < 0 || burn_in < 0 || L < 1 ||
        n_windows < 0 || pool_slots <= 0 || n_queue_rows < 0 || batch <= 0 || ring_rows <= 0 || !queue || !head)
        return bad_arg("asac_batch_put");
    if (n_windows > 0 && (!win_start || !win_slot)) return bad_arg("asac_batch_put: windows");
    if (n_queue_rows > 0 && (!queue_rows || !queue_slots)) return bad_arg("asac_batch_put: queue rows");
    BatchPutArgs a;
    a.n_keys = n_keys;
    a.ep_len = ep_len;
    a.burn_in = burn_in;
    a.L = L;
    a.n_windows = n_windows;
    a.pool_slots = pool_slots;
    a.win_start = win_start;
    a.win_slot = win_slot;
    a.queue_rows = queue_rows;
    a.queue_slots = queue_slots;
    a.n_queue_rows = n_queue_rows;
    a.batch = batch;
    a.ring_rows = ring_rows;
    a.queue = queue;
    a.head = head;
    a.new_head = new_head;
    uint64_t blocks = 0;
    const int64_t rows = (int64_t)n_windows * L;
    for (int q = 0; q < n_keys; ++q) {
        const asac_batch_put_key_t& h = keys_host[q];
        BatchPutKeyDev& d = a.key[q];
        if (!h.pool || h.row_bytes <= 0) return bad_arg("asac_batch_put: key");
        if (h.pad_mode == ASAC_PAD_EMIT_MASK) {
            if (h.row_bytes != 1) return bad_arg("asac_batch_put: mask key");
        } else if (!h.src || (h.pad_mode == ASAC_PAD_ROW && !h.pad_row) || h.pad_mode < ASAC_PAD_WORD ||
                   h.pad_mode > ASAC_PAD_ROW) {
            return bad_arg("asac_batch_put: key source / padding");
        }
        d.src = static_cast<const uint8_t*>(h.src);
        d.pool = static_cast<uint8_t*>(h.pool);
        d.pad_row = static_cast<const uint8_t*>(h.pad_row);
        d.src_stride = h.src_stride;
        d.row_bytes = h.row_bytes;
        d.pad_mode = h.pad_mode;
        d.pad_word = h.pad_word;
        const uint64_t al = reinterpret_cast<uintptr_t>(h.src) | reinterpret_cast<uintptr_t>(h.pool) |
                            reinterpret_cast<uintptr_t>(h.pad_row) | (uint64_t)h.src_stride | (uint64_t)h.row_bytes;
        d.unit_log2 = h.pad_mode == ASAC_PAD_EMIT_MASK ? 0 : unit_log2_of(al);
        d.units_per_row = h.pad_mode == ASAC_PAD_EMIT_MASK ? 1 : h.row_bytes >> d.unit_log2;
        d.first_block = (uint32_t)blocks;
        const int64_t units = rows * d.units_per_row;
        blocks += (uint64_t)((units + kBatchBlock * kBatchUnroll - 1) / (kBatchBlock * kBatchUnroll));
    }
    a.queue_block = (uint32_t)blocks;
    blocks += 1;
    if (blocks > 0x7fffffffull) return bad_arg("asac_batch_put: grid");
    ASAC_LAUNCH(k_batch_put, dim3((unsigned)blocks), dim3(kBatchBlock), 0, as_stream(stream), a);
    return finish_launch("asac_batch_put");
}

int asac_batch_pop_gather(const asac_batch_gather_key_t* keys_host, int n_keys, const int32_t* queue,
                          const int32_t* head, int ring_rows, int batch, int L, int pool_slots, void* stream) {
    if (n_keys <= 0 || n_keys > ASAC_MAX_GATHER_KEYS || !keys_host || !queue || !head || ring_rows <= 0 ||
        batch <= 0 || L < 1 || pool_slots <= 0)
        return bad_arg("asac_batch_pop_gather");
    BatchGatherArgs a;
    a.n_keys = n_keys;
    a.batch = batch;
    a.L = L;
    a.ring_rows = ring_rows;
    a.pool_slots = pool_slots;
    a.queue = queue;
    a.head = head;
    uint64_t blocks = 0;
    for (int q = 0; q < n_keys; ++q) {
        const asac_batch_gather_key_t& h = keys_host[q];
        BatchGatherKeyDev& d = a.key[q];
        if (!h.pool || !h.dst || h.row_bytes <= 0 || h.convert < ASAC_CVT_NONE || h.convert > ASAC_CVT_BOOL_TO_F32)
            return bad_arg("asac_batch_pop_gather: key");
        d.pool = static_cast<const uint8_t*>(h.pool);
        d.dst = static_cast<uint8_t*>(h.dst);
        d.row_bytes = h.row_bytes;
        d.convert = h.convert;
        const uint64_t al = reinterpret_cast<uintptr_t>(h.pool) | reinterpret_cast<uintptr_t>(h.dst) | (uint64_t)h.row_bytes;
        d.unit_log2 = unit_log2_of(al);
        if (h.convert != ASAC_CVT_NONE && d.unit_log2 == 4) d.unit_log2 = 2;   // (4 bytes in, one float4 out)
        d.units_per_row = h.row_bytes >> d.unit_log2;
        d.first_block = (uint32_t)blocks;
        const int64_t units = (int64_t)batch * L * d.units_per_row;
        blocks += (uint64_t)((units + kBatchBlock * kBatchUnroll - 1) / (kBatchBlock * kBatchUnroll));
    }
    if (blocks == 0 || blocks > 0x7fffffffull) return bad_arg("asac_batch_pop_gather: grid");
    ASAC_LAUNCH(k_batch_pop_gather, dim3((unsigned)blocks), dim3(kBatchBlock), 0, as_stream(stream), a);
    return finish_launch("asac_batch_pop_gather");
}

}  // extern "C"
