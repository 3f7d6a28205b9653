/*
 * asac_hip.h — C ABI of libasac_hip.so: the MI355X (gfx950) kernels behind the SAC training step
 * of BlueFisher/Advanced-Soft-Actor-Critic (`SAC_Base.train()`).
 *
 * The reference has no FFI: its "operator API" for this path is two Python classes
 * (SURVEY.md §8b).  Each entry point below names the reference code it replaces (file:line under
 * the reference root) — that is the binding a maintainer would route through ctypes, see
 * INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`; no ownership transfer,
 *     no allocation, no host synchronisation; re-entrant per stream (safe to capture in a hipGraph)
 *   - `stream` is a hipStream_t passed as void*
 *   - return value: 0 on success, otherwise the hipError_t of the failed launch / argument check
 *     (asac_last_error() gives text)
 *   - f32 sums, products and scans follow the reference's evaluation order; the library is built with
 *     -ffp-contract=off so no multiply-add is fused behind the reference's back.  Transcendentals are the device's
 *     (`expf`, `logf`, `tanhf`, `powf`: within a few ulp of the host's).  ONE function is an approximation by design:
 *     GELU inside the fused MLP / convolution kernels is x * Phi(x) with erf from Abramowitz-Stegun 7.1.26 (one
 *     `__expf`, one `v_rcp_f32`; csrc/asac_gelu.h) instead of ATen's erff.  Bound, against float64 GELU on [-12, 12]:
 *     |gelu - gelu64| <= 6e-7 + 3e-7 |gelu64|, |gelu' - gelu64'| <= 6e-7 (observed on MI355X: 4.6e-7 and 2.8e-7;
 *     ATen's own f32 GELU is 4.5e-7 from the same float64 values) — asserted by
 *     tests/test_kernels_gpu.py::test_gelu_against_torch through asac_gelu_eval() below
 */
#ifndef ASAC_HIP_H
#define ASAC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASAC_ABI_VERSION 91
#define ASAC_MAX_GATHER_KEYS 16
#define ASAC_MAX_ENSEMBLE 16
#define ASAC_MAX_ACTION 64
#define ASAC_MLP_MAX_BLOCKS 4

int asac_version(void);
/* sizeof of a by-value struct of this header ("asac_mlp_job_t", ...) as the library was compiled, -1 for an unknown name:
 * bindings in other languages check their mirrors of the structs against it */
int64_t asac_struct_size(const char* name);
const char* asac_last_error(void);

/* Measurement knob: every kernel launch inside an entry point is issued `repeat` times
 * back-to-back (default 1).  bench.py sets it during its profile pass so that HIP events around one
 * call resolve per-launch device time.  Returns the previous value.  Not for production use. */
int asac_set_launch_repeat(int repeat);

/* ---------------------------------------------------------------------------------------------
 * Sum tree (HBM-resident segment tree).  `tree` is the reference's array heap: f32[2C-1], root
 * at 0, leaves at [C-1, 2C-1), C a power of two.  replay_buffer.py:145-167.
 * ------------------------------------------------------------------------------------------- */

/* K1(+K2) stratified inverse-CDF sample, fused with leaf->slot->id lookup and (optionally) the
 * importance-sampling weights.
 * Replaces SumTree.sample (replay_buffer.py:185-205) + _prefetch_loop lines 347-354.
 *   u            f64[batch] uniforms in [0,1): v_i = lo_i + (hi_i-lo_i)*u_i exactly as
 *                np.random.uniform does; parity mode feeds recorded draws, fast mode device RNG
 *   slot_ids     i64[C]   DataStorage._id (id currently stored in each ring slot)
 *   beta_state   f64[1]   importance exponent; updated in place to min(1, beta+beta_increment)
 *                BEFORE use (line 353).  May be NULL together with is_weights_out.
 *   leaf_out     i32[batch] tree index of the sampled leaf        (bit-exact vs reference)
 *   p_out        f32[batch] leaf priority
 *   ids_out      i64[batch] data ids (what PrioritizedReplayBuffer.sample returns first)
 *   is_weights_out f32[batch] ((p/total)/min(p/total))^-beta, or NULL to skip (multi-GPU: use
 *                asac_per_is_weights after the cross-rank reduction)
 *   min_p_out    f32[2]  [0] = min over the batch of p (always written); [1] scratch (min ratio)
 *                of the multi-workgroup path (batch > 256)
 */
int asac_sumtree_sample(const float* tree, int capacity, int batch, const double* u,
                        const int64_t* slot_ids, double* beta_state, double beta_increment,
                        int32_t* leaf_out, float* p_out, int64_t* ids_out, float* is_weights_out,
                        float* min_p_out, void* stream);

/* The binary descent of asac_sumtree_sample alone, for n explicit f64 values (each in [0, root]): leaf index, leaf
 * priority and stored id per value; same comparisons (f64 value against f32 node sums, replay_buffer.py:196-205).
 * Used by the sharded "parity" sampling (algorithm/parallel.py): the G shard trees are the subtrees of one tree whose
 * top levels every rank walks on the host; the owner finishes the walk here with the residual values. */
int asac_sumtree_descend(const float* tree, int capacity, int n, const double* values, const int64_t* slot_ids,
                         int32_t* leaf_out, float* p_out, int64_t* ids_out, void* stream);

/* Sharded replay, "parity" sampling (no reference counterpart beyond the single tree it
 * reproduces, replay_buffer.py:172-205): the G = 2^k shard trees are the subtrees of ONE sum tree.
 *   asac_sumtree_plan_top       the k top levels: parents = left + right (f32) over the G shard roots; every sample of the
 *                               GLOBAL batch draws v = lo + (hi - lo) u over the global root and walks them with the
 *                               reference's comparisons -> owner_out i32[batch] (the shard that holds the sample),
 *                               value_out f64[batch] (the residual value its tree continues with), total_out f32[1]
 *   asac_sumtree_descend_owned  asac_sumtree_descend for the samples with owner[i] == rank; the others get leaf -1,
 *                               priority 0, id -1 (so that a SUM all-reduce of p_out over the ranks is the batch's
 *                               priorities, and update / scatter launches on ids_out skip them as stale)
 *   asac_per_is_weights_slice   IS weights of rows [first, first + count) of the global batch: minimum over all n_all
 *                               priorities, beta advanced first (352-354)
 * Everything stays on the device: with the roots all-gathered and the windows exchanged by fixed-size collectives the
 * sharded step has no host synchronisation and is captured like the plain one. */
int asac_sumtree_plan_top(const float* shard_roots, int n_shards, int batch, const double* u, int32_t* owner_out,
                          double* value_out, float* total_out, void* stream);
int asac_sumtree_descend_owned(const float* tree, int capacity, int n, const double* values, const int32_t* owner,
                               int rank, const int64_t* slot_ids, int32_t* leaf_out, float* p_out, int64_t* ids_out,
                               void* stream);
int asac_per_is_weights_slice(const float* p_all, int n_all, int first, int count, const float* total, double* beta_state,
                              double beta_increment, float* is_weights_out, void* stream);

/* K2 stand-alone: w_i = ((p_i/total)/(min_ratio))^-beta, beta_state advanced first.
 * total / min_ratio are device scalars so a cross-rank all-reduce can produce them without a
 * host round trip.  replay_buffer.py:352-354. */
int asac_per_is_weights(const float* p, int batch, const float* total, const float* min_ratio,
                        double* beta_state, double beta_increment, float* is_weights_out,
                        void* stream);

/* K6 priority update: p = clip(td, td_min, td_max)^alpha, rows whose ring slot was overwritten
 * since the sample are dropped (slot_ids[id % C] != id), duplicate ids: last one wins, then every
 * ancestor is recomputed as left+right, level by level.
 * Replaces PrioritizedReplayBuffer.update (replay_buffer.py:412-427) + SumTree.update (172-183).
 *   mode 0: td_error -> priority as above;  mode 1: `td_error` already holds priorities
 *   winner   i32[C] scratch, plus 2k more entries when k > 1024; the first C entries are all -1 on entry and are
 *            restored to -1 on exit (the tail spills per-item state when k > 1024)
 *   nan_flag i32[1] set to 1 (and nothing is written) when a td_error is NaN (lines 418-420)
 */
int asac_sumtree_update(float* tree, int capacity, int k, const int64_t* ids,
                        const int64_t* slot_ids, const float* td_error, float alpha, float td_min,
                        float td_max, int mode, int32_t* winner, int32_t* nan_flag, void* stream);

/* Episode ingress into the tree: rows [first_id, first_id+count) (ids mod 10*C) get priority
 * max_p, except the episode's last `ignore_size` rows and ring slots >= C-ignore_size which get
 * 0; slot_ids is updated; ancestors recomputed.  Replaces PrioritizedReplayBuffer.add
 * (replay_buffer.py:293-307) minus the row copy (done by the caller with async copies).
 *   max_p_dev  f32[1] device scalar (result of asac_sumtree_leaf_max) or NULL -> max_p_host */
int asac_per_add(float* tree, int capacity, int64_t first_id, int count, int ignore_size,
                 const float* max_p_dev, float max_p_host, int64_t* slot_ids, void* stream);

/* K8 max over the C leaves -> out[0].  Replaces SumTree.max (replay_buffer.py:237-239). */
int asac_sumtree_leaf_max(const float* tree, int capacity, float* out, void* stream);

/* Debug invariant: counts internal nodes with tree[i] != tree[2i+1]+tree[2i+2] into out[0]. */
int asac_sumtree_check(const float* tree, int capacity, int32_t* out, void* stream);

/* Measurement: value[i] = gelu(z[i]), deriv[i] = gelu'(z[i]) exactly as the fused MLP / convolution kernels evaluate
 * them (replaces nothing: the reference's activation is ATen's `nn.GELU()`, linear_layers.py:24-119; this exposes
 * the library's evaluation so that its distance from ATen's can be bounded by a test). */
int asac_gelu_eval(const float* z, float* value, float* deriv, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ring storage: window gather with episode-continuity padding, and predicated row scatter.
 * ------------------------------------------------------------------------------------------- */
enum {
    ASAC_PAD_KEEP = 0,      /* copy rows as stored (observations, last_mask)                     */
    ASAC_PAD_WORD = 1,      /* invalid rows: every 4-byte word := pad_word (index -1, reward 0,
                               mu_prob 1.0f, hidden 0)                                             */
    ASAC_PAD_BYTE = 2,      /* invalid rows: every byte := pad_word & 0xff (done := 1)            */
    ASAC_PAD_ROW = 3,       /* invalid rows := pad_row[0:row_bytes] (action := padding action)    */
    ASAC_PAD_EMIT_MASK = 4  /* no source: dst byte := row is invalid (the padding_mask itself)    */
};
enum {
    ASAC_CVT_NONE = 0,
    ASAC_CVT_U8_TO_F32_UNIT = 1, /* uint8 -> f32 / 255  (sac_base.py:783-786) */
    ASAC_CVT_BOOL_TO_F32 = 2     /* bool  -> f32        (sac_base.py:787-788) */
};
/* Derived keys: a sequence representation is fed the window's step indexes, padding mask and PREVIOUS actions
 * extended / shifted by one row (SAC_Base.get_bnx_data, sac_base.py:1090-1115; utils/operators.py gen_n_pre_actions);
 * a key with `derive` set delivers that form straight from the ring — the padded window row it shows is
 *   PREVIOUS         row j-1, zeros for j = 0                                  (pre_action from the action column)
 *   HOLD_LAST        row min(j, L-2)                                           (the padding mask, ASAC_PAD_EMIT_MASK)
 *   HOLD_LAST_NEXT   row min(j, L-2); at j = L-1 the i32 value + (value != -1)  (the step index)
 * — the values asac_window_aux forms from the gathered window, without its launch.  L >= 2, no conversion. */
enum { ASAC_DERIVE_NONE = 0, ASAC_DERIVE_PREVIOUS = 1, ASAC_DERIVE_HOLD_LAST = 2, ASAC_DERIVE_HOLD_LAST_NEXT = 3 };
typedef struct {
    const void* src;     /* ring [C, row_bytes]                                                   */
    void* dst;           /* [batch, L, out_row_bytes]; out_row_bytes = row_bytes (x4 if converting) */
    const void* pad_row; /* ASAC_PAD_ROW only                                                     */
    int32_t row_bytes;
    int32_t pad_mode;
    uint32_t pad_word;
    int32_t convert;
    int32_t dst_row_pitch; /* bytes between destination rows; 0 = dense (out_row_bytes).  A wider pitch lets a key
                              land as a column block of a wider [batch, L, *] tensor: the vector observation beside
                              the previous action, the concatenation a recurrent representation starts with */
    int32_t derive;        /* ASAC_DERIVE_*: which window row a destination row shows (0: its own)                */
} asac_gather_key_t;

/* K3: for every sampled id gather the rows id-prev_n .. id+post_n of every key (ring slot =
 * id mod C, negative ids wrap like NumPy's %), fused with the validity test
 *   valid(j) := j == prev_n  or  index[j] - index[prev_n] == j - prev_n
 * and the padding values.  Replaces DataStorage.get over the window ids
 * (replay_buffer.py:356-364, 64-75) + SAC_Base._sample_from_replay_buffer padding
 * (sac_base.py:2435-2453) + _process_torch_obs_list (783-788).
 *   keys_host  HOST array of n_keys descriptors (copied into the kernel argument buffer)
 *   index_ring i32[C]  the stored 'index' column */
int asac_window_gather_pad(const asac_gather_key_t* keys_host, int n_keys, const int64_t* ids,
                           int batch, int prev_n, int post_n, int capacity,
                           const int32_t* index_ring, void* stream);

/* Random reads: dst_key[r] = ring_key[ids[r] mod capacity] for every key (pad_mode ASAC_PAD_KEEP, convert
 * ASAC_CVT_NONE), any ids, no residency check, ONE launch for all keys — the reference's
 * `DataStorage.get(ids)` behind `PrioritizedReplayBuffer.get_storage_data` (replay_buffer.py:64-75, 401-406), which
 * the option-critic variant calls per key-transition hop (oc/option_selector_base.py:2205, 2223). */
/* The same gather as a PLAN in device memory (asac_window_gather_plan_bytes() bytes at plan_dev, written with a blocking
 * copy: build time, not step time) for an ASAC_SIDECAR_WINDOW_GATHER job: the windows of the batch the lookahead schedule
 * (`hip_config['lookahead']`) draws one step ahead are gathered by extra workgroups of a launch of the current step
 * (replay_buffer.py:377-396 `sample`'s `get_storage_data` part).  blocks_out: the workgroups the job needs. */
int64_t asac_window_gather_plan_bytes(void);
int asac_window_gather_plan(const asac_gather_key_t* keys_host, int n_keys, const int64_t* ids, int batch, int prev_n,
                            int post_n, int capacity, const int32_t* index_ring, void* plan_dev, int* blocks_out);

/* ... with the batch's IS weights as one more workgroup (the arguments of asac_window_gather_pad_w), for an
 * ASAC_SIDECAR_WINDOW_GATHER_W job.  plan_dev: asac_window_gather_plan_bytes() bytes. */
int asac_window_gather_plan_w(const asac_gather_key_t* keys_host, int n_keys, const int64_t* ids, int batch, int prev_n,
                              int post_n, int capacity, const int32_t* index_ring, const float* p, const float* tree,
                              double* beta_state, double beta_increment, float* is_weights_out, float* min_p_out,
                              void* plan_dev, int* blocks_out);

int asac_gather_rows(const asac_gather_key_t* keys_host, int n_keys, const int64_t* ids, int n_rows, int capacity,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Episode slabs: the agent-side episode assembly (reference algorithm/agent.py) in HBM.
 * One row mover serves every movement of an environment step, over all agents and all keys in ONE launch:
 *   commit   pending rows + this step's scalars -> slab[slot, cursor]   (Agent._add_transition, agent.py:191-235)
 *   collect  pending action / hidden state of the listed agents -> dense batch
 *                                                 (AgentManager._get_merged_action/_seq_hidden_state, 481-485)
 *   stage    policy outputs + new observations -> pending rows          (Agent.set_tmp_obs_action, 87-97)
 *   window   the last rows of the agents' running episodes, left-padded (Agent.get_episode_trans(force_length)
 *            258-316 + the concatenations of AgentManager.get_action 536-552)
 * Item i of a key copies row_bytes from  src + a*src_stride0 + b*src_stride1  to  dst + c*dst_stride0 +
 * d*dst_stride1  with (a, b) resp. (c, d) given by the side's addressing mode:
 *   ASAC_ROW_ITEM (i, 0)   ASAC_ROW_SLOT (slot[i], 0)   ASAC_ROW_SLOT_ROW (slot[i], row[i] (+ src_row_offset))
 *   ASAC_ROW_BROADCAST (0, 0; sources only)
 * A SLOT_ROW source whose row index is negative yields padding: every 4-byte word := pad_word (byte-wide keys:
 * its low byte); a SLOT_ROW destination with a negative row is skipped.  Strides in bytes. */
enum { ASAC_ROW_ITEM = 0, ASAC_ROW_SLOT = 1, ASAC_ROW_SLOT_ROW = 2, ASAC_ROW_BROADCAST = 3 };
typedef struct {
    const void* src;
    void* dst;
    int64_t src_stride0, src_stride1;
    int64_t dst_stride0, dst_stride1;
    int32_t row_bytes;
    int32_t src_mode, dst_mode;
    int32_t src_row_offset;
    uint32_t pad_word;
    int32_t reserved_;
} asac_row_move_t;

/*   keys_host  HOST array of n_keys (<= ASAC_MAX_GATHER_KEYS) descriptors (copied into the kernel arguments)
 *   slot, src_row, dst_row   i32[n_items] device arrays (each may be NULL when no key's mode reads it) */
int asac_rows_move(const asac_row_move_t* keys_host, int n_keys, const int32_t* slot, const int32_t* src_row,
                   const int32_t* dst_row, int n_items, void* stream);

/* The representation's window inputs derived from the sampled window, in one launch (SAC_Base.get_bnx_data,
 * sac_base.py:1090-1115; utils/operators.py gen_n_pre_actions with keep_last_action): for the L-1 leading
 * rows `bn` of every sampled window
 *   index_x      [B][L]    = bn indexes, then last + (last != -1)
 *   pad_x        [B][L]    = bn padding mask, then its last entry again
 *   pre_action   [B][L][A] = zeros, then the bn actions (rows pre_action_stride_t floats apart; 0 = A, dense)
 * index / padding_mask / action are the window tensors ([B][>=L-1] with the given strides in elements). */
int asac_window_aux(const int32_t* index, int64_t index_stride_b, const uint8_t* padding_mask,
                    int64_t mask_stride_b, const float* action, int64_t action_stride_b, int64_t action_stride_t,
                    int B, int L, int A, int32_t* index_x_out, uint8_t* padding_mask_x_out,
                    float* pre_action_out, int64_t pre_action_stride_t, void* stream);

/* K7: rows[s, j] -> ring[(ids[s] + first_off + j) mod C] for j in [0, count), only where
 * padding_mask[s, j] == 0 and the slot still holds that id; when several rows target one slot the
 * last in row-major (s, j) order wins (NumPy fancy-assignment order).
 * Replaces PrioritizedReplayBuffer.update_transitions (replay_buffer.py:429-434) + the target-id
 * construction in SAC_Base.train (sac_base.py:2589-2605).
 *   rows            [batch, count, row_bytes] with row stride rows_row_stride_bytes between j's
 *                   and rows_sample_stride_bytes between samples
 *   padding_mask    u8 [batch, count], strides in bytes (mask_sample_stride)
 *   winner          i32[C] scratch, all -1 on entry and on exit */
int asac_scatter_rows_if_id_match(void* ring, int row_bytes, int capacity, const int64_t* ids,
                                  int batch, int first_off, int count, const int64_t* slot_ids,
                                  const uint8_t* padding_mask, int mask_sample_stride,
                                  const void* rows, int64_t rows_sample_stride_bytes,
                                  int64_t rows_row_stride_bytes, int32_t* winner, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Return / target kernels (the non-GEMM arithmetic of _get_y, _v_trace, the Q loss).
 * ------------------------------------------------------------------------------------------- */

/* x = loc + eps*scale (Normal.rsample), a = tanh(x), and the tanh-squash-corrected log-prob
 *   logp = sum_d [ N(x_d; loc_d, scale_d).log_prob - sum_e log(max(1 - tanh(x_e)^2, 1e-2)) ]
 * (the correction is summed over the action dim and broadcast back before the final sum, as
 * operators.py:12-14,22-24 do).  Replaces sac_base.py:1346,1351(tanh),1430 and 1883-1890.
 *   loc, scale   row r at loc + r*ls_row_stride (A for dense [rows, A]; 2A when they are the two
 *                halves of the fused policy network's [rows, 2A] output)
 *   eps, a_tanh_out  dense [rows, A]; logp_out [rows]; x_out may be NULL
 *   optional, same launch: the per-dimension probability of STORED actions under the same Gaussian
 *   (see asac_squash_prob for the addressing); action == NULL skips it.  sac_base.py:1452. */
int asac_squash_sample_fwd(const float* loc, const float* scale, int64_t ls_row_stride, const float* eps,
                           int64_t rows, int A, float* a_tanh_out, float* logp_out, float* x_out,
                           const float* action, int T, int64_t action_stride_b, int64_t action_stride_t,
                           int action_offset, float* prob_out, int64_t prob_stride_b, int64_t prob_stride_t,
                           int prob_offset, void* stream);

/* Backward of the sampling part for the policy update: given dL/da_tanh [rows, A] (may be NULL) and
 * dL/dlogp [rows] (may be NULL; then, with log_alpha != NULL, the policy objective's constant
 * exp(*log_alpha) / rows is used) produce dL/dloc, dL/dscale (rows grad_row_stride floats apart, so
 * they can be the two halves of one [rows, 2A] gradient for the fused policy network). */
int asac_squash_sample_bwd(const float* loc, const float* scale, int64_t ls_row_stride, const float* eps,
                           const float* grad_a, int grad_a_members, int64_t grad_a_member_stride,
                           const float* grad_logp, const float* log_alpha, int64_t rows, int A,
                           float* grad_loc, float* grad_scale, int64_t grad_row_stride, void* stream);

/* Sidecar jobs: small, off-critical-path launches of the train step executed by EXTRA workgroups of a hosting
 * launch (asac_squash_multi, asac_mlp_forward_multi) instead of paying a dependent kernel boundary of their own.
 * A sidecar is ordered after everything launched before its host and before everything launched after it; it must
 * not touch what the host launch itself reads or writes.  Fields as the arguments of the stand-alone entry points:
 *   ASAC_SIDECAR_ALPHA_ADAM      asac_alpha_adam_step (reference sac_base.py:1913-1949)
 *   ASAC_SIDECAR_SCATTER_ELECT   pass 1 of asac_scatter_rows_if_id_match (replay_buffer.py:429-434)
 *   ASAC_SIDECAR_SCATTER_WRITE   pass 2; needs a launch boundary after the ELECT job of the same scatter
 *   ASAC_SIDECAR_WINDOW_GATHER   asac_window_gather_pad of a plan made by asac_window_gather_plan (the NEXT batch's
 *                                windows of the lookahead schedule); hosted by asac_policy_sample_q_forward only */
#define ASAC_SIDECAR_ALPHA_ADAM 1
#define ASAC_SIDECAR_SCATTER_ELECT 2
#define ASAC_SIDECAR_SCATTER_WRITE 3
#define ASAC_SIDECAR_WINDOW_GATHER 4
/*   ASAC_SIDECAR_WINDOW_GATHER_W a plan made by asac_window_gather_plan_w: the gather and, as its first workgroup, the
 *                                IS weights of the batch asac_step_prologue_sample_partial drew (asac_window_gather_pad_w
 *                                as a rider); hosted by asac_policy_sample_q_forward with ring-addressed rows only */
#define ASAC_SIDECAR_WINDOW_GATHER_W 5
#define ASAC_MAX_SIDECARS 4
typedef struct {
    int32_t kind;
    /* ALPHA_ADAM */
    const float* logp;
    int32_t B;
    float target;
    int32_t slot;
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int32_t n;
    float lr, beta1, beta2, eps;
    int64_t* steps_done;
    int32_t advance_counter;
    /* SCATTER_ELECT / SCATTER_WRITE */
    void* ring;
    int32_t row_bytes, capacity;
    const int64_t* ids;
    int32_t batch, first_off, count;
    const int64_t* slot_ids;
    const uint8_t* padding_mask;
    int32_t mask_sample_stride;
    const void* rows;
    int64_t rows_sample_stride_bytes, rows_row_stride_bytes;
    int32_t* winner;
    /* WINDOW_GATHER */
    const void* gather_plan;
    int32_t gather_blocks;
} asac_sidecar_t;

/* Up to ASAC_SQUASH_MAX_JOBS independent jobs of the two kinds above / below in ONE launch (a train
 * step samples for the target, for the policy step, for the temperature step and for the TD error, and
 * scores the stored actions, on outputs of at most two policy forwards).  Fields as the arguments of
 * asac_squash_sample_fwd; eps == NULL makes the job a probability-only job (asac_squash_prob). */
#define ASAC_SQUASH_MAX_JOBS 4
typedef struct {
    const float* loc;
    const float* scale;
    int64_t ls_row_stride;
    const float* eps;
    int64_t rows;
    int32_t A;
    int32_t T;
    float* a_tanh_out;
    float* logp_out;
    float* x_out;
    const float* action;
    int64_t action_stride_b, action_stride_t;
    float* prob_out;
    int64_t prob_stride_b, prob_stride_t;
    int32_t action_offset, prob_offset;
} asac_squash_job_t;
int asac_squash_multi(const asac_squash_job_t* jobs_host, int n_jobs, const asac_sidecar_t* sidecars_host,
                      int n_sidecars, void* stream);

/* Per-dimension tanh-squashed policy probability of STORED actions:
 *   x = atanh(clamp(a, -0.999, 0.999)); prob_d = exp(N.log_prob(x_d)) / prod_e max(1-tanh(x_e)^2, 1e-2)
 * Replaces sac_base.py:1183-1187 (get_l_probs) and 1452 (pi for V-trace); operators.py:17-19.
 *   rows = (#samples) * T;  action element (s, t, d) at
 *   s*action_stride_b + t*action_stride_t + action_offset + d (floats); prob_out likewise */
int asac_squash_prob(const float* loc, const float* scale, int64_t ls_row_stride, const float* action, int T,
                     int64_t action_stride_b, int64_t action_stride_t, int action_offset,
                     int64_t rows, int A, float* prob_out, int64_t prob_stride_b,
                     int64_t prob_stride_t, int prob_offset, void* stream);

typedef struct {
    /* target-Q table q[e][b][t], t in [0, n]: strides in floats */
    const float* q;
    int64_t q_stride_e, q_stride_b, q_stride_t;
    const int32_t* subset_n;    /* DEVICE i32[E_sample] members used for V(s_t) (randperm draw 1); NULL = 0..E_sample-1 */
    const int32_t* subset_next; /* DEVICE i32[E_sample] members used for V(s_t+1) (randperm draw 2)                     */
    int32_t E_sample;
    const float* logp;          /* [B, n+1] log pi(a'|s), contiguous                              */
    const float* log_alpha;     /* f32[1]                                                         */
    const float* reward;        /* [B, n]  row stride reward_stride (floats)                      */
    int64_t reward_stride;
    const uint8_t* done;        /* [B, n]  row stride mask_stride (bytes), same for last / pad    */
    const uint8_t* last_mask;
    const uint8_t* padding_mask;
    int64_t mask_stride;
    const float* mu_prob;       /* [B, n, A_total] behaviour probs; NULL when !use_n_step_is       */
    int64_t mu_stride_b, mu_stride_t;
    int32_t mu_offset;          /* first continuous component                                     */
    const float* pi_prob;       /* [B, >=n, A] current-policy per-dim probs (asac_squash_prob)     */
    int64_t pi_stride_b, pi_stride_t;
    int32_t A;                  /* continuous action size                                         */
    const float* gamma_ratio;   /* f32[n]  gamma^t   (torch.logspace, computed by the host once)   */
    const float* lambda_ratio;  /* f32[n]                                                         */
    float gamma, v_rho, v_c;
    int32_t use_n_step_is;
    int32_t B, n;
    /* optional fused TD error: td[b] = mean_e |q_online[e][b] - y[b]|  (sac_base.py:2233-2244)   */
    const float* q_online;      /* [E_online, B] contiguous or NULL                               */
    int32_t E_online;
    float* td_error_out;        /* f32[B] or NULL                                                 */
    float* y_out;               /* f32[B]                                                         */
} asac_vtrace_args_t;

/* K4: ensemble subset + min over E, V = minQ - alpha*logpi, pi/mu products with the reference's
 * inf/nan masking (operators.py:27-31), rho/c clipping, cumprod of c, gamma^t lambda^t, masks,
 * sum -> y[B].  One lane per batch row; the [rows x n] input slabs of a 64-row tile are staged
 * through LDS with coalesced loads.  Replaces sac_base.py:1434-1445 + 1450-1464 + _v_trace
 * (1244-1295). */
int asac_vtrace_return_min(const asac_vtrace_args_t* args_host, void* stream);
/* ... with sidecar jobs riding as extra workgroups of the launch (e.g. the write pass of the behaviour-probability
 * write-back beside the TD error's return) */
/* pending_alpha (optional): an ASAC_SIDECAR_ALPHA_ADAM job that has NOT run yet but precedes this return in the
 * reference's order (the TD error sees the updated temperature): the launch uses the value that job will write
 * (args.log_alpha must be its parameter slot); the job itself rides in a later launch (asac_sumtree_update_sc). */
int asac_vtrace_return_min_sc(const asac_vtrace_args_t* args_host, const asac_sidecar_t* sidecars_host,
                              int n_sidecars, const asac_sidecar_t* pending_alpha, void* stream);
/* The TD errors' return and the priority update that consumes them as ONE launch (asac_vtrace_return_min with
 * q_online/td_error_out set, then asac_sumtree_update mode 0 over ids[0..B) with those TD errors): the update's single
 * workgroup forms the B returns itself (bit-identical to the return kernel's) and goes on to the tree without a launch
 * boundary.  `alpha_step` (optional): an ASAC_SIDECAR_ALPHA_ADAM job that precedes the return in the reference's order
 * (sac_base.py:1913-1949 before 2182-2245) and has not run yet — the workgroup RUNS it first (args.log_alpha must be
 * its parameter slot).  Sidecar jobs ride as workgroups 1...  Replaces sac_base.py:2182-2245 + replay_buffer.py:412-427
 * for one batch; B <= 1024 and 2 B (n+2) + 2 B floats of LDS <= 128 KB.  The `winner` scratch is not touched (the
 * last-writer election among the batch's rows runs on chip). */
int asac_td_update(const asac_vtrace_args_t* args_host, float* tree, int capacity, const int64_t* ids,
                   const int64_t* slot_ids, float alpha, float td_min, float td_max, int32_t* winner, int32_t* nan_flag,
                   const asac_sidecar_t* sidecars_host, int n_sidecars, const asac_sidecar_t* alpha_step, void* stream);
/* asac_sumtree_update (declared above) with sidecar jobs riding as extra workgroups */
int asac_sumtree_update_sc(float* tree, int capacity, int k, const int64_t* ids, const int64_t* slot_ids,
                           const float* td_error, float alpha, float td_min, float td_max, int mode, int32_t* winner,
                           int32_t* nan_flag, const asac_sidecar_t* sidecars_host, int n_sidecars, void* stream);

/* Same scan with V(s_t), V(s_t+1) [B, n] and the pi / mu products [B, n] handed in directly (the
 * discrete-action branch computes its V from categorical probabilities, sac_base.py:1387-1421;
 * only reward / masks / ratios / gamma fields of `args_host` are read).  _v_trace, 1244-1295. */
int asac_vtrace_return_direct(const asac_vtrace_args_t* args_host, const float* v_n,
                              const float* v_next, const float* pi_prod, const float* mu_prod,
                              void* stream);

/* Clipped double-Q loss, forward value and gradient in one pass (sac_base.py:1539-1561):
 *   l_e = mean_b w_b * max( (tq+clamp(q-tq,-eps,eps) - y)^2, (q - y)^2 )    (eps <= 0: 2x plain MSE
 *   is NOT reproduced here; callers fall back to eager ops for clip_epsilon <= 0)
 *   q, tq: [E, B] contiguous; y, w: [B] (w may be NULL)
 *   loss_out f32[E] per-ensemble means; grad_q_out [E, B] = d(sum_e l_e)/dq */
int asac_q_loss_fwd_bwd(const float* q, const float* tq, const float* y, const float* w, int E,
                        int B, float clip_eps, float* loss_out, float* grad_q_out, void* stream);

/* Policy objective of the continuous head, value + gradients in one launch (sac_base.py:1882-1903,
 * 1910-1911):  L = mean_b(alpha*logp_b - min_{e in subset} q[e][b]);  grad_logp[b] = alpha/B;
 * grad_q[e][b] = -1/B at the first arg-min member of the subset, 0 elsewhere;  entropy_out (may be
 * NULL, needs scale [B, A], rows scale_row_stride floats apart) = mean_b sum_d (log scale + 1/2 + 1/2 log 2pi).
 *   q [E, B] contiguous; subset DEVICE i32[E_sample] or NULL (= members 0..E_sample-1) */
int asac_policy_loss_fwd_bwd(const float* logp, const float* q, const int32_t* subset, int E, int E_sample,
                             int B, const float* log_alpha, const float* scale, int64_t scale_row_stride, int A,
                             float* loss_out, float* grad_logp, float* grad_q, float* entropy_out, void* stream);

/* The offline loss' term of that objective (sac_base.py:1899-1900): *loss_inout += mean_b sum_d (u - a)^2 with
 * u = loc + eps * scale the pre-tanh sample and a the stored action; grad_u_out [N][A] (may be NULL) = 2 (u - a) / N.
 * One workgroup, fixed summation order.  loc, scale: rows ls_row_stride floats apart; eps [N][A]; off_action: rows
 * off_row_stride floats apart.  For the logged objective and the autograd path; the fused policy step forms the
 * gradient inside its own launch (the *_offline entry points below). */
int asac_policy_offline_term(const float* loc, const float* scale, int64_t ls_row_stride, const float* eps,
                             const float* off_action, int64_t off_row_stride, int N, int A, float* loss_inout,
                             float* grad_u_out, void* stream);

/* Temperature gradient of the continuous head (sac_base.py:1931-1944):
 * *grad_slot = mean_b(-logp_b) - target, where target = target_c_alpha * (-A).  grad_slot is the
 * flat-gradient element of log_c_alpha. */
int asac_alpha_grad(const float* logp, int B, float target, float* grad_slot, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused residual MLP (MFMA f32): the stock Q / policy networks as ONE launch per pass.
 * Network: x = [x0 | x1] -> n_blocks x { z = W_l x + b_l; x = GELU(z) (+ x if residual[l]) } -> up to
 * two Linear heads whose outputs are concatenated (Q: one head of 1 column; policy: mean | logstd).
 * This is reference `LinearLayers` (nn_models/layers/linear_layers.py:24-119) as composed by the
 * stock `ModelQ.c_dense` (q.py:67-91) and `ModelPolicy.c_dense / mean_dense / logstd_dense`
 * (policy.py:147-174), and as the ResBlock head of the visual encoders (`ConvLayers.dense`,
 * image_layers.py:178-216).  Block widths <= 64, total head columns <= 16; input size in0 + in1 <= 64, or
 * <= 128 for networks of at most ASAC_MLP_MAX_BLOCKS - 1 blocks whose first block is not residual (the first
 * layer then runs as two 64-column halves).  An ensemble of E
 * structurally identical networks whose parameter segments lie `member_stride` floats apart in one
 * flat buffer is evaluated by the same launch (grid.y = E).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t in0, in1;                        /* widths of the two concatenated inputs (in1 may be 0) */
    int32_t n_blocks;                        /* 1..ASAC_MLP_MAX_BLOCKS                               */
    int32_t width[ASAC_MLP_MAX_BLOCKS];      /* output width of block l                              */
    int32_t residual[ASAC_MLP_MAX_BLOCKS];   /* block adds its input (requires equal widths)         */
    int32_t head_cols[2];                    /* output columns of head 0 / head 1 (head 1 may be 0)  */
    int64_t w_off[ASAC_MLP_MAX_BLOCKS];      /* float offsets inside ONE member's parameter segment: */
    int64_t b_off[ASAC_MLP_MAX_BLOCKS];      /*   block weight [width][in] row-major, bias [width]    */
    int64_t head_w_off[2], head_b_off[2];    /*   head weight [cols][width_last], bias [cols]         */
    int32_t head_transform;                  /* 0: raw outputs; 1: Gaussian policy head — head 0 ->   */
                                             /*    5*tanh(x/5), head 1 -> exp(clamp(x, -20, 0.5))     */
                                             /*    (policy.py:170-172); backward applies the chain    */
    int32_t reserved_;
} asac_mlp_desc_t;

/* One pass of E networks over N rows: what every entry point below takes first (host memory; device pointers inside).
 *   x0 element (e, row, c) at x0 + e*x0_member_stride + row*x0_row_stride + c (member stride 0 =
 *   the same input for every ensemble member); same for x1 (NULL when in1 == 0).
 *   out[e][row][0:head_cols0+head_cols1] for e < E, row < N: written by the forward passes; the backward passes
 *   ignore it (may be NULL). */
typedef struct {
    const asac_mlp_desc_t* desc;
    const float* params;
    int64_t member_stride;
    const float* x0;
    int64_t x0_row_stride, x0_member_stride;
    const float* x1;
    int64_t x1_row_stride, x1_member_stride;
    int64_t N;
    float* out;
    int32_t E;
    /* window addressing of x0 (forward_multi / forward_multi_sampled / policy_sample_q_forward only; every other
     * entry point refuses a non-zero value): with x0_window_T > 0, row = s * T + t is read at
     * x0 + s * x0_sample_stride + t * x0_row_stride — a [samples, T, in0] view of a larger replay window
     * (states[:, b:]) without a staging copy; 0: flat rows */
    int32_t x0_window_T;
    int64_t x0_sample_stride;
} asac_mlp_job_t;

/* job->out = the networks' outputs.  Also serves first layers of 65..128 inputs (at most ASAC_MLP_MAX_BLOCKS - 1 blocks,
 * the first not residual). */
int asac_mlp_forward(const asac_mlp_job_t* job, void* stream);

/* Up to ASAC_MLP_MAX_JOBS independent forward passes (different networks and / or inputs) in ONE launch:
 * e.g. the target-Q of the stored (s, a) pairs beside the policy's forward over the window, or the online
 * and the target ensemble of the TD error. */
#define ASAC_MLP_MAX_JOBS 2
int asac_mlp_forward_multi(const asac_mlp_job_t* jobs_host, int n_jobs, const asac_sidecar_t* sidecars_host,
                           int n_sidecars, void* stream);

/* asac_mlp_forward_multi whose Gaussian-head policy jobs also run asac_squash_multi's jobs on the rows they have just
 * formed — the chain  policy forward -> [sample a ~ pi(s), log pi(a); pi(stored action); second sample at window position
 * t2]  of sac_base.py:1346-1351, 1430, 1183-1187, 1452, 2182-2245 as ONE launch: the lanes that hold a row's
 * (loc | scale) head values in MFMA layout do the elementwise work (csrc/asac_squash.h `sample_epilogue`), bit for bit
 * what asac_squash_multi writes.  epilogues[k] belongs to jobs[k]; a job without one has sample.eps == sample.action ==
 * eps2 == NULL.  In `sample`: eps / a_tanh_out / logp_out (main sample over every row), action / prob_out with their strides
 * and T (stored actions), rows (= the job's N) and A; loc / scale / ls_row_stride / x_out are unused.  A job with an epilogue:
 * E == 1, head_transform 1, 2 A <= 16.  _ok: 1 when the launch qualifies (at least one epilogue, all of them valid). */
typedef struct {
    asac_squash_job_t sample;
    const float* eps2;          /* [samples][A] or NULL: second sample from row (sample, t2) of every window */
    int32_t t2;
    int32_t reserved_;
    float* a2_out;              /* [samples][A] */
    float* logp2_out;           /* [samples] */
} asac_mlp_sample_epilogue_t;
int asac_mlp_forward_multi_sampled_ok(const asac_mlp_job_t* jobs_host, int n_jobs, const asac_mlp_sample_epilogue_t* epilogues);
int asac_mlp_forward_multi_sampled(const asac_mlp_job_t* jobs_host, int n_jobs, const asac_mlp_sample_epilogue_t* epilogues,
                                   const asac_sidecar_t* sidecars_host, int n_sidecars, void* stream);

/* Policy forward -> sampling -> critic ensemble forward over the same rows in ONE launch: the chain
 * asac_mlp_forward(_multi)[policy] -> asac_squash_multi -> asac_mlp_forward(_multi)[critics] of the return target
 * (sac_base.py:1297-1466: a' ~ pi(s_t), Q'_e(s_t, a')) and of the TD error / new behaviour probabilities (2182-2245,
 * 1159-1189), bit for bit.  A workgroup owns (16-row tile, critic e) end to end; the policy's output and the sampled
 * actions stay on chip between the three stages.
 *   pi      the policy (E = 1) over N rows (flat or window addressing); out: [N][2A] (loc | scale) or NULL
 *   sample  the main sample over every row: eps [N][A] -> a_tanh_out [N][A], logp_out [N]; with `action` also the
 *           stored actions' probabilities (fields as asac_squash_job_t; loc / scale / ls_row_stride / x_out unused)
 *   eps2    optional second sample from the same (loc | scale) at window position t2 of every sample (rows are
 *           [samples][sample.T]): eps2 [samples][A] -> a2_out [samples][A], logp2_out [samples]
 *   q       the critics (E members) on (the policy's rows, the main sample): x0 fields equal pi's, x1 ignored,
 *           out [E][N]
 * extra_jobs: up to ASAC_MLP_MAX_JOBS plain forward passes (three 64-wide blocks) riding as further workgroups;
 * sidecars as asac_mlp_forward_multi.  asac_policy_sample_q_forward_ok: 1 when `job` qualifies (both networks three
 * 64-wide blocks on <= 64 inputs, 16-byte aligned weights, scalar-head critics on (in0 | A), Gaussian-head policy).
 *
 * Ring-addressed rows (`ring`, ids != NULL): the launch reads its input rows where they lie in the replay ring instead of
 * from a gathered batch — the values asac_window_gather_pad would have delivered, bit for bit (same slot, validity test and
 * padding), so the gather of the very batch the launch works on can ride in it as an ASAC_SIDECAR_WINDOW_GATHER job.
 * Logical row r of the fused job is window row j0 + r % T of sample r / T (T = sample.T, N = batch * T):
 *   x0       the key pi.x0 / q.x0 are taken from (float32 rows of >= in0 columns; their x0 addressing is ignored)
 *   action   the key sample.action is taken from (columns action_offset .. + A), when sample.action is set
 * x_j0 >= 0: extra_jobs[0] too reads rows of the ring — one per sample, window row x_j0: x0 from key `x0`, x1 from
 * columns x_action_offset .. + in1 of key `action` (the stored pair of the clipped double-Q loss).  Keys are plain
 * float32 keys of the gather (no conversion, not derived); pad_mode ASAC_PAD_KEEP, ASAC_PAD_WORD or ASAC_PAD_ROW. */
typedef struct {
    const void* src;      /* the key's ring [capacity][row_bytes] */
    const void* pad_row;  /* ASAC_PAD_ROW only */
    int32_t row_bytes;
    int32_t pad_mode;
    uint32_t pad_word;
    int32_t reserved_;
} asac_ring_key_t;
typedef struct {
    const int64_t* ids;         /* [batch] sampled ids; NULL: rows are read as the jobs describe them */
    const int32_t* index_ring;  /* i32[capacity] the stored 'index' column */
    int32_t capacity, prev_n, L;
    int32_t j0;                 /* first window row of the fused job's rows */
    int32_t x_j0;               /* window row of extra_jobs[0]'s rows; < 0: that job reads memory as it says */
    int32_t x_action_offset;
    asac_ring_key_t x0, action;
} asac_ring_rows_t;
typedef struct {
    asac_mlp_job_t pi;
    asac_squash_job_t sample;
    const float* eps2;
    int32_t t2;
    int32_t reserved_;
    float* a2_out;
    float* logp2_out;
    asac_mlp_job_t q;
    asac_ring_rows_t ring;
} asac_pi_q_job_t;
int asac_policy_sample_q_forward_ok(const asac_pi_q_job_t* job);
/* ... and the extra jobs with it, the ring description of the first one included (x_j0, x_action_offset, one row per
 * sample): 1 exactly when asac_policy_sample_q_forward accepts the three arguments. */
int asac_policy_sample_q_forward_jobs_ok(const asac_pi_q_job_t* job, const asac_mlp_job_t* extra_jobs, int n_extra);
int asac_policy_sample_q_forward(const asac_pi_q_job_t* job, const asac_mlp_job_t* extra_jobs, int n_extra,
                                 const asac_sidecar_t* sidecars_host, int n_sidecars, void* stream);

/* asac_policy_sample_q_forward carrying the CRITIC-FORWARD RIDER: further four-wave workgroups of the same launch (a block
 * range behind the extra jobs and in front of the sidecars, one per 16-row tile and member) run the ONLINE critics'
 * forward `online_job` (stock scalar-head ensemble, E members) on the stored pair — the rows of extra job 0, read from
 * the static batch or, with ring-addressed rows, through the ring description extra job 0 uses — and save per (tile,
 * member), all 16 rows (rows >= N evaluated on zeros), what the Q-loss backward's forward recompute produces, bit for bit:
 *   save [tiles][E][6160] floats = x_1..x_3 [3][16][64] | gelu'(z_l) [3][4 waves][64 lanes][4] (the MFMA C fragment each
 *   lane holds) | raw q [16] (head bias added);  asac_critic_forward_save_floats(N, E) floats, 16-byte aligned.
 * asac_mlp_backward_qloss_return_loaded reads it.  The launch's own outputs are asac_policy_sample_q_forward's, bit for
 * bit; the rider reads nothing this launch writes.  `_ok`: what asac_policy_sample_q_forward accepts (sidecars included),
 * n_extra >= 1, an online job on extra job 0's rows whose backward runs 16-row tiles, a save buffer, and no more workgroups
 * in front of the sidecars' (the fused job's, the extra jobs', the rider's) than the device has CUs: the launch holds one
 * workgroup per CU and dispatches in block order, so beyond that the rider would wait for a second round.  The sidecars'
 * own workgroups follow in the grid and are not counted. */
int64_t asac_critic_forward_save_floats(int64_t N, int E);
int asac_policy_sample_q_forward_saving_ok(const asac_pi_q_job_t* job, const asac_mlp_job_t* extra_jobs, int n_extra,
                                           const asac_sidecar_t* sidecars_host, int n_sidecars,
                                           const asac_mlp_job_t* online_job, const float* save);
int asac_policy_sample_q_forward_saving(const asac_pi_q_job_t* job, const asac_mlp_job_t* extra_jobs, int n_extra,
                                        const asac_sidecar_t* sidecars_host, int n_sidecars, const asac_mlp_job_t* online_job,
                                        float* save, void* stream);

#define ASAC_MLP_REDUCE_OVERWRITE 0
#define ASAC_MLP_REDUCE_ACCUMULATE 1
#define ASAC_MLP_REDUCE_DEFER 2
/* floats of scratch `asac_mlp_backward` needs when parameter gradients are requested */
int64_t asac_mlp_backward_workspace(int64_t member_stride, int E, int64_t N);
/* Row tiles the backward of an [E][N] pass is cut into (16-row tiles while E * ceil(N / 16) workgroups fit one
 * resident round on the 256 CUs, else 32-row tiles): the number of per-tile partial slabs in `workspace`, i.e. the
 * `tiles` argument asac_adam_step_partials needs after an ASAC_MLP_REDUCE_DEFER backward. */
int64_t asac_mlp_backward_tiles(int64_t N, int E);

/* Backward of the pass `job` (the forward is recomputed on chip; nothing is saved between the two).
 *   grad_out     [E][N][head columns]
 *   grad_x0/x1   [E][N][in0] / [E][N][in1], written (not accumulated); either may be NULL
 *   grad_params  flat gradient buffer with the SAME layout as `params`: the tiles' partial sums are
 *                combined in a fixed order (deterministic) and, per reduce_mode, written over it
 *                (ASAC_MLP_REDUCE_OVERWRITE), added to it (ASAC_MLP_REDUCE_ACCUMULATE) or left in the
 *                workspace for asac_adam_step_partials (ASAC_MLP_REDUCE_DEFER); NULL = input
 *                gradients only
 *   workspace    asac_mlp_backward_workspace() floats (only with grad_params) */
int asac_mlp_backward(const asac_mlp_job_t* job, const float* grad_out, float* grad_x0, float* grad_x1, float* grad_params,
                      float* workspace, int reduce_mode, void* stream);

/* The Q step's loss and backward in ONE launch (sac_base.py:1539-1570 for the stock ModelQ ensemble):
 * the forward is recomputed on chip anyway, so q = Q_e(x0, x1) is formed there, the clipped double-Q
 * loss  l = max((tq + clamp(q - tq, +-clip_eps) - y)^2, (q - y)^2) * w  and d(mean_b l)/dq replace
 * grad_out, and back-propagation continues as in asac_mlp_backward (parameter gradients).
 *   target_q [E][N], y [N], weights [N] or NULL;  loss_out [E] = mean_b l  (written by the reducing
 *   launch: this call, or asac_adam_step_partials with ASAC_MLP_REDUCE_DEFER)
 *   grad_x0 [E][N][in0] or NULL: the gradient of the summed member losses w.r.t. the STATE input (one per member; the
 *   caller sums them) — a trainable representation's Q step needs no separate critic forward / loss launch
 *   (sac_base.py:1539-1570 with the representation in the graph). */
int asac_mlp_backward_qloss(const asac_mlp_job_t* job, const float* target_q, const float* y, const float* weights,
                            float clip_eps, float* loss_out, float* grad_x0, float* grad_params, float* workspace,
                            int reduce_mode, void* stream);

/* asac_mlp_backward_qloss forming its own return target (sac_base.py:1423-1464 + 1244-1295 inside 1539-1570): every
 * workgroup evaluates the n-step V-trace return `ret` describes for ITS tile's rows — the loads travel under the weight
 * staging, the per-step terms and the scan association are asac_vtrace_return_min's (bit-identical y) — so no return
 * launch precedes the Q step.  ret->y_out [N] is written as well (member 0's workgroups); ret->td_error_out must be
 * NULL, ret->B == N; grad_x0 as in asac_mlp_backward_qloss.  `_ok`: stock three-block network, n <= 16, the tile's steps
 * fit LDS (otherwise: the two launches); it reads the job's desc, params, member_stride, E and N only. */
int asac_mlp_backward_qloss_return_ok(const asac_mlp_job_t* job, const asac_vtrace_args_t* ret);
int asac_mlp_backward_qloss_return(const asac_mlp_job_t* job, const float* target_q, const asac_vtrace_args_t* ret,
                                   const float* weights, float clip_eps, float* loss_out, float* grad_x0, float* grad_params,
                                   float* workspace, int reduce_mode, void* stream);

/* asac_mlp_backward_qloss_return carrying a RIDER: further workgroups of the same launch (a second plane of its grid)
 * run the POLICY's forward on the 16-row tiles of `pi_job` (E = 1, stock three-block Gaussian-head policy on its state
 * rows x0; x1, out and the window fields unused) and save, per tile and for all 16 rows (rows >= N are evaluated on zeros),
 * what the policy's backward needs of it — the values the forward recompute inside asac_policy_step_fused produces, bit
 * for bit:   save [tiles][6400] floats = x_1..x_3 [3][16][64] | gelu'(z_l) [3][4 waves][64 lanes][4] (the MFMA C fragment
 * each lane holds) | raw head values [16][16];  tiles = ceil(pi_job->N / 16), asac_policy_forward_save_floats(N) floats,
 * 16-byte aligned.  asac_policy_step_fused_loaded reads it.  The Q job's own outputs are those of
 * asac_mlp_backward_qloss_return, bit for bit; the rider reads nothing this launch writes.
 * `_ok`: asac_mlp_backward_qloss_return_ok, the Q job on 16-row tiles, a qualifying policy job, a save buffer, and no more
 * policy tiles than the Q job has workgroups (NULL job, N <= 0, a non-stock policy or a NULL buffer: 0). */
int64_t asac_policy_forward_save_floats(int64_t N);
int asac_mlp_backward_qloss_return_rider_ok(const asac_mlp_job_t* job, const asac_vtrace_args_t* ret,
                                            const asac_mlp_job_t* pi_job, const float* save);
int asac_mlp_backward_qloss_return_rider(const asac_mlp_job_t* job, const float* target_q, const asac_vtrace_args_t* ret,
                                         const float* weights, float clip_eps, float* loss_out, float* grad_x0,
                                         float* grad_params, float* workspace, int reduce_mode, const asac_mlp_job_t* pi_job,
                                         float* save, void* stream);

/* asac_mlp_backward_qloss_return / _rider LOADING the critics' forward instead of recomputing it: `saved` is what
 * asac_policy_sample_q_forward_saving wrote for the SAME parameters and the same rows (x0 | x1) of `job` (the caller's
 * responsibility: neither may have changed in between).  The tile's x_1..x_3, gelu' fragments and raw q are requested
 * with the weights; the launch then computes what the plain form computes, bit for bit — slabs, loss, y_out.  No input
 * gradient (no grad_x0: the first layer's weights, which only that product reads, are not even fetched).
 * `_ok`: the plain form's `_ok`, 16-row tiles and a 16-byte aligned `saved`. */
int asac_mlp_backward_qloss_return_loaded_ok(const asac_mlp_job_t* job, const asac_vtrace_args_t* ret, const float* saved);
int asac_mlp_backward_qloss_return_loaded(const asac_mlp_job_t* job, const float* target_q, const asac_vtrace_args_t* ret,
                                          const float* weights, float clip_eps, float* loss_out, float* grad_params,
                                          float* workspace, int reduce_mode, const float* saved, void* stream);
int asac_mlp_backward_qloss_return_rider_loaded_ok(const asac_mlp_job_t* job, const asac_vtrace_args_t* ret,
                                                   const asac_mlp_job_t* pi_job, const float* save, const float* saved);
int asac_mlp_backward_qloss_return_rider_loaded(const asac_mlp_job_t* job, const float* target_q,
                                                const asac_vtrace_args_t* ret, const float* weights, float clip_eps,
                                                float* loss_out, float* grad_params, float* workspace, int reduce_mode,
                                                const asac_mlp_job_t* pi_job, float* save, const float* saved,
                                                void* stream);

/* The policy step's Q backward (sac_base.py:1896-1903): the gradient of mean_b(-min_{e in subset} q_e)
 * w.r.t. the ensemble outputs is formed on chip from the value table q_table [E][N] the preceding
 * asac_mlp_forward produced (-1/N at the first arg-min member of the subset, else 0) and pushed back to
 * the ACTION input only: grad_x1 [E][N][in1] (one gradient per member; asac_squash_sample_bwd sums them).
 * subset: device i32[E_sample] or NULL (= members 0..E_sample-1). */
int asac_mlp_backward_policy_q(const asac_mlp_job_t* job, const float* q_table, const int32_t* subset, int E_sample,
                               float* grad_x1, void* stream);

/* The WHOLE policy step of the stock networks with two critics in one launch (sac_base.py:1883-1906): the critics'
 * forward on (x, action), d(mean_b -min_e q_e)/dq, both critics' backward to the action, the rsample / tanh /
 * log-prob backward (dL/dlogp = exp(*log_alpha) / N) and the policy's backward — what asac_mlp_forward +
 * asac_mlp_backward_policy_q (E = E_sample = 2) + asac_mlp_backward_policy_sample compute in three launches,
 * bit for bit (same MFMA chains).  An ensemble of more than two critics with E_sample = 2 qualifies too: `subset`
 * (device i32[2], NULL = members 0, 1) names the two the objective samples — the others get no gradient from it and
 * are not evaluated; q_out is then [E][N] with those two rows written.
 * A workgroup of 8 waves owns a 16-row tile end to end; nothing but the policy's
 * per-tile parameter-gradient partials (workspace, tiles = asac_mlp_backward_tiles(N, 1); reduce_mode as above)
 * and the value table q_out [2][N] (optional) leaves the chip.
 *   x [N] rows of in0 floats (row stride x_row_stride), action [N][A] = tanh(loc + eps * scale), eps [N][A].
 *   action == NULL: the action is sampled HERE from a first run of the policy on the tile (what asac_mlp_forward +
 *   asac_squash_sample_fwd would have produced, bit for bit) and stored in a_tanh_out [N][A] with its log-probability
 *   logp_out [N] and, optionally, the policy's output ls_out [N][2A] (loc | scale).
 * asac_policy_step_fused_ok: 1 when the shapes qualify (both networks three 64-wide blocks on <= 64 inputs with
 * 16-byte aligned weights, scalar-head critics on (in0 | A), Gaussian-head policy on in0, N <= 4096). */
int asac_policy_step_fused_ok(const asac_mlp_desc_t* q_desc, const float* q_params, int64_t q_member_stride,
                              const asac_mlp_desc_t* pi_desc, const float* pi_params, int64_t pi_member_stride, int64_t N);
int asac_policy_step_fused(const asac_mlp_desc_t* q_desc, const float* q_params, int64_t q_member_stride,
                           const asac_mlp_desc_t* pi_desc, const float* pi_params, int64_t pi_member_stride,
                           const float* x, int64_t x_row_stride, int64_t N, const float* action, const float* eps,
                           const float* log_alpha, const int32_t* subset, float* q_out, float* a_tanh_out,
                           float* logp_out, float* ls_out, float* pi_grad_params, float* workspace, int reduce_mode,
                           void* stream);
/* ... with the offline loss (sac_base.py:1899-1900): the objective gains mean_b sum_d (u - a)^2, u = loc + eps * scale the
 * pre-tanh sample, a = off_action[row * off_row_stride + d] the stored action (non-NULL, off_row_stride >= A); its
 * gradient 2 (u - a) / N joins the sampling backward inside the same launch.  Bit for bit the chain with
 * asac_mlp_backward_policy_sample_offline.  asac_policy_step_fused is this entry point without the term. */
int asac_policy_step_fused_offline(const asac_mlp_desc_t* q_desc, const float* q_params, int64_t q_member_stride,
                                   const asac_mlp_desc_t* pi_desc, const float* pi_params, int64_t pi_member_stride,
                                   const float* x, int64_t x_row_stride, int64_t N, const float* action, const float* eps,
                                   const float* log_alpha, const int32_t* subset, const float* off_action,
                                   int64_t off_row_stride, float* q_out, float* a_tanh_out, float* logp_out, float* ls_out,
                                   float* pi_grad_params, float* workspace, int reduce_mode, void* stream);

/* asac_policy_step_fused (action given) LOADING the policy's forward instead of running it again behind the critics:
 * `saved` is what the rider of asac_mlp_backward_qloss_return_rider wrote for the SAME policy parameters and the same N
 * rows x (the caller's responsibility: neither may have changed in between).  The tile's saved values are requested with
 * the weights and parked in LDS beside the critics; the launch then computes what asac_policy_step_fused computes, bit for
 * bit.  action must not be NULL.  `_ok`: asac_policy_step_fused_ok and a 16-byte aligned `saved`. */
int asac_policy_step_fused_loaded_ok(const asac_mlp_desc_t* q_desc, const float* q_params, int64_t q_member_stride,
                                     const asac_mlp_desc_t* pi_desc, const float* pi_params, int64_t pi_member_stride, int64_t N,
                                     const float* saved);
int asac_policy_step_fused_loaded(const asac_mlp_desc_t* q_desc, const float* q_params, int64_t q_member_stride,
                                  const asac_mlp_desc_t* pi_desc, const float* pi_params, int64_t pi_member_stride,
                                  const float* x, int64_t x_row_stride, int64_t N, const float* action, const float* eps,
                                  const float* log_alpha, const int32_t* subset, const float* saved, float* q_out,
                                  float* pi_grad_params, float* workspace, int reduce_mode, void* stream);
int asac_policy_step_fused_loaded_offline(const asac_mlp_desc_t* q_desc, const float* q_params, int64_t q_member_stride,
                                          const asac_mlp_desc_t* pi_desc, const float* pi_params, int64_t pi_member_stride,
                                          const float* x, int64_t x_row_stride, int64_t N, const float* action,
                                          const float* eps, const float* log_alpha, const int32_t* subset,
                                          const float* off_action, int64_t off_row_stride, const float* saved, float* q_out,
                                          float* pi_grad_params, float* workspace, int reduce_mode, void* stream);

/* The policy step's policy backward (sac_base.py:1883-1906, stock Gaussian-head ModelPolicy): the
 * gradient of the objective w.r.t. (loc | scale) — asac_squash_sample_bwd's math with dL/dlogp =
 * exp(*log_alpha) / N and dL/da = sum over grad_a_members of grad_a [m][N][A] — is formed on chip from the
 * forward the backward recomputes, then back-propagated (parameter gradients only; reduce_mode as above).
 * The pass is one policy on its state rows: job->E == 1, job->x1 == NULL. */
int asac_mlp_backward_policy_sample(const asac_mlp_job_t* job, const float* eps, const float* grad_a, int grad_a_members,
                                    const float* log_alpha, float* grad_params, float* workspace, int reduce_mode,
                                    void* stream);
/* ... with the offline loss' term 2 (u - a) / N added to the gradient at the pre-tanh sample u, a =
 * off_action[row * off_row_stride + d] (non-NULL, off_row_stride >= A). */
int asac_mlp_backward_policy_sample_offline(const asac_mlp_job_t* job, const float* eps, const float* grad_a,
                                            int grad_a_members, const float* log_alpha, const float* off_action,
                                            int64_t off_row_stride, float* grad_params, float* workspace, int reduce_mode,
                                            void* stream);

/* floats of one member's parameter block that the network actually uses (<= member_stride) */
int64_t asac_mlp_param_extent(const asac_mlp_desc_t* desc_host);

/* Gaussian policy head bounding (policy.py:170-172): loc = 5*tanh(mean/5),
 * scale = exp(clamp(logstd, -20, 0.5)); raw = [rows][2A] (mean | logstd).  Backward: graw from
 * gloc / gscale (either may be NULL). */
int asac_gauss_head_fwd(const float* raw, int64_t rows, int A, float* loc, float* scale, void* stream);
int asac_gauss_head_bwd(const float* raw, const float* grad_loc, const float* grad_scale,
                        int64_t rows, int A, float* grad_raw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused GRU stack over a padded window (the RNN burn-in, sac_base.py:1117-1146 `get_l_states`
 * through nn_models/layers/seq_layers.py:14-114 `GRU`): nn.GRU(batch_first=True) cell semantics,
 * gate order (r, z, n).  Padding as in that layer: steps before the first unpadded step are skipped
 * (state untouched), later steps all run, and the output of every padded step is zero.  One launch
 * per pass instead of one MIOpen launch per time step.
 *   w_ih/w_hh/b_ih/b_hh  HOST arrays of `layers` device pointers: [3H][I_l], [3H][H], [3H], [3H]
 *   x             [B][L][input] with strides (floats) x_stride_b / x_stride_t
 *   h0            [B][layers][H] with batch stride h0_stride_b floats, or NULL (zeros)
 *   padding_mask  [B][L] bytes, row stride mask_stride_b, or NULL
 *   hn_out        [B][L][layers][H]   every layer's output at every step (top layer = the output;
 *                                     the state after the last valid step = next hidden state)
 *   out_top       [B][L][H]           the top layer's output once more, dense (may be NULL)
 *   gates_out     [B][L][layers][5H]  (r, z, n, W_hn h + b_hn, unmasked state) saved for backward;
 *                                     NULL = inference
 * Limits: input, hidden <= ASAC_GRU_MAX_DIM, layers <= ASAC_GRU_MAX_LAYERS, hidden_pow2 = hidden
 * rounded up to a power of two; anything else returns ASAC_ERR_BAD_ARG (callers keep their own
 * generic path for such cells).
 * ------------------------------------------------------------------------------------------- */
#define ASAC_GRU_MAX_LAYERS 2
#define ASAC_GRU_MAX_DIM 16
typedef struct {
    int32_t input, hidden, hidden_pow2, layers;
} asac_gru_desc_t;

/* floats of the packed parameter-gradient buffer: per layer w_ih | w_hh | b_ih | b_hh */
int64_t asac_gru_param_count(const asac_gru_desc_t* desc_host);
int64_t asac_gru_backward_workspace(const asac_gru_desc_t* desc_host, int B);

int asac_gru_forward(const asac_gru_desc_t* desc_host, const float* const* w_ih, const float* const* w_hh,
                     const float* const* b_ih, const float* const* b_hh, const float* x,
                     int64_t x_stride_b, int64_t x_stride_t, const float* h0, int64_t h0_stride_b,
                     const uint8_t* padding_mask, int64_t mask_stride_b, int B, int L, float* hn_out,
                     float* out_top, float* gates_out, void* stream);

/* The same launch with a SECOND parameter set run over the same window for inference: the target
 * representation's pass beside the online one's (sac_base.py:2066-2079 calls `get_l_states` for `model_rep`
 * and then for `model_target_rep` on identical inputs).  twin_hn_out [B][L][layers][H], twin_out_top [B][L][H]
 * (may be NULL); the twin saves no activations.  Values are those of two asac_gru_forward calls. */
int asac_gru_forward_twin(const asac_gru_desc_t* desc_host, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, const float* const* twin_w_ih,
                          const float* const* twin_w_hh, const float* const* twin_b_ih,
                          const float* const* twin_b_hh, const float* x, int64_t x_stride_b, int64_t x_stride_t,
                          const float* h0, int64_t h0_stride_b, const uint8_t* padding_mask,
                          int64_t mask_stride_b, int B, int L, float* hn_out, float* out_top, float* gates_out,
                          float* twin_hn_out, float* twin_out_top, void* stream);

/* BPTT of the above.  grad_hn [B][L][layers][H] (gradient w.r.t. hn_out) and grad_top [B][L][H]
 * (gradient w.r.t. out_top) may each be NULL; grad_x [B][L][input] and grad_h0 [B][layers][H] are
 * written (either may be NULL).  Parameter gradients, summed in a fixed order: either WRITTEN packed into
 * grad_params (asac_gru_param_count floats), or written / added (accumulate != 0) straight into the 4*layers
 * tensors grad_param_tensors points at (HOST array of device pointers: w_ih, w_hh, b_ih, b_hh per layer) —
 * exactly one of the two is non-NULL. */
int asac_gru_backward(const asac_gru_desc_t* desc_host, const float* const* w_ih, const float* const* w_hh,
                      const float* const* b_ih, const float* const* b_hh, const float* x,
                      int64_t x_stride_b, int64_t x_stride_t, const float* h0, int64_t h0_stride_b,
                      const uint8_t* padding_mask, int64_t mask_stride_b, int B, int L, const float* hn,
                      const float* gates, const float* grad_hn, const float* grad_top, float* grad_x,
                      float* grad_h0, float* grad_params, float* const* grad_param_tensors, int accumulate,
                      float* workspace, void* stream);

/* BPTT from ONE window position: the loss reads the representation's state at a single step of the window
 * (SAC_Base._train_rep_q takes `m_states[:, burn_in_step]`, sac_base.py:2104-2110, everything behind it only feeds
 * detached targets), and E critics each hand back d loss / d state there.  The gradient of out_top is
 * sum_e grad_top_members[e][b][:] (summed in member order) at `position` and zero elsewhere, grad_hn is zero — the
 * values asac_gru_backward returns for that dense gradient, bit for bit, but the recursion starts AT the position
 * (the steps behind it carry zeros) and no [B][L][H] gradient tensor is formed or read.
 *   grad_top_members [members][B][H];  0 <= position < L;  grad_x (when asked for) is zero behind the position.
 *   adam (may be NULL; grad_param_tensors form only): the launch that finishes the parameter gradients also takes the
 *   optimizer step of those parameters — the representation's `optimizer_rep.step()` (sac_base.py:1601-1603) without a
 *   launch of its own. */
typedef struct {
    float* param_base;          /* the parameter whose gradient is grad_base[k] is param_base[k] ...             */
    const float* grad_base;     /* ... (the learner's flat buffers: every grad_param_tensors entry points inside) */
    float* exp_avg_base;        /* Adam moments at the same offsets                                              */
    float* exp_avg_sq_base;
    float lr, beta1, beta2, eps;
    const int64_t* steps_done;  /* device counter; the update uses step *steps_done + 1 and does not advance it  */
} asac_adam_epilogue_t;
int asac_gru_backward_at(const asac_gru_desc_t* desc_host, const float* const* w_ih, const float* const* w_hh,
                         const float* const* b_ih, const float* const* b_hh, const float* x,
                         int64_t x_stride_b, int64_t x_stride_t, const float* h0, int64_t h0_stride_b,
                         const uint8_t* padding_mask, int64_t mask_stride_b, int B, int L, const float* hn,
                         const float* gates, const float* grad_top_members, int members, int position,
                         float* grad_x, float* grad_h0, float* grad_params, float* const* grad_param_tensors,
                         int accumulate, const asac_adam_epilogue_t* adam, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GRU recurrence for hidden sizes 32 / 64 / 128 on f32 MFMA (csrc/gru_wide.hip): the time loops of ONE layer of the
 * plugin layer `GRU` (nn_models/layers/seq_layers.py:14-114; `m.GRU(…, 64, 1)` envs/square/memory_corridor/nn.py:19,
 * `m.GRU(…, 128, 1)` envs/uav/uav_hole/nn.py:22) under `get_l_states` (sac_base.py:1117-1146).  The batched products
 * around them are library GEMMs on the host side (algorithm/fused_gru_wide.py): gi = x W_ih^T + b_ih before, dW_ih =
 * dgi^T x, dW_hh = dgh^T h_prev, dx = dgi W_ih and the bias sums after.
 *   forward : gi [B][L][3H] (strides in floats), w_hh [3H][H], b_hh [3H], h0 [B][H] (row stride) or NULL, padding_mask
 *             [B][L] bytes or NULL -> out (the masked output, strided: may be a layer's slice of hn [B][L][layers][H]),
 *             h_raw [B][L][H] (the unmasked state after every step) and gates [B][L][4H] (r | z | n | W_hn h + b_hn): both
 *             saved for the backward, both or neither NULL.  Padding as asac_gru_forward: steps before a row's first
 *             unpadded one are skipped (state held), the output of a padded step is 0.
 *   backward: grad_out [B][L][H] (gradient of the masked output, strided), w_hh_t [H][3H] = W_hh^T -> grad_gi, grad_gh
 *             [B][L][3H] (gradients of gi and of W_hh h + b_hh; zero where a step did not run), grad_h0 [B][H] or NULL.
 * Every pointer 16-byte aligned, every stride a multiple of 4 floats.  Deterministic (no atomics).
 * ------------------------------------------------------------------------------------------- */
int asac_gru_wide_supported(int hidden);
int asac_gru_wide_forward(const float* gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* w_hh, const float* b_hh,
                          const float* h0, int64_t h0_stride_b, const uint8_t* padding_mask, int64_t mask_stride_b, int B,
                          int L, int hidden, float* out, int64_t out_stride_b, int64_t out_stride_t, float* h_raw,
                          float* gates, void* stream);
/* Twin form: the same B windows under TWO networks' recurrent weights in one launch (the online representation and its target
 * copy over the sampled windows, reference sac_base.py:2066-2079): gi / out hold 2B rows (network 1 then network 2),
 * h0 / padding_mask B rows (shared), h_raw / gates B rows (network 1 only: the target pass is not differentiated).  B % 16 == 0. */
int asac_gru_wide_forward_twin(const float* gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* w_hh, const float* b_hh,
                               const float* w_hh_twin, const float* b_hh_twin, const float* h0, int64_t h0_stride_b,
                               const uint8_t* padding_mask, int64_t mask_stride_b, int B, int L, int hidden, float* out,
                               int64_t out_stride_b, int64_t out_stride_t, float* h_raw, float* gates, void* stream);
int asac_gru_wide_backward(const float* grad_out, int64_t go_stride_b, int64_t go_stride_t, const float* w_hh_t,
                           const float* gates, const float* h_raw, const float* h0, int64_t h0_stride_b,
                           const uint8_t* padding_mask, int64_t mask_stride_b, int B, int L, int hidden, float* grad_gi,
                           float* grad_gh, float* grad_h0, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused two-layer convolution stack: Conv2d(C->out1, kernel1, stride1) GELU Conv2d(out1->out2, kernel2,
 * stride2) GELU (no padding, square kernels) over N small frames — the `simple` visual encoder
 * (nn_models/layers/image_layers.py:70-80) that `get_l_states` (sac_base.py:1117-1146) applies to every
 * frame of the sampled windows, three times per train step.  One launch per pass.
 *   x  [N][C][H][W];  w1 [out1][C][k1][k1], b1 [out1];  w2 [out2][out1][k2][k2], b2 [out2]  (nn.Conv2d layout)
 *   y  [N][out2*H2*W2]  = the second activation map flattened channel-major (what `.reshape(N, -1)` of the NCHW
 *      map gives)
 *   z1_out [N][H1*W1][out1], z2_out [N][out2*H2*W2]: pre-activations saved for the backward (both or neither)
 * Backward: gradients of the four parameter tensors only (frames are data), packed w1 | b1 | w2 | b2 into
 * grad_params (asac_conv2_param_count floats; written, or added with accumulate != 0 — the layout of the
 * parameters' gradient views inside the learner's flat buffer), summed in a fixed order; workspace of
 * asac_conv2_backward_workspace floats.
 * Limits (asac_conv2_supported): out1 <= 16, out2 <= 32, C*k1*k1 and out1*k2*k2 multiples of 16 and
 * <= ASAC_CONV2_MAX_K, H2*W2 a divisor of 16, a group of 16/(H2*W2) frames within the LDS budget; anything else
 * returns ASAC_ERR_BAD_ARG and callers keep their generic path.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_CONV2_MAX_K 256
typedef struct {
    int32_t channels, height, width;
    int32_t out1, kernel1, stride1;
    int32_t out2, kernel2, stride2;
} asac_conv2_desc_t;

int asac_conv2_supported(const asac_conv2_desc_t* desc_host);
/* Frames whose second-layer map has more than 16 positions (the 84 x 84 frames of the reference's environments:
 * ConvLayers(84, 84, C, 'simple'), 20 x 20 -> 9 x 9, envs/roller/nn_visual_hard_attn.py) run TILED: asac_conv2_tiles(desc)
 * blocks of <= 16 positions per frame, each formed from the crop of the frame it needs (csrc/conv.hip).  Same results;
 * z1_out then holds asac_conv2_z1_floats(desc, N) floats (the crops' first-layer pre-activations, not the frame's map:
 * per block, or — where the forward works by rows of blocks — per row of blocks; an opaque buffer between the two passes). */
int asac_conv2_tiles(const asac_conv2_desc_t* desc_host);
int64_t asac_conv2_z1_floats(const asac_conv2_desc_t* desc_host, int64_t N);
int64_t asac_conv2_param_count(const asac_conv2_desc_t* desc_host);
int64_t asac_conv2_backward_workspace(const asac_conv2_desc_t* desc_host, int64_t N);
/* partial slabs (one per workgroup, n_cot x the packed parameter count floats each) a backward launch over N frames with
 * n_cot cotangents leaves in its workspace — what asac_sum_partials_multi sums after accumulate == ASAC_CONV_SUM_DEFER */
int asac_conv2_backward_slabs(const asac_conv2_desc_t* desc_host, int64_t N, int n_cot);
int asac_conv2_forward(const asac_conv2_desc_t* desc_host, const float* x, int64_t N, const float* w1,
                       const float* b1, const float* w2, const float* b2, float* y, float* z1_out, float* z2_out,
                       void* stream);
/* The same forward over a SLICE of the sampled windows read where it lies: x points at frame [0][b] of a
 * [B][L][C][H][W] batch, a sample's frames_per_sample frames are consecutive, samples sample_stride floats apart
 * (N = B * frames_per_sample).  A representation without a sequence encoder only needs the states of the positions
 * behind the burn-in before its update (sac_base.py:2066-2103: `m_states[:, burn_in_step:]`), so those two passes skip
 * the burn-in frames without a copy.  frames_per_sample must be a multiple of asac_conv2_group_frames(desc) (a
 * workgroup's frames then never straddle two samples); anything else returns ASAC_ERR_BAD_ARG (callers copy). */
int asac_conv2_group_frames(const asac_conv2_desc_t* desc_host);
int asac_conv2_forward_windows(const asac_conv2_desc_t* desc_host, const float* x, int64_t N, int frames_per_sample,
                               int64_t sample_stride, const float* w1, const float* b1, const float* w2, const float* b2,
                               float* y, float* z1_out, float* z2_out, void* stream);
/* ... and the backward of such a pass: x addressed the same way, z1 / z2 / grad_y dense over the N frames. */
int asac_conv2_backward_windows(const asac_conv2_desc_t* desc_host, const float* x, int64_t N, int frames_per_sample,
                                int64_t sample_stride, const float* w2, const float* z1, const float* z2,
                                const float* grad_y, float* grad_params, int accumulate, float* workspace, void* stream);

/* Several backward walks of ONE forward pass as one launch: the reference differentiates the representation's graph once per
 * gated auxiliary loss (`calculate_adaptive_weights`, sac_base.py:1607-1631, called from 1798-1839) — the same frames, the same
 * saved pre-activations, n_cot (1..4) different output gradients grad_ys[c] [N][out2 * M2].  What does not depend on the
 * cotangent (the frames' staging, the activations, the gathered patch operands of both weight-gradient products) is done once
 * per group of frames.  grads_out [n_cot][asac_conv2_param_count]: cotangent c's packed gradients w1 | b1 | w2 | b2, bit-identical
 * to asac_conv2_backward_windows(..., grad_ys[c], ...); workspace: n_cot x asac_conv2_backward_workspace floats.  More
 * cotangents than asac_conv2_backward_multi_max (their LDS buffers beside the double-buffered frames: 3 for 30 x 30 frames)
 * go in launches of at most that many. */
int asac_conv2_backward_multi_max(const asac_conv2_desc_t* desc);     /* cotangents ONE launch takes for these frames (1..3) */
int asac_conv2_backward_multi(const asac_conv2_desc_t* desc, const float* x, int64_t N, int frames_per_sample,
                              int64_t sample_stride, const float* w2, const float* z1, const float* z2,
                              const float* const* grad_ys, int n_cot, float* grads_out, int accumulate, float* workspace,
                              void* stream);
int asac_conv2_backward(const asac_conv2_desc_t* desc_host, const float* x, int64_t N, const float* w2,
                        const float* z1, const float* z2, const float* grad_y, float* grad_params, int accumulate,
                        float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One-launch 1-D convolution stack over rays: Conv1d(C -> out1, k1, s1) LeakyReLU Conv1d(out1 -> out2, k2, s2) LeakyReLU,
 * no padding, dilation 1, groups 1 — the `default` stack of `Conv1dLayers` (nn_models/layers/image_layers.py; the
 * reference's ray-sensor encoders with 400 and 61 rays of 2 channels).  csrc/conv1d.hip, f32 MFMA 16x16x4.
 *   x  [N][L][C]              rays as stored, channels LAST (the module's permute(0, 2, 1) is folded in)
 *   w1 [out1][C][k1], b1 [out1], w2 [out2][out1][k2], b2 [out2]     nn.Conv1d layouts
 *   y  [N][out2 * L2]         channel-major: `.reshape(N, -1)` of the [N, out2, L2] map
 * A workgroup stages a group of rays once; the layer-1 activations stay in LDS; position tiles span the rays of the group.
 * a1_out / a1: reserved for a form that saves the layer-1 activations; this library recomputes them and takes NULL only.
 * Backward: gradients of the four parameter tensors only (rays are data), packed w1 | b1 | w2 | b2 into grad_params
 * (asac_conv1_param_count floats), from x, w1, b1, w2, y (the sign of y is the sign of the second pre-activation) and grad_y.
 * One slab of partial sums per workgroup in `workspace` (asac_conv1_backward_workspace floats), asac_conv1_backward_slabs(desc, N)
 * of them, summed in a fixed order by a second launch: accumulate == 0 writes grad_params, 1 adds to it, ASAC_CONV_SUM_DEFER
 * leaves the slabs to asac_sum_partials_multi (16 slices).  Equal inputs give equal bits.
 * Limits (asac_conv1_supported): out1 <= 16, out2 <= 32, C*k1 and out1*k2 multiples of 4, C*k1 <= 64, out1*k2 <= 256,
 * L2 >= 1, negative_slope > 0 and finite, one ray within the LDS budget (L = 802, C = 2 is); anything else returns
 * ASAC_ERR_BAD_ARG before any launch and callers keep the module path.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t length, channels;
    int32_t out1, kernel1, stride1;
    int32_t out2, kernel2, stride2;
    float negative_slope;
} asac_conv1_desc_t;
int asac_conv1_supported(const asac_conv1_desc_t* desc_host);
int64_t asac_conv1_param_count(const asac_conv1_desc_t* desc_host);
int64_t asac_conv1_backward_workspace(const asac_conv1_desc_t* desc_host, int64_t N);
int asac_conv1_backward_slabs(const asac_conv1_desc_t* desc_host, int64_t N);
int asac_conv1_forward(const asac_conv1_desc_t* desc_host, const float* x, int64_t N, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* y, float* a1_out, void* stream);
int asac_conv1_backward(const asac_conv1_desc_t* desc_host, const float* x, int64_t N, const float* w1, const float* b1,
                        const float* w2, const float* y, const float* a1, const float* grad_y, float* grad_params,
                        int accumulate, float* workspace, void* stream);

/* Cosine-sign gating of auxiliary gradients: `calculate_adaptive_weights` (sac_base.py:1607-1631) after its autograd
 * calls.  main / aux_k / grad: flat f32[n] (the representation's gradient segment and K <= 4 auxiliary gradients of the
 * same layout; aux_host = host array of K device pointers):  gate_k = clamp(sign(cos(main, aux_k)), min = 0)  — the sign
 * of the dot product —, then grad += gate_k * aux_k for k = 0 .. K-1 in that order.  gates_out (f32[K], or NULL) receives
 * the gates.  One workgroup, fixed summation order (deterministic); n <= ASAC_GATE_MAX_N. */
#define ASAC_GATE_MAX_LOSSES 4
#define ASAC_GATE_MAX_N (1 << 20)
int asac_cosine_gate_add(const float* main, const float* const* aux_host, int K, int64_t n, float* grad, float* gates_out,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Observation decoder of the recurrent prediction models (`use_prediction`): `ConvTransposeLayers`
 * (nn_models/layers/image_layers.py:231-253) with the decoder every reference plugin with an image observation
 * model builds (envs/roller/nn_visual_hard_attn.py:64-96, envs/roller/nn_visual_hard.py:47-57,
 * envs/pyramid/nn_visual.py:50-60), called from `_train_rpm` (sac_base.py:1798-1839) through the plugin's
 * `ModelObservation.get_loss`:
 *   state [N, S <= 16] -> Linear(S, 64) GELU -> Linear(64, 128) -> [32, 2, 2] -> ConvTranspose2d(32, 32, 4, 2) LeakyReLU
 *   -> ConvTranspose2d(32, 16, 8, 4) LeakyReLU -> ConvTranspose2d(16, 3, 3, 1) LeakyReLU -> frames [N, 3, 30, 30]
 * as f32 MFMA products with the states as the N dimension (csrc/decoder.hip).  Parameters in PyTorch's layouts
 * (Linear [out, in]; ConvTranspose2d [in, out, kh, kw]).
 *   forward : packs the weights into operand order (`packed`, asac_obs_decoder_packed_floats floats), keeps the
 *             layers' activations in `saved` (asac_obs_decoder_saved_floats(N) floats) for the backward, writes `frames`
 *   backward: grad_frames [N, 3, 30, 30] -> grad_state [N, S] (or NULL) and the ten parameter gradients (written, or
 *             added with accumulate != 0; per-group partial sums added in group order: deterministic);
 *             `workspace` asac_obs_decoder_workspace_floats(N) floats; `packed` / `saved` / `frames` as the forward left them
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float* dense1_w;  /* [64, S]  */
    float* dense1_b;  /* [64]     */
    float* dense2_w;  /* [128, 64] */
    float* dense2_b;  /* [128]    */
    float* ct1_w;     /* [32, 32, 4, 4] */
    float* ct1_b;     /* [32]     */
    float* ct2_w;     /* [32, 16, 8, 8] */
    float* ct2_b;     /* [16]     */
    float* ct3_w;     /* [16, 3, 3, 3]  */
    float* ct3_b;     /* [3]      */
} asac_obs_decoder_params_t;

int64_t asac_obs_decoder_packed_floats(void);
int64_t asac_obs_decoder_saved_floats(int64_t N);
int64_t asac_obs_decoder_workspace_floats(int64_t N);
int asac_obs_decoder_forward(const float* state, int64_t state_stride, int64_t N, int state_size,
                             const asac_obs_decoder_params_t* params_host, float* packed, float* saved, float* frames,
                             void* stream);
int asac_obs_decoder_backward(const float* state, int64_t state_stride, int64_t N, int state_size, const float* packed,
                              const float* saved, const float* frames, const float* grad_frames, float* grad_state,
                              const asac_obs_decoder_params_t* grad_params_host, int accumulate, float* workspace,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-head attention core for short windows on f32 MFMA (csrc/attn_mh.hip): the scores / mask / softmax / weighted-sum
 * part of `MultiheadAttention.forward` (nn_models/layers/seq_layers.py:239-333) for num_heads >= 1 heads of head_dim <= 64
 * channels and windows of <= 32 positions — the widths of the reference's environments (`EpisodeMultiheadAttention(64, …)`
 * with 2 - 8 heads: envs/square/obstacle/nn_attn.py:16, envs/gym/toy_queue/nn_attn.py:28-45).  The q / k / v / output
 * projections around it stay Linears (library GEMMs) on the host side.
 *   q [B][Lq][E], k / v [B][Lk][E], E = heads * head_dim, head h = channels [h * head_dim, (h + 1) * head_dim);
 *   mask as asac_attention_forward (shared by the heads).  out [B][Lq][E] (heads concatenated);  weights [B][Lq][Lk] = the
 *   mean over the heads of softmax(s) * keep;  keep [B][Lq] = 1 - dead;  p_heads [B][heads][Lq][Lk] (or NULL): every head's
 *   softmax, saved for the backward.  row_zero u8 [B][Lq] (or NULL) = the caller's padded positions and keep_rows [B][Lq]
 *   (or NULL) <- keep * !row_zero: the ONE factor the caller multiplies the projected output with (`out * keep` and
 *   `out * ~out_row_mask` of seq_layers.py:320-333 as one product).
 * Backward: grad_out [B][Lq][E], grad_weights [B][Lq][Lk] (w.r.t. the returned weights) or NULL -> grad_q / grad_k / grad_v.
 * One workgroup per batch entry, its heads dealt over four waves; sums in a fixed order: deterministic.
 * ------------------------------------------------------------------------------------------- */
int asac_attention_mh_supported(int Lq, int Lk, int heads, int head_dim);
int asac_attention_mh_forward(const float* q, const float* k, const float* v, const uint8_t* mask, int64_t mask_stride_b,
                              int64_t mask_stride_q, int64_t mask_stride_k, int B, int Lq, int Lk, int heads, int head_dim,
                              float* out, float* weights, float* keep, float* p_heads, const uint8_t* row_zero, float* keep_rows, void* stream);
int asac_attention_mh_backward(const float* q, const float* k, const float* v, const uint8_t* mask, int64_t mask_stride_b,
                               int64_t mask_stride_q, int64_t mask_stride_k, int B, int Lq, int Lk, int heads, int head_dim,
                               const float* p_heads, const float* grad_out, const float* grad_weights, float* grad_q,
                               float* grad_k, float* grad_v, void* stream);

/* The same core with DROPOUT of the softmax weights inside the launch (`nn.functional.dropout(weights, p)` between the softmax
 * and the product with V, seq_layers.py:269-274, live whenever the module is in training mode):  Pd = P (.) M * scale,
 * out = Pd V, weights = mean over the heads of Pd * keep;  backward dP = dPd (.) M * scale, dS from the UNDROPPED P (p_heads
 * holds it, as above), grad_v from Pd.  The mask M is never stored.  Entry (b, h, i, j) is kept iff word j & 3 of
 *   Philox4x32-10(counter = (((b * heads + h) * 32 + i) * 8 + (j >> 2), (5 << 28) | (instance & 0x0FFFFFFF), c lo, c hi), key = seed)
 * is >= thr, c being the module instance's call counter (csrc/asac_dropout.h; tests/attn_dropout_ref.py restates it).
 *   thr = floor(p * 2^32) >= 1 and scale = float32(1 / (1 - p)), both formed in float64 by the caller, p in (0, 1);
 *   B * heads <= 2^24.
 *   state: int64 [544] on the device, owned by the module instance, ZERO except [0] = the call counter before the first launch:
 *   [16] and [32 + 16 g], g < 32, are arrival words (a 128-byte line each), which every launch leaves zero.  Every workgroup reads [0]; the last one to arrive
 *   (csrc/asac_ordered_finish.h, two levels; nothing polls) stores [0] + 1, so a captured launch draws afresh on every
 *   replay.  used: int64 [1] <- the counter this call drew with; the backward reads it THROUGH THE POINTER, so inside a
 *   captured step it follows each replay's forward.  One state per concurrently running launch. */
int asac_attention_mh_dropout_forward(const float* q, const float* k, const float* v, const uint8_t* mask, int64_t mask_stride_b,
                                      int64_t mask_stride_q, int64_t mask_stride_k, int B, int Lq, int Lk, int heads, int head_dim,
                                      float* out, float* weights, float* keep, float* p_heads, const uint8_t* row_zero,
                                      float* keep_rows, uint32_t thr, float scale, uint64_t seed, uint32_t instance,
                                      int64_t* state, int64_t* used, void* stream);
int asac_attention_mh_dropout_backward(const float* q, const float* k, const float* v, const uint8_t* mask, int64_t mask_stride_b,
                                       int64_t mask_stride_q, int64_t mask_stride_k, int B, int Lq, int Lk, int heads, int head_dim,
                                       const float* p_heads, const float* grad_out, const float* grad_weights, float* grad_q,
                                       float* grad_k, float* grad_v, uint32_t thr, float scale, uint64_t seed, uint32_t instance,
                                       const int64_t* used, void* stream);

/* asac_attention_mh_forward with the q / k / v projections of the block's input in front of the scores, in the same launch
 * (`self.q_proj(query), self.k_proj(key), self.v_proj(value)` with value = key and query = the last Lq positions of key,
 * seq_layers.py:239-333): x [B][Lk][E] with strides in floats (multiples of 4, 16-byte aligned), weights / biases = HOST arrays
 * of the three [E][E] / [E] device pointers (q, k, v order); q [B][Lq][E], k / v [B][Lk][E] are OUTPUTS (dense; what the
 * backward reads); row_zero [B][Lq] with a batch stride in bytes (a slice of a wider mask is read in place).  Windows Lq <= Lk <= 16, E = heads * head_dim in {32, 64, 128}, head_dim a multiple of 4.  out_weight non-NULL:
 * the output ResBlock of asac_rows_resblock_forward runs behind the core in the same launch — y / pre [B][Lq][E] as there, with
 * row_scale = keep * !row_zero (`out` still receives the core's own output: the ResBlock's input).  The backward is
 * asac_rows_resblock_backward (if fused), asac_attention_mh_backward, asac_rows_proj_backward. */
int asac_attention_mh_proj_supported(int Lq, int Lk, int heads, int head_dim);
int asac_attention_mh_proj_forward(const float* x, int64_t x_stride_b, int64_t x_stride_t, const float* const* weights,
                                   const float* const* biases, const uint8_t* mask, int64_t mask_stride_b,
                                   int64_t mask_stride_q, int64_t mask_stride_k, int B, int Lq, int Lk, int heads, int head_dim,
                                   float* q, float* k, float* v, float* out, float* attn_weights, float* keep, float* p_heads,
                                   const uint8_t* row_zero, int64_t row_zero_stride_b, float* keep_rows, const float* out_weight,
                                   const float* out_bias, float* y, float* pre, void* stream);

/* The backward of asac_attention_mh_proj_forward WITH its output block as one launch: asac_rows_resblock_backward in front of the
 * core's backward (grad_y [B][Lq][E] with strides in floats — multiples of 4, feature stride 1 —, pre, row_scale = the forward's keep_rows or NULL, out_weight -> grad_pre [B][Lq][E], and the gradient
 * of the core's output, which stays on chip), asac_attention_mh_backward (-> grad_q / grad_k / grad_v, written for the parameter
 * gradient products), asac_rows_proj_backward behind it (proj_weights = HOST array of the three [E][E] device pointers ->
 * grad_x [B][Lk][E]).  Same values as the three launches. */
int asac_attention_mh_block_backward(const float* q, const float* k, const float* v, const uint8_t* mask, int64_t mask_stride_b,
                                     int64_t mask_stride_q, int64_t mask_stride_k, int B, int Lq, int Lk, int heads, int head_dim,
                                     const float* p_heads, const float* grad_y, int64_t grad_y_stride_b, int64_t grad_y_stride_t,
                                     const float* pre, const float* row_scale, const float* out_weight, const float* grad_weights,
                                     const float* const* proj_weights, float* grad_q, float* grad_k, float* grad_v, float* grad_pre,
                                     float* grad_x, void* stream);

/* The Linear layers around that core over the rows of a batch of windows, one launch each (csrc/rows_proj.hip) — replaces, in
 * `MultiheadAttention.forward` (nn_models/layers/seq_layers.py:239-333): `self.q_proj(query), self.k_proj(key),
 * self.v_proj(value)` (three nn.Linear(E, E) = three library GEMMs at the launch floor; backward three GEMMs and two
 * accumulations) and `self.out_proj` when it is ONE residual GELU ResBlock (LinearLayers(E, E, dense_depth 1),
 * linear_layers.py:24-119) followed by the dead-row / padded-row factor (a GEMM and three elementwise launches).
 * width = E in {32, 64, 128}; all pointers 16-byte aligned; weights [E][E] (out x in), biases [E].
 *
 * asac_rows_proj_forward: x [batch][window][E] with strides in floats (feature stride 1; multiples of 4); job j (n_jobs <= 3)
 * writes outs[j] [batch][tails[j]][E] = x[:, window - tails[j]:] weights[j]^T + biases[j]  (tails[j] in 1..window: the cut
 * query of the episode blocks projects the newest positions only).  The pointer arrays are HOST arrays read at the call.
 * asac_rows_proj_backward: grad_x [batch][window][E] (dense, overwritten) = sum_j grads[j] weights[j], job j reaching the
 * newest tails[j] positions only; summation order: jobs in order, features in order.
 * asac_rows_resblock_forward: y = (x + gelu(x W^T + b)) * row_scale[row] (row_scale NULL: 1), pre = x W^T + b (saved for the
 * backward); x [rows][E] with row stride x_row_stride (multiple of 4), y / pre dense.
 * asac_rows_resblock_backward: g = grad_y * row_scale; grad_pre = g * gelu'(pre) (dense: its products over the rows with x
 * are the parameter gradients, asac_xty); grad_x = g + grad_pre W. */
int asac_rows_proj_supported(int width);
int asac_rows_proj_forward(const float* x, int64_t x_stride_b, int64_t x_stride_t, int batch, int window, int width, int n_jobs,
                           const float* const* weights, const float* const* biases, const int* tails, float* const* outs,
                           void* stream);
int asac_rows_proj_backward(const float* const* grads, const int* tails, int n_jobs, const float* const* weights, int batch,
                            int window, int width, float* grad_x, void* stream);
int asac_rows_resblock_forward(const float* x, int64_t x_row_stride, const float* weight, const float* bias,
                               const float* row_scale, int64_t rows, int width, float* y, float* pre, void* stream);
int asac_rows_resblock_backward(const float* grad_y, const float* pre, const float* weight, const float* row_scale,
                                int64_t rows, int width, float* grad_x, float* grad_pre, void* stream);

/* The `nn.Dropout` modules INSIDE the dense stacks around the core (`LinearLayers(E, E, dense_depth 1, dropout p)`:
 * ResBlock -> nn.Dropout(p) [-> nn.Linear], linear_layers.py:24-119; live in every pass, the reference never leaves training
 * mode), inside the row launches.  The draw contract is the core's (csrc/asac_dropout.h; thr, scale, seed, instance, state,
 * used as for asac_attention_mh_dropout_forward; tests/dense_dropout_ref.py restates it): element (row r, feature f) is kept
 * iff word f & 3 of
 *   Philox4x32-10(counter = (r * (width / 4) + (f >> 2), (tag << 28) | (instance & 0x0FFFFFFF), c lo, c hi), key = seed)
 * is >= thr; tag 6 / 7 / 8 = job 0 / 1 / 2 of the dense launch (q / k / v) with r = b * window + t, the position in the FULL
 * window (a draw does not depend on tails[j]); tag 9 = the output block with r the flat row.  rows * width < 2^34.
 * Each of the two launch sites owns a state int64 [544] of the core's layout — one state per concurrently running launch:
 * never the core's.  The mask is never stored.
 *
 * asac_rows_dense_proj_dropout_forward: the <= 3 stacks of one input x (layout and tails as asac_rows_proj_forward), per job j
 *   pres[j] = x W1_j^T + b1_j;  hiddens[j] = (x + gelu(pres[j])) (.) M_j * scale;  outs[j] = hiddens[j] W2_j^T + b2_j
 * all three dense [batch][tails[j]][width] (hiddens: the operand of asac_xty for the gradients of W2_j / b2_j).
 * asac_rows_dense_proj_dropout_backward: g_h_j = (grads[j] W2_j) (.) M_j * scale;  grad_pres[j] = g_h_j * gelu'(pres[j])
 * (dense like grads[j]);  grad_x [batch][window][width] (dense, overwritten) = sum_j (g_h_j + grad_pres[j] W1_j), job j
 * reaching the newest tails[j] positions only.
 * asac_rows_resblock_dropout_forward / _backward: asac_rows_resblock_* with the drop in front of the row factor,
 *   y = (x + gelu(x W^T + b)) (.) M * scale * row_scale;  g = grad_y * row_scale (.) M * scale, grad_pre and grad_x as there. */
int asac_rows_dense_proj_dropout_forward(const float* x, int64_t x_stride_b, int64_t x_stride_t, int batch, int window, int width,
                                         int n_jobs, const float* const* weights1, const float* const* biases1,
                                         const float* const* weights2, const float* const* biases2, const int* tails,
                                         float* const* outs, float* const* pres, float* const* hiddens, uint32_t thr, float scale,
                                         uint64_t seed, uint32_t instance, int64_t* state, int64_t* used, void* stream);
int asac_rows_dense_proj_dropout_backward(const float* const* grads, const float* const* pres, const int* tails, int n_jobs,
                                          const float* const* weights1, const float* const* weights2, int batch, int window,
                                          int width, float* grad_x, float* const* grad_pres, uint32_t thr, float scale,
                                          uint64_t seed, uint32_t instance, const int64_t* used, void* stream);
int asac_rows_resblock_dropout_forward(const float* x, int64_t x_row_stride, const float* weight, const float* bias,
                                       const float* row_scale, int64_t rows, int width, float* y, float* pre, uint32_t thr,
                                       float scale, uint64_t seed, uint32_t instance, int64_t* state, int64_t* used, void* stream);
int asac_rows_resblock_dropout_backward(const float* grad_y, const float* pre, const float* weight, const float* row_scale,
                                        int64_t rows, int width, float* grad_x, float* grad_pre, uint32_t thr, float scale,
                                        uint64_t seed, uint32_t instance, const int64_t* used, void* stream);
/* The gate an episode attention block puts behind its attention, with the padded-row factor, one launch per pass
 * (csrc/rows_gate.hip) — replaces, in `EpisodeMultiheadAttentionBlock.forward` (nn_models/layers/seq_layers.py:460-547),
 * `self.gatedlayer(residual_src, output)` (the gate layers of seq_layers.py:297-345) and the
 * `output * (~key_padding_mask[...]).to(dtype).unsqueeze(-1)` behind it.
 * kind = 1 RESIDUAL, 2 OUTPUT, 3 RECURRENT (the values of `GATE`); width = E in {32, 64, 128}; every pointer 16-byte aligned
 * (row_zero excepted).  x [batch][window][E] = the residual source, read through its strides in floats (feature stride 1;
 * multiples of 4); y [batch][window][E] = the attention output, dense; row_zero uint8 / bool [batch][window] with its own batch
 * stride in bytes (position stride 1), or NULL; s = 1 - row_zero (NULL: 1).  weights = HOST array, read at the call, of the
 * kind's [E][E] device matrices (out x in): none (may be NULL) / {W} / {Wxr, Wyr, Wxz, Wyz, Wxg, Wyg}; bias_z [E] (RECURRENT,
 * else ignored).  Every output is dense [batch][window][E].
 *
 * asac_rows_gate_forward:
 *   RESIDUAL   out = (x + y) s
 *   OUTPUT     a = x W^T;  out = (x + sigmoid(a * y)) s;  saved = {a}
 *   RECURRENT  r = sigmoid(x Wxr^T + y Wyr^T);  z = sigmoid(x Wxz^T + y Wyz^T + bias_z);  h = tanh(y Wyg^T + (r * x) Wxg^T);
 *              out = ((1 - z) x + z h) s;  saved = {r, z, h}
 *   saved = HOST array of the device buffers to fill, or NULL (no backward will follow).
 * asac_rows_gate_backward: g = grad_out s (grad_out dense), with the buffers the forward saved:
 *   RESIDUAL   grad_x = grad_y = g (grad_y may BE grad_x)
 *   OUTPUT     p = sigmoid(a y);  d = g p (1 - p);  grad_y = d a;  grad_pre = {d y};  grad_x = g + (d y) W
 *   RECURRENT  dz_pre = g (h - x) z (1 - z);  dh_pre = g z (1 - h^2);  q = dh_pre Wxg;  dr_pre = q x r (1 - r);
 *              grad_x = (g (1 - z) + q r) + (dr_pre Wxr + dz_pre Wxz);  grad_y = dr_pre Wyr + dz_pre Wyz + dh_pre Wyg;
 *              grad_pre = {dr_pre, dz_pre, dh_pre};  rx = r * x (the left operand of Wxg's gradient; else ignored)
 *   The weight gradients are the products of grad_pre over the rows with x, y and rx, bias_z's the column sums of dz_pre
 *   (asac_xty / asac_xty_multi).  Summation order: each product over the input features in ascending blocks of 16, the lower
 *   and the upper half of the features in an accumulator each (E = 32: one), lower + upper; products that feed one result are
 *   formed on their own and added in the order written, left to right; the other terms as bracketed. */
int asac_rows_gate_supported(int kind, int width);
int asac_rows_gate_forward(int kind, const float* x, int64_t x_stride_b, int64_t x_stride_t, const float* y,
                           const uint8_t* row_zero, int64_t row_zero_stride_b, int batch, int window, int width,
                           const float* const* weights, const float* bias_z, float* out, float* const* saved, void* stream);
int asac_rows_gate_backward(int kind, const float* grad_out, const float* x, int64_t x_stride_b, int64_t x_stride_t,
                            const float* y, const uint8_t* row_zero, int64_t row_zero_stride_b, int batch, int window, int width,
                            const float* const* weights, const float* const* saved, float* grad_x, float* grad_y,
                            float* const* grad_pre, float* rx, void* stream);
/* The rotary position encodings of `MultiheadAttention.forward` (nn_models/layers/seq_layers.py:239-333:
 * `q, k = self.rope(query_index, key_index, q, k)` with `RotaryPositionalEncoding` / `RotaryPositionalEncoding2`, 140-215), one
 * launch per pass — on their own (csrc/rope.hip) or as the epilogue of the q / k / v projection launch (csrc/rows_proj.hip).
 * kind = 3 ROPE, 4 ROPE2 (the values of `POSITIONAL_ENCODING`).  The tables are the module's own buffers, table_rows = T rows;
 * no sine or cosine is computed on the device:
 *   ROPE   table0 = `freqs_cis` (complex64 [T][E/2]) read as floats [T][E/2][2] = (c, s); table1 ignored
 *   ROPE2  table0 = `cos_cached`, table1 = `sin_cached`, float [T][E]
 * Indexes: int32 or int64 (index_bytes = 4 / 8) arrays [batch][positions] with their own strides in ELEMENTS (a batch stride of
 * 0: one row of positions for every batch entry).  Index i reads table row i, i < 0 row i + T (the module's `table[i]`: the
 * episode block's -1 reads row T - 1); an index outside [-T, T) is clamped into the table, the values of such rows are
 * unspecified.  With c, s the values of the row at column i (ROPE) or cos / sin at the row's column j (ROPE2, h = E / 2):
 *   forward   ROPE   y[2i] = x[2i] c - x[2i+1] s;  y[2i+1] = x[2i] s + x[2i+1] c
 *             ROPE2  y[j] = x[j] cos[j] + (-x[j+h]) sin[j]  (j < h);  y[j] = x[j] cos[j] + x[j-h] sin[j]  (j >= h)
 *   backward  ROPE   gx[2i] = g[2i] c + g[2i+1] s;  gx[2i+1] = g[2i+1] c - g[2i] s
 *             ROPE2  gx[j] = g[j] cos[j] + g[j+h] sin[j+h]  (j < h);  gx[j] = g[j] cos[j] - g[j-h] sin[j-h]  (j >= h)
 * every result two products and one sum in that order, no contraction: both forms give the same bits.
 *
 * asac_rope_forward: q [batch][q_len][E] and k [batch][k_len][E] (f32, feature stride 1, batch / position strides in floats, no
 * alignment asked) with an index array each -> out_q, out_k dense; width = E any even number (asac_rope_supported).
 * asac_rope_backward: the same operands with the gradients of out_q / out_k in place of q / k -> the gradients of q / k, dense.
 * asac_rows_proj_rope_forward: asac_rows_proj_forward for the three jobs q, k, v (tails[0] = the query's newest positions) with
 * the rotation behind jobs 0 and 1; the table row of BOTH comes from ONE index array [batch][window] (the query's indexes are its
 * newest tails[0] entries); job 2 (v) is untouched.  width in {32, 64, 128}, the tables 16-byte aligned as every other pointer.
 * Same bits as asac_rows_proj_forward followed by asac_rope_forward.
 * asac_rows_proj_rope_backward: grads = the gradients of the rotated q, k and of v; the first two are un-rotated as they are
 * loaded and written to grads_unrotated[0], [1] (HOST array of two dense device buffers shaped like grads[0], grads[1]: with
 * grads[2] and x the operands of the parameter gradients, asac_xty); grad_x as asac_rows_proj_backward forms it from the
 * un-rotated gradients, same summation order. */
int asac_rope_supported(int kind, int width);
int asac_rope_forward(int kind, const float* table0, const float* table1, int table_rows, int width, int batch, const float* q,
                      int64_t q_stride_b, int64_t q_stride_t, int q_len, const void* q_index, int64_t q_index_stride_b,
                      int64_t q_index_stride_t, const float* k, int64_t k_stride_b, int64_t k_stride_t, int k_len,
                      const void* k_index, int64_t k_index_stride_b, int64_t k_index_stride_t, int index_bytes, float* out_q,
                      float* out_k, void* stream);
int asac_rope_backward(int kind, const float* table0, const float* table1, int table_rows, int width, int batch,
                       const float* grad_q, int64_t grad_q_stride_b, int64_t grad_q_stride_t, int q_len, const void* q_index,
                       int64_t q_index_stride_b, int64_t q_index_stride_t, const float* grad_k, int64_t grad_k_stride_b,
                       int64_t grad_k_stride_t, int k_len, const void* k_index, int64_t k_index_stride_b, int64_t k_index_stride_t,
                       int index_bytes, float* out_q, float* out_k, void* stream);
int asac_rows_proj_rope_forward(int kind, const float* table0, const float* table1, int table_rows, const void* index,
                                int64_t index_stride_b, int64_t index_stride_t, int index_bytes, const float* x,
                                int64_t x_stride_b, int64_t x_stride_t, int batch, int window, int width,
                                const float* const* weights, const float* const* biases, const int* tails, float* const* outs,
                                void* stream);
int asac_rows_proj_rope_backward(int kind, const float* table0, const float* table1, int table_rows, const void* index,
                                 int64_t index_stride_b, int64_t index_stride_t, int index_bytes, const float* const* grads,
                                 const int* tails, const float* const* weights, int batch, int window, int width, float* grad_x,
                                 float* const* grads_unrotated, void* stream);
/* y [rows][N] = x [rows][K] weight[N][K]^T + bias[N] for a narrow input (K <= 64) and a wide output (N a multiple of 16, <= 1024):
 * the input products `x W_ih^T + b_ih` of every step in front of a recurrence (reference seq_layers.py:14-114 through nn.GRU;
 * observation ++ action -> 3 x hidden); x with a row stride in floats, y dense and 16-byte aligned. */
int asac_rows_affine_supported(int K, int N);
int asac_rows_affine_forward(const float* x, int64_t x_row_stride, int K, const float* weight, const float* bias, int64_t rows,
                             int N, float* y, void* stream);
/* ... with the GELU of a `ResBlock` without a residual path (widths differ: the embedding `LinearLayers(n_in, 64, dense_depth 1)`
 * in front of a sequence encoder, linear_layers.py:24-119): y = gelu(x W^T + b), pre = x W^T + b (dense, saved for the backward). */
int asac_rows_affine_gelu_forward(const float* x, int64_t x_row_stride, int K, const float* weight, const float* bias,
                                  int64_t rows, int N, float* y, float* pre, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention core for short windows: the scores / mask / softmax / weighted-sum part of
 * `MultiheadAttention.forward` (nn_models/layers/seq_layers.py:239-333) under the episode attention of
 * `get_l_states` (sac_base.py:1117-1146).  One head per batch entry (callers fold heads into the batch).
 *   q [B][Lq][D], k / v [B][Lk][D] dense;  mask element (b, i, j) at mask + b*stride_b + i*stride_q + j*stride_k
 *   bytes, nonzero = blocked, or NULL (strides of 0 broadcast a [Lq][Lk] or [B][1][Lk] mask)
 *   scores s_ij = (q_i / sqrt(D)) . k_j; blocked -> -inf, except on rows whose every key is blocked ("dead" rows:
 *   they attend unmasked and are zeroed by the caller after its output projection, like the reference)
 *   out [B][Lq][D] = softmax(s) v;  weights [B][Lq][Lk] = softmax(s) * keep;  keep [B][Lq] = 1 - dead
 * Backward: grad_weights (w.r.t. the returned weights) may be NULL; writes grad_q / grad_k / grad_v.
 * Limits: Lq, Lk <= ASAC_ATTN_MAX_LEN, D <= ASAC_ATTN_MAX_DIM (asac_attention_supported).
 * ------------------------------------------------------------------------------------------- */
#define ASAC_ATTN_MAX_LEN 32
#define ASAC_ATTN_MAX_DIM 16
int asac_attention_supported(int Lq, int Lk, int D);
int asac_attention_forward(const float* q, const float* k, const float* v, const uint8_t* mask, int64_t mask_stride_b,
                           int64_t mask_stride_q, int64_t mask_stride_k, int B, int Lq, int Lk, int D, float* out,
                           float* weights, float* keep, void* stream);
int asac_attention_backward(const float* q, const float* k, const float* v, const float* weights,
                            const float* grad_out, const float* grad_weights, int B, int Lq, int Lk, int D,
                            float* grad_q, float* grad_k, float* grad_v, void* stream);

/* The same with the three input projections on chip (seq_layers.py:268-276 with qkv_dense_depth = 0: q_proj,
 * k_proj, v_proj are Linear(E, E)):  q = Wq x_q + bq, k = Wk x_k + bk, v = Wv x_k + bv, one head of E <= 16 channels.
 *   x_q element (b, i, c) at x_q + b*stride_b + i*stride_r + c (floats; the query slice of the key window needs no
 *   copy), x_k likewise;  params = HOST array of 8 device pointers Wq [E][E], bq [E], Wk, bk, Wv, bv, Wo, bo
 *   Wo / bo (both or neither; NULL = none): the output ResBlock of out_dense_depth = 1 applied to the attention
 *   output o on chip, with the dead-row rule:  out = (GELU(Wo o + bo) + o) * keep;  attn_out [B][Lq][E] then
 *   receives o (the backward reads it back together with keep);  row_zero (optional, with the output block):
 *   bytes [B][Lq] with the given strides, nonzero = the row's output is zeroed as well (the episode block's
 *   padded positions, seq_layers.py:445-447)
 * Backward recomputes the projections; grad_out element (b, i, c) at grad_out + b*stride_b + i*stride_r + c (a slice of a
 * longer gradient needs no copy); grad_xq [B][Lq][E] and grad_xk [B][Lk][E] are written dense — grad_xq == NULL: the
 * queries are the LAST Lq key rows (the episode blocks' cut query, seq_layers.py:600-610) and their input gradient is added
 * to those rows of grad_xk inside the launch; the parameter
 * gradients, packed Wq | bq | Wk | bk | Wv | bv (| Wo | bo) (3 or 4 times E*E+E floats), are written or (accumulate == 1) added to
 * grad_params after a fixed-order reduction over workgroups; accumulate == ASAC_ATTN_SUM_DEFER (2): the reduction is left to
 * asac_sum_partials_multi (the partials stay in the workspace); workspace of asac_attention_proj_workspace floats. */
int64_t asac_attention_proj_workspace(int B, int Lq, int Lk, int E);
int asac_attention_proj_forward(const float* xq, int64_t xq_stride_b, int64_t xq_stride_r, const float* xk,
                                int64_t xk_stride_b, int64_t xk_stride_r, const float* const* params_host,
                                const uint8_t* mask, int64_t mask_stride_b, int64_t mask_stride_q,
                                int64_t mask_stride_k, int B, int Lq, int Lk, int E, float* out, float* weights,
                                float* keep, float* attn_out, const uint8_t* row_zero, int64_t row_zero_stride_b,
                                int64_t row_zero_stride_q, void* stream);
int asac_attention_proj_backward(const float* xq, int64_t xq_stride_b, int64_t xq_stride_r, const float* xk,
                                 int64_t xk_stride_b, int64_t xk_stride_r, const float* const* params_host,
                                 const float* weights, const float* keep, const float* attn_out,
                                 const float* grad_out, int64_t grad_out_stride_b, int64_t grad_out_stride_r,
                                 const float* grad_weights, const uint8_t* row_zero,
                                 int64_t row_zero_stride_b, int64_t row_zero_stride_q, int B, int Lq, int Lk, int E,
                                 float* grad_xq, float* grad_xk, float* grad_params, int accumulate,
                                 float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter updates over flat f32 buffers.
 * ------------------------------------------------------------------------------------------- */

/* K5 Polyak: target = target*(1-tau) + source*tau  (two multiplies then an add, like
 * sac_base.py:761-764).  n floats, 16-byte vector loads when aligned. */
int asac_polyak(float* target, const float* source, int64_t n, float tau, void* stream);

/* Adam (torch.optim.Adam defaults: no weight decay, no amsgrad) over a flat segment.
 * `steps_done` is a device counter holding the number of optimizer steps ALREADY taken; the kernel
 * uses t = *steps_done + 1 for the bias corrections and does not modify it (the caller advances it
 * once per train step, so every optimizer of the step shares one counter).
 * sac_base.py:296-300 (optimizer construction), 1589-1603, 1906-1908, 1942-1944. */
int asac_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, const int64_t* steps_done,
                   void* stream);

/* The same update over the E member blocks (E * member_stride floats from param / grad / moments) of a
 * stock network whose gradients were left as per-tile partial sums by asac_mlp_backward* with
 * ASAC_MLP_REDUCE_DEFER: tile sum (same fixed order), optional accumulation, grad write-out and Adam in
 * one launch.  workspace / tiles as that call used them; used = asac_mlp_param_extent().  loss_out [E]
 * (may be NULL) receives the mean-over-loss_rows loss of the qloss variant. */
int asac_adam_step_partials(float* param, float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                            float beta1, float beta2, float eps, const int64_t* steps_done,
                            const float* workspace, int64_t tiles, int E, int64_t member_stride,
                            int64_t used, int accumulate, float* loss_out, int64_t loss_rows, void* stream);

/* Every random draw of one train step in one launch: n_uniform f64 in [0, 1) (the stratified PER
 * sample's uniforms, replay_buffer.py:196) and n_normal f32 N(0, 1) (the rsample noise, sac_base.py:1346,
 * 1883, 1927).  Philox4x32-10 keyed by `seed`, counter = (lane, *step_counter): the counter lives in
 * device memory so a launch frozen inside a hipGraph still draws fresh numbers every step.
 * subsets_out [n_subsets][E_sample] i32 (may be NULL / 0): independent uniformly random E_sample-subsets of
 * range(E) in random order — the ensemble members each target / objective uses (`torch.randperm(E)[:Es]`,
 * sac_base.py:1434). */
int asac_noise_fill(uint64_t seed, const int64_t* step_counter, double* uniform_out, int64_t n_uniform,
                    float* normal_out, int64_t n_normal, int32_t* subsets_out, int n_subsets, int E_sample,
                    int E, void* stream);

/* asac_polyak + a gradient-buffer memset + asac_noise_fill as ONE launch: the independent launches a train
 * step begins with (sac_base.py:2512-2514 target update, the optimizers' zero_grad 1589-1603, the step's random
 * draws).  Either of the two leading parts may be absent (n_polyak == 0 / n_zero == 0), not both. */
int asac_step_prologue(float* target, const float* source, int64_t n_polyak, float tau, float* zero_out,
                       int64_t n_zero, uint64_t seed, const int64_t* step_counter, double* uniform_out,
                       int64_t n_uniform, float* normal_out, int64_t n_normal, int32_t* subsets_out, int n_subsets,
                       int E_sample, int E, void* stream);

/* asac_step_prologue and the fused form of asac_sumtree_sample (batch <= 1024, IS weights in the launch) as ONE
 * launch, the first of a captured train step: the first ceil(batch / 256) workgroups sample 256 rows each, drawing their
 * stratified uniforms themselves (the very numbers asac_step_prologue would have stored in uniform_out, which they
 * also fill), the other workgroups are the prologue's.  replay_buffer.py:185-205, 347-354 + sac_base.py:745-764.
 * min_p_out is f32[528], 64-byte aligned, HERE: [0] min p, [1] min ratio, [2..7] the workgroups' exchange (partial minima,
 * two counters) — which must be ZERO before the first launch and are left zero by every launch.
 * is_weights_out == NULL defers the weights (sharded replay: they are normalised by the minimum sampling ratio over
 * all ranks' shards): min_p_out[0] = min p, min_p_out[1] = min p / total, beta untouched; after the MIN all-reduce of
 * min_p_out[1], asac_per_is_weights advances beta and writes the weights. */
int asac_step_prologue_sample(float* target, const float* source, int64_t n_polyak, float tau, float* zero_out,
                              int64_t n_zero, uint64_t seed, const int64_t* step_counter, double* uniform_out,
                              float* normal_out, int64_t n_normal, int32_t* subsets_out, int n_subsets, int E_sample,
                              int E, const float* tree, int capacity, int batch, const int64_t* slot_ids,
                              double* beta_state, double beta_increment, int32_t* leaf_out, float* p_out,
                              int64_t* ids_out, float* is_weights_out, float* min_p_out, void* stream);

/* The pair for batches of 257 .. 1 024 rows on one GPU (hip_config['defer_is_weights']; smaller batches too where the weights
 * ride in the step's first network launch, ASAC_SIDECAR_WINDOW_GATHER_W): the sampler's workgroups (256
 * samples each) only leave their minima in min_p_out[2 ..] — no exchange between them, no weights, beta untouched —, and
 * asac_window_gather_pad_w, the NEXT launch, forms the weights in one extra workgroup beside the gather's (minimum over the
 * workgroups' minima, beta advanced first, f64 power: replay_buffer.py:352-354), min_p_out[0] = min p.  Same numbers as
 * asac_step_prologue_sample followed by asac_window_gather_pad, bit for bit. */
int asac_step_prologue_sample_partial(float* target, const float* source, int64_t n_polyak, float tau, float* zero_out,
                                      int64_t n_zero, uint64_t seed, const int64_t* step_counter, double* uniform_out,
                                      float* normal_out, int64_t n_normal, int32_t* subsets_out, int n_subsets, int E_sample,
                                      int E, const float* tree, int capacity, int batch, const int64_t* slot_ids,
                                      int32_t* leaf_out, float* p_out, int64_t* ids_out, float* min_p_out, void* stream);
int asac_window_gather_pad_w(const asac_gather_key_t* keys_host, int n_keys, const int64_t* ids, int batch, int prev_n,
                             int post_n, int capacity, const int32_t* index_ring, const float* p, const float* tree,
                             double* beta_state, double beta_increment, float* is_weights_out, float* min_p_out,
                             void* stream);

/* hipGraphLaunch of an instantiated graph (the captured train step) on `stream`. */
int asac_graph_launch(void* graph_exec, void* stream);

/* Fix-up pass over the captured train step (a hipGraph_t, before it is instantiated): every 1-D memset node is replaced by a
 * kernel node with the same edges (csrc/graph_fix.hip).  On ROCm 7.2 / gfx950 a captured hipMemsetAsync of >= 16 bytes takes
 * effect on the first launch of the instantiated graph only; ATen's split reductions zero their semaphores with one, so a
 * captured bias gradient (`x.sum(0)` of an nn.Linear backward inside `SAC_Base._train_rep_q`, sac_base.py:1916-2010) is wrong
 * from the second replay on.  n_replaced / n_kept (2-D memsets, left alone) may be NULL. */
int asac_graph_replace_memset_nodes(void* graph, int* n_replaced, int* n_kept);

/* Temperature step in one launch: dL/dlog_alpha = mean_b(-logp_b) - target into grad[slot], then the
 * same Adam update as asac_adam_step over the n temperature parameters (param / grad / moments point
 * at the alpha segment).  sac_base.py:1913-1949 (continuous head) + 1942-1944.  Single-GPU form; with
 * a gradient all-reduce between the two halves use asac_alpha_grad + asac_adam_step.  This is the last
 * optimizer launch of a train step: with advance_counter != 0 it also advances *steps_done by one
 * (after reading it), which saves the step a counter-increment launch. */
int asac_alpha_adam_step(const float* logp, int B, float target, int slot, float* param, float* grad,
                         float* exp_avg, float* exp_avg_sq, int n, float lr, float beta1, float beta2,
                         float eps, int64_t* steps_done, int advance_counter, void* stream);

/* Curiosity (SAC_Base._get_y, sac_base.py:1333-1343): reward[b][t] += strength * 0.5 * sum_k (approx - actual)^2 over
 * the sampled window, in place.  approx [B][T][K] dense (the dynamics model's output); actual [B][T][K] with strides in
 * floats (the next states of the window for the FORWARD model, the stored actions for the INVERSE one); reward [B][T]
 * with batch stride reward_stride_b.  One launch for ATen's subtract, square, sum, scale and add. */
int asac_curiosity_bonus(const float* approx, const float* actual, int64_t actual_stride_b, int64_t actual_stride_t,
                         float* reward, int64_t reward_stride_b, int B, int T, int K, float strength, void* stream);
/* Loss of the curiosity model and its gradient (SAC_Base._train_curiosity, sac_base.py:1951-1976):
 *   d = (pred - target) * !padding_mask[b][t];  *loss_out = sum d^2 / N;  grad_out = d * 2 / N,  N = B T K
 * pred / grad_out [B][T][K] dense, target strided like `actual` above, padding_mask u8 [B][T] or NULL.  The
 * workgroups' sums are added in workgroup order by the last workgroup to arrive (fixed summation order).
 * workspace: asac_masked_mse_workspace(N) floats, ZERO before its first use (the launch leaves its arrival counter at
 * zero again); N <= ASAC_MASKED_MSE_MAX, larger problems return ASAC_ERR_BAD_ARG and keep ATen's chain. */
#define ASAC_MASKED_MSE_MAX (1 << 20)
int64_t asac_masked_mse_workspace(int64_t n);
int asac_masked_mse(const float* pred, const float* target, int64_t target_stride_b, int64_t target_stride_t,
                    const uint8_t* padding_mask, int64_t mask_stride_b, int B, int T, int K, float* grad_out,
                    float* loss_out, float* workspace, void* stream);

/* The plain mean squared error over millions of elements and its gradient, one launch, one read of both operands (a
 * plugin's observation loss `mse_loss(decoded frames, frames)` under sac_base.py:1817 / 1798-1839:
 * *loss_out = sum (pred - target)^2 / N, grad_out = grad_scale * (pred - target) * 2 / N, N = B T K; grad_scale: the factor
 * the caller is going to multiply the loss with — 1 / n_step in `_train_rpm` — so that the gradient needs no second pass
 * over its 44 MB).  pred / grad_out [B][T][K]
 * dense, target strided (floats) like asac_masked_mse's; K and the strides multiples of 4, 16-byte aligned pointers;
 * N < 2^33.  Fixed summation order.  workspace: f32[asac_mse_mean_grad_workspace()], ZERO before its first use (left
 * zero by every launch). */
int64_t asac_mse_mean_grad_workspace(void);
int asac_mse_mean_grad(const float* pred, const float* target, int64_t target_stride_b, int64_t target_stride_t, int B, int T,
                       int K, float grad_scale, float* grad_out, float* loss_out, float* workspace, void* stream);

/* Loss of the recurrent prediction model's transition head and its gradient (SAC_Base._train_rpm,
 * sac_base.py:1798-1816; torch/distributions/normal.py log_prob / entropy, kl.py _kl_normal_normal):
 *   out[0] = -mean(log N(target; loc, scale)) + kl_weight * mean(KL(N(loc, scale) || N(0, 1)))
 *   out[1] = mean entropy of N(loc, scale)
 *   grad_loc / grad_scale [B][T][K] dense = d out[0] / d loc, / d scale
 * loc / scale / target [B][T][K] views with strides in floats (the two halves of the model's output, a slice of the
 * target representation's window).  One launch for ~60 elementwise ATen launches forward and backward; sums in
 * workgroup order (last to arrive); workspace asac_normal_nll_kl_workspace(N) floats, zero before first use. */
int64_t asac_normal_nll_kl_workspace(int64_t n);
int asac_normal_nll_kl(const float* loc, int64_t loc_stride_b, int64_t loc_stride_t, const float* scale,
                       int64_t scale_stride_b, int64_t scale_stride_t, const float* target, int64_t target_stride_b,
                       int64_t target_stride_t, int B, int T, int K, float kl_weight, float* grad_loc, float* grad_scale,
                       float* loss_entropy_out, float* workspace, void* stream);

/* The same with the head's activation inside: mean_logstd [B][T][2K] (strides in floats) is the transition model's raw
 * output (mean | logstd, `torch.chunk` of nn_models/predictions.py:39-44), the distribution's scale is
 * clamp(exp(logstd), scale_min, scale_max); grad_mean_logstd [B][T][2K] dense = d out[0] / d (mean | logstd) — exp's and
 * clamp's backward (pass-through where scale_min <= exp <= scale_max) applied in the launch. */
int asac_normal_nll_kl_logstd(const float* mean_logstd, int64_t stride_b, int64_t stride_t, float scale_min, float scale_max,
                              const float* target, int64_t target_stride_b, int64_t target_stride_t, int B, int T, int K,
                              float kl_weight, float* grad_mean_logstd, float* loss_entropy_out, float* workspace,
                              void* stream);

/* Products over the ROWS of two tall matrices (csrc/xty.hip, f32 MFMA):  out [M][N] = sum_r x[r][m] y[r][n]  and, optionally,
 * colsum_x [M] = sum_r x[r][m] — the weight and bias gradients of a Linear over thousands of rows (x = grad_out, y = input:
 * `nn.Linear` backward inside `LinearLayers` / `ResBlock`, nn_models/layers/linear_layers.py:24-119; the attention
 * projections, seq_layers.py:239-333) and the input / recurrent weight gradients of the GRU (seq_layers.py:14-114) at the widths
 * of the reference's environments (M <= 512, N <= 128).  Row strides in floats; accumulate != 0 adds to out / colsum_x;
 * fixed summation order (per-workgroup partials in `workspace`, asac_xty_workspace floats, summed in workgroup order). */
int asac_xty_supported(int64_t rows, int M, int N);
int64_t asac_xty_workspace(int64_t rows, int M, int N);
int asac_xty(const float* x, int64_t x_row_stride, int M, const float* y, int64_t y_row_stride, int N, int64_t rows, float* out,
             float* colsum_x, int accumulate, float* workspace, void* stream);
/* n_jobs <= 4 such products as ONE launch pair (the parameter gradients of the Linear layers of one attention block: q / k / v
 * projections and the output block).  Arrays of n_jobs entries (HOST arrays, read at the call); colsums NULL or with NULL
 * entries: no column sums; no output may appear twice; workspace: asac_xty_multi_workspace floats.  Same values as n_jobs
 * calls of asac_xty (same partition of the rows, same summation order). */
int64_t asac_xty_multi_workspace(int n_jobs, const int64_t* rows, const int* M, const int* N);
int asac_xty_multi(int n_jobs, const float* const* x, const int64_t* x_row_strides, const int* M, const float* const* y,
                   const int64_t* y_row_strides, const int* N, const int64_t* rows, float* const* outs, float* const* colsums,
                   int accumulate, float* workspace, void* stream);

/* State head of a representation plugin: y = tanh(x W^T + b) over the N = batch * window rows of an encoder
 * output, one launch per pass (the reference's test plugins end their representations with
 * `nn.Sequential(nn.Linear(n, 8), nn.Tanh())`: tests/nn_conv_vanilla.py:11-14, tests/nn_conv_attn.py:15-17,
 * envs/test/nn_rnn.py; stock torch runs a GEMM and a tanh forward, two GEMMs, a bias reduction, a tanh backward and
 * two gradient accumulations backward).  x [N][K] with row stride x_row_stride >= K floats, weight [O][K], bias [O]
 * (torch.nn.Linear layout), y [N][O].  K <= ASAC_LINEAR_TANH_MAX_IN, O <= ASAC_LINEAR_TANH_MAX_OUT.
 * Backward: grad_x [N][K] (may be NULL), grad_params = weight gradient [O][K] | bias gradient [O], overwritten or
 * (accumulate != 0) added to; per-workgroup partial sums are combined in workgroup order by the last workgroup
 * to finish (deterministic).  workspace: asac_linear_tanh_workspace(N, K, O) floats, ZERO before its first use
 * (the launch leaves its arrival counter at zero again); one workspace per concurrently running launch. */
#define ASAC_LINEAR_TANH_MAX_IN 64
#define ASAC_LINEAR_TANH_MAX_OUT 16
int64_t asac_linear_tanh_workspace(int64_t N, int K, int O);
int asac_linear_tanh_forward(const float* x, int64_t x_row_stride, const float* weight, const float* bias, int64_t N,
                             int K, int O, float* y, void* stream);
int asac_linear_tanh_backward(const float* x, int64_t x_row_stride, const float* weight, const float* y,
                              const float* grad_y, int64_t N, int K, int O, float* grad_x, float* grad_params,
                              int accumulate, float* workspace, void* stream);
/* The same head over an input that is the concatenation of two row blocks, x0 [N][K0] | x1 [N][K1] (x1 NULL: x0
 * alone), read in place — `self.dense(torch.cat([vec, self.conv(img)], dim=-1))`, tests/nn_conv_vanilla.py:16-19 —
 * with K = K0 + K1 <= ASAC_LINEAR_TANH_MAX_IN (weight [O][K]).  Backward: grad_x0 [N][K0], grad_x1 [N][K1] (each may be
 * NULL); the output gradient is given as grad_y [grad_members][N / grad_window][O]: row r receives
 * sum_e grad_y[e][r / grad_window] (member order) when r % grad_window == grad_position and zero otherwise — the
 * critics' state gradients at the one window position the Q loss reads (sac_base.py:2104-2110), summed in the launch
 * (grad_members = 1, grad_window = 1: a dense [N][O] gradient).  Values of asac_linear_tanh_forward / _backward on
 * the materialised concatenation / gradient, bit for bit. */
int asac_linear_tanh_forward2(const float* x0, int64_t x0_row_stride, int K0, const float* x1, int64_t x1_row_stride,
                              int K1, const float* weight, const float* bias, int64_t N, int O, float* y, void* stream);
/* ... forward / backward (`2w`) with x0 a [samples][x0_window_T][K0] slice of the sampled windows (`vec[:, burn_in_step:]`) read in place:
 * row r lies at (r / x0_window_T) * x0_sample_stride + (r % x0_window_T) * x0_row_stride (x0_window_T = 0: uniform rows) */
int asac_linear_tanh_forward2w(const float* x0, int64_t x0_row_stride, int x0_window_T, int64_t x0_sample_stride, int K0,
                               const float* x1, int64_t x1_row_stride, int K1, const float* weight, const float* bias,
                               int64_t N, int O, float* y, void* stream);
int asac_linear_tanh_backward2w(const float* x0, int64_t x0_row_stride, int x0_window_T, int64_t x0_sample_stride, int K0,
                                const float* x1, int64_t x1_row_stride, int K1, const float* weight, const float* y,
                                const float* grad_y, int grad_members, int grad_window, int grad_position, int64_t N, int O,
                                float* grad_x0, float* grad_x1, float* grad_params, int accumulate, float* workspace,
                                void* stream);
int asac_linear_tanh_backward2(const float* x0, int64_t x0_row_stride, int K0, const float* x1, int64_t x1_row_stride,
                               int K1, const float* weight, const float* y, const float* grad_y, int grad_members,
                               int grad_window, int grad_position, int64_t N, int O, float* grad_x0, float* grad_x1,
                               float* grad_params, int accumulate, float* workspace, void* stream);

/* ---- a Linear layer with a WIDE input (csrc/wide.hip) ----------------------------------------------------------------
 * y = act(x W^T + b) for x [R][K] (rows x_row_stride floats apart), W [N][K] row-major, N in {32, 64, 128}, K a multiple of
 * 16 up to 16 384; act: 0 identity, 1 GELU (exact).  The first layer of the dense head behind a flattened convolution map:
 * `ConvLayers.dense = LinearLayers(h * w * out_c, out_dense_n, ...)` with h * w * out_c = 2 592 for 84 x 84 frames
 * (nn_models/layers/image_layers.py:188-227, linear_layers.py:24-119: `ResBlock` = Linear + GELU without a residual path when
 * the widths differ), under autograd the GEMM / GELU / bias-reduction launches of `nn.Linear`.
 *   forward          split-K partials in `workspace`, summed in order with the bias; `pre` (or NULL): the pre-activations
 *   backward_input   dpre_out [R][N] = grad_y * act'(pre), dx [R][K] = dpre W (dx NULL: dpre only)
 *   backward_params  dw [N][K] (+)= dpre^T x, db [N] (+)= column sums of dpre (db may be NULL); fixed-order partial sums
 * workspace: asac_rows_wide_workspace(R, K, N) floats (-1: unsupported shape), for either launch. */
int asac_rows_wide_supported(int64_t R, int K, int N);
int64_t asac_rows_wide_workspace(int64_t R, int K, int N);
int asac_rows_wide_forward(const float* x, int64_t x_row_stride, int64_t R, int K, const float* w, const float* b, int N,
                           int act, float* y, float* pre, float* workspace, void* stream);
int asac_rows_wide_backward_input(const float* grad_y, const float* pre, int act, int64_t R, int K, const float* w, int N,
                                  float* dpre_out, float* dx, int64_t dx_row_stride, void* stream);
int asac_rows_wide_backward_params(const float* dpre, const float* x, int64_t x_row_stride, int64_t R, int K, int N, float* dw,
                                   float* db, int accumulate, float* workspace, void* stream);

/* ---- several fixed-order partial sums as one launch (csrc/reduce.hip) ---------------------------------------------------
 * The second launch of a backward — the per-workgroup parameter-gradient partials added in workgroup order — for up to
 * ASAC_SUM_PARTIALS_MAX_JOBS backwards at once: the walks of the representation's graph, one per gated loss, of
 * `calculate_adaptive_weights` (reference sac_base.py:1607-1631, entered from `_train_rpm` 1798-1839) read none of their
 * parameter gradients before all walks are done.  A job: out[i] (+)= sum over slabs t of partial[t * slab_stride + i], i < n,
 * in the order of the launch it replaces — slices = 16: sixteen contiguous slices of the slabs, each summed in order, then
 * the slice sums in order (asac_mlp_backward with >= 64 tiles, asac_attention_proj_backward); slices = 1: slab order
 * (asac_mlp_backward with fewer tiles).  The partials are what those entry points leave in their workspace under
 * ASAC_MLP_REDUCE_DEFER / accumulate == ASAC_ATTN_SUM_DEFER:
 *   asac_mlp_backward             [tiles = asac_mlp_backward_tiles(N, E)][E][member_stride], n = asac_mlp_param_extent(desc)
 *   asac_attention_proj_backward  [blocks][n], n = (3 | 4) (E E + E), blocks = asac_attention_proj_workspace / (4 (E E + E))
 *   asac_linear_tanh_backward*    (accumulate == ASAC_LINEAR_SUM_DEFER)  [blocks = ceil(N / 64)][n = O K + O]; 16 slices
 *   asac_conv2_backward(_windows / _multi)  (accumulate == ASAC_CONV_SUM_DEFER)  [blocks][n], n = n_cot x the packed parameter
 *                                 count, blocks = asac_conv2_backward_slabs(desc, N, n_cot); 16 slices
 * jobs_host: a HOST array.  The jobs run side by side in no order: two jobs of one launch whose [out, out + n) overlap are
 * refused ("one output twice") — such sums go into consecutive launches. */
#define ASAC_SUM_PARTIALS_MAX_JOBS 16
#define ASAC_ATTN_SUM_DEFER 2
#define ASAC_CONV_SUM_DEFER 2
#define ASAC_LINEAR_SUM_DEFER 2
typedef struct {
    const float* partial;
    float* out;
    int64_t slab_stride;
    int64_t n;
    int32_t slabs, slices, accumulate, pad_;
} asac_partial_sum_t;
int asac_sum_partials_multi(int n_jobs, const asac_partial_sum_t* jobs_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Episode batch queue: training without a replay buffer (SAC_Base(use_replay_buffer=False), reference
 * algorithm/batch_buffer.py, utils/operators.py:105-206 `episode_to_batch`, sac_base.py:2496-2609).
 * HBM layout (algorithm/batch_buffer.py): per key a window pool [P][L][row_bytes] (L = burn_in + n_step + 1, every
 * live window stored once, already padded), the queue i32[ring_rows][batch] of pool slots, a head i32[1] holding the
 * ABSOLUTE number of the next batch to pop (its queue row: head % ring_rows).  The host planner decides every slot,
 * queue row and head value.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const void* src;     /* episode rows, src_stride bytes apart (NULL with ASAC_PAD_EMIT_MASK)               */
    void* pool;          /* [P][L][row_bytes]                                                                */
    const void* pad_row; /* ASAC_PAD_ROW only                                                                */
    int64_t src_stride;
    int32_t row_bytes;   /* ASAC_PAD_EMIT_MASK: 1                                                            */
    int32_t pad_mode;    /* ASAC_PAD_WORD / _BYTE / _ROW: rows outside the episode; ASAC_PAD_EMIT_MASK: the
                            padding mask itself (1 on the rows in front of the episode, 0 from its first row on:
                            the reference's mask, utils/operators.py:151-153)                                */
    uint32_t pad_word;
    int32_t reserved_;
} asac_batch_put_key_t;

/* One launch per episode (BatchBuffer.put_episode + episode_to_batch): window w (pool slot win_slot[w]) row j of
 * every key := episode row win_start[w] + j (win_start = window start - burn_in), or the key's padding where that row
 * lies outside [0, ep_len); the same launch writes queue[queue_rows[q]][:] := queue_slots[q][:] and head := new_head.
 *   win_start, win_slot  i32[n_windows];  queue_rows i32[n_queue_rows], queue_slots i32[n_queue_rows][batch]
 * Slots outside [0, pool_slots) and queue rows outside [0, ring_rows) are skipped. */
int asac_batch_put(const asac_batch_put_key_t* keys_host, int n_keys, int ep_len, int burn_in, int L,
                   const int32_t* win_start, const int32_t* win_slot, int n_windows, int pool_slots,
                   const int32_t* queue_rows, const int32_t* queue_slots, int n_queue_rows, int batch,
                   int32_t* queue, int ring_rows, int32_t* head, int32_t new_head, void* stream);

typedef struct {
    const void* pool;    /* [P][L][row_bytes]                                                                */
    void* dst;           /* [batch][L][row_bytes] (f32 [batch][L][row_bytes] elements with a conversion)     */
    int32_t row_bytes;
    int32_t convert;     /* ASAC_CVT_*                                                                       */
} asac_batch_gather_key_t;

/* The per-step launch (BatchBuffer.get_batch; captured in the train step's hipGraph): dst_k[b][j] := pool_k[
 * queue[head % ring_rows][b]][j] for every key, uint8 / bool observations widened to f32 (ASAC_CVT_*).  Reads the head,
 * does not advance it (the step does, after its last launch). */
int asac_batch_pop_gather(const asac_batch_gather_key_t* keys_host, int n_keys, const int32_t* queue,
                          const int32_t* head, int ring_rows, int batch, int L, int pool_slots, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Behaviour cloning (ImitationBase.train, imitation_base.py:57-59): over rows [0, *t_valid) of one padded episode
 *   loss = mean(-Normal(loc, scale).log_prob(a) - entropy_coef * Normal(loc, scale).entropy()),   a = action[:, offset:]
 * with z = (a - loc) / scale:  dloss/dloc = -z / scale,  dloss/dscale = (1 - entropy_coef - z^2) / scale, each over
 * (*t_valid * A); rows >= *t_valid add nothing and get zero gradients.  ONE launch; the sum has a fixed order (lane,
 * wave, workgroup, then the workgroups' sums in workgroup order by the last to arrive: no float atomics), so equal inputs
 * give equal bits.  t_valid is read on the device: one captured launch serves every episode length up to Tp.
 *   loc, scale   rows ld_in floats apart;   dloc, dscale   rows ld_out floats apart;   action rows action_stride apart
 *   raw_head != 0: loc / scale hold the stock policy's raw (mean | logstd) head outputs, the launch applies
 *     loc = 5 tanh(mean / 5), scale = exp(clamp(logstd, -20, 0.5)) (nn_models/policy.py:169) and the gradients are
 *     with respect to the raw values
 *   workspace    asac_bc_loss_grad_workspace() floats, zero before the first launch (every launch leaves them usable)
 *                one launch at a time per workspace: launches on different streams need workspaces of their own
 * Tp * A <= ASAC_BC_MAX_ELEMENTS. */
#define ASAC_BC_MAX_BLOCKS 64
#define ASAC_BC_MAX_ELEMENTS (1 << 24)
int64_t asac_bc_loss_grad_workspace(void);
int asac_bc_loss_grad(const float* loc, const float* scale, int64_t ld_in, const float* action, int64_t action_stride,
                      int action_offset, const int32_t* t_valid, int Tp, int A, float entropy_coef, int raw_head,
                      float* loss, float* dloc, float* dscale, int64_t ld_out, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The option-critic's per-option learner (OptionBase, algorithm/oc/option_base.py).
 *
 * asac_option_return: asac_vtrace_return_min with the option's termination mix in front of the scan — OptionBase._get_y's
 * continuous branch (option_base.py:287, 376-427 + sac_base.py _v_trace 1244-1295) in ONE launch:
 *   V(s_t)   = min_{e in subset_n}    Q_e(s_t, a_t) - alpha logpi_t
 *   V(s_t+1) = (1 - beta[b, t]) * (min_{e in subset_next} Q_e(s_t+1, a_t+1) - alpha logpi_t+1)
 *              + beta[b, t] * mean_o v_options[b, t, o]
 * `args_host` as for asac_vtrace_return_min (q, logp, log_alpha, masks, ratios, optional q_online / td_error_out:
 * td[b] = mean_e |q_online[e][b] - y[b]|, option_base.py:788-800 for continuous-only action spaces); beta [B, n] and
 * v_options [B, n, num_options] with their strides in floats.  The mean over the options is the sum in option order by
 * one lane, divided by num_options; neither it nor V(s_t) / V(s_t+1) reach memory.  Same step arithmetic and scan
 * association as asac_vtrace_return_min: with beta == 0 the two produce the same bits.
 * Bad arguments (null beta / v_options, num_options <= 0 or > ASAC_OPTION_MAX_OPTIONS, importance sampling without
 * probabilities, n too large for 64 KB of LDS) return hipErrorInvalidValue without a launch. */
#define ASAC_OPTION_MAX_OPTIONS 1024
int asac_option_return(const asac_vtrace_args_t* args_host, const float* beta, int64_t beta_stride_b,
                       int64_t beta_stride_t, const float* v_options, int64_t v_stride_b, int64_t v_stride_t,
                       int64_t v_stride_o, int num_options, void* stream);

/* asac_termination_loss_grad: OptionBase.compute_termination_grads behind the head's forward (option_base.py:695-703):
 *   loss = mean_b(beta[b] * (y[b] - mean_o v_options[b, o] + terminal_entropy) * ~done[b] * priority_is[b])
 *   dbeta[b] = d loss / d beta[b] = (y[b] - mean_o v_options[b, o] + terminal_entropy) * ~done[b] * priority_is[b] / B
 * value and gradient from ONE launch for any B <= ASAC_TERMINATION_MAX_ROWS; priority_is may be NULL.  The sum has a
 * fixed order (lane, wave, workgroup, then the workgroups' sums in workgroup order by the last to arrive: no float
 * atomics): equal inputs give equal bits.  Rows with done set add an exact 0 and get an exact 0 gradient.
 *   beta, y, priority_is   element b at b * stride (floats);   v_options element (b, o) at b * v_stride_b + o * v_stride_o
 *   dbeta f32[B] contiguous;  loss f32[1]
 *   workspace    asac_termination_loss_grad_workspace() floats, zero before the first launch (every launch leaves them
 *                usable); one launch at a time per workspace */
#define ASAC_TERMINATION_MAX_BLOCKS 64
#define ASAC_TERMINATION_MAX_ROWS (1 << 24)
int64_t asac_termination_loss_grad_workspace(void);
int asac_termination_loss_grad(const float* beta, int64_t beta_stride, const float* y, int64_t y_stride,
                               const float* v_options, int64_t v_stride_b, int64_t v_stride_o, int num_options,
                               const uint8_t* done, const float* priority_is, int64_t is_stride, float terminal_entropy,
                               int B, float* loss, float* dbeta, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pure-discrete, policy-based SAC (d_action_sizes set, c_action_size == 0, discrete_dqn_like False): the learner's
 * row-wise arithmetic around the networks as one launch per item (csrc/discrete.hip, csrc/asac_categorical.h).
 * Notation: logits z[row, j]; K branches of sizes s_k, D = sum s_k; within a branch p = softmax(z),
 * lp = z - logsumexp(z), cl(p) = log(max(p, 1e-8)); Qbar_j = the mean over the members of a device-resident subset.
 * The branch table and the ensemble members' base pointers travel by value: the members' head outputs are separate
 * tensors of one shape.  Nothing allocates or synchronises.  Bad arguments (null outputs, a branch table that does not
 * add up, E_sample > E, a size over the limits below) return hipErrorInvalidValue without a launch.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_DISCRETE_MAX_WIDTH 64      /* D  */
#define ASAC_DISCRETE_MAX_BRANCHES 8    /* K  */
#define ASAC_DISCRETE_MAX_MEMBERS 8     /* E  */
#define ASAC_DISCRETE_MAX_STEPS 64      /* n  */
#define ASAC_DISCRETE_MAX_ROWS 1024     /* B of the single-workgroup reductions (the two losses, the temperature) */
typedef struct {
    int32_t K, D;
    int32_t size[ASAC_DISCRETE_MAX_BRANCHES];
} asac_branches_t;
typedef struct {
    const float* base[ASAC_DISCRETE_MAX_MEMBERS];  /* member e: element (b, t, j) at base[e] + b*stride_b + t*stride_t + j */
    int64_t stride_b, stride_t;
    int32_t E, reserved_;
} asac_members_t;

/* The return target of SAC_Base._get_y's policy-based discrete branch (sac_base.py:1383-1421 + _v_trace 1244-1295) in
 * ONE launch (with q_online: _get_td_error's 2219-2244 too).  Per window position u in [0, n]:
 *   V = (1/K) sum_j p_j (Qbar_j - alpha cl(p_j));  positions 0..n-1 use
 * subset_n, positions 1..n subset_next.  Under use_n_step_is: pi_t = exp(sum_k lp[argmax of the stored one-hot in
 * branch k]) (first maximum, as torch), mu_t = prod_j (mu_j a_j, zeros -> 1), ratio pi / max(mu, 1e-8).  Then
 * asac_vtrace.h's step arithmetic and row scan.
 *   args      reward / done / masks / ratios / gamma / B / n / y_out as for asac_vtrace_return_min; also read:
 *             subset_n, subset_next, E_sample, log_alpha (= log_d_alpha), mu_prob + mu_stride_b/t (entries [0, D)),
 *             td_error_out.  q, logp, pi_prob, A, mu_offset, q_online, E_online are not read.
 *   q_target  the target members' head outputs [B, n+1, D];  logits [B, n+1, D] (rows logits_stride_b/t floats apart)
 *   action    the stored actions' window [B, >= n, >= D] (needed under use_n_step_is and for the TD error)
 *   q_online  optional (E == 0: none) online members' head outputs [B, D] at the step's state (stride_t not read): with
 *             args->td_error_out the launch writes td[b] = mean_e |(1/K) sum_j a_j q_e[b, j] - y_b|, a = action at t = 0
 * Many workgroups, no exchange between them.  n <= ASAC_DISCRETE_MAX_STEPS; any B. */
typedef struct {
    asac_branches_t branches;
    asac_members_t q_target;
    asac_members_t q_online;
    const float* logits;
    int64_t logits_stride_b, logits_stride_t;
    const float* action;
    int64_t action_stride_b, action_stride_t;
} asac_discrete_return_t;
int asac_discrete_return(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host, void* stream);

/* The return target of OptionBase._get_y's policy-based discrete branch (oc/option_base.py:287, 333-373 + sac_base.py
 * _v_trace 1244-1295) in ONE launch (with q_online: the option's _get_td_error too).  asac_discrete_return's launch with
 * the option's two differences, per window position u in [0, n], c_j = alpha cl(p_j):
 *   Qn_j = min over subset_n of q_target[e][b, u, j],  Qx_j = min over subset_next        (the MINIMUM, not the mean)
 *   Vn[u] = (1/K) sum_j p_j (Qn_j - c_j)                                                               u < n
 *   Vx[u] = (1/K) sum_j p_j ((1 - beta[b, u-1]) (Qx_j - c_j) + beta[b, u-1] vbar[b, u-1])              u >= 1
 *   vbar[b, t] = mean_o v_options[b, t, o]: the sum in option order by one lane, divided by num_options (the bits of
 *   asac_option_return's and asac_termination_loss_grad's)
 * Step t takes Vn[t] and Vx[t+1]; ratios, step arithmetic, row scan and the TD error are asac_discrete_return's: with
 * beta == 0 and E_sample == 1 the two launches give the same y and TD error.  `args` and `job` as for
 * asac_discrete_return; beta [B, n] and v_options [B, n, num_options] with their strides in floats.  No float atomics:
 * equal inputs give equal bits.  Inputs are finite.
 * n <= ASAC_DISCRETE_MAX_STEPS, num_options <= ASAC_OPTION_MAX_OPTIONS, any B; B == 0 launches nothing.  Bad arguments
 * (asac_discrete_return's, a null beta or v_options, num_options out of range) return hipErrorInvalidValue without a
 * launch. */
int asac_option_discrete_return(const asac_vtrace_args_t* args_host, const asac_discrete_return_t* job_host,
                                const float* beta, int64_t beta_stride_b, int64_t beta_stride_t,
                                const float* v_options, int64_t v_stride_b, int64_t v_stride_t, int64_t v_stride_o,
                                int num_options, void* stream);

/* Q loss of the discrete heads and its gradient (sac_base.py:1533-1538, 1563-1568):
 *   qs[e][b] = (1/K) sum_j a[b][j] q_e[b][j];   loss_out[e] = mean_b w_b (qs - y_b)^2   (w may be NULL)
 *   grad_q[e][b][j] = 2 w_b (qs - y_b) a[b][j] / (K B)      one contiguous [E, B, D] buffer
 * One workgroup per member, the batch mean summed in a fixed order.  q: members' head outputs [B, D] (stride_t not read);
 * action rows action_stride floats apart; y, w: element b at b * stride.  B <= ASAC_DISCRETE_MAX_ROWS. */
int asac_discrete_q_loss_grad(const asac_branches_t* branches, const asac_members_t* q, const float* action,
                              int64_t action_stride, const float* y, int64_t y_stride, const float* w, int64_t w_stride,
                              int B, float* loss_out, float* grad_q, void* stream);

/* Policy objective of the discrete heads, value + gradient with respect to the logits (sac_base.py:1858-1880, 1903):
 *   L = mean_b [ (1/K) sum_j p_j (alpha cl(p_j) - Qbar_j) + (lambda/2) (H_mu - H_pi)^2 ]
 *   H_mu = -(1/K) sum_j mu_j cl(mu_j),  H_pi = (1/K) sum_k H_k
 *   dL_b/dz_i = p_i (g_i - sum_j p_j g_j) + (lambda/K)(H_mu - H_pi) p_i (lp_i + H_k)   per branch, all of it / B
 *   g_j = (1/K)(alpha cl(p_j) - Qbar_j + alpha [p_j >= 1e-8])
 * loss_out f32[1]; grad_logits [B, D] rows grad_stride apart; entropy_out f32[1] = mean_b H_pi.  Optional (may be NULL):
 * probs_out [B, D] contiguous = p, row_entropy_out f32[B] = H_pi per row.  One workgroup;  B <= ASAC_DISCRETE_MAX_ROWS. */
int asac_discrete_policy_loss_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                                   const asac_members_t* q, const int32_t* subset, int E_sample, const float* mu,
                                   int64_t mu_stride, const float* log_alpha, float entropy_penalty, int B,
                                   float* loss_out, float* grad_logits, int64_t grad_stride, float* entropy_out,
                                   float* probs_out, float* row_entropy_out, void* stream);

/* Temperature gradient of the discrete heads (sac_base.py:1924-1929, 1944):
 *   *grad_slot = mean_b (1/K) sum_j p_j (-cl(p_j) - target[j])       target: DEVICE f32[D]
 * grad_slot is the flat-gradient element of log_d_alpha.  Optional probs_out / row_entropy_out as above (the same
 * functions form them: same bits as asac_discrete_policy_loss_grad on the same logits).  One workgroup;
 * B <= ASAC_DISCRETE_MAX_ROWS. */
int asac_discrete_alpha_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                             const float* target, int B, float* grad_slot, float* probs_out, float* row_entropy_out,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hybrid action spaces, policy-based SAC (d_action_sizes set AND c_action_size > 0, discrete_dqn_like False): the
 * learner's row-wise arithmetic around the networks as one launch per item (csrc/hybrid.hip).  The reference's hybrid Q
 * loss, TD error, policy objective and temperature loss each add a discrete and a continuous term per row; each launch
 * forms both.  Notation and tables as above; the continuous head's tensors as for the continuous entry points
 * (asac_vtrace_return_min, asac_q_loss_fwd_bwd, asac_policy_loss_fwd_bwd, asac_alpha_grad).  Batch means: lane partials
 * in a fixed tree, one division by B, no float atomics: equal inputs give equal bits.  Nothing allocates or synchronises.
 * Limits: D <= 64, K <= 8, E <= 8, n <= ASAC_DISCRETE_MAX_STEPS, 1 <= A <= ASAC_MAX_ACTION; the return takes any B, the
 * three single-workgroup reductions B <= ASAC_DISCRETE_MAX_ROWS.  Bad arguments return hipErrorInvalidValue without a
 * launch; B == 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */

/* Both returns of SAC_Base._get_y on a hybrid space (sac_base.py:1383-1464 + _v_trace 1244-1295) in ONE launch.
 *   d_args, job  exactly what asac_discrete_return reads (subset MEANS, branch softmax, log_alpha = log_d_alpha, the
 *                discrete pi / mu under use_n_step_is)
 *   c_args       exactly what asac_vtrace_return_min reads (q [E, B, n+1], subset MINIMUM, logp, log_alpha = log_c_alpha,
 *                pi_prob / mu_prob with mu_offset = D and A; A is checked with and without importance sampling)
 * The two blocks must name the same B, n, reward, masks (pointers and strides), gamma_ratio / lambda_ratio, gamma, v_rho,
 * v_c and use_n_step_is, and different y_out: a step's reward and masks are loaded once for both scans.  Writes
 * d_args->y_out (the bits of asac_discrete_return) and c_args->y_out (the bits of asac_vtrace_return_min).
 * td_error_out (optional) f32[B]: needs job->q_online, job->action, c_args->q_online [E, B] and c_args->E_online == E;
 *   td[b] = (1/E) sum_e (|(1/K) sum_j a_j q_e[b, j] - d_y_b| + |c_q_e[b] - c_y_b|)      (sac_base.py:2233-2244)
 * per member the discrete addend first, members in ascending order.  td_error_out INSIDE either block must be NULL. */
int asac_hybrid_return(const asac_vtrace_args_t* d_args, const asac_vtrace_args_t* c_args,
                       const asac_discrete_return_t* job, float* td_error_out, void* stream);

/* Q loss of a hybrid space and its gradients (sac_base.py:1533-1568), one workgroup per member:
 *   qs[e][b] = (1/K) sum_j a[b][j] q_e[b][j]
 *   loss_out[e] = mean_b w_b [ (qs - d_y_b)^2 + max((tq + clamp(cq - tq, +-eps) - c_y_b)^2, (cq - c_y_b)^2) ]
 *   grad_qd [E, B, D] = d (sum_e l_e) / d (discrete head outputs)   (asac_discrete_q_loss_grad's term)
 *   grad_cq [E, B]    = d (sum_e l_e) / d cq                         (the bits of asac_q_loss_fwd_bwd: same side on ties)
 * q_d: the members' discrete head outputs [B, D]; cq, tq [E, B] contiguous; d_y, c_y, w (may be NULL): element b at
 * b * stride.  clip_eps <= 0 is refused (the reference's doubling quirk there stays with the caller). */
int asac_hybrid_q_loss_grad(const asac_branches_t* branches, const asac_members_t* q_d, const float* action,
                            int64_t action_stride, const float* cq, const float* tq, const float* d_y, int64_t d_y_stride,
                            const float* c_y, int64_t c_y_stride, const float* w, int64_t w_stride, int B, float clip_eps,
                            float* loss_out, float* grad_qd, float* grad_cq, void* stream);

/* Policy objective of a hybrid space, value + gradients (sac_base.py:1858-1903, 1910-1911), one workgroup:
 *   L = mean_b [ ld_b + lc_b ];  ld_b = asac_discrete_policy_loss_grad's row term (entropy penalty included, means over
 *   subset_d of q_d);  lc_b = alpha_c logp_b - min_{e in subset_c} cq[e][b]
 * loss_out f32[1]; grad_logits [B, D] rows grad_stride apart; grad_logp [B] = alpha_c / B and grad_cq [E, B] = -1/B at
 * the first arg-min member of subset_c, 0 elsewhere (the bits of asac_policy_loss_fwd_bwd); d_entropy_out = mean_b H_pi;
 * c_entropy_out = mean_b sum_d (log scale + 1/2 + 1/2 log 2 pi), scale [B, A] rows scale_stride apart.  E = q_d->E
 * members in cq [E, B]; subset_d / subset_c: DEVICE i32[E_sample] or NULL (members 0..E_sample-1). */
int asac_hybrid_policy_loss_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                                 const asac_members_t* q_d, const int32_t* subset_d, const float* mu, int64_t mu_stride,
                                 const float* log_d_alpha, float entropy_penalty, const float* logp, const float* cq,
                                 const int32_t* subset_c, int E_sample, const float* log_c_alpha, const float* scale,
                                 int64_t scale_stride, int A, int B, float* loss_out, float* grad_logits,
                                 int64_t grad_stride, float* grad_logp, float* grad_cq, float* d_entropy_out,
                                 float* c_entropy_out, void* stream);

/* Both temperature gradients (sac_base.py:1924-1944), one workgroup: grad_slots f32[2] = the flat-gradient elements of
 * [log_d_alpha, log_c_alpha];  slot 0 as asac_discrete_alpha_grad (target_d: DEVICE f32[D]), slot 1 =
 * mean_b(-logp_b) - target_c as asac_alpha_grad (logp [B] contiguous).  Each slot has the bits of that launch. */
int asac_hybrid_alpha_grad(const asac_branches_t* branches, const float* logits, int64_t logits_stride,
                           const float* target_d, const float* logp, float target_c, int B, float* grad_slots,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pure-discrete, DQN-like learner (d_action_sizes set, c_action_size == 0, discrete_dqn_like True: critics only): the
 * arithmetic around the critics as three launches (csrc/dqn.hip; the per-row target is csrc/asac_dqn.h's, one
 * implementation for both launches that form it).  Branch table, member tables and limits as above.
 *   eval[e]    online member e's head outputs over the NEXT positions [B, n, D]: position t is window row t + 1
 *   target[e]  target member e's head outputs [B, n+1, D]
 * Double-DQN n-step target (sac_base.py get_dqn_like_d_y 1194-1242, called from _get_y 1363-1382), per row b:
 *   L    = the largest t in [0, n) with !(last[b,t] | pad[b,t]); n - 1 where there is none
 *   j*_k = the LOWEST index of the maximum of eval[subset_n[i]][b, L, branch k]            (torch.argmax), i < E_sample
 *   v_i  = (1/K) sum_k target[subset_next[i]][b, L+1, j*_k]        (the two subsets pair by position i)
 *   y_b  = sum_t gamma_ratio[t] reward[b,t] + gamma^(L+1) min_i v_i (done[b,L] ? 0 : 1)
 * Inputs are finite; nothing is promised for NaN.
 *   args  read: reward / done / last_mask / padding_mask and their strides, gamma_ratio, gamma, subset_n (eval subset),
 *         subset_next (target subset; NULL = 0..E_sample-1 each), E_sample, B, n, y_out, td_error_out.  Nothing else.
 *   action   the stored action at the step's state [B, >= D], rows action_stride floats apart
 *   q_online the online members' head outputs [B, D] at the step's state (stride_t not read)
 * Bad arguments (null outputs, E_sample > E, eval and target tables of different E, D > 64, K > 8, a branch table that
 * does not add up, n > 64, B > 1024 for the loss) return hipErrorInvalidValue without a launch; B == 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    asac_branches_t branches;
    asac_members_t q_eval;
    asac_members_t q_target;
    asac_members_t q_online;
    const float* action;
    int64_t action_stride;
} asac_dqn_job_t;

/* y -> args->y_out.  With args->td_error_out (then job->q_online and job->action are needed) also _get_td_error's
 * sac_base.py:2219-2244:  td[b] = mean over ALL E online members of |(1/K) sum_j a[b,j] q_e[b,j] - y_b|.
 * One lane per row, workgroups of 64 rows, no exchange between them.  n <= ASAC_DISCRETE_MAX_STEPS; any B. */
int asac_dqn_return(const asac_vtrace_args_t* args_host, const asac_dqn_job_t* job_host, void* stream);

/* The Q step's loss launch (sac_base.py:1533-1538, 1563-1568); it forms the target itself:
 *   qs[e][b] = (1/K) sum_j a[b][j] q_e[b][j];   loss_out[e] = mean_b w_b (qs - y_b)^2   (w may be NULL; element b at b * w_stride)
 *   grad_q[e][b][j] = 2 w_b (qs - y_b) a[b][j] / (K B)      one contiguous [E, B, D] buffer
 * One workgroup per online member (job->q_online), each computing its rows' y; workgroup 0 also stores y to
 * args->y_out when that is non-null (the same bits asac_dqn_return writes).  The batch mean is summed in a fixed order.
 * B <= ASAC_DISCRETE_MAX_ROWS. */
int asac_dqn_q_loss_grad(const asac_vtrace_args_t* args_host, const asac_dqn_job_t* job_host, const float* w,
                         int64_t w_stride, float* loss_out, float* grad_q, void* stream);

/* Epsilon-greedy acting (sac_base.py:904-930 without RND), per row: the greedy one-hot of each branch (lowest index at
 * ties) from the first critic's heads q [B, D] (rows q_stride apart).  With u ([B, 1+K] uniforms in [0, 1), rows
 * u_stride apart) and u[b,0] < epsilon, branch k's index is min(floor(u[b,1+k] * s_k), s_k - 1) instead.  u == NULL:
 * greedy only.  Writes every element of the D columns of action_out (rows action_stride apart).  Any B. */
int asac_dqn_act(const asac_branches_t* branches, const float* q, int64_t q_stride, const float* u, int64_t u_stride,
                 float epsilon, float* action_out, int64_t action_stride, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Random network distillation with continuous actions on the stock stacks (csrc/rnd.hip; shared device code
 * csrc/asac_rnd.h).  One "RND stack" is ModelRND.c_dense = LinearLayers(S + A, 64, 2, None): two GELU (erf form)
 * ResBlocks  in -> 64 -> 64,  in = S + A <= ASAC_RND_MAX_IN, biases present, dropout 0, no output Linear
 * (nn.Linear layout: w1 [64][in], w2 [64][64]):
 *   x = [state | action],  z1 = W1 x + b1,  h1 = gelu(z1) + r1 x,  z2 = W2 h1 + b2,  p = gelu(z2) + r2 h1
 * residual[0] = r1 may be 1 only where in == 64 (ResBlock adds its input whenever the widths agree), residual[1] = r2.
 * The four parameter pointers of a stack and the dense outputs are 16-byte aligned; the rows of states, actions,
 * locations and scales may lie at any stride.  Products are f32 MFMA: each sum runs over the inputs in two interleaved
 * blocks-of-16 chains that are added once; GELU is asac_gelu.h's.  No float atomics: equal inputs give equal bits.
 * Bad arguments (a null required pointer, a misaligned parameter or output, in > 128, A > ASAC_MAX_ACTION, k < 1 or
 * k > ASAC_RND_MAX_SAMPLES, r1 at another width, more than ASAC_RND_MAX_ROWS rows) return hipErrorInvalidValue without
 * a launch; B == 0 / batch == 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_RND_WIDTH 64
#define ASAC_RND_MAX_IN 128
#define ASAC_RND_MAX_SAMPLES 64
#define ASAC_RND_MAX_ROWS (1 << 20)
typedef struct {
    int32_t S, A;
    int32_t residual[2];
} asac_rnd_desc_t;
typedef struct {
    const float *w1, *b1, *w2, *b2;
} asac_rnd_stack_t;

/* the limits above: 1 where (S, A) and k candidates per entry are within them (k = 1 for the distillation) */
int asac_rnd_supported(int S, int A, int k);

/* The distillation step without its weight gradients (sac_base.py _train_rnd 1978-2025, continuous branch), ONE launch.
 * Row (b, t) of N = B n rows reads state[b * state_stride_b + t * state_stride_t + 0..S) and action likewise (strides in
 * floats: window views of the step's batch); padding_mask (u8, element (b, t) at b * mask_stride_b + t * mask_stride_t)
 * may be NULL.  With p the predictor's and t the frozen target's output:
 *   d = (p - t) * !pad,   *loss_out = sum d^2 / (N 64),   g = 2 d / (N 64)
 *   gz2 = g gelu'(z2),   gh1 = r2 g + gz2 W2,   gz1 = gh1 gelu'(z1)             (the predictor's pre-activations)
 * Dense outputs: x_cat [N][S + A], h1 [N][64], gz1 [N][64], gz2 [N][64].  The predictor's gradients are products over
 * the rows, formed by asac_xty_multi:  dW2 = gz2^T h1, db2 = colsum gz2, dW1 = gz1^T x_cat, db1 = colsum gz1.
 * workspace: asac_rnd_distill_workspace(N) floats, zero before the first launch and left zero (the workgroups' loss sums
 * are added in workgroup order by the last one to arrive). */
int64_t asac_rnd_distill_workspace(int64_t n_rows);
int asac_rnd_distill(const asac_rnd_desc_t* desc, const asac_rnd_stack_t* predictor, const asac_rnd_stack_t* target,
                     const float* state, int64_t state_stride_b, int64_t state_stride_t, const float* action,
                     int64_t action_stride_b, int64_t action_stride_t, const uint8_t* padding_mask, int64_t mask_stride_b,
                     int64_t mask_stride_t, int B, int n, float* x_cat, float* h1, float* gz1, float* gz2, float* loss_out,
                     float* workspace, void* stream);

/* Novelty-guided acting (sac_base.py rnd_sample_c_action 829-856 and the probability of _choose_action 948-951), ONE
 * launch behind the policy's forward.  state [batch][S] (rows state_stride apart), loc / scale [batch][A] (rows
 * ls_row_stride apart: the two halves of the policy launch's [batch][2A] output), eps [batch][k][A] dense.  Candidate j
 * of an entry is a_j = tanh(loc + scale eps_j) (the bits of asac_squash_sample_fwd), err_j = sum_f (p - t)^2 on
 * [state | a_j];  action_out [batch][A] <- the candidate of the largest err_j (the lowest j among equal maxima, NaN the
 * largest: torch.argmax), prob_out [batch][A] <- its squash-corrected density under (loc, scale) (the bits of
 * asac_squash_prob on that action).  Optional (NULL-able): err_out [batch][k], index_out [batch] (int32).  Whole entries
 * are mapped to a workgroup: an entry's candidates are compared in one place. */
int asac_rnd_pick(const asac_rnd_desc_t* desc, const asac_rnd_stack_t* predictor, const asac_rnd_stack_t* target,
                  const float* state, int64_t state_stride, const float* loc, const float* scale, int64_t ls_row_stride,
                  const float* eps, int k, int batch, float* action_out, float* prob_out, float* err_out, int32_t* index_out,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Random network distillation for a pure-discrete, policy-based learner (csrc/drnd.hip; device code shared with the block
 * above: csrc/asac_rnd.h, and csrc/asac_categorical.h).  ModelRND.d_dense_list holds D = sum of the branch sizes
 * independent stacks LinearLayers(S, 64, 2, None) (the stack of the block above with in = S and no action columns; r1 may
 * be 1 only where S == 64).  A row's action is K concatenated one-hot vectors; per (row, branch) it SELECTS the member at
 * the first non-zero element of the branch, and that element's value is the weight w (1 for every stored action).  A branch
 * without a non-zero element selects nothing.  Rows that are not one-hot per branch are outside the contract.  A member a
 * row did not select is not evaluated for it (the reference multiplies its output by 0, which turns an infinite output
 * into NaN; this path does not).
 * predictors / targets: DEVICE tables of D asac_rnd_stack_t (member m's four parameter pointers, each 16-byte aligned —
 * the caller checks the members when it fills the table; the host side checks the table pointers); residual: HOST int32[2]
 * (r1, r2), the same for all members.  Limits (asac_drnd_supported): S <= ASAC_RND_MAX_IN, D <= ASAC_DRND_MAX_MEMBERS,
 * K <= ASAC_DISCRETE_MAX_BRANCHES, k <= ASAC_RND_MAX_SAMPLES, rows <= ASAC_RND_MAX_ROWS, tables and records 16-byte aligned.
 * Anything outside returns hipErrorInvalidValue without a launch; B == 0 / n_rows == 0 / batch == 0 launches nothing.
 * No float atomics: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_DRND_MAX_MEMBERS 16
typedef struct {
    float *w1, *b1, *w2, *b2;
} asac_rnd_grads_t;

int asac_drnd_supported(int S, int D, int K, int k);

/* The distillation step without its parameter gradients (sac_base.py _train_rnd 1997-2010), ONE launch.  Row (b, t) of
 * N = B n rows reads state and action as asac_rnd_distill does (strides in floats); padding_mask may be NULL.  With P_m,
 * T_m member m of the predictor and of the frozen target and (m_j, w_j) the selection of branch j:
 *   d = sum_j w_j (P_{m_j}(x) - T_{m_j}(x))      (members in ascending order; padded rows select nothing: d = 0)
 *   *loss_out = sum d^2 / (N 64)                 (lanes -> waves -> workgroup in a fixed order; the workgroups' sums are
 *                                                 added in workgroup order by the last one to arrive)
 *   g_j = w_j (2 d / (N 64)),  gz2_j = g_j gelu'(z2),  gh1_j = r2 g_j + gz2_j W2,  gz1_j = gh1_j gelu'(z1)    (of P_{m_j})
 * Outputs: sel i32 [N][K] (m_j or -1), the records h1 / gz1 / gz2 f32 [N][K][64] (zeros where sel is -1), x [N][S].
 * workspace: asac_drnd_distill_workspace(N) floats (the workgroups' sums, then the arrival counter), zero before the first
 * launch; every launch leaves the COUNTER zero — the sums stay in their slots and are rewritten by the next launch. */
int64_t asac_drnd_distill_workspace(int64_t n_rows);
int asac_drnd_distill(const asac_branches_t* branches, int S, const int32_t* residual, const asac_rnd_stack_t* predictors,
                      const asac_rnd_stack_t* targets, const float* state, int64_t state_stride_b, int64_t state_stride_t,
                      const float* action, int64_t action_stride_b, int64_t action_stride_t, const uint8_t* padding_mask,
                      int64_t mask_stride_b, int64_t mask_stride_t, int B, int n, int32_t* sel, float* x, float* h1, float* gz1,
                      float* gz2, float* loss_out, float* workspace, void* stream);

/* The predictor's parameter gradients from those records (autograd's walk through the D stacks), ONE launch.  For member
 * m of branch j, over the rows r with sel[r][j] == m in ASCENDING order (fmaf chains, float32):
 *   dW2_m = sum gz2[r][j]^T h1[r][j],  db2_m = sum gz2[r][j],  dW1_m = sum gz1[r][j]^T x[r],  db1_m = sum gz1[r][j]
 * grads: DEVICE table of D asac_rnd_grads_t (member m's four gradient views, nn.Linear layout).  Every element of all D
 * members' views is overwritten (zeros for a member nobody selected).  Rows are split in at most 64 chunks; the chunks'
 * sums are added in chunk order by the member's last arriver.  workspace: asac_drnd_param_grads_workspace(N, S, D)
 * floats (the chunks' sums, then one arrival counter a member), zero before the first launch; every launch leaves the
 * counters zero. */
int64_t asac_drnd_param_grads_workspace(int64_t n_rows, int S, int D);
int asac_drnd_param_grads(const asac_branches_t* branches, int S, const int32_t* sel, const float* x, const float* h1,
                          const float* gz1, const float* gz2, int64_t n_rows, const asac_rnd_grads_t* grads, float* workspace,
                          void* stream);

/* Novelty-guided acting (sac_base.py rnd_sample_d_action 793-826 and the probability of _choose_action 957-961), ONE
 * launch behind the policy's logits.  state [batch][S] (rows state_stride apart), logits [batch][D] (rows logits_stride
 * apart), u [batch][k][K] dense uniforms in [0, 1).  p = the branch softmax (the bits of asac_discrete_policy_loss_grad's
 * probs_out).  Candidate c's index in a branch of s entries is #{i < s - 1 : c_i <= u}, c_i the running float32 sum of p in
 * index order;  err_c = sum_f (sum_j E_{m_j}[f])^2 with E_m = P_m(x) - T_m(x), j and then f in ascending order.
 * action_out [batch][D] <- the one-hot candidate of the largest err (the lowest c among equal maxima, NaN the largest:
 * torch.argmax), every element written; prob_out [batch][D] <- p.  Optional (NULL-able): err_out [batch][k], cand_out i32
 * [batch][k][K], index_out i32 [batch].  An entry is decided inside one workgroup. */
int asac_drnd_pick(const asac_branches_t* branches, int S, const int32_t* residual, const asac_rnd_stack_t* predictors,
                   const asac_rnd_stack_t* targets, const float* state, int64_t state_stride, const float* logits,
                   int64_t logits_stride, const float* u, int k, int batch, float* action_out, float* prob_out, float* err_out,
                   int32_t* cand_out, int32_t* index_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Head banks: the discrete-action branch stacks of a critic ensemble or of a policy (csrc/head_bank.hip; nn_models
 * ModelQ.d_dense_list / ModelPolicy.d_dense_list).  A bank is G groups of K stacks, M = G K in all, every one reading the
 * same rows x [N][S].  Stack (g, k) is LinearLayers(S, W, depth, size_k): depth ResBlocks
 *   z_l = W_l h_l + b_l,  h_{l+1} = gelu(z_l) + residual[l] h_l        (h_0 = x; erf-form GELU on the library's erff)
 * and the output Linear(W, size_k).  depth, W, residual and the branch sizes belong to the bank; only the parameters differ.
 * Limits (asac_head_bank_supported): W <= ASAC_HEAD_BANK_MAX_WIDTH (tiles of 64 or 128 features; a narrower stack runs on
 * zero-padded tiles: a padded feature is gelu(0) = 0 and carries no cotangent), S <= ASAC_HEAD_BANK_MAX_IN, 1 <= depth <=
 * ASAC_HEAD_BANK_MAX_DEPTH, K <= ASAC_DISCRETE_MAX_BRANCHES, D = sum size_k <= ASAC_DISCRETE_MAX_WIDTH, G <=
 * ASAC_HEAD_BANK_MAX_GROUPS, M <= ASAC_HEAD_BANK_MAX_STACKS, N <= ASAC_HEAD_BANK_MAX_ROWS; residual[0] only where S == W.
 * params: a DEVICE table of M records of 2 (depth + 1) pointers, stack m = g K + k:  w_0, b_0, .., w_{depth-1}, b_{depth-1},
 * head w, head b  (nn.Linear layout, out x in).  The pointers need float alignment only: the stacks of one network lie back
 * to back in a flat buffer, and every load of a parameter and store of a gradient is one dword.  grads: the same table of
 * the gradient views.  Row r of N = samples * steps reads x + (r / steps) x_stride_sample + (r % steps) x_stride_step (in
 * floats; the S features dense): a [samples][steps][S] window is read in place.
 * A workgroup owns (tile of 16 rows, stack); the activations stay in LDS, one layer's weights are staged at a time, the
 * products are __builtin_amdgcn_mfma_f32_16x16x4f32.  Nothing allocates or synchronises; no float atomics: equal inputs
 * give equal bits.  Bad arguments (a null required pointer, a size outside the limits, residual[0] at S != W, a branch
 * table that does not add up) return hipErrorInvalidValue without a launch; N == 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_HEAD_BANK_MAX_DEPTH 3
#define ASAC_HEAD_BANK_MAX_WIDTH 128
#define ASAC_HEAD_BANK_MAX_IN 128
#define ASAC_HEAD_BANK_MAX_GROUPS 8
#define ASAC_HEAD_BANK_MAX_STACKS 64
#define ASAC_HEAD_BANK_MAX_ROWS (1 << 20)
typedef struct {
    int32_t S, W, depth, G;
    int32_t residual[ASAC_HEAD_BANK_MAX_DEPTH];
    int32_t reserved_;
    asac_branches_t branches;
} asac_head_bank_t;

int asac_head_bank_supported(int S, int W, int depth, int K, int D, int G);

/* out [G][N][D] (dense): out[g][r][off_k .. off_k + size_k) <- stack (g, k) on row r, off_k the branch's first column —
 * each group's branches arrive concatenated.  ONE launch, grid (row tiles, M). */
int asac_head_bank_forward(const asac_head_bank_t* bank, const float* const* params, const float* x, int64_t x_stride_sample,
                           int64_t x_stride_step, int64_t samples, int steps, float* out, void* stream);

/* The gradients for grad_out [G][N][D] (dense), TWO launches; nothing is kept from the forward: it is redone on chip.
 *   launch 1, grid (row tiles, M): the forward, then the chain  gz_l = gh_{l+1} gelu'(z_l),  gh_l = gz_l W_l + residual[l]
 *     gh_{l+1}  back from the head; the layers' inputs and cotangents go to records in the workspace.  With grad_x non-NULL
 *     ([N][S] dense, every element written) each stack's gh_0 is published and the tile's last arriver adds the M of them
 *     in ascending stack order (csrc/asac_ordered_finish.h).
 *   launch 2, grid (blocks of 16 outputs, depth + 1 layers, M): dW = sum_r gz[r]^T h[r], db = sum_r gz[r] on the matrix
 *     pipe (float64 MFMA on the float32 records, rounded once), rows in ascending order inside one workgroup: no
 *     cross-workgroup sum.  Every element of every view of the grads
 *     table is written (accumulate == 0) or added to (accumulate != 0).  grads == NULL: launch 1 only (grad_x required).
 * workspace: asac_head_bank_backward_workspace(N, S, W, depth, D, M) floats (-1 outside the limits), 16-byte aligned, zero
 * before its first use; every launch leaves its counters zero. */
int64_t asac_head_bank_backward_workspace(int64_t n_rows, int S, int W, int depth, int D, int M);
int asac_head_bank_backward(const asac_head_bank_t* bank, const float* const* params, float* const* grads, const float* x,
                            int64_t x_stride_sample, int64_t x_stride_step, int64_t samples, int steps, const float* grad_out,
                            float* grad_x, int accumulate, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Acting of a policy-based learner on the policy's head outputs (csrc/act.hip; sac_base.py _choose_action 931-966 and
 * _random_action 858-880, operators.py squash_correction_prob 17-19): discrete branches, continuous actions or both, sampled
 * or deterministic, with or without action_noise, as ONE launch.  One lane per row, workgroups of 64 rows, no exchange
 * between them; any B, B == 0 launches nothing.  It allocates nothing and synchronises nothing.
 *
 * Row b of B, branches (K, D) and A continuous actions (either part may be absent, not both):
 *   noise_b  = torch.linspace(noise_lo, noise_hi, B)[b] in float32: step = (hi - lo) / (B - 1),
 *              b < B / 2 ? fma(step, b, lo) : fma(-step, B - 1 - b, hi);  lo at B == 1
 *   branch k (s_k entries, logits z):  p = softmax(z) (the bits of asac_discrete_policy_loss_grad's probs_out)
 *     sampled        index = #{i < s_k - 1 : c_i <= u[b, k]}, c the running float32 sum of p in index order (asac_drnd_pick's
 *                    rule), then lowered to the last entry with p > 0: an entry of probability zero is never returned
 *     deterministic  index = the first maximum of z
 *     with noise     u[b, gate] < noise_b: every branch's index becomes min(floor(u[b, idx_k] * s_k), s_k - 1) (asac_dqn_act's
 *                    rule for its random rows)
 *   continuous  (loc, scale) as given, or with head_raw = 1 loc = tanh(mean / 5) * 5, scale = exp(clamp(logstd, -20, 0.5))
 *     sampled        a = tanh(loc + eps[b, d] * scale)         (the bits of asac_squash_sample_fwd's a_tanh)
 *     deterministic  a = tanh(loc)
 *     with noise     a = tanh(atanh(a) + eps[b, noise_d] * noise_b), infinities included
 *   action_out[b] = (one-hot per branch | a)                            D + A floats, every one written
 *   prob_out[b]   = (p | exp(N(loc, scale).log_prob(x_d)) / prod_e max(1 - tanh(x_e)^2, 1e-2)), x = atanh(clamp(a, +-0.999))
 *                   (the bits of asac_squash_prob on the returned action)
 *
 * Draw buffers, float32, rows u_stride / eps_stride floats apart; the caller fills them (uniforms in [0, 1), standard
 * normals).  Columns, in this order, a group being ABSENT (not skipped) when its condition fails:
 *   u    [K sampling columns: !deterministic] [1 gate column, K index columns: use_noise]         (none without branches)
 *   eps  [A sampling columns: !deterministic] [A noise columns: use_noise]                       (none when A == 0)
 * A buffer of no columns may be NULL.
 *
 * Limits: K <= ASAC_DISCRETE_MAX_BRANCHES, D <= ASAC_DISCRETE_MAX_WIDTH, A <= ASAC_ACT_MAX_CONT.  branches.K == 0: no
 * discrete part (logits not read); A == 0: no continuous part (loc / scale not read).  Bad arguments (null outputs, a branch
 * table that does not add up, sizes over the limits, neither part present, a missing input or draw buffer the mode needs,
 * noise_lo > noise_hi, negative or NaN noise, B < 0) return hipErrorInvalidValue without a launch.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_ACT_MAX_CONT 8

typedef struct {
    asac_branches_t branches;      /* K == 0: no discrete part */
    const float* logits;           /* [B, D], rows logits_stride floats apart */
    int64_t logits_stride;
    const float* loc;              /* [B, A] each, rows ls_row_stride floats apart: two pointers, so that they may be the */
    const float* scale;            /* two halves of a [B, 2A] row */
    int64_t ls_row_stride;
    int32_t A;
    int32_t head_raw;              /* 1: loc / scale hold the stock policy's (mean, logstd) before the bounding */
    const float* u;
    int64_t u_stride;
    const float* eps;
    int64_t eps_stride;
    int32_t deterministic;
    int32_t use_noise;
    float noise_lo, noise_hi;
    float* action_out;             /* [B, D + A], rows action_stride floats apart */
    int64_t action_stride;
    float* prob_out;               /* [B, D + A], rows prob_stride floats apart */
    int64_t prob_stride;
    int32_t B;
    int32_t reserved_;
} asac_act_job_t;

/* 1 when (branches, A) is within the limits above (branches NULL or K == 0: no discrete part), else 0 */
int asac_act_sizes_ok(const asac_branches_t* branches, int A);
int asac_act_policy(const asac_act_job_t* job_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Siamese representation losses (csrc/siamese.hip; sac_base.py _train_siamese_representation_learning 1633-1796), loss
 * and gradients in ONE launch each.  All tensors float32 with dense rows.  No float atomics: equal inputs give equal bits.
 * Anything outside the limits, a NULL pointer or N == 0 returns hipErrorInvalidValue without a launch.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_SIAMESE_MAX_WIDTH 128
#define ASAC_SIAMESE_MAX_BLOCK 64
#define ASAC_SIAMESE_MAX_ROWS 16384
#define ASAC_SIAMESE_BYOL_MAX_WIDTH 256
#define ASAC_SIAMESE_BYOL_MAX_ROWS (1 << 20)
#define ASAC_SIAMESE_BYOL_WORKSPACE_FLOATS 257

/* ATC.  e [N][E] online and te [N][E] target encoders, w [E][E], pad [N] row weights, n the block length (n divides N):
 *   z = e w,  l_ij = z_i . te_j,  y_ij = (i / n == j / n)
 *   *loss_out = (1 / N^2) sum_ij pad_i (max(l, 0) - l y + log1p(exp(-|l|)))
 *   dl_ij = pad_i (sigmoid(l_ij) - y_ij) / N^2,  dz = dl te,  g_w [E][E] = e^T dz,  g_e [N][E] = dz w^T
 * l, y and dl stay in registers; the products over te are v_mfma_f32_16x16x4_f32.  Limits: 1 <= E <= ASAC_SIAMESE_MAX_WIDTH,
 * 1 <= n <= ASAC_SIAMESE_MAX_BLOCK, 1 <= N <= ASAC_SIAMESE_MAX_ROWS.  Every element of the three outputs is written.
 * workspace: asac_siamese_atc_workspace_floats(N, E) floats (-1 outside the limits), zero before the first launch; every
 * launch leaves its counters zero and rewrites the partial sums it reads (added in workgroup order by the last to arrive). */
int64_t asac_siamese_atc_workspace_floats(int64_t N, int E);
int asac_siamese_atc_loss_grad(const float* e, const float* te, const float* w, const float* pad, int64_t N, int E, int n,
                               float* loss_out, float* g_e, float* g_w, float* workspace, void* stream);

/* BYOL.  pred [N][P], t_proj [N][P], pad [N]:
 *   c_i = (pred_i / max(|pred_i|, 1e-8)) . (t_proj_i / max(|t_proj_i|, 1e-8))     (torch's cosine_similarity, whose clamp
 *                                                  is outside autograd: the gradient runs through |pred_i| either way)
 *   *loss_out = (1 / N) sum_i pad_i c_i,   g_pred [N][P] = d loss / d pred
 * Limits: 1 <= P <= ASAC_SIAMESE_BYOL_MAX_WIDTH, 1 <= N <= ASAC_SIAMESE_BYOL_MAX_ROWS.
 * workspace: ASAC_SIAMESE_BYOL_WORKSPACE_FLOATS floats, zero before the first launch and left ready by every launch. */
int asac_siamese_byol_loss_grad(const float* pred, const float* t_proj, const float* pad, int64_t N, int P, float* loss_out,
                                float* g_pred, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image augmentations (csrc/image.hip; algorithm/utils/image_transforms.py), ONE launch per call, one 256-thread workgroup
 * per plane (a grid of at most 512: beyond that a workgroup takes several planes in turn).
 * x [planes][H][W] -> y [planes][Ho][Wo], float32, contiguous; planes = frames * C.  The plane is staged in LDS,
 * so H * W <= ASAC_IMAGE_MAX_PLANE (two planes and the taps of two workgroups fit a CU's 160 KiB).
 *
 * `ops`: a HOST table of 1 .. ASAC_IMAGE_MAX_OPS descriptors, copied into the launch.  One entry: that op.  Several: one is
 * picked per call, uniformly, ON THE DEVICE.  Every op but CROP_RESIZE needs Ho == H and Wo == W.
 *   COPY           y = x
 *   BLUR           separable Gaussian, kx / ky taps (odd, <= ASAC_IMAGE_MAX_KERNEL, k / 2 < the plane's extent), reflect
 *                  indexing; sigma = lo, or uniform in [lo, hi) per call; w = exp(-0.5 (x / sigma)^2) over
 *                  x = linspace(-(k - 1) / 2, (k - 1) / 2, k), normalised, computed in the kernel
 *   BRIGHTNESS     y = clamp(x * f, 0, 1), f = lo or uniform in [lo, hi) per call
 *   CROP_RESIZE    the window [top, top + crop_h) x [left, left + crop_w) resampled to Ho x Wo, bilinear, align_corners =
 *                  False; Ho >= crop_h and Wo >= crop_w only (no antialiasing is needed then); equal sizes copy the
 *                  window's bits.  top / left >= 0: fixed; -1: uniform over the valid offsets per call
 *   SALT_PEPPER    one draw r per (frame, pixel), shared by the frame's C planes: r < b adds a, r > c subtracts a, clamped
 *   UNIFORM_NOISE  y = clamp(x + r * b + a, 0, 1), one draw per element
 *
 * Draws.  `state`: 16 bytes owned by the caller, zero-initialised: an int64 draw counter, then the arrival word.  Every
 * workgroup reads the counter and derives the call's choice, offsets, sigma / factor and its pixels' noise from
 * Philox4x32-10(seed, instance (28 bits), counter); the last workgroup to arrive stores counter + 1 and leaves the arrival
 * word zero.  No host value is involved: a captured launch draws afresh on every replay.  `state` may be NULL only for a
 * table that draws nothing.  `drawn` (NULL or 6 doubles) receives counter, choice, top, left, sigma, factor of this call
 * (-1 / NaN where the chosen op has none).  Anything outside the limits returns hipErrorInvalidValue without a launch.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_IMAGE_MAX_OPS 8
#define ASAC_IMAGE_MAX_PLANE 9216
#define ASAC_IMAGE_MAX_KERNEL 31
#define ASAC_IMAGE_COPY 0
#define ASAC_IMAGE_BLUR 1
#define ASAC_IMAGE_BRIGHTNESS 2
#define ASAC_IMAGE_CROP_RESIZE 3
#define ASAC_IMAGE_SALT_PEPPER 4
#define ASAC_IMAGE_UNIFORM_NOISE 5

typedef struct {
    int32_t kind;
    int32_t kx, ky;            /* BLUR */
    int32_t crop_h, crop_w;    /* CROP_RESIZE */
    int32_t top, left;         /* CROP_RESIZE: fixed offsets, -1: drawn */
    float lo, hi;              /* BLUR: sigma range; BRIGHTNESS: factor range (lo == hi: fixed) */
    float a, b, c;             /* SALT_PEPPER: amount, lower and upper threshold; UNIFORM_NOISE: mean, std */
} asac_image_op_t;

int asac_image_augment(const float* x, float* y, int64_t planes, int C, int H, int W, int Ho, int Wo, const asac_image_op_t* ops,
                       int n_ops, uint64_t seed, uint32_t instance, int64_t* state, double* drawn, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image warps (csrc/image.hip; `RandomResizedCrop` and `ElasticTransform` of algorithm/utils/image_transforms.py with
 * NEAREST interpolation), ONE launch per call.  x [planes][H][W] -> y [planes][Ho][Wo], float32, contiguous;
 * H * W <= ASAC_IMAGE_MAX_PLANE.  Every output pixel is a copy of an input pixel's bits (or zero): the planes are gathered
 * straight from global memory, a workgroup of the capped grid takes several planes in turn.
 *
 * `ops`: a HOST table of 1 .. ASAC_IMAGE_MAX_OPS descriptors, copied into the launch; several: one is picked per call,
 * uniformly, on the device.  Every op but RESIZED_CROP needs Ho == H and Wo == W.
 *   COPY          y = x
 *   RESIZED_CROP  torchvision's window rule: up to 10 tries of area = H W U(scale), aspect = exp(U(log ratio)),
 *                 w = rint(sqrt(area aspect)), h = rint(sqrt(area / aspect)), the first with 0 < w <= W and 0 < h <= H wins
 *                 and its offsets are drawn uniformly; after 10 rejections the central window of the nearest allowed aspect.
 *                 The window is resampled to Ho x Wo by torch's legacy nearest rule,
 *                 src = min(floor(dst * (float)in / out), in - 1): shrinking and enlarging alike.
 *   ELASTIC       one displacement field per call, shared by all planes: 2 H W uniforms in [-1, 1), field f (0: x, 1: y)
 *                 blurred separably with k_f taps on both axes (odd, <= ASAC_IMAGE_WARP_MAX_KERNEL, k / 2 < min(H, W);
 *                 the taps along x from sigma0, along y from sigma1, both > 0; reflect indexing) and scaled by alpha0 / H
 *                 (x) or alpha1 / W (y).  Pixel (i, j) reads the input at the rounded (half to even) unnormalised
 *                 coordinate ((g + 1) * n - 1) / 2 of g = linspace((1 - n) / n, (n - 1) / n, n)[.] + field, zero outside.
 *                 Every workgroup builds the field in LDS (3 H W floats) from the call's Philox stream.
 *
 * Draws: `state`, seed, instance and the last-arriver finish exactly as for asac_image_augment; `state` may be NULL only
 * for a table that is one COPY.  `drawn` (NULL or 6 doubles) receives counter, choice, top, left, height, width of this call
 * (-1 where the chosen op has no window).  `noise_out` / `disp_out`: NULL, or [2][H][W] floats that receive the field's raw
 * noise and the final displacement (x, then y, in grid units) when the chosen op is ELASTIC.
 * Anything outside the limits returns hipErrorInvalidValue without a launch.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_IMAGE_WARP_MAX_KERNEL 63
#define ASAC_IMAGE_WARP_COPY 0
#define ASAC_IMAGE_WARP_RESIZED_CROP 1
#define ASAC_IMAGE_WARP_ELASTIC 2

typedef struct {
    int32_t kind;
    int32_t k0, k1;                 /* ELASTIC: taps of the x field, of the y field */
    float scale_lo, scale_hi;       /* RESIZED_CROP: the window's share of the frame's area */
    float ratio_lo, ratio_hi;       /* RESIZED_CROP: its aspect w / h */
    float alpha0, alpha1;           /* ELASTIC */
    float sigma0, sigma1;           /* ELASTIC */
} asac_image_warp_op_t;

int asac_image_warp(const float* x, float* y, int64_t planes, int C, int H, int W, int Ho, int Wo,
                    const asac_image_warp_op_t* ops, int n_ops, uint64_t seed, uint32_t instance, int64_t* state, double* drawn,
                    float* noise_out, float* disp_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Observation normalization (csrc/normalize.hip; `use_normalization` of the reference, sac_base.py:302-336 and 766-781).
 * Both entry points take a HOST table of 1 .. ASAC_NORM_MAX_OBS jobs, one per observation, copied into the launch.
 *
 * asac_obs_whiten: ONE launch for all observations of a call.  Per element, with j the index inside the row,
 *     dst = clamp((src - mean[j]) / sqrt(variance[j] / (float)(*step + 1)), -5, 5)
 * — the module expression's operations in its order: IEEE divide and square root, the int32 `step + 1` rounded to float
 * as torch's promotion does, NaN kept as torch.clamp keeps it.  `step`, `mean` and `variance` are read from device memory
 * when the launch RUNS: a captured launch replayed after a later update whitens with the newer statistics.
 *   src / dst   float32, `rows` rows of D elements, consecutive rows `*_row_pitch` elements apart (0: D, dense).
 *               dst == src with equal pitches (in place) is allowed; any other overlap is refused.
 *   16-byte units where D, both pitches and all four pointers allow it, else 4-byte units.
 *
 * asac_normalizer_update: ONE launch per episode of T rows for all observations.  Per column j of a job
 *     step' = step + T;  d_t = x_t - mean;  mean' = mean + sum_t (d_t / (float)step');
 *     variance' = variance + sum_t (x_t - mean') * d_t
 *   x       [T][D] rows `x_row_pitch` elements apart (0: D), ASAC_NORM_F32, or ASAC_NORM_U8 taken as its integer value
 *   order   row t belongs to lane t mod ASAC_NORM_ROW_LANES, every lane adds its rows in ascending t, the lane partials
 *           are combined by the binary tree p[l] += p[l + off], off = LANES / 2 .. 1.  No float atomics: equal inputs
 *           give equal bits.  A workgroup owns 64 columns and all their rows; no float crosses a workgroup.
 *   step    int32 on the device; every workgroup reads it, the LAST to arrive at `counter` writes step + T.
 *   counter one zeroed 32-bit word (asac_ordered_finish.h); every launch leaves it zero.
 * Under the measurement repeat knob only the first repetition writes.
 * Anything outside the limits returns hipErrorInvalidValue without a launch.
 * ------------------------------------------------------------------------------------------- */
#define ASAC_NORM_MAX_OBS 8
#define ASAC_NORM_ROW_LANES 64
#define ASAC_NORM_F32 0
#define ASAC_NORM_U8 1

typedef struct {
    const float* src;
    float* dst;
    const float* mean;             /* [D] */
    const float* variance;         /* [D] */
    int64_t D;
    int64_t rows;
    int64_t src_row_pitch;         /* elements; 0: D */
    int64_t dst_row_pitch;
} asac_whiten_job_t;

typedef struct {
    const void* x;
    float* mean;                   /* [D], updated in place */
    float* variance;
    int64_t D;
    int64_t x_row_pitch;           /* elements; 0: D */
    int32_t dtype;                 /* ASAC_NORM_F32 | ASAC_NORM_U8 */
    int32_t reserved_;
} asac_normalizer_job_t;

int asac_normalizer_row_lanes(void);
int asac_obs_whiten(const asac_whiten_job_t* jobs_host, int n_jobs, const int32_t* step, void* stream);
int asac_normalizer_update(const asac_normalizer_job_t* jobs_host, int n_jobs, int T, int32_t* step,
                           unsigned int* counter, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASAC_HIP_H */
