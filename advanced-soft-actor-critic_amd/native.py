"""ctypes binding of `libasac_hip.so` (C ABI: `include/asac_hip.h`).  The signatures, the structs and the `ASAC_*` constants
are not restated here: `abi.py` reads them from the header, and this module names the structs and wraps the entry points.

There is NO fallback: if the library is missing or a launch fails this module raises.  torch must
be imported before the library is loaded so that both bind to the same `libamdhip64.so.7` (the HIP
runtime bundled with PyTorch-ROCm), which is what lets these kernels run on torch's streams, on
torch-allocated HBM, and inside torch-captured hipGraphs.
"""
import ctypes as C
import math
from pathlib import Path

import torch  # noqa: F401  (must precede the dlopen below, see module docstring)

from . import abi as _abi
from .abi import AsacNativeError  # noqa: F401  (every failure of this binding raises it)

PKG_DIR = Path(__file__).resolve().parent
import os as _os

LIB_PATH = Path(_os.environ.get('ASAC_HIP_LIB', PKG_DIR / 'lib' / 'libasac_hip.so'))   # env override: debugging builds


def _defined(*names):
    """the header's integer constants `ASAC_<name>` (a `#define` or an enumerator)"""
    values = tuple(_abi.defines['ASAC_' + n] for n in names)
    return values if len(values) > 1 else values[0]


ABI_VERSION = _defined('ABI_VERSION')

MAX_GATHER_KEYS = _defined('MAX_GATHER_KEYS')
PAD_KEEP, PAD_WORD, PAD_BYTE, PAD_ROW, PAD_EMIT_MASK = _defined('PAD_KEEP', 'PAD_WORD', 'PAD_BYTE', 'PAD_ROW', 'PAD_EMIT_MASK')
CVT_NONE, CVT_U8_TO_F32_UNIT, CVT_BOOL_TO_F32 = _defined('CVT_NONE', 'CVT_U8_TO_F32_UNIT', 'CVT_BOOL_TO_F32')
ROW_ITEM, ROW_SLOT, ROW_SLOT_ROW, ROW_BROADCAST = _defined('ROW_ITEM', 'ROW_SLOT', 'ROW_SLOT_ROW', 'ROW_BROADCAST')
DERIVE_NONE, DERIVE_PREVIOUS, DERIVE_HOLD_LAST, DERIVE_HOLD_LAST_NEXT = _defined(
    'DERIVE_NONE', 'DERIVE_PREVIOUS', 'DERIVE_HOLD_LAST', 'DERIVE_HOLD_LAST_NEXT')
DISCRETE_MAX_WIDTH, DISCRETE_MAX_BRANCHES, DISCRETE_MAX_MEMBERS, DISCRETE_MAX_STEPS, DISCRETE_MAX_ROWS = _defined(
    'DISCRETE_MAX_WIDTH', 'DISCRETE_MAX_BRANCHES', 'DISCRETE_MAX_MEMBERS', 'DISCRETE_MAX_STEPS', 'DISCRETE_MAX_ROWS')
ACT_MAX_CONT = _defined('ACT_MAX_CONT')
MLP_MAX_JOBS = _defined('MLP_MAX_JOBS')
SIDECAR_ALPHA_ADAM, SIDECAR_SCATTER_ELECT, SIDECAR_SCATTER_WRITE, SIDECAR_WINDOW_GATHER, SIDECAR_WINDOW_GATHER_W = _defined(
    'SIDECAR_ALPHA_ADAM', 'SIDECAR_SCATTER_ELECT', 'SIDECAR_SCATTER_WRITE', 'SIDECAR_WINDOW_GATHER', 'SIDECAR_WINDOW_GATHER_W')
MAX_SIDECARS = _defined('MAX_SIDECARS')
SQUASH_MAX_JOBS = _defined('SQUASH_MAX_JOBS')
GRU_MAX_LAYERS, GRU_MAX_DIM = _defined('GRU_MAX_LAYERS', 'GRU_MAX_DIM')
# the policy forward's sampling epilogue (`mlp_forward_multi_sampled`) instead of a `squash_multi` launch behind it;
# ASAC_SAMPLE_EPILOGUE=0: the chain (A/B runs)
SAMPLE_EPILOGUE = _os.environ.get('ASAC_SAMPLE_EPILOGUE', '1') != '0'

# The structs of the header, one line each; fields, in the header's order, and layouts are `abi.ctypes_struct`'s
# (tests/test_abi_host.py holds every size and offset to the host C compiler's).  A new struct of the header needs its
# line here: `abi.signatures` refuses a header struct that has none.
GatherKey = _abi.ctypes_struct('asac_gather_key_t')
RowMove = _abi.ctypes_struct('asac_row_move_t')
Sidecar = _abi.ctypes_struct('asac_sidecar_t')
SquashJob = _abi.ctypes_struct('asac_squash_job_t')
VtraceArgs = _abi.ctypes_struct('asac_vtrace_args_t')
MlpDesc = _abi.ctypes_struct('asac_mlp_desc_t')
MlpJob = _abi.ctypes_struct('asac_mlp_job_t')
SampleEpilogue = _abi.ctypes_struct('asac_mlp_sample_epilogue_t')
RingKey = _abi.ctypes_struct('asac_ring_key_t')
RingRows = _abi.ctypes_struct('asac_ring_rows_t')
PiQJob = _abi.ctypes_struct('asac_pi_q_job_t')
GruDesc = _abi.ctypes_struct('asac_gru_desc_t')
AdamEpilogue = _abi.ctypes_struct('asac_adam_epilogue_t')
Conv2Desc = _abi.ctypes_struct('asac_conv2_desc_t')
Conv1Desc = _abi.ctypes_struct('asac_conv1_desc_t')
ObsDecoderParams = _abi.ctypes_struct('asac_obs_decoder_params_t')
PartialSum = _abi.ctypes_struct('asac_partial_sum_t')
BatchPutKey = _abi.ctypes_struct('asac_batch_put_key_t')
BatchGatherKey = _abi.ctypes_struct('asac_batch_gather_key_t')
Branches = _abi.ctypes_struct('asac_branches_t')
Members = _abi.ctypes_struct('asac_members_t')
DiscreteReturn = _abi.ctypes_struct('asac_discrete_return_t')
DqnJob = _abi.ctypes_struct('asac_dqn_job_t')
RndDesc = _abi.ctypes_struct('asac_rnd_desc_t')
RndStack = _abi.ctypes_struct('asac_rnd_stack_t')
RndGrads = _abi.ctypes_struct('asac_rnd_grads_t')
ActJob = _abi.ctypes_struct('asac_act_job_t')
ImageOp = _abi.ctypes_struct('asac_image_op_t')
ImageWarpOp = _abi.ctypes_struct('asac_image_warp_op_t')
WhitenJob = _abi.ctypes_struct('asac_whiten_job_t')
NormalizerJob = _abi.ctypes_struct('asac_normalizer_job_t')
HeadBankDesc = _abi.ctypes_struct('asac_head_bank_t')
_PtrArray = C.c_void_p * GRU_MAX_LAYERS

# every entry point of the header: {name: (restype, [argtypes])} by the typing rule of abi.py
_SIGNATURES = _abi.signatures([v for v in list(globals().values()) if isinstance(v, type) and issubclass(v, C.Structure)])
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def adam_epilogue(param_flat, grad_flat, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, steps_done) -> AdamEpilogue:
    """The optimizer step a gradient-finishing launch takes itself (`asac_adam_epilogue_t`): flat buffers of one
    layout; the gradients the launch writes must be views of `grad_flat`."""
    for t in (param_flat, grad_flat, exp_avg, exp_avg_sq):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == param_flat.numel()
    assert steps_done.dtype == torch.int64 and steps_done.is_cuda
    ep = AdamEpilogue(param_flat.data_ptr(), grad_flat.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                      float(lr), float(beta1), float(beta2), float(eps), steps_done.data_ptr())
    ep._keep = (param_flat, grad_flat, exp_avg, exp_avg_sq, steps_done)
    ep._span = (grad_flat.data_ptr(), grad_flat.data_ptr() + 4 * grad_flat.numel())
    return ep


_lib = None


def load() -> C.CDLL:
    """dlopen the library (once) and type every entry point; raises if absent or ABI-mismatched."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise AsacNativeError(
            f'{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). '
            'There is no CPU or eager fallback for the SAC hot path.')
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.asac_version() != ABI_VERSION:
        raise AsacNativeError(f'libasac_hip.so ABI {lib.asac_version()} != binding {ABI_VERSION}; rebuild')
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise AsacNativeError(f'{what} failed (hipError {rc}): {load().asac_last_error().decode()}')


def _p(t):
    """device pointer of a tensor (or None)"""
    if t is None:
        return None
    assert t.is_cuda, 'libasac_hip kernels take device memory only'
    return C.c_void_p(t.data_ptr())


def _stream():
    # (the raw handle of torch's current stream on the current device; `torch.cuda.current_stream().cuda_stream` builds
    # a Stream object per call: 13 us of host time in front of every eager launch)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


class LaunchProfiler:
    """Per-entry-point device time from HIP events recorded on the launch stream (eager mode only:
    nothing is recorded while a graph is being captured).  A single launch here lasts 3-10 us, which
    is below both what one event pair resolves and the host cost of issuing it through ctypes, so
    while the profiler is active the library re-issues every launch `repeat` times back-to-back
    (`asac_set_launch_repeat`) and the elapsed time is divided by `repeat`.  Used by bench.py's
    profile pass AFTER the timed region, where repeating an optimizer / Polyak launch is harmless.
    `summary()` synchronises."""

    def __init__(self, repeat: int = 20):
        self.repeat = max(1, int(repeat))
        self.records: dict[str, list] = {}

    def __enter__(self):
        load().asac_set_launch_repeat(self.repeat)
        set_profiler(self)
        return self

    def __exit__(self, *exc):
        set_profiler(None)
        load().asac_set_launch_repeat(1)
        return False

    def bracket(self, name, fn, *a, **k):
        global _last_work
        if torch.cuda.is_current_stream_capturing():
            return fn(*a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        _last_work = None
        e0.record()
        out = fn(*a, **k)          # the library issues each launch `repeat` times (asac_set_launch_repeat)
        e1.record()
        self.records.setdefault(name, []).append((e0, e1, _last_work))
        return out

    def summary(self) -> dict:
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.records.items():
            us = [1e3 * a.elapsed_time(b) / self.repeat for a, b, _ in evs]
            # a bracket also spans the host's time to issue the first launch when the device had run dry
            # (allocator hiccups): the median over calls is the robust per-launch figure, the mean is kept
            med = sorted(us)[len(us) // 2]
            kept = [t for t in us if t <= 3.0 * med]       # (host-stall outliers: one 4 ms bracket in 50 doubles a mean)
            out[name] = {'calls': len(us), 'avg_us': sum(kept) / len(kept), 'avg_us_raw': sum(us) / len(us),
                         'min_us': min(us), 'med_us': med}
            pairs = [(t, ev[2]) for t, ev in zip(us, evs) if ev[2] is not None and t <= 3.0 * med]
            if pairs:   # wrappers that know their per-launch work (flops) report it: achieved = sum / sum over
                        # the calls that are not host-stall outliers (launch sizes differ, so no plain median)
                out[name]['flops_per_launch'] = sum(w for _, w in pairs) / len(pairs)
                out[name]['tflops'] = sum(w for _, w in pairs) / (sum(t for t, _ in pairs) * 1e-6) / 1e12
        return out


_profiler: LaunchProfiler | None = None
_last_work = None    # per-launch algorithmic work reported by a wrapper to the active profiler


def set_profiler(p: 'LaunchProfiler | None') -> None:
    global _profiler
    _profiler = p


def _profiled(fn, name=None):
    name = name or 'asac_' + fn.__name__

    def wrapper(*a, **k):
        if _profiler is None:
            return fn(*a, **k)
        return _profiler.bracket(name, fn, *a, **k)
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


# ------------------------------------------------------------------------------------------------
# thin typed wrappers (tensor in, launch on torch's current stream)
# ------------------------------------------------------------------------------------------------
@_profiled
def sumtree_sample(tree, capacity, batch, u, slot_ids, beta_state, beta_increment, leaf_out, p_out,
                   ids_out, is_weights_out, min_p_out):
    assert tree.dtype == torch.float32 and u.dtype == torch.float64 and slot_ids.dtype == torch.int64
    assert leaf_out.dtype == torch.int32 and ids_out.dtype == torch.int64 and min_p_out.numel() >= 2
    _check(load().asac_sumtree_sample(_p(tree), capacity, batch, _p(u), _p(slot_ids), _p(beta_state),
                                      float(beta_increment), _p(leaf_out), _p(p_out), _p(ids_out),
                                      _p(is_weights_out), _p(min_p_out), _stream()), 'asac_sumtree_sample')


@_profiled
def sumtree_descend(tree, capacity, values, slot_ids, leaf_out, p_out, ids_out):
    """leaf / priority / id for explicit f64 `values` (the descent of `sumtree_sample` alone)"""
    assert values.dtype == torch.float64 and leaf_out.dtype == torch.int32 and ids_out.dtype == torch.int64
    _check(load().asac_sumtree_descend(_p(tree), capacity, values.numel(), _p(values), _p(slot_ids), _p(leaf_out),
                                       _p(p_out), _p(ids_out), _stream()), 'asac_sumtree_descend')


@_profiled
def per_is_weights(p, batch, total, min_ratio, beta_state, beta_increment, w_out):
    _check(load().asac_per_is_weights(_p(p), batch, _p(total), _p(min_ratio), _p(beta_state),
                                      float(beta_increment), _p(w_out), _stream()), 'asac_per_is_weights')


@_profiled
def sumtree_update(tree, capacity, ids, slot_ids, td_error, alpha, td_min, td_max, mode, winner, nan_flag, sidecars=None):
    k = ids.numel()
    assert ids.dtype == torch.int64 and td_error.dtype == torch.float32 and td_error.numel() == k
    assert winner.dtype == torch.int32 and winner.numel() >= capacity + (2 * k if k > 1024 else 0)
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_sumtree_update_sc(_p(tree), capacity, k, _p(ids), _p(slot_ids), _p(td_error),
                                         alpha, td_min, td_max, mode, _p(winner), _p(nan_flag), sc, n_sc, _stream()),
           'asac_sumtree_update')


@_profiled
def per_add(tree, capacity, first_id, count, ignore_size, max_p_dev, max_p_host, slot_ids):
    _check(load().asac_per_add(_p(tree), capacity, int(first_id), int(count), int(ignore_size),
                               _p(max_p_dev), float(max_p_host), _p(slot_ids), _stream()), 'asac_per_add')


@_profiled
def sumtree_leaf_max(tree, capacity, out):
    _check(load().asac_sumtree_leaf_max(_p(tree), capacity, _p(out), _stream()), 'asac_sumtree_leaf_max')


def sumtree_check(tree, capacity, out):
    _check(load().asac_sumtree_check(_p(tree), capacity, _p(out), _stream()), 'asac_sumtree_check')


def sumtree_plan_top(shard_roots, batch, u, owner_out, value_out, total_out):
    assert shard_roots.dtype == torch.float32 and u.dtype == torch.float64 and owner_out.dtype == torch.int32
    assert value_out.dtype == torch.float64 and u.numel() >= batch
    _check(load().asac_sumtree_plan_top(_p(shard_roots), shard_roots.numel(), batch, _p(u), _p(owner_out), _p(value_out),
                                        _p(total_out), _stream()), 'asac_sumtree_plan_top')


def sumtree_descend_owned(tree, capacity, values, owner, rank, slot_ids, leaf_out, p_out, ids_out):
    assert values.dtype == torch.float64 and owner.dtype == torch.int32 and ids_out.dtype == torch.int64
    _check(load().asac_sumtree_descend_owned(_p(tree), capacity, values.numel(), _p(values), _p(owner), int(rank),
                                             _p(slot_ids), _p(leaf_out), _p(p_out), _p(ids_out), _stream()),
           'asac_sumtree_descend_owned')


def per_is_weights_slice(p_all, first, count, total, beta_state, beta_increment, w_out):
    _check(load().asac_per_is_weights_slice(_p(p_all), p_all.numel(), first, count, _p(total), _p(beta_state),
                                            float(beta_increment), _p(w_out), _stream()), 'asac_per_is_weights_slice')


def gelu_eval(z, value, deriv):
    _check(load().asac_gelu_eval(_p(z), _p(value), _p(deriv), z.numel(), _stream()), 'asac_gelu_eval')


@_profiled
def window_gather_pad(keys, ids, batch, prev_n, post_n, capacity, index_ring):
    """keys: ctypes array of GatherKey (build once with `make_gather_keys`)."""
    _check(load().asac_window_gather_pad(keys, len(keys), _p(ids), batch, prev_n, post_n, capacity,
                                         _p(index_ring), _stream()), 'asac_window_gather_pad')


def sidecar_window_gather(keys, ids, batch, prev_n, post_n, capacity, index_ring) -> Sidecar:
    """`window_gather_pad` as a sidecar job (hosted by `policy_sample_q_forward`): the launch description goes to device
    memory once (a blocking copy: call at build time, not inside a capture); the job keeps it alive through `_keep`."""
    import torch
    plan = torch.empty(int(load().asac_window_gather_plan_bytes()), dtype=torch.uint8, device=ids.device)
    blocks = C.c_int(0)
    _check(load().asac_window_gather_plan(keys, len(keys), _p(ids), batch, prev_n, post_n, capacity, _p(index_ring), _p(plan),
                                          C.byref(blocks)), 'asac_window_gather_plan')
    sc = Sidecar(kind=SIDECAR_WINDOW_GATHER, gather_plan=_p(plan), gather_blocks=blocks.value)
    sc._keep = (plan, keys, ids, index_ring)
    return sc


def sidecar_window_gather_w(keys, ids, batch, prev_n, post_n, capacity, index_ring, p, tree, beta_state, beta_increment,
                            is_weights_out, min_p_out) -> Sidecar:
    """`window_gather_pad_w` as a sidecar job (hosted by `policy_sample_q_forward` with ring-addressed rows): the gather and,
    as one more workgroup, the IS weights of the batch `step_prologue_sample_partial` drew.  Build time, as
    `sidecar_window_gather`."""
    import torch
    plan = torch.empty(int(load().asac_window_gather_plan_bytes()), dtype=torch.uint8, device=ids.device)
    blocks = C.c_int(0)
    _check(load().asac_window_gather_plan_w(keys, len(keys), _p(ids), batch, prev_n, post_n, capacity, _p(index_ring), _p(p),
                                            _p(tree), _p(beta_state), float(beta_increment), _p(is_weights_out),
                                            _p(min_p_out), _p(plan), C.byref(blocks)), 'asac_window_gather_plan_w')
    sc = Sidecar(kind=SIDECAR_WINDOW_GATHER_W, gather_plan=_p(plan), gather_blocks=blocks.value)
    sc._keep = (plan, keys, ids, index_ring, p, tree, beta_state, is_weights_out, min_p_out)
    return sc


@_profiled
def gather_rows(keys, ids, capacity):
    """dst_key[r] = ring_key[ids[r] % capacity] for every key of `keys` (all PAD_KEEP) in one launch"""
    _check(load().asac_gather_rows(keys, len(keys), _p(ids), ids.numel(), capacity, _stream()), 'asac_gather_rows')


def make_row_moves(specs):
    """specs: list of dicts(src, dst, row_bytes, src_mode, dst_mode, src_stride0/1, dst_stride0/1 (bytes),
    src_row_offset=0, pad_word=0); src / dst are tensors (their data_ptr is taken; keep them alive)."""
    assert 0 < len(specs) <= MAX_GATHER_KEYS
    arr = (RowMove * len(specs))()
    for k, s in zip(arr, specs):
        k.src, k.dst = s['src'].data_ptr(), s['dst'].data_ptr()
        k.row_bytes = int(s['row_bytes'])
        k.src_mode, k.dst_mode = int(s['src_mode']), int(s['dst_mode'])
        k.src_stride0, k.src_stride1 = int(s.get('src_stride0', 0)), int(s.get('src_stride1', 0))
        k.dst_stride0, k.dst_stride1 = int(s.get('dst_stride0', 0)), int(s.get('dst_stride1', 0))
        k.src_row_offset = int(s.get('src_row_offset', 0))
        k.pad_word = int(s.get('pad_word', 0)) & 0xffffffff
    return arr


@_profiled
def rows_move(keys, slot, src_row, dst_row, n_items):
    """one launch: every key of `keys` (ctypes array from `make_row_moves`) moves `n_items` rows"""
    _check(load().asac_rows_move(keys, len(keys), _p(slot), _p(src_row), _p(dst_row), int(n_items), _stream()),
           'asac_rows_move')


def make_batch_put_keys(specs):
    """specs: list of dicts(src (tensor or None), src_stride (bytes), pool, row_bytes, pad_mode, pad_word=0,
    pad_row=None); keep the tensors alive while the array is in use."""
    assert 0 < len(specs) <= MAX_GATHER_KEYS
    arr = (BatchPutKey * len(specs))()
    for k, s in zip(arr, specs):
        k.src = s['src'].data_ptr() if s.get('src') is not None else None
        k.pool = s['pool'].data_ptr()
        k.pad_row = s['pad_row'].data_ptr() if s.get('pad_row') is not None else None
        k.src_stride = int(s.get('src_stride', 0))
        k.row_bytes = int(s['row_bytes'])
        k.pad_mode = int(s['pad_mode'])
        k.pad_word = int(s.get('pad_word', 0)) & 0xffffffff
    return arr


@_profiled
def batch_put(keys, ep_len, burn_in, L, win_start, win_slot, n_windows, pool_slots, queue_rows, queue_slots,
              n_queue_rows, batch, queue, head, new_head):
    """one launch: an episode's surviving windows -> their pool slots, the new queue rows, the head (csrc/batch.hip)"""
    assert queue.dtype == torch.int32 and head.dtype == torch.int32 and queue.is_contiguous()
    _check(load().asac_batch_put(keys, len(keys), int(ep_len), int(burn_in), int(L), _p(win_start), _p(win_slot),
                                 int(n_windows), int(pool_slots), _p(queue_rows), _p(queue_slots), int(n_queue_rows),
                                 int(batch), _p(queue), queue.shape[0], _p(head), int(new_head), _stream()),
           'asac_batch_put')


def make_batch_gather_keys(specs):
    """specs: list of dicts(pool, dst, row_bytes, convert=CVT_NONE)"""
    assert 0 < len(specs) <= MAX_GATHER_KEYS
    arr = (BatchGatherKey * len(specs))()
    for k, s in zip(arr, specs):
        k.pool, k.dst = s['pool'].data_ptr(), s['dst'].data_ptr()
        k.row_bytes = int(s['row_bytes'])
        k.convert = int(s.get('convert', CVT_NONE))
    return arr


@_profiled
def batch_pop_gather(keys, queue, head, batch, L, pool_slots):
    """one launch: the windows of queue[head % rows] -> the keys' dense [batch, L] destinations (csrc/batch.hip)"""
    assert queue.dtype == torch.int32 and head.dtype == torch.int32 and queue.is_contiguous()
    _check(load().asac_batch_pop_gather(keys, len(keys), _p(queue), _p(head), queue.shape[0], int(batch), int(L),
                                        int(pool_slots), _stream()), 'asac_batch_pop_gather')


def make_gather_keys(specs):
    """specs: list of dicts(src, dst, row_bytes, pad_mode, pad_word=0, pad_row=None, convert=0)."""
    assert 0 < len(specs) <= MAX_GATHER_KEYS
    arr = (GatherKey * len(specs))()
    for k, s in zip(arr, specs):
        k.src = s['src'].data_ptr() if s.get('src') is not None else None
        k.dst = s['dst'].data_ptr()
        k.pad_row = s['pad_row'].data_ptr() if s.get('pad_row') is not None else None
        k.row_bytes = int(s.get('row_bytes', 1))
        k.pad_mode = int(s['pad_mode'])
        k.pad_word = int(s.get('pad_word', 0)) & 0xffffffff
        k.convert = int(s.get('convert', 0))
        k.dst_row_pitch = int(s.get('dst_row_pitch', 0))
        k.derive = int(s.get('derive', 0))
    return arr


@_profiled
def scatter_rows_if_id_match(ring, row_bytes, capacity, ids, batch, first_off, count, slot_ids,
                             padding_mask, mask_sample_stride, rows, rows_sample_stride_bytes,
                             rows_row_stride_bytes, winner):
    _check(load().asac_scatter_rows_if_id_match(
        _p(ring), row_bytes, capacity, _p(ids), batch, first_off, count, _p(slot_ids), _p(padding_mask),
        mask_sample_stride, _p(rows), rows_sample_stride_bytes, rows_row_stride_bytes, _p(winner),
        _stream()), 'asac_scatter_rows_if_id_match')


def _ls_rows(loc, scale):
    """loc / scale [..., A] with a dense inner dim and one uniform row stride (dense [rows, A] tensors
    or the two column halves of a dense [rows, 2A] tensor) -> (rows, A, row_stride)."""
    A = loc.shape[-1]
    assert loc.shape == scale.shape and loc.stride() == scale.stride()
    assert loc.stride(-1) == 1 or A == 1
    rs = loc.stride(-2) if loc.dim() >= 2 else A
    for d in range(loc.dim() - 2):            # leading dims must collapse onto the row stride
        assert loc.stride(d) == loc.stride(d + 1) * loc.shape[d + 1], 'loc/scale rows are not uniformly strided'
    return loc.numel() // A, A, rs


@_profiled
def window_aux(bn_indexes, bn_padding_masks, bn_actions, index_x, pad_x, pre_action):
    """bn_* = the L-1 leading rows of the sampled window ([B, L-1(, A)] views) -> index_x i32 [B, L],
    pad_x bool [B, L] (dense), pre_action f32 [B, L, A] (dense, or a column block of a wider [B, L, *] tensor)."""
    B, Lm1 = bn_indexes.shape
    A = bn_actions.shape[-1]
    assert bn_indexes.dtype == torch.int32 and bn_indexes.stride(1) == 1 and bn_padding_masks.stride(1) == 1
    assert bn_padding_masks.element_size() == 1 and bn_actions.stride(2) == 1 and bn_actions.dtype == torch.float32
    assert index_x.is_contiguous() and pad_x.is_contiguous()
    assert pre_action.shape == (B, Lm1 + 1, A) and pre_action.stride(2) == 1 and pre_action.dtype == torch.float32
    assert pre_action.stride(0) == (Lm1 + 1) * pre_action.stride(1)
    _check(load().asac_window_aux(_p(bn_indexes), bn_indexes.stride(0), _p(bn_padding_masks), bn_padding_masks.stride(0),
                                  _p(bn_actions), bn_actions.stride(0), bn_actions.stride(1), B, Lm1 + 1, A,
                                  _p(index_x), _p(pad_x), _p(pre_action), pre_action.stride(1), _stream()),
           'asac_window_aux')


@_profiled
def squash_sample_fwd(loc, scale, eps, a_out, logp_out, x_out=None, action=None, action_offset=0,
                      prob_out=None, prob_offset=0):
    """eps / a_out dense [rows, A]; with `action` ([S, T, >=off+A] view) also writes the stored-action
    probabilities into prob_out ([S, T, >=off+A] view) in the same launch."""
    rows, A, ls = _ls_rows(loc, scale)
    assert eps.is_contiguous() and a_out.is_contiguous()
    T = asb = ast = psb = pst = 0
    if action is not None:
        assert action.dim() == 3 and prob_out.dim() == 3 and action.stride(-1) == 1 and prob_out.stride(-1) == 1
        assert action.shape[0] * action.shape[1] == rows
        T, asb, ast, psb, pst = action.shape[1], action.stride(0), action.stride(1), prob_out.stride(0), prob_out.stride(1)
    _check(load().asac_squash_sample_fwd(_p(loc), _p(scale), ls, _p(eps), rows, A, _p(a_out), _p(logp_out), _p(x_out),
                                         _p(action), T, asb, ast, action_offset, _p(prob_out), psb, pst, prob_offset,
                                         _stream()), 'asac_squash_sample_fwd')


@_profiled
def squash_sample_bwd(loc, scale, eps, grad_a, grad_logp, grad_loc, grad_scale, log_alpha=None):
    """grad_a: dense [rows, A] or [members, rows, A] (one gradient per ensemble member that consumed the
    action: summed in member order by the kernel).  grad_logp None + log_alpha: dL/dlogp = exp(log_alpha)/rows."""
    rows, A, ls = _ls_rows(loc, scale)
    _, _, gs = _ls_rows(grad_loc, grad_scale)
    members, mstride = 1, 0
    if grad_a is not None:
        assert grad_a.is_contiguous() and grad_a.numel() % (rows * A) == 0
        members, mstride = grad_a.numel() // (rows * A), rows * A
    _check(load().asac_squash_sample_bwd(_p(loc), _p(scale), ls, _p(eps), _p(grad_a), members, mstride,
                                         _p(grad_logp), _p(log_alpha), rows, A, _p(grad_loc), _p(grad_scale), gs,
                                         _stream()), 'asac_squash_sample_bwd')


def _stored_action(s: SquashJob, rows, action, action_offset, prob_out, prob_offset):
    """the stored-action fields of `s`: `action` / `prob_out` are [samples, T, >= offset + A] views (dense last dim) of
    the job's `rows` = samples * T rows; sets s.T"""
    assert action.dim() == 3 and prob_out.dim() == 3 and action.stride(-1) == 1 and prob_out.stride(-1) == 1
    assert action.shape[0] * action.shape[1] == rows and prob_out.shape[:2] == action.shape[:2]
    s.action, s.T = action.data_ptr(), action.shape[1]
    s.action_stride_b, s.action_stride_t, s.action_offset = action.stride(0), action.stride(1), action_offset
    s.prob_out, s.prob_stride_b, s.prob_stride_t, s.prob_offset = \
        prob_out.data_ptr(), prob_out.stride(0), prob_out.stride(1), prob_offset


def _second_sample(j, samples, A, eps2, t2, a2_out, logp2_out):
    """the second-sample fields of a `SampleEpilogue` / `PiQJob`: eps2 [samples, A] -> a2_out, logp2_out at position t2"""
    assert eps2.is_contiguous() and a2_out.is_contiguous() and eps2.numel() == samples * A
    j.eps2, j.t2, j.a2_out, j.logp2_out = eps2.data_ptr(), t2, a2_out.data_ptr(), logp2_out.data_ptr()


def squash_job(loc, scale, eps=None, a_out=None, logp_out=None, action=None, action_offset=0, prob_out=None,
               prob_offset=0) -> SquashJob:
    """One job of `squash_multi`: a sampling job (eps, a_out, logp_out; optionally also the stored-action
    probabilities) or, without eps, a probability-only job.  Tensor conventions as `squash_sample_fwd` /
    `squash_prob`.  The job holds raw pointers: keep the tensors alive until the launch."""
    rows, A, ls = _ls_rows(loc, scale)
    j = SquashJob()
    j.loc, j.scale, j.ls_row_stride, j.rows, j.A = loc.data_ptr(), scale.data_ptr(), ls, rows, A
    if eps is not None:
        assert eps.is_contiguous() and a_out.is_contiguous() and eps.numel() == rows * A
        j.eps, j.a_tanh_out, j.logp_out = eps.data_ptr(), a_out.data_ptr(), logp_out.data_ptr()
    if action is not None:
        _stored_action(j, rows, action, action_offset, prob_out, prob_offset)
    else:
        assert eps is not None, 'a job needs eps (sampling) or action (stored-action probabilities)'
    return j


def _sidecar_array(sidecars):
    sidecars = list(sidecars or ())
    assert len(sidecars) <= MAX_SIDECARS
    return ((Sidecar * len(sidecars))(*sidecars) if sidecars else None), len(sidecars)


def sidecar_alpha_adam(logp, target, slot, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, steps_done,
                       advance_counter=True) -> Sidecar:
    """`alpha_adam_step` as a sidecar of a hosting launch (keeps the tensors alive through `_keep`)"""
    sc = Sidecar(kind=SIDECAR_ALPHA_ADAM, logp=_p(logp), B=logp.numel(), target=float(target), slot=int(slot),
                 param=_p(param), grad=_p(grad), exp_avg=_p(exp_avg), exp_avg_sq=_p(exp_avg_sq), n=param.numel(),
                 lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps), steps_done=_p(steps_done),
                 advance_counter=int(bool(advance_counter)))
    sc._keep = (logp, param, grad, exp_avg, exp_avg_sq, steps_done)
    return sc


def sidecar_scatter(kind, ring, row_bytes, capacity, ids, batch, first_off, count, slot_ids, padding_mask,
                    mask_sample_stride, rows, rows_sample_stride_bytes, rows_row_stride_bytes, winner) -> Sidecar:
    """one pass (`SIDECAR_SCATTER_ELECT` / `SIDECAR_SCATTER_WRITE`) of `scatter_rows_if_id_match` as a sidecar"""
    sc = Sidecar(kind=kind, ring=_p(ring), row_bytes=row_bytes, capacity=capacity, ids=_p(ids), batch=batch,
                 first_off=first_off, count=count, slot_ids=_p(slot_ids), padding_mask=_p(padding_mask),
                 mask_sample_stride=mask_sample_stride, rows=_p(rows), rows_sample_stride_bytes=rows_sample_stride_bytes,
                 rows_row_stride_bytes=rows_row_stride_bytes, winner=_p(winner))
    sc._keep = (ring, ids, slot_ids, padding_mask, rows, winner)
    return sc


@_profiled
def squash_multi(jobs, sidecars=None):
    """Run 1..SQUASH_MAX_JOBS `squash_job`s in one launch (+ sidecar jobs as extra workgroups)."""
    assert 1 <= len(jobs) <= SQUASH_MAX_JOBS
    arr = (SquashJob * len(jobs))(*jobs)
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_squash_multi(arr, len(jobs), sc, n_sc, _stream()), 'asac_squash_multi')


@_profiled
def squash_prob(loc, scale, action, action_offset, prob_out, prob_offset):
    """loc/scale: [S, T, A] (uniform row stride); action / prob_out: [S, T, >=offset+A] views."""
    rows, A, ls = _ls_rows(loc, scale)
    S, T = action.shape[0], action.shape[1]
    assert S * T == rows and action.stride(-1) == 1 and prob_out.stride(-1) == 1 and prob_out.shape[:2] == (S, T)
    _check(load().asac_squash_prob(_p(loc), _p(scale), ls, _p(action), T, action.stride(0), action.stride(1),
                                   action_offset, rows, A, _p(prob_out), prob_out.stride(0),
                                   prob_out.stride(1), prob_offset, _stream()), 'asac_squash_prob')


@_profiled
def vtrace_return_min(args: VtraceArgs, sidecars=None, pending_alpha: 'Sidecar | None' = None):
    """`pending_alpha`: the temperature step's sidecar job when it has not run yet (it rides in a LATER launch): the
    return is evaluated with the temperature that job will write"""
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_vtrace_return_min_sc(C.byref(args), sc, n_sc,
                                            C.byref(pending_alpha) if pending_alpha is not None else None, _stream()),
           'asac_vtrace_return_min')


def td_update_ok(B: int, n: int) -> bool:
    """can `td_update` take a batch of B windows of n steps (one workgroup, its LDS)?"""
    return 0 < B <= 1024 and (((2 * B * ((n + 1) | 1) + 3) & ~3) + 2 * ((B + 63) & ~63) + 4) * 4 <= 128 * 1024


@_profiled
def td_update(args: VtraceArgs, tree, capacity, ids, slot_ids, alpha, td_min, td_max, winner, nan_flag, sidecars=None,
              alpha_step: 'Sidecar | None' = None):
    """the TD errors' return (args.q_online / td_error_out set) + the priority update of `ids` with them: one launch"""
    assert ids.dtype == torch.int64 and ids.numel() == args.B and winner.dtype == torch.int32
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_td_update(C.byref(args), _p(tree), capacity, _p(ids), _p(slot_ids), alpha, td_min, td_max,
                                 _p(winner), _p(nan_flag), sc, n_sc,
                                 C.byref(alpha_step) if alpha_step is not None else None, _stream()), 'asac_td_update')


@_profiled
def vtrace_return_direct(args: VtraceArgs, v_n, v_next, pi_prod, mu_prod):
    _check(load().asac_vtrace_return_direct(C.byref(args), _p(v_n), _p(v_next), _p(pi_prod), _p(mu_prod),
                                            _stream()), 'asac_vtrace_return_direct')


@_profiled
def q_loss_fwd_bwd(q, tq, y, w, clip_eps, loss_out, grad_q_out):
    E, B = q.shape[0], q.shape[1]
    _check(load().asac_q_loss_fwd_bwd(_p(q), _p(tq), _p(y), _p(w), E, B, float(clip_eps), _p(loss_out),
                                      _p(grad_q_out), _stream()), 'asac_q_loss_fwd_bwd')


def _rows_view(x):
    """(ptr, row_stride, member_stride) of an input given as [N, K] (shared by every ensemble
    member) or [E, N, K]; the inner dimension must be dense."""
    if x is None:
        return None, 0, 0
    assert x.stride(-1) == 1 or x.shape[-1] == 1
    if x.dim() == 2:
        return _p(x), x.stride(0), 0
    assert x.dim() == 3
    return _p(x), x.stride(1), x.stride(0)


def mlp_flops(desc, E, N, backward=False, param_grads=True) -> float:
    """Algorithmic FLOPs of one fused-MLP pass: 2*rows*in*out per Linear (x2 for dX, x2 for dW)."""
    k, mac = desc.in0 + desc.in1, 0
    for l in range(desc.n_blocks):
        mac += k * desc.width[l]
        k = desc.width[l]
    mac += k * (desc.head_cols[0] + desc.head_cols[1])
    passes = (1 + 1 + (1 if param_grads else 0)) if backward else 1    # recompute + dX (+ dW)
    return 2.0 * mac * N * E * passes


class WindowRows:
    """Marks a non-collapsible [samples, T, K] view (dense last dim) as the row source of a forward job:
    the kernel addresses rows as (sample, t) instead of the caller staging a contiguous copy."""

    def __init__(self, t: torch.Tensor):
        self.t = t
        self.shape = (t.shape[0] * t.shape[1], t.shape[2])


def mlp_job(desc, params, member_stride, E, x0, x1, N, out=None) -> MlpJob:
    """One pass of E networks (`desc`; parameter segments `member_stride` floats apart in `params`) over N rows: x0 / x1
    [N, K] (shared by every member) or [E, N, K], x1 None when in1 == 0; `out` [E, N, head columns] for the forward
    passes.  What the mlp_* wrappers below take first.  Raw pointers: keep the tensors and the descriptor alive until
    the launch."""
    j = MlpJob()
    j.desc, j.params, j.member_stride, j.E, j.N = C.pointer(desc), params.data_ptr(), member_stride, E, N
    if isinstance(x0, WindowRows):      # [samples, T, K] view shared by every member, read in place
        t = x0.t
        assert t.dim() == 3 and t.stride(2) == 1 and t.shape[0] * t.shape[1] == N
        p0, j.x0_row_stride, j.x0_member_stride = _p(t), t.stride(1), 0
        j.x0_window_T, j.x0_sample_stride = t.shape[1], t.stride(0)
    else:
        p0, j.x0_row_stride, j.x0_member_stride = _rows_view(x0)
    p1, j.x1_row_stride, j.x1_member_stride = _rows_view(x1)
    j.x0, j.x1 = p0.value if p0 is not None else None, p1.value if p1 is not None else None
    if out is not None:
        assert out.is_cuda and out.is_contiguous()
        j.out = out.data_ptr()
    return j


def _pass_flops(job: MlpJob, backward=False, param_grads=True) -> float:
    return mlp_flops(job.desc.contents, job.E, job.N, backward, param_grads)


@_profiled
def mlp_forward(job: MlpJob):
    global _last_work
    _last_work = _pass_flops(job)
    _check(load().asac_mlp_forward(C.byref(job), _stream()), 'asac_mlp_forward')


@_profiled
def mlp_forward_multi(jobs, sidecars=None):
    global _last_work
    _last_work = sum(mlp_flops(j.desc.contents, j.E, j.N) for j in jobs)
    assert 1 <= len(jobs) <= MLP_MAX_JOBS
    arr = (MlpJob * len(jobs))(*jobs)
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_mlp_forward_multi(arr, len(jobs), sc, n_sc, _stream()), 'asac_mlp_forward_multi')


def sample_epilogue(job: MlpJob | None = None, eps=None, a_out=None, logp_out=None, T=0, action=None, action_offset=0,
                    prob_out=None, prob_offset=0, eps2=None, t2=0, a2_out=None, logp2_out=None) -> SampleEpilogue:
    """The epilogue of a policy job of `mlp_forward_multi_sampled` (`job` from `mlp_job`; None / no arguments: the job has
    none): the main sample over every row (eps -> a_out, logp_out), the stored actions' probabilities ([samples, T, >= A]
    `action` -> `prob_out`), a second sample at window position `t2` of every sample.  Raw pointers: keep the tensors alive."""
    e = SampleEpilogue()
    if job is None:
        return e
    A, N = job.desc.contents.head_cols[0], job.N
    s = e.sample
    s.rows, s.A, s.T = N, A, T
    if eps is not None:
        assert eps.is_contiguous() and a_out.is_contiguous() and eps.numel() == N * A and logp_out.numel() == N
        assert logp_out.is_contiguous()
        s.eps, s.a_tanh_out, s.logp_out = eps.data_ptr(), a_out.data_ptr(), logp_out.data_ptr()
    if action is not None:
        _stored_action(s, N, action, action_offset, prob_out, prob_offset)
        assert T in (0, s.T)
    if eps2 is not None:
        assert s.T > 0 and logp2_out.is_contiguous() and logp2_out.numel() == N // s.T
        _second_sample(e, N // s.T, A, eps2, t2, a2_out, logp2_out)
    return e


def mlp_forward_multi_sampled_ok(jobs, epilogues) -> bool:
    assert len(jobs) == len(epilogues) and 1 <= len(jobs) <= MLP_MAX_JOBS
    return bool(load().asac_mlp_forward_multi_sampled_ok((MlpJob * len(jobs))(*jobs), len(jobs),
                                                         (SampleEpilogue * len(jobs))(*epilogues)))


@_profiled
def mlp_forward_multi_sampled(jobs, epilogues, sidecars=None):
    """`mlp_forward_multi` whose policy jobs sample from / score stored actions under the rows they form (`sample_epilogue`):
    the policy forward and `squash_multi` as one launch"""
    global _last_work
    _last_work = sum(mlp_flops(j.desc.contents, j.E, j.N) for j in jobs)
    assert len(jobs) == len(epilogues) and 1 <= len(jobs) <= MLP_MAX_JOBS
    arr = (MlpJob * len(jobs))(*jobs)
    epi = (SampleEpilogue * len(jobs))(*epilogues)
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_mlp_forward_multi_sampled(arr, len(jobs), epi, sc, n_sc, _stream()), 'asac_mlp_forward_multi_sampled')


def pi_q_job(pi_job: MlpJob, q_job: MlpJob, eps, a_out, logp_out, T, action=None, action_offset=0, prob_out=None,
             prob_offset=0, eps2=None, t2=0, a2_out=None, logp2_out=None) -> PiQJob:
    """The fused policy -> sample -> critics forward (`policy_sample_q_forward`): `pi_job` / `q_job` from `mlp_job`
    on the same rows ([samples, T] flattened); the main sample (eps -> a_out, logp_out), optionally the stored
    actions' probabilities and a second sample at window position `t2`.  Raw pointers: keep the tensors alive."""
    j = PiQJob()
    j.pi, j.q = pi_job, q_job
    A = pi_job.desc.contents.head_cols[0]
    N = pi_job.N
    assert eps.is_contiguous() and a_out.is_contiguous() and eps.numel() == N * A and logp_out.numel() == N
    s = j.sample
    s.eps, s.a_tanh_out, s.logp_out, s.rows, s.A, s.T = eps.data_ptr(), a_out.data_ptr(), logp_out.data_ptr(), N, A, T
    if action is not None:
        assert action.dim() == 3 and action.shape[1] == T
        _stored_action(s, N, action, action_offset, prob_out, prob_offset)
    if eps2 is not None:
        _second_sample(j, N // T, A, eps2, t2, a2_out, logp2_out)
    return j


def ring_key(spec) -> RingKey | None:
    """a gather key spec (`make_gather_keys`) as a key of `pi_q_ring_rows`; None: not a plain float32 key (converted,
    derived, a mask, rows that are no whole words)"""
    src = spec.get('src')
    if (src is None or src.dtype != torch.float32 or spec.get('convert', CVT_NONE) != CVT_NONE or spec.get('derive', 0)
            or spec['pad_mode'] not in (PAD_KEEP, PAD_WORD, PAD_ROW) or int(spec['row_bytes']) % 4):
        return None
    k = RingKey()
    k.src, k.row_bytes, k.pad_mode = src.data_ptr(), int(spec['row_bytes']), int(spec['pad_mode'])
    k.pad_word = int(spec.get('pad_word', 0)) & 0xffffffff
    if spec['pad_mode'] == PAD_ROW:
        k.pad_row = spec['pad_row'].data_ptr()
    return k


def pi_q_ring_rows(job: PiQJob, ids, index_ring, capacity, prev_n, L, j0, x0_key: RingKey, action_key: RingKey | None = None,
                   x_j0=-1, x_action_offset=0) -> PiQJob:
    """-> a copy of `job` (from `pi_q_job`) whose rows — the policy's / critics' x0 and, with `action_key`, the stored
    actions — are read where they lie in the replay ring: row r of the job is window row j0 + r % T of sample r // T, as
    `window_gather_pad` would have delivered it.  `x_j0 >= 0`: the first extra job of the launch reads (x0 | stored
    action) of window row x_j0 of every sample the same way.  Raw pointers: keep the tensors alive."""
    assert ids.dtype == torch.int64 and index_ring.dtype == torch.int32
    out = PiQJob()
    C.memmove(C.byref(out), C.byref(job), C.sizeof(PiQJob))
    r = out.ring
    r.ids, r.index_ring = ids.data_ptr(), index_ring.data_ptr()
    r.capacity, r.prev_n, r.L, r.j0, r.x_j0, r.x_action_offset = capacity, prev_n, L, j0, x_j0, x_action_offset
    r.x0 = x0_key
    if action_key is not None:
        r.action = action_key
    return out


def policy_sample_q_forward_ok(job: PiQJob, extra_jobs=None) -> bool:
    """the launch qualifies; with `extra_jobs` also they, and what `job`'s ring description says about the first of them:
    exactly what `policy_sample_q_forward(job, extra_jobs)` accepts"""
    if extra_jobs is None:
        return bool(load().asac_policy_sample_q_forward_ok(C.byref(job)))
    extra_jobs = list(extra_jobs)
    arr = (MlpJob * len(extra_jobs))(*extra_jobs) if extra_jobs else None
    return bool(load().asac_policy_sample_q_forward_jobs_ok(C.byref(job), arr, len(extra_jobs)))


@_profiled
def policy_sample_q_forward(job: PiQJob, extra_jobs=(), sidecars=None):
    global _last_work
    # algorithmic work: the policy once (the E workgroups of a tile repeat it side by side), every critic once
    _last_work = (mlp_flops(job.pi.desc.contents, 1, job.pi.N) + mlp_flops(job.q.desc.contents, job.q.E, job.q.N)
                  + sum(mlp_flops(j.desc.contents, j.E, j.N) for j in extra_jobs))
    extra_jobs = list(extra_jobs)
    assert len(extra_jobs) <= MLP_MAX_JOBS
    arr = (MlpJob * len(extra_jobs))(*extra_jobs) if extra_jobs else None
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_policy_sample_q_forward(C.byref(job), arr, len(extra_jobs), sc, n_sc, _stream()),
           'asac_policy_sample_q_forward')


def critic_forward_save_floats(N: int, E: int) -> int:
    """floats of the buffer the critic-forward rider saves an [E][N] forward in (`policy_sample_q_forward_saving`)"""
    return int(load().asac_critic_forward_save_floats(int(N), int(E)))


def policy_sample_q_forward_saving_ok(job: PiQJob, extra_jobs, sidecars, online_job: MlpJob, save) -> bool:
    """may `policy_sample_q_forward(job, extra_jobs, sidecars)` also carry the online critics' forward `online_job` on the
    rows of `extra_jobs[0]` (saved in `save`) as a rider?  (Among the conditions: the workgroups in front of the sidecars' —
    the fused job's, the extra jobs', the rider's — fit the device's CUs.)"""
    extra_jobs = list(extra_jobs)
    arr = (MlpJob * len(extra_jobs))(*extra_jobs) if extra_jobs else None
    sc, n_sc = _sidecar_array(sidecars)
    return bool(load().asac_policy_sample_q_forward_saving_ok(C.byref(job), arr, len(extra_jobs), sc, n_sc,
                                                              C.byref(online_job) if online_job is not None else None,
                                                              _p(save)))


def _policy_sample_q_forward_saving(job: PiQJob, extra_jobs, sidecars, online_job: MlpJob, save):
    """`policy_sample_q_forward` with the online critics' forward `online_job` (on the rows of `extra_jobs[0]`) riding on
    further workgroups of the launch: `save` (float32, `critic_forward_save_floats(N, E)`) receives what
    `mlp_backward_qloss_return_loaded` reads.  The launch's own outputs are `policy_sample_q_forward`'s, bit for bit."""
    global _last_work
    _last_work = (mlp_flops(job.pi.desc.contents, 1, job.pi.N) + mlp_flops(job.q.desc.contents, job.q.E, job.q.N)
                  + sum(mlp_flops(j.desc.contents, j.E, j.N) for j in extra_jobs) + _pass_flops(online_job))
    extra_jobs = list(extra_jobs)
    assert 1 <= len(extra_jobs) <= MLP_MAX_JOBS
    assert save.dtype == torch.float32 and save.is_contiguous()
    assert save.numel() >= critic_forward_save_floats(online_job.N, online_job.E)
    arr = (MlpJob * len(extra_jobs))(*extra_jobs)
    sc, n_sc = _sidecar_array(sidecars)
    _check(load().asac_policy_sample_q_forward_saving(C.byref(job), arr, len(extra_jobs), sc, n_sc, C.byref(online_job),
                                                      _p(save), _stream()), 'asac_policy_sample_q_forward_saving')


# (one launch of the step under the name it has without the rider: the kernel tables key on it)
policy_sample_q_forward_saving = _profiled(_policy_sample_q_forward_saving, 'asac_policy_sample_q_forward')


def mlp_backward_workspace(member_stride, E, N) -> int:
    return int(load().asac_mlp_backward_workspace(member_stride, E, N))


def mlp_backward_tiles(N, E) -> int:
    """row tiles (= per-tile partial slabs) the backward of an [E][N] pass uses"""
    return int(load().asac_mlp_backward_tiles(N, E))


MLP_REDUCE_OVERWRITE, MLP_REDUCE_ACCUMULATE, MLP_REDUCE_DEFER = _defined(
    'MLP_REDUCE_OVERWRITE', 'MLP_REDUCE_ACCUMULATE', 'MLP_REDUCE_DEFER')


def mlp_param_extent(desc) -> int:
    return int(load().asac_mlp_param_extent(C.byref(desc)))


@_profiled
def mlp_backward_qloss(job: MlpJob, target_q, y, weights, clip_eps, loss_out, grad_params, workspace, reduce_mode,
                       grad_x0=None):
    """Q loss + backward of the stock Q ensemble in one launch (parameter gradients; with `grad_x0` [E, N, in0] also
    the members' gradients w.r.t. the state input)."""
    global _last_work
    _last_work = _pass_flops(job, backward=True)
    E, N = job.E, job.N
    assert target_q.is_contiguous() and target_q.numel() == E * N and y.is_contiguous() and y.numel() == N
    assert grad_x0 is None or (grad_x0.is_contiguous() and grad_x0.numel() == E * N * job.desc.contents.in0)
    _check(load().asac_mlp_backward_qloss(C.byref(job), _p(target_q), _p(y), _p(weights), float(clip_eps), _p(loss_out),
                                          _p(grad_x0), _p(grad_params), _p(workspace), int(reduce_mode), _stream()),
           'asac_mlp_backward_qloss')


def mlp_backward_qloss_return_ok(job: MlpJob, ret: VtraceArgs) -> bool:
    """(reads the job's network, E and N only: its inputs may be unset)"""
    return bool(load().asac_mlp_backward_qloss_return_ok(C.byref(job), C.byref(ret)))


@_profiled
def mlp_backward_qloss_return(job: MlpJob, target_q, ret: VtraceArgs, weights, clip_eps, loss_out, grad_params, workspace,
                              reduce_mode, grad_x0=None):
    """`mlp_backward_qloss` whose workgroups form the return target `ret` describes themselves (no return launch)"""
    global _last_work
    _last_work = _pass_flops(job, backward=True)
    E, N = job.E, job.N
    assert target_q.is_contiguous() and target_q.numel() == E * N
    assert grad_x0 is None or (grad_x0.is_contiguous() and grad_x0.numel() == E * N * job.desc.contents.in0)
    _check(load().asac_mlp_backward_qloss_return(C.byref(job), _p(target_q), C.byref(ret), _p(weights), float(clip_eps),
                                                 _p(loss_out), _p(grad_x0), _p(grad_params), _p(workspace), int(reduce_mode),
                                                 _stream()), 'asac_mlp_backward_qloss_return')


def policy_forward_save_floats(N: int) -> int:
    """floats of the buffer the policy-forward rider saves N rows' forward in (`mlp_backward_qloss_return_rider`)"""
    return int(load().asac_policy_forward_save_floats(int(N)))


def mlp_backward_qloss_return_rider_ok(job: MlpJob, ret: VtraceArgs, pi_job, save) -> bool:
    """may the Q-loss backward launch carry the policy's forward on `pi_job`'s rows (saved in `save`) as a rider?"""
    return bool(load().asac_mlp_backward_qloss_return_rider_ok(C.byref(job), C.byref(ret),
                                                               C.byref(pi_job) if pi_job is not None else None, _p(save)))


def _mlp_backward_qloss_return_rider(job: MlpJob, target_q, ret: VtraceArgs, weights, clip_eps, loss_out, grad_params,
                                     workspace, reduce_mode, pi_job: MlpJob, save, grad_x0=None):
    """`mlp_backward_qloss_return` with the policy's forward on `pi_job`'s rows riding on further workgroups of the launch:
    `save` (float32, `policy_forward_save_floats(pi_job.N)`) receives what `policy_step_fused_loaded` reads.  The Q job's
    outputs are `mlp_backward_qloss_return`'s, bit for bit."""
    global _last_work
    _last_work = _pass_flops(job, backward=True) + _pass_flops(pi_job)
    E, N = job.E, job.N
    assert target_q.is_contiguous() and target_q.numel() == E * N
    assert grad_x0 is None or (grad_x0.is_contiguous() and grad_x0.numel() == E * N * job.desc.contents.in0)
    assert save.dtype == torch.float32 and save.is_contiguous() and save.numel() >= policy_forward_save_floats(pi_job.N)
    _check(load().asac_mlp_backward_qloss_return_rider(C.byref(job), _p(target_q), C.byref(ret), _p(weights),
                                                       float(clip_eps), _p(loss_out), _p(grad_x0), _p(grad_params),
                                                       _p(workspace), int(reduce_mode), C.byref(pi_job), _p(save),
                                                       _stream()), 'asac_mlp_backward_qloss_return_rider')


# (one launch of the step under the name it has without the rider: the kernel tables key on it)
mlp_backward_qloss_return_rider = _profiled(_mlp_backward_qloss_return_rider, 'asac_mlp_backward_qloss_return')


def mlp_backward_qloss_return_loaded_ok(job: MlpJob, ret: VtraceArgs, saved, pi_job=None, save=None) -> bool:
    """may the Q-loss backward load the critics' forward from `saved` (`policy_sample_q_forward_saving`)?  With `pi_job`:
    ... while carrying the policy-forward rider (`mlp_backward_qloss_return_rider_ok`)"""
    if pi_job is None:
        return bool(load().asac_mlp_backward_qloss_return_loaded_ok(C.byref(job), C.byref(ret), _p(saved)))
    return bool(load().asac_mlp_backward_qloss_return_rider_loaded_ok(C.byref(job), C.byref(ret), C.byref(pi_job), _p(save),
                                                                      _p(saved)))


def _mlp_backward_qloss_return_loaded(job: MlpJob, target_q, ret: VtraceArgs, weights, clip_eps, loss_out, grad_params,
                                      workspace, reduce_mode, saved, pi_job=None, save=None):
    """`mlp_backward_qloss_return` (with `pi_job` / `save`: `mlp_backward_qloss_return_rider`) LOADING the critics' forward
    on the job's rows from `saved` instead of recomputing it: same slabs, loss and y, bit for bit.  No input gradient."""
    global _last_work
    _last_work = _pass_flops(job, backward=True) + (_pass_flops(pi_job) if pi_job is not None else 0)
    E, N = job.E, job.N
    assert target_q.is_contiguous() and target_q.numel() == E * N
    assert saved.dtype == torch.float32 and saved.is_contiguous() and saved.numel() >= critic_forward_save_floats(N, E)
    if pi_job is None:
        _check(load().asac_mlp_backward_qloss_return_loaded(C.byref(job), _p(target_q), C.byref(ret), _p(weights),
                                                            float(clip_eps), _p(loss_out), _p(grad_params), _p(workspace),
                                                            int(reduce_mode), _p(saved), _stream()),
               'asac_mlp_backward_qloss_return_loaded')
        return
    assert save.dtype == torch.float32 and save.is_contiguous() and save.numel() >= policy_forward_save_floats(pi_job.N)
    _check(load().asac_mlp_backward_qloss_return_rider_loaded(C.byref(job), _p(target_q), C.byref(ret), _p(weights),
                                                              float(clip_eps), _p(loss_out), _p(grad_params), _p(workspace),
                                                              int(reduce_mode), C.byref(pi_job), _p(save), _p(saved),
                                                              _stream()), 'asac_mlp_backward_qloss_return_rider_loaded')


mlp_backward_qloss_return_loaded = _profiled(_mlp_backward_qloss_return_loaded, 'asac_mlp_backward_qloss_return')


@_profiled
def mlp_backward_policy_q(job: MlpJob, q_table, subset, E_sample, grad_x1):
    """Policy step: action gradients of mean_b(-min_{e in subset} q_e) through the stock Q ensemble."""
    global _last_work
    _last_work = _pass_flops(job, backward=True, param_grads=False)
    assert q_table.is_contiguous() and q_table.numel() == job.E * job.N and grad_x1.is_contiguous()
    _check(load().asac_mlp_backward_policy_q(C.byref(job), _p(q_table), _p(subset), E_sample, _p(grad_x1), _stream()),
           'asac_mlp_backward_policy_q')


def _offline_view(offline, N, A):
    """pointer and row stride of the stored actions of the offline loss: an [N, A] view whose rows may be strided"""
    assert offline.dtype == torch.float32 and tuple(offline.shape) == (N, A), 'offline: [N, A] float32 stored actions'
    assert offline.stride(1) == 1, 'offline: the action dimension must be contiguous'
    assert N == 1 or offline.stride(0) >= A, 'offline: overlapping rows'
    return _p(offline), (offline.stride(0) if N > 1 else max(offline.stride(0), A))


def _mlp_backward_policy_sample(job: MlpJob, eps, grad_a, log_alpha, grad_params, workspace, reduce_mode):
    global _last_work
    _last_work = _pass_flops(job, backward=True)
    N, A = job.N, job.desc.contents.head_cols[0]
    assert eps.is_contiguous() and eps.numel() == N * A and grad_a.is_contiguous() and grad_a.numel() % (N * A) == 0
    _check(load().asac_mlp_backward_policy_sample(C.byref(job), _p(eps), _p(grad_a), grad_a.numel() // (N * A),
                                                  _p(log_alpha), _p(grad_params), _p(workspace), int(reduce_mode),
                                                  _stream()), 'asac_mlp_backward_policy_sample')


_mlp_backward_policy_sample = _profiled(_mlp_backward_policy_sample, 'asac_mlp_backward_policy_sample')


@_profiled
def mlp_backward_policy_sample_offline(job: MlpJob, eps, grad_a, log_alpha, offline, grad_params, workspace, reduce_mode):
    """`mlp_backward_policy_sample` with the offline loss' term on the pre-tanh sample (stored actions `offline`)."""
    global _last_work
    _last_work = _pass_flops(job, backward=True)
    N, A = job.N, job.desc.contents.head_cols[0]
    assert eps.is_contiguous() and eps.numel() == N * A and grad_a.is_contiguous() and grad_a.numel() % (N * A) == 0
    po, rso = _offline_view(offline, N, A)
    _check(load().asac_mlp_backward_policy_sample_offline(C.byref(job), _p(eps), _p(grad_a), grad_a.numel() // (N * A),
                                                          _p(log_alpha), po, rso, _p(grad_params), _p(workspace),
                                                          int(reduce_mode), _stream()),
           'asac_mlp_backward_policy_sample_offline')


def mlp_backward_policy_sample(job: MlpJob, eps, grad_a, log_alpha, grad_params, workspace, reduce_mode, offline=None):
    """Policy step: sampling backward + policy backward of the stock Gaussian-head policy (E = 1, no x1) in one launch.
    `offline`: the stored actions ([N, A], rows may be strided) of the offline loss, or None."""
    if offline is None:
        return _mlp_backward_policy_sample(job, eps, grad_a, log_alpha, grad_params, workspace, reduce_mode)
    return mlp_backward_policy_sample_offline(job, eps, grad_a, log_alpha, offline, grad_params, workspace, reduce_mode)


def policy_step_fused_ok(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, N) -> bool:
    return bool(load().asac_policy_step_fused_ok(C.byref(q_desc), _p(q_params), q_member_stride, C.byref(pi_desc),
                                                 _p(pi_params), pi_member_stride, N))


def policy_step_fused(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action, eps,
                      log_alpha, q_out, pi_grad_params, workspace, reduce_mode, subset=None, a_out=None, logp_out=None,
                      ls_out=None, offline=None):
    """The stock networks' whole policy step (two critics) in one launch: critics forward on (x, action), objective
    gradient, critics backward to the action, sampling backward, policy backward (per-tile partials / reduced).
    `offline`: the stored actions ([N, A], rows may be strided) of the offline loss, or None."""
    if offline is not None:
        _offline_view(offline, N, pi_desc.head_cols[0])       # (refused here, before anything is launched)
        return policy_step_fused_offline(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N,
                                         action, eps, log_alpha, q_out, pi_grad_params, workspace, reduce_mode, subset,
                                         a_out, logp_out, ls_out, offline)
    return _policy_step_fused_plain(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action,
                                    eps, log_alpha, q_out, pi_grad_params, workspace, reduce_mode, subset, a_out, logp_out,
                                    ls_out)


@_profiled
def policy_step_fused_offline(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action, eps,
                              log_alpha, q_out, pi_grad_params, workspace, reduce_mode, subset, a_out, logp_out, ls_out,
                              offline):
    """`policy_step_fused` with the offline loss' term on the pre-tanh sample (stored actions `offline`)."""
    return _policy_step_fused(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action, eps,
                              log_alpha, q_out, pi_grad_params, workspace, reduce_mode, subset, a_out, logp_out, ls_out,
                              offline)


def _policy_step_fused(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action, eps,
                       log_alpha, q_out, pi_grad_params, workspace, reduce_mode, subset=None, a_out=None, logp_out=None,
                       ls_out=None, offline=None):
    global _last_work
    _last_work = (mlp_flops(q_desc, 2, N, backward=True, param_grads=False)
                  + mlp_flops(pi_desc, 1, N, backward=True, param_grads=True))
    p0, rs0, _ = _rows_view(x)
    A = pi_desc.head_cols[0]
    assert eps.is_contiguous() and eps.numel() == N * A
    if action is not None:
        assert action.is_contiguous() and action.numel() == N * A
    else:       # sampled on chip
        assert a_out.is_contiguous() and a_out.numel() == N * A and logp_out.is_contiguous() and logp_out.numel() == N
        assert ls_out is None or (ls_out.is_contiguous() and ls_out.numel() == 2 * N * A)
    assert q_out is None or (q_out.is_contiguous() and q_out.numel() % N == 0 and q_out.numel() >= 2 * N)
    assert subset is None or (subset.dtype == torch.int32 and subset.numel() == 2)
    if offline is not None:
        po, rso = _offline_view(offline, N, A)
        _check(load().asac_policy_step_fused_offline(C.byref(q_desc), _p(q_params), q_member_stride, C.byref(pi_desc),
                                                     _p(pi_params), pi_member_stride, p0, rs0, N, _p(action), _p(eps),
                                                     _p(log_alpha), _p(subset), po, rso, _p(q_out), _p(a_out),
                                                     _p(logp_out), _p(ls_out), _p(pi_grad_params), _p(workspace),
                                                     int(reduce_mode), _stream()),
               'asac_policy_step_fused_offline')
        return
    _check(load().asac_policy_step_fused(C.byref(q_desc), _p(q_params), q_member_stride, C.byref(pi_desc), _p(pi_params),
                                         pi_member_stride, p0, rs0, N, _p(action), _p(eps), _p(log_alpha), _p(subset),
                                         _p(q_out), _p(a_out), _p(logp_out), _p(ls_out), _p(pi_grad_params), _p(workspace),
                                         int(reduce_mode), _stream()),
           'asac_policy_step_fused')


_policy_step_fused_plain = _profiled(_policy_step_fused, 'asac_policy_step_fused')


def policy_step_fused_loaded_ok(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, N, saved) -> bool:
    return bool(load().asac_policy_step_fused_loaded_ok(C.byref(q_desc), _p(q_params), q_member_stride, C.byref(pi_desc),
                                                        _p(pi_params), pi_member_stride, N, _p(saved)))


def _policy_step_fused_loaded(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action, eps,
                              log_alpha, saved, q_out, pi_grad_params, workspace, reduce_mode, subset=None, offline=None):
    global _last_work
    _last_work = (mlp_flops(q_desc, 2, N, backward=True, param_grads=False)
                  + mlp_flops(pi_desc, 1, N, backward=True, param_grads=True))
    p0, rs0, _ = _rows_view(x)
    A = pi_desc.head_cols[0]
    assert eps.is_contiguous() and eps.numel() == N * A
    assert action is not None and action.is_contiguous() and action.numel() == N * A
    assert saved.dtype == torch.float32 and saved.is_contiguous() and saved.numel() >= policy_forward_save_floats(N)
    assert q_out is None or (q_out.is_contiguous() and q_out.numel() % N == 0 and q_out.numel() >= 2 * N)
    assert subset is None or (subset.dtype == torch.int32 and subset.numel() == 2)
    if offline is not None:
        po, rso = _offline_view(offline, N, A)
        _check(load().asac_policy_step_fused_loaded_offline(C.byref(q_desc), _p(q_params), q_member_stride,
                                                            C.byref(pi_desc), _p(pi_params), pi_member_stride, p0, rs0, N,
                                                            _p(action), _p(eps), _p(log_alpha), _p(subset), po, rso,
                                                            _p(saved), _p(q_out), _p(pi_grad_params), _p(workspace),
                                                            int(reduce_mode), _stream()),
               'asac_policy_step_fused_loaded_offline')
        return
    _check(load().asac_policy_step_fused_loaded(C.byref(q_desc), _p(q_params), q_member_stride, C.byref(pi_desc),
                                                _p(pi_params), pi_member_stride, p0, rs0, N, _p(action), _p(eps),
                                                _p(log_alpha), _p(subset), _p(saved), _p(q_out), _p(pi_grad_params),
                                                _p(workspace), int(reduce_mode), _stream()),
           'asac_policy_step_fused_loaded')


# (recorded under the names of the launches they stand in for)
_policy_step_fused_loaded_plain = _profiled(_policy_step_fused_loaded, 'asac_policy_step_fused')
_policy_step_fused_loaded_offline = _profiled(_policy_step_fused_loaded, 'asac_policy_step_fused_offline')


def policy_step_fused_loaded(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action, eps,
                             log_alpha, saved, q_out, pi_grad_params, workspace, reduce_mode, subset=None, offline=None):
    """`policy_step_fused` with the action given, loading the policy's forward on the rows of `x` from `saved` (what
    `mlp_backward_qloss_return_rider` wrote for the same parameters and rows) instead of recomputing it: same results,
    bit for bit."""
    fn = _policy_step_fused_loaded_plain if offline is None else _policy_step_fused_loaded_offline
    return fn(q_desc, q_params, q_member_stride, pi_desc, pi_params, pi_member_stride, x, N, action, eps, log_alpha, saved,
              q_out, pi_grad_params, workspace, reduce_mode, subset, offline)


@_profiled
def adam_step_partials(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, steps_done, workspace, tiles, E,
                       member_stride, used, accumulate, loss_out=None, loss_rows=0):
    """Adam over E member blocks whose gradients are still per-tile partial sums in `workspace`."""
    assert param.numel() >= E * member_stride and steps_done.dtype == torch.int64
    _check(load().asac_adam_step_partials(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), lr, beta1, beta2, eps,
                                          _p(steps_done), _p(workspace), tiles, E, member_stride, used,
                                          int(bool(accumulate)), _p(loss_out), loss_rows, _stream()),
           'asac_adam_step_partials')


@_profiled
def mlp_backward(job: MlpJob, grad_out, grad_x0, grad_x1, grad_params, workspace, reduce_mode=MLP_REDUCE_ACCUMULATE):
    global _last_work
    _last_work = _pass_flops(job, backward=True, param_grads=grad_params is not None)
    _check(load().asac_mlp_backward(C.byref(job), _p(grad_out), _p(grad_x0), _p(grad_x1), _p(grad_params), _p(workspace),
                                    int(reduce_mode), _stream()), 'asac_mlp_backward')


def attention_supported(Lq: int, Lk: int, D: int) -> bool:
    return bool(load().asac_attention_supported(int(Lq), int(Lk), int(D)))


@_profiled
def attention_forward(q, k, v, mask, out, weights, keep):
    """q [B, Lq, D], k / v [B, Lk, D] dense f32; mask bool / u8 broadcastable view of [B, Lq, Lk] (True = blocked)
    or None -> out [B, Lq, D], weights [B, Lq, Lk] (x keep), keep [B, Lq]."""
    _dense_f32(q, k, v, out, weights, keep)
    B, Lq, D = q.shape
    sb = si = sj = 0
    if mask is not None:
        assert mask.element_size() == 1 and mask.dim() == 3
        sb, si, sj = (0 if mask.shape[d] == 1 else mask.stride(d) for d in range(3))
    _check(load().asac_attention_forward(_p(q), _p(k), _p(v), _p(mask), sb, si, sj, B, Lq, k.shape[1], D, _p(out),
                                         _p(weights), _p(keep), _stream()), 'asac_attention_forward')


@_profiled
def attention_backward(q, k, v, weights, grad_out, grad_weights, grad_q, grad_k, grad_v):
    _dense_f32(q, k, v, weights, grad_out, grad_weights, grad_q, grad_k, grad_v)
    B, Lq, D = q.shape
    _check(load().asac_attention_backward(_p(q), _p(k), _p(v), _p(weights), _p(grad_out), _p(grad_weights), B, Lq,
                                          k.shape[1], D, _p(grad_q), _p(grad_k), _p(grad_v), _stream()),
           'asac_attention_backward')


def _proj_ptrs(params):
    """6 tensors (Wq, bq, Wk, bk, Wv, bv) or 8 (+ Wo, bo: the output ResBlock)"""
    assert len(params) in (6, 8)
    arr = (C.c_void_p * 8)()
    for i, t in enumerate(params):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
        arr[i] = t.data_ptr()
    return arr


def _rows3(x):
    """[B, L, E] view with a dense last dim -> (ptr, batch stride, row stride)"""
    assert x.dim() == 3 and x.stride(2) == 1 and x.dtype == torch.float32 and x.is_cuda
    return _p(x), x.stride(0), x.stride(1)


def attention_proj_workspace(B, Lq, Lk, E) -> int:
    return int(load().asac_attention_proj_workspace(B, Lq, Lk, E))


def _row_mask(row_zero):
    if row_zero is None:
        return None, 0, 0
    assert row_zero.dim() == 2 and row_zero.element_size() == 1 and row_zero.is_cuda
    return _p(row_zero), row_zero.stride(0), row_zero.stride(1)


@_profiled
def attention_proj_forward(xq, xk, params, mask, out, weights, keep, attn_out=None, row_zero=None):
    """q / k / v projections (params = Wq, bq, Wk, bk, Wv, bv [, Wo, bo]) + attention core [+ output ResBlock and
    the dead-row rule] in one launch; xq [B, Lq, E] and xk [B, Lk, E] may be strided views (dense last dim);
    attn_out [B, Lq, E] receives the attention output when the output block is on chip."""
    _dense_f32(out, weights, keep, attn_out)
    pq, qsb, qsr = _rows3(xq)
    pk, ksb, ksr = _rows3(xk)
    sb = si = sj = 0
    if mask is not None:
        assert mask.element_size() == 1 and mask.dim() == 3
        sb, si, sj = (0 if mask.shape[d] == 1 else mask.stride(d) for d in range(3))
    _check(load().asac_attention_proj_forward(pq, qsb, qsr, pk, ksb, ksr, _proj_ptrs(params), _p(mask), sb, si, sj,
                                              xq.shape[0], xq.shape[1], xk.shape[1], xq.shape[2], _p(out), _p(weights),
                                              _p(keep), _p(attn_out), *_row_mask(row_zero), _stream()),
           'asac_attention_proj_forward')


@_profiled
def attention_proj_backward(xq, xk, params, weights, grad_out, grad_weights, grad_xq, grad_xk, grad_params, accumulate,
                            workspace, keep=None, attn_out=None, row_zero=None):
    """grad_out: [B, Lq, E] view with a dense last dim (read in place); grad_xq None: the queries are the last Lq key
    rows and their gradient is added into those rows of grad_xk by the launch"""
    _dense_f32(weights, grad_weights, grad_xq, grad_xk, grad_params, workspace, keep, attn_out)
    pq, qsb, qsr = _rows3(xq)
    pk, ksb, ksr = _rows3(xk)
    pg, gsb, gsr = _rows3(grad_out)
    _check(load().asac_attention_proj_backward(pq, qsb, qsr, pk, ksb, ksr, _proj_ptrs(params), _p(weights), _p(keep),
                                               _p(attn_out), pg, gsb, gsr, _p(grad_weights), *_row_mask(row_zero),
                                               xq.shape[0], xq.shape[1], xk.shape[1], xq.shape[2],
                                               _p(grad_xq), _p(grad_xk), _p(grad_params),
                                               _sum_mode(accumulate),
                                               _p(workspace), _stream()), 'asac_attention_proj_backward')


# `accumulate` of attention_proj_backward / conv2_backward*: the partials stay in the workspace (for `sum_partials_multi`)
ATTN_SUM_DEFER, CONV_SUM_DEFER = _defined('ATTN_SUM_DEFER', 'CONV_SUM_DEFER')
SUM_DEFER = ATTN_SUM_DEFER
SUM_PARTIALS_MAX_JOBS = _defined('SUM_PARTIALS_MAX_JOBS')


def attention_proj_partials(workspace, E: int, output_block: bool):
    """-> (slabs, n) of the partials an `attention_proj_backward(..., accumulate=ATTN_SUM_DEFER)` left in `workspace`"""
    return workspace.numel() // (4 * (E * E + E)), (4 if output_block else 3) * (E * E + E)


@_profiled
def sum_partials_multi(jobs):
    """jobs: [(partial, slabs, slices, slab_stride, n, out, accumulate), ...] (at most SUM_PARTIALS_MAX_JOBS) — out[:n]
    (+)= the slabs of `partial` in the fixed order of the launch each job stands for (slices 16: the sliced reductions of
    `mlp_backward` with >= 64 tiles and of `attention_proj_backward`; 1: slab order), as ONE launch.  The jobs run side by
    side: no two of them may name overlapping `out[:n]` (RuntimeError, "one output twice")"""
    assert 1 <= len(jobs) <= SUM_PARTIALS_MAX_JOBS
    arr = (PartialSum * len(jobs))()
    for k, (partial, slabs, slices, slab_stride, n, out, accumulate) in enumerate(jobs):
        assert partial.dtype == out.dtype == torch.float32 and partial.is_cuda and out.is_cuda
        assert partial.numel() >= (slabs - 1) * slab_stride + n and out.numel() >= n
        arr[k] = PartialSum(partial.data_ptr(), out.data_ptr(), int(slab_stride), int(n), int(slabs), int(slices),
                            int(bool(accumulate)), 0)
    _check(load().asac_sum_partials_multi(len(jobs), arr, _stream()), 'asac_sum_partials_multi')


LINEAR_TANH_MAX_IN, LINEAR_TANH_MAX_OUT = _defined('LINEAR_TANH_MAX_IN', 'LINEAR_TANH_MAX_OUT')


def _rows2(x):
    """[N, K] view with a dense last dim -> (ptr, row stride)"""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and x.is_cuda
    return _p(x), x.stride(0)


def linear_tanh_workspace(N, K, O) -> int:
    return int(load().asac_linear_tanh_workspace(N, K, O))


@_profiled
def linear_tanh_forward(x, weight, bias, y):
    """y[N, O] = tanh(x[N, K] weight[O, K]^T + bias) in one launch; x may have a row stride"""
    _dense_f32(weight, bias, y)
    px, sx = _rows2(x)
    _check(load().asac_linear_tanh_forward(px, sx, _p(weight), _p(bias), x.shape[0], x.shape[1], weight.shape[0], _p(y),
                                           _stream()), 'asac_linear_tanh_forward')


@_profiled
def linear_tanh_backward(x, weight, y, grad_y, grad_x, grad_params, accumulate, workspace):
    """grad_x [N, K] (or None) and the packed (weight | bias) gradient from grad_y [N, O]; `workspace` holds
    linear_tanh_workspace floats and must be zero before its first use"""
    _dense_f32(weight, y, grad_y, grad_x, grad_params, workspace)
    px, sx = _rows2(x)
    _check(load().asac_linear_tanh_backward(px, sx, _p(weight), _p(y), _p(grad_y), x.shape[0], x.shape[1],
                                            weight.shape[0], _p(grad_x), _p(grad_params), int(bool(accumulate)),
                                            _p(workspace), _stream()), 'asac_linear_tanh_backward')


MASKED_MSE_MAX = _defined('MASKED_MSE_MAX')
_EXCHANGE_WS = {}


def _exchange_words(entry: str, device, *size) -> torch.Tensor:
    """the cached exchange words (workgroup partials + arrival counter, csrc/asac_ordered_finish.h) of one entry point on one
    device, `<entry>_workspace(*size)` floats (asked once per size): zero before first use, left ready by every launch"""
    key = (entry, size, torch.device(device))
    if key not in _EXCHANGE_WS:
        _EXCHANGE_WS[key] = torch.zeros(int(getattr(load(), entry + '_workspace')(*size)), dtype=torch.float32, device=key[2])
    return _EXCHANGE_WS[key]


def _window3(t):
    """[B, T, K] f32 view with a dense last dim -> (pointer, batch stride, step stride)"""
    assert t.dim() == 3 and t.dtype == torch.float32 and t.is_cuda and (t.stride(2) == 1 or t.shape[2] == 1)
    return _p(t), t.stride(0), t.stride(1)


@_profiled
def curiosity_bonus(approx, actual, reward, strength):
    """reward[B, T] += strength * 0.5 * sum_k (approx - actual)^2 in place (approx dense [B, T, K]; actual, reward views)"""
    B, T, K = approx.shape
    assert approx.is_contiguous() and actual.shape == approx.shape and reward.shape == (B, T)
    assert reward.dtype == torch.float32 and (reward.stride(1) == 1 or T == 1)
    pa, sb, st = _window3(actual)
    _check(load().asac_curiosity_bonus(_p(approx), pa, sb, st, _p(reward), reward.stride(0), B, T, K, float(strength),
                                       _stream()), 'asac_curiosity_bonus')


@_profiled
def masked_mse(pred, target, padding_mask, grad_out, loss_out, workspace=None):
    """loss_out <- mean over all elements of ((pred - target) * ~mask)^2, grad_out <- its gradient w.r.t. pred
    (`workspace`, here and below: the caller's own zeroed exchange words instead of the cached ones)"""
    B, T, K = pred.shape
    assert pred.is_contiguous() and grad_out.is_contiguous() and grad_out.shape == pred.shape and target.shape == pred.shape
    pt, sb, st = _window3(target)
    pm, ms = None, 0
    if padding_mask is not None:
        assert padding_mask.shape == (B, T) and padding_mask.element_size() == 1 and (padding_mask.stride(1) == 1 or T == 1)
        pm, ms = _p(padding_mask), padding_mask.stride(0)
    ws = workspace if workspace is not None else _exchange_words('asac_masked_mse', pred.device, pred.numel())
    _check(load().asac_masked_mse(_p(pred), pt, sb, st, pm, ms, B, T, K, _p(grad_out), _p(loss_out), _p(ws),
                                  _stream()), 'asac_masked_mse')


@_profiled
def mse_mean_grad(pred, target, grad_out, loss_out, workspace, grad_scale: float = 1.0):
    """loss_out <- mean((pred - target)^2), grad_out <- its gradient w.r.t. pred; pred [B, T, K] dense, target a [B, T, K]
    view with a dense last dimension (see `mse_mean_grad_ok`); `workspace`: zeros(mse_mean_grad_workspace()), kept by the caller"""
    B, T, K = pred.shape
    pt, sb, st = _window3(target)
    _check(load().asac_mse_mean_grad(_p(pred), pt, sb, st, B, T, K, float(grad_scale), _p(grad_out), _p(loss_out),
                                     _p(workspace), _stream()), 'asac_mse_mean_grad')


def mse_mean_grad_workspace() -> int:
    return int(load().asac_mse_mean_grad_workspace())


def mse_mean_grad_ok(pred, target) -> bool:
    return (pred.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32 and pred.dim() == 3
            and pred.is_contiguous() and target.shape == pred.shape and target.stride(2) == 1 and pred.shape[2] % 4 == 0
            and target.stride(0) % 4 == 0 and target.stride(1) % 4 == 0 and pred.data_ptr() % 16 == 0
            and target.data_ptr() % 16 == 0 and 0 < pred.numel() < 2 ** 33)


@_profiled
def normal_nll_kl(loc, scale, target, kl_weight, grad_loc, grad_scale, out, workspace=None):
    """out[0] <- -mean(log N(target; loc, scale)) + kl_weight * mean(KL(N(loc, scale) || N(0, 1))), out[1] <- mean
    entropy, grad_loc / grad_scale <- d out[0] / d loc, / d scale ([B, T, K] views in, dense gradients out)"""
    B, T, K = loc.shape
    assert scale.shape == loc.shape and target.shape == loc.shape and grad_loc.is_contiguous() and grad_scale.is_contiguous()
    assert grad_loc.numel() == loc.numel() == grad_scale.numel() and out.numel() == 2 and out.is_contiguous()
    pl, lb, lt = _window3(loc)
    ps, sb, st = _window3(scale)
    pt, tb, tt = _window3(target)
    ws = workspace if workspace is not None else _exchange_words('asac_normal_nll_kl', loc.device, loc.numel())
    _check(load().asac_normal_nll_kl(pl, lb, lt, ps, sb, st, pt, tb, tt, B, T, K, float(kl_weight), _p(grad_loc),
                                     _p(grad_scale), _p(out), _p(ws), _stream()), 'asac_normal_nll_kl')


@_profiled
def normal_nll_kl_logstd(raw, scale_min, scale_max, target, kl_weight, grad_raw, out, workspace=None):
    """`normal_nll_kl` of N(mean, clamp(exp(logstd), scale_min, scale_max)) with (mean | logstd) = the halves of raw
    [B, T, 2K]; grad_raw [B, T, 2K] dense <- d out[0] / d raw"""
    B, T, K2 = raw.shape
    K = K2 // 2
    assert K2 == 2 * K and raw.stride(2) == 1 and target.shape == (B, T, K) and target.stride(2) == 1
    assert grad_raw.is_contiguous() and grad_raw.shape == raw.shape and out.numel() == 2 and out.is_contiguous()
    _dense_f32(grad_raw, out)
    ws = workspace if workspace is not None else _exchange_words('asac_normal_nll_kl', raw.device, B * T * K)  # (its kernel)
    _check(load().asac_normal_nll_kl_logstd(_p(raw), raw.stride(0), raw.stride(1), float(scale_min), float(scale_max),
                                            _p(target), target.stride(0), target.stride(1), B, T, K, float(kl_weight),
                                            _p(grad_raw), _p(out), _p(ws), _stream()), 'asac_normal_nll_kl_logstd')


@_profiled
def linear_tanh_forward2(x0, x1, weight, bias, y):
    """y[N, O] = tanh([x0 | x1][N, K0 + K1] weight^T + bias): the concatenation read in place (x1 may be None)"""
    _dense_f32(weight, bias, y)
    if isinstance(x0, WindowRows):      # [samples, T, K0] slice of the sampled windows, read in place
        t = x0.t
        assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.float32
        p0, s0, T, sb, N, K0 = _p(t), t.stride(1), t.shape[1], t.stride(0), t.shape[0] * t.shape[1], t.shape[2]
    else:
        (p0, s0), T, sb, N, K0 = _rows2(x0), 0, 0, x0.shape[0], x0.shape[1]
    p1, s1 = _rows2(x1) if x1 is not None else (None, 0)
    assert x1 is None or x1.shape[0] == N
    _check(load().asac_linear_tanh_forward2w(p0, s0, T, sb, K0, p1, s1, 0 if x1 is None else x1.shape[1], _p(weight),
                                             _p(bias), N, weight.shape[0], _p(y), _stream()),
           'asac_linear_tanh_forward2')


@_profiled
def linear_tanh_backward2(x0, x1, weight, y, grad_y, grad_x0, grad_x1, grad_params, accumulate, workspace,
                          members=1, window=1, position=0):
    """`linear_tanh_backward` over the two-part input; grad_y [members, N / window, O]: row r's output gradient is
    sum_e grad_y[e, r // window] when r % window == position, zero otherwise (1, 1, 0: dense [N, O])."""
    _dense_f32(weight, y, grad_y, grad_x0, grad_x1, grad_params, workspace)
    if isinstance(x0, WindowRows):      # [samples, T, K0] slice of the sampled windows, read in place
        t = x0.t
        assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.float32
        p0, s0, T, sb, N, K0 = _p(t), t.stride(1), t.shape[1], t.stride(0), t.shape[0] * t.shape[1], t.shape[2]
    else:
        (p0, s0), T, sb, N, K0 = _rows2(x0), 0, 0, x0.shape[0], x0.shape[1]
    p1, s1 = _rows2(x1) if x1 is not None else (None, 0)
    O = weight.shape[0]
    assert grad_y.numel() == members * (N // window) * O and N % window == 0
    _check(load().asac_linear_tanh_backward2w(p0, s0, T, sb, K0, p1, s1, 0 if x1 is None else x1.shape[1], _p(weight),
                                              _p(y), _p(grad_y), members, window, position, N, O, _p(grad_x0),
                                              _p(grad_x1), _p(grad_params), _sum_mode(accumulate), _p(workspace),
                                              _stream()), 'asac_linear_tanh_backward2')


def conv2_desc(channels, height, width, out1, kernel1, stride1, out2, kernel2, stride2) -> Conv2Desc:
    return Conv2Desc(channels, height, width, out1, kernel1, stride1, out2, kernel2, stride2)


def conv2_supported(desc) -> bool:
    return bool(load().asac_conv2_supported(C.byref(desc)))


def conv2_param_count(desc) -> int:
    return int(load().asac_conv2_param_count(C.byref(desc)))


def _sum_mode(accumulate) -> int:
    """False / True / SUM_DEFER -> the entry points' `accumulate` argument"""
    return SUM_DEFER if (accumulate is not True and accumulate is not False and accumulate == SUM_DEFER) else int(bool(accumulate))


def conv2_backward_slabs(desc, N, n_cot=1) -> int:
    """partial slabs a backward launch over N frames with n_cot cotangents leaves in its workspace (`SUM_DEFER`)"""
    return int(load().asac_conv2_backward_slabs(C.byref(desc), N, n_cot))


def conv2_backward_workspace(desc, N) -> int:
    return int(load().asac_conv2_backward_workspace(C.byref(desc), N))


def _dense_f32(*ts):
    for t in ts:
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32)


def conv2_flops(desc, N, backward=False) -> float:
    """multiply-adds x 2 of the two implicit GEMMs (backward: both weight-gradient GEMMs + the layer-1
    activation gradient)"""
    h1 = (desc.height - desc.kernel1) // desc.stride1 + 1
    w1 = (desc.width - desc.kernel1) // desc.stride1 + 1
    h2, w2 = (h1 - desc.kernel2) // desc.stride2 + 1, (w1 - desc.kernel2) // desc.stride2 + 1
    g1 = h1 * w1 * desc.channels * desc.kernel1 ** 2 * desc.out1
    g2 = h2 * w2 * desc.out1 * desc.kernel2 ** 2 * desc.out2
    return 2.0 * N * ((g1 + 2 * g2) if backward else (g1 + g2))


@_profiled
def conv2_forward(desc, x, w1, b1, w2, b2, y, z1_out=None, z2_out=None):
    """x [N, C, H, W] -> y [N, out2*H2*W2] (Conv2d GELU Conv2d GELU, flattened channel-major); z1_out
    [N, H1*W1, out1] / z2_out [N, out2*H2*W2]: pre-activations for the backward (both or neither)."""
    global _last_work
    _last_work = conv2_flops(desc, x.shape[0])
    _dense_f32(x, w1, b1, w2, b2, y, z1_out, z2_out)
    _check(load().asac_conv2_forward(C.byref(desc), _p(x), x.shape[0], _p(w1), _p(b1), _p(w2), _p(b2), _p(y),
                                     _p(z1_out), _p(z2_out), _stream()), 'asac_conv2_forward')


def conv2_group_frames(desc) -> int:
    return int(load().asac_conv2_group_frames(C.byref(desc)))


def conv2_tiles(desc) -> int:
    """blocks per frame (1: the whole frame in one piece; > 1: frames whose second-layer map exceeds 16 positions)"""
    return int(load().asac_conv2_tiles(C.byref(desc)))


def conv2_z1_floats(desc, N) -> int:
    """size of the `z1_out` buffer of a training forward over N frames"""
    return int(load().asac_conv2_z1_floats(C.byref(desc), int(N)))


@_profiled
def conv2_forward_windows(desc, x, w1, b1, w2, b2, y, z1_out=None, z2_out=None):
    """`conv2_forward` over x [B, T, C, H, W] = a slice of the sampled windows (dense frames, samples x.stride(0)
    floats apart, T a multiple of `conv2_group_frames`), read in place -> y [B * T, out]"""
    global _last_work
    B, T = x.shape[:2]
    _last_work = conv2_flops(desc, B * T)
    _dense_f32(w1, b1, w2, b2, y, z1_out, z2_out)
    assert x.dtype == torch.float32 and x.is_cuda and x[0].is_contiguous()
    _check(load().asac_conv2_forward_windows(C.byref(desc), _p(x), B * T, T, x.stride(0), _p(w1), _p(b1), _p(w2), _p(b2),
                                             _p(y), _p(z1_out), _p(z2_out), _stream()), 'asac_conv2_forward_windows')


@_profiled
def conv2_backward_windows(desc, x, w2, z1, z2, grad_y, grad_params, workspace, accumulate=False):
    """`conv2_backward` with x [B, T, C, H, W] a slice of the sampled windows read in place (see `conv2_forward_windows`)"""
    global _last_work
    B, T = x.shape[:2]
    _last_work = conv2_flops(desc, B * T, backward=True)
    _dense_f32(w2, z1, z2, grad_y, grad_params, workspace)
    assert x.dtype == torch.float32 and x.is_cuda and x[0].is_contiguous()
    _check(load().asac_conv2_backward_windows(C.byref(desc), _p(x), B * T, T, x.stride(0), _p(w2), _p(z1), _p(z2),
                                              _p(grad_y), _p(grad_params), _sum_mode(accumulate), _p(workspace),
                                              _stream()), 'asac_conv2_backward_windows')


CONV2_MAX_COTANGENTS = 4


def conv2_backward_multi_max(desc) -> int:
    """cotangents ONE launch of `conv2_backward_multi` takes for these frames (more: launches of at most this many)"""
    return int(load().asac_conv2_backward_multi_max(C.byref(desc)))


@_profiled
def conv2_backward_multi(desc, x, w2, z1, z2, grad_ys, grads_out, workspace, accumulate=False):
    """Several backward walks of ONE forward pass as one launch: `grad_ys` = 1..4 output gradients, `grads_out`
    [len(grad_ys), param_count] <- the packed gradients per cotangent, bit-identical to one `conv2_backward(_windows)` each.
    `x` [N, C, H, W] dense, or [B, T, C, H, W] a slice of the sampled windows read in place; workspace: len(grad_ys) x
    `conv2_backward_workspace` floats."""
    global _last_work
    nc = len(grad_ys)
    assert 1 <= nc <= CONV2_MAX_COTANGENTS and grads_out.shape[0] == nc
    windows = x.dim() == 5
    n_frames = x.shape[0] * x.shape[1] if windows else x.shape[0]
    _last_work = nc * conv2_flops(desc, n_frames, backward=True)
    _dense_f32(w2, z1, z2, grads_out, workspace, *grad_ys)
    if windows:
        assert x.dtype == torch.float32 and x.is_cuda and x[0].is_contiguous()
        fps, stride = x.shape[1], x.stride(0)
    else:
        _dense_f32(x)
        fps, stride = 0, 0
    ptrs = (C.c_void_p * nc)(*[g.data_ptr() for g in grad_ys])
    _check(load().asac_conv2_backward_multi(C.byref(desc), _p(x), n_frames, fps, stride, _p(w2), _p(z1), _p(z2), ptrs, nc,
                                            _p(grads_out), _sum_mode(accumulate), _p(workspace), _stream()),
           'asac_conv2_backward_multi')


@_profiled
def conv2_backward(desc, x, w2, z1, z2, grad_y, grad_params, workspace, accumulate=False):
    """-> grad_params (packed w1 | b1 | w2 | b2: written, or added with `accumulate`)."""
    global _last_work
    _last_work = conv2_flops(desc, x.shape[0], backward=True)
    _dense_f32(x, w2, z1, z2, grad_y, grad_params, workspace)
    _check(load().asac_conv2_backward(C.byref(desc), _p(x), x.shape[0], _p(w2), _p(z1), _p(z2), _p(grad_y),
                                      _p(grad_params), _sum_mode(accumulate), _p(workspace), _stream()),
           'asac_conv2_backward')


def conv1_desc(length, channels, out1, kernel1, stride1, out2, kernel2, stride2, negative_slope=0.01) -> Conv1Desc:
    return Conv1Desc(length, channels, out1, kernel1, stride1, out2, kernel2, stride2, negative_slope)


def conv1_supported(desc) -> bool:
    return bool(load().asac_conv1_supported(C.byref(desc)))


def conv1_param_count(desc) -> int:
    return int(load().asac_conv1_param_count(C.byref(desc)))


def conv1_backward_workspace(desc, N) -> int:
    return int(load().asac_conv1_backward_workspace(C.byref(desc), N))


def conv1_backward_slabs(desc, N) -> int:
    """partial slabs a backward launch over N rays leaves in its workspace (`SUM_DEFER`)"""
    return int(load().asac_conv1_backward_slabs(C.byref(desc), N))


def conv1_out_shape(desc):
    """-> (L1, L2): positions of the two maps"""
    l1 = (desc.length - desc.kernel1) // desc.stride1 + 1
    return l1, (l1 - desc.kernel2) // desc.stride2 + 1


def conv1_flops(desc, N, backward=False) -> float:
    """multiply-adds x 2 of the two products (backward: layer 1 again, both weight-gradient products and W2^T dz2)"""
    l1, l2 = conv1_out_shape(desc)
    g1 = l1 * desc.channels * desc.kernel1 * desc.out1
    g2 = l2 * desc.out1 * desc.kernel2 * desc.out2
    return 2.0 * N * ((2 * g1 + 2 * g2) if backward else (g1 + g2))


@_profiled
def conv1_forward(desc, x, w1, b1, w2, b2, y, a1_out=None):
    """x [N, L, C] (channels last, as stored) -> y [N, out2*L2] (Conv1d LeakyReLU Conv1d LeakyReLU, flattened
    channel-major).  `a1_out`: reserved (a form that saves the layer-1 activations); None."""
    global _last_work
    _last_work = conv1_flops(desc, x.shape[0])
    _dense_f32(x, w1, b1, w2, b2, y, a1_out)
    _check(load().asac_conv1_forward(C.byref(desc), _p(x), x.shape[0], _p(w1), _p(b1), _p(w2), _p(b2), _p(y), _p(a1_out),
                                     _stream()), 'asac_conv1_forward')


@_profiled
def conv1_backward(desc, x, w1, b1, w2, y, grad_y, grad_params, workspace, accumulate=False, a1=None):
    """-> grad_params (packed w1 | b1 | w2 | b2: written, added with `accumulate`, or left as slabs with `SUM_DEFER`)."""
    global _last_work
    _last_work = conv1_flops(desc, x.shape[0], backward=True)
    _dense_f32(x, w1, b1, w2, y, a1, grad_y, grad_params, workspace)
    _check(load().asac_conv1_backward(C.byref(desc), _p(x), x.shape[0], _p(w1), _p(b1), _p(w2), _p(y), _p(a1), _p(grad_y),
                                      _p(grad_params), _sum_mode(accumulate), _p(workspace), _stream()),
           'asac_conv1_backward')


def gru_desc(input_size: int, hidden: int, layers: int) -> GruDesc:
    hp = 1
    while hp < hidden:
        hp <<= 1
    return GruDesc(input_size, hidden, hp, layers)


def gru_supported(input_size: int, hidden: int, layers: int) -> bool:
    return 1 <= input_size <= GRU_MAX_DIM and 1 <= hidden <= GRU_MAX_DIM and 1 <= layers <= GRU_MAX_LAYERS


def gru_param_count(desc) -> int:
    return int(load().asac_gru_param_count(C.byref(desc)))


def gru_backward_workspace(desc, B) -> int:
    return int(load().asac_gru_backward_workspace(C.byref(desc), B))


def _gru_ptrs(weights, desc):
    """weights: per layer (w_ih, w_hh, b_ih, b_hh) contiguous f32 device tensors."""
    arrs = [_PtrArray() for _ in range(4)]
    for l in range(desc.layers):
        for k in range(4):
            t = weights[l][k]
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
            arrs[k][l] = t.data_ptr()
    return arrs


def _gru_x(x):
    assert x.dim() == 3 and x.stride(2) == 1 and x.dtype == torch.float32
    return _p(x), x.stride(0), x.stride(1)


def _gru_mask(mask):
    if mask is None:
        return None, 0
    assert mask.dim() == 2 and mask.stride(1) == 1 and mask.element_size() == 1
    return _p(mask), mask.stride(0)


def _gru_h0(h0, desc):
    if h0 is None:
        return None, 0
    assert h0.dim() == 3 and h0.shape[1:] == (desc.layers, desc.hidden) and h0.stride(2) == 1
    assert h0.stride(1) == desc.hidden, 'h0: layers x hidden must be dense per row'
    return _p(h0), h0.stride(0)


@_profiled
def gru_forward(desc, weights, x, h0, padding_mask, hn_out, out_top, gates_out):
    """x [B, L, I]; h0 [B, layers, H] (any batch stride) | None; padding_mask bool/u8 [B, L] | None ->
    hn_out [B, L, layers, H], out_top [B, L, H] | None, gates_out [B, L, layers, 5H] | None."""
    wi, wh, bi, bh = _gru_ptrs(weights, desc)
    px, sb, st = _gru_x(x)
    pm, ms = _gru_mask(padding_mask)
    ph, hs = _gru_h0(h0, desc)
    _check(load().asac_gru_forward(C.byref(desc), wi, wh, bi, bh, px, sb, st, ph, hs, pm, ms, x.shape[0],
                                   x.shape[1], _p(hn_out), _p(out_top), _p(gates_out), _stream()), 'asac_gru_forward')


@_profiled
def gru_forward_twin(desc, weights, twin_weights, x, h0, padding_mask, hn_out, out_top, gates_out, twin_hn_out,
                     twin_out_top):
    """`gru_forward` plus a second parameter set (`twin_weights`, inference only) over the same window in
    the same launch -> twin_hn_out [B, L, layers, H], twin_out_top [B, L, H] | None."""
    wi, wh, bi, bh = _gru_ptrs(weights, desc)
    ti, th, tbi, tbh = _gru_ptrs(twin_weights, desc)
    px, sb, st = _gru_x(x)
    pm, ms = _gru_mask(padding_mask)
    ph, hs = _gru_h0(h0, desc)
    _check(load().asac_gru_forward_twin(C.byref(desc), wi, wh, bi, bh, ti, th, tbi, tbh, px, sb, st, ph, hs, pm, ms,
                                        x.shape[0], x.shape[1], _p(hn_out), _p(out_top), _p(gates_out),
                                        _p(twin_hn_out), _p(twin_out_top), _stream()), 'asac_gru_forward_twin')


def _gru_grad_ptrs(grad_tensors, desc):
    if grad_tensors is None:
        return None
    gt = (C.c_void_p * (4 * GRU_MAX_LAYERS))()
    for l in range(desc.layers):
        for k in range(4):
            t = grad_tensors[l][k]
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
            gt[4 * l + k] = t.data_ptr()
    return gt


@_profiled
def gru_backward(desc, weights, x, h0, padding_mask, hn, gates, grad_hn, grad_top, grad_x, grad_h0, grad_params,
                 grad_tensors, accumulate, workspace):
    """grad_params: packed f32 buffer (written) | None; grad_tensors: per layer (w_ih, w_hh, b_ih, b_hh) gradient
    tensors written / added in place | None — exactly one of the two."""
    wi, wh, bi, bh = _gru_ptrs(weights, desc)
    px, sb, st = _gru_x(x)
    pm, ms = _gru_mask(padding_mask)
    ph, hs = _gru_h0(h0, desc)
    gt = _gru_grad_ptrs(grad_tensors, desc)
    _check(load().asac_gru_backward(C.byref(desc), wi, wh, bi, bh, px, sb, st, ph, hs, pm, ms, x.shape[0],
                                    x.shape[1], _p(hn), _p(gates), _p(grad_hn), _p(grad_top), _p(grad_x), _p(grad_h0),
                                    _p(grad_params), gt, int(bool(accumulate)), _p(workspace), _stream()),
           'asac_gru_backward')


@_profiled
def gru_backward_at(desc, weights, x, h0, padding_mask, hn, gates, grad_top_members, position, grad_x, grad_h0,
                    grad_params, grad_tensors, accumulate, workspace, adam=None):
    """`gru_backward` for an output gradient that lives at ONE window position: grad_top_members [E, B, H] are the
    ensemble members' gradients of out_top[:, position] (summed inside the launch); the recursion starts there.
    `adam` (`adam_epilogue`, with `grad_tensors`): the launch that finishes the gradients also steps those parameters."""
    wi, wh, bi, bh = _gru_ptrs(weights, desc)
    px, sb, st = _gru_x(x)
    pm, ms = _gru_mask(padding_mask)
    ph, hs = _gru_h0(h0, desc)
    m = grad_top_members
    assert m.dim() == 3 and m.is_contiguous() and m.dtype == torch.float32 and m.shape[1:] == (x.shape[0], desc.hidden)
    gt = _gru_grad_ptrs(grad_tensors, desc)
    if adam is not None:
        assert grad_tensors is not None
        for l in range(desc.layers):
            for t in grad_tensors[l]:
                assert adam._span[0] <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= adam._span[1], \
                    'adam epilogue: a gradient tensor outside the flat gradient buffer'
    _check(load().asac_gru_backward_at(C.byref(desc), wi, wh, bi, bh, px, sb, st, ph, hs, pm, ms, x.shape[0],
                                       x.shape[1], _p(hn), _p(gates), _p(m), m.shape[0], int(position), _p(grad_x),
                                       _p(grad_h0), _p(grad_params), gt, int(bool(accumulate)),
                                       C.byref(adam) if adam is not None else None, _p(workspace),
                                       _stream()), 'asac_gru_backward_at')


@_profiled
def gauss_head_fwd(raw, A, loc, scale):
    _check(load().asac_gauss_head_fwd(_p(raw), raw.numel() // (2 * A), A, _p(loc), _p(scale), _stream()),
           'asac_gauss_head_fwd')


@_profiled
def gauss_head_bwd(raw, grad_loc, grad_scale, A, grad_raw):
    _check(load().asac_gauss_head_bwd(_p(raw), _p(grad_loc), _p(grad_scale), raw.numel() // (2 * A), A,
                                      _p(grad_raw), _stream()), 'asac_gauss_head_bwd')


@_profiled
def policy_loss_fwd_bwd(logp, q, subset, E_sample, log_alpha, scale, loss_out, grad_logp, grad_q, entropy_out):
    E, B = q.shape
    A = scale.shape[-1] if scale is not None else 0
    rs = scale.stride(-2) if scale is not None else 0
    _check(load().asac_policy_loss_fwd_bwd(_p(logp), _p(q), _p(subset), E, E_sample, B, _p(log_alpha), _p(scale),
                                           rs, A, _p(loss_out), _p(grad_logp), _p(grad_q), _p(entropy_out), _stream()),
           'asac_policy_loss_fwd_bwd')


@_profiled
def policy_offline_term(ls, eps, offline, loss_inout, grad_u_out=None):
    """The offline loss' term of the policy objective: `loss_inout += mean_b sum_d (u - a)^2`, u = loc + eps * scale from
    the [N, 2A] rows `ls` = (loc | scale), a the stored actions `offline` ([N, A], rows may be strided); with
    `grad_u_out` ([N, A]) also its gradient at u."""
    N, A = eps.shape[0], eps.shape[-1]
    assert ls.dtype == torch.float32 and tuple(ls.shape) == (N, 2 * A) and ls.stride(1) == 1
    assert eps.is_contiguous() and eps.numel() == N * A
    assert grad_u_out is None or (grad_u_out.is_contiguous() and grad_u_out.numel() == N * A)
    po, rso = _offline_view(offline, N, A)
    rs = ls.stride(0) if N > 1 else max(ls.stride(0), 2 * A)
    _check(load().asac_policy_offline_term(_p(ls), C.c_void_p(ls.data_ptr() + 4 * A), rs, _p(eps), po, rso, N, A,
                                           _p(loss_inout), _p(grad_u_out), _stream()), 'asac_policy_offline_term')


@_profiled
def alpha_grad(logp, target, grad_slot):
    _check(load().asac_alpha_grad(_p(logp), logp.numel(), float(target), _p(grad_slot), _stream()),
           'asac_alpha_grad')


@_profiled
def noise_fill(seed, step_counter, uniform_out, normal_out, subsets_out=None, ensemble=0):
    """uniform_out: f64 tensor | None; normal_out: f32 tensor | None (both dense); `step_counter` i64[1] on
    the device selects the block of the Philox stream.  subsets_out: i32 [k, E_sample] | None — k random
    E_sample-subsets of range(ensemble)."""
    assert step_counter.dtype == torch.int64
    nu = 0 if uniform_out is None else uniform_out.numel()
    nn_ = 0 if normal_out is None else normal_out.numel()
    assert (uniform_out is None or (uniform_out.dtype == torch.float64 and uniform_out.is_contiguous()))
    assert (normal_out is None or (normal_out.dtype == torch.float32 and normal_out.is_contiguous()))
    ns = es = 0
    if subsets_out is not None:
        assert subsets_out.dtype == torch.int32 and subsets_out.is_contiguous() and subsets_out.dim() == 2
        ns, es = subsets_out.shape
    _check(load().asac_noise_fill(C.c_uint64(int(seed) & (2 ** 64 - 1)), _p(step_counter), _p(uniform_out), nu,
                                  _p(normal_out), nn_, _p(subsets_out), ns, es, int(ensemble), _stream()),
           'asac_noise_fill')


@_profiled
def step_prologue(polyak, zero, seed, step_counter, uniform_out, normal_out, subsets_out=None, ensemble=0):
    """`polyak` (= (target_flat, source_flat, tau) | None) + a memset of `zero` (flat f32 | None) + `noise_fill`
    in one launch."""
    target_flat, source_flat, tau = polyak if polyak is not None else (None, None, 0.0)
    if polyak is not None:
        assert target_flat.is_contiguous() and source_flat.is_contiguous() \
            and target_flat.numel() == source_flat.numel()
    assert zero is None or (zero.is_contiguous() and zero.dtype == torch.float32)
    nu = 0 if uniform_out is None else uniform_out.numel()
    nn_ = 0 if normal_out is None else normal_out.numel()
    ns = es = 0
    if subsets_out is not None:
        assert subsets_out.dtype == torch.int32 and subsets_out.is_contiguous() and subsets_out.dim() == 2
        ns, es = subsets_out.shape
    _check(load().asac_step_prologue(_p(target_flat), _p(source_flat), 0 if polyak is None else target_flat.numel(),
                                     float(tau), _p(zero), 0 if zero is None else zero.numel(),
                                     C.c_uint64(int(seed) & (2 ** 64 - 1)), _p(step_counter), _p(uniform_out), nu,
                                     _p(normal_out), nn_, _p(subsets_out), ns, es, int(ensemble), _stream()),
           'asac_step_prologue')


PROLOGUE_SAMPLE_MAX_BATCH = 1024


@_profiled
def step_prologue_sample(polyak, zero, seed, step_counter, uniform_out, normal_out, subsets_out, ensemble, tree,
                         capacity, batch, slot_ids, beta_state, beta_increment, leaf_out, p_out, ids_out, is_weights_out,
                         min_p_out):
    """`step_prologue` + the single-workgroup `sumtree_sample` (batch <= 1024, IS weights fused) in one launch; the
    sampler draws its `batch` uniforms itself and stores them in `uniform_out`."""
    target_flat, source_flat, tau = polyak if polyak is not None else (None, None, 0.0)
    assert uniform_out.numel() == batch and uniform_out.dtype == torch.float64 and batch <= PROLOGUE_SAMPLE_MAX_BATCH
    assert min_p_out.numel() >= 528 and min_p_out.dtype == torch.float32      # [2..9]: the workgroups' exchange
    assert zero is None or (zero.is_contiguous() and zero.dtype == torch.float32)
    nn_ = 0 if normal_out is None else normal_out.numel()
    ns = es = 0
    if subsets_out is not None:
        assert subsets_out.dtype == torch.int32 and subsets_out.is_contiguous() and subsets_out.dim() == 2
        ns, es = subsets_out.shape
    _check(load().asac_step_prologue_sample(
        _p(target_flat), _p(source_flat), 0 if polyak is None else target_flat.numel(), float(tau), _p(zero),
        0 if zero is None else zero.numel(), C.c_uint64(int(seed) & (2 ** 64 - 1)), _p(step_counter), _p(uniform_out),
        _p(normal_out), nn_, _p(subsets_out), ns, es, int(ensemble), _p(tree), capacity, batch, _p(slot_ids),
        _p(beta_state), float(beta_increment), _p(leaf_out), _p(p_out), _p(ids_out), _p(is_weights_out), _p(min_p_out),
        _stream()), 'asac_step_prologue_sample')


@_profiled
def step_prologue_sample_partial(polyak, zero, seed, step_counter, uniform_out, normal_out, subsets_out, ensemble, tree,
                                 capacity, batch, slot_ids, leaf_out, p_out, ids_out, min_p_out):
    """`step_prologue_sample` without the weights: the sampler workgroups leave their minima in `min_p_out[2:]`;
    `window_gather_pad_w` (the next launch; 256 < batch <= 1024) or its sidecar form `sidecar_window_gather_w` (a rider of
    the step's first network launch) forms the weights and advances beta"""
    target_flat, source_flat, tau = polyak if polyak is not None else (None, None, 0.0)
    assert uniform_out.numel() == batch and uniform_out.dtype == torch.float64 and 0 < batch <= PROLOGUE_SAMPLE_MAX_BATCH
    assert min_p_out.numel() >= 528 and min_p_out.dtype == torch.float32
    assert zero is None or (zero.is_contiguous() and zero.dtype == torch.float32)
    nn_ = 0 if normal_out is None else normal_out.numel()
    ns = es = 0
    if subsets_out is not None:
        assert subsets_out.dtype == torch.int32 and subsets_out.is_contiguous() and subsets_out.dim() == 2
        ns, es = subsets_out.shape
    _check(load().asac_step_prologue_sample_partial(
        _p(target_flat), _p(source_flat), 0 if polyak is None else target_flat.numel(), float(tau), _p(zero),
        0 if zero is None else zero.numel(), C.c_uint64(int(seed) & (2 ** 64 - 1)), _p(step_counter), _p(uniform_out),
        _p(normal_out), nn_, _p(subsets_out), ns, es, int(ensemble), _p(tree), capacity, batch, _p(slot_ids),
        _p(leaf_out), _p(p_out), _p(ids_out), _p(min_p_out), _stream()), 'asac_step_prologue_sample_partial')


@_profiled
def window_gather_pad_w(keys, ids, batch, prev_n, post_n, capacity, index_ring, p, tree, beta_state, beta_increment,
                        is_weights_out, min_p_out):
    """`window_gather_pad` + the IS weights of the batch `step_prologue_sample_partial` drew, one launch"""
    _check(load().asac_window_gather_pad_w(keys, len(keys), _p(ids), batch, prev_n, post_n, capacity, _p(index_ring), _p(p),
                                           _p(tree), _p(beta_state), float(beta_increment), _p(is_weights_out),
                                           _p(min_p_out), _stream()), 'asac_window_gather_pad_w')


def graph_launch(graph_exec: int):
    """Replay an instantiated hipGraphExec_t (raw pointer value) on torch's current stream."""
    _check(load().asac_graph_launch(C.c_void_p(int(graph_exec)), _stream()), 'asac_graph_launch')


def graph_replace_memset_nodes(graph: int):
    """Fix-up pass over a captured hipGraph_t (raw pointer value, not yet instantiated): 1-D memset nodes -> kernel nodes
    (csrc/graph_fix.hip: captured memsets take effect on the first launch only on this ROCm).  -> (replaced, kept)"""
    rep, kept = C.c_int(0), C.c_int(0)
    _check(load().asac_graph_replace_memset_nodes(C.c_void_p(int(graph)), C.byref(rep), C.byref(kept)),
           'asac_graph_replace_memset_nodes')
    return rep.value, kept.value


@_profiled
def alpha_adam_step(logp, target, slot, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, steps_done,
                    advance_counter=False):
    """param / grad / exp_avg / exp_avg_sq: the temperature segment [n]; grad[slot] <- mean(-logp) - target,
    then Adam on the segment (single launch); optionally advances the shared step counter afterwards."""
    assert steps_done.dtype == torch.int64 and param.numel() == grad.numel()
    _check(load().asac_alpha_adam_step(_p(logp), logp.numel(), float(target), int(slot), _p(param), _p(grad),
                                       _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, beta1, beta2, eps,
                                       _p(steps_done), int(bool(advance_counter)), _stream()), 'asac_alpha_adam_step')


@_profiled
def polyak(target_flat, source_flat, tau):
    assert target_flat.numel() == source_flat.numel() and target_flat.dtype == torch.float32
    _check(load().asac_polyak(_p(target_flat), _p(source_flat), target_flat.numel(), float(tau), _stream()),
           'asac_polyak')


@_profiled
def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, steps_done):
    assert steps_done.dtype == torch.int64
    _check(load().asac_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr,
                                 beta1, beta2, eps, _p(steps_done), _stream()), 'asac_adam_step')


# ------------------------------------------------------------------------------------------------
# observation decoder of the prediction models (csrc/decoder.hip)
# ------------------------------------------------------------------------------------------------
OBS_DECODER_SHAPES = ((64, None), (64,), (128, 64), (128,), (32, 32, 4, 4), (32,), (32, 16, 8, 8), (16,), (16, 3, 3, 3), (3,))
# multiply-adds of one state's pass through the three transposed convolutions and the dense head
OBS_DECODER_MACS = 64 * 16 + 128 * 64 + 4 * 16 * 32 * 32 + 36 * 64 * 32 * 16 + 784 * 9 * 16 * 3


def _obs_decoder_params(tensors, state_size) -> ObsDecoderParams:
    assert len(tensors) == 10
    for t, shape in zip(tensors, OBS_DECODER_SHAPES):
        want = tuple(state_size if d is None else d for d in shape)
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == want, (t.shape, want)
    ps = ObsDecoderParams(*[t.data_ptr() for t in tensors])
    ps._keep = tuple(tensors)
    return ps


def obs_decoder_packed_floats() -> int:
    return int(load().asac_obs_decoder_packed_floats())


def obs_decoder_saved_floats(N) -> int:
    return int(load().asac_obs_decoder_saved_floats(N))


def obs_decoder_workspace_floats(N) -> int:
    return int(load().asac_obs_decoder_workspace_floats(N))


@_profiled
def obs_decoder_forward(state, params, packed, saved, frames):
    """state [N, S] -> frames [N, 3, 30, 30]; `packed` / `saved`: see include/asac_hip.h"""
    global _last_work
    N, S = state.shape
    _last_work = 2.0 * N * OBS_DECODER_MACS
    _dense_f32(packed, saved, frames)
    assert state.is_cuda and state.dtype == torch.float32 and state.stride(1) == 1 and frames.shape == (N, 3, 30, 30)
    ps = _obs_decoder_params(params, S)
    _check(load().asac_obs_decoder_forward(_p(state), state.stride(0), N, S, C.byref(ps), _p(packed), _p(saved),
                                           _p(frames), _stream()), 'asac_obs_decoder_forward')


@_profiled
def obs_decoder_backward(state, packed, saved, frames, grad_frames, grad_state, grad_params, workspace, accumulate=False):
    """grad_frames [N, 3, 30, 30] -> grad_state [N, S] (or None) and the ten parameter gradients"""
    global _last_work
    N, S = state.shape
    _last_work = 4.0 * N * OBS_DECODER_MACS
    _dense_f32(packed, saved, frames, grad_frames, grad_state, workspace)
    assert state.is_cuda and state.dtype == torch.float32 and state.stride(1) == 1
    gs = _obs_decoder_params(grad_params, S)
    _check(load().asac_obs_decoder_backward(_p(state), state.stride(0), N, S, _p(packed), _p(saved), _p(frames),
                                            _p(grad_frames), _p(grad_state), C.byref(gs), int(bool(accumulate)),
                                            _p(workspace), _stream()), 'asac_obs_decoder_backward')


GATE_MAX_LOSSES, GATE_MAX_N = _defined('GATE_MAX_LOSSES', 'GATE_MAX_N')


@_profiled
def cosine_gate_add(main, aux_list, grad, gates_out=None):
    """grad += sum_k clamp(sign(cos(main, aux_k)), min=0) * aux_k, k in order (flat f32 tensors of one length)"""
    n = main.numel()
    assert 0 < len(aux_list) <= GATE_MAX_LOSSES and 0 < n <= GATE_MAX_N
    _dense_f32(main, grad, gates_out, *aux_list)
    assert grad.numel() == n and all(t.numel() == n for t in aux_list)
    ptrs = (C.c_void_p * len(aux_list))(*[t.data_ptr() for t in aux_list])
    _check(load().asac_cosine_gate_add(_p(main), ptrs, len(aux_list), n, _p(grad), _p(gates_out), _stream()),
           'asac_cosine_gate_add')


# ------------------------------------------------------------------------------------------------
# GRU recurrence for hidden 32 / 64 / 128 (csrc/gru_wide.hip)
# ------------------------------------------------------------------------------------------------
def gru_wide_supported(hidden: int) -> bool:
    return bool(load().asac_gru_wide_supported(int(hidden)))


def _mask_ptr(mask):
    if mask is None:
        return None, 0
    assert mask.is_cuda and mask.element_size() == 1 and mask.dim() == 2 and mask.stride(1) == 1
    return _p(mask), mask.stride(0)


@_profiled
def gru_wide_forward(gi, w_hh, b_hh, h0, mask, out, h_raw, gates):
    """one layer's recurrence: gi [B, L, 3H] -> out [B, L, H] (a strided view is fine); see include/asac_hip.h"""
    global _last_work
    B, L, H3 = gi.shape
    H = H3 // 3
    _last_work = 2.0 * B * L * 3 * H * H
    assert gi.stride(2) == 1 and out.stride(2) == 1 and out.shape == (B, L, H)
    _dense_f32(w_hh, b_hh, h_raw, gates)
    pm, ms = _mask_ptr(mask)
    _check(load().asac_gru_wide_forward(_p(gi), gi.stride(0), gi.stride(1), _p(w_hh), _p(b_hh), _p(h0),
                                        0 if h0 is None else h0.stride(0), pm, ms, B, L, H, _p(out), out.stride(0),
                                        out.stride(1), _p(h_raw), _p(gates), _stream()), 'asac_gru_wide_forward')


@_profiled
def gru_wide_forward_twin(gi2, w_hh, b_hh, w_hh_twin, b_hh_twin, h0, mask, out2, h_raw, gates):
    """the recurrence of ONE layer of two networks over the same B windows: gi2 / out2 [2B, L, .] (network 1 then its twin),
    h0 / mask [B, .], h_raw / gates [B, L, .] (network 1) or None"""
    global _last_work
    B2, L, H3 = gi2.shape
    B, H = B2 // 2, H3 // 3
    _last_work = 2.0 * B2 * L * 3 * H * H
    assert gi2.stride(2) == 1 and out2.stride(2) == 1 and out2.shape == (B2, L, H) and B % 16 == 0
    _dense_f32(w_hh, b_hh, w_hh_twin, b_hh_twin, h_raw, gates)
    pm, ms = _mask_ptr(mask)
    _check(load().asac_gru_wide_forward_twin(_p(gi2), gi2.stride(0), gi2.stride(1), _p(w_hh), _p(b_hh), _p(w_hh_twin),
                                             _p(b_hh_twin), _p(h0), 0 if h0 is None else h0.stride(0), pm, ms, B, L, H,
                                             _p(out2), out2.stride(0), out2.stride(1), _p(h_raw), _p(gates), _stream()),
           'asac_gru_wide_forward_twin')


@_profiled
def gru_wide_backward(grad_out, w_hh_t, gates, h_raw, h0, mask, grad_gi, grad_gh, grad_h0):
    global _last_work
    B, L, H = grad_out.shape
    _last_work = 2.0 * B * L * 3 * H * H
    assert grad_out.stride(2) == 1
    _dense_f32(w_hh_t, gates, h_raw, grad_gi, grad_gh, grad_h0)
    pm, ms = _mask_ptr(mask)
    _check(load().asac_gru_wide_backward(_p(grad_out), grad_out.stride(0), grad_out.stride(1), _p(w_hh_t), _p(gates),
                                         _p(h_raw), _p(h0), 0 if h0 is None else h0.stride(0), pm, ms, B, L, H,
                                         _p(grad_gi), _p(grad_gh), _p(grad_h0), _stream()), 'asac_gru_wide_backward')


# ------------------------------------------------------------------------------------------------
# multi-head attention core (csrc/attn_mh.hip)
# ------------------------------------------------------------------------------------------------
def attention_mh_supported(Lq, Lk, heads, head_dim) -> bool:
    return bool(load().asac_attention_mh_supported(int(Lq), int(Lk), int(heads), int(head_dim)))


def _mask3(mask, B):
    """[1 | B, 1 | Lq, Lk] byte mask -> (pointer, stride_b, stride_q, stride_k) with broadcast strides of 0"""
    if mask is None:
        return None, 0, 0, 0
    assert mask.is_cuda and mask.element_size() == 1 and mask.dim() == 3
    return (_p(mask), 0 if mask.shape[0] == 1 and B > 1 else mask.stride(0), 0 if mask.shape[1] == 1 else mask.stride(1),
            mask.stride(2))


@_profiled
def attention_mh_forward(q, k, v, mask, heads, out, weights, keep, p_heads, row_zero=None, keep_rows=None):
    global _last_work
    B, Lq, E = q.shape
    Lk = k.shape[1]
    _last_work = 4.0 * B * Lq * Lk * E
    _dense_f32(q, k, v, out, weights, keep, p_heads)
    pm, sb, si, sj = _mask3(mask, B)
    if row_zero is not None:
        assert row_zero.shape == (B, Lq) and row_zero.is_contiguous() and row_zero.element_size() == 1 and keep_rows is not None
    _check(load().asac_attention_mh_forward(_p(q), _p(k), _p(v), pm, sb, si, sj, B, Lq, Lk, heads, E // heads, _p(out),
                                            _p(weights), _p(keep), _p(p_heads), _p(row_zero), _p(keep_rows), _stream()),
           'asac_attention_mh_forward')


def attention_mh_proj_supported(Lq, Lk, heads, head_dim) -> bool:
    return bool(load().asac_attention_mh_proj_supported(int(Lq), int(Lk), int(heads), int(head_dim)))


@_profiled
def attention_mh_proj_forward(x, weights, biases, mask, heads, q, k, v, out, attn_weights, keep, p_heads, row_zero=None,
                              keep_rows=None, out_weight=None, out_bias=None, y=None, pre=None):
    """`attention_mh_forward` of q / k / v = the three projections of x [B, Lk, E] (q: its last Lq positions), formed in the
    same launch and written to q / k / v for the backward"""
    global _last_work
    B, Lk, E = x.shape
    Lq = q.shape[1]
    assert x.stride(2) == 1 and len(weights) == len(biases) == 3
    _last_work = 4.0 * B * Lq * Lk * E + 2.0 * B * (Lq + 2 * Lk) * E * E
    _dense_f32(*weights, *biases, q, k, v, out, attn_weights, keep, p_heads, out_weight, out_bias, y, pre)
    if out_weight is not None:
        _last_work += 2.0 * B * Lq * E * E
    pm, sb, si, sj = _mask3(mask, B)
    if row_zero is not None:      # (a slice of a wider mask is read in place: batch stride)
        assert row_zero.shape == (B, Lq) and row_zero.stride(1) == 1 and row_zero.element_size() == 1 and keep_rows is not None
    _check(load().asac_attention_mh_proj_forward(_p(x), x.stride(0), x.stride(1), _ptr_array(weights), _ptr_array(biases), pm, sb,
                                                 si, sj, B, Lq, Lk, heads, E // heads, _p(q), _p(k), _p(v), _p(out),
                                                 _p(attn_weights), _p(keep), _p(p_heads), _p(row_zero),
                                                 0 if row_zero is None else row_zero.stride(0), _p(keep_rows),
                                                 _p(out_weight), _p(out_bias), _p(y), _p(pre), _stream()),
           'asac_attention_mh_proj_forward')


@_profiled
def attention_mh_block_backward(q, k, v, mask, heads, p_heads, grad_y, pre, row_scale, out_weight, grad_weights, proj_weights,
                                grad_q, grad_k, grad_v, grad_pre, grad_x):
    """the backward of `attention_mh_proj_forward` with its output block: ResBlock backward, core backward and the projections'
    input gradient as one launch"""
    global _last_work
    B, Lq, E = q.shape
    Lk = k.shape[1]
    _last_work = 10.0 * B * Lq * Lk * E + 2.0 * B * (2 * Lq + 2 * Lk) * E * E
    _dense_f32(q, k, v, p_heads, pre, row_scale, out_weight, grad_weights, *proj_weights, grad_q, grad_k, grad_v, grad_pre, grad_x)
    assert grad_y.shape == q.shape and grad_y.stride(2) == 1 and grad_y.dtype == torch.float32 and grad_y.is_cuda
    pm, sb, si, sj = _mask3(mask, B)
    _check(load().asac_attention_mh_block_backward(_p(q), _p(k), _p(v), pm, sb, si, sj, B, Lq, Lk, heads, E // heads, _p(p_heads),
                                                   _p(grad_y), grad_y.stride(0), grad_y.stride(1), _p(pre), _p(row_scale),
                                                   _p(out_weight), _p(grad_weights),
                                                   _ptr_array(proj_weights), _p(grad_q), _p(grad_k), _p(grad_v), _p(grad_pre),
                                                   _p(grad_x), _stream()), 'asac_attention_mh_block_backward')


@_profiled
def attention_mh_backward(q, k, v, mask, heads, p_heads, grad_out, grad_weights, grad_q, grad_k, grad_v):
    global _last_work
    B, Lq, E = q.shape
    Lk = k.shape[1]
    _last_work = 10.0 * B * Lq * Lk * E
    _dense_f32(q, k, v, p_heads, grad_out, grad_weights, grad_q, grad_k, grad_v)
    pm, sb, si, sj = _mask3(mask, B)
    _check(load().asac_attention_mh_backward(_p(q), _p(k), _p(v), pm, sb, si, sj, B, Lq, Lk, heads, E // heads, _p(p_heads),
                                             _p(grad_out), _p(grad_weights), _p(grad_q), _p(grad_k), _p(grad_v), _stream()),
           'asac_attention_mh_backward')


# attention-weight dropout inside those launches (csrc/asac_dropout.h)
ATTN_DROPOUT_STATE_WORDS = 544      # int64: [0] the call counter, [16] the root arrival word, [32 + 16 g] leaf arrival word g < 32
ATTN_DROPOUT_MAX_BATCH_HEADS = 1 << 24


def dropout_threshold(p: float) -> int:
    """floor(p * 2^32) in float64: an element is DROPPED iff its 32-bit Philox word is below it"""
    return int(math.floor(float(p) * 4294967296.0))


def dropout_scale(p: float) -> float:
    """float32(1 / (1 - p)), the quotient formed in double precision (as ATen's dropout forms it)"""
    return C.c_float(1.0 / (1.0 - float(p))).value


def _drop_state_ok(state, used):
    assert state.is_cuda and state.dtype == torch.int64 and state.is_contiguous() and state.numel() == ATTN_DROPOUT_STATE_WORDS
    assert used.is_cuda and used.dtype == torch.int64 and used.numel() == 1 and used.device == state.device


@_profiled
def attention_mh_dropout_forward(q, k, v, mask, heads, out, weights, keep, p_heads, row_zero, keep_rows, p, seed, instance,
                                 state, used):
    """`attention_mh_forward` with dropout(p) of the softmax weights inside the launch; `state` int64 [544] (the instance's
    call counter and arrival words), `used` int64 [1] <- the counter this call drew with"""
    global _last_work
    B, Lq, E = q.shape
    Lk = k.shape[1]
    _last_work = 4.0 * B * Lq * Lk * E
    _dense_f32(q, k, v, out, weights, keep, p_heads)
    _drop_state_ok(state, used)
    pm, sb, si, sj = _mask3(mask, B)
    if row_zero is not None:
        assert row_zero.shape == (B, Lq) and row_zero.is_contiguous() and row_zero.element_size() == 1 and keep_rows is not None
    _check(load().asac_attention_mh_dropout_forward(_p(q), _p(k), _p(v), pm, sb, si, sj, B, Lq, Lk, heads, E // heads, _p(out),
                                                    _p(weights), _p(keep), _p(p_heads), _p(row_zero), _p(keep_rows),
                                                    dropout_threshold(p), 1.0 / (1.0 - float(p)), int(seed) & (2 ** 64 - 1),
                                                    int(instance) & 0xFFFFFFFF, _p(state), _p(used), _stream()),
           'asac_attention_mh_dropout_forward')


@_profiled
def attention_mh_dropout_backward(q, k, v, mask, heads, p_heads, grad_out, grad_weights, grad_q, grad_k, grad_v, p, seed,
                                  instance, used):
    """the backward of `attention_mh_dropout_forward`: the mask is regenerated from the counter in `used` (read on the device)"""
    global _last_work
    B, Lq, E = q.shape
    Lk = k.shape[1]
    _last_work = 10.0 * B * Lq * Lk * E
    _dense_f32(q, k, v, p_heads, grad_out, grad_weights, grad_q, grad_k, grad_v)
    assert used.is_cuda and used.dtype == torch.int64 and used.numel() == 1
    pm, sb, si, sj = _mask3(mask, B)
    _check(load().asac_attention_mh_dropout_backward(_p(q), _p(k), _p(v), pm, sb, si, sj, B, Lq, Lk, heads, E // heads,
                                                     _p(p_heads), _p(grad_out), _p(grad_weights), _p(grad_q), _p(grad_k),
                                                     _p(grad_v), dropout_threshold(p), 1.0 / (1.0 - float(p)),
                                                     int(seed) & (2 ** 64 - 1), int(instance) & 0xFFFFFFFF, _p(used), _stream()),
           'asac_attention_mh_dropout_backward')


# ------------------------------------------------------------------------------------------------
# the Linear layers around the multi-head attention core (csrc/rows_proj.hip)
# ------------------------------------------------------------------------------------------------
def rows_proj_supported(width) -> bool:
    return bool(load().asac_rows_proj_supported(int(width)))


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


@_profiled
def rows_proj_forward(x, weights, biases, tails, outs):
    """outs[j] [B][tails[j]][E] = x[:, L - tails[j]:] weights[j]^T + biases[j] for the <= 3 jobs, one launch; x [B][L][E] with
    feature stride 1"""
    global _last_work
    B, L, E = x.shape
    assert x.stride(2) == 1 and len(weights) == len(biases) == len(tails) == len(outs) <= 3
    _dense_f32(*weights, *biases, *outs)
    for o, n in zip(outs, tails):
        assert o.shape == (B, n, E)
    _last_work = 2.0 * B * sum(tails) * E * E
    _check(load().asac_rows_proj_forward(_p(x), x.stride(0), x.stride(1), B, L, E, len(outs), _ptr_array(weights),
                                         _ptr_array(biases), (C.c_int * len(tails))(*tails), _ptr_array(outs), _stream()),
           'asac_rows_proj_forward')


@_profiled
def rows_proj_backward(grads, tails, weights, grad_x):
    """grad_x [B][L][E] = sum_j grads[j] weights[j] (job j reaching the newest tails[j] positions), one launch"""
    global _last_work
    B, L, E = grad_x.shape
    _dense_f32(*grads, *weights, grad_x)
    for g, n in zip(grads, tails):
        assert g.shape == (B, n, E)
    _last_work = 2.0 * B * sum(tails) * E * E
    _check(load().asac_rows_proj_backward(_ptr_array(grads), (C.c_int * len(tails))(*tails), len(grads), _ptr_array(weights), B,
                                          L, E, _p(grad_x), _stream()), 'asac_rows_proj_backward')


def rows_affine_supported(K, N) -> bool:
    return bool(load().asac_rows_affine_supported(int(K), int(N)))


@_profiled
def rows_affine_forward(x, weight, bias, y):
    """y [rows, N] = x [rows, K] weight^T + bias (K <= 64, N a multiple of 16): one launch; x may have a row stride"""
    global _last_work
    rows, K = x.shape
    N = weight.shape[0]
    assert x.stride(1) == 1 and x.dtype == torch.float32 and x.is_cuda and y.shape == (rows, N)
    _dense_f32(weight, bias, y)
    _last_work = 2.0 * rows * K * N
    _check(load().asac_rows_affine_forward(_p(x), x.stride(0), K, _p(weight), _p(bias), rows, N, _p(y), _stream()),
           'asac_rows_affine_forward')


@_profiled
def rows_affine_gelu_forward(x, weight, bias, y, pre):
    """y = gelu(x weight^T + bias), pre = x weight^T + bias; as `rows_affine_forward`"""
    global _last_work
    rows, K = x.shape
    N = weight.shape[0]
    assert x.stride(1) == 1 and x.dtype == torch.float32 and x.is_cuda and y.shape == (rows, N) and pre.shape == (rows, N)
    _dense_f32(weight, bias, y, pre)
    _last_work = 2.0 * rows * K * N
    _check(load().asac_rows_affine_gelu_forward(_p(x), x.stride(0), K, _p(weight), _p(bias), rows, N, _p(y), _p(pre), _stream()),
           'asac_rows_affine_gelu_forward')


@_profiled
def rows_resblock_forward(x, weight, bias, row_scale, y, pre):
    """y = (x + gelu(x W^T + b)) * row_scale[:, None], pre = x W^T + b; x [rows][E] with feature stride 1"""
    global _last_work
    rows, E = x.shape
    assert x.stride(1) == 1
    _dense_f32(weight, bias, y, pre, *([] if row_scale is None else [row_scale]))
    _last_work = 2.0 * rows * E * E
    _check(load().asac_rows_resblock_forward(_p(x), x.stride(0), _p(weight), _p(bias), _p(row_scale), rows, E, _p(y), _p(pre),
                                             _stream()), 'asac_rows_resblock_forward')


@_profiled
def rows_resblock_backward(grad_y, pre, weight, row_scale, grad_x, grad_pre):
    global _last_work
    rows, E = grad_y.shape
    _dense_f32(grad_y, pre, weight, grad_x, grad_pre, *([] if row_scale is None else [row_scale]))
    _last_work = 2.0 * rows * E * E
    _check(load().asac_rows_resblock_backward(_p(grad_y), _p(pre), _p(weight), _p(row_scale), rows, E, _p(grad_x), _p(grad_pre),
                                              _stream()), 'asac_rows_resblock_backward')


# the nn.Dropout modules inside the dense stacks around the core, inside the row launches (csrc/rows_proj.hip; draws:
# csrc/asac_dropout.h under tags 6 / 7 / 8 = q / k / v and 9 = the output block; state and `used` as for the core, one state per
# launch site)
ROWS_DROPOUT_TAG_QKV, ROWS_DROPOUT_TAG_OUT = 6, 9


def _draw_args(p, seed, instance):
    return dropout_threshold(p), 1.0 / (1.0 - float(p)), int(seed) & (2 ** 64 - 1), int(instance) & 0xFFFFFFFF


@_profiled
def rows_dense_proj_dropout_forward(x, weights1, biases1, weights2, biases2, tails, outs, pres, hiddens, p, seed, instance,
                                    state, used):
    """the <= 3 stacks ResBlock -> Dropout(p) -> Linear of one input, one launch: pres[j] = x W1^T + b1,
    hiddens[j] = (x + gelu(pres[j])) * mask * s, outs[j] = hiddens[j] W2^T + b2 over x[:, L - tails[j]:]; x [B][L][E] with feature
    stride 1; `used` int64 [1] <- the counter this call drew with"""
    global _last_work
    B, L, E = x.shape
    n = len(outs)
    assert x.stride(2) == 1 and n <= 3 and all(len(t) == n for t in (weights1, biases1, weights2, biases2, tails, pres, hiddens))
    _dense_f32(*weights1, *biases1, *weights2, *biases2, *outs, *pres, *hiddens)
    _drop_state_ok(state, used)
    for o, pr, h, t in zip(outs, pres, hiddens, tails):
        assert o.shape == pr.shape == h.shape == (B, t, E)
    _last_work = 4.0 * B * sum(tails) * E * E
    _check(load().asac_rows_dense_proj_dropout_forward(
        _p(x), x.stride(0), x.stride(1), B, L, E, n, _ptr_array(weights1), _ptr_array(biases1), _ptr_array(weights2),
        _ptr_array(biases2), (C.c_int * n)(*tails), _ptr_array(outs), _ptr_array(pres), _ptr_array(hiddens),
        *_draw_args(p, seed, instance), _p(state), _p(used), _stream()), 'asac_rows_dense_proj_dropout_forward')


@_profiled
def rows_dense_proj_dropout_backward(grads, pres, tails, weights1, weights2, grad_x, grad_pres, p, seed, instance, used):
    """the backward of `rows_dense_proj_dropout_forward`: grad_pres[j] and grad_x [B][L][E] = sum_j (g_h_j + grad_pres[j] W1_j);
    the masks are regenerated from the counter in `used` (read on the device)"""
    global _last_work
    B, L, E = grad_x.shape
    n = len(grads)
    _dense_f32(*grads, *pres, *weights1, *weights2, grad_x, *grad_pres)
    assert used.is_cuda and used.dtype == torch.int64 and used.numel() == 1
    for g, pr, gp, t in zip(grads, pres, grad_pres, tails):
        assert g.shape == pr.shape == gp.shape == (B, t, E)
    _last_work = 4.0 * B * sum(tails) * E * E
    _check(load().asac_rows_dense_proj_dropout_backward(
        _ptr_array(grads), _ptr_array(pres), (C.c_int * n)(*tails), n, _ptr_array(weights1), _ptr_array(weights2), B, L, E,
        _p(grad_x), _ptr_array(grad_pres), *_draw_args(p, seed, instance), _p(used), _stream()),
        'asac_rows_dense_proj_dropout_backward')


@_profiled
def rows_resblock_dropout_forward(x, weight, bias, row_scale, y, pre, p, seed, instance, state, used):
    """y = (x + gelu(x W^T + b)) * mask * s * row_scale[:, None], pre = x W^T + b; x [rows][E] with feature stride 1"""
    global _last_work
    rows, E = x.shape
    assert x.stride(1) == 1
    _dense_f32(weight, bias, y, pre, *([] if row_scale is None else [row_scale]))
    _drop_state_ok(state, used)
    _last_work = 2.0 * rows * E * E
    _check(load().asac_rows_resblock_dropout_forward(_p(x), x.stride(0), _p(weight), _p(bias), _p(row_scale), rows, E, _p(y),
                                                     _p(pre), *_draw_args(p, seed, instance), _p(state), _p(used), _stream()),
           'asac_rows_resblock_dropout_forward')


@_profiled
def rows_resblock_dropout_backward(grad_y, pre, weight, row_scale, grad_x, grad_pre, p, seed, instance, used):
    global _last_work
    rows, E = grad_y.shape
    _dense_f32(grad_y, pre, weight, grad_x, grad_pre, *([] if row_scale is None else [row_scale]))
    assert used.is_cuda and used.dtype == torch.int64 and used.numel() == 1
    _last_work = 2.0 * rows * E * E
    _check(load().asac_rows_resblock_dropout_backward(_p(grad_y), _p(pre), _p(weight), _p(row_scale), rows, E, _p(grad_x),
                                                      _p(grad_pre), *_draw_args(p, seed, instance), _p(used), _stream()),
           'asac_rows_resblock_dropout_backward')


# ------------------------------------------------------------------------------------------------
# the gate behind an episode attention block, with its padded-row factor (csrc/rows_gate.hip)
# ------------------------------------------------------------------------------------------------
GATE_RESIDUAL, GATE_OUTPUT, GATE_RECURRENT = 1, 2, 3      # (the values of seq_layers.GATE)
_GATE_WEIGHTS = {GATE_RESIDUAL: 0, GATE_OUTPUT: 1, GATE_RECURRENT: 6}
_GATE_SAVED = {GATE_RESIDUAL: 0, GATE_OUTPUT: 1, GATE_RECURRENT: 3}


def rows_gate_supported(kind, width) -> bool:
    return bool(load().asac_rows_gate_supported(int(kind), int(width)))


def _gate_operands(kind, x, y, row_zero, weights):
    B, L, E = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.stride(2) == 1 and y.shape == (B, L, E)
    assert len(weights) == _GATE_WEIGHTS[kind]
    _dense_f32(y, *weights)
    for w in weights:
        assert w.shape == (E, E)
    rz_stride = 0
    if row_zero is not None:
        assert row_zero.is_cuda and row_zero.dtype in (torch.bool, torch.uint8) and row_zero.shape == (B, L)
        assert L == 1 or row_zero.stride(1) == 1
        rz_stride = row_zero.stride(0) if B > 1 else L
    return B, L, E, rz_stride


@_profiled
def rows_gate_forward(kind, x, y, row_zero, weights, bias_z, out, saved):
    """out = gate(x, y) * ~row_zero[..., None] for kind RESIDUAL / OUTPUT / RECURRENT, one launch (formulas: asac_hip.h).
    x [B][L][E] with feature stride 1 (batch / position strides multiples of 4); y, out and the `saved` buffers ([a] /
    [r, z, h]; None: not kept) dense; row_zero bool [B][L] or None; weights [] / [W] / [Wxr, Wyr, Wxz, Wyz, Wxg, Wyg]"""
    global _last_work
    B, L, E, rz_stride = _gate_operands(kind, x, y, row_zero, weights)
    _dense_f32(out, bias_z, *(saved or ()))
    assert out.shape == (B, L, E) and (not saved or len(saved) == _GATE_SAVED[kind])
    _last_work = 2.0 * B * L * E * E * len(weights)
    _check(load().asac_rows_gate_forward(int(kind), _p(x), x.stride(0), x.stride(1), _p(y), _p(row_zero), rz_stride, B, L, E,
                                         _ptr_array(weights) if weights else None, _p(bias_z), _p(out),
                                         _ptr_array(saved) if saved else None, _stream()), 'asac_rows_gate_forward')


@_profiled
def rows_gate_backward(kind, grad_out, x, y, row_zero, weights, saved, grad_x, grad_y, grad_pre, rx=None):
    """the backward of `rows_gate_forward`: grad_x, grad_y (RESIDUAL: may be one tensor), the dense pre-activation gradients
    grad_pre ([grad_a] / [dr_pre, dz_pre, dh_pre]) and, RECURRENT, rx = r * x — the operands of the weight-gradient products"""
    global _last_work
    B, L, E, rz_stride = _gate_operands(kind, x, y, row_zero, weights)
    _dense_f32(grad_out, grad_x, grad_y, rx, *saved, *grad_pre)
    assert grad_out.shape == (B, L, E) and len(saved) == len(grad_pre) == _GATE_SAVED[kind]
    _last_work = 2.0 * B * L * E * E * len(weights)
    _check(load().asac_rows_gate_backward(int(kind), _p(grad_out), _p(x), x.stride(0), x.stride(1), _p(y), _p(row_zero), rz_stride,
                                          B, L, E, _ptr_array(weights) if weights else None,
                                          _ptr_array(saved) if saved else None, _p(grad_x), _p(grad_y),
                                          _ptr_array(grad_pre) if grad_pre else None, _p(rx), _stream()),
           'asac_rows_gate_backward')


# ------------------------------------------------------------------------------------------------
# rotary position encodings: on their own (csrc/rope.hip) and behind the q / k / v projections (csrc/rows_proj.hip)
# ------------------------------------------------------------------------------------------------
ROPE, ROPE2 = 3, 4      # (the values of seq_layers.POSITIONAL_ENCODING)


def rope_supported(kind, width) -> bool:
    return bool(load().asac_rope_supported(int(kind), int(width)))


def _rope_tables(kind, tables, E):
    """(table0, table1, T): ROPE `view_as_real(freqs_cis)` [T][E/2][2]; ROPE2 (`cos_cached`, `sin_cached`) [T][E] each"""
    t0, t1 = tables if kind == ROPE2 else (tables[0], None)
    _dense_f32(t0, t1)
    assert t0.shape[1:] == ((E // 2, 2) if kind == ROPE else (E,)) and (t1 is None or t1.shape == t0.shape)
    return t0, t1, t0.shape[0]


def _rope_index(index, B, L):
    assert index.is_cuda and index.dtype in (torch.int32, torch.int64) and index.shape == (B, L)
    return _p(index), index.stride(0), index.stride(1)


def _rope_launch(fn, what, kind, tables, q, k, q_index, k_index, out_q, out_k):
    B, Lq, E = q.shape
    Lk = k.shape[1]
    assert k.shape == (B, Lk, E) and q.stride(2) == 1 and k.stride(2) == 1 and q.dtype == k.dtype == torch.float32
    assert q_index.dtype == k_index.dtype and out_q.shape == (B, Lq, E) and out_k.shape == (B, Lk, E)
    _dense_f32(out_q, out_k)
    t0, t1, T = _rope_tables(kind, tables, E)
    _check(fn(int(kind), _p(t0), _p(t1), T, E, B, _p(q), q.stride(0), q.stride(1), Lq, *_rope_index(q_index, B, Lq),
              _p(k), k.stride(0), k.stride(1), Lk, *_rope_index(k_index, B, Lk), q_index.element_size(), _p(out_q), _p(out_k),
              _stream()), what)


@_profiled
def rope_forward(kind, tables, q, k, q_index, k_index, out_q, out_k):
    """out_q, out_k (dense) = q [B][Lq][E], k [B][Lk][E] (feature stride 1) rotated by the table rows of their int32 / int64
    indexes [B][L] (any strides; negative: from the table's end), one launch; kind ROPE / ROPE2, `tables` as `_rope_tables`"""
    _rope_launch(load().asac_rope_forward, 'asac_rope_forward', kind, tables, q, k, q_index, k_index, out_q, out_k)


@_profiled
def rope_backward(kind, tables, grad_q, grad_k, q_index, k_index, out_q, out_k):
    """the transpose of `rope_forward`: the gradients of its outputs -> the gradients of its inputs, one launch"""
    _rope_launch(load().asac_rope_backward, 'asac_rope_backward', kind, tables, grad_q, grad_k, q_index, k_index, out_q, out_k)


@_profiled
def rows_proj_rope_forward(kind, tables, index, x, weights, biases, tails, outs):
    """`rows_proj_forward` for the jobs q, k, v with q and k rotated behind it in the same launch; the table row of a position
    comes from `index` [B][L] (the key's: the query's indexes are its newest tails[0] entries).  Same bits as
    `rows_proj_forward` + `rope_forward`"""
    global _last_work
    B, L, E = x.shape
    assert x.stride(2) == 1 and len(weights) == len(biases) == len(tails) == len(outs) == 3
    _dense_f32(*weights, *biases, *outs)
    for o, n in zip(outs, tails):
        assert o.shape == (B, n, E)
    t0, t1, T = _rope_tables(kind, tables, E)
    _last_work = 2.0 * B * sum(tails) * E * E
    _check(load().asac_rows_proj_rope_forward(int(kind), _p(t0), _p(t1), T, *_rope_index(index, B, L), index.element_size(), _p(x),
                                              x.stride(0), x.stride(1), B, L, E, _ptr_array(weights), _ptr_array(biases),
                                              (C.c_int * 3)(*tails), _ptr_array(outs), _stream()), 'asac_rows_proj_rope_forward')


@_profiled
def rows_proj_rope_backward(kind, tables, index, grads, tails, weights, grad_x, grads_unrotated):
    """`rows_proj_backward` of the gradients of the ROTATED q, k and of v: the first two are un-rotated on the way in and written
    to `grads_unrotated` (two dense buffers: the operands of the parameter gradients).  Same bits as `rope_backward` +
    `rows_proj_backward`"""
    global _last_work
    B, L, E = grad_x.shape
    assert len(grads) == len(tails) == len(weights) == 3 and len(grads_unrotated) == 2
    _dense_f32(*grads, *weights, grad_x, *grads_unrotated)
    for g, n in zip(grads, tails):
        assert g.shape == (B, n, E)
    for u, g in zip(grads_unrotated, grads):
        assert u.shape == g.shape
    t0, t1, T = _rope_tables(kind, tables, E)
    _last_work = 2.0 * B * sum(tails) * E * E
    _check(load().asac_rows_proj_rope_backward(int(kind), _p(t0), _p(t1), T, *_rope_index(index, B, L), index.element_size(),
                                               _ptr_array(grads), (C.c_int * 3)(*tails), _ptr_array(weights), B, L, E,
                                               _p(grad_x), _ptr_array(grads_unrotated), _stream()), 'asac_rows_proj_rope_backward')


# ------------------------------------------------------------------------------------------------
# products over the rows of two tall matrices (csrc/xty.hip)
# ------------------------------------------------------------------------------------------------
def xty_supported(rows, M, N) -> bool:
    return bool(load().asac_xty_supported(int(rows), int(M), int(N)))


def rows_wide_supported(R: int, K: int, N: int) -> bool:
    return bool(load().asac_rows_wide_supported(R, K, N))


def rows_wide_workspace(x, N: int) -> torch.Tensor:
    R, K = x.shape
    return torch.empty(int(load().asac_rows_wide_workspace(R, K, N)), dtype=torch.float32, device=x.device)


@_profiled
def rows_wide_forward(x, w, b, y, pre=None, act=True, workspace=None):
    """y [R, N] = act(x W^T + b) for a wide x [R, K] (row stride allowed), W [N, K]; `pre`: the pre-activations (training)"""
    global _last_work
    R, K = x.shape
    N = w.shape[0]
    assert x.stride(1) == 1 and w.is_contiguous() and b.is_contiguous() and y.is_contiguous() and y.shape == (R, N)
    assert pre is None or (pre.is_contiguous() and pre.shape == (R, N))
    _last_work = 2.0 * R * K * N
    ws = rows_wide_workspace(x, N) if workspace is None else workspace
    _check(load().asac_rows_wide_forward(_p(x), x.stride(0), R, K, _p(w), _p(b), N, int(bool(act)), _p(y), _p(pre), _p(ws),
                                         _stream()), 'asac_rows_wide_forward')


@_profiled
def rows_wide_backward_input(grad_y, pre, w, dpre, dx=None, act=True):
    """dpre [R, N] = grad_y * act'(pre); dx [R, K] = dpre W (dx None: dpre only)"""
    global _last_work
    R, N = grad_y.shape
    K = w.shape[1]
    assert grad_y.is_contiguous() and dpre.is_contiguous() and w.is_contiguous() and (pre is None or pre.is_contiguous())
    assert dx is None or (dx.stride(1) == 1 and dx.shape == (R, K))
    _last_work = 2.0 * R * K * N if dx is not None else 0.0
    _check(load().asac_rows_wide_backward_input(_p(grad_y), _p(pre), int(bool(act)), R, K, _p(w), N, _p(dpre), _p(dx),
                                                0 if dx is None else dx.stride(0), _stream()), 'asac_rows_wide_backward_input')


@_profiled
def rows_wide_backward_params(dpre, x, dw, db=None, accumulate=False, workspace=None):
    """dw [N, K] (+)= dpre^T x, db [N] (+)= column sums of dpre"""
    global _last_work
    R, K = x.shape
    N = dpre.shape[1]
    assert dpre.is_contiguous() and x.stride(1) == 1 and dw.is_contiguous() and dw.shape == (N, K)
    assert db is None or (db.is_contiguous() and db.numel() == N)
    _last_work = 2.0 * R * K * N
    ws = rows_wide_workspace(x, N) if workspace is None else workspace
    _check(load().asac_rows_wide_backward_params(_p(dpre), _p(x), x.stride(0), R, K, N, _p(dw), _p(db), int(bool(accumulate)),
                                                 _p(ws), _stream()), 'asac_rows_wide_backward_params')


@_profiled
def xty(x, y, out, colsum_x=None, accumulate=False):
    """out [M, N] (+)= x^T y over the rows of x [R, M] and y [R, N] (row strides allowed, dense last dim);
    colsum_x [M] (+)= the column sums of x"""
    global _last_work
    R, M = x.shape
    N = y.shape[1]
    assert y.shape[0] == R and x.stride(1) == 1 and y.stride(1) == 1 and out.shape == (M, N) and out.is_contiguous()
    assert x.dtype == y.dtype == out.dtype == torch.float32 and x.is_cuda
    _last_work = 2.0 * R * M * N
    ws = torch.empty(int(load().asac_xty_workspace(R, M, N)), dtype=torch.float32, device=x.device)
    if colsum_x is not None:
        assert colsum_x.numel() == M and colsum_x.is_contiguous()
    _check(load().asac_xty(_p(x), x.stride(0), M, _p(y), y.stride(0), N, R, _p(out), _p(colsum_x), int(bool(accumulate)), _p(ws),
                           _stream()), 'asac_xty')


@_profiled
def xty_multi(jobs, accumulate=False):
    """`xty(x, y, out, colsum_x)` for up to 4 jobs [(x, y, out, colsum_x | None), ...] as one launch pair (same values)"""
    global _last_work
    n = len(jobs)
    assert 1 <= n <= 4
    work = 0.0
    for x, y, out, cs in jobs:
        R, M = x.shape
        N = y.shape[1]
        assert y.shape[0] == R and x.stride(1) == 1 and y.stride(1) == 1 and out.shape == (M, N) and out.is_contiguous()
        assert x.dtype == y.dtype == out.dtype == torch.float32 and x.is_cuda
        assert cs is None or (cs.numel() == M and cs.is_contiguous())
        work += 2.0 * R * M * N
    _last_work = work
    i64, i32, ptr = C.c_int64 * n, C.c_int * n, C.c_void_p * n
    rows = i64(*[j[0].shape[0] for j in jobs])
    Ms, Ns = i32(*[j[0].shape[1] for j in jobs]), i32(*[j[1].shape[1] for j in jobs])
    ws = torch.empty(int(load().asac_xty_multi_workspace(n, rows, Ms, Ns)), dtype=torch.float32, device=jobs[0][0].device)
    _check(load().asac_xty_multi(n, ptr(*[j[0].data_ptr() for j in jobs]), i64(*[j[0].stride(0) for j in jobs]), Ms,
                                 ptr(*[j[1].data_ptr() for j in jobs]), i64(*[j[1].stride(0) for j in jobs]), Ns, rows,
                                 ptr(*[j[2].data_ptr() for j in jobs]),
                                 ptr(*[None if j[3] is None else j[3].data_ptr() for j in jobs]), int(bool(accumulate)),
                                 _p(ws), _stream()), 'asac_xty_multi')


# ------------------------------------------------------------------------------------------------
# behaviour cloning (csrc/imitation.hip)
# ------------------------------------------------------------------------------------------------
BC_MAX_ELEMENTS = _defined('BC_MAX_ELEMENTS')


def bc_loss_grad_workspace(device) -> torch.Tensor:
    """the zeroed exchange words of `bc_loss_grad` on `device` (every launch leaves them ready for the next)"""
    return _exchange_words('asac_bc_loss_grad', device)


@_profiled
def bc_loss_grad(loc, scale, action, action_offset, t_valid, entropy_coef, loss_out, dloc, dscale, raw_head=False,
                 workspace=None):
    """loss_out[0] <- mean over rows < t_valid[0] of -Normal(loc, scale).log_prob(action[:, action_offset:]) -
    entropy_coef * entropy, dloc / dscale <- its gradients (zero for the other rows).  loc, scale, dloc, dscale: [Tp, A]
    views with a dense last dimension (loc / scale share a row stride, so do dloc / dscale: the halves of a [Tp, 2A] buffer
    qualify); action [Tp, >= action_offset + A]; t_valid: device int32[1].  `raw_head`: see include/asac_hip.h."""
    Tp, A = loc.shape
    assert scale.shape == (Tp, A) and dloc.shape == (Tp, A) and dscale.shape == (Tp, A) and action.shape[0] == Tp
    assert all(t.dtype == torch.float32 and (t.stride(1) == 1 or A == 1) for t in (loc, scale, dloc, dscale))
    assert action.dim() == 2 and action.dtype == torch.float32 and (action.stride(1) == 1 or action.shape[1] == 1)
    assert action.shape[1] >= action_offset + A and t_valid.dtype == torch.int32 and t_valid.numel() == 1
    assert Tp * A <= BC_MAX_ELEMENTS and loss_out.dtype == torch.float32 and loss_out.numel() == 1

    def ld(a, b, width):      # the common row stride of a pair (a single row has none: any stride >= its width does)
        if Tp == 1:
            return width
        assert a.stride(0) == b.stride(0) >= width
        return a.stride(0)
    ld_in, ld_out = ld(loc, scale, A), ld(dloc, dscale, A)
    a_stride = action.stride(0) if Tp > 1 else action.shape[1]
    ws = workspace if workspace is not None else bc_loss_grad_workspace(loc.device)
    _check(load().asac_bc_loss_grad(_p(loc), _p(scale), ld_in, _p(action), a_stride, int(action_offset), _p(t_valid), Tp, A,
                                    float(entropy_coef), int(bool(raw_head)), _p(loss_out), _p(dloc), _p(dscale), ld_out,
                                    _p(ws), _stream()), 'asac_bc_loss_grad')


# ------------------------------------------------------------------------------------------------
# the option-critic's per-option learner (csrc/option.hip)
# ------------------------------------------------------------------------------------------------
OPTION_MAX_OPTIONS = _defined('OPTION_MAX_OPTIONS')
TERMINATION_MAX_ROWS = _defined('TERMINATION_MAX_ROWS')


@_profiled
def option_return(args: VtraceArgs, beta, v_options):
    """`vtrace_return_min` with the option's termination mix: beta [B, n] and v_options [B, n, O] float32 views (any
    strides); V(s_t+1) = (1 - beta) * (min Q - alpha logpi) + beta * mean_o v_options.  `args` as for `vtrace_return_min`
    (with `q_online` / `td_error_out` set the launch writes the TD error too)."""
    if beta is not None:
        assert beta.dtype == torch.float32 and beta.shape == (args.B, args.n), (tuple(beta.shape), args.B, args.n)
    if v_options is not None:
        assert v_options.dtype == torch.float32 and v_options.dim() == 3 and v_options.shape[:2] == (args.B, args.n)
    bs = (beta.stride(0), beta.stride(1)) if beta is not None else (0, 0)
    vs = tuple(v_options.stride()) if v_options is not None else (0, 0, 0)
    O = v_options.shape[2] if v_options is not None else 0
    _check(load().asac_option_return(C.byref(args), _p(beta), bs[0], bs[1], _p(v_options), vs[0], vs[1], vs[2], O,
                                     _stream()), 'asac_option_return')


def termination_loss_grad_workspace(device) -> torch.Tensor:
    """the zeroed exchange words of `termination_loss_grad` on `device` (every launch leaves them ready for the next)"""
    return _exchange_words('asac_termination_loss_grad', device)


@_profiled
def termination_loss_grad(beta, y, v_options, done, priority_is, terminal_entropy, loss_out, dbeta, workspace=None):
    """loss_out[0] <- mean_b(beta * (y - mean_o v_options + terminal_entropy) * ~done * priority_is), dbeta [B] <- its
    gradient with respect to beta.  beta, y, priority_is (optional): B float32 elements each ([B] or [B, 1], any row
    stride); v_options [B, O] float32 (any strides); done: bool / uint8 [B] contiguous."""
    B = beta.shape[0]

    def col(t, name):
        assert t.dtype == torch.float32 and t.numel() == B and t.shape[0] == B, name
        return t.stride(0) if B > 1 else 1
    assert v_options.dtype == torch.float32 and v_options.dim() == 2 and v_options.shape[0] == B
    assert done.dtype in (torch.bool, torch.uint8) and done.numel() == B and done.is_contiguous()
    assert dbeta.dtype == torch.float32 and dbeta.numel() == B and dbeta.is_contiguous()
    assert loss_out.dtype == torch.float32 and loss_out.numel() == 1 and B <= TERMINATION_MAX_ROWS
    ws = workspace if workspace is not None else termination_loss_grad_workspace(beta.device)
    _check(load().asac_termination_loss_grad(
        _p(beta), col(beta, 'beta'), _p(y), col(y, 'y'), _p(v_options), v_options.stride(0), v_options.stride(1),
        v_options.shape[1], _p(done), _p(priority_is), col(priority_is, 'priority_is') if priority_is is not None else 0,
        float(terminal_entropy), B, _p(loss_out), _p(dbeta), _p(ws), _stream()), 'asac_termination_loss_grad')


# ------------------------------------------------------------------------------------------------
# pure-discrete, policy-based SAC (csrc/discrete.hip)
# ------------------------------------------------------------------------------------------------
def discrete_sizes_ok(d_action_sizes, E: int, n: int, B: int) -> bool:
    """the limits of the `discrete_*` entry points (include/asac_hip.h ASAC_DISCRETE_MAX_*)"""
    sizes = list(d_action_sizes)
    return (0 < len(sizes) <= DISCRETE_MAX_BRANCHES and all(s > 0 for s in sizes) and sum(sizes) <= DISCRETE_MAX_WIDTH
            and 0 < E <= DISCRETE_MAX_MEMBERS and 0 < n <= DISCRETE_MAX_STEPS and 0 < B <= DISCRETE_MAX_ROWS)


def branches(d_action_sizes) -> Branches:
    sizes = [int(s) for s in d_action_sizes]
    br = Branches()
    br.K, br.D = len(sizes), sum(sizes)
    for k, s in enumerate(sizes[:DISCRETE_MAX_BRANCHES]):      # (a longer table is refused by the entry point: K)
        br.size[k] = s
    return br


def members(tensors, D: int) -> Members:
    """the members' head outputs ([B, D] or [B, T, D] float32 each, one shape and one set of strides, dense rows) ->
    `Members`; the tensors must stay alive until the launch that reads the table is issued"""
    m = Members()
    m.E = len(tensors)
    if not tensors:
        return m
    t0 = tensors[0]
    for e, t in enumerate(tensors[:DISCRETE_MAX_MEMBERS]):     # (more members are refused by the entry point: E)
        assert t.is_cuda and t.dtype == torch.float32 and t.shape == t0.shape and t.stride() == t0.stride()
        assert t.shape[-1] == D and (t.stride(-1) == 1 or D == 1) and t.dim() in (2, 3)
        m.base[e] = t.data_ptr()
    m.stride_b = t0.stride(0)
    m.stride_t = t0.stride(1) if t0.dim() == 3 else 0
    return m


def _discrete_rows(t, D, name):
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] >= D and (t.stride(1) == 1 or D == 1), name
    return t.stride(0)


def _discrete_return_job(args: VtraceArgs, br: Branches, q_target, logits, action, q_online) -> DiscreteReturn:
    D, B, n = br.D, args.B, args.n
    job = DiscreteReturn()
    job.branches = br
    job.q_target = members(list(q_target), D)
    assert all(t.shape[:2] == (B, n + 1) for t in q_target)
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.shape == (B, n + 1, D)
    assert logits.stride(2) == 1 or D == 1
    job.logits, job.logits_stride_b, job.logits_stride_t = logits.data_ptr(), logits.stride(0), logits.stride(1)
    if action is not None:
        assert action.is_cuda and action.dtype == torch.float32 and action.dim() == 3 and action.shape[0] == B
        assert action.shape[1] >= n and action.shape[2] >= D and (action.stride(2) == 1 or D == 1)
        job.action, job.action_stride_b, job.action_stride_t = action.data_ptr(), action.stride(0), action.stride(1)
    if q_online is not None:
        job.q_online = members(list(q_online), D)
        assert all(t.shape == (B, D) for t in q_online)
    return job


@_profiled
def discrete_return(args: VtraceArgs, br: Branches, q_target, logits, action=None, q_online=None):
    """`args` (`_vtrace_args` + subset_n / subset_next / E_sample / log_alpha, mu_prob and its strides under importance
    sampling, td_error_out with `q_online`) -> y_out (and the TD error): one launch.  q_target: the target members' head
    outputs [B, n+1, D]; logits [B, n+1, D]; action: the stored window [B, >= n, >= D]; q_online: the online members'
    head outputs [B, D]."""
    job = _discrete_return_job(args, br, q_target, logits, action, q_online)
    _check(load().asac_discrete_return(C.byref(args), C.byref(job), _stream()), 'asac_discrete_return')


@_profiled
def option_discrete_return(args: VtraceArgs, br: Branches, q_target, logits, beta, v_options, action=None, q_online=None):
    """`discrete_return` with the option's arithmetic (csrc/discrete.hip, second instantiation): the minimum over each
    subset instead of the mean, and the termination mix on the next positions' entries, (1 - beta) * (min Q - alpha
    log p) + beta * mean_o v_options.  beta [B, n] and v_options [B, n, O] float32 views (any strides); everything else
    as for `discrete_return`."""
    job = _discrete_return_job(args, br, q_target, logits, action, q_online)
    if beta is not None:
        assert beta.is_cuda and beta.dtype == torch.float32 and beta.shape == (args.B, args.n)
    if v_options is not None:
        assert v_options.is_cuda and v_options.dtype == torch.float32 and v_options.dim() == 3
        assert v_options.shape[:2] == (args.B, args.n)
    bs = (beta.stride(0), beta.stride(1)) if beta is not None else (0, 0)
    vs = tuple(v_options.stride()) if v_options is not None else (0, 0, 0)
    O = v_options.shape[2] if v_options is not None else 0
    _check(load().asac_option_discrete_return(C.byref(args), C.byref(job), _p(beta), bs[0], bs[1], _p(v_options), vs[0],
                                              vs[1], vs[2], O, _stream()), 'asac_option_discrete_return')


@_profiled
def discrete_q_loss_grad(br: Branches, q, action, y, w, loss_out, grad_q):
    """q: the online members' head outputs [B, D]; action [B, >= D]; y, w (optional): B float32 elements each ([B] or
    [B, 1]); loss_out [E]; grad_q [E, B, D] contiguous <- d (sum_e loss_e) / d q"""
    B, D, E = action.shape[0], br.D, len(q)

    def col(t, name):
        assert t.is_cuda and t.dtype == torch.float32 and t.numel() == B and t.shape[0] == B, name
        return t.stride(0) if B > 1 else 1
    if loss_out is not None and grad_q is not None:
        assert loss_out.dtype == torch.float32 and loss_out.numel() >= E and loss_out.is_contiguous()
        assert grad_q.dtype == torch.float32 and grad_q.shape == (E, B, D) and grad_q.is_contiguous()
    _check(load().asac_discrete_q_loss_grad(C.byref(br), C.byref(members(list(q), D)), _p(action),
                                            _discrete_rows(action, D, 'action'),
                                            _p(y), col(y, 'y'), _p(w), col(w, 'w') if w is not None else 0, B,
                                            _p(loss_out), _p(grad_q), _stream()), 'asac_discrete_q_loss_grad')


@_profiled
def discrete_policy_loss_grad(br: Branches, logits, q, subset, E_sample, mu, log_alpha, entropy_penalty, loss_out,
                              grad_logits, entropy_out, probs_out=None, row_entropy_out=None):
    """logits [B, D]; q: the online members' head outputs [B, D]; subset: int32 [E_sample] device tensor or None (members
    0..E_sample-1); mu [B, >= D]; -> loss_out [1], grad_logits [B, D], entropy_out [1] (and, optionally, p [B, D]
    contiguous and the rows' entropies [B])"""
    B, D = logits.shape[0], br.D
    for t in (probs_out, row_entropy_out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == (B * D if t is probs_out else B))
    gs = _discrete_rows(grad_logits, D, 'grad_logits') if grad_logits is not None else 0
    _check(load().asac_discrete_policy_loss_grad(
        C.byref(br), _p(logits), _discrete_rows(logits, D, 'logits'), C.byref(members(list(q), D)), _p(subset), int(E_sample),
        _p(mu), _discrete_rows(mu, D, 'mu'), _p(log_alpha), float(entropy_penalty), B, _p(loss_out), _p(grad_logits), gs,
        _p(entropy_out), _p(probs_out), _p(row_entropy_out), _stream()), 'asac_discrete_policy_loss_grad')


@_profiled
def discrete_alpha_grad(br: Branches, logits, target, grad_slot, probs_out=None, row_entropy_out=None):
    """*grad_slot <- mean_b (1/K) sum_j p_j (-cl(p_j) - target_j); logits [B, D], target [D] (device)"""
    B, D = logits.shape[0], br.D
    assert target.is_cuda and target.dtype == torch.float32 and target.numel() == D and target.is_contiguous()
    for t in (probs_out, row_entropy_out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == (B * D if t is probs_out else B))
    _check(load().asac_discrete_alpha_grad(C.byref(br), _p(logits), _discrete_rows(logits, D, 'logits'), _p(target), B,
                                           _p(grad_slot), _p(probs_out), _p(row_entropy_out), _stream()),
           'asac_discrete_alpha_grad')


# ------------------------------------------------------------------------------------------------
# hybrid action spaces, policy-based SAC (csrc/hybrid.hip)
# ------------------------------------------------------------------------------------------------
MAX_ACTION = _defined('MAX_ACTION')


def hybrid_sizes_ok(d_action_sizes, c_action_size: int, E: int, n: int, B: int) -> bool:
    """the limits of the `hybrid_*` entry points: those of the `discrete_*` ones and 1 <= A <= ASAC_MAX_ACTION"""
    return discrete_sizes_ok(d_action_sizes, E, n, B) and 0 < c_action_size <= MAX_ACTION


def _ensemble_rows(t, E, B, name):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == E * B and t.shape[0] == E, name


@_profiled
def hybrid_return(d_args: VtraceArgs, c_args: VtraceArgs, br: Branches, q_target, logits, action=None, q_online=None,
                  c_q_online=None, td_out=None):
    """Both returns of a hybrid space in one launch.  `d_args`: what `discrete_return` takes; `c_args`: what
    `vtrace_return_min` takes (`A` set with and without importance sampling); they share reward, masks and ratios and
    write different `y_out`.  q_target / logits / action / q_online: the discrete side's, as for `discrete_return`.  With
    `td_out` [B] (then `q_online` [B, D] each and `c_q_online` [E, B] contiguous) the launch also writes
    mean_e (|(1/K) sum_j a_j q_e - d_y| + |c_q_e - c_y|)."""
    job = _discrete_return_job(d_args, br, q_target, logits, action, q_online)
    if td_out is not None:
        E = len(q_online)
        _ensemble_rows(c_q_online, E, d_args.B, 'c_q_online')
        assert td_out.dtype == torch.float32 and td_out.is_contiguous() and td_out.numel() == d_args.B
        c_args.q_online, c_args.E_online = c_q_online.data_ptr(), E
    _check(load().asac_hybrid_return(C.byref(d_args), C.byref(c_args), C.byref(job), _p(td_out), _stream()),
           'asac_hybrid_return')


@_profiled
def hybrid_q_loss_grad(br: Branches, q_d, action, c_q, t_q, d_y, c_y, w, clip_eps, loss_out, grad_qd, grad_cq):
    """q_d: the online members' discrete head outputs [B, D]; action [B, >= D]; c_q, t_q [E, B] contiguous; d_y, c_y, w
    (optional): B float32 elements each ([B] or [B, 1]); -> loss_out [E], grad_qd [E, B, D] and grad_cq [E, B] contiguous
    <- d (sum_e loss_e) / d (head outputs, continuous values)"""
    B, D, E = action.shape[0], br.D, len(q_d)

    def col(t, name):
        assert t.is_cuda and t.dtype == torch.float32 and t.numel() == B and t.shape[0] == B, name
        return t.stride(0) if B > 1 else 1
    _ensemble_rows(c_q, E, B, 'c_q'), _ensemble_rows(t_q, E, B, 't_q'), _ensemble_rows(grad_cq, E, B, 'grad_cq')
    assert loss_out.dtype == torch.float32 and loss_out.numel() >= E and loss_out.is_contiguous()
    assert grad_qd.dtype == torch.float32 and grad_qd.shape == (E, B, D) and grad_qd.is_contiguous()
    _check(load().asac_hybrid_q_loss_grad(
        C.byref(br), C.byref(members(list(q_d), D)), _p(action), _discrete_rows(action, D, 'action'), _p(c_q), _p(t_q),
        _p(d_y), col(d_y, 'd_y'), _p(c_y), col(c_y, 'c_y'), _p(w), col(w, 'w') if w is not None else 0, B, float(clip_eps),
        _p(loss_out), _p(grad_qd), _p(grad_cq), _stream()), 'asac_hybrid_q_loss_grad')


@_profiled
def hybrid_policy_loss_grad(br: Branches, logits, q_d, subset_d, mu, log_d_alpha, entropy_penalty, logp, c_q, subset_c,
                            E_sample, log_c_alpha, scale, loss_out, grad_logits, grad_logp, grad_cq, d_entropy_out,
                            c_entropy_out):
    """logits [B, D]; q_d: the online members' discrete head outputs [B, D]; mu [B, >= D]; logp [B] and c_q [E, B]
    contiguous; scale [B, A]; subset_d / subset_c: int32 [E_sample] device tensors or None (members 0..E_sample-1); ->
    loss_out [1], grad_logits [B, D], grad_logp [B], grad_cq [E, B], d_entropy_out [1], c_entropy_out [1]"""
    B, D, E = logits.shape[0], br.D, len(q_d)
    _ensemble_rows(c_q, E, B, 'c_q'), _ensemble_rows(grad_cq, E, B, 'grad_cq')
    for t in (logp, grad_logp):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == B
    assert scale.is_cuda and scale.dtype == torch.float32 and scale.dim() == 2 and scale.shape[0] == B
    A = scale.shape[1]
    assert scale.stride(1) == 1 or A == 1
    _check(load().asac_hybrid_policy_loss_grad(
        C.byref(br), _p(logits), _discrete_rows(logits, D, 'logits'), C.byref(members(list(q_d), D)), _p(subset_d), _p(mu),
        _discrete_rows(mu, D, 'mu'), _p(log_d_alpha), float(entropy_penalty), _p(logp), _p(c_q), _p(subset_c),
        int(E_sample), _p(log_c_alpha), _p(scale), max(scale.stride(0), A), A, B, _p(loss_out), _p(grad_logits),
        _discrete_rows(grad_logits, D, 'grad_logits'), _p(grad_logp), _p(grad_cq), _p(d_entropy_out), _p(c_entropy_out),
        _stream()), 'asac_hybrid_policy_loss_grad')


@_profiled
def hybrid_alpha_grad(br: Branches, logits, target_d, logp, target_c, grad_slots):
    """grad_slots [2] <- (mean_b (1/K) sum_j p_j (-cl(p_j) - target_d_j), mean_b(-logp_b) - target_c): the flat-gradient
    elements of [log_d_alpha, log_c_alpha]; logits [B, D], target_d [D] (device), logp [B] contiguous"""
    B, D = logits.shape[0], br.D
    assert target_d.is_cuda and target_d.dtype == torch.float32 and target_d.numel() == D and target_d.is_contiguous()
    assert logp.is_cuda and logp.dtype == torch.float32 and logp.is_contiguous() and logp.numel() == B
    assert grad_slots.dtype == torch.float32 and grad_slots.is_contiguous() and grad_slots.numel() == 2
    _check(load().asac_hybrid_alpha_grad(C.byref(br), _p(logits), _discrete_rows(logits, D, 'logits'), _p(target_d),
                                         _p(logp), float(target_c), B, _p(grad_slots), _stream()),
           'asac_hybrid_alpha_grad')


# ------------------------------------------------------------------------------------------------
# pure-discrete, DQN-like learner (csrc/dqn.hip)
# ------------------------------------------------------------------------------------------------
def dqn_job(br: Branches, q_eval, q_target, action=None, q_online=None) -> DqnJob:
    """q_eval: the online members' head outputs over the NEXT positions [B, n, D]; q_target: the target members' head
    outputs [B, n+1, D] (as many); action: the stored action at the step's state [B, >= D]; q_online: the online members'
    head outputs [B, D] there.  The tensors must stay alive until the launch that reads the job is issued."""
    D = br.D
    job = DqnJob()
    job.branches = br
    job.q_eval, job.q_target = members(list(q_eval), D), members(list(q_target), D)
    B, n = q_eval[0].shape[0], q_eval[0].shape[1]
    assert all(t.shape[:2] == (B, n) for t in q_eval) and all(t.shape[:2] == (B, n + 1) for t in q_target)
    if action is not None:
        assert action.shape[0] == B
        job.action, job.action_stride = action.data_ptr(), _discrete_rows(action, D, 'action')
    if q_online is not None:
        job.q_online = members(list(q_online), D)
        assert all(t.shape == (B, D) for t in q_online)
    return job


@_profiled
def dqn_return(args: VtraceArgs, job: DqnJob):
    """`args` (`_vtrace_args` + subset_n = the eval subset / subset_next = the target subset / E_sample; td_error_out with
    the job's `q_online` and `action`) -> y_out (and the TD error): one launch"""
    _check(load().asac_dqn_return(C.byref(args), C.byref(job), _stream()), 'asac_dqn_return')


@_profiled
def dqn_q_loss_grad(args: VtraceArgs, job: DqnJob, w, loss_out, grad_q):
    """The Q step's loss launch, forming the target itself: `job` with `q_online` and `action`; w (optional): B float32
    elements ([B] or [B, 1]); loss_out [E]; grad_q [E, B, D] contiguous <- d (sum_e loss_e) / d q; `args.y_out`
    (optional) <- y"""
    B, D, E = args.B, job.branches.D, job.q_online.E
    ws = 0
    if w is not None:
        assert w.is_cuda and w.dtype == torch.float32 and w.numel() == B and w.shape[0] == B, 'w'
        ws = w.stride(0) if B > 1 else 1
    if loss_out is not None and grad_q is not None:
        assert loss_out.dtype == torch.float32 and loss_out.numel() >= E and loss_out.is_contiguous()
        assert grad_q.dtype == torch.float32 and grad_q.shape == (E, B, D) and grad_q.is_contiguous()
    _check(load().asac_dqn_q_loss_grad(C.byref(args), C.byref(job), _p(w), ws, _p(loss_out), _p(grad_q), _stream()),
           'asac_dqn_q_loss_grad')


@_profiled
def dqn_act(br: Branches, q, u, epsilon: float, action_out):
    """q: the first critic's head outputs [B, D]; u: [B, 1 + K] uniforms in [0, 1) or None (greedy only);
    action_out [B, >= D] <- the one-hot action per branch: one launch"""
    B, D = q.shape[0], br.D
    us = 0
    if u is not None:
        assert u.is_cuda and u.dtype == torch.float32 and u.shape == (B, 1 + br.K) and u.stride(1) == 1, 'u'
        us = u.stride(0)
    assert action_out.shape[0] == B
    _check(load().asac_dqn_act(C.byref(br), _p(q), _discrete_rows(q, D, 'q'), _p(u), us, float(epsilon), _p(action_out),
                               _discrete_rows(action_out, D, 'action_out'), B, _stream()), 'asac_dqn_act')


# ------------------------------------------------------------------------------------------------
# acting of a policy-based learner (csrc/act.hip)
# ------------------------------------------------------------------------------------------------
def act_sizes_ok(d_action_sizes, c_action_size: int) -> bool:
    """the limits of `act_policy` (include/asac_hip.h: K <= 8, D <= 64, A <= ASAC_ACT_MAX_CONT, at least one part present):
    what `asac_act_sizes_ok` answers, decided on the host (it is asked once per environment step)"""
    sizes, A = list(d_action_sizes), int(c_action_size)
    if sizes and not (len(sizes) <= DISCRETE_MAX_BRANCHES and all(s > 0 for s in sizes) and sum(sizes) <= DISCRETE_MAX_WIDTH):
        return False
    return 0 <= A <= ACT_MAX_CONT and (bool(sizes) or A > 0)


def act_draw_columns(K: int, A: int, deterministic: bool, use_noise: bool):
    """-> (columns of `u`, columns of `eps`) of `act_policy` (the layout of include/asac_hip.h):
    u   = [K sampling columns: not deterministic] [1 gate column, K index columns: use_noise], none without branches;
    eps = [A sampling columns: not deterministic] [A noise columns: use_noise]"""
    nu = ((0 if deterministic else K) + ((1 + K) if use_noise else 0)) if K else 0
    ne = (0 if deterministic else A) + (A if use_noise else 0)
    return nu, ne


def act_job(br, logits, loc, scale, u, eps, action_out, prob_out, *, head_raw=False, deterministic=False,
            action_noise=None) -> ActJob:
    """The arguments of `act_policy`.  br: `Branches` or None (no discrete part) with logits [B, D]; loc, scale: [B, A]
    views of one row stride (the two halves of a [B, 2A] row) or None (no continuous part), with `head_raw` the stock
    policy's (mean, logstd) before the bounding; u / eps: the draws in the column layout of `act_draw_columns` (None where
    that is no column); action_noise: None or (lo, hi); action_out, prob_out: [B, D + A].  The tensors must stay alive
    until the launch is issued."""
    K, D = (br.K, br.D) if br is not None else (0, 0)
    A = loc.shape[1] if loc is not None else 0
    B = action_out.shape[0]
    job = ActJob()
    if K:
        assert logits.shape[0] == B
        job.branches = br
        job.logits, job.logits_stride = logits.data_ptr(), _discrete_rows(logits, D, 'logits')
    if A:
        for t, name in ((loc, 'loc'), (scale, 'scale')):
            assert t.is_cuda and t.dtype == torch.float32 and t.shape == (B, A) and (t.stride(1) == 1 or A == 1), name
        assert B <= 1 or loc.stride(0) == scale.stride(0), 'loc and scale rows at one stride'
        job.loc, job.scale, job.ls_row_stride = loc.data_ptr(), scale.data_ptr(), loc.stride(0)
    job.A, job.head_raw, job.deterministic = A, int(bool(head_raw)), int(bool(deterministic))
    if action_noise is not None:
        job.use_noise, job.noise_lo, job.noise_hi = 1, float(action_noise[0]), float(action_noise[1])
    nu, ne = act_draw_columns(K, A, bool(deterministic), action_noise is not None)
    for t, n, name in ((u, nu, 'u'), (eps, ne, 'eps')):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.shape == (B, n) and (t.stride(1) == 1 or n == 1)), name
    if u is not None and nu:
        job.u, job.u_stride = u.data_ptr(), u.stride(0)
    if eps is not None and ne:
        job.eps, job.eps_stride = eps.data_ptr(), eps.stride(0)
    assert prob_out.shape[0] == B
    job.action_out, job.action_stride = action_out.data_ptr(), _discrete_rows(action_out, D + A, 'action_out')
    job.prob_out, job.prob_stride = prob_out.data_ptr(), _discrete_rows(prob_out, D + A, 'prob_out')
    job.B = B
    return job


@_profiled
def act_policy(job: ActJob):
    """One launch: the policy's head outputs and the draws -> (action, prob) (`act_job`)"""
    _check(load().asac_act_policy(C.byref(job), _stream()), 'asac_act_policy')


# ------------------------------------------------------------------------------------------------
# random network distillation, continuous actions (csrc/rnd.hip)
# ------------------------------------------------------------------------------------------------
RND_WIDTH, RND_MAX_IN, RND_MAX_SAMPLES, RND_MAX_ROWS = _defined('RND_WIDTH', 'RND_MAX_IN', 'RND_MAX_SAMPLES', 'RND_MAX_ROWS')


def rnd_sizes_ok(S: int, A: int, k: int = 1, rows: int = 1) -> bool:
    """the limits of the `rnd_*` entry points (include/asac_hip.h ASAC_RND_*): k candidates per entry, `rows` = B * n"""
    return bool(load().asac_rnd_supported(int(S), int(A), int(k))) and 0 <= rows <= RND_MAX_ROWS


def rnd_desc(S: int, A: int, residual=(False, True)) -> RndDesc:
    d = RndDesc()
    d.S, d.A = int(S), int(A)
    d.residual[0], d.residual[1] = int(bool(residual[0])), int(bool(residual[1]))
    return d


def rnd_stack(w1, b1, w2, b2) -> RndStack:
    """the parameters of one stack (float32 device tensors, each contiguous; nn.Linear layout) -> `RndStack`; the tensors
    must stay alive until the launch that reads the table is issued"""
    for t in (w1, b1, w2, b2):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert w1.shape[0] == RND_WIDTH and w2.shape == (RND_WIDTH, RND_WIDTH) and b1.numel() == b2.numel() == RND_WIDTH
    s = RndStack()
    s.w1, s.b1, s.w2, s.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    return s


def rnd_distill_workspace_floats(rows: int) -> int:
    """floats of a caller-owned workspace of `rnd_distill` over `rows` rows (zero before the first launch)"""
    return int(load().asac_rnd_distill_workspace(int(rows)))


def rnd_distill_workspace(device, rows: int) -> torch.Tensor:
    """the zeroed exchange words of `rnd_distill` over `rows` rows on `device` (every launch leaves them ready for the next)"""
    return _exchange_words('asac_rnd_distill', device, int(rows))


@_profiled
def rnd_distill(desc: RndDesc, predictor: RndStack, target: RndStack, state, action, padding_mask, x_cat, h1, gz1, gz2,
                loss_out, workspace=None):
    """state [B, n, S] and action [B, n, A]: float32 views with a dense last dim (any batch / time strides); padding_mask
    [B, n] (one byte an element, any strides) or None -> x_cat [B * n, S + A], h1 / gz1 / gz2 [B * n, 64] (contiguous) and
    the masked mean squared distillation error in loss_out: one launch (the weight gradients: `xty_multi` on these buffers)"""
    B, n, S = state.shape
    A = action.shape[2]
    N = B * n
    ps, s_sb, s_st = _window3(state)
    pa, a_sb, a_st = _window3(action)
    assert action.shape[:2] == (B, n) and (S, A) == (desc.S, desc.A)
    pm, m_sb, m_st = None, 0, 0
    if padding_mask is not None:
        assert padding_mask.shape == (B, n) and padding_mask.element_size() == 1 and padding_mask.is_cuda
        pm, m_sb, m_st = _p(padding_mask), padding_mask.stride(0), padding_mask.stride(1)
    for t, width in ((x_cat, S + A), (h1, RND_WIDTH), (gz1, RND_WIDTH), (gz2, RND_WIDTH)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N * width
    assert loss_out.is_cuda and loss_out.dtype == torch.float32 and loss_out.numel() == 1
    ws = workspace if workspace is not None else (rnd_distill_workspace(state.device, N) if 0 < N <= RND_MAX_ROWS else loss_out)
    _check(load().asac_rnd_distill(C.byref(desc), C.byref(predictor), C.byref(target), ps, s_sb, s_st, pa, a_sb, a_st, pm, m_sb,
                                   m_st, B, n, _p(x_cat), _p(h1), _p(gz1), _p(gz2), _p(loss_out), _p(ws), _stream()),
           'asac_rnd_distill')


@_profiled
def rnd_pick(desc: RndDesc, predictor: RndStack, target: RndStack, state, loc, scale, eps, action_out, prob_out,
             err_out=None, index_out=None):
    """state [batch, S]; loc / scale [batch, A] with one row stride (the halves of the policy's [batch, 2A] output); eps
    [batch, k, A] contiguous -> action_out [batch, A] <- the candidate tanh(loc + scale * eps_j) of the largest distillation
    error, prob_out [batch, A] <- its squash-corrected density; optionally err_out [batch, k] and index_out [batch] (int32):
    one launch"""
    batch, k, A = eps.shape
    S = state.shape[1]
    assert (S, A) == (desc.S, desc.A) and state.shape[0] == batch and loc.shape == scale.shape == (batch, A)
    for t in (state, loc, scale):
        assert t.is_cuda and t.dtype == torch.float32 and (t.stride(1) == 1 or t.shape[1] == 1)
    assert loc.stride(0) == scale.stride(0) or batch <= 1
    assert eps.is_cuda and eps.dtype == torch.float32 and eps.is_contiguous()
    for t in (action_out, prob_out):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (batch, A)
    if err_out is not None:
        assert err_out.is_cuda and err_out.dtype == torch.float32 and err_out.is_contiguous() and err_out.shape == (batch, k)
    if index_out is not None:
        assert index_out.is_cuda and index_out.dtype == torch.int32 and index_out.is_contiguous() and index_out.numel() == batch
    _check(load().asac_rnd_pick(C.byref(desc), C.byref(predictor), C.byref(target), _p(state), state.stride(0), _p(loc),
                                _p(scale), loc.stride(0), _p(eps), k, batch, _p(action_out), _p(prob_out), _p(err_out),
                                _p(index_out), _stream()), 'asac_rnd_pick')


# ------------------------------------------------------------------------------------------------
# random network distillation, pure-discrete policy-based learner (csrc/drnd.hip)
# ------------------------------------------------------------------------------------------------
DRND_MAX_MEMBERS = _defined('DRND_MAX_MEMBERS')


def drnd_sizes_ok(S: int, d_action_sizes, k: int = 1, rows: int = 1) -> bool:
    """the limits of the `drnd_*` entry points (include/asac_hip.h): S, D = sum of the branch sizes, K branches, k candidates
    per entry, `rows` = B * n"""
    sizes = [int(s) for s in d_action_sizes]
    return (len(sizes) > 0 and all(s > 0 for s in sizes)
            and bool(load().asac_drnd_supported(int(S), sum(sizes), len(sizes), int(k))) and 0 <= rows <= RND_MAX_ROWS)


def drnd_table(members, device=None) -> torch.Tensor:
    """the members' tensors ((w1, b1, w2, b2) each: parameters, or their gradient views) -> the DEVICE table the `drnd_*`
    launches read (`asac_rnd_stack_t` / `asac_rnd_grads_t` x D, int64 [D, 4]).  Every tensor is float32, contiguous, on the
    device and 16-byte aligned (the entry points cannot see the members: this is their check); the tensors must stay alive
    and keep their addresses as long as the table is used."""
    members = [tuple(m) for m in members]
    if not 0 < len(members) <= DRND_MAX_MEMBERS:
        raise AsacNativeError(f'drnd_table: {len(members)} members (1..{DRND_MAX_MEMBERS})')
    for w1, b1, w2, b2 in members:
        for t in (w1, b1, w2, b2):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0):
                raise AsacNativeError('drnd_table: a member tensor is not a contiguous, 16-byte-aligned float32 device tensor')
        if not (w1.shape[0] == RND_WIDTH and tuple(w2.shape) == (RND_WIDTH, RND_WIDTH)
                and b1.numel() == b2.numel() == RND_WIDTH and w1.shape[1] == members[0][0].shape[1]):
            raise AsacNativeError('drnd_table: a member is not a  S -> 64 -> 64  stack')
    dev = members[0][0].device if device is None else device
    return torch.tensor([[t.data_ptr() for t in m] for m in members], dtype=torch.int64).to(dev)


def _table_p(table, struct):
    """a `drnd_table` (or None) as the pointer to device `struct`s its entry points declare"""
    return C.cast(_p(table), C.POINTER(struct))


def _residual2(residual):
    return (C.c_int32 * 2)(int(bool(residual[0])), int(bool(residual[1])))


def drnd_distill_workspace_floats(rows: int) -> int:
    return int(load().asac_drnd_distill_workspace(int(rows)))


def drnd_param_grads_workspace_floats(rows: int, S: int, D: int) -> int:
    return int(load().asac_drnd_param_grads_workspace(int(rows), int(S), int(D)))


def drnd_distill_workspace(device, rows: int) -> torch.Tensor:
    """the zeroed exchange words of `drnd_distill` over `rows` rows on `device` (every launch leaves them ready for the next)"""
    return _exchange_words('asac_drnd_distill', device, int(rows))


def drnd_param_grads_workspace(device, rows: int, S: int, D: int) -> torch.Tensor:
    return _exchange_words('asac_drnd_param_grads', device, int(rows), int(S), int(D))


@_profiled
def drnd_distill(br: Branches, residual, predictors, targets, state, action, padding_mask, sel, x, h1, gz1, gz2, loss_out,
                 workspace=None):
    """state [B, n, S] and action [B, n, >= D]: float32 views with a dense last dim (any batch / time strides); padding_mask
    [B, n] (one byte an element) or None; predictors / targets: `drnd_table`s of the D members -> sel int32 [B * n, K], the
    records h1 / gz1 / gz2 [B * n, K, 64], x [B * n, S] (contiguous) and the masked mean squared distillation error in
    loss_out: one launch (the parameter gradients: `drnd_param_grads` on these buffers)"""
    B, n, S = state.shape
    N, K, D = B * n, br.K, br.D
    ps, s_sb, s_st = _window3(state)
    pa, a_sb, a_st = _window3(action)
    assert action.shape[:2] == (B, n) and action.shape[2] >= D
    pm, m_sb, m_st = None, 0, 0
    if padding_mask is not None:
        assert padding_mask.shape == (B, n) and padding_mask.element_size() == 1 and padding_mask.is_cuda
        pm, m_sb, m_st = _p(padding_mask), padding_mask.stride(0), padding_mask.stride(1)
    for t, width in ((x, S), (h1, K * RND_WIDTH), (gz1, K * RND_WIDTH), (gz2, K * RND_WIDTH)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N * width
    assert sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == N * K
    assert loss_out.is_cuda and loss_out.dtype == torch.float32 and loss_out.numel() == 1
    for tab in (predictors, targets):
        assert tab is None or (tab.is_cuda and tab.dtype == torch.int64 and tab.is_contiguous() and tab.shape == (D, 4))
    ws = workspace if workspace is not None else (drnd_distill_workspace(state.device, N) if 0 < N <= RND_MAX_ROWS else loss_out)
    _check(load().asac_drnd_distill(C.byref(br), S, _residual2(residual), _table_p(predictors, RndStack),
                                    _table_p(targets, RndStack), ps, s_sb, s_st, pa, a_sb, a_st, pm, m_sb, m_st, B, n, _p(sel),
                                    _p(x), _p(h1), _p(gz1), _p(gz2), _p(loss_out), _p(ws), _stream()), 'asac_drnd_distill')


@_profiled
def drnd_param_grads(br: Branches, S: int, sel, x, h1, gz1, gz2, grads, workspace=None):
    """the records of `drnd_distill` -> every element of the D members' gradient views (`grads`: the `drnd_table` of
    (w1.grad, b1.grad, w2.grad, b2.grad) per member), rows in ascending order: one launch"""
    N, K, D = sel.numel() // br.K, br.K, br.D
    for t, width in ((x, S), (h1, K * RND_WIDTH), (gz1, K * RND_WIDTH), (gz2, K * RND_WIDTH)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N * width
    assert sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous()
    assert grads is None or (grads.is_cuda and grads.dtype == torch.int64 and grads.is_contiguous() and grads.shape == (D, 4))
    ws = workspace if workspace is not None else (drnd_param_grads_workspace(x.device, N, S, D) if 0 < N <= RND_MAX_ROWS else x)
    _check(load().asac_drnd_param_grads(C.byref(br), int(S), _p(sel), _p(x), _p(h1), _p(gz1), _p(gz2), N,
                                        _table_p(grads, RndGrads), _p(ws), _stream()), 'asac_drnd_param_grads')


@_profiled
def drnd_pick(br: Branches, residual, predictors, targets, state, logits, u, action_out, prob_out, err_out=None,
              cand_out=None, index_out=None):
    """state [batch, S]; logits [batch, D] (the policy's branch head outputs); u [batch, k, K] contiguous uniforms in [0, 1)
    -> action_out [batch, D] <- the one-hot candidate of the largest distillation error, prob_out [batch, D] <- the branch
    softmax; optionally err_out [batch, k], cand_out [batch, k, K] (int32) and index_out [batch] (int32): one launch"""
    batch, k, K = u.shape
    S, D = state.shape[1], br.D
    assert K == br.K and state.shape[0] == batch and logits.shape == (batch, D)
    for t in (state, logits):
        assert t.is_cuda and t.dtype == torch.float32 and (t.stride(1) == 1 or t.shape[1] == 1)
    assert u.is_cuda and u.dtype == torch.float32 and u.is_contiguous()
    for t in (action_out, prob_out):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (batch, D)
    if err_out is not None:
        assert err_out.is_cuda and err_out.dtype == torch.float32 and err_out.is_contiguous() and err_out.shape == (batch, k)
    if cand_out is not None:
        assert cand_out.is_cuda and cand_out.dtype == torch.int32 and cand_out.is_contiguous() and cand_out.shape == (batch, k, K)
    if index_out is not None:
        assert index_out.is_cuda and index_out.dtype == torch.int32 and index_out.is_contiguous() and index_out.numel() == batch
    for tab in (predictors, targets):
        assert tab is None or (tab.is_cuda and tab.dtype == torch.int64 and tab.is_contiguous() and tab.shape == (D, 4))
    _check(load().asac_drnd_pick(C.byref(br), S, _residual2(residual), _table_p(predictors, RndStack),
                                 _table_p(targets, RndStack), _p(state), state.stride(0), _p(logits), logits.stride(0), _p(u), k,
                                 batch, _p(action_out), _p(prob_out), _p(err_out), _p(cand_out), _p(index_out), _stream()),
           'asac_drnd_pick')


# ------------------------------------------------------------------------------------------------
# siamese representation losses (csrc/siamese.hip)
# ------------------------------------------------------------------------------------------------
SIAMESE_MAX_WIDTH, SIAMESE_MAX_BLOCK, SIAMESE_MAX_ROWS = _defined('SIAMESE_MAX_WIDTH', 'SIAMESE_MAX_BLOCK', 'SIAMESE_MAX_ROWS')
SIAMESE_BYOL_MAX_WIDTH, SIAMESE_BYOL_MAX_ROWS, SIAMESE_BYOL_WORKSPACE_FLOATS = _defined(
    'SIAMESE_BYOL_MAX_WIDTH', 'SIAMESE_BYOL_MAX_ROWS', 'SIAMESE_BYOL_WORKSPACE_FLOATS')


def siamese_atc_workspace_floats(N: int, E: int) -> int:
    """floats of the caller-owned workspace of `siamese_atc_loss_grad` (zero before the first launch); -1 outside the limits"""
    return int(load().asac_siamese_atc_workspace_floats(int(N), int(E)))


def _dense_rows(t, rows, width):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == rows * width


@_profiled
def siamese_atc_loss_grad(e, te, w, pad, n, loss_out, g_e, g_w, workspace):
    """e / te [N, E], w [E, E], pad [N] float row weights, n the block length -> loss_out (one float) <- the mean over the
    N x N logits (e w) te^T of pad_i * BCE-with-logits against the block-diagonal labels, g_e [N, E] and g_w [E, E] <- its
    gradients: one launch, no N x N buffer.  workspace: `siamese_atc_workspace_floats(N, E)` zeroed floats, kept by the caller"""
    N, E = e.shape
    assert _dense_rows(e, N, E) and _dense_rows(te, N, E) and _dense_rows(w, E, E) and _dense_rows(pad, N, 1)
    assert _dense_rows(g_e, N, E) and _dense_rows(g_w, E, E) and _dense_rows(loss_out, 1, 1)
    assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous()
    assert workspace.numel() >= max(1, siamese_atc_workspace_floats(N, E))
    _check(load().asac_siamese_atc_loss_grad(_p(e), _p(te), _p(w), _p(pad), N, E, int(n), _p(loss_out), _p(g_e), _p(g_w),
                                             _p(workspace), _stream()), 'asac_siamese_atc_loss_grad')


@_profiled
def siamese_byol_loss_grad(pred, t_proj, pad, loss_out, g_pred, workspace):
    """pred / t_proj [N, P], pad [N] float row weights -> loss_out (one float) <- mean_i(pad_i * cosine_similarity(pred_i,
    t_proj_i)), g_pred [N, P] <- its gradient: one launch.  workspace: SIAMESE_BYOL_WORKSPACE_FLOATS zeroed floats"""
    N, P = pred.shape
    assert _dense_rows(pred, N, P) and _dense_rows(t_proj, N, P) and _dense_rows(pad, N, 1)
    assert _dense_rows(g_pred, N, P) and _dense_rows(loss_out, 1, 1)
    assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.numel() >= SIAMESE_BYOL_WORKSPACE_FLOATS
    _check(load().asac_siamese_byol_loss_grad(_p(pred), _p(t_proj), _p(pad), N, P, _p(loss_out), _p(g_pred), _p(workspace),
                                              _stream()), 'asac_siamese_byol_loss_grad')


# ------------------------------------------------------------------------------------------------
# image augmentations (csrc/image.hip)
# ------------------------------------------------------------------------------------------------
IMAGE_MAX_OPS, IMAGE_MAX_PLANE, IMAGE_MAX_KERNEL = _defined('IMAGE_MAX_OPS', 'IMAGE_MAX_PLANE', 'IMAGE_MAX_KERNEL')
IMAGE_COPY, IMAGE_BLUR, IMAGE_BRIGHTNESS, IMAGE_CROP_RESIZE, IMAGE_SALT_PEPPER, IMAGE_UNIFORM_NOISE = _defined(
    'IMAGE_COPY', 'IMAGE_BLUR', 'IMAGE_BRIGHTNESS', 'IMAGE_CROP_RESIZE', 'IMAGE_SALT_PEPPER', 'IMAGE_UNIFORM_NOISE')
IMAGE_STATE_WORDS = 2          # int64: the draw counter, the arrival word
IMAGE_DRAWN = ('counter', 'choice', 'top', 'left', 'sigma', 'factor')     # the f64 record of a call's draws


def image_ops(ops):
    """a host table (ctypes array of `ImageOp`) from dicts of its fields; kept by the caller for as long as it launches"""
    assert 1 <= len(ops) <= IMAGE_MAX_OPS
    arr = (ImageOp * len(ops))()
    for slot, fields in zip(arr, ops):
        slot.top = slot.left = -1
        for k, v in fields.items():
            setattr(slot, k, v)
    return arr


@_profiled
def image_augment(x, y, ops, seed=0, instance=0, state=None, drawn=None):
    """x [N, C, H, W] -> y [N, C, Ho, Wo] (float32, contiguous) through the op of the table `ops` (`image_ops`), or through
    one member per call picked on the device where it has several: one launch.  state: int64 [2] zeros (draw counter, arrival
    word) owned by the drawing module — None only where nothing is drawn; drawn: float64 [6] | None, see `IMAGE_DRAWN`"""
    N, Cc, H, W = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    assert y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and y.dim() == 4 and y.shape[:2] == x.shape[:2]
    assert state is None or (state.is_cuda and state.dtype == torch.int64 and state.numel() == IMAGE_STATE_WORDS)
    assert drawn is None or (drawn.is_cuda and drawn.dtype == torch.float64 and drawn.numel() == len(IMAGE_DRAWN))
    _check(load().asac_image_augment(_p(x), _p(y), N * Cc, Cc, H, W, y.shape[2], y.shape[3], ops, len(ops),
                                     C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(instance) & 0x0FFFFFFF), _p(state),
                                     _p(drawn), _stream()), 'asac_image_augment')


# ------------------------------------------------------------------------------------------------
# image warps (csrc/image.hip): RandomResizedCrop / ElasticTransform with nearest sampling
# ------------------------------------------------------------------------------------------------
IMAGE_WARP_MAX_KERNEL = _defined('IMAGE_WARP_MAX_KERNEL')
IMAGE_WARP_COPY, IMAGE_WARP_RESIZED_CROP, IMAGE_WARP_ELASTIC = _defined(
    'IMAGE_WARP_COPY', 'IMAGE_WARP_RESIZED_CROP', 'IMAGE_WARP_ELASTIC')
IMAGE_WARP_DRAWN = ('counter', 'choice', 'top', 'left', 'height', 'width')     # the f64 record of a call's draws


def warp_image_ops(ops):
    """a host table (ctypes array of `ImageWarpOp`) from dicts of its fields; kept by the caller for as long as it launches"""
    assert 1 <= len(ops) <= IMAGE_MAX_OPS
    arr = (ImageWarpOp * len(ops))()
    for slot, fields in zip(arr, ops):
        for k, v in fields.items():
            setattr(slot, k, v)
    return arr


def warp_image(x, y, ops, seed=0, instance=0, state=None, drawn=None, noise_out=None, disp_out=None):
    """x [N, C, H, W] -> y [N, C, Ho, Wo] (float32, contiguous) through the op of the table `ops` (`warp_image_ops`), or
    through one member per call picked on the device where it has several: one launch.  state: as for `image_augment`, None
    only for a table that is one COPY; drawn: float64 [6] | None, see `IMAGE_WARP_DRAWN`; noise_out / disp_out: None, or
    float32 [2, H, W] that receive an ELASTIC call's field noise and its displacement (x, y) in grid units"""
    N, Cc, H, W = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    assert y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and y.dim() == 4 and y.shape[:2] == x.shape[:2]
    assert state is None or (state.is_cuda and state.dtype == torch.int64 and state.numel() == IMAGE_STATE_WORDS)
    assert drawn is None or (drawn.is_cuda and drawn.dtype == torch.float64 and drawn.numel() == len(IMAGE_WARP_DRAWN))
    for t in (noise_out, disp_out):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (2, H, W))
    _check(load().asac_image_warp(_p(x), _p(y), N * Cc, Cc, H, W, y.shape[2], y.shape[3], ops, len(ops),
                                  C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(instance) & 0x0FFFFFFF), _p(state),
                                  _p(drawn), _p(noise_out), _p(disp_out), _stream()), 'asac_image_warp')


warp_image = _profiled(warp_image, 'asac_image_warp')


# ------------------------------------------------------------------------------------------------
# observation normalization (csrc/normalize.hip): one-launch whitening, one-launch statistics update
# ------------------------------------------------------------------------------------------------
NORM_MAX_OBS = _defined('NORM_MAX_OBS')
NORM_ROW_LANES = _defined('NORM_ROW_LANES')        # logical row lanes of the update's sums: the tests' bound derives from it
NORM_F32, NORM_U8 = _defined('NORM_F32', 'NORM_U8')


def whiten_jobs(specs):
    """a host table (ctypes array of `WhitenJob`) from (src, dst, mean, variance) tensors: src / dst float32 with unit
    innermost stride whose trailing `mean.dim()` dimensions are dense and whose leading ones fold into rows of one pitch;
    kept by the caller (with the tensors) for as long as it launches.  -> None where a tensor does not have that form"""
    if not 1 <= len(specs) <= NORM_MAX_OBS:
        return None
    arr = (WhitenJob * len(specs))()
    for slot, (src, dst, mean, variance) in zip(arr, specs):
        D = mean.numel()
        ps, pd = _row_pitch(src, mean.dim(), D), _row_pitch(dst, mean.dim(), D)
        if (ps is None or pd is None or src.shape != dst.shape or src.dtype != torch.float32 or dst.dtype != torch.float32
                or mean.dtype != torch.float32 or variance.dtype != torch.float32 or not mean.is_contiguous()
                or not variance.is_contiguous() or variance.numel() != D or not (src.is_cuda and dst.is_cuda and mean.is_cuda)):
            return None
        slot.src, slot.dst, slot.mean, slot.variance = src.data_ptr(), dst.data_ptr(), mean.data_ptr(), variance.data_ptr()
        slot.D, slot.rows, slot.src_row_pitch, slot.dst_row_pitch = D, src.numel() // D, ps, pd
    return arr


def _row_pitch(t, inner_dims, D):
    """elements between consecutive rows of `t` seen as [rows, D] (D = the product of its last `inner_dims` dimensions,
    dense), or None where the leading dimensions do not fold into one pitch"""
    lead = t.dim() - inner_dims
    if lead < 0 or D == 0 or t.numel() == 0:
        return None
    expect = 1
    for size, stride in zip(reversed(t.shape[lead:]), reversed(t.stride()[lead:])):
        if size != 1 and stride != expect:
            return None
        expect *= size
    if expect != D:
        return None
    pitch = None
    for size, stride in zip(reversed(t.shape[:lead]), reversed(t.stride()[:lead])):
        if size == 1:
            continue
        if pitch is None:
            pitch, span = stride, stride * size
        elif stride == span:
            span = stride * size
        else:
            return None
    if pitch is None:
        return D
    return pitch if pitch >= D else None


@_profiled
def obs_whiten(jobs, step):
    """dst = clamp((src - mean) / sqrt(variance / (step + 1)), -5, 5) for every job of the table (`whiten_jobs`): one
    launch; `step` int32 on the device, read when the launch runs"""
    assert step.is_cuda and step.dtype == torch.int32
    _check(load().asac_obs_whiten(jobs, len(jobs), _p(step), _stream()), 'asac_obs_whiten')


@_profiled
def normalizer_update(jobs, T, step, counter):
    """the running statistics of every job of the table (ctypes array of `NormalizerJob`) over an episode of T rows, and
    step += T: one launch; `counter`: one zeroed int32 word owned by the caller, left zero"""
    assert step.is_cuda and step.dtype == torch.int32 and counter.is_cuda and counter.dtype == torch.int32
    _check(load().asac_normalizer_update(jobs, len(jobs), int(T), _p(step), _p(counter), _stream()),
           'asac_normalizer_update')


# ------------------------------------------------------------------------------------------------
# head banks: the discrete branch stacks of an ensemble or a policy, one launch per pass (csrc/head_bank.hip)
# ------------------------------------------------------------------------------------------------
HEAD_BANK_MAX_DEPTH, HEAD_BANK_MAX_ROWS = _defined('HEAD_BANK_MAX_DEPTH', 'HEAD_BANK_MAX_ROWS')


def head_bank_supported(S: int, W: int, depth: int, sizes, G: int) -> bool:
    """the limits of the `head_bank_*` entry points (include/asac_hip.h)"""
    sizes = [int(s) for s in sizes]
    return (len(sizes) > 0 and all(s > 0 for s in sizes)
            and bool(load().asac_head_bank_supported(int(S), int(W), int(depth), len(sizes), sum(sizes), int(G))))


def head_bank_desc(S: int, W: int, residual, sizes, G: int) -> HeadBankDesc:
    d = HeadBankDesc()
    d.S, d.W, d.depth, d.G = int(S), int(W), len(residual), int(G)
    for l, r in enumerate(list(residual)[:HEAD_BANK_MAX_DEPTH]):      # (a deeper stack is refused by the entry point: depth)
        d.residual[l] = int(bool(r))
    d.branches = branches(sizes)
    return d


def head_bank_table(stacks, device=None) -> torch.Tensor:
    """the stacks' tensors ((w_0, b_0, .., head w, head b) each, group-major: parameters, or gradient views) -> the DEVICE table
    of the `head_bank_*` launches, int64 [M, 2 (depth + 1)].  Every tensor is a contiguous float32 device tensor (any float
    alignment); the tensors must stay alive and keep their addresses as long as the table is used."""
    stacks = [tuple(s) for s in stacks]
    for s in stacks:
        if len(s) != len(stacks[0]) or len(s) % 2:
            raise AsacNativeError('head_bank_table: stacks of unequal depth')
        for t in s:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise AsacNativeError('head_bank_table: a tensor is not a contiguous float32 device tensor')
    dev = stacks[0][0].device if device is None else device
    return torch.tensor([[t.data_ptr() for t in s] for s in stacks], dtype=torch.int64).to(dev)


def _head_bank_rows(x, S):
    """x [.., S] (dense) or a [samples, T, S] window view with a dense last dim -> (pointer, sample stride, step stride,
    samples, steps)"""
    assert x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == S and (x.stride(-1) == 1 or S == 1)
    if x.dim() == 3 and not x.is_contiguous():
        return _p(x), x.stride(0), x.stride(1), x.shape[0], x.shape[1]
    assert x.is_contiguous(), 'head bank rows: dense rows, or a [samples, T, S] window view'
    return _p(x), S, S, x.numel() // S, 1


def _head_bank_table_ok(table, desc):
    return (table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
            and tuple(table.shape) == (desc.G * desc.branches.K, 2 * (desc.depth + 1)))


def head_bank_backward_workspace(device, rows: int, desc: HeadBankDesc) -> torch.Tensor:
    """a zeroed workspace of `head_bank_backward` over `rows` rows (records, partial sums, arrival counters); every launch
    leaves it ready for the next.  One per bank: two banks' launches must not meet in one workspace"""
    words = int(load().asac_head_bank_backward_workspace(int(rows), desc.S, desc.W, desc.depth, desc.branches.D,
                                                         desc.G * desc.branches.K))
    if words < 0:
        raise AsacNativeError(f'head_bank_backward_workspace: {rows} rows, or a bank outside the limits')
    return torch.zeros(words, dtype=torch.float32, device=device)


@_profiled
def head_bank_forward(desc: HeadBankDesc, params, x, out):
    """out [G, N, D] (contiguous) <- every stack of the bank on the rows of x: one launch"""
    px, ss, st, samples, steps = _head_bank_rows(x, desc.S)
    assert _head_bank_table_ok(params, desc)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    assert out.numel() == desc.G * samples * steps * desc.branches.D
    _check(load().asac_head_bank_forward(C.byref(desc), _p(params), px, ss, st, samples, steps, _p(out), _stream()),
           'asac_head_bank_forward')


@_profiled
def head_bank_backward(desc: HeadBankDesc, params, grads, x, grad_out, grad_x=None, accumulate=False, workspace=None):
    """grad_out [G, N, D] (contiguous) -> the views of the `grads` table written or (accumulate) added to, and, if given,
    grad_x [N, S] written: the chain launch and (with `grads`) the product launch"""
    px, ss, st, samples, steps = _head_bank_rows(x, desc.S)
    N = samples * steps
    assert _head_bank_table_ok(params, desc) and (grads is None or _head_bank_table_ok(grads, desc))
    assert grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.is_contiguous()
    assert grad_out.numel() == desc.G * N * desc.branches.D
    assert grad_x is None or (grad_x.is_cuda and grad_x.dtype == torch.float32 and grad_x.is_contiguous()
                              and grad_x.numel() == N * desc.S)
    ws = workspace if workspace is not None else (
        head_bank_backward_workspace(x.device, N, desc) if 0 < N <= HEAD_BANK_MAX_ROWS else grad_out)
    _check(load().asac_head_bank_backward(C.byref(desc), _p(params), _p(grads), px, ss, st, samples, steps, _p(grad_out),
                                          _p(grad_x), int(bool(accumulate)), _p(ws), _stream()), 'asac_head_bank_backward')
