"""Sequence layers of the model-plugin surface (reference `algorithm/nn_models/layers/seq_layers.py`): the
padding-aware `GRU` stack (14-114) and the attention layers (117-851).

-- Recurrent layers of the model-plugin surface.

`GRU` keeps the interface of reference `algorithm/nn_models/layers/seq_layers.py:14-114`
(stack of single-layer batch-first `nn.GRU`s held in `_grus`, per-step hidden states of every
layer returned as `[batch, seq, layers, hidden]`, padding-aware).  The reference packs the
left-aligned sequence with `pack_padded_sequence`, which forces a device->host copy of the valid
lengths on every call (seq_layers.py:71).  Here the valid block is left-aligned with a gather and
the recurrence simply runs over the full window: steps after the valid block cannot influence
earlier outputs and are masked to zero afterwards, so the values at valid positions are the same
and no host synchronisation is needed (the step stays graph-capturable).

On the device, cells that fit `csrc/gru.hip` (input, hidden <= 16, <= 2 layers) run as ONE fused
launch per pass (`algorithm/fused_gru.py`); the cell loop below is the generic path for larger cells
and for CPU tensors (model construction / plugin unit tests — the train step itself is device-only).

-- Attention layers of the model-plugin surface: `MultiheadAttention`, the gate layers and the
episodic (windowed, stateful) `EpisodeMultiheadAttention` stack with absolute / rotary positional
encodings.

API, sub-module names (`q_proj`, `k_proj`, `v_proj`, `out_proj`, `abpe`, `rope`, `attn`, `gatedlayer`,
`layer_norm`, `_attn_list`) and numerics follow reference
`algorithm/nn_models/layers/seq_layers.py:117-851`, so user representation files and checkpoints
interchange.  On the device, in float32, the math runs as hand-written launches (csrc/attn.hip, attn_mh.hip,
rows_proj.hip, rope.hip, rows_gate.hip) whose autograd glue is `algorithm/fused_attention.py`; this file keeps
the modules, the `FUSED_*` switches, the recognisers that decide whether a call fits a launch, and the dropout
draw states.  `MultiheadAttention.forward` picks one of four routes — one head with the projections on chip, the
multi-head launches, the one-head core, the library's module code (CPU, other dtypes, shapes the kernels do not
have) — and nothing here synchronises with the host, so an attention representation stays inside the captured
train step.

Per-layer "hidden state" of the episodic stack = the previous layers' outputs at the query
positions, which lets a window be continued from where the last one stopped:
  * hidden_state None            — run every layer over the full key window
  * is_prev_hidden_state False   — `hidden_state` holds, per layer, outputs for positions BEFORE the
                                   window (acting: history of up to burn_in steps)
  * is_prev_hidden_state True    — `hidden_state` holds the state just before the window's first
                                   element (training: one stored state per sampled window)
"""
import math
import os
from enum import Enum

import torch
from torch import nn

from asac_amd import native

from algorithm.fused_attention import (_AttnBlockFn, _AttnCoreFn, _AttnMhFn, _AttnProjFn, _GateRowsFn, _OutResRowsFn,
                                       _QkvAttnMhFn, _QkvDenseDropFn, _QkvRowsFn, _RopeFn)

from .linear_layers import LinearLayers

# the name the output block with live dropout was applied under before it became `_OutResRowsFn(..., draws)`: same arguments
# (tests/test_dense_dropout_gpu.py calls the launch pair directly through it)
_OutResDropRowsFn = _OutResRowsFn

__all__ = ['GRU', 'step_mask_cache', 'POSITIONAL_ENCODING', 'GATE', 'MultiheadAttention', 'GatedResidualLayer', 'GatedOutputLayer',
           'GatedRecurrentLayer', 'GatedCatLayer', 'EpisodeMultiheadAttentionBlock',
           'EpisodeMultiheadAttention', 'AbsolutePositionalEncoding', 'RotaryPositionalEncoding',
           'RotaryPositionalEncoding2']


class GRU(nn.Module):
    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, dropout=0.0,
                 device=None, dtype=None):
        super().__init__()
        self.num_layers = num_layers
        self._fusable = bool(bias) and dropout == 0.0
        self._grus = nn.ModuleList([
            nn.GRU(input_size=input_size if i == 0 else hidden_size, hidden_size=hidden_size,
                   num_layers=1, bias=bias, batch_first=True, dropout=dropout,
                   device=device, dtype=dtype)
            for i in range(num_layers)])

    def forward(self, x, h0=None, padding_mask=None):
        """
        x: [batch, seq, input]; h0: [batch, layers, hidden] or None; padding_mask: bool [batch, seq]
        returns output [batch, seq, hidden], hn [batch, seq, layers, hidden]
        """
        from algorithm.fused_gru import fused_gru, fused_gru_supported   # lazy: avoids an import cycle
        cell = self._grus[0]
        if self._fusable and fused_gru_supported(x, cell.input_size, cell.hidden_size, self.num_layers):
            # one launch for the whole window (csrc/gru.hip); same values as the cell loop below
            return fused_gru(x, h0, padding_mask, list(self._grus), layer=self)     # (top layer [B, L, H], hn)
        if self._fusable and x.is_cuda:
            from algorithm.fused_gru_wide import fused_gru_wide, fused_gru_wide_supported
            if fused_gru_wide_supported(x, list(self._grus)):
                # hidden 32 / 64 / 128: the recurrence of each layer as one MFMA launch (csrc/gru_wide.hip)
                return fused_gru_wide(x, h0, padding_mask, list(self._grus), layer=self)

        if h0 is not None:
            h0 = h0.transpose(0, 1).contiguous()  # [layers, batch, hidden]
        batch, seq_len, _ = x.shape

        if padding_mask is not None:
            lead = padding_mask.long().argmin(dim=1, keepdim=True)  # first valid position
            steps = torch.arange(seq_len, device=x.device).unsqueeze(0)
            fwd_idx = torch.clamp(steps + lead, max=seq_len - 1)  # left-align the valid block
            bwd_idx = torch.clamp(steps - lead, min=0)            # and put results back
            x = x.gather(1, fwd_idx.unsqueeze(-1).expand(-1, -1, x.shape[-1]))

        per_layer = []
        for i, gru in enumerate(self._grus):
            out, _ = gru(x, None if h0 is None else h0[i:i + 1])
            x = out
            if padding_mask is not None:
                out = out.gather(1, bwd_idx.unsqueeze(-1).expand(-1, -1, out.shape[-1]))
                out = out.masked_fill(padding_mask.unsqueeze(-1), 0.0)
            per_layer.append(out)

        return per_layer[-1], torch.stack(per_layer, dim=2)


class POSITIONAL_ENCODING(Enum):
    ABSOLUTE = 1
    ABSOLUTE_CAT = 2
    ROPE = 3
    ROPE2 = 4


class GATE(Enum):
    RESIDUAL = 1
    OUTPUT = 2
    RECURRENT = 3
    CAT = 4


# ------------------------------------------------------------------------------------------------
# positional encodings
# ------------------------------------------------------------------------------------------------
class AbsolutePositionalEncoding(nn.Module):
    def __init__(self, d_model: int, max_seq_len: int = 5000):
        super().__init__()
        self.d_model = d_model
        pos = torch.arange(max_seq_len, dtype=torch.float64).unsqueeze(1)
        i = torch.arange(0, d_model, 2, dtype=torch.float64)
        pe = torch.zeros(max_seq_len, d_model, dtype=torch.float64)
        # even slot i: sin(pos / 10000^(2i/d)); odd slot i+1: cos(pos / 10000^(2(i+1)/d))
        pe[:, 0::2] = torch.sin(pos / torch.pow(10000., 2 * i / d_model))
        pe[:, 1::2] = torch.cos(pos / torch.pow(10000., 2 * (i + 1) / d_model))[:, :d_model // 2]
        self.register_buffer('pe', pe.to(torch.float32))

    @torch.no_grad()
    def forward(self, indexes):
        return self.pe[indexes.type(torch.int64)]


class RotaryPositionalEncoding(nn.Module):
    """Complex-pair rotary encoding: consecutive feature pairs are rotated by index * theta_i."""

    def __init__(self, d_model: int, max_seq_len: int = 5000, theta: float = 10000.0):
        super().__init__()
        freqs = 1.0 / (theta ** (torch.arange(0, d_model, 2)[: (d_model // 2)] / d_model))
        angles = torch.outer(torch.arange(max_seq_len), freqs)
        self.register_buffer('freqs_cis', torch.polar(torch.ones_like(angles), angles))

    def _rotate(self, x, indexes):
        rot = self.freqs_cis[indexes.type(torch.int64)]
        xc = torch.view_as_complex(x.reshape(*x.shape[:-1], -1, 2))
        return torch.view_as_real(xc * rot).flatten(2).type_as(x)

    def forward(self, xq_indexes, xk_indexes, xq, xk):
        return self._rotate(xq, xq_indexes), self._rotate(xk, xk_indexes)


class RotaryPositionalEncoding2(nn.Module):
    """Half-split rotary encoding: feature j is paired with j + d/2."""

    def __init__(self, d_model: int, max_seq_len: int = 5000, base: int = 10_000):
        super().__init__()
        self.d_model = d_model
        theta = 1. / (base ** (torch.arange(0, d_model, 2).float() / d_model))
        idx_theta = torch.einsum('n,d->nd', torch.arange(max_seq_len).float(), theta)
        idx_theta2 = torch.cat([idx_theta, idx_theta], dim=1)
        self.register_buffer('cos_cached', idx_theta2.cos())
        self.register_buffer('sin_cached', idx_theta2.sin())

    def _neg_half(self, x):
        d_2 = self.d_model // 2
        return torch.cat([-x[:, :, d_2:], x[:, :, :d_2]], dim=-1)

    def _rotate(self, x, indexes):
        rope, rest = x[..., :self.d_model], x[..., self.d_model:]
        rope = rope * self.cos_cached[indexes] + self._neg_half(rope) * self.sin_cached[indexes]
        return torch.cat((rope, rest), dim=-1)

    def forward(self, xq_indexes, xk_indexes, xq, xk):
        return self._rotate(xq, xq_indexes), self._rotate(xk, xk_indexes)


# ------------------------------------------------------------------------------------------------
FUSED_PROJECTIONS = True      # q / k / v Linear projections inside the attention launch when they are plain Linears
# several heads: the core of all heads as one MFMA launch (csrc/attn_mh.hip); ASAC_ATTN_MH=0 keeps the module path (A/B runs)
FUSED_MULTIHEAD = os.environ.get('ASAC_ATTN_MH', '1') != '0'
# the Linear layers around the multi-head core as one launch each (csrc/rows_proj.hip)   (0: library GEMMs — A/B runs)
FUSED_ROWS_PROJ = os.environ.get('ASAC_ROWS_PROJ', '1') != '0'
# ... and, for windows of <= 16 positions, the q / k / v projections inside the core's forward launch   (0: a launch of their own)
FUSED_QKV_IN_CORE = os.environ.get('ASAC_QKV_IN_CORE', '1') != '0'
# ... and the block's backward as one launch too   (0: ResBlock backward, core backward, projections' backward)
FUSED_BLOCK_BACKWARD = os.environ.get('ASAC_ATTN_BLOCK_BWD', '1') != '0'
# the gate behind an episode block's attention, with the padded-row factor, as one launch per pass (csrc/rows_gate.hip)
# (False: the gate layer's module code — tests and tools/gate_bench.py).  On for all three kinds: the captured step of each is
# faster than with the module code by far more than the box spread (NOTES.md, gate round: 1.15x / 1.59x / 3.2x)
FUSED_GATE = True
# a rotary position encoding (ROPE / ROPE2) as the epilogue of the q / k / v projection launch (csrc/rows_proj.hip), or as one
# launch per pass behind other projections (csrc/rope.hip)   (False: `self.rope(...)` as module code behind library GEMMs —
# tests and tools/rope_bench.py)
FUSED_ROPE = True
# dropout of the attention weights (training mode, 0 < dropout < 1) inside the multi-head core's launches: the mask is drawn on
# the device from a counter the module instance owns and regenerated by the backward (csrc/asac_dropout.h)   (False: the
# baddbmm / softmax / F.dropout / bmm chain of the module code — tests and tools/attn_dropout_bench.py)
FUSED_ATTN_DROPOUT = True
# the LIVE nn.Dropout modules inside the dense stacks around the core (`qkv_dense_depth=1`: ResBlock -> Dropout -> Linear three
# times; `out_dense_depth=1`: ResBlock -> Dropout) inside one row launch per site and pass (csrc/rows_proj.hip), drawn like the
# weights' dropout from a counter state the site owns   (False: the stacks module by module with ATen's dropout, which draws
# from torch's generator — tests and tools/attn_dropout_bench.py --dense)
FUSED_DENSE_DROPOUT = True


def _fused_rope_tables(module, query, key, query_index, key_index):
    """the tables `_RopeFn` / `_QkvRowsFn` read for the rotary encoding of `module`, or None: `self.rope` runs as module
    code (CPU, other dtypes, odd widths, tables that are not contiguous f32 / complex64 buffers on the tensors' device, indexes
    that are not int32 / int64 [batch, len] there, a subclassed rope module)"""
    rope, E = module.rope, module.embed_dim
    if not (FUSED_ROPE and query.is_cuda and key.is_cuda and query.dtype == key.dtype == torch.float32
            and query.dim() == key.dim() == 3 and E % 2 == 0):
        return None
    for index, t in ((query_index, query), (key_index, key)):
        if not (index.device == t.device and index.dtype in (torch.int32, torch.int64) and index.dtype == key_index.dtype
                and index.shape == t.shape[:2]):
            return None
    if type(rope) is RotaryPositionalEncoding:
        tables = (rope.freqs_cis,)
        if rope.freqs_cis.dtype != torch.complex64 or rope.freqs_cis.dim() != 2 or rope.freqs_cis.shape[1] != E // 2:
            return None
    elif type(rope) is RotaryPositionalEncoding2:
        tables = (rope.cos_cached, rope.sin_cached)
        if any(t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != E for t in tables) or rope.d_model != E \
                or rope.cos_cached.shape != rope.sin_cached.shape:
            return None
    else:
        return None
    if not all(t.device == key.device and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in tables):
        return None
    if not native.rope_supported(module.pe.value, E):
        return None
    return (torch.view_as_real(tables[0]),) if len(tables) == 1 else tables


def _is_index_tail(query_index, key_index):
    """query_index is `key_index[:, -q:]` (the 2-D sibling of `_is_tail_view`): one index array serves the projection launch"""
    q = query_index.shape[1]
    return (query_index.dim() == key_index.dim() == 2 and q <= key_index.shape[1] and query_index.shape[0] == key_index.shape[0]
            and query_index.dtype == key_index.dtype and query_index.stride() == key_index.stride()
            and query_index.untyped_storage().data_ptr() == key_index.untyped_storage().data_ptr()
            and query_index.storage_offset() == key_index.storage_offset() + (key_index.shape[1] - q) * key_index.stride(1))


def _gate_linear_ok(lin, width, bias) -> bool:
    return (type(lin) is nn.Linear and lin.in_features == lin.out_features == width and (lin.bias is not None) == bias
            and lin.weight.dtype == torch.float32 and _params_aligned16(lin))


def _fused_gate_params(block, x, y, key_padding_mask):
    """the parameters `_GateRowsFn` takes for the gate of `block`, or None: the gate layer's module code runs (CPU, other
    dtypes, widths the kernel does not have, parameters that are misaligned views, CAT, a subclassed gate layer)"""
    gate, layer = block.gate, block.gatedlayer
    if not (FUSED_GATE and isinstance(gate, GATE) and gate in (GATE.RESIDUAL, GATE.OUTPUT, GATE.RECURRENT)
            and x.is_cuda and y.is_cuda and x.dtype == y.dtype == torch.float32 and x.dim() == 3 and x.shape == y.shape):
        return None
    if key_padding_mask is not None and not (key_padding_mask.dtype == torch.bool and key_padding_mask.is_cuda
                                             and key_padding_mask.dim() == 2 and key_padding_mask.shape[0] == x.shape[0]
                                             and key_padding_mask.shape[1] >= x.shape[1]):
        return None
    E = x.shape[2]
    if not native.rows_gate_supported(gate.value, E):
        return None
    if gate == GATE.RESIDUAL:
        return () if type(layer) is GatedResidualLayer else None
    if gate == GATE.OUTPUT:
        if type(layer) is GatedOutputLayer and _gate_linear_ok(layer.dense, E, False):
            return (layer.dense.weight,)
        return None
    if type(layer) is not GatedRecurrentLayer:
        return None
    lins = (layer.dense_x_r, layer.dense_y_r, layer.dense_x_z, layer.dense_y_z, layer.dense_x_g, layer.dense_y_g)
    if not all(_gate_linear_ok(lin, E, lin is layer.dense_x_z) for lin in lins):
        return None
    return (*(lin.weight for lin in lins), layer.dense_x_z.bias)


def _rows_proj_ok(module, query, key) -> bool:
    """the q / k / v projections of `module` as one `_QkvRowsFn` launch: plain Linears E -> E over a device window batch whose
    query is the key tensor or its newest positions"""
    if not (FUSED_ROWS_PROJ and key.is_cuda and key.dtype == torch.float32 and key.dim() == 3 and key.stride(2) == 1):
        return False
    if not (query is key or _is_tail_view(query, key)):
        return False
    E = module.embed_dim
    if not native.rows_proj_supported(E):
        return False
    for ll in (module.q_proj, module.k_proj, module.v_proj):
        lin = _plain_linear(ll)
        if lin is None or lin.in_features != E or lin.out_features != E:
            return False
    return True


def _is_tail_view(query, key):
    """query is `key[:, -q:]` (the episode blocks' cut query): same memory, so one gradient serves both"""
    q = query.shape[1]
    return (q <= key.shape[1] and query.shape[0] == key.shape[0]
            and query.shape[2] == key.shape[2] and query.stride() == key.stride()
            and query.untyped_storage().data_ptr() == key.untyped_storage().data_ptr()
            and query.storage_offset() == key.storage_offset() + (key.shape[1] - q) * key.stride(1))


def _plain_resblock(ll, width):
    """the Linear of a `LinearLayers` stack that is exactly ONE residual GELU ResBlock width -> width, or None"""
    mods = [m for m in ll.dense if not (isinstance(m, nn.Dropout) and m.p == 0)]
    if len(mods) != 1 or not _fusable_resblock(mods[0], width):
        return None
    return mods[0].linear


def _live_dropout(mod) -> bool:
    """an nn.Dropout that drops in this pass — the sub-module's OWN state, not the attention module's"""
    return type(mod) is nn.Dropout and mod.training and 0. < mod.p < 1.


def _fusable_resblock(rb, width) -> bool:
    from .linear_layers import ResBlock
    return (isinstance(rb, ResBlock) and rb.residual and type(rb.act) is nn.GELU
            and getattr(rb.act, 'approximate', 'none') == 'none' and rb.linear.bias is not None
            and rb.linear.in_features == rb.linear.out_features == width and _params_aligned16(rb.linear))


def _dropout_resblock(ll, width):
    """(the ResBlock's Linear, the nn.Dropout) of a `LinearLayers` stack that is exactly ONE residual exact-GELU ResBlock
    width -> width and ONE LIVE nn.Dropout, or None"""
    mods = list(ll.dense)
    if len(mods) == 2 and _fusable_resblock(mods[0], width) and _live_dropout(mods[1]):
        return mods[0].linear, mods[1]
    return None


def _dropout_dense_stack(ll, width):
    """(the ResBlock's Linear, the nn.Dropout, the Linear) of a `LinearLayers` stack that is exactly ONE residual exact-GELU
    ResBlock width -> width, ONE LIVE nn.Dropout and ONE nn.Linear width -> width with bias, or None"""
    mods = list(ll.dense)
    if (len(mods) == 3 and _fusable_resblock(mods[0], width) and _live_dropout(mods[1]) and type(mods[2]) is nn.Linear
            and mods[2].bias is not None and mods[2].in_features == mods[2].out_features == width and _params_aligned16(mods[2])):
        return mods[0].linear, mods[1], mods[2]
    return None


def _dense_qkv_ok(module, query, key):
    """the three (ResBlock Linear, Dropout, Linear) of `module`'s q / k / v stacks for one `_QkvDenseDropFn` launch — the
    envelope of `_rows_proj_ok` with `_dropout_dense_stack` in the place of `_plain_linear`, and one p — or None"""
    if not (FUSED_DENSE_DROPOUT and FUSED_ROWS_PROJ and key.is_cuda):
        return None
    E = module.embed_dim
    if not native.rows_proj_supported(E):      # (first: the cheapest way out for the narrow toy plugins)
        return None
    if not (key.dtype == torch.float32 and key.dim() == 3 and key.stride(2) == 1 and (query is key or _is_tail_view(query, key))):
        return None
    stacks = [_dropout_dense_stack(ll, E) for ll in (module.q_proj, module.k_proj, module.v_proj)]
    if any(s is None for s in stacks) or len({s[1].p for s in stacks}) != 1:
        return None
    return stacks


def _params_aligned16(linear) -> bool:
    """The MFMA row kernels read weights and biases as 16-byte vectors and reject anything else (`bad_arg` -> AsacNativeError).
    Parameters are views packed back to back in the learner's flat buffer: only SEGMENT starts are aligned, so a plugin
    whose model holds an earlier parameter of numel % 4 != 0 (a scalar gate, an odd-width Linear) shifts everything behind
    it — such layers take the nn.Linear path instead of crashing in forward."""
    return (linear.weight.data_ptr() % 16 == 0 and linear.weight.is_contiguous()
            and (linear.bias is None or (linear.bias.data_ptr() % 16 == 0 and linear.bias.is_contiguous())))


def _plain_linear(ll):
    """the single nn.Linear (with bias) of a `LinearLayers` stack that is nothing else, or None"""
    mods = [m for m in ll.dense if not (isinstance(m, nn.Dropout) and m.p == 0)]
    if len(mods) == 1 and type(mods[0]) is nn.Linear and mods[0].bias is not None and _params_aligned16(mods[0]):
        return mods[0]
    return None


def _fused_core_ok(q, k, num_heads, dropout_active) -> bool:
    if not (q.is_cuda and q.dtype == torch.float32 and num_heads == 1 and not dropout_active):
        return False
    return native.attention_supported(q.shape[1], k.shape[1], q.shape[2])


def _fold_masks(attn_mask, key_padding_mask, q_len):
    """the padded keys blocked for every query -> (attn_mask as the module code reads it, the same as the 3-D bool / uint8
    mask the launches read); (None, None) without masks"""
    if key_padding_mask is not None:
        kpm = key_padding_mask.unsqueeze(1)                               # [bsz, 1, k]
        attn_mask = kpm.expand(-1, q_len, -1) if attn_mask is None else torch.logical_or(attn_mask, kpm)
    m = attn_mask
    if m is not None:
        m = m.unsqueeze(0) if m.dim() == 2 else m
        m = m if m.dtype in (torch.bool, torch.uint8) else m != 0
    return attn_mask, m


def _row_mask(out_row_mask):
    """out_row_mask as bool / uint8 [batch, q], or None"""
    if out_row_mask is None:
        return None
    rz = out_row_mask.reshape(-1, out_row_mask.shape[-1])
    return rz if rz.dtype in (torch.bool, torch.uint8) else rz != 0


class _DrawSite:
    """One dropout site of a module (the attention weights, the 'qkv' stacks, the 'out' stack): its draw state on every
    device it launched on — int64 [544]: the call counter and the arrival words — and the `used` record of its last call"""

    def __init__(self, what: str):
        self.what, self.states, self.used = what, {}, None

    def draws(self, device, p, key):
        """(p, seed, instance id, state, used) of one dropout launch on `device`, or None where the module code has to run:
        the state does not exist yet and the stream is capturing (allocating and seeding are not part of a capture).  `key()`
        -> (seed, instance id, first counter) is asked only past that point.  `used` is this CALL's record: a module applied
        twice before its backwards (observations and next observations) keeps both counters apart."""
        state = self.states.get(device)
        if state is None and torch.cuda.is_current_stream_capturing():
            return None
        seed, instance, counter0 = key()
        if state is None:
            state = self.states[device] = torch.tensor([counter0] + [0] * (native.ATTN_DROPOUT_STATE_WORDS - 1),
                                                       dtype=torch.int64, device=device)
        self.used = torch.empty(1, dtype=torch.int64, device=device)
        return p, seed, instance, state, self.used

    def state(self, device=None):
        """(call counter, how many arrival words are not zero) of the state on `device` (default: the only one), or None where
        there is none yet.  Synchronises."""
        if not self.states:
            return None
        state = self.states[device] if device is not None else next(iter(self.states.values()))
        return int(state[0].item()), int(torch.count_nonzero(state[1:]).item())

    def drawn(self) -> int:
        """the call counter the last launch drew with.  Synchronises."""
        if self.used is None:
            raise RuntimeError(f'no {self.what} launch yet')
        return int(self.used.item())


class MultiheadAttention(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int = 1, pe=None, qkv_dense_depth: int = 0,
                 out_dense_depth: int = 0, out_size: int | None = None, dropout: float = 0.) -> None:
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, 'embed_dim must be divisible by num_heads'
        self.pe, self.dropout = pe, dropout

        in_dim = embed_dim
        if pe == POSITIONAL_ENCODING.ABSOLUTE:
            self.abpe = AbsolutePositionalEncoding(embed_dim)
        elif pe == POSITIONAL_ENCODING.ABSOLUTE_CAT:
            self.abpe = AbsolutePositionalEncoding(embed_dim)
            in_dim = embed_dim * 2
        elif pe == POSITIONAL_ENCODING.ROPE:
            self.rope = RotaryPositionalEncoding(embed_dim)
        elif pe == POSITIONAL_ENCODING.ROPE2:
            self.rope = RotaryPositionalEncoding2(embed_dim)

        proj = lambda: LinearLayers(in_dim, dense_n=embed_dim, dense_depth=qkv_dense_depth,  # noqa: E731
                                    output_size=embed_dim, dropout=dropout)
        self.q_proj, self.k_proj, self.v_proj = proj(), proj(), proj()
        self.out_proj = LinearLayers(embed_dim, dense_n=embed_dim, dense_depth=out_dense_depth,
                                     output_size=out_size, dropout=dropout)
        # the dropout launches' streams of draws (csrc/asac_dropout.h): plain attributes, no buffers — the state_dict keeps the
        # reference's keys.  Instance id and seed are taken when the first draw state is created.
        self._drop_instance = None         # from the one counter of algorithm/utils/image_transforms.py
        self._drop_seed = None             # None: torch.initial_seed() at the first launch
        self._drop_counter0 = 0            # where a device first launched on later starts counting
        # the attention weights' site and the dense stacks' ('qkv', 'out': seq_layers.FUSED_DENSE_DROPOUT): all draw from the
        # same (seed, instance id), the dense sites under tags of their own, each with a state and a `used` record of its own
        self._drop_weights = _DrawSite('dropout')
        self._drop_dense = {'qkv': _DrawSite('qkv dropout'), 'out': _DrawSite('out dropout')}

    _drop_used = property(lambda self: self._drop_weights.used)      # int64 [1]: the counter the last weights launch drew with

    def reseed(self, seed: int, counter: int = 0, instance_id: int | None = None):
        """the draws of the module's dropout launches (the attention weights', the dense stacks') are functions of (seed,
        instance id, call counter): re-seat all three, in every state"""
        self._drop_seed = int(seed)
        if instance_id is not None:
            self._drop_instance = int(instance_id)
        for site in (self._drop_weights, *self._drop_dense.values()):
            for state in site.states.values():
                state.copy_(torch.tensor([int(counter)] + [0] * (state.numel() - 1), dtype=torch.int64))
        self._drop_counter0 = int(counter)
        return self

    def _drop_key(self):
        """(seed, instance id, first counter) of the module's draws; takes the instance id and the seed if nobody has yet"""
        if self._drop_instance is None:
            from algorithm.utils.image_transforms import _instance_ids
            self._drop_instance = next(_instance_ids)
        if self._drop_seed is None:
            self._drop_seed = torch.initial_seed()
        return self._drop_seed, self._drop_instance, self._drop_counter0

    def dropout_drawn(self) -> int:
        """the call counter the last dropout launch drew with.  Synchronises."""
        return self._drop_weights.drawn()

    def dropout_state(self, device=None):
        """(call counter, how many arrival words are not zero) of the dropout state on `device` (default: the only one), or
        None where there is none yet.  Synchronises."""
        return self._drop_weights.state(device)

    def dense_dropout_drawn(self, site: str) -> int:
        """the call counter the last dense-stack dropout launch of `site` ('qkv' or 'out') drew with.  Synchronises."""
        return self._drop_dense[site].drawn()

    def dense_dropout_state(self, site: str, device=None):
        """`dropout_state` of the dense-stack dropout launch of `site` ('qkv' or 'out')"""
        return self._drop_dense[site].state(device)

    def _split_heads(self, x):
        """[bsz, len, embed] -> [bsz * heads, len, head_dim], head-major like chunk+cat on dim 0"""
        if self.num_heads == 1:
            return x
        b, l, _ = x.shape
        return x.view(b, l, self.num_heads, self.head_dim).permute(2, 0, 1, 3).reshape(self.num_heads * b, l, self.head_dim)

    def forward(self, query, key, value, query_index=None, key_index=None, key_padding_mask=None, attn_mask=None,
                out_row_mask=None):
        """query [batch, q, E]; key / value [batch, k, E]; *_index [batch, len]; key_padding_mask
        [batch, k] (True = ignore); attn_mask [batch, q, k] or [q, k] (True = blocked); out_row_mask
        [batch, q] (True = zero that output row: the caller's padded positions)
        -> (output [batch, q, E_out], weights [batch, q, k] averaged over heads)"""
        lead = query.shape[:-2]
        same_kv = value is key
        query, key, value = (t.reshape(-1, *t.shape[-2:]) for t in (query, key, value))
        bsz, q_len, k_len = query.shape[0], query.shape[1], key.shape[1]
        if key_padding_mask is not None:
            key_padding_mask = key_padding_mask.reshape(-1, key_padding_mask.shape[-1])
        if attn_mask is not None:
            assert attn_mask.dim() in (2, 3)

        # positional encodings (the rotary ones follow the projections: `_project`)
        own_index = query_index is None and key_index is None
        if self.pe:       # (None and False both mean no positional encoding)
            if query_index is None:
                query_index = torch.arange(q_len, device=query.device).unsqueeze(0).expand(bsz, -1)
            if key_index is None:
                key_index = torch.arange(k_len, device=key.device).unsqueeze(0).expand(bsz, -1)
        if self.pe == POSITIONAL_ENCODING.ABSOLUTE:
            query = self.abpe(query_index) + query
            kpe = self.abpe(key_index)
            key, value = kpe + key, kpe + value
        elif self.pe == POSITIONAL_ENCODING.ABSOLUTE_CAT:
            query = torch.cat([query, self.abpe(query_index)], dim=-1)
            kpe = self.abpe(key_index)
            key, value = torch.cat([key, kpe], dim=-1), torch.cat([value, kpe], dim=-1)

        # masks: `attn_mask` with the padded keys blocked as the module code reads it, `m` / `rz` as the launches do
        attn_mask, m = _fold_masks(attn_mask, key_padding_mask, q_len)
        rz = _row_mask(out_row_mask)

        # the first route that takes the call: projections, core and output stack of each are in its method
        no_pe = self.pe is None or self.pe is False
        res = self._attend_proj(query, key, m, rz) if no_pe and same_kv else None       # one head, projections on chip
        if res is None:
            q, k, v, fused_qkv = self._project(query, key, value, same_kv, query_index, key_index, own_index)
            res = self._attend_multihead(q, k, v, fused_qkv, key, q_len, m, rz)         # the multi-head launches
        if res is None:
            q, k, v = self._split_heads(q), self._split_heads(k), self._split_heads(v)
            res = self._attend_core(q, k, v, m, rz)                                     # one head, the core alone
        if res is None:
            res = self._attend_module(q, k, v, attn_mask, rz, bsz)                      # the library's module code
        out, weights = res
        return out.reshape(*lead, *out.shape[1:]), weights.reshape(*lead, *weights.shape[1:])

    def _drop_active(self) -> bool:
        return self.training and self.dropout > 0.

    def _out_stack(self, out, scale, rz):
        """the output stack, then the dead-row factor `scale` [batch, q] (None: no query can be fully masked), then the
        caller's padded rows"""
        out = self.out_proj(out)
        if scale is not None:
            out = out * scale.unsqueeze(-1)
        if rz is not None:
            out = out * (~rz).to(out.dtype).unsqueeze(-1)
        return out

    def _project(self, query, key, value, same_kv, query_index, key_index, own_index):
        """q / k / v stacks and the rotary encoding -> (q, k, v, fused_qkv).  With `fused_qkv` (the six parameters of plain
        Linears) the projections are left to the multi-head core's forward launch and q, k, v are still the key tensor."""
        bsz, q_len, k_len = query.shape[0], query.shape[1], key.shape[1]
        fused_qkv = None
        rotary = self.pe in (POSITIONAL_ENCODING.ROPE, POSITIONAL_ENCODING.ROPE2)
        rope_tables = _fused_rope_tables(self, query, key, query_index, key_index) if rotary else None
        plain_or_rotary = self.pe is None or self.pe is False or rope_tables is not None
        dense, dense_draws = (_dense_qkv_ok(self, query, key) if plain_or_rotary and same_kv else None), None
        if dense is not None and bsz * k_len * self.embed_dim < 1 << 34:
            # None: this call runs the module code below
            dense_draws = self._drop_dense['qkv'].draws(key.device, dense[0][1].p, self._drop_key)
        if dense_draws is not None:
            # dense q / k / v stacks with their live nn.Dropout: one launch per pass (csrc/rows_proj.hip); a rotary encoding
            # follows as the `_RopeFn` launch
            q, k, v = _QkvDenseDropFn.apply(key, q_len, dense_draws,
                                            *(t for r, _, lin in dense for t in (r.weight, r.bias, lin.weight, lin.bias)))
        elif plain_or_rotary and same_kv and _rows_proj_ok(self, query, key):
            qkv_params = [t for ll in (self.q_proj, self.k_proj, self.v_proj) for t in (_plain_linear(ll).weight, _plain_linear(ll).bias)]
            # (without indexes the query's positions count from 0: the key's newest entries only when the lengths agree)
            if rotary and ((own_index and q_len == k_len) or query_index is key_index or _is_index_tail(query_index, key_index)):
                # projections and rotation: one launch per pass (csrc/rows_proj.hip)
                q, k, v = _QkvRowsFn.apply(key, q_len, (key_index, self.pe.value, rope_tables), *qkv_params)
                rotary = False
            elif (not rotary and FUSED_MULTIHEAD and FUSED_QKV_IN_CORE and (self.num_heads > 1 or self.head_dim > 16)
                    and not self._drop_active() and native.attention_mh_proj_supported(q_len, k_len, self.num_heads, self.head_dim)):
                fused_qkv = qkv_params      # windows of <= 16 positions: the projections run inside the core's forward launch
                q = k = v = key
            else:
                q, k, v = _QkvRowsFn.apply(key, q_len, None, *qkv_params)
        else:
            q, k, v = self.q_proj(query), self.k_proj(key), self.v_proj(value)
        if rotary and rope_tables is not None:
            q, k = _RopeFn.apply(q, k, query_index, key_index, self.pe.value, rope_tables)      # one launch per pass (csrc/rope.hip)
        elif rotary:
            q, k = self.rope(query_index, key_index, q, k)
        return q, k, v, fused_qkv

    def _attend_proj(self, query, key, m, rz):
        """one head, no positional encoding, plain Linears: projections + scores / mask / softmax / weighted sum — and an
        output stack that is one ResBlock, with the dead-row rule and the row mask — as one launch per pass (csrc/attn.hip)"""
        if not (FUSED_PROJECTIONS and query.dim() == 3 and _fused_core_ok(query, key, self.num_heads, self._drop_active())):
            return None
        lq, lk, lv = _plain_linear(self.q_proj), _plain_linear(self.k_proj), _plain_linear(self.v_proj)
        if lq is None or lk is None or lv is None or not lq.in_features == lq.out_features == self.embed_dim:
            return None
        qkv = (lq.weight, lq.bias, lk.weight, lk.bias, lv.weight, lv.bias)
        xq = query.shape[1] if _is_tail_view(query, key) else query
        lo = _plain_resblock(self.out_proj, self.embed_dim)
        if lo is not None:
            out, weights, _ = _AttnProjFn.apply(xq, key, m, rz, *qkv, lo.weight, lo.bias)
            return out, weights
        out, weights, keep = _AttnProjFn.apply(xq, key, m, None, *qkv)
        return self._out_stack(out, keep if m is not None else None, rz), weights

    def _attend_multihead(self, q, k, v, fused_qkv, x, q_len, m, rz):
        """several heads (or one wide head): scores, mask, softmax, weighted sum and the head average as one MFMA launch per
        pass (csrc/attn_mh.hip), the output ResBlock in a row launch behind it or — windows of <= 16 positions — in the same"""
        bsz, k_len, E = x.shape[0], x.shape[1], self.embed_dim
        drop_active = self._drop_active()
        if not (FUSED_MULTIHEAD and (self.num_heads > 1 or self.head_dim > 16) and q.is_cuda and q.dtype == torch.float32
                and (not drop_active or (FUSED_ATTN_DROPOUT and self.dropout < 1.))
                and native.attention_mh_supported(q_len, k_len, self.num_heads, self.head_dim)):
            return None
        draws = None
        if drop_active:
            # the weights' dropout inside the core's launches; None: this call runs the module code
            if bsz * self.num_heads <= native.ATTN_DROPOUT_MAX_BATCH_HEADS:
                draws = self._drop_weights.draws(q.device, self.dropout, self._drop_key)
            if draws is None:
                return None
        lo = _plain_resblock(self.out_proj, E) if FUSED_ROWS_PROJ else None
        # an output stack with a LIVE nn.Dropout behind its ResBlock: the drop inside the ResBlock launch
        lod = _dropout_resblock(self.out_proj, E) \
            if lo is None and FUSED_ROWS_PROJ and FUSED_DENSE_DROPOUT and native.rows_proj_supported(E) else None
        out_draws = None
        if lod is not None and bsz * q_len * E < 1 << 34:
            out_draws = self._drop_dense['out'].draws(q.device, lod[1].p, self._drop_key)
        if fused_qkv is not None and lo is not None and FUSED_BLOCK_BACKWARD:
            # projections, core and output ResBlock: the block is ONE launch forward and ONE backward
            out, weights, _, _ = _AttnBlockFn.apply(x, q_len, *fused_qkv, lo.weight, lo.bias, m, self.num_heads, rz,
                                                    rz is not None or m is not None)
            return out, weights
        y_pre = None
        if fused_qkv is not None:
            out, weights, keep, keep_rows, *y_pre = _QkvAttnMhFn.apply(x, q_len, *fused_qkv, m, self.num_heads, rz,
                                                                       None if lo is None else (lo.weight, lo.bias))
        else:
            out, weights, keep, keep_rows = _AttnMhFn.apply(q, k, v, m, self.num_heads, rz, draws)
        # the dead-row rule and the caller's padded rows as ONE factor formed by the launch itself (keep * ~row mask:
        # a product with `keep`, a `bitwise_not`, a cast and a second product were four launches per block and pass)
        scale = keep_rows if rz is not None else (keep if m is not None else None)
        if y_pre:
            out = _OutResRowsFn.apply(out, lo.weight, lo.bias, scale, None, tuple(y_pre))
        elif lo is not None and native.rows_proj_supported(E):
            # the output ResBlock and the dead-row / padded-row factor: one launch
            out = _OutResRowsFn.apply(out, lo.weight, lo.bias, scale)
        elif out_draws is not None:
            # ... with the stack's live nn.Dropout between the ResBlock and the factor: still one launch
            out = _OutResRowsFn.apply(out, lod[0].weight, lod[0].bias, scale, out_draws)
        else:
            out = self._out_stack(out, scale, None)
        return out, weights

    def _attend_core(self, q, k, v, m, rz):
        """short windows, one head: scores, mask, softmax and the weighted sum as one launch (csrc/attn.hip)"""
        if not _fused_core_ok(q, k, self.num_heads, self._drop_active()):
            return None
        out, weights, keep = _AttnCoreFn.apply(q, k, v, m)
        # fully masked queries produce zeros (the kernel already zeroed their weights)
        return self._out_stack(out, keep if m is not None else None, rz), weights

    def _attend_module(self, q, k, v, attn_mask, rz, bsz):
        """the library's batched GEMMs and softmax over the split heads [bsz * heads, len, head_dim]"""
        q_len, k_len = q.shape[1], k.shape[1]
        q = q / math.sqrt(self.head_dim)
        dead_rows = None
        if attn_mask is not None:
            if attn_mask.dim() == 2:
                attn_mask = attn_mask.unsqueeze(0).expand(bsz, -1, -1)
            dead_rows = attn_mask.all(dim=-1)                                 # [bsz, q]: nothing to attend to
            bias = torch.zeros(attn_mask.shape, dtype=q.dtype, device=q.device)
            bias = bias.masked_fill(attn_mask & ~dead_rows.unsqueeze(-1), float('-inf'))   # dead rows stay 0
            scores = torch.baddbmm(bias.repeat(self.num_heads, 1, 1), q, k.transpose(-2, -1))
        else:
            scores = torch.bmm(q, k.transpose(-2, -1))
        weights = torch.softmax(scores, dim=-1)                               # [bsz * heads, q, k]
        if self._drop_active():
            weights = nn.functional.dropout(weights, p=self.dropout)
        out = torch.bmm(weights, v)                                           # [bsz * heads, q, head_dim]

        if self.num_heads > 1:
            weights = weights.view(self.num_heads, bsz, q_len, k_len).mean(0)
            out = out.view(self.num_heads, bsz, q_len, self.head_dim).permute(1, 2, 0, 3).reshape(bsz, q_len, self.embed_dim)
        keep = None
        if dead_rows is not None:   # fully masked queries produce zeros, not NaN
            keep = ~dead_rows
            weights = weights * keep.unsqueeze(-1)
        return self._out_stack(out, keep, rz), weights


# ------------------------------------------------------------------------------------------------
def _kaiming_linear(n, bias):
    lin = nn.Linear(n, n, bias=bias)
    nn.init.kaiming_uniform_(lin.weight.data)
    return lin


class GatedResidualLayer(nn.Module):
    def forward(self, x, y):
        return x + y


class GatedOutputLayer(nn.Module):
    def __init__(self, embed_dim: int):
        super().__init__()
        self.embed_dim = embed_dim
        self.dense = _kaiming_linear(embed_dim, bias=False)

    def forward(self, x, y):
        return x + torch.sigmoid(self.dense(x) * y)


class GatedRecurrentLayer(nn.Module):
    """GRU-style gate (GTrXL): r, z gates from (x, y), candidate from (r*x, y)."""

    def __init__(self, embed_dim: int):
        super().__init__()
        self.embed_dim = embed_dim
        self.dense_x_r = _kaiming_linear(embed_dim, False)
        self.dense_y_r = _kaiming_linear(embed_dim, False)
        self.dense_x_z = _kaiming_linear(embed_dim, True)
        self.dense_y_z = _kaiming_linear(embed_dim, False)
        self.dense_x_g = _kaiming_linear(embed_dim, False)
        self.dense_y_g = _kaiming_linear(embed_dim, False)

    def forward(self, x, y):
        r = torch.sigmoid(self.dense_x_r(x) + self.dense_y_r(y))
        z = torch.sigmoid(self.dense_x_z(x) + self.dense_y_z(y))
        h = torch.tanh(self.dense_x_g(r * x) + self.dense_y_g(y))
        return (1 - z) * x + z * h


class GatedCatLayer(nn.Module):
    def forward(self, x, y):
        return torch.cat([x, y], dim=-1)


# ------------------------------------------------------------------------------------------------
class step_mask_cache:
    """`with step_mask_cache():` — inside, attention blocks reuse the (index / padding / attention) masks they
    built for identical inputs (same tensors, same lengths).  The learner wraps one train step in it: the online,
    the target and the post-update representation pass see the very same window buffers, and the buffers are only
    rewritten between steps (by kernels that do not bump torch's version counters — hence an explicit scope instead
    of version-keyed memoisation)."""
    active = None

    def __enter__(self):
        self._prev = step_mask_cache.active
        step_mask_cache.active = {}
        return self

    def __exit__(self, *exc):
        step_mask_cache.active = self._prev
        return False


_CAUSAL = {}


def _causal_mask(k: int, device):
    """[k, k] bool, True above the diagonal (never written to by its users)"""
    key = (k, str(device))
    m = _CAUSAL.get(key)
    if m is None:
        m = _CAUSAL[key] = torch.triu(torch.ones(k, k, dtype=torch.bool, device=device), diagonal=1)
    return m


def _tkey(t):
    return None if t is None else (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)


def _tail(x, n):
    """x[:, -n:] — x itself when that is all of it (no slice node: its backward is a fill and a copy)"""
    return x if x.shape[1] == n else x[:, -n:]


class EpisodeMultiheadAttentionBlock(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int, pe=None, qkv_dense_depth: int = 0,
                 out_dense_depth: int = 1, dropout: float = 0., gate=None, use_layer_norm: bool = False):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.gate, self.use_layer_norm = gate, use_layer_norm
        self.output_dim = embed_dim
        if use_layer_norm:
            self.layer_norm = nn.LayerNorm(embed_dim)
        self.attn = MultiheadAttention(embed_dim=embed_dim, num_heads=num_heads, pe=pe,
                                       qkv_dense_depth=qkv_dense_depth, out_dense_depth=out_dense_depth,
                                       dropout=dropout)
        if gate == GATE.RESIDUAL:
            self.gatedlayer = GatedResidualLayer()
        elif gate == GATE.OUTPUT:
            self.gatedlayer = GatedOutputLayer(embed_dim)
        elif gate == GATE.RECURRENT:
            self.gatedlayer = GatedRecurrentLayer(embed_dim)
        elif gate == GATE.CAT:
            self.gatedlayer = GatedCatLayer()
            self.output_dim = embed_dim * 2

    def get_attn_mask(self, seq_k_len: int, seq_q_len_only_attend_to_rest_key: int | None = None,
                      key_index=None, key_padding_mask=None, device='cpu'):
        """True = blocked.  Default: causal [k, k].  With `seq_q_len_only_attend_to_rest_key` = q the last
        q positions attend only to themselves and to the earlier ("rest") keys whose index is not
        in their future, and the rest keys only to themselves.  Padded keys are blocked everywhere."""
        if seq_q_len_only_attend_to_rest_key is None:
            mask = _causal_mask(seq_k_len, device)          # constant: built once per (length, device)
        else:
            q = seq_q_len_only_attend_to_rest_key
            rest = seq_k_len - q
            mask = torch.ones(seq_k_len, seq_k_len, dtype=torch.bool, device=device)
            mask[:rest, :rest] = torch.eye(rest, rest, dtype=torch.bool, device=device)
            mask[-q:, -q:] = torch.logical_or(mask[-q:, -q:], ~torch.eye(q, dtype=torch.bool, device=device))
            if key_index is not None:
                mask = mask.repeat(key_index.shape[0], 1, 1)
                q_idx = key_index[:, -q:].unsqueeze(-1)             # [batch, q, 1]
                rest_idx = key_index[:, :rest].unsqueeze(1)         # [batch, 1, rest]
                mask[:, -q:, :rest] = ~(q_idx >= rest_idx)
        if key_padding_mask is not None:      # (a 2-D mask broadcasts over the batch: same values as repeat + or)
            mask = torch.logical_or(mask if mask.dim() == 3 else mask.unsqueeze(0), key_padding_mask.unsqueeze(1))
        return mask

    def forward(self, key, seq_q_len: int, cut_query: bool = True, query_only_attend_to_rest_key: bool = False,
                key_index=None, key_padding_mask=None):
        """key [batch, k, E]; key_index / key_padding_mask may be SHORTER than k (they describe the
        newest positions; the older ones get index -1 / the first mask value)
        -> (output [batch, q or k, output_dim], weights [batch, q or k, k])"""
        seq_k_len = key.shape[1]
        residual_src = _tail(key, seq_q_len) if cut_query else key
        if self.use_layer_norm:
            key = self.layer_norm(key)

        cache = step_mask_cache.active
        ck = None if cache is None else ('masks', seq_k_len, seq_q_len, query_only_attend_to_rest_key,
                                         _tkey(key_index), _tkey(key_padding_mask), str(key.device))
        if ck is not None and ck in cache:
            key_index, key_padding_mask, attn_mask = cache[ck]
        else:
            if key_index is not None:
                short = seq_k_len - key_index.shape[1]
                assert short >= 0
                if not (query_only_attend_to_rest_key or self.attn.pe):
                    key_index = None        # read by the rest-key mask and the positional encodings only
                elif short:
                    key_index = torch.cat([key_index.new_full((key_index.shape[0], short), -1), key_index], dim=1)
            if key_padding_mask is not None:
                short = seq_k_len - key_padding_mask.shape[1]
                assert short >= 0
                if short:
                    key_padding_mask = torch.cat([key_padding_mask[:, :1].expand(-1, short), key_padding_mask], dim=1)
            attn_mask = self.get_attn_mask(seq_k_len, seq_q_len if query_only_attend_to_rest_key else None,
                                           key_index=key_index, key_padding_mask=key_padding_mask, device=key.device)
            if ck is not None:
                cache[ck] = (key_index, key_padding_mask, attn_mask)
        query_index = key_index
        query = key
        if cut_query:
            query = _tail(key, seq_q_len)
            if query_index is not None:
                query_index = query_index[:, -seq_q_len:]
            attn_mask = attn_mask[-seq_q_len:] if attn_mask.dim() == 2 else attn_mask[:, -seq_q_len:]

        # padded positions produce zeros: without a gate in between, the attention layer zeroes those rows itself
        # (inside its fused launch when it has one)
        row_mask = None
        if key_padding_mask is not None and self.gate is None:
            row_mask = key_padding_mask[:, -query.shape[1]:]
        output, weights = self.attn(query, key, key, query_index=query_index, key_index=key_index,
                                    attn_mask=attn_mask, out_row_mask=row_mask)
        if self.gate is not None:
            gate_params = _fused_gate_params(self, residual_src, output, key_padding_mask)
            if gate_params is not None:
                # the gate and the padded-row factor: one launch per pass (csrc/rows_gate.hip), the mask read where it lies
                row_zero = None if key_padding_mask is None else key_padding_mask[:, -output.shape[1]:]
                return _GateRowsFn.apply(self.gate.value, residual_src, output, row_zero, *gate_params), weights
            output = self.gatedlayer(residual_src, output)
            if key_padding_mask is not None:
                output = output * (~key_padding_mask[:, -output.shape[1]:]).to(output.dtype).unsqueeze(-1)
        return output, weights


class EpisodeMultiheadAttention(nn.Module):
    def __init__(self, embed_dim: int, num_layers: int = 2, num_heads=1, pe=False, qkv_dense_depth=0,
                 out_dense_depth=1, dropout=0., gate=None, use_layer_norm=False):
        super().__init__()
        self.num_layers = num_layers

        def per_layer(v):
            v = v if isinstance(v, list) else [v] * num_layers
            assert len(v) == num_layers
            return v

        num_heads, pe, qkv_dense_depth, out_dense_depth, dropout, gate, use_layer_norm = map(
            per_layer, (num_heads, pe, qkv_dense_depth, out_dense_depth, dropout, gate, use_layer_norm))

        self._attn_list = nn.ModuleList()
        dim = embed_dim
        for i in range(num_layers):
            block = EpisodeMultiheadAttentionBlock(dim, num_heads[i], pe=pe[i], qkv_dense_depth=qkv_dense_depth[i],
                                                   out_dense_depth=out_dense_depth[i], dropout=dropout[i],
                                                   gate=gate[i], use_layer_norm=use_layer_norm[i])
            self._attn_list.append(block)
            dim = block.output_dim
        self._output_dim_list = [b.output_dim for b in self._attn_list]
        self.output_dim = dim
        self.output_hidden_state_dim = sum(self._output_dim_list[:-1]) if num_layers > 1 else 1

    def forward(self, key, seq_q_len: int = 1, cut_query: bool = True, hidden_state=None,
                is_prev_hidden_state: bool = False, query_only_attend_to_rest_key: bool = False,
                key_index=None, key_padding_mask=None):
        """-> (encoded [batch, q or k, output_dim], next_hidden_state [batch, q, sum(dims[:-1])],
        list of per-layer attention weights)"""
        seq_k_len = key.shape[1]
        assert seq_q_len <= seq_k_len
        blocks, L = self._attn_list, self.num_layers
        kw = dict(query_only_attend_to_rest_key=query_only_attend_to_rest_key, key_index=key_index,
                  key_padding_mask=key_padding_mask)
        next_hidden, weights = [], []

        def run(block, k, cut):
            out, w = block(k, seq_q_len, cut_query=cut, **kw)
            weights.append(w)
            return out

        if hidden_state is None:
            k = key
            for block in blocks[:-1]:
                k = run(block, k, False)
                next_hidden.append(_tail(k, seq_q_len))
            out = run(blocks[-1], k, cut_query)
        else:
            states = hidden_state.split(self._output_dim_list[:-1], dim=-1) if L > 1 else ()
            if not is_prev_hidden_state:
                out = run(blocks[0], key, False if L > 1 else cut_query)
                for i, block in enumerate(blocks[1:]):
                    next_hidden.append(_tail(out, seq_q_len))
                    out = run(block, torch.cat([states[i], out], dim=1), False if i != L - 2 else cut_query)
            else:
                out = run(blocks[0], key, False)
                next_hidden.append(_tail(out, seq_q_len))
                if L == 1 and cut_query:
                    out = _tail(out, seq_q_len)
                for i, block in enumerate(blocks[1:-1]):
                    out = run(block, torch.cat([states[i], _tail(out, seq_k_len)], dim=1), False)
                    next_hidden.append(_tail(out, seq_q_len))
                if L > 1:
                    out = run(blocks[-1], torch.cat([states[-1], _tail(out, seq_k_len)], dim=1), cut_query)

        if L > 1:
            return out, (next_hidden[0] if len(next_hidden) == 1 else torch.cat(next_hidden, dim=-1)), weights
        return out, torch.zeros(key.shape[0], seq_q_len, 1, device=key.device), weights
