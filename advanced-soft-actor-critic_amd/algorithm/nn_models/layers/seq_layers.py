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
interchange.  The math runs as batched GEMMs + softmax on PyTorch-ROCm (MFMA through
rocBLAS/hipBLASLt); nothing here synchronises with the host, so an attention representation stays
inside the captured train step.

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

from algorithm.param_grads import deliver_packed, direct_enabled, direct_skips, flat_grad_alias, queue_param_grads

from .linear_layers import LinearLayers

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


class _AttnCoreFn(torch.autograd.Function):
    """scores / mask / softmax / weighted sum of one attention head as one launch per pass
    (`asac_attention_forward/backward`, csrc/attn.hip) -> (out, weights * keep, keep)"""

    @staticmethod
    def forward(ctx, q, k, v, mask):
        from asac_amd import native
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Lq, D = q.shape
        out = torch.empty(B, Lq, D, dtype=q.dtype, device=q.device)
        weights = torch.empty(B, Lq, k.shape[1], dtype=q.dtype, device=q.device)
        keep = torch.empty(B, Lq, dtype=q.dtype, device=q.device)
        native.attention_forward(q, k, v, mask, out, weights, keep)
        ctx.save_for_backward(q, k, v, weights)
        ctx.mark_non_differentiable(keep)
        ctx.set_materialize_grads(False)
        return out, weights, keep

    @staticmethod
    def backward(ctx, g_out, g_w, _g_keep):
        from asac_amd import native
        q, k, v, weights = ctx.saved_tensors
        if g_out is None and g_w is None:
            return None, None, None, None
        if g_out is None:
            g_out = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
        g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        native.attention_backward(q, k, v, weights, g_out.contiguous(), None if g_w is None else g_w.contiguous(),
                                  g_q, g_k, g_v)
        return g_q, g_k, g_v, None


class _AttnMhFn(torch.autograd.Function):
    """scores / mask / softmax / weighted sum of ALL heads and the head-averaged weights as one MFMA launch per pass
    (`asac_attention_mh_forward/backward`, csrc/attn_mh.hip): q, k, v [B, L, heads * d] -> (out [B, Lq, heads * d] with the
    heads concatenated, mean-over-heads weights * keep, keep)"""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, row_zero=None):
        """`row_zero` bool [B, Lq]: the caller's padded positions — the fourth result is then keep * ~row_zero, the one
        factor the caller's output needs (else it is `keep` again)"""
        from asac_amd import native
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Lq, E = q.shape
        Lk = k.shape[1]
        out = torch.empty(B, Lq, E, dtype=q.dtype, device=q.device)
        weights = torch.empty(B, Lq, Lk, dtype=q.dtype, device=q.device)
        keep = torch.empty(B, Lq, dtype=q.dtype, device=q.device)
        keep_rows = torch.empty(B, Lq, dtype=q.dtype, device=q.device) if row_zero is not None else keep
        p_heads = torch.empty(B, heads, Lq, Lk, dtype=q.dtype, device=q.device) if any(ctx.needs_input_grad[:3]) else None
        native.attention_mh_forward(q, k, v, mask, heads, out, weights, keep, p_heads,
                                    None if row_zero is None else row_zero.contiguous(),
                                    keep_rows if row_zero is not None else None)
        if p_heads is not None:
            ctx.save_for_backward(q, k, v, p_heads, *([mask] if mask is not None else []))
        ctx.heads, ctx.has_mask = heads, mask is not None
        ctx.mark_non_differentiable(keep, keep_rows)
        ctx.set_materialize_grads(False)
        return out, weights, keep, keep_rows

    @staticmethod
    def backward(ctx, g_out, g_w, _g_keep, _g_keep_rows=None):
        from asac_amd import native
        q, k, v, p_heads, *rest = ctx.saved_tensors
        if g_out is None and g_w is None:
            return None, None, None, None, None, None
        if g_out is None:
            g_out = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
        g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        native.attention_mh_backward(q, k, v, rest[0] if ctx.has_mask else None, ctx.heads, p_heads, g_out.contiguous(),
                                     None if g_w is None else g_w.contiguous(), g_q, g_k, g_v)
        return g_q, g_k, g_v, None, None, None


class _AttnMhDropFn(torch.autograd.Function):
    """`_AttnMhFn` with dropout of the softmax weights inside both launches (`asac_attention_mh_dropout_forward/backward`):
    the weights returned are the DROPPED ones' head mean, as the reference returns them.  `draws` = (p, seed, instance id,
    state, used): the module instance's stream of draws, its device state and this call's `used` record — the backward
    launch reads the counter from it on the device, so a captured pair stays in step on every replay."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, row_zero, draws):
        from asac_amd import native
        p, seed, instance, state, used = draws
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Lq, E = q.shape
        Lk = k.shape[1]
        out = torch.empty(B, Lq, E, dtype=q.dtype, device=q.device)
        weights = torch.empty(B, Lq, Lk, dtype=q.dtype, device=q.device)
        keep = torch.empty(B, Lq, dtype=q.dtype, device=q.device)
        keep_rows = torch.empty(B, Lq, dtype=q.dtype, device=q.device) if row_zero is not None else keep
        p_heads = torch.empty(B, heads, Lq, Lk, dtype=q.dtype, device=q.device) if any(ctx.needs_input_grad[:3]) else None
        native.attention_mh_dropout_forward(q, k, v, mask, heads, out, weights, keep, p_heads,
                                            None if row_zero is None else row_zero.contiguous(),
                                            keep_rows if row_zero is not None else None, p, seed, instance, state, used)
        if p_heads is not None:
            ctx.save_for_backward(q, k, v, p_heads, used, *([mask] if mask is not None else []))
        ctx.heads, ctx.has_mask, ctx.draws = heads, mask is not None, (p, seed, instance)
        ctx.mark_non_differentiable(keep, keep_rows)
        ctx.set_materialize_grads(False)
        return out, weights, keep, keep_rows

    @staticmethod
    def backward(ctx, g_out, g_w, _g_keep, _g_keep_rows=None):
        from asac_amd import native
        q, k, v, p_heads, used, *rest = ctx.saved_tensors
        if g_out is None and g_w is None:
            return None, None, None, None, None, None, None
        if g_out is None:
            g_out = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
        g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        native.attention_mh_dropout_backward(q, k, v, rest[0] if ctx.has_mask else None, ctx.heads, p_heads, g_out.contiguous(),
                                             None if g_w is None else g_w.contiguous(), g_q, g_k, g_v, *ctx.draws, used)
        return g_q, g_k, g_v, None, None, None, None


class _AttnProjFn(torch.autograd.Function):
    """`_AttnCoreFn` with the q / k / v Linear projections — and, with 8 parameters, the output ResBlock
    y = (GELU(Wo o + bo) + o) * keep — on chip (`asac_attention_proj_*`): x_q, x_k in, (out, weights * keep, keep) out.
    The parameter gradients are added straight into their `.grad` views when those are consecutive slices of one
    buffer (the learner's flat gradient buffer), else returned."""

    @staticmethod
    def forward(ctx, xq, xk, mask, row_zero, *params):
        from asac_amd import native
        xk = xk if xk.stride(-1) == 1 else xk.contiguous()
        ctx.tail = 0
        if isinstance(xq, int):      # the queries are the last `xq` rows of x_k: one gradient, no slice node
            ctx.tail = xq
            xq = xk[:, -xq:]
        xq = xq if xq.stride(-1) == 1 else xq.contiguous()
        B, Lq, E = xq.shape
        pd = [t.detach().contiguous() for t in params]
        out = torch.empty(B, Lq, E, dtype=xq.dtype, device=xq.device)
        weights = torch.empty(B, Lq, xk.shape[1], dtype=xq.dtype, device=xq.device)
        keep = torch.empty(B, Lq, dtype=xq.dtype, device=xq.device)
        attn_out = torch.empty(B, Lq, E, dtype=xq.dtype, device=xq.device) if len(params) == 8 else None
        native.attention_proj_forward(xq, xk, pd, mask, out, weights, keep, attn_out, row_zero)
        ctx.save_for_backward(xk if ctx.tail else xq, xk, weights, keep, *([attn_out] if attn_out is not None else []))
        ctx.params, ctx.row_zero = params, row_zero
        ctx.mark_non_differentiable(keep)
        ctx.set_materialize_grads(False)
        return out, weights, keep

    @staticmethod
    def backward(ctx, g_out, g_w, _g_keep):
        from asac_amd import native
        xq, xk, weights, keep, *rest = ctx.saved_tensors
        attn_out = rest[0] if rest else None
        params, tail = ctx.params, ctx.tail
        if tail:
            xq = xk[:, -tail:]
        if g_out is None and g_w is None:
            return (None,) * (4 + len(params))
        if g_out is None:
            g_out = torch.zeros(xq.shape[0], xq.shape[1], xq.shape[2], dtype=xq.dtype, device=xq.device)
        B, Lq, E = xq.shape
        Lk = xk.shape[1]
        # (tail: the queries are the last rows of the keys — the launch adds their gradient into those rows of g_xk)
        g_xq = None if tail else torch.empty(B, Lq, E, dtype=xq.dtype, device=xq.device)
        g_xk = torch.empty(B, Lk, E, dtype=xq.dtype, device=xq.device)
        if g_out.stride(2) != 1:
            g_out = g_out.contiguous()
        ws = torch.empty(native.attention_proj_workspace(B, Lq, Lk, E), dtype=xq.dtype, device=xq.device)
        pd = [t.detach().contiguous() for t in params]
        gw = None if g_w is None else g_w.contiguous()
        slabs, n = native.attention_proj_partials(ws, E, len(params) == 8)
        grads = deliver_packed(
            params, flat_grad_alias(params) if direct_enabled() else None, n,
            lambda out, mode: native.attention_proj_backward(xq, xk, pd, weights, g_out, gw, g_xq, g_xk, out, mode, ws, keep,
                                                             attn_out, ctx.row_zero),
            lambda: (ws, slabs, 16, n, n))
        return (g_xq, g_xk, None, None, *grads)


def _rows_param_grads(ctx_needs, params, g2, x2, jobs=None):
    """weight / bias gradient of one Linear (bias: None without one) from its output gradient rows g2 and input rows x2
    (`asac_xty`): added straight into the `.grad` views under the learner's direct mode, else returned.  With a list `jobs` the
    returned product is not launched but appended to it: the caller has several and runs them together (`_run_xty_jobs`)"""
    from asac_amd import native
    weight, bias = params
    held = [p for p in params if p is not None]
    if not any(ctx_needs) or direct_skips(*held):
        return None, None
    if direct_enabled() and all(p.grad is not None and p.grad.is_contiguous() for p in held):
        queue_param_grads(g2, x2, weight.grad, None if bias is None else bias.grad)
        return None, None
    gw, gb = torch.empty_like(weight), None if bias is None else torch.empty_like(bias)
    if jobs is None:
        native.xty(g2, x2, gw, gb)
    else:
        jobs.append((g2, x2, gw, gb))
    return gw, gb


def _run_xty_jobs(jobs):
    """the products `_rows_param_grads` left in `jobs`, up to four a launch pair (`asac_xty_multi`: their outputs are distinct)"""
    from asac_amd import native
    for i in range(0, len(jobs), 4):
        if len(jobs[i:i + 4]) == 1:
            native.xty(*jobs[i])
        else:
            native.xty_multi(jobs[i:i + 4])


class _QkvRowsFn(torch.autograd.Function):
    """`q_proj(x[:, -tail:]), k_proj(x), v_proj(x)` — three nn.Linear(E, E) over the rows of a window batch — as ONE MFMA
    launch; backward: the input gradient of the three as one launch, the parameter gradients as products over the rows
    (`asac_rows_proj_*`, csrc/rows_proj.hip; `asac_xty`)"""

    @staticmethod
    def forward(ctx, x, tail, wq, bq, wk, bk, wv, bv):
        from asac_amd import native
        if x.stride(2) != 1 or (x.stride(0) | x.stride(1) | (x.data_ptr() >> 2)) & 3:
            x = x.contiguous()
        B, L, E = x.shape
        q = torch.empty(B, tail, E, dtype=x.dtype, device=x.device)
        k, v = torch.empty(B, L, E, dtype=x.dtype, device=x.device), torch.empty(B, L, E, dtype=x.dtype, device=x.device)
        native.rows_proj_forward(x, [wq.detach(), wk.detach(), wv.detach()], [bq.detach(), bk.detach(), bv.detach()],
                                 [tail, L, L], [q, k, v])
        ctx.save_for_backward(x)
        ctx.tail, ctx.params = tail, (wq, bq, wk, bk, wv, bv)
        return q, k, v

    @staticmethod
    def backward(ctx, gq, gk, gv):
        from asac_amd import native
        x, = ctx.saved_tensors
        B, L, E = x.shape
        wq, bq, wk, bk, wv, bv = ctx.params
        grads = [g.contiguous() for g in (gq, gk, gv)]
        tails = [ctx.tail, L, L]
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(B, L, E, dtype=x.dtype, device=x.device)
            native.rows_proj_backward(grads, tails, [wq.detach(), wk.detach(), wv.detach()], gx)
        x2 = x.reshape(-1, E)
        xq2 = x2 if ctx.tail == L else x[:, -ctx.tail:].reshape(-1, E)
        out = [gx, None]
        for j, (g, xin) in enumerate(zip(grads, (xq2, x2, x2))):
            out.extend(_rows_param_grads(ctx.needs_input_grad[2 + 2 * j:4 + 2 * j], ctx.params[2 * j:2 * j + 2],
                                         g.view(-1, E), xin))
        return tuple(out)


class _QkvRopeRowsFn(torch.autograd.Function):
    """`_QkvRowsFn` with `self.rope(index[:, -tail:], index, q, k)` behind it in the same launch, and the un-rotation of the
    gradients in front of the backward launch's products (`asac_rows_proj_rope_*`, csrc/rows_proj.hip); the parameter gradients
    are products of the un-rotated gradients the backward launch writes.  `tables`: `_fused_rope_tables`"""

    @staticmethod
    def forward(ctx, x, tail, index, kind, tables, wq, bq, wk, bk, wv, bv):
        from asac_amd import native
        if x.stride(2) != 1 or (x.stride(0) | x.stride(1) | (x.data_ptr() >> 2)) & 3:
            x = x.contiguous()
        B, L, E = x.shape
        q = torch.empty(B, tail, E, dtype=x.dtype, device=x.device)
        k, v = torch.empty(B, L, E, dtype=x.dtype, device=x.device), torch.empty(B, L, E, dtype=x.dtype, device=x.device)
        native.rows_proj_rope_forward(kind, tables, index, x, [wq.detach(), wk.detach(), wv.detach()],
                                      [bq.detach(), bk.detach(), bv.detach()], [tail, L, L], [q, k, v])
        ctx.save_for_backward(x, index)
        ctx.tail, ctx.kind, ctx.tables, ctx.params = tail, kind, tables, (wq, bq, wk, bk, wv, bv)
        return q, k, v

    @staticmethod
    def backward(ctx, gq, gk, gv):
        from asac_amd import native
        x, index = ctx.saved_tensors
        B, L, E = x.shape
        wq, bq, wk, bk, wv, bv = ctx.params
        grads = [g.contiguous() for g in (gq, gk, gv)]
        plain = [torch.empty_like(grads[0]), torch.empty_like(grads[1])]
        gx = torch.empty(B, L, E, dtype=x.dtype, device=x.device)
        native.rows_proj_rope_backward(ctx.kind, ctx.tables, index, grads, [ctx.tail, L, L],
                                       [wq.detach(), wk.detach(), wv.detach()], gx, plain)
        x2 = x.reshape(-1, E)
        xq2 = x2 if ctx.tail == L else x[:, -ctx.tail:].reshape(-1, E)
        out = [gx if ctx.needs_input_grad[0] else None, None, None, None, None]
        for j, (g, xin) in enumerate(zip((*plain, grads[2]), (xq2, x2, x2))):
            out.extend(_rows_param_grads(ctx.needs_input_grad[5 + 2 * j:7 + 2 * j], ctx.params[2 * j:2 * j + 2],
                                         g.view(-1, E), xin))
        return tuple(out)


class _QkvDenseDropFn(torch.autograd.Function):
    """`q_proj(x[:, -tail:]), k_proj(x), v_proj(x)` where each stack is ResBlock(E, E) -> LIVE nn.Dropout(p) -> nn.Linear(E, E),
    as ONE MFMA launch per pass (`asac_rows_dense_proj_dropout_*`, csrc/rows_proj.hip).  `draws` = (p, seed, instance id, state,
    used) of the module's 'qkv' site: the masks are drawn on the device and regenerated by the backward from the counter this
    call's `used` holds.  `params`: (ResBlock weight, bias, Linear weight, bias) of q, k, v.  The twelve parameter gradients are
    products over the rows (`asac_xty`): of the pre-activation gradients with x, of the output gradients with the dropped hidden
    rows the forward wrote."""

    @staticmethod
    def forward(ctx, x, tail, draws, *params):
        from asac_amd import native
        p, seed, instance, state, used = draws
        if x.stride(2) != 1 or (x.stride(0) | x.stride(1) | (x.data_ptr() >> 2)) & 3:
            x = x.contiguous()
        B, L, E = x.shape
        tails = [tail, L, L]
        new = lambda: [torch.empty(B, t, E, dtype=x.dtype, device=x.device) for t in tails]      # noqa: E731
        outs, pres, hiddens = new(), new(), new()
        pd = [t.detach() for t in params]
        native.rows_dense_proj_dropout_forward(x, pd[0::4], pd[1::4], pd[2::4], pd[3::4], tails, outs, pres, hiddens, p, seed,
                                               instance, state, used)
        ctx.save_for_backward(x, used, *pres, *hiddens)
        ctx.tail, ctx.params, ctx.draws = tail, params, (p, seed, instance)
        return tuple(outs)

    @staticmethod
    def backward(ctx, gq, gk, gv):
        from asac_amd import native
        x, used, *saved = ctx.saved_tensors
        pres, hiddens = saved[:3], saved[3:]
        B, L, E = x.shape
        params, tails = ctx.params, [ctx.tail, L, L]
        grads = [torch.zeros_like(pre) if g is None else g.contiguous() for g, pre in zip((gq, gk, gv), pres)]
        gx = torch.empty(B, L, E, dtype=x.dtype, device=x.device)
        gpres = [torch.empty_like(pre) for pre in pres]
        native.rows_dense_proj_dropout_backward(grads, list(pres), tails, [t.detach() for t in params[0::4]],
                                                [t.detach() for t in params[2::4]], gx, gpres, *ctx.draws, used)
        x2 = x.reshape(-1, E)
        xq2 = x2 if ctx.tail == L else x[:, -ctx.tail:].reshape(-1, E)
        out, jobs = [gx if ctx.needs_input_grad[0] else None, None, None], []
        for j, xin in enumerate((xq2, x2, x2)):
            at = 3 + 4 * j
            out.extend(_rows_param_grads(ctx.needs_input_grad[at:at + 2], params[4 * j:4 * j + 2], gpres[j].view(-1, E), xin, jobs))
            out.extend(_rows_param_grads(ctx.needs_input_grad[at + 2:at + 4], params[4 * j + 2:4 * j + 4], grads[j].view(-1, E),
                                         hiddens[j].view(-1, E), jobs))
        _run_xty_jobs(jobs)
        return tuple(out)


class _RopeFn(torch.autograd.Function):
    """`self.rope(q_index, k_index, q, k)` as one launch per pass for both tensors (`asac_rope_*`, csrc/rope.hip)"""

    @staticmethod
    def forward(ctx, q, k, q_index, k_index, kind, tables):
        from asac_amd import native
        q, k = (t if t.stride(2) == 1 else t.contiguous() for t in (q, k))
        out_q, out_k = torch.empty(q.shape, dtype=q.dtype, device=q.device), torch.empty(k.shape, dtype=k.dtype, device=k.device)
        native.rope_forward(kind, tables, q, k, q_index, k_index, out_q, out_k)
        ctx.save_for_backward(q_index, k_index)
        ctx.kind, ctx.tables = kind, tables
        return out_q, out_k

    @staticmethod
    def backward(ctx, gq, gk):
        from asac_amd import native
        q_index, k_index = ctx.saved_tensors
        gq, gk = (g if g.stride(2) == 1 else g.contiguous() for g in (gq, gk))
        out_q, out_k = torch.empty(gq.shape, dtype=gq.dtype, device=gq.device), torch.empty(gk.shape, dtype=gk.dtype, device=gk.device)
        native.rope_backward(ctx.kind, ctx.tables, gq, gk, q_index, k_index, out_q, out_k)
        return out_q, out_k, None, None, None, None


def _fused_rope_tables(module, query, key, query_index, key_index):
    """the tables `_RopeFn` / `_QkvRopeRowsFn` read for the rotary encoding of `module`, or None: `self.rope` runs as module
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
    from asac_amd import native
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


class _QkvAttnMhFn(torch.autograd.Function):
    """`_QkvRowsFn` and `_AttnMhFn` as ONE forward launch for windows of <= 16 positions (`asac_attention_mh_proj_forward`:
    the projections run in front of the scores inside the launch); backward: the core's launch, then the projections' input
    gradient and parameter-gradient products as in `_QkvRowsFn`"""

    @staticmethod
    def forward(ctx, x, tail, wq, bq, wk, bk, wv, bv, mask, heads, row_zero=None, out_block=None):
        """`out_block` = (weight, bias) of the output ResBlock: it runs behind the core in the same launch and two more tensors
        come back (y, pre) — non-differentiable HERE: `_OutResSavedFn` turns them into the block's output and carries its
        backward"""
        from asac_amd import native
        if x.stride(2) != 1 or (x.stride(0) | x.stride(1) | (x.data_ptr() >> 2)) & 3:
            x = x.contiguous()
        B, L, E = x.shape
        dd = dict(dtype=x.dtype, device=x.device)
        q, k, v = torch.empty(B, tail, E, **dd), torch.empty(B, L, E, **dd), torch.empty(B, L, E, **dd)
        out, weights, keep = torch.empty(B, tail, E, **dd), torch.empty(B, tail, L, **dd), torch.empty(B, tail, **dd)
        keep_rows = torch.empty(B, tail, **dd) if row_zero is not None else keep
        need = any(ctx.needs_input_grad[i] for i in (0, 2, 3, 4, 5, 6, 7))
        p_heads = torch.empty(B, heads, tail, L, **dd) if need else None
        y = pre = None
        if out_block is not None:
            y, pre = torch.empty(B, tail, E, **dd), torch.empty(B, tail, E, **dd)
        native.attention_mh_proj_forward(x, [wq.detach(), wk.detach(), wv.detach()], [bq.detach(), bk.detach(), bv.detach()],
                                         mask, heads, q, k, v, out, weights, keep, p_heads,
                                         None if row_zero is None else (row_zero if row_zero.stride(-1) == 1 else row_zero.contiguous()),
                                         keep_rows if row_zero is not None else None,
                                         *(() if out_block is None else (out_block[0].detach().contiguous(),
                                                                         out_block[1].detach().contiguous(), y, pre)))
        if need:
            ctx.save_for_backward(x, q, k, v, p_heads, *([mask] if mask is not None else []))
        ctx.tail, ctx.heads, ctx.has_mask, ctx.params = tail, heads, mask is not None, (wq, bq, wk, bk, wv, bv)
        ctx.set_materialize_grads(False)
        if out_block is None:
            ctx.mark_non_differentiable(keep, keep_rows)
            return out, weights, keep, keep_rows
        ctx.mark_non_differentiable(keep, keep_rows, y, pre)
        return out, weights, keep, keep_rows, y, pre

    @staticmethod
    def backward(ctx, g_out, g_w, _g_keep, _g_keep_rows=None, _g_y=None, _g_pre=None):
        from asac_amd import native
        if g_out is None and g_w is None:
            return (None,) * 12
        x, q, k, v, p_heads, *rest = ctx.saved_tensors
        B, L, E = x.shape
        if g_out is None:
            g_out = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
        g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        native.attention_mh_backward(q, k, v, rest[0] if ctx.has_mask else None, ctx.heads, p_heads, g_out.contiguous(),
                                     None if g_w is None else g_w.contiguous(), g_q, g_k, g_v)
        wq, bq, wk, bk, wv, bv = ctx.params
        grads, tails = [g_q, g_k, g_v], [ctx.tail, L, L]
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(B, L, E, dtype=x.dtype, device=x.device)
            native.rows_proj_backward(grads, tails, [wq.detach(), wk.detach(), wv.detach()], gx)
        x2 = x.reshape(-1, E)
        xq2 = x2 if ctx.tail == L else x[:, -ctx.tail:].reshape(-1, E)
        out = [gx, None]
        for j, (g, xin) in enumerate(zip(grads, (xq2, x2, x2))):
            out.extend(_rows_param_grads(ctx.needs_input_grad[2 + 2 * j:4 + 2 * j], ctx.params[2 * j:2 * j + 2],
                                         g.view(-1, E), xin))
        return (*out, None, None, None, None)


class _AttnBlockFn(torch.autograd.Function):
    """The whole attention block for windows of <= 16 positions — q / k / v projections, core, output ResBlock with the
    dead-row / padded-row factor — as ONE launch forward (`asac_attention_mh_proj_forward`) and ONE backward
    (`asac_attention_mh_block_backward`), plus the four parameter-gradient products (`asac_xty`, queued)"""

    @staticmethod
    def forward(ctx, x, tail, wq, bq, wk, bk, wv, bv, wo, bo, mask, heads, row_zero, scaled):
        from asac_amd import native
        if x.stride(2) != 1 or (x.stride(0) | x.stride(1) | (x.data_ptr() >> 2)) & 3:
            x = x.contiguous()
        B, L, E = x.shape
        dd = dict(dtype=x.dtype, device=x.device)
        q, k, v = torch.empty(B, tail, E, **dd), torch.empty(B, L, E, **dd), torch.empty(B, L, E, **dd)
        out, weights, keep = torch.empty(B, tail, E, **dd), torch.empty(B, tail, L, **dd), torch.empty(B, tail, **dd)
        keep_rows = torch.empty(B, tail, **dd) if row_zero is not None else keep
        need = any(ctx.needs_input_grad[i] for i in (0, 2, 3, 4, 5, 6, 7, 8, 9))
        p_heads = torch.empty(B, heads, tail, L, **dd) if need else None
        y, pre = torch.empty(B, tail, E, **dd), torch.empty(B, tail, E, **dd)
        native.attention_mh_proj_forward(x, [wq.detach(), wk.detach(), wv.detach()], [bq.detach(), bk.detach(), bv.detach()],
                                         mask, heads, q, k, v, out, weights, keep, p_heads,
                                         None if row_zero is None else (row_zero if row_zero.stride(-1) == 1 else row_zero.contiguous()),
                                         keep_rows if row_zero is not None else None,
                                         wo.detach().contiguous(), bo.detach().contiguous(), y, pre)
        if need:
            # (`scaled`: the block's output was multiplied by keep_rows — with a row mask — or by keep — with an attention mask)
            ctx.save_for_backward(x, q, k, v, p_heads, out, pre, *([keep_rows] if scaled else []), *([mask] if mask is not None else []))
        ctx.tail, ctx.heads, ctx.has_mask, ctx.scaled = tail, heads, mask is not None, scaled
        ctx.params = (wq, bq, wk, bk, wv, bv, wo, bo)
        ctx.mark_non_differentiable(keep, keep_rows)
        ctx.set_materialize_grads(False)
        return y, weights, keep, keep_rows

    @staticmethod
    def backward(ctx, g_y, g_w, _g_keep, _g_keep_rows=None):
        from asac_amd import native
        if g_y is None and g_w is None:
            return (None,) * 14
        x, q, k, v, p_heads, out, pre, *rest = ctx.saved_tensors
        scale = rest.pop(0) if ctx.scaled else None
        mask = rest[0] if ctx.has_mask else None
        B, L, E = x.shape
        if g_y is None:
            g_y = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
        wq, bq, wk, bk, wv, bv, wo, bo = ctx.params
        g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        g_pre, g_x = torch.empty_like(pre), torch.empty(B, L, E, dtype=x.dtype, device=x.device)
        if g_y.stride(2) != 1 or (g_y.stride(0) | g_y.stride(1) | (g_y.data_ptr() >> 2)) & 3:
            g_y = g_y.contiguous()      # (otherwise a slice — the gradient of a concatenation's part — is read in place)
        native.attention_mh_block_backward(q, k, v, mask, ctx.heads, p_heads, g_y, pre,
                                           None if scale is None else scale.contiguous(), wo.detach().contiguous(),
                                           None if g_w is None else g_w.contiguous(),
                                           [wq.detach(), wk.detach(), wv.detach()], g_q, g_k, g_v, g_pre, g_x)
        x2 = x.reshape(-1, E)
        xq2 = x2 if ctx.tail == L else x[:, -ctx.tail:].reshape(-1, E)
        grads = [g_x if ctx.needs_input_grad[0] else None, None]
        # (the output block's product first: the order the three-launch form queues them in)
        go = _rows_param_grads(ctx.needs_input_grad[8:10], (wo, bo), g_pre.view(-1, E), out.view(-1, E))
        for j, (g, xin) in enumerate(zip((g_q, g_k, g_v), (xq2, x2, x2))):
            grads.extend(_rows_param_grads(ctx.needs_input_grad[2 + 2 * j:4 + 2 * j], ctx.params[2 * j:2 * j + 2], g.view(-1, E), xin))
        return (*grads, *go, None, None, None, None)


class _OutResRowsFn(torch.autograd.Function):
    """`(x + gelu(linear(x))) * row_scale[..., None]` — the output ResBlock of an attention layer and its dead-row / padded-row
    factor — as one MFMA launch per pass (`asac_rows_resblock_*`, csrc/rows_proj.hip); the parameter gradients from `asac_xty`"""

    @staticmethod
    def forward(ctx, x, weight, bias, row_scale):
        from asac_amd import native
        x2 = x.reshape(-1, x.shape[-1])
        if x2.stride(1) != 1 or (x2.stride(0) | (x2.data_ptr() >> 2)) & 3:
            x2 = x2.contiguous()
        y, pre = torch.empty(x2.shape, dtype=x.dtype, device=x.device), torch.empty(x2.shape, dtype=x.dtype, device=x.device)
        sc = None if row_scale is None else row_scale.reshape(-1).contiguous()
        native.rows_resblock_forward(x2, weight.detach(), bias.detach(), sc, y, pre)
        ctx.save_for_backward(x2, pre, *([sc] if sc is not None else []))
        ctx.params, ctx.lead = (weight, bias), x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        from asac_amd import native
        x2, pre, *rest = ctx.saved_tensors
        weight, bias = ctx.params
        gy2 = gy.reshape(x2.shape).contiguous()
        gx, gpre = torch.empty_like(pre), torch.empty_like(pre)
        native.rows_resblock_backward(gy2, pre, weight.detach(), rest[0] if rest else None, gx, gpre)
        gw, gb = _rows_param_grads(ctx.needs_input_grad[1:3], ctx.params, gpre, x2)
        return gx.view(ctx.lead), gw, gb, None


class _OutResDropRowsFn(torch.autograd.Function):
    """`_OutResRowsFn` with the output stack's LIVE nn.Dropout(p) between the ResBlock and the row factor, inside both launches
    (`asac_rows_resblock_dropout_*`): `dropout(x + gelu(linear(x))) * row_scale[..., None]`.  `draws`: the module's 'out' site,
    as for `_QkvDenseDropFn`"""

    @staticmethod
    def forward(ctx, x, weight, bias, row_scale, draws):
        from asac_amd import native
        p, seed, instance, state, used = draws
        x2 = x.reshape(-1, x.shape[-1])
        if x2.stride(1) != 1 or (x2.stride(0) | (x2.data_ptr() >> 2)) & 3:
            x2 = x2.contiguous()
        y, pre = torch.empty(x2.shape, dtype=x.dtype, device=x.device), torch.empty(x2.shape, dtype=x.dtype, device=x.device)
        sc = None if row_scale is None else row_scale.reshape(-1).contiguous()
        native.rows_resblock_dropout_forward(x2, weight.detach(), bias.detach(), sc, y, pre, p, seed, instance, state, used)
        ctx.save_for_backward(x2, pre, used, *([sc] if sc is not None else []))
        ctx.params, ctx.lead, ctx.draws = (weight, bias), x.shape, (p, seed, instance)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        from asac_amd import native
        x2, pre, used, *rest = ctx.saved_tensors
        weight, bias = ctx.params
        gy2 = gy.reshape(x2.shape).contiguous()
        gx, gpre = torch.empty_like(pre), torch.empty_like(pre)
        native.rows_resblock_dropout_backward(gy2, pre, weight.detach(), rest[0] if rest else None, gx, gpre, *ctx.draws, used)
        gw, gb = _rows_param_grads(ctx.needs_input_grad[1:3], ctx.params, gpre, x2)
        return gx.view(ctx.lead), gw, gb, None, None


class _OutResSavedFn(torch.autograd.Function):
    """`_OutResRowsFn` whose forward already ran (inside `asac_attention_mh_proj_forward`): y and pre are handed in, the
    backward is the same"""

    @staticmethod
    def forward(ctx, x, weight, bias, row_scale, y_pre):
        y, pre = y_pre          # (a tuple, not tensor arguments: the result must not be a view of an input)
        x2 = x.reshape(-1, x.shape[-1])
        sc = None if row_scale is None else row_scale.reshape(-1)
        ctx.save_for_backward(x2, pre.view(x2.shape), *([sc] if sc is not None else []))
        ctx.params, ctx.lead = (weight, bias), x.shape
        return y.view_as(x)

    @staticmethod
    def backward(ctx, gy):
        gx, gw, gb, _ = _OutResRowsFn.backward(ctx, gy)
        return gx, gw, gb, None, None


class _GateRowsFn(torch.autograd.Function):
    """`gatedlayer(x, y) * ~row_zero[..., None]` for a RESIDUAL / OUTPUT / RECURRENT gate — the gate behind an episode block's
    attention and its padded-row factor — as one launch per pass (`asac_rows_gate_*`, csrc/rows_gate.hip); the parameter
    gradients from `asac_xty` over the pre-activation gradients the backward launch writes.
    params: () / (W,) / (Wxr, Wyr, Wxz, Wyz, Wxg, Wyg, bz)"""

    @staticmethod
    def forward(ctx, kind, x, y, row_zero, *params):
        from asac_amd import native
        B, L, E = y.shape
        # (a view expanded along the batch or the positions — a stride of 0 — is made dense like a misaligned one: the launch
        # takes rows that do not overlap)
        if (x.stride(2) != 1 or (x.stride(0) | x.stride(1) | (x.data_ptr() >> 2)) & 3 or (L > 1 and x.stride(1) < E)
                or (B > 1 and x.stride(0) < E)):
            x = x.contiguous()
        if not y.is_contiguous() or y.data_ptr() & 15:
            y = y.clone(memory_format=torch.contiguous_format)
        if row_zero is not None and ((L > 1 and row_zero.stride(1) != 1) or (B > 1 and row_zero.stride(0) < L)):
            row_zero = row_zero.contiguous()
        weights = [w.detach() for w in params[:6]]
        bz = params[6].detach() if len(params) == 7 else None
        out = torch.empty(y.shape, dtype=y.dtype, device=y.device)
        need = any(ctx.needs_input_grad)
        saved = [torch.empty_like(out) for _ in range({1: 0, 2: 1, 3: 3}[kind])] if need else []
        native.rows_gate_forward(kind, x, y, row_zero, weights, bz, out, saved or None)
        if need:
            ctx.save_for_backward(x, y, *saved, *([row_zero] if row_zero is not None else []))
        ctx.kind, ctx.params, ctx.masked = kind, params, row_zero is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        from asac_amd import native
        kind, params = ctx.kind, ctx.params
        x, y, *saved = ctx.saved_tensors
        row_zero = saved.pop() if ctx.masked else None
        E = y.shape[-1]
        if not g_out.is_contiguous() or g_out.data_ptr() & 15:
            g_out = g_out.clone(memory_format=torch.contiguous_format)
        weights = [w.detach() for w in params[:6]]
        g_x = torch.empty_like(y)
        if kind == GATE.RESIDUAL.value:
            native.rows_gate_backward(kind, g_out, x, y, row_zero, weights, [], g_x, g_x, [])
            return None, g_x, g_x, None
        g_y = torch.empty_like(y)
        g_pre = [torch.empty_like(y) for _ in saved]
        rx = torch.empty_like(y) if kind == GATE.RECURRENT.value else None
        native.rows_gate_backward(kind, g_out, x, y, row_zero, weights, saved, g_x, g_y, g_pre, rx)
        needs = ctx.needs_input_grad[4:]
        if not any(needs):
            return (None, g_x, g_y, None, *([None] * len(params)))
        x2, y2, jobs = x.reshape(-1, E), y.view(-1, E), []
        if kind == GATE.OUTPUT.value:
            gw, _ = _rows_param_grads(needs[:1], (params[0], None), g_pre[0].view(-1, E), x2, jobs)
            _run_xty_jobs(jobs)
            return None, g_x, g_y, None, gw
        dr, dz, dh = (g.view(-1, E) for g in g_pre)
        wxr, wyr, wxz, wyz, wxg, wyg, bz = params
        # six products with six distinct outputs, the bias gradient the column sums of dz_pre beside the first product over it
        gxr, _ = _rows_param_grads(needs[0:1], (wxr, None), dr, x2, jobs)
        gyr, _ = _rows_param_grads(needs[1:2], (wyr, None), dr, y2, jobs)
        gxz, gbz = _rows_param_grads((needs[2], needs[6]), (wxz, bz), dz, x2, jobs)
        gyz, _ = _rows_param_grads(needs[3:4], (wyz, None), dz, y2, jobs)
        gxg, _ = _rows_param_grads(needs[4:5], (wxg, None), dh, rx.view(-1, E), jobs)
        gyg, _ = _rows_param_grads(needs[5:6], (wyg, None), dh, y2, jobs)
        _run_xty_jobs(jobs)
        return None, g_x, g_y, None, gxr, gyr, gxz, gyz, gxg, gyg, gbz


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
    from asac_amd import native
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
    from asac_amd import native
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
    from asac_amd import native
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
    from asac_amd import native
    return native.attention_supported(q.shape[1], k.shape[1], q.shape[2])


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
        # the attention-weight dropout's stream of draws (csrc/asac_dropout.h): plain attributes, no buffers — the state_dict
        # keeps the reference's keys.  Instance id, seed and the per-device state are taken at the first dropout launch.
        self._drop_instance = None         # from the one counter of algorithm/utils/image_transforms.py
        self._drop_seed = None             # None: torch.initial_seed() at the first launch
        self._drop_counter0 = 0            # where a device first launched on later starts counting
        self._drop_states = {}             # device -> int64 [544]: the call counter and the arrival words
        self._drop_used = None             # int64 [1]: the counter the last dropout launch drew with
        # the dense stacks' dropout launches ('qkv', 'out': seq_layers.FUSED_DENSE_DROPOUT) draw from the same (seed, instance
        # id) under tags of their own, each site with a state and a `used` record of its own
        self._dense_drop_states = {'qkv': {}, 'out': {}}
        self._dense_drop_used = {'qkv': None, 'out': None}

    def reseed(self, seed: int, counter: int = 0, instance_id: int | None = None):
        """the draws of the module's dropout launches (the attention weights', the dense stacks') are functions of (seed,
        instance id, call counter): re-seat all three, in every state"""
        self._drop_seed = int(seed)
        if instance_id is not None:
            self._drop_instance = int(instance_id)
        for states in (self._drop_states, *self._dense_drop_states.values()):
            for state in states.values():
                state.copy_(torch.tensor([int(counter)] + [0] * (state.numel() - 1), dtype=torch.int64))
        self._drop_counter0 = int(counter)
        return self

    def dense_dropout_drawn(self, site: str) -> int:
        """the call counter the last dense-stack dropout launch of `site` ('qkv' or 'out') drew with.  Synchronises."""
        if self._dense_drop_used[site] is None:
            raise RuntimeError(f'no {site} dropout launch yet')
        return int(self._dense_drop_used[site].item())

    def dense_dropout_state(self, site: str, device=None):
        """`dropout_state` of the dense-stack dropout launch of `site` ('qkv' or 'out')"""
        states = self._dense_drop_states[site]
        if not states:
            return None
        state = states[device] if device is not None else next(iter(states.values()))
        return int(state[0].item()), int(torch.count_nonzero(state[1:]).item())

    def _new_drop_state(self, device):
        """a draw state on `device` (the stream is not capturing); takes the instance id and the seed if nobody has yet"""
        from asac_amd import native
        if self._drop_instance is None:
            from algorithm.utils.image_transforms import _instance_ids
            self._drop_instance = next(_instance_ids)
        if self._drop_seed is None:
            self._drop_seed = torch.initial_seed()
        return torch.tensor([self._drop_counter0] + [0] * (native.ATTN_DROPOUT_STATE_WORDS - 1), dtype=torch.int64, device=device)

    def _dense_dropout_draws(self, site, device, rows, p):
        """(p, seed, instance id, state, used) of one dense-stack dropout launch of `site` over `rows` rows on `device`, or None
        where the module code has to run — the rules of `_dropout_draws`; `used` is this CALL's record"""
        if rows * self.embed_dim >= 1 << 34:
            return None
        states = self._dense_drop_states[site]
        state = states.get(device)
        if state is None:
            if torch.cuda.is_current_stream_capturing():
                return None
            state = states[device] = self._new_drop_state(device)
        used = self._dense_drop_used[site] = torch.empty(1, dtype=torch.int64, device=device)
        return p, self._drop_seed, self._drop_instance, state, used

    def dropout_drawn(self) -> int:
        """the call counter the last dropout launch drew with.  Synchronises."""
        if self._drop_used is None:
            raise RuntimeError('no dropout launch yet')
        return int(self._drop_used.item())

    def dropout_state(self, device=None):
        """(call counter, how many arrival words are not zero) of the dropout state on `device` (default: the only one), or
        None where there is none yet.  Synchronises."""
        if not self._drop_states:
            return None
        state = self._drop_states[device] if device is not None else next(iter(self._drop_states.values()))
        return int(state[0].item()), int(torch.count_nonzero(state[1:]).item())

    def _dropout_draws(self, device, bsz):
        """(p, seed, instance id, state, used) of one dropout launch on `device`, or None where the module code has to run:
        the state does not exist yet and the stream is capturing (allocating and seeding are not part of a capture), or
        the batch is beyond the draw layout.  `used` is this CALL's record: a module applied twice before its backwards
        (observations and next observations) keeps both counters apart."""
        from asac_amd import native
        if bsz * self.num_heads > native.ATTN_DROPOUT_MAX_BATCH_HEADS:
            return None
        state = self._drop_states.get(device)
        if state is None:
            if torch.cuda.is_current_stream_capturing():
                return None
            state = self._drop_states[device] = self._new_drop_state(device)
        self._drop_used = torch.empty(1, dtype=torch.int64, device=device)
        return self.dropout, self._drop_seed, self._drop_instance, state, self._drop_used

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

        if (self.pe is None or self.pe is False) and same_kv and FUSED_PROJECTIONS and query.dim() == 3 \
                and _fused_core_ok(query, key, self.num_heads, self.training and self.dropout > 0.):
            lq, lk, lv = _plain_linear(self.q_proj), _plain_linear(self.k_proj), _plain_linear(self.v_proj)
            if lq is not None and lk is not None and lv is not None and lq.in_features == lq.out_features == self.embed_dim:
                # projections + scores / mask / softmax / weighted sum: one launch per pass (csrc/attn.hip)
                m = attn_mask
                if key_padding_mask is not None:
                    kpm = key_padding_mask.unsqueeze(1)
                    m = kpm.expand(-1, q_len, -1) if m is None else torch.logical_or(m, kpm)
                if m is not None:
                    m = m.unsqueeze(0) if m.dim() == 2 else m
                    m = m if m.dtype in (torch.bool, torch.uint8) else m != 0
                lo = _plain_resblock(self.out_proj, self.embed_dim)
                rz = out_row_mask
                if rz is not None:
                    rz = rz.reshape(-1, rz.shape[-1])
                    rz = rz if rz.dtype in (torch.bool, torch.uint8) else rz != 0
                xq = q_len if _is_tail_view(query, key) else query
                if lo is not None:      # ... and the output ResBlock with the dead-row rule and the row mask
                    out, weights, keep = _AttnProjFn.apply(xq, key, m, rz, lq.weight, lq.bias, lk.weight, lk.bias,
                                                           lv.weight, lv.bias, lo.weight, lo.bias)
                else:
                    out, weights, keep = _AttnProjFn.apply(xq, key, m, None, lq.weight, lq.bias, lk.weight, lk.bias,
                                                           lv.weight, lv.bias)
                    out = self.out_proj(out)
                    if m is not None:
                        out = out * keep.unsqueeze(-1)
                    if rz is not None:
                        out = out * (~rz).to(out.dtype).unsqueeze(-1)
                return out.reshape(*lead, *out.shape[1:]), weights.reshape(*lead, *weights.shape[1:])

        fused_qkv = None
        rotary = self.pe in (POSITIONAL_ENCODING.ROPE, POSITIONAL_ENCODING.ROPE2)
        rope_tables = _fused_rope_tables(self, query, key, query_index, key_index) if rotary else None
        plain_or_rotary = self.pe is None or self.pe is False or rope_tables is not None
        dense, dense_draws = (_dense_qkv_ok(self, query, key) if plain_or_rotary and same_kv else None), None
        if dense is not None:
            # None: this call runs the module code below
            dense_draws = self._dense_dropout_draws('qkv', key.device, bsz * k_len, dense[0][1].p)
        if dense_draws is not None:
            # dense q / k / v stacks with their live nn.Dropout: one launch per pass (csrc/rows_proj.hip); a rotary encoding
            # follows as the `_RopeFn` launch
            q, k, v = _QkvDenseDropFn.apply(key, q_len, dense_draws,
                                            *(t for r, _, lin in dense for t in (r.weight, r.bias, lin.weight, lin.bias)))
        elif plain_or_rotary and same_kv and _rows_proj_ok(self, query, key):
            qkv_params = [t for ll in (self.q_proj, self.k_proj, self.v_proj) for t in (_plain_linear(ll).weight, _plain_linear(ll).bias)]
            from asac_amd import native
            if rotary:
                # (without indexes the query's positions count from 0: the key's newest entries only when the lengths agree)
                if (own_index and q_len == k_len) or query_index is key_index or _is_index_tail(query_index, key_index):
                    # projections and rotation: one launch per pass (csrc/rows_proj.hip)
                    q, k, v = _QkvRopeRowsFn.apply(key, q_len, key_index, self.pe.value, rope_tables, *qkv_params)
                    rotary = False
                else:
                    q, k, v = _QkvRowsFn.apply(key, q_len, *qkv_params)
            elif (FUSED_MULTIHEAD and FUSED_QKV_IN_CORE and (self.num_heads > 1 or self.head_dim > 16)
                    and not (self.training and self.dropout > 0.)
                    and native.attention_mh_proj_supported(q_len, k_len, self.num_heads, self.head_dim)):
                fused_qkv = qkv_params      # windows of <= 16 positions: the projections run inside the core's forward launch
                q = k = v = key
            else:
                q, k, v = _QkvRowsFn.apply(key, q_len, *qkv_params)
        else:
            q, k, v = self.q_proj(query), self.k_proj(key), self.v_proj(value)
        if rotary and rope_tables is not None:
            q, k = _RopeFn.apply(q, k, query_index, key_index, self.pe.value, rope_tables)      # one launch per pass (csrc/rope.hip)
        elif rotary:
            q, k = self.rope(query_index, key_index, q, k)
        drop_active = self.training and self.dropout > 0.
        if (FUSED_MULTIHEAD and (self.num_heads > 1 or self.head_dim > 16) and q.is_cuda and q.dtype == torch.float32
                and (not drop_active or (FUSED_ATTN_DROPOUT and self.dropout < 1.))):
            from asac_amd import native
            draws = None
            supported = native.attention_mh_supported(q_len, k_len, self.num_heads, self.head_dim)
            if supported and drop_active:
                # the weights' dropout inside the core's launches; None: this call runs the module code below
                draws = self._dropout_draws(q.device, bsz)
                supported = draws is not None
            if supported:
                # several heads (or one wide head): scores, mask, softmax, weighted sum and the head average as one MFMA launch (csrc/attn_mh.hip)
                m = attn_mask
                if key_padding_mask is not None:
                    kpm = key_padding_mask.unsqueeze(1)
                    m = kpm.expand(-1, q_len, -1) if m is None else torch.logical_or(m, kpm)
                if m is not None:
                    m = m.unsqueeze(0) if m.dim() == 2 else m
                    m = m if m.dtype in (torch.bool, torch.uint8) else m != 0
                # the dead-row rule and the caller's padded rows as ONE factor formed by the launch itself (keep * ~row mask:
                # a product with `keep`, a `bitwise_not`, a cast and a second product were four launches per block and pass)
                rz = out_row_mask
                if rz is not None:
                    rz = rz.reshape(-1, rz.shape[-1])
                    rz = rz if rz.dtype in (torch.bool, torch.uint8) else rz != 0
                lo = _plain_resblock(self.out_proj, self.embed_dim) if FUSED_ROWS_PROJ else None
                # an output stack with a LIVE nn.Dropout behind its ResBlock: the drop inside the ResBlock launch
                lod = _dropout_resblock(self.out_proj, self.embed_dim) \
                    if lo is None and FUSED_ROWS_PROJ and FUSED_DENSE_DROPOUT and native.rows_proj_supported(self.embed_dim) else None
                out_draws = None
                if lod is not None:
                    out_draws = self._dense_dropout_draws('out', q.device, bsz * q_len, lod[1].p)
                y_pre = None
                block_done = False
                if fused_qkv is not None and lo is not None and FUSED_BLOCK_BACKWARD:
                    # ... and the output ResBlock behind it: the block is ONE launch forward and ONE backward
                    out, weights, keep, keep_rows = _AttnBlockFn.apply(key, q_len, *fused_qkv, lo.weight, lo.bias, m, self.num_heads,
                                                                       rz, rz is not None or m is not None)
                    block_done = True
                elif fused_qkv is not None and lo is not None:
                    out, weights, keep, keep_rows, *y_pre = _QkvAttnMhFn.apply(key, q_len, *fused_qkv, m, self.num_heads, rz,
                                                                               (lo.weight, lo.bias))
                elif fused_qkv is not None:
                    out, weights, keep, keep_rows = _QkvAttnMhFn.apply(key, q_len, *fused_qkv, m, self.num_heads, rz)
                elif draws is not None:
                    out, weights, keep, keep_rows = _AttnMhDropFn.apply(q, k, v, m, self.num_heads, rz, draws)
                else:
                    out, weights, keep, keep_rows = _AttnMhFn.apply(q, k, v, m, self.num_heads, rz)
                scale = keep_rows if rz is not None else (keep if m is not None else None)
                if block_done:
                    pass
                elif y_pre:
                    out = _OutResSavedFn.apply(out, lo.weight, lo.bias, scale, tuple(y_pre))
                elif lo is not None and native.rows_proj_supported(self.embed_dim):
                    # the output ResBlock and the dead-row / padded-row factor: one launch
                    out = _OutResRowsFn.apply(out, lo.weight, lo.bias, scale)
                elif out_draws is not None:
                    # ... with the stack's live nn.Dropout between the ResBlock and the factor: still one launch
                    out = _OutResDropRowsFn.apply(out, lod[0].weight, lod[0].bias, scale, out_draws)
                else:
                    out = self.out_proj(out)
                    if scale is not None:
                        out = out * scale.unsqueeze(-1)
                return out.reshape(*lead, *out.shape[1:]), weights.reshape(*lead, *weights.shape[1:])
        q, k, v = self._split_heads(q), self._split_heads(k), self._split_heads(v)

        if key_padding_mask is not None:
            kpm = key_padding_mask.unsqueeze(1)                               # [bsz, 1, k]
            attn_mask = kpm.expand(-1, q_len, -1) if attn_mask is None else torch.logical_or(attn_mask, kpm)

        if _fused_core_ok(q, k, self.num_heads, self.training and self.dropout > 0.):
            # short windows, one head: scores, mask, softmax and the weighted sum as one launch (csrc/attn.hip)
            m = attn_mask
            if m is not None:
                m = m.unsqueeze(0) if m.dim() == 2 else m
                m = m if m.dtype in (torch.bool, torch.uint8) else m != 0
            out, weights, keep = _AttnCoreFn.apply(q, k, v, m)
            out = self.out_proj(out)
            if m is not None:      # fully masked queries produce zeros (the kernel already zeroed their weights)
                out = out * keep.unsqueeze(-1)
            if out_row_mask is not None:
                out = out * (~out_row_mask.reshape(-1, out_row_mask.shape[-1])).to(out.dtype).unsqueeze(-1)
            return out.reshape(*lead, *out.shape[1:]), weights.reshape(*lead, *weights.shape[1:])
        q = q / math.sqrt(self.head_dim)

        dead_rows = None
        if attn_mask is not None:
            if attn_mask.dim() == 2:
                attn_mask = attn_mask.unsqueeze(0).expand(bsz, -1, -1)
            dead_rows = attn_mask.all(dim=-1)                                 # [bsz, q]: nothing to attend to
            bias = torch.zeros(attn_mask.shape, dtype=query.dtype, device=query.device)
            bias = bias.masked_fill(attn_mask & ~dead_rows.unsqueeze(-1), float('-inf'))   # dead rows stay 0
            scores = torch.baddbmm(bias.repeat(self.num_heads, 1, 1), q, k.transpose(-2, -1))
        else:
            scores = torch.bmm(q, k.transpose(-2, -1))
        weights = torch.softmax(scores, dim=-1)                               # [bsz * heads, q, k]
        if self.training and self.dropout > 0.:
            weights = nn.functional.dropout(weights, p=self.dropout)
        out = torch.bmm(weights, v)                                           # [bsz * heads, q, head_dim]

        if self.num_heads > 1:
            weights = weights.view(self.num_heads, bsz, q_len, k_len).mean(0)
            out = out.view(self.num_heads, bsz, q_len, self.head_dim).permute(1, 2, 0, 3).reshape(bsz, q_len, self.embed_dim)
        out = self.out_proj(out)
        if dead_rows is not None:   # fully masked queries produce zeros, not NaN
            keep = ~dead_rows.unsqueeze(-1)
            out, weights = out * keep, weights * keep
        if out_row_mask is not None:
            out = out * (~out_row_mask.reshape(-1, out_row_mask.shape[-1])).to(out.dtype).unsqueeze(-1)
        return out.reshape(*lead, *out.shape[1:]), weights.reshape(*lead, *weights.shape[1:])


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
