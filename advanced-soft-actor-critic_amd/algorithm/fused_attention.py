"""Autograd glue of the attention launches (csrc/attn.hip, attn_mh.hip, rows_proj.hip, rope.hip, rows_gate.hip).

`nn_models.layers.seq_layers` decides WHICH of these a call takes (its `FUSED_*` switches and recognisers); here is only what
a launch pair needs around it: aligned inputs, output allocation, what the backward keeps, and where the parameter gradients
go.  Entry points, all `torch.autograd.Function`s applied by `MultiheadAttention.forward` / `EpisodeMultiheadAttentionBlock`:

  one head      `_AttnCoreFn` (scores / mask / softmax / weighted sum), `_AttnProjFn` (... with the q / k / v projections and
                the output ResBlock on chip)
  many heads    `_AttnMhFn` (the core of all heads; `draws`: dropout of the weights inside the launches), `_QkvAttnMhFn` (...
                with the projections in the forward launch), `_AttnBlockFn` (... and the output ResBlock: one launch a pass)
  rows around   `_QkvRowsFn` (q / k / v Linears, optionally rotated), `_QkvDenseDropFn` (q / k / v dense stacks with live
                dropout), `_RopeFn`, `_OutResRowsFn` (output ResBlock and row factor; `draws`: live dropout; `y_pre`: the
                forward already ran) — also behind `fused_rows_linear.rows_resblock` — and `_GateRowsFn`

`draws` = (p, seed, instance id, state, used): a dropout site's stream of draws, its device state and this call's `used`
record (`seq_layers._DrawSite`) — the backward launch reads the counter from `used` on the device, so a captured pair stays
in step on every replay.  Parameter gradients are products over the rows (`asac_xty`): added straight into the `.grad` views
under the learner's direct mode, in the order they are queued here, else returned.
"""
import torch

from asac_amd import native

from .param_grads import deliver_packed, direct_enabled, direct_skips, flat_grad_alias, queue_param_grads

GATE_RESIDUAL, GATE_OUTPUT, GATE_RECURRENT = 1, 2, 3       # seq_layers.GATE values (the `kind` of `_GateRowsFn`)


# ------------------------------------------------------------------------------------------------
# shared helpers
# ------------------------------------------------------------------------------------------------
def _rows_misaligned(x) -> bool:
    """the row launches read x ([B, L, E] or flattened [rows, E]) as 16-byte vectors: unit feature stride, every row start
    a multiple of four floats"""
    lead = x.data_ptr() >> 2
    for s in x.stride()[:-1]:
        lead |= s
    return x.stride(-1) != 1 or bool(lead & 3)


def _aligned_rows(x):
    return x.contiguous() if _rows_misaligned(x) else x


def _unpack_draws(draws):
    """draws -> ((p, seed, instance id) for the context, state, used); ((), None, None) without dropout"""
    if draws is None:
        return (), None, None
    return tuple(draws[:3]), draws[3], draws[4]


def _qkv_outputs(x, tail):
    B, L, E = x.shape
    return [torch.empty(B, t, E, dtype=x.dtype, device=x.device) for t in (tail, L, L)]


def _core_outputs(like, Lq, Lk, heads, row_zero, need_p_heads):
    """(out, weights, keep, keep_rows, p_heads) of a multi-head core launch: keep_rows is `keep` without a row mask, p_heads
    None where no backward follows"""
    B, E = like.shape[0], like.shape[2]
    dd = dict(dtype=like.dtype, device=like.device)
    out, weights, keep = torch.empty(B, Lq, E, **dd), torch.empty(B, Lq, Lk, **dd), torch.empty(B, Lq, **dd)
    keep_rows = torch.empty(B, Lq, **dd) if row_zero is not None else keep
    p_heads = torch.empty(B, heads, Lq, Lk, **dd) if need_p_heads else None
    return out, weights, keep, keep_rows, p_heads


def _rows_param_grads(ctx_needs, params, g2, x2, jobs=None):
    """weight / bias gradient of one Linear (bias: None without one) from its output gradient rows g2 and input rows x2
    (`asac_xty`): added straight into the `.grad` views under the learner's direct mode, else returned.  With a list `jobs` the
    returned product is not launched but appended to it: the caller has several and runs them together (`_run_xty_jobs`)"""
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
    for i in range(0, len(jobs), 4):
        if len(jobs[i:i + 4]) == 1:
            native.xty(*jobs[i])
        else:
            native.xty_multi(jobs[i:i + 4])


def _qkv_inputs(x, tail):
    """the input rows of the q, k, v projections of x [B, L, E]: the newest `tail` positions, all, all"""
    E = x.shape[2]
    x2 = x.reshape(-1, E)
    return (x2 if tail == x.shape[1] else x[:, -tail:].reshape(-1, E)), x2, x2


def _qkv_param_grads(needs, params, grads, inputs):
    """[gwq, gbq, gwk, gbk, gwv, gbv] of (wq, bq, wk, bk, wv, bv) from the three output gradients, in that order"""
    out = []
    for j, (g, xin) in enumerate(zip(grads, inputs)):
        out.extend(_rows_param_grads(needs[2 * j:2 * j + 2], params[2 * j:2 * j + 2], g.view(-1, g.shape[-1]), xin))
    return out


def _qkv_backward(need_x, needs, params, x, tail, grads):
    """[gx, six parameter gradients] of plain q / k / v Linears: the input gradient of the three as one launch — none where
    x needs no gradient — then the products"""
    gx = None
    if need_x:
        gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        native.rows_proj_backward(grads, [tail, x.shape[1], x.shape[1]], [w.detach() for w in params[0::2]], gx)
    return [gx, *_qkv_param_grads(needs, params, grads, _qkv_inputs(x, tail))]


def _core_mh_backward(q, k, v, mask, heads, p_heads, g_out, g_w, draws=(), used=None):
    """(g_q, g_k, g_v) of the multi-head core from one launch"""
    if g_out is None:
        g_out = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
    g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    args = (q, k, v, mask, heads, p_heads, g_out.contiguous(), None if g_w is None else g_w.contiguous(), g_q, g_k, g_v)
    if used is None:
        native.attention_mh_backward(*args)
    else:
        native.attention_mh_dropout_backward(*args, *draws, used)
    return g_q, g_k, g_v


def _mh_proj_forward(x, tail, qkv, mask, heads, row_zero, out_block, need_p_heads):
    """`asac_attention_mh_proj_forward` for windows of <= 16 positions: the q / k / v projections in front of the scores and,
    with `out_block` = (weight, bias), the output ResBlock behind the core, all in one launch
    -> (x as read, [q, k, v], (out, weights, keep, keep_rows, p_heads), (y, pre) or (None, None))"""
    x = _aligned_rows(x)
    qkv_out = _qkv_outputs(x, tail)
    core = _core_outputs(x, tail, x.shape[1], heads, row_zero, need_p_heads)
    out, weights, keep, keep_rows, p_heads = core
    y = pre = None
    if out_block is not None:
        y, pre = torch.empty_like(out), torch.empty_like(out)
    native.attention_mh_proj_forward(x, [w.detach() for w in qkv[0::2]], [b.detach() for b in qkv[1::2]],
                                     mask, heads, *qkv_out, out, weights, keep, p_heads,
                                     None if row_zero is None else (row_zero if row_zero.stride(-1) == 1 else row_zero.contiguous()),
                                     keep_rows if row_zero is not None else None,
                                     *(() if out_block is None else (out_block[0].detach().contiguous(),
                                                                     out_block[1].detach().contiguous(), y, pre)))
    return x, qkv_out, core, (y, pre)


# ------------------------------------------------------------------------------------------------
# one head
# ------------------------------------------------------------------------------------------------
class _AttnCoreFn(torch.autograd.Function):
    """scores / mask / softmax / weighted sum of one attention head as one launch per pass
    (`asac_attention_forward/backward`, csrc/attn.hip) -> (out, weights * keep, keep)"""

    @staticmethod
    def forward(ctx, q, k, v, mask):
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
        q, k, v, weights = ctx.saved_tensors
        if g_out is None and g_w is None:
            return None, None, None, None
        if g_out is None:
            g_out = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
        g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        native.attention_backward(q, k, v, weights, g_out.contiguous(), None if g_w is None else g_w.contiguous(),
                                  g_q, g_k, g_v)
        return g_q, g_k, g_v, None


class _AttnProjFn(torch.autograd.Function):
    """`_AttnCoreFn` with the q / k / v Linear projections — and, with 8 parameters, the output ResBlock
    y = (GELU(Wo o + bo) + o) * keep — on chip (`asac_attention_proj_*`): x_q, x_k in, (out, weights * keep, keep) out.
    The parameter gradients are added straight into their `.grad` views when those are consecutive slices of one
    buffer (the learner's flat gradient buffer), else returned."""

    @staticmethod
    def forward(ctx, xq, xk, mask, row_zero, *params):
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


# ------------------------------------------------------------------------------------------------
# many heads
# ------------------------------------------------------------------------------------------------
class _AttnMhFn(torch.autograd.Function):
    """scores / mask / softmax / weighted sum of ALL heads and the head-averaged weights as one MFMA launch per pass
    (`asac_attention_mh_forward/backward`, csrc/attn_mh.hip): q, k, v [B, L, heads * d] -> (out [B, Lq, heads * d] with the
    heads concatenated, mean-over-heads weights * keep, keep, keep_rows).  With `draws`: dropout of the softmax weights inside
    both launches (`asac_attention_mh_dropout_forward/backward`) — the weights returned are the DROPPED ones' head mean, as
    the reference returns them."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, row_zero=None, draws=None):
        """`row_zero` bool [B, Lq]: the caller's padded positions — the fourth result is then keep * ~row_zero, the one
        factor the caller's output needs (else it is `keep` again)"""
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, weights, keep, keep_rows, p_heads = _core_outputs(q, q.shape[1], k.shape[1], heads, row_zero,
                                                               any(ctx.needs_input_grad[:3]))
        args = (q, k, v, mask, heads, out, weights, keep, p_heads, None if row_zero is None else row_zero.contiguous(),
                keep_rows if row_zero is not None else None)
        ctx.draws, state, used = _unpack_draws(draws)
        if draws is None:
            native.attention_mh_forward(*args)
        else:
            native.attention_mh_dropout_forward(*args, *ctx.draws, state, used)
        if p_heads is not None:
            ctx.save_for_backward(q, k, v, p_heads, mask, used)
        ctx.heads = heads
        ctx.mark_non_differentiable(keep, keep_rows)
        ctx.set_materialize_grads(False)
        return out, weights, keep, keep_rows

    @staticmethod
    def backward(ctx, g_out, g_w, _g_keep, _g_keep_rows=None):
        if g_out is None and g_w is None:
            return (None,) * 7
        q, k, v, p_heads, mask, used = ctx.saved_tensors
        return (*_core_mh_backward(q, k, v, mask, ctx.heads, p_heads, g_out, g_w, ctx.draws, used), None, None, None, None)


class _QkvAttnMhFn(torch.autograd.Function):
    """`_QkvRowsFn` and `_AttnMhFn` as ONE forward launch for windows of <= 16 positions (`_mh_proj_forward`); backward: the
    core's launch, then the projections' input gradient and parameter-gradient products as in `_QkvRowsFn`"""

    @staticmethod
    def forward(ctx, x, tail, wq, bq, wk, bk, wv, bv, mask, heads, row_zero=None, out_block=None):
        """`out_block` = (weight, bias) of the output ResBlock: it runs behind the core in the same launch and two more tensors
        come back (y, pre) — non-differentiable HERE: `_OutResRowsFn` with `y_pre` turns them into the block's output and
        carries its backward"""
        need = any(ctx.needs_input_grad[i] for i in (0, 2, 3, 4, 5, 6, 7))
        ctx.params = (wq, bq, wk, bk, wv, bv)
        x, qkv, (out, weights, keep, keep_rows, p_heads), y_pre = _mh_proj_forward(x, tail, ctx.params, mask, heads, row_zero,
                                                                                   out_block, need)
        if need:
            ctx.save_for_backward(x, *qkv, p_heads, mask)
        ctx.tail, ctx.heads = tail, heads
        ctx.set_materialize_grads(False)
        if out_block is None:
            ctx.mark_non_differentiable(keep, keep_rows)
            return out, weights, keep, keep_rows
        ctx.mark_non_differentiable(keep, keep_rows, *y_pre)
        return (out, weights, keep, keep_rows, *y_pre)

    @staticmethod
    def backward(ctx, g_out, g_w, _g_keep, _g_keep_rows=None, _g_y=None, _g_pre=None):
        if g_out is None and g_w is None:
            return (None,) * 12
        x, q, k, v, p_heads, mask = ctx.saved_tensors
        grads = list(_core_mh_backward(q, k, v, mask, ctx.heads, p_heads, g_out, g_w))
        gx, *gp = _qkv_backward(ctx.needs_input_grad[0], ctx.needs_input_grad[2:8], ctx.params, x, ctx.tail, grads)
        return (gx, None, *gp, None, None, None, None)


class _AttnBlockFn(torch.autograd.Function):
    """The whole attention block for windows of <= 16 positions — q / k / v projections, core, output ResBlock with the
    dead-row / padded-row factor — as ONE launch forward (`_mh_proj_forward`) and ONE backward
    (`asac_attention_mh_block_backward`), plus the four parameter-gradient products (`asac_xty`, queued)"""

    @staticmethod
    def forward(ctx, x, tail, wq, bq, wk, bk, wv, bv, wo, bo, mask, heads, row_zero, scaled):
        need = any(ctx.needs_input_grad[i] for i in (0, 2, 3, 4, 5, 6, 7, 8, 9))
        ctx.params = (wq, bq, wk, bk, wv, bv, wo, bo)
        x, qkv, (out, weights, keep, keep_rows, p_heads), (y, pre) = _mh_proj_forward(x, tail, ctx.params[:6], mask, heads,
                                                                                      row_zero, (wo, bo), need)
        if need:
            # (`scaled`: the block's output was multiplied by keep_rows — with a row mask — or by keep — with an attention mask)
            ctx.save_for_backward(x, *qkv, p_heads, out, pre, keep_rows if scaled else None, mask)
        ctx.tail, ctx.heads = tail, heads
        ctx.mark_non_differentiable(keep, keep_rows)
        ctx.set_materialize_grads(False)
        return y, weights, keep, keep_rows

    @staticmethod
    def backward(ctx, g_y, g_w, _g_keep, _g_keep_rows=None):
        if g_y is None and g_w is None:
            return (None,) * 14
        x, q, k, v, p_heads, out, pre, scale, mask = ctx.saved_tensors
        E = x.shape[2]
        if g_y is None:
            g_y = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
        wq, _, wk, _, wv, _, wo, bo = ctx.params
        g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        g_pre, g_x = torch.empty_like(pre), torch.empty(x.shape, dtype=x.dtype, device=x.device)
        g_y = _aligned_rows(g_y)      # (otherwise a slice — the gradient of a concatenation's part — is read in place)
        native.attention_mh_block_backward(q, k, v, mask, ctx.heads, p_heads, g_y, pre,
                                           None if scale is None else scale.contiguous(), wo.detach().contiguous(),
                                           None if g_w is None else g_w.contiguous(),
                                           [wq.detach(), wk.detach(), wv.detach()], g_q, g_k, g_v, g_pre, g_x)
        inputs = _qkv_inputs(x, ctx.tail)
        # (the output block's product first: the order the three-launch form queues them in)
        go = _rows_param_grads(ctx.needs_input_grad[8:10], (wo, bo), g_pre.view(-1, E), out.view(-1, E))
        gqkv = _qkv_param_grads(ctx.needs_input_grad[2:8], ctx.params[:6], (g_q, g_k, g_v), inputs)
        return (g_x if ctx.needs_input_grad[0] else None, None, *gqkv, *go, None, None, None, None)


# ------------------------------------------------------------------------------------------------
# the rows around the core
# ------------------------------------------------------------------------------------------------
class _QkvRowsFn(torch.autograd.Function):
    """`q_proj(x[:, -tail:]), k_proj(x), v_proj(x)` — three nn.Linear(E, E) over the rows of a window batch — as ONE MFMA
    launch; backward: the input gradient of the three as one launch, the parameter gradients as products over the rows
    (`asac_rows_proj_*`, csrc/rows_proj.hip; `asac_xty`).  With `rope` = (index, kind, tables — `seq_layers._fused_rope_tables`):
    `self.rope(index[:, -tail:], index, q, k)` behind it in the same launch, and the un-rotation of the gradients in front of
    the backward launch's products (`asac_rows_proj_rope_*`); the parameter gradients are then products of the un-rotated
    gradients the backward launch writes — which is why that launch runs even where x needs no gradient."""

    @staticmethod
    def forward(ctx, x, tail, rope, wq, bq, wk, bk, wv, bv):
        x = _aligned_rows(x)
        L, qkv = x.shape[1], _qkv_outputs(x, tail)
        ws, bs = [wq.detach(), wk.detach(), wv.detach()], [bq.detach(), bk.detach(), bv.detach()]
        index = None
        if rope is None:
            native.rows_proj_forward(x, ws, bs, [tail, L, L], qkv)
        else:
            index, kind, tables = rope
            native.rows_proj_rope_forward(kind, tables, index, x, ws, bs, [tail, L, L], qkv)
        ctx.save_for_backward(x, index)
        ctx.tail, ctx.rope, ctx.params = tail, rope and rope[1:], (wq, bq, wk, bk, wv, bv)
        return tuple(qkv)

    @staticmethod
    def backward(ctx, gq, gk, gv):
        x, index = ctx.saved_tensors
        L, params, needs = x.shape[1], ctx.params, ctx.needs_input_grad
        grads = [g.contiguous() for g in (gq, gk, gv)]
        if ctx.rope is None:
            gx, *gp = _qkv_backward(needs[0], needs[3:], params, x, ctx.tail, grads)
        else:
            plain = [torch.empty_like(grads[0]), torch.empty_like(grads[1])]
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            native.rows_proj_rope_backward(*ctx.rope, index, grads, [ctx.tail, L, L], [w.detach() for w in params[0::2]], gx, plain)
            gx = gx if needs[0] else None
            gp = _qkv_param_grads(needs[3:], params, (*plain, grads[2]), _qkv_inputs(x, ctx.tail))
        return (gx, None, None, *gp)


class _QkvDenseDropFn(torch.autograd.Function):
    """`q_proj(x[:, -tail:]), k_proj(x), v_proj(x)` where each stack is ResBlock(E, E) -> LIVE nn.Dropout(p) -> nn.Linear(E, E),
    as ONE MFMA launch per pass (`asac_rows_dense_proj_dropout_*`, csrc/rows_proj.hip).  `draws`: the module's 'qkv' site — the
    masks are drawn on the device and regenerated by the backward from the counter this call's `used` holds.  `params`:
    (ResBlock weight, bias, Linear weight, bias) of q, k, v.  The twelve parameter gradients are products over the rows
    (`asac_xty`): of the pre-activation gradients with x, of the output gradients with the dropped hidden rows the forward
    wrote."""

    @staticmethod
    def forward(ctx, x, tail, draws, *params):
        ctx.draws, state, used = _unpack_draws(draws)
        x = _aligned_rows(x)
        tails = [tail, x.shape[1], x.shape[1]]
        outs, pres, hiddens = _qkv_outputs(x, tail), _qkv_outputs(x, tail), _qkv_outputs(x, tail)
        pd = [t.detach() for t in params]
        native.rows_dense_proj_dropout_forward(x, pd[0::4], pd[1::4], pd[2::4], pd[3::4], tails, outs, pres, hiddens, *ctx.draws,
                                               state, used)
        ctx.save_for_backward(x, used, *pres, *hiddens)
        ctx.tail, ctx.params = tail, params
        return tuple(outs)

    @staticmethod
    def backward(ctx, gq, gk, gv):
        x, used, *saved = ctx.saved_tensors
        pres, hiddens = saved[:3], saved[3:]
        E = x.shape[2]
        params, tails = ctx.params, [ctx.tail, x.shape[1], x.shape[1]]
        grads = [torch.zeros_like(pre) if g is None else g.contiguous() for g, pre in zip((gq, gk, gv), pres)]
        gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        gpres = [torch.empty_like(pre) for pre in pres]
        native.rows_dense_proj_dropout_backward(grads, list(pres), tails, [t.detach() for t in params[0::4]],
                                                [t.detach() for t in params[2::4]], gx, gpres, *ctx.draws, used)
        out, jobs = [gx if ctx.needs_input_grad[0] else None, None, None], []
        for j, xin in enumerate(_qkv_inputs(x, ctx.tail)):
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
        q, k = (t if t.stride(2) == 1 else t.contiguous() for t in (q, k))
        out_q, out_k = torch.empty(q.shape, dtype=q.dtype, device=q.device), torch.empty(k.shape, dtype=k.dtype, device=k.device)
        native.rope_forward(kind, tables, q, k, q_index, k_index, out_q, out_k)
        ctx.save_for_backward(q_index, k_index)
        ctx.kind, ctx.tables = kind, tables
        return out_q, out_k

    @staticmethod
    def backward(ctx, gq, gk):
        q_index, k_index = ctx.saved_tensors
        gq, gk = (g if g.stride(2) == 1 else g.contiguous() for g in (gq, gk))
        out_q, out_k = torch.empty(gq.shape, dtype=gq.dtype, device=gq.device), torch.empty(gk.shape, dtype=gk.dtype, device=gk.device)
        native.rope_backward(ctx.kind, ctx.tables, gq, gk, q_index, k_index, out_q, out_k)
        return out_q, out_k, None, None, None, None


class _OutResRowsFn(torch.autograd.Function):
    """`(x + gelu(linear(x))) * row_scale[..., None]` — the output ResBlock of an attention layer and its dead-row / padded-row
    factor — as one MFMA launch per pass (`asac_rows_resblock_*`, csrc/rows_proj.hip); the parameter gradients from `asac_xty`.
    With `draws` (the module's 'out' site): the output stack's LIVE nn.Dropout(p) between the ResBlock and the row factor,
    inside both launches (`asac_rows_resblock_dropout_*`): `dropout(x + gelu(linear(x))) * row_scale[..., None]`.
    With `y_pre` = (y, pre): the forward already ran (inside `asac_attention_mh_proj_forward`), the backward is the same."""

    @staticmethod
    def forward(ctx, x, weight, bias, row_scale, draws=None, y_pre=None):
        x2 = x.reshape(-1, x.shape[-1])
        sc = None if row_scale is None else row_scale.reshape(-1).contiguous()
        ctx.draws, state, used = _unpack_draws(draws)
        if y_pre is not None:       # (a tuple, not tensor arguments: the result must not be a view of an input)
            y, pre = y_pre[0], y_pre[1].view(x2.shape)
        else:
            x2 = _aligned_rows(x2)
            y, pre = torch.empty(x2.shape, dtype=x.dtype, device=x.device), torch.empty(x2.shape, dtype=x.dtype, device=x.device)
            if draws is None:
                native.rows_resblock_forward(x2, weight.detach(), bias.detach(), sc, y, pre)
            else:
                native.rows_resblock_dropout_forward(x2, weight.detach(), bias.detach(), sc, y, pre, *ctx.draws, state, used)
        ctx.save_for_backward(x2, pre, sc, used)
        ctx.params, ctx.lead = (weight, bias), x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        x2, pre, sc, used = ctx.saved_tensors
        weight, _ = ctx.params
        gy2 = gy.reshape(x2.shape).contiguous()
        gx, gpre = torch.empty_like(pre), torch.empty_like(pre)
        if used is None:
            native.rows_resblock_backward(gy2, pre, weight.detach(), sc, gx, gpre)
        else:
            native.rows_resblock_dropout_backward(gy2, pre, weight.detach(), sc, gx, gpre, *ctx.draws, used)
        gw, gb = _rows_param_grads(ctx.needs_input_grad[1:3], ctx.params, gpre, x2)
        return gx.view(ctx.lead), gw, gb, None, None, None


class _GateRowsFn(torch.autograd.Function):
    """`gatedlayer(x, y) * ~row_zero[..., None]` for a RESIDUAL / OUTPUT / RECURRENT gate — the gate behind an episode block's
    attention and its padded-row factor — as one launch per pass (`asac_rows_gate_*`, csrc/rows_gate.hip); the parameter
    gradients from `asac_xty` over the pre-activation gradients the backward launch writes.
    params: () / (W,) / (Wxr, Wyr, Wxz, Wyz, Wxg, Wyg, bz)"""

    @staticmethod
    def forward(ctx, kind, x, y, row_zero, *params):
        B, L, E = y.shape
        # (a view expanded along the batch or the positions — a stride of 0 — is made dense like a misaligned one: the launch
        # takes rows that do not overlap)
        if _rows_misaligned(x) or (L > 1 and x.stride(1) < E) or (B > 1 and x.stride(0) < E):
            x = x.contiguous()
        if not y.is_contiguous() or y.data_ptr() & 15:
            y = y.clone(memory_format=torch.contiguous_format)
        if row_zero is not None and ((L > 1 and row_zero.stride(1) != 1) or (B > 1 and row_zero.stride(0) < L)):
            row_zero = row_zero.contiguous()
        weights = [w.detach() for w in params[:6]]
        bz = params[6].detach() if len(params) == 7 else None
        out = torch.empty(y.shape, dtype=y.dtype, device=y.device)
        need = any(ctx.needs_input_grad)
        saved = [torch.empty_like(out) for _ in range({GATE_RESIDUAL: 0, GATE_OUTPUT: 1, GATE_RECURRENT: 3}[kind])] if need else []
        native.rows_gate_forward(kind, x, y, row_zero, weights, bz, out, saved or None)
        if need:
            ctx.save_for_backward(x, y, *saved, *([row_zero] if row_zero is not None else []))
        ctx.kind, ctx.params, ctx.masked = kind, params, row_zero is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        kind, params = ctx.kind, ctx.params
        x, y, *saved = ctx.saved_tensors
        row_zero = saved.pop() if ctx.masked else None
        E = y.shape[-1]
        if not g_out.is_contiguous() or g_out.data_ptr() & 15:
            g_out = g_out.clone(memory_format=torch.contiguous_format)
        weights = [w.detach() for w in params[:6]]
        g_x = torch.empty_like(y)
        if kind == GATE_RESIDUAL:
            native.rows_gate_backward(kind, g_out, x, y, row_zero, weights, [], g_x, g_x, [])
            return None, g_x, g_x, None
        g_y = torch.empty_like(y)
        g_pre = [torch.empty_like(y) for _ in saved]
        rx = torch.empty_like(y) if kind == GATE_RECURRENT else None
        native.rows_gate_backward(kind, g_out, x, y, row_zero, weights, saved, g_x, g_y, g_pre, rx)
        needs = ctx.needs_input_grad[4:]
        if not any(needs):
            return (None, g_x, g_y, None, *([None] * len(params)))
        x2, y2, jobs = x.reshape(-1, E), y.view(-1, E), []
        if kind == GATE_OUTPUT:
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
