"""Restatements the dense-stack dropout tests compare against (nothing is compared with torch's own dropout draws):

* the draw layout of the row launches (csrc/rows_proj.hip under the contract of csrc/asac_dropout.h) in NumPy — `rows_mask`;
* the two functions with the masks as INPUTS, in float64 torch, gradients by autograd — `dense_stacks`, `resblock`;
* a self-attention `MultiheadAttention` with dense stacks around `attn_dropout_ref.core`, fed all five of its masks —
  `module_forward`.
"""
import numpy as np
import torch
from torch.nn.functional import gelu

from tests.attn_dropout_ref import blocked_mask, core, mask as weights_mask, philox4x32_10, scale, threshold

TAG_Q, TAG_K, TAG_V, TAG_OUT = 6, 7, 8, 9


def rows_words(seed, instance, counter, tag, rows, E):
    """uint32 [rows, E]: entry (r, f) is word f & 3 of block r * (E / 4) + (f >> 2), the tag in the second counter word"""
    assert E % 4 == 0 and rows * E < 1 << 34
    r, f4 = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(E // 4, dtype=np.uint64), indexing='ij')
    second = (int(tag) << 28) | (int(instance) & 0x0FFFFFFF)
    counter, seed = int(counter) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    out = philox4x32_10((r * np.uint64(E // 4) + f4, second, counter & 0xFFFFFFFF, counter >> 32),
                        (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1).reshape(rows, E)


def rows_mask(seed, instance, counter, tag, rows, E, p):
    """bool [rows, E], True = KEPT: the entry's word is >= floor(p * 2^32)"""
    assert 0. < p < 1.
    return rows_words(seed, instance, counter, tag, rows, E) >= np.uint32(threshold(p))


def qkv_masks(seed, instance, counter, B, L, tail, E, p):
    """the kept masks of the q / k / v jobs, [B, tail, E], [B, L, E], [B, L, E]: row r = b * L + t is the position in the FULL
    window, so the q job's mask is the newest `tail` positions of a full-window mask"""
    full = [rows_mask(seed, instance, counter, tag, B * L, E, p).reshape(B, L, E) for tag in (TAG_Q, TAG_K, TAG_V)]
    return [full[0][:, L - tail:], full[1], full[2]]


def _as(m, like):
    return torch.as_tensor(np.ascontiguousarray(m), dtype=like.dtype)


def dense_stack(x, w1, b1, w2, b2, kept, s):
    """one stack ResBlock -> Dropout -> Linear over rows x [..., E] -> (out, pre, h)"""
    pre = x @ w1.T + b1
    h = (x + gelu(pre)) * _as(kept, x) * s
    return h @ w2.T + b2, pre, h


def dense_stacks(x, tail, params, kept, p):
    """float64 x [B, L, E]; params: (w1, b1, w2, b2) of q, k, v; kept: `qkv_masks` -> [(out, pre, h)] of q, k, v"""
    L = x.shape[1]
    return [dense_stack(x[:, L - t:], *params[4 * j:4 * j + 4], kept[j], scale(p)) for j, t in enumerate((tail, L, L))]


def resblock(x, w, b, kept, p, row_scale=None):
    """float64 x [rows, E] -> y = (x + gelu(x W^T + b)) (.) M s * row_scale"""
    y = (x + gelu(x @ w.T + b)) * _as(kept, x) * scale(p)
    return y if row_scale is None else y * row_scale.unsqueeze(-1)


def module_masks(seed, instance, counters, B, L, q_len, E, H, p):
    """the five kept masks of one pass of a self-attention block, from the counters (qkv, core, out) its launches report"""
    mq, mk, mv = qkv_masks(seed, instance, counters[0], B, L, q_len, E, p)
    return dict(q=mq, k=mk, v=mv, w=weights_mask(seed, instance, counters[1], B, H, q_len, L, p),
                out=rows_mask(seed, instance, counters[2], TAG_OUT, B * q_len, E, p).reshape(B, q_len, E))


def module_forward(layer64, x, q_len, kept, p, query_index=None, key_index=None, attn_mask=None, key_padding_mask=None,
                   out_row_mask=None):
    """a float64 CPU `MultiheadAttention(E, H, pe in (None, ROPE, ROPE2), qkv_dense_depth=1, out_dense_depth=1)` applied to
    (x[:, -q_len:], x, x), fed all of its masks (`module_masks`; p = 0 with all-kept masks: s = 1, no drop)"""
    B, L, _ = x.shape
    params = [t for ll in (layer64.q_proj, layer64.k_proj, layer64.v_proj)
              for t in (ll.dense[0].linear.weight, ll.dense[0].linear.bias, ll.dense[2].weight, ll.dense[2].bias)]
    (q, _, _), (k, _, _), (v, _, _) = dense_stacks(x, q_len, params, [kept['q'], kept['k'], kept['v']], p)
    if hasattr(layer64, 'rope'):
        q, k = layer64.rope(query_index, key_index, q, k)
    out, w, keep = core(q, k, v, layer64.num_heads, blocked_mask(B, q_len, L, attn_mask, key_padding_mask), kept['w'], p)
    lin = layer64.out_proj.dense[0].linear
    row_scale = keep if out_row_mask is None else keep * (~out_row_mask).to(keep.dtype)
    y = resblock(out.reshape(B * q_len, -1), lin.weight, lin.bias, kept['out'].reshape(B * q_len, -1), p, row_scale.reshape(-1))
    return y.view(B, q_len, -1), w


# ---- what the host and the GPU tests share: modules, cases, the composition, the cap ----
def make_layer(E=64, H=2, pe=None, p=0.5, seed=1):
    import algorithm.nn_models as m
    torch.manual_seed(seed)
    layer = m.MultiheadAttention(E, H, pe=pe, qkv_dense_depth=1, out_dense_depth=1, dropout=p)
    with torch.no_grad():      # (the biases start at zero: give them values)
        for name, t in layer.named_parameters():
            if name.endswith('bias'):
                t.normal_(0., 0.1)
    return layer


def fraction_of_cap(got, want, p, param_rows=None):
    """max over the entries of |got - want| / (s (rtol |want| + atol)), rtol 3e-4; atol 3e-5 for outputs and input gradients,
    2e-7 rows max(1, sqrt(max |want|)) + 3e-5 for a parameter gradient summed over `param_rows` rows
    (tests/test_attn_dropout_gpu.py::_fraction_of_cap with the row count in place of B * Lq)"""
    s = 1.0 / (1.0 - p)
    atol = 3e-5 if param_rows is None else 2e-7 * param_rows * max(1.0, float(np.abs(want).max()) ** 0.5) + 3e-5
    return float((np.abs(got - want) / (s * (3e-4 * np.abs(want) + atol))).max())


def composition(x, tail, params, lin_out, kept, kept_out, p, g_outs, g_y, row_scale):
    """the two functions composed in the dtype of `x` from the restated masks -> named arrays: out_j, grad_x, the twelve
    parameter gradients; y, gx, dW, db of the output block over the q job's output rows"""
    dt = x.dtype
    x = x.clone().requires_grad_(True)
    params = [t.detach().to(dt).requires_grad_(True) for t in params]
    outs = dense_stacks(x, tail, params, kept, p)
    sum((o * g.to(dt)).sum() for (o, _, _), g in zip(outs, g_outs)).backward()
    res = {f'out_{n}': o.detach().numpy() for n, (o, _, _) in zip('qkv', outs)}
    res['grad_x'] = x.grad.numpy()
    for j, n in enumerate('qkv'):
        for i, kind in enumerate(('dW1', 'db1', 'dW2', 'db2')):
            res[f'{kind}_{n}'] = params[4 * j + i].grad.numpy()
    E = x.shape[-1]
    xo = x.detach()[:, x.shape[1] - tail:].reshape(-1, E).clone().requires_grad_(True)      # (the block's input: the newest rows of x)
    w, b = (t.detach().to(dt).requires_grad_(True) for t in lin_out)
    y = resblock(xo, w, b, kept_out, p, None if row_scale is None else row_scale.to(dt))
    (y * g_y.to(dt)).sum().backward()
    res.update(y=y.detach().numpy(), gx=xo.grad.numpy(), dW=w.grad.numpy(), db=b.grad.numpy())
    return res


def case(B, L, tail, E, p, counter=3, seed=20240229, instance=77):
    """parameters, inputs and restated masks of a shape: shared by this file and tests/test_dense_dropout_gpu.py"""
    layer = make_layer(E, 2, p=p, seed=E + L)
    params = [t.detach() for ll in (layer.q_proj, layer.k_proj, layer.v_proj)
              for t in (ll.dense[0].linear.weight, ll.dense[0].linear.bias, ll.dense[2].weight, ll.dense[2].bias)]
    lin_out = [layer.out_proj.dense[0].linear.weight.detach(), layer.out_proj.dense[0].linear.bias.detach()]
    gen = torch.Generator().manual_seed(B * 1000 + L * 10 + tail)
    x = torch.randn(B, L, E, generator=gen)
    g_outs = [torch.randn(B, t, E, generator=gen) for t in (tail, L, L)]
    g_y = torch.randn(B * tail, E, generator=gen)
    row_scale = (torch.rand(B * tail, generator=gen) < 0.7).float()
    row_scale[0] = 0.
    kept = qkv_masks(seed, instance, counter, B, L, tail, E, p)
    kept_out = rows_mask(seed, instance, counter, TAG_OUT, B * tail, E, p)
    return dict(x=x, params=params, lin_out=lin_out, g_outs=g_outs, g_y=g_y, row_scale=row_scale, kept=kept, kept_out=kept_out)


def param_rows(name, B, L, tail):
    """how many rows a parameter gradient is summed over, or None for outputs and input gradients"""
    if not name.startswith('d'):
        return None
    return B * tail if name in ('dW', 'db') or name.endswith('_q') else B * L
