"""CPU: the dense-stack dropout launches (csrc/rows_proj.hip) without a GPU — the four additive exports and their host
checks, the draw layout as tests/dense_dropout_ref.py restates it, the restatement against the module's own arithmetic, and
the float32 CPU composition fed the restated masks against the cap the GPU tests hold the kernels to."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dense_dropout_ref as ref

NEW = ('asac_rows_dense_proj_dropout_forward', 'asac_rows_dense_proj_dropout_backward',
       'asac_rows_resblock_dropout_forward', 'asac_rows_resblock_dropout_backward')
SHAPES = [(3, 7, 7, 32), (3, 7, 1, 64), (5, 9, 4, 128), (1, 9, 9, 64), (70, 9, 3, 64), (3, 7, 2, 64)]      # (B, L, tail, E)


def _declared(name):
    """the header's parameters of `name` ((name, base type, pointer depth) each), None where it declares none such"""
    from asac_amd import abi
    return abi.functions[name][1] if name in abi.functions else None


def test_the_four_exports_exist_and_the_abi_number_is_unchanged():
    from asac_amd import native
    lib = native.load()
    for name in NEW:
        params = _declared(name)
        assert params is not None and hasattr(lib, name), name
        res, args = native._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params)
        for (pname, base, depth), ct in zip(params, args):      # every declared type travels as the ctypes type of its width
            want = (C.c_void_p if depth else
                    {'int': C.c_int, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64,
                     'float': C.c_float}[base])
            assert ct is want, (name, pname, ct)
        tail = [a[0] for a in params[-7:]]
        want = ['thr', 'scale', 'seed', 'instance', 'state', 'used', 'stream']
        assert tail == want if name.endswith('forward') else tail[1:] == want[:4] + want[5:], (name, tail)
    from asac_amd import abi
    assert lib.asac_version() == abi.defines['ASAC_ABI_VERSION'] == native.ABI_VERSION == 91
    for name in NEW:
        assert callable(getattr(native, name[len('asac_'):]))


def test_host_checks_return_before_any_launch():
    """no GPU here: a call that reached a launch would report something other than hipErrorInvalidValue.  The device pointers
    are never followed; the pointer ARRAYS are host arrays and real."""
    from asac_amd import native
    lib = native.load()
    ptr, invalid_value = 0x1000, 1
    thr5 = native.dropout_threshold(0.5)
    arr = lambda n=3, p_=ptr: (C.c_void_p * n)(*[p_] * n)      # noqa: E731
    tails = lambda n=3: (C.c_int * n)(*[2] * n)                   # noqa: E731

    def dense_f(x=ptr, B=4, L=9, E=64, n=3, thr=thr5, scale=2.0, state=ptr, used=ptr, w1=None, out=None):
        m = min(n, 3)
        return lib.asac_rows_dense_proj_dropout_forward(x, 9 * E, E, B, L, E, n, w1 or arr(m), arr(m), arr(m), arr(m), tails(m),
                                                        out or arr(m), arr(m), arr(m), thr, scale, 1, 1, state, used, None)

    def dense_b(gx=ptr, B=4, L=9, E=64, n=3, thr=thr5, scale=2.0, used=ptr, g=None):
        m = min(n, 3)
        return lib.asac_rows_dense_proj_dropout_backward(g or arr(m), arr(m), tails(m), n, arr(m), arr(m), B, L, E, gx, arr(m),
                                                         thr, scale, 1, 1, used, None)

    def res_f(x=ptr, rows=36, E=64, thr=thr5, scale=2.0, state=ptr, used=ptr, y=ptr):
        return lib.asac_rows_resblock_dropout_forward(x, E, ptr, ptr, None, rows, E, y, ptr, thr, scale, 1, 1, state, used, None)

    def res_b(gy=ptr, rows=36, E=64, thr=thr5, scale=2.0, used=ptr):
        return lib.asac_rows_resblock_dropout_backward(gy, ptr, ptr, None, rows, E, ptr, ptr, thr, scale, 1, 1, used, None)

    for call in (dense_f, dense_b, res_f, res_b):
        assert call(thr=0) == invalid_value
        assert call(scale=0.5) == call(scale=float('inf')) == call(scale=float('nan')) == invalid_value
        for E in (0, 16, 48, 96, 256):
            assert call(E=E) == invalid_value, E
        assert call(used=None) == invalid_value
        assert b'dropout' in lib.asac_last_error()
    # rows * E >= 2^34
    assert dense_f(B=1 << 20, L=1 << 8, E=64) == dense_b(B=1 << 20, L=1 << 8, E=64) == invalid_value
    assert res_f(rows=1 << 28, E=64) == res_b(rows=1 << 28, E=64) == invalid_value
    assert res_f(rows=1 << 27, E=128) == res_f(rows=1 << 29, E=32) == invalid_value
    # more than three jobs, none
    assert dense_f(n=4) == dense_b(n=4) == dense_f(n=0) == dense_b(n=0) == invalid_value
    # misaligned pointers
    assert dense_f(x=ptr + 4) == dense_b(gx=ptr + 8) == res_f(x=ptr + 4) == res_f(y=ptr + 12) == res_b(gy=ptr + 4) == invalid_value
    assert dense_f(w1=arr(3, ptr + 4)) == dense_f(out=arr(3, ptr + 8)) == dense_b(g=arr(3, ptr + 4)) == invalid_value
    assert dense_f(state=None) == res_f(state=None) == invalid_value


def test_the_four_tags_give_four_masks():
    masks = [ref.rows_mask(11, 3, 7, tag, 64, 64, 0.5) for tag in (ref.TAG_Q, ref.TAG_K, ref.TAG_V, ref.TAG_OUT)]
    assert len({m.tobytes() for m in masks}) == 4
    for a in range(4):
        for b in range(a + 1, 4):      # unrelated, not shifted copies: about half of the entries differ
            assert 0.4 < (masks[a] != masks[b]).mean() < 0.6
    # another counter, instance or seed: another mask
    for other in (dict(counter=8), dict(instance=4), dict(seed=12)):
        args = dict(seed=11, instance=3, counter=7)
        args.update(other)
        assert (ref.rows_mask(tag=ref.TAG_Q, rows=64, E=64, p=0.5, **args) != masks[0]).any()


def test_an_entry_does_not_depend_on_tail_or_on_the_number_of_rows():
    big = ref.rows_mask(5, 2, 1, ref.TAG_K, 630, 64, 0.5)
    small = ref.rows_mask(5, 2, 1, ref.TAG_K, 21, 64, 0.5)
    assert (big[:21] == small).all()
    B, L, E = 3, 7, 64
    q_all = ref.qkv_masks(5, 2, 1, B, L, L, E, 0.5)[0]
    for tail in (1, 2, 6):
        q = ref.qkv_masks(5, 2, 1, B, L, tail, E, 0.5)[0]
        assert q.shape == (B, tail, E) and (q == q_all[:, L - tail:]).all()
    # the width is part of the layout: entry (r, f) of another width is another draw
    assert (ref.rows_mask(5, 2, 1, ref.TAG_K, 21, 32, 0.5) != small[:, :32]).any()


@pytest.mark.parametrize('p', [0.005, 0.2, 0.5])
def test_dropped_share_of_a_fixed_draw(p):
    kept = ref.rows_mask(seed=1234, instance=3, counter=7, tag=ref.TAG_OUT, rows=4096, E=64, p=p)
    n = kept.size
    assert n == 1 << 18
    dropped, sigma = 1.0 - kept.mean(), (p * (1 - p) / n) ** 0.5
    assert abs(dropped - p) <= 4 * sigma, (dropped, p, sigma)


@pytest.mark.parametrize('pe', [None, 'ROPE', 'ROPE2'])
def test_restatement_without_drops_is_the_module(pe):
    """all-kept masks and s = 1 (p = 0): the float64 restatement is the module's own arithmetic in `.eval()`"""
    from algorithm.nn_models.layers.seq_layers import POSITIONAL_ENCODING
    B, L, q_len, E, H = 3, 7, 3, 64, 2
    layer = ref.make_layer(E, H, None if pe is None else POSITIONAL_ENCODING[pe]).double().eval()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(B, L, E, generator=gen, dtype=torch.float64)
    am = torch.rand(B, q_len, L, generator=gen) < 0.4
    am[0, 0] = True
    rz = torch.rand(B, q_len, generator=gen) < 0.3
    ki = torch.arange(L).unsqueeze(0).expand(B, -1) + torch.arange(B).unsqueeze(1)
    qi = ki[:, -q_len:]
    want = layer(x[:, -q_len:], x, x, query_index=qi, key_index=ki, attn_mask=am, out_row_mask=rz)
    ones = dict(q=np.ones((B, q_len, E), bool), k=np.ones((B, L, E), bool), v=np.ones((B, L, E), bool),
                w=np.ones((B, H, q_len, L), bool), out=np.ones((B, q_len, E), bool))
    got = ref.module_forward(copy.deepcopy(layer), x, q_len, ones, 0.0, qi, ki, am, None, rz)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def test_cpu_tensors_run_the_module_code():
    from algorithm.nn_models.layers import seq_layers
    assert isinstance(seq_layers.FUSED_DENSE_DROPOUT, bool)
    layer = ref.make_layer(64, 2, p=0.5)
    assert layer.training
    keys = set(layer.state_dict())
    x = torch.randn(3, 7, 64, requires_grad=True)
    out, w = layer(x[:, -2:], x, x)
    (out.sum() + w.sum()).backward()
    assert out.shape == (3, 2, 64) and torch.isfinite(x.grad).all()
    # module code: torch's dropout zeroed about half of the output block's entries; no device state, no new state_dict key
    assert 0.3 < float((out == 0).float().mean()) < 0.7
    assert layer.dense_dropout_state('qkv') is None and layer.dense_dropout_state('out') is None
    assert set(layer.state_dict()) == keys
    for site in ('qkv', 'out'):
        with pytest.raises(RuntimeError):
            layer.dense_dropout_drawn(site)


def test_recognisers_ask_the_dropout_modules_own_state():
    from torch import nn
    from algorithm.nn_models.layers import seq_layers as sl
    layer = ref.make_layer(64, 2, p=0.5)
    assert sl._dropout_dense_stack(layer.q_proj, 64) is not None and sl._dropout_resblock(layer.out_proj, 64) is not None
    assert sl._plain_linear(layer.q_proj) is None and sl._plain_resblock(layer.out_proj, 64) is None
    assert sl._dropout_dense_stack(layer.q_proj, 32) is None and sl._dropout_dense_stack(layer.out_proj, 64) is None
    for mod in layer.modules():
        if isinstance(mod, nn.Dropout):
            mod.eval()
    assert layer.training      # the attention module itself stays in training mode
    assert sl._dropout_dense_stack(layer.q_proj, 64) is None and sl._dropout_resblock(layer.out_proj, 64) is None
    for p in (0., 1.):
        other = ref.make_layer(64, 2, p=p)
        assert sl._dropout_dense_stack(other.q_proj, 64) is None and sl._dropout_resblock(other.out_proj, 64) is None
    deep = ref.make_layer(64, 2, p=0.5)
    deep.out_proj = type(deep.out_proj)(64, dense_n=64, dense_depth=2, dropout=0.5)
    assert sl._dropout_resblock(deep.out_proj, 64) is None


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('B,L,tail,E', SHAPES)
def test_float32_composition_stays_inside_the_cap(B, L, tail, E, p):
    c = ref.case(B, L, tail, E, p)
    args = (tail, c['params'], c['lin_out'], c['kept'], c['kept_out'], p, c['g_outs'], c['g_y'], c['row_scale'])
    got, want = ref.composition(c['x'], *args), ref.composition(c['x'].double(), *args)
    worst = 0.
    for name in want:
        frac = ref.fraction_of_cap(got[name], want[name], p, ref.param_rows(name, B, L, tail))
        worst = max(worst, frac)
        assert frac <= 1.0, (name, frac)
    print(f'float32 composition {(B, L, tail, E)} p={p}: at most {worst:.4f} of the cap')
