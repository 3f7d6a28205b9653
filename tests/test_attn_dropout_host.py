"""CPU: the draw contract of the attention-weight dropout (csrc/asac_dropout.h) as tests/attn_dropout_ref.py restates it —
Philox4x32-10 against the published Random123 known-answer vectors, the threshold, the statistics and the independence of
the restated mask — and the additive ABI of the two dropout entry points and the Python gate."""

import numpy as np
import pytest
import torch

from tests import attn_dropout_ref as ref


# Random123 (kat_vectors, philox4x32 with 10 rounds): counter, key -> output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize('counter,key,want', KAT)
def test_philox_restatement_matches_the_published_vectors(counter, key, want):
    got = ref.philox4x32_10([np.array([w], dtype=np.uint32) for w in counter], key)
    assert tuple(int(w[0]) for w in got) == want


def test_philox_restatement_is_elementwise():
    """a vector of counters gives what each counter gives alone (the mask is built from one vectorised call)"""
    idx = np.array([0, 1, 7, 0xFFFFFFFF, 123456789], dtype=np.uint32)
    many = ref.philox4x32_10((idx, 5 << 28 | 3, 9, 0), (11, 0))
    for n, i in enumerate(idx):
        one = ref.philox4x32_10((np.array([i], dtype=np.uint32), 5 << 28 | 3, 9, 0), (11, 0))
        assert [int(w[n]) for w in many] == [int(w[0]) for w in one]


@pytest.mark.parametrize('p,thr', [(0.005, 21474836), (0.01, 42949672), (0.2, 858993459), (0.5, 2147483648)])
def test_threshold(p, thr):
    from asac_amd import native
    assert ref.threshold(p) == thr == native.dropout_threshold(p)
    assert native.dropout_scale(p) == ref.scale(p) == float(np.float32(1.0 / (1.0 - p)))


@pytest.mark.parametrize('p', [0.005, 0.2])
def test_dropped_fraction_and_independence_of_the_restated_mask(p):
    B, H, L = 256, 8, 9
    kept = ref.mask(seed=1234, instance=3, counter=7, B=B, H=H, Lq=L, Lk=L, p=p)
    assert kept.shape == (B, H, L, L) and kept.dtype == bool
    n = kept.size
    assert n == 165888
    dropped = 1.0 - kept.mean()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(dropped - p) <= 5 * sigma, (dropped, p, sigma)
    # no two heads and no two batch entries share a mask: the 81 words behind each (entry, head) are its own ...
    w = ref.words(seed=1234, instance=3, counter=7, B=B, H=H, Lq=L, Lk=L)
    assert len({row.tobytes() for row in w.reshape(B * H, L * L)}) == B * H
    assert (kept == (w >= ref.threshold(p))).all()
    if p == 0.2:
        # ... and so are the 81 bits (at p = 0.005 two thirds of these small masks drop nothing at all and are alike for
        # that reason: 0.995^81 = 0.67; there the bits are compared per head over the whole batch)
        assert len({row.tobytes() for row in kept.reshape(B * H, L * L)}) == B * H
        assert len({row.tobytes() for row in kept.reshape(B, H * L * L)}) == B
    per_head = kept.transpose(1, 0, 2, 3).reshape(H, B * L * L)
    assert len({row.tobytes() for row in per_head}) == H
    # another counter, instance or seed: another mask
    for other in (dict(counter=8), dict(instance=4), dict(seed=1235)):
        args = dict(seed=1234, instance=3, counter=7)
        args.update(other)
        assert (ref.mask(B=B, H=H, Lq=L, Lk=L, p=p, **args) != kept).any()


def test_mask_layout_does_not_depend_on_the_window():
    """entry (b, h, i, j) is the same draw whatever Lq and Lk are (a Philox block may hang over the window's edge)"""
    big = ref.mask(5, 2, 1, B=3, H=2, Lq=32, Lk=32, p=0.5)
    small = ref.mask(5, 2, 1, B=3, H=2, Lq=7, Lk=5, p=0.5)
    assert (big[:, :, :7, :5] == small).all()


def _declared(name):
    """the header's parameters of `name` ((name, base type, pointer depth) each), None where it declares none such"""
    from asac_amd import abi
    return abi.functions[name][1] if name in abi.functions else None


def test_abi_is_additive():
    import ctypes as C
    from asac_amd import native
    lib = native.load()
    fwd, bwd = _declared('asac_attention_mh_dropout_forward'), _declared('asac_attention_mh_dropout_backward')
    plain_f, plain_b = _declared('asac_attention_mh_forward'), _declared('asac_attention_mh_backward')
    assert fwd is not None and bwd is not None
    # the arguments of the plain entry points, then thr, scale, seed, instance, (state,) used, stream
    assert fwd[:len(plain_f) - 1] == plain_f[:-1] and bwd[:len(plain_b) - 1] == plain_b[:-1]
    assert [a[0] for a in fwd[len(plain_f) - 1:]] == ['thr', 'scale', 'seed', 'instance', 'state', 'used', 'stream']
    assert [a[0] for a in bwd[len(plain_b) - 1:]] == ['thr', 'scale', 'seed', 'instance', 'used', 'stream']
    for name, params in (('asac_attention_mh_dropout_forward', fwd), ('asac_attention_mh_dropout_backward', bwd)):
        assert hasattr(lib, name)
        res, args = native._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params)
        for (pname, base, depth), ct in zip(params, args):      # every declared type travels as the ctypes type of its width
            want = (C.c_void_p if depth else
                    {'int': C.c_int, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64,
                     'float': C.c_float}[base])
            assert ct is want, (name, pname, ct)
    assert len(_declared('asac_attention_mh_forward')) == 19 and len(_declared('asac_attention_mh_backward')) == 19
    from asac_amd import abi
    assert lib.asac_version() == abi.defines['ASAC_ABI_VERSION'] == native.ABI_VERSION == 91
    assert callable(native.attention_mh_dropout_forward) and callable(native.attention_mh_dropout_backward)


def test_host_checks_refuse_what_the_draw_layout_cannot_hold():
    """the entry points return before any launch (so this needs no GPU; the pointers are never followed): thr = 0 (p below
    2^-32, p = 0), a scale below 1 or not finite (p outside (0, 1)), and more than 2^24 (batch entry, head) pairs"""
    from asac_amd import native
    lib = native.load()
    ptr = 0x1000

    def fwd(B=4, heads=2, thr=native.dropout_threshold(0.5), scale=2.0, state=ptr, used=ptr):
        return lib.asac_attention_mh_dropout_forward(ptr, ptr, ptr, None, 0, 0, 0, B, 9, 9, heads, 8, ptr, ptr, ptr, None, None,
                                                     None, thr, scale, 1, 1, state, used, None)

    def bwd(B=4, heads=2, thr=native.dropout_threshold(0.5), scale=2.0, used=ptr):
        return lib.asac_attention_mh_dropout_backward(ptr, ptr, ptr, None, 0, 0, 0, B, 9, 9, heads, 8, ptr, ptr, None, ptr, ptr,
                                                      ptr, thr, scale, 1, 1, used, None)

    invalid_value = 1      # hipErrorInvalidValue: what `bad_arg` returns (a launch that failed would report something else)
    for call in (fwd, bwd):
        assert call(thr=0) == invalid_value
        assert call(scale=0.5) == call(scale=float('inf')) == call(scale=float('nan')) == invalid_value
        assert call(B=(1 << 21) + 1, heads=8) == invalid_value           # B * heads = 2^24 + 8
        assert call(used=None) == invalid_value
        assert b'asac_attention_mh_dropout' in lib.asac_last_error()
    assert fwd(state=None) == invalid_value
    assert native.dropout_threshold(0.) == 0 and native.dropout_threshold(2.0 ** -33) == 0


def test_cpu_tensors_run_the_module_code():
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import seq_layers
    assert seq_layers.FUSED_ATTN_DROPOUT is True
    torch.manual_seed(0)
    layer = m.MultiheadAttention(24, 2, out_dense_depth=1, dropout=0.5)
    assert layer.training
    keys = set(layer.state_dict())
    x = torch.randn(3, 7, 24, requires_grad=True)
    out, w = layer(x, x, x)
    (out.sum() + w.sum()).backward()
    assert out.shape == (3, 7, 24) and w.shape == (3, 7, 7) and torch.isfinite(x.grad).all()
    # module code: torch's dropout zeroed about half of the weights of both heads; no device state, no new state_dict key
    assert 0.05 < float((w == 0).float().mean()) < 0.6
    assert layer.dropout_state() is None and set(layer.state_dict()) == keys
    with pytest.raises(RuntimeError):
        layer.dropout_drawn()


def test_restated_core_without_drops_is_the_module():
    """the float64 restatement with an all-kept mask and s = 1 (p = 0) is the module's own arithmetic: dead rows and all"""
    import copy
    import algorithm.nn_models as m
    torch.manual_seed(1)
    layer = m.MultiheadAttention(24, 2, out_dense_depth=1).double()
    gen = torch.Generator().manual_seed(2)
    B, Lq, Lk = 3, 7, 5
    q, k, v = (torch.randn(B, L, 24, generator=gen, dtype=torch.float64) for L in (Lq, Lk, Lk))
    am = torch.rand(B, Lq, Lk, generator=gen) < 0.4
    am[0, 0] = True
    am[1] = True
    kpm = torch.rand(B, Lk, generator=gen) < 0.3
    rz = torch.rand(B, Lq, generator=gen) < 0.3
    want = layer(q, k, v, attn_mask=am, key_padding_mask=kpm, out_row_mask=rz)
    got = ref.module_forward(copy.deepcopy(layer), q, k, v, np.ones((B, 2, Lq, Lk), bool), 0.0, am, kpm, rz)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
