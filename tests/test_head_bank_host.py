"""Host: what `algorithm/fused_heads.describe_head_bank` accepts and rejects, the limits of `asac_head_bank_supported` at their
edges, and the head-bank entry points in the tables `abi.py` derives from the header (no GPU)."""
import pytest
import torch
from torch import nn


def _lists(S=6, W=64, depth=3, sizes=(3, 2), G=2, **kw):
    from algorithm.nn_models.layers import LinearLayers
    return [nn.ModuleList([LinearLayers(S, W, depth, s, **kw) for s in sizes]) for _ in range(G)]


def _describe(groups):
    from algorithm import fused_heads
    return fused_heads.describe_head_bank(groups, require_device=False)


def test_describe_accepts_the_stock_and_the_128_wide_compositions():
    import asac_amd  # noqa: F401
    from algorithm.nn_models import ModelPolicy, ModelQ
    shape = _describe(_lists())
    assert (shape.S, shape.W, shape.residual, shape.sizes, shape.G) == (6, 64, (False, True, True), (3, 2), 2)
    assert len(shape.stacks) == 4 and all(len(st) == 8 for st in shape.stacks)
    q = ModelQ(6, (3, 2), 0, False)
    pi = ModelPolicy(6, (3, 2), 0)
    assert _describe([q.d_dense_list]).G == 1 and _describe([pi.d_dense_list]).sizes == (3, 2)
    # group-major, each stack (w_0, b_0, .., head w, head b): the order of the modules' own parameters
    got = [id(p) for st in _describe([q.d_dense_list]).stacks for p in st]
    assert got == [id(p) for p in q.d_dense_list.parameters()]
    wide = _describe(_lists(W=128, depth=2))
    assert (wide.W, wide.residual) == (128, (False, True))
    assert _describe(_lists(W=128, depth=1, G=1)).residual == (False,)
    assert _describe(_lists(S=64, W=64)).residual == (True, True, True)
    # on the device only, unless told otherwise: host parameters are no bank for the launches
    from algorithm import fused_heads
    assert fused_heads.describe_head_bank(_lists()) is None


def test_describe_rejects_what_the_kernel_does_not_compute():
    import asac_amd  # noqa: F401
    from algorithm.nn_models.layers import LinearLayers
    assert _describe(_lists(dropout=0.2)) is None, 'a live dropout'
    assert _describe(_lists(dropout=0.)) is not None
    mixed_w = _lists()
    mixed_w[1][0] = LinearLayers(6, 128, 3, 3)
    assert _describe(mixed_w) is None, 'mixed widths'
    inner = _lists()
    inner[0][1] = LinearLayers(6, [64, 128, 128], 3, 2)
    assert _describe(inner) is None, 'one stack of two widths'
    mixed_d = _lists()
    mixed_d[0][1] = LinearLayers(6, 64, 2, 2)
    assert _describe(mixed_d) is None, 'mixed depths'
    no_head = _lists()
    no_head[0][0] = LinearLayers(6, 64, 3)
    assert _describe(no_head) is None, 'a missing head'
    assert _describe(_lists(activation=nn.ReLU)) is None, 'another activation'
    assert _describe(_lists(activation=lambda: nn.GELU(approximate='tanh'))) is None, 'the tanh GELU'
    unequal = _lists()
    unequal[1][0] = LinearLayers(6, 64, 3, 4)
    assert _describe(unequal) is None, 'unequal branch sizes across groups'
    flags = _lists(S=64)
    flags[0][0] = LinearLayers(64, 64, 3, 3, residual=False)
    assert _describe(flags) is None, 'unequal residual flags'
    assert _describe(_lists(depth=0)) is None, 'no ResBlock at all'
    assert _describe(_lists(W=96)) is not None and _describe(_lists(W=32)) is not None, 'zero-padded tiles'
    assert _describe(_lists(W=160, G=1)) is None, 'a width the kernel refuses'
    assert _describe(_lists(sizes=(65,), G=1)) is None, 'a branch of 65 logits'
    half = _lists()
    for p in half[0][0].parameters():
        p.data = p.data.half()
    assert _describe(half) is None, 'parameters that are not float32'
    assert _describe([]) is None and _describe([nn.ModuleList()]) is None
    assert _describe([[nn.Linear(6, 3)]]) is None, 'not a LinearLayers'


@pytest.mark.parametrize('args,ok', [
    ((6, 64, 3, 2, 5, 2), True), ((6, 128, 1, 2, 5, 2), True),
    ((128, 64, 1, 1, 1, 1), True), ((129, 64, 1, 1, 1, 1), False), ((0, 64, 1, 1, 1, 1), False),
    ((6, 64, 0, 2, 5, 2), False), ((6, 64, 4, 2, 5, 2), False),
    ((6, 32, 1, 2, 5, 2), True), ((6, 96, 1, 2, 5, 2), True), ((6, 1, 1, 2, 5, 2), True), ((6, 0, 1, 2, 5, 2), False),
    ((6, 129, 1, 2, 5, 2), False), ((6, 256, 1, 2, 5, 2), False),
    ((6, 64, 1, 8, 64, 8), True), ((6, 64, 1, 9, 64, 7), False), ((6, 64, 1, 0, 5, 1), False),
    ((6, 64, 1, 1, 64, 1), True), ((6, 64, 1, 1, 65, 1), False), ((6, 64, 1, 3, 2, 1), False),
    ((6, 64, 1, 2, 5, 8), True), ((6, 64, 1, 2, 5, 9), False), ((6, 64, 1, 2, 5, 0), False)])
def test_supported_agrees_with_the_documented_limits(args, ok):
    """(S, W, depth, K, D, G): S <= 128; W <= 128 (narrower than 64 / 128: zero-padded tiles); 1 <= depth <= 3; K <= 8; K <= D <= 64; G <= 8 (so M <= 64)"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    assert bool(native.load().asac_head_bank_supported(*args)) == ok


def test_the_entry_points_and_the_struct_are_in_the_derived_tables():
    import asac_amd  # noqa: F401
    from asac_amd import abi, native
    for name in ('asac_head_bank_supported', 'asac_head_bank_forward', 'asac_head_bank_backward',
                 'asac_head_bank_backward_workspace'):
        assert name in abi.functions and name in native.EXPORTED_SYMBOLS
        assert hasattr(native.load(), name)
    fields = [f[0] for f in abi.structs['asac_head_bank_t']]
    assert fields == ['S', 'W', 'depth', 'G', 'residual', 'reserved_', 'branches']
    assert native.HeadBankDesc is abi.ctypes_struct('asac_head_bank_t')
    assert abi.defines['ASAC_HEAD_BANK_MAX_ROWS'] == 1 << 20 and abi.defines['ASAC_HEAD_BANK_MAX_DEPTH'] == 3
    d = native.head_bank_desc(6, 128, (False, True), (3, 2), 2)
    assert (d.S, d.W, d.depth, d.G, d.branches.K, d.branches.D) == (6, 128, 2, 2, 2, 5)
    assert list(d.residual) == [0, 1, 0]
    ret, params = abi.functions['asac_head_bank_backward']
    assert ret == 'int' and [p[0] for p in params][:3] == ['bank', 'params', 'grads']
