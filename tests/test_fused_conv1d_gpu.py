"""GPU: the ray encoder's one-launch convolution stack (`asac_conv1_forward` / `asac_conv1_backward`, csrc/conv1d.hip) against
a float64 copy of the module stack it replaces — Conv1d LeakyReLU Conv1d LeakyReLU over `x.permute(0, 2, 1)` — for the
flattened activations and the gradients of the four parameter tensors.

Yardstick: the module path itself.  For y and each gradient, err(a) = max|a - ref64| / max|ref64|; e_mod is the larger of
that error of the f32 module run by ATen on the device and of the f32 module on the CPU; the kernel must hold
err <= max(4 e_mod, sqrt(n) 2^-24) with n the tensor's reduction length (C k1 + out1 k2 for y, N L2 for w2 / b2, N L1 for
w1 / b1): 4x is the project's margin, the second term the random-walk rounding of any f32 summation
order.  The observed figures are recorded in tests/conv1d_tolerances.json.

A pre-activation closer to zero than f32 rounding can take the other LeakyReLU slope in f32, which moves a gradient by a
whole term; the inputs are therefore chosen (seed per case) so that no element of z1 or z2 of the float64 reference lies within
1e-6 of zero, and the test asserts that first: a condition on the inputs, not a tolerance."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

# (N, L, C, out1, k1, s1, out2, k2, s2) -> seed
CASES = {
    (37, 400, 2, 16, 8, 4, 32, 4, 2): 1,     # ugv rays, ragged last group, L1 = 99, L2 = 48
    (130, 61, 2, 16, 8, 4, 32, 4, 2): 0,     # usv rays, tiles span rays, L1 = 14, L2 = 6
    (1, 400, 2, 16, 8, 4, 32, 4, 2): 1,      # less than one group
    (19, 67, 3, 12, 4, 2, 20, 4, 3): 0,      # channel counts not multiples of 16, stride 3, L1 = 32, L2 = 10
    (9, 802, 2, 16, 8, 4, 32, 4, 2): 1,      # long ray, L1 = 199, L2 = 98
    (23, 64, 1, 16, 8, 4, 32, 4, 2): 0,      # one channel, K1 = 8
    (11, 100, 2, 16, 8, 4, 32, 3, 1): 1,     # overlapping second layer (3 col2im contributions), K2 = 48
}
NAMES = ('y', 'w1', 'b1', 'w2', 'b2')


def _build(case):
    N, L, C, o1, k1, s1, o2, k2, s2 = case
    seed = CASES[case]
    torch.manual_seed(seed)
    ref = nn.Sequential(nn.Conv1d(C, o1, k1, s1), nn.LeakyReLU(), nn.Conv1d(o1, o2, k2, s2), nn.LeakyReLU())
    x = torch.randn(N, L, C, generator=torch.Generator().manual_seed(seed + 1000))
    l1 = (L - k1) // s1 + 1
    l2 = (l1 - k2) // s2 + 1
    gy = torch.randn(N, o2 * l2, generator=torch.Generator().manual_seed(seed + 2000))
    return ref, x, gy, l1, l2


def _module_run(stack, x, gy):
    """[y, dw1, db1, dw2, db2] of the module path on x's device in x's dtype"""
    stack.zero_grad(set_to_none=True)
    y = stack(x.permute(0, 2, 1)).reshape(x.shape[0], -1)
    (y * gy).sum().backward()
    return [y.detach().double().cpu()] + [p.grad.detach().double().cpu() for p in stack.parameters()]


def _err(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def _reference(case):
    """-> (ref64 outputs, e_mod per tensor, min |z| of the float64 pre-activations); computed once per case"""
    ref, x, gy, l1, l2 = _build(case)
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        z1 = ref64[0](x.double().permute(0, 2, 1))
        z2 = ref64[2](ref64[1](z1))
    min_z = min(float(z1.abs().min()), float(z2.abs().min()))
    want = _module_run(ref64, x.double(), gy.double())
    cpu32 = _module_run(copy.deepcopy(ref), x, gy)
    dev32 = _module_run(copy.deepcopy(ref).cuda(), x.cuda(), gy.cuda())
    e_mod = [max(_err(a, w), _err(b, w)) for a, b, w in zip(cpu32, dev32, want)]
    return want, e_mod, min_z


@pytest.mark.parametrize('case', list(CASES), ids=lambda c: 'x'.join(map(str, c)))
def test_fused_conv1d_stack_matches_the_float64_modules(case):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused_conv import conv1d_stack_desc, fused_conv1d_stack
    N, L, C, o1, k1, s1, o2, k2, s2 = case
    ref, x, gy, l1, l2 = _build(case)
    want, e_mod, min_z = _reference(case)
    assert min_z > 1e-6, f'a pre-activation within 1e-6 of the LeakyReLU kink ({min_z:.3g}): pick the next seed'
    dev = copy.deepcopy(ref).cuda()
    xd, gyd = x.cuda(), gy.cuda()
    desc = conv1d_stack_desc(dev, xd)
    assert desc is not None and native.conv1_out_shape(desc) == (l1, l2)
    with native.LaunchProfiler() as prof:
        got = fused_conv1d_stack(xd, desc, dev)
        (got * gyd).sum().backward()
    seen = prof.summary()
    assert seen['asac_conv1_forward']['calls'] == 1 and seen['asac_conv1_backward']['calls'] == 1
    assert got.shape == (N, o2 * l2)
    outs = [got.detach().double().cpu()] + [p.grad.double().cpu() for p in dev.parameters()]
    reduction = {'y': C * k1 + o1 * k2, 'w1': N * l1, 'b1': N * l1, 'w2': N * l2, 'b2': N * l2}
    figures, failed = {}, []
    for name, a, w, em in zip(NAMES, outs, want, e_mod):
        assert a.shape == w.shape and torch.isfinite(a).all(), name
        err, bound = _err(a, w), max(4.0 * em, math.sqrt(reduction[name]) * 2.0 ** -24)
        figures[name] = (err, em, bound)
        if not err <= bound:
            failed.append(name)
    print('conv1d', case, 'min|z| %.3g' % min_z, {k: '%.3g / e_mod %.3g / bound %.3g' % v for k, v in figures.items()})
    assert not failed, (failed, figures)
    # inference: nothing saved, same values
    with torch.no_grad():
        again = fused_conv1d_stack(xd, desc, dev)
    assert not again.requires_grad and torch.equal(again, got.detach())
    # deterministic: equal inputs give equal bits
    g1 = [p.grad.clone() for p in dev.parameters()]
    dev.zero_grad()
    (fused_conv1d_stack(xd, desc, dev) * gyd).sum().backward()
    assert all(torch.equal(a, b.grad) for a, b in zip(g1, dev.parameters()))


def test_conv1d_stack_adds_parameter_gradients_in_place_inside_flat_buffers():
    """With the four parameters' `.grad`s consecutive views of one buffer (as inside SAC_Base), the reduction kernel adds into
    them itself: the values of the returned-gradient path, bit for bit (the sum of the slabs is formed first, then added)."""
    import asac_amd  # noqa: F401
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_conv import conv1d_stack_desc, fused_conv1d_stack
    torch.manual_seed(0)
    dev = nn.Sequential(nn.Conv1d(2, 16, 8, 4), nn.LeakyReLU(), nn.Conv1d(16, 32, 4, 2), nn.LeakyReLU()).cuda()
    free = copy.deepcopy(dev)
    group = FlatParamGroup([('conv', list(dev.parameters()))], 'cuda')
    x = torch.randn(203, 61, 2, device='cuda')
    gy = torch.randn(203, 32 * 6, device='cuda')
    desc = conv1d_stack_desc(dev, x)
    (fused_conv1d_stack(x, desc, free) * gy).sum().backward()
    group.grad.zero_()
    (fused_conv1d_stack(x, desc, dev) * gy).sum().backward()
    for pf, pd in zip(free.parameters(), dev.parameters()):
        assert pd.grad.data_ptr() >= group.grad.data_ptr() and torch.equal(pd.grad, pf.grad)
    group.grad.fill_(1.0)
    (fused_conv1d_stack(x, desc, dev) * gy).sum().backward()
    for pf, pd in zip(free.parameters(), dev.parameters()):
        assert torch.equal(pd.grad, 1.0 + pf.grad)


def test_conv1d_layers_route_to_the_fused_stack():
    """`Conv1dLayers(61, 2, 'default', ...)` on device rays uses the fused launch (with leading batch dims) and agrees with
    its own module path; inputs that need gradients and the switch keep the module path."""
    import asac_amd  # noqa: F401
    from asac_amd import native
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import image_layers
    torch.manual_seed(0)
    layer = m.Conv1dLayers(61, 2, 'default', out_dense_n=64, out_dense_depth=2).cuda()
    x = torch.randn(5, 9, 61, 2, device='cuda')
    assert image_layers.FUSED_CONV1D in (True, False)
    before = image_layers.FUSED_CONV1D
    image_layers.FUSED_CONV1D = True
    try:
        with native.LaunchProfiler() as prof:
            got = layer(x)
        assert prof.summary()['asac_conv1_forward']['calls'] == 1 and got.shape == (5, 9, 64)
        conv = lambda t: layer.conv_layers(t.reshape(-1, 61, 2).permute(0, 2, 1)).reshape(5, 9, -1)      # noqa: E731
        want32 = layer.dense(conv(x))
        l64 = copy.deepcopy(layer).double()
        want64 = l64.dense(l64.conv_layers(x.double().reshape(-1, 61, 2).permute(0, 2, 1)).reshape(5, 9, -1))
        e_mod = _err(want32.detach().double(), want64.detach())
        bound = max(4.0 * e_mod, math.sqrt(2 * 8 + 16 * 4 + 192 + 64) * 2.0 ** -24)      # (the two products and the head's)
        err = _err(got.detach().double(), want64.detach())
        print('conv1d layer', err, e_mod, bound)
        assert err <= bound
        xg = x.clone().requires_grad_(True)
        with native.LaunchProfiler() as prof:
            layer(xg).sum().backward()
        assert 'asac_conv1_forward' not in prof.summary() and xg.grad is not None
        image_layers.FUSED_CONV1D = False
        with native.LaunchProfiler() as prof:
            off = layer(x)
        assert 'asac_conv1_forward' not in prof.summary() and torch.equal(off, want32)
    finally:
        image_layers.FUSED_CONV1D = before


def test_unsupported_stack_keeps_the_module_path():
    import asac_amd  # noqa: F401
    from asac_amd import native
    import algorithm.nn_models as m
    from algorithm.fused_conv import conv1d_stack_desc
    torch.manual_seed(0)
    stack = nn.Sequential(nn.Conv1d(1, 8, 3, 1), nn.LeakyReLU(), nn.Conv1d(8, 16, 3, 1), nn.LeakyReLU())
    layer = m.Conv1dLayers(50, 1, (stack, 46, 16), out_dense_n=32, out_dense_depth=1).cuda()
    x = torch.randn(5, 50, 1, device='cuda')
    assert conv1d_stack_desc(layer.conv_layers, x) is None       # C k1 = 3 is not a multiple of 4
    with native.LaunchProfiler() as prof:
        got = layer(x)
    assert 'asac_conv1_forward' not in prof.summary()
    want = layer.dense(layer.conv_layers(x.permute(0, 2, 1)).reshape(5, -1))
    assert got.shape == (5, 32) and torch.equal(got, want)
