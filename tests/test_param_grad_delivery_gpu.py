"""GPU: the four ways a fused backward delivers its PARAMETER gradients give the same floats, per producer of packed
gradients (dense stack, attention projection block, conv2 and conv1d stack, Linear + Tanh head; the modules, shapes and
inputs of tests/test_shared_params_gpu.py, one use each):

  returned   `autograd.grad` hands them back (a scratch block cut into per-parameter views);
  direct     inside `direct_param_grads()` the backward launch ADDS them into the flat `.grad` buffer, zeroed before;
  deferred   inside `DeferredPartialSums()` the walk returns None and `flush()` hands them back;
  both       direct mode inside `DeferredPartialSums()`: nothing is written before `flush()`, which adds them.

Same launch, same per-workgroup partials, same summation order in every mode — the sum is formed by the launch's own
reduction or by the `asac_sum_partials_multi` job that stands for it — and 0 + s == s: `torch.equal`, no tolerance."""
import functools

import pytest
import torch

from tests.test_shared_params_gpu import _Case

pytestmark = pytest.mark.gpu

KINDS = ['dense_sequential', 'attention', 'conv2', 'conv1d', 'linear_tanh']
MODES = ['returned', 'direct', 'deferred', 'both']


@functools.lru_cache(maxsize=None)
def _deliveries(kind):
    """-> ({mode: {parameter name: gradient}}, launches seen per mode); every mode once per kind"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused import FlatParamGroup
    from algorithm.param_grads import DeferredPartialSums, direct_param_grads
    case = _Case(kind, uses=1)
    dev, params, arm, apply = case.device_module()
    group = FlatParamGroup([(kind, params)], 'cuda')
    arm()
    x, cot = case.xs[0].cuda(), case.cots[0].cuda()
    names = [name for name, _ in dev.named_parameters()]

    def from_flat():
        return {name: p.grad.detach().clone() for name, p in dev.named_parameters()}

    got, seen = {}, {}
    with native.LaunchProfiler(repeat=1) as prof:
        grads = torch.autograd.grad(apply(x), params, grad_outputs=cot)
    got['returned'], seen['returned'] = {name: g.clone() for name, g in zip(names, grads)}, prof.summary()

    group.grad.zero_()
    with native.LaunchProfiler(repeat=1) as prof:
        with direct_param_grads():
            torch.autograd.backward([apply(x)], [cot])
    got['direct'], seen['direct'] = from_flat(), prof.summary()

    with native.LaunchProfiler(repeat=1) as prof:
        with DeferredPartialSums() as later:
            grads = torch.autograd.grad(apply(x), params, grad_outputs=cot, allow_unused=True)
        assert all(g is None for g in grads), 'a deferred walk handed autograd a parameter gradient'
        late = later.flush()
    assert list(late) == [0]
    got['deferred'], seen['deferred'] = {name: late[0][id(p)].clone() for name, p in zip(names, params)}, prof.summary()

    group.grad.zero_()
    with native.LaunchProfiler(repeat=1) as prof:
        with direct_param_grads(), DeferredPartialSums() as later:
            torch.autograd.backward([apply(x)], [cot])
        assert not group.grad.any(), 'a deferred backward wrote parameter gradients before the flush'
        assert later.flush() == {}          # (direct mode: nothing is handed back)
    got['both'], seen['both'] = from_flat(), prof.summary()
    return case, got, seen


@pytest.mark.parametrize('kind', KINDS)
def test_the_four_delivery_modes_give_the_same_floats(kind):
    case, got, seen = _deliveries(kind)
    differ = {(a, b): sum(int((got[a][name] != got[b][name]).sum()) for name in got[a])
              for i, a in enumerate(MODES) for b in MODES[i + 1:]}
    print('delivery', kind, 'floats that differ per pair of modes:', differ)
    for name, g in got['returned'].items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, name
    for (a, b), n in differ.items():
        for name in got[a]:
            assert torch.equal(got[a][name], got[b][name]), (a, b, name, f'{n} floats differ between the two modes')


@pytest.mark.parametrize('kind', KINDS)
def test_every_mode_is_one_backward_launch_and_the_deferred_ones_one_sum_launch(kind):
    case, _, seen = _deliveries(kind)
    for mode in MODES:
        assert seen[mode][case.backward]['calls'] == 1, mode
        assert seen[mode].get('asac_sum_partials_multi', {'calls': 0})['calls'] == (mode in ('deferred', 'both')), mode
