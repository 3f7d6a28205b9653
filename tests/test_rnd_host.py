"""CPU: the host side of random network distillation on the native path (`hip_config['fused_rnd']`): the float64
restatement the GPU tests compare the `asac_rnd_*` kernels with (tests/rnd_ref.py) against the recorded reference function
(`tests/golden/f17_rnd_pick.npz`) and against float64 autograd on the module code, the dispatch predicate, the stack
descriptor, the fixtures' margin and sizes, and the entry points' names in the C header and the binding."""

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401
from tests import rnd_ref as rr
from tests.golden.make_rnd_golden import CASES, MIN_GAP, PICK_SHAPES

ENTRY_POINTS = ('asac_rnd_supported', 'asac_rnd_distill_workspace', 'asac_rnd_distill', 'asac_rnd_pick')


def fixture_stacks(g, c):
    pred = rr.stack_params({k[len(f'c{c}/rnd/'):]: g[k] for k in g.files if k.startswith(f'c{c}/rnd/')})
    targ = rr.stack_params({k[len(f'c{c}/target/'):]: g[k] for k in g.files if k.startswith(f'c{c}/target/')})
    return pred, targ


@pytest.mark.parametrize('c', range(len(PICK_SHAPES)))
def test_restatement_reproduces_the_recorded_reference_function(golden_dir, c):
    """tests/rnd_ref.pick in float64 against the reference's float32 `rnd_sample_c_action`: the chosen indices are equal,
    the per-candidate errors and the actions agree to 1e-6 relative (of each tensor's largest entry: float32 rounding of
    the reference's own sums).  The third case has S + A == 64: its first block is residual."""
    g = np.load(golden_dir / 'f17_rnd_pick.npz')
    batch, k, S, A = PICK_SHAPES[c]
    assert tuple(g[f'c{c}/shape']) == (batch, k, S, A) and g[f'c{c}/eps'].shape == (batch, k, A)
    pred, targ = fixture_stacks(g, c)
    assert pred[0].shape == (64, S + A) and rr.residual_flags(S + A) == (S + A == 64, True)
    got = rr.pick(g[f'c{c}/state'], g[f'c{c}/loc'], g[f'c{c}/scale'], g[f'c{c}/eps'], pred, targ)
    assert np.array_equal(got['index'], g[f'c{c}/index'])
    for name in ('err', 'action'):
        want = g[f'c{c}/{name}'].astype(np.float64)
        np.testing.assert_allclose(got[name], want, rtol=0, atol=1e-6 * float(np.abs(want).max()), err_msg=name)
    assert (rr.margin(g[f'c{c}/err']) >= MIN_GAP).all()


def test_pick_fixture_keeps_the_margin(golden_dir):
    path = golden_dir / 'f17_rnd_pick.npz'
    g = np.load(path)
    assert float(g['meta/min_gap']) >= MIN_GAP == 1e-5 and int(g['n_cases']) == len(PICK_SHAPES)
    assert path.stat().st_size <= 1 << 20


@pytest.mark.parametrize('case', list(CASES))
def test_step_fixtures_hold_the_rnd_step(golden_dir, case):
    path = golden_dir / f'f6_step_{case}.npz'
    g = np.load(path)
    assert path.stat().st_size <= 1 << 20 and int(g['n_steps']) == 3
    grads = sorted(k for k in g.files if k.startswith('g0/optimizer_rnd/'))
    assert grads == [f'g0/optimizer_rnd/{j}' for j in (4, 5, 6, 7)], 's_dense has no gradient, c_dense all four'
    for k in g.files:        # s_dense never moves in the reference either
        if k.startswith('w0/model_rnd/s_dense'):
            assert np.array_equal(g[k], g['w1' + k[2:]])


@pytest.mark.parametrize('B,n,S,A', [(3, 2, 6, 2), (4, 3, 61, 3), (2, 2, 20, 5)])
def test_distillation_gradients_against_float64_autograd(B, n, S, A):
    """tests/rnd_ref.distill against `torch.autograd` in float64 on the module code (`ModelRND.cal_c_rnd`, today's
    `_train_rnd` lines): loss, the four parameter gradients (the products `xty_multi` forms from the launch's buffers) and
    the hidden activations; 1e-12 of each tensor's largest entry.  (4, 3, 61, 3): the residual first block."""
    from algorithm.nn_models.exploration import ModelRND
    torch.manual_seed(B + S)
    c = rr.make_distill_case(B, n, S, A, seed=S)
    models = []
    for stack in (c['pred'], c['targ']):
        m = ModelRND(S, 0, A).double()
        sd = m.state_dict()
        for key, v in zip(('dense.0.linear.weight', 'dense.0.linear.bias', 'dense.2.linear.weight', 'dense.2.linear.bias'), stack):
            sd['c_dense.' + key].copy_(v.double())
        models.append(m)
    rnd, target = models
    assert rnd.c_dense.dense[0].residual == (S + A == 64) and rnd.c_dense.dense[2].residual
    states, actions, keep = c['state'].double(), c['action'].double(), ~c['pad'].unsqueeze(-1)
    pred = rnd.cal_c_rnd(states, actions)
    with torch.no_grad():
        t = target.cal_c_rnd(states, actions)
    loss = torch.mean(torch.nn.functional.mse_loss(pred, t, reduction='none') * keep)
    params = [rnd.c_dense.dense[0].linear.weight, rnd.c_dense.dense[0].linear.bias, rnd.c_dense.dense[2].linear.weight,
              rnd.c_dense.dense[2].linear.bias]
    grads = torch.autograd.grad(loss, params)
    got = rr.distill(c['state'].numpy(), c['action'].numpy(), c['pad'].numpy(), tuple(p.double().numpy() for p in c['pred']),
                     tuple(p.double().numpy() for p in c['targ']))
    want = dict(loss=loss.detach().numpy(), dw1=grads[0].numpy(), db1=grads[1].numpy(), dw2=grads[2].numpy(), db2=grads[3].numpy())
    for name, ref in want.items():
        np.testing.assert_allclose(got[name], ref, rtol=0, atol=1e-12 * max(float(np.abs(ref).max()), 1e-30), err_msg=name)
    row = B // 2 * n        # the wholly padded row: no cotangent
    assert not got['gz1'][row:row + n].any() and not got['gz2'][row:row + n].any() and got['gz2'].any()


# ------------------------------------------------------------------------------------------------
PLAIN = dict(enabled=True, plain_learner=True, d_action_sizes=[], c_action_size=2, data_parallel=False, float32_on_device=True,
             stack_ok=True, state_size=6, n_sample=10, rows=16 * 3)


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(n_sample=1), True), (dict(n_sample=64), True), (dict(state_size=100, c_action_size=28), True),
    (dict(state_size=61, c_action_size=3), True), (dict(rows=1 << 20), True), (dict(c_action_size=64, state_size=64), True),
    (dict(enabled=False), False),                          # hip_config['fused_rnd'] = False
    (dict(plain_learner=False), False),                    # an OptionBase
    (dict(d_action_sizes=[3]), False),                     # hybrid
    (dict(d_action_sizes=[3, 2], c_action_size=0), False),  # pure discrete
    (dict(c_action_size=0), False),
    (dict(data_parallel=True), False), (dict(float32_on_device=False), False),
    (dict(stack_ok=False), False),                         # a plugin's other stack, or misaligned / scattered parameters
    (dict(n_sample=65), False), (dict(n_sample=0), False), (dict(state_size=127), False), (dict(c_action_size=65), False),
    (dict(rows=(1 << 20) + 1), False),
])
def test_dispatch_predicate(change, taken):
    """each excluded condition alone turns the path off"""
    from algorithm.sac_base import fused_rnd_applies
    assert fused_rnd_applies(**{**PLAIN, **change}) is taken


def test_stack_descriptor():
    """the stock stack and the S + A == 64 corner are described; three blocks, a final Linear, width 32, tanh and
    dropout > 0 are refused (`None`: the caller keeps the module code)"""
    from torch import nn

    from algorithm.fused_mlp import describe_rnd_stack, rnd_stack_tensors
    from algorithm.nn_models.exploration import ModelRND
    from algorithm.nn_models.layers.linear_layers import LinearLayers
    d = describe_rnd_stack(ModelRND(6, 0, 2).c_dense, 6, 2)
    assert (d.S, d.A, list(d.residual)) == (6, 2, [0, 1])
    d = describe_rnd_stack(ModelRND(61, 0, 3).c_dense, 61, 3)
    assert (d.S, d.A, list(d.residual)) == (61, 3, [1, 1])
    d = describe_rnd_stack(ModelRND(100, 0, 28).c_dense, 100, 28)
    assert (d.S, d.A, list(d.residual)) == (100, 28, [0, 1])
    assert describe_rnd_stack(LinearLayers(8, 64, 2, None, residual=False), 6, 2).residual[1] == 0
    w1, b1, w2, b2 = rnd_stack_tensors(ModelRND(6, 0, 2).c_dense)
    assert w1.shape == (64, 8) and b1.shape == (64,) and w2.shape == (64, 64) and b2.shape == (64,)
    refused = {
        'three blocks': LinearLayers(8, 64, 3, None),
        'one block': LinearLayers(8, 64, 1, None),
        'a final Linear': LinearLayers(8, 64, 2, 16),
        'width 32': LinearLayers(8, 32, 2, None),
        'widths 64, 32': LinearLayers(8, [64, 32], 2, None),
        'tanh': LinearLayers(8, 64, 2, None, activation=nn.Tanh),
        'dropout': LinearLayers(8, 64, 2, None, dropout=0.1),
        'in 129': LinearLayers(129, 64, 2, None),
    }
    for what, ll in refused.items():
        assert describe_rnd_stack(ll, ll.input_size - 2, 2) is None, what
    assert describe_rnd_stack(LinearLayers(8, 64, 2, None), 7, 2) is None, 'the widths must add up to the input'
    assert describe_rnd_stack(LinearLayers(8, 64, 2, None), 8, 0) is None, 'no action'
    assert describe_rnd_stack(nn.Linear(8, 64), 6, 2) is None

    class Narrow(ModelRND):
        def _build_model(self):
            return super()._build_model(dense_n=32)
    assert describe_rnd_stack(Narrow(6, 0, 2).c_dense, 6, 2) is None


def test_header_and_binding_name_the_entry_points():
    from asac_amd import abi, native
    declared = {name for name in abi.functions if name.startswith('asac_rnd_')}
    bound = {name for name in native.EXPORTED_SYMBOLS if name.startswith('asac_rnd_')}
    assert declared == bound == set(ENTRY_POINTS)
    assert all(callable(getattr(native, name)) for name in ('rnd_distill', 'rnd_pick', 'rnd_sizes_ok'))
    assert abi.defines['ASAC_ABI_VERSION'] == native.ABI_VERSION == 91
    for macro, value in (('ASAC_RND_WIDTH', native.RND_WIDTH), ('ASAC_RND_MAX_IN', native.RND_MAX_IN),
                         ('ASAC_RND_MAX_SAMPLES', native.RND_MAX_SAMPLES)):
        assert abi.defines[macro] == value
    assert native.rnd_sizes_ok(6, 2, 10, 1024) and not native.rnd_sizes_ok(6, 2, 65) and not native.rnd_sizes_ok(125, 4)
