"""CPU: the host side of random network distillation for a pure-discrete, policy-based learner on the native path
(`hip_config['fused_rnd_discrete']`): the float64 restatement the GPU tests compare the `asac_drnd_*` kernels with
(tests/drnd_ref.py) against float64 autograd on the module code and against the recorded reference function
(`tests/golden/f18_drnd_pick.npz`), the candidate rule, the dispatch predicate, the member descriptor, the fixtures' margins
and sizes, the share of rows the GPU test's seeds leave with a clear margin, and the entry points' names."""
from pathlib import Path

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401
from tests import drnd_ref as dr
from tests import rnd_ref as rr
from tests.golden.make_drnd_golden import CASES, MIN_GAP, MIN_WIDTH, PICK_SHAPES, Fixture

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ('asac_drnd_supported', 'asac_drnd_distill_workspace', 'asac_drnd_distill', 'asac_drnd_param_grads_workspace',
                'asac_drnd_param_grads', 'asac_drnd_pick')
KEYS = ('dense.0.linear.weight', 'dense.0.linear.bias', 'dense.2.linear.weight', 'dense.2.linear.bias')


def fixture_members(g, c, D):
    sd = lambda name: {k.split('/', 2)[2]: g[k] for k in g.files if k.startswith(f'c{c}/{name}/')}      # noqa: E731
    return tuple([rr.stack_params(sd(name), f'd_dense_list.{m}.') for m in range(D)] for name in ('rnd', 'target'))


def _module(members, S, D):
    """a float64 `ModelRND` whose `d_dense_list` holds `members`"""
    from algorithm.nn_models.exploration import ModelRND
    m = ModelRND(S, D, 0).double()
    sd = m.state_dict()
    for i, stack in enumerate(members):
        for key, v in zip(KEYS, stack):
            sd[f'd_dense_list.{i}.{key}'].copy_(v.double())
    return m


@pytest.mark.parametrize('B,n,S,sizes', [(3, 2, 6, (3,)), (4, 3, 64, (2, 3)), (2, 2, 20, (3, 2, 2))])
def test_distillation_gradients_against_float64_autograd(B, n, S, sizes):
    """tests/drnd_ref.distill against `torch.autograd` in float64 on the module code (`ModelRND.cal_d_rnd`, today's
    `_train_rnd` lines): loss and all 4 D parameter gradients, 1e-12 of each tensor's largest entry; a member nobody selected
    has exact zeros, the wholly padded entry no record.  (4, 3, 64, (2, 3)): the residual first block."""
    torch.manual_seed(B + S)
    D = sum(sizes)
    c = dr.make_distill_case(B, n, S, sizes, seed=S)
    rnd, target = _module(c['pred'], S, D), _module(c['targ'], S, D)
    assert rnd.d_dense_list[0].dense[0].residual == (S == 64) and rnd.d_dense_list[0].dense[2].residual
    states, sel, keep = c['state'].double(), c['action'].double().unsqueeze(-1), ~c['pad'].unsqueeze(-1)
    d = (sel * rnd.cal_d_rnd(states)).sum(-2)
    with torch.no_grad():
        t = (sel * target.cal_d_rnd(states)).sum(-2)
    loss = torch.mean(torch.nn.functional.mse_loss(d, t, reduction='none') * keep)
    params = [p for m in rnd.d_dense_list for p in (m.dense[0].linear.weight, m.dense[0].linear.bias, m.dense[2].linear.weight,
                                                    m.dense[2].linear.bias)]
    grads = torch.autograd.grad(loss, params)
    got = dr.distill(c['state'].numpy(), c['action'].numpy(), c['pad'].numpy(), sizes, dr.as64(c['pred']), dr.as64(c['targ']))
    np.testing.assert_allclose(got['loss'], loss.detach().numpy(), rtol=1e-12)
    for i, name in enumerate(('dw1', 'db1', 'dw2', 'db2')):
        ref = np.stack([grads[4 * m + i].numpy() for m in range(D)])
        np.testing.assert_allclose(got[name], ref, rtol=0, atol=1e-12 * max(float(np.abs(ref).max()), 1e-30), err_msg=name)
        assert not got[name][D - 1].any() and got[name].any(), name
    rows = slice(B // 2 * n, B // 2 * n + n)
    assert (got['sel'][rows] == -1).all() and not got['gz1'][rows].any() and got['gz2'].any()


def test_candidate_rule():
    """#{i < s - 1 : c_i <= u}: the index whose CDF interval [c_(i-1), c_i) holds u; u = 0 gives 0, u just under 1 the last
    index, an edge itself belongs to the interval above it"""
    p = np.array([0.25, 0.5, 0.25], dtype=np.float32)
    assert [dr.inverse_cdf(p, u) for u in (0., 0.2499, 0.25, 0.5, 0.7499, 0.75, 0.999999)] == [0, 0, 1, 1, 1, 2, 2]
    assert dr.inverse_cdf(np.array([1.], dtype=np.float32), 0.3) == 0
    logits = np.array([[0.3, -0.9, 1.1, 0.5, -0.2]])
    u, narrow = dr.midpoint_uniforms(logits, (3, 2), np.array([[[2, 0], [0, 1], [1, 1]]]))
    assert np.array_equal(dr.candidate_indices(logits, (3, 2), u)[0], [[2, 0], [0, 1], [1, 1]]) and narrow > 0.05
    assert np.array_equal(dr.one_hot(np.array([[2, 0]]), (3, 2)), [[0, 0, 1, 1, 0]])
    assert dr.select(np.array([0., 0., 1., 0., 0.]), (3, 2)) == [(2, 1.), (-1, 0.)]
    assert dr.select(np.array([0., .5, 1., 0., 2.]), (3, 2)) == [(1, .5), (4, 2.)]


@pytest.mark.parametrize('c', range(len(PICK_SHAPES)))
def test_restatement_reproduces_the_recorded_reference_function(golden_dir, c):
    """tests/drnd_ref.pick in float64 against the reference's float32 `rnd_sample_d_action`: the uniforms rebuilt from the
    recorded candidates give the recorded candidates back, the chosen indices and actions are equal, the per-candidate errors
    agree to 1e-6 of the largest; every row keeps the margin and every CDF interval its width"""
    g = np.load(golden_dir / 'f18_drnd_pick.npz')
    batch, k, S, sizes = PICK_SHAPES[c]
    assert tuple(g[f'c{c}/shape']) == (batch, k, S) and tuple(g[f'c{c}/sizes']) == sizes
    pred, targ = fixture_members(g, c, sum(sizes))
    assert pred[0][0].shape == (64, S) and len(pred) == len(targ) == sum(sizes)
    u, narrow = dr.midpoint_uniforms(g[f'c{c}/logits'], sizes, g[f'c{c}/cand'])
    assert narrow > MIN_WIDTH
    got = dr.pick(g[f'c{c}/state'], g[f'c{c}/logits'], u, sizes, pred, targ)
    assert np.array_equal(got['cand'], g[f'c{c}/cand'])
    assert np.array_equal(got['index'], g[f'c{c}/index']) and np.array_equal(got['action'], g[f'c{c}/action'])
    want = g[f'c{c}/err'].astype(np.float64)
    np.testing.assert_allclose(got['err'], want, rtol=0, atol=1e-6 * float(np.abs(want).max()))
    assert (dr.margin(g[f'c{c}/err'], g[f'c{c}/cand']) >= MIN_GAP).all()
    p = dr.branch_probs(g[f'c{c}/logits'], sizes)
    np.testing.assert_allclose(p, torch.cat([torch.softmax(t, -1) for t in torch.from_numpy(g[f'c{c}/logits']).double().split(list(sizes), -1)], -1).numpy(), rtol=1e-14)


def test_pick_fixture_keeps_the_margins(golden_dir):
    path = golden_dir / 'f18_drnd_pick.npz'
    g = np.load(path)
    assert float(g['meta/min_gap']) >= MIN_GAP == 1e-5 and float(g['meta/min_width']) > MIN_WIDTH == 1e-3
    assert int(g['n_cases']) == len(PICK_SHAPES) and path.stat().st_size < 1_000_000


@pytest.mark.parametrize('case', list(CASES))
def test_step_fixtures_hold_the_rnd_step(golden_dir, case):
    path = golden_dir / f'f6_step_{case}.npz'
    g = Fixture(path)
    D = sum(CASES[case][1])
    assert path.stat().st_size < 1_000_000 and int(g['n_steps']) == 3
    grads = sorted((k for k in g.files if k.startswith('g0/optimizer_rnd/')), key=lambda k: int(k.rsplit('/', 1)[1]))
    assert grads == [f'g0/optimizer_rnd/{j}' for j in range(4, 4 + 4 * D)], 's_dense has no gradient, every member all four'
    for k in g.files:        # s_dense never moves in the reference either, nor does the target
        if k.startswith('w0/model_rnd/s_dense') or k.startswith('w0/model_target_rnd/'):
            assert np.array_equal(g[k], g['w1' + k[2:]]), k
    assert any(not np.array_equal(g[k], g['w1' + k[2:]]) for k in g.files if k.startswith('w0/model_rnd/d_dense_list.'))


def test_the_gpu_tests_seeds_leave_most_rows_a_clear_margin():
    """for the cases tests/test_drnd_gpu.py::test_pick_against_float64 runs, the share of rows whose float64 margin over
    candidates with another action is at least MIN_GAP is above 0.9 — by the reference alone, whatever the device computes"""
    from tests.test_drnd_gpu import PICK_CASES, _pick_case
    for case in PICK_CASES:
        _, ref = _pick_case(*case)
        share = float((dr.margin(ref['err'], ref['cand']) >= MIN_GAP).mean())
        print(case, 'rows with a clear margin', share)
        assert share > 0.9, case


# ------------------------------------------------------------------------------------------------
PLAIN = dict(enabled=True, plain_learner=True, d_action_sizes=[3], c_action_size=0, discrete_dqn_like=False, data_parallel=False,
             float32_on_device=True, stack_ok=True, state_size=6, n_sample=10, rows=16 * 3)


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(n_sample=1), True), (dict(n_sample=64), True), (dict(state_size=128), True), (dict(d_action_sizes=[3, 2]), True),
    (dict(d_action_sizes=[5, 4, 3, 2, 2]), True), (dict(d_action_sizes=[2] * 8), True), (dict(rows=1 << 20), True),
    (dict(enabled=False), False),                          # hip_config['fused_rnd_discrete'] = False
    (dict(plain_learner=False), False),                    # an OptionBase
    (dict(c_action_size=2), False),                        # hybrid
    (dict(d_action_sizes=[]), False), (dict(d_action_sizes=[], c_action_size=2), False),      # continuous: `fused_rnd`'s
    (dict(discrete_dqn_like=True), False),                 # the s_dense + sigmoid form
    (dict(data_parallel=True), False), (dict(float32_on_device=False), False),
    (dict(stack_ok=False), False),                         # a plugin's other stack, or misaligned / scattered parameters
    (dict(d_action_sizes=[9, 8]), False),                  # D = 17
    (dict(d_action_sizes=[1] * 9), False),                 # K = 9
    (dict(n_sample=65), False), (dict(n_sample=0), False), (dict(state_size=129), False),
    (dict(rows=(1 << 20) + 1), False),
])
def test_dispatch_predicate(change, taken):
    """each excluded condition alone turns the path off"""
    from algorithm.sac_base import fused_rnd_discrete_applies
    assert fused_rnd_discrete_applies(**{**PLAIN, **change}) is taken


def test_member_descriptor():
    """`describe_drnd_member`: `describe_rnd_stack`'s rules at action width 0; `describe_rnd_stack` itself still refuses it"""
    from torch import nn

    from algorithm.fused_mlp import describe_drnd_member, describe_rnd_stack
    from algorithm.nn_models.exploration import ModelRND
    from algorithm.nn_models.layers.linear_layers import LinearLayers
    assert describe_drnd_member(ModelRND(6, 3, 0).d_dense_list[2], 6) == (False, True)
    assert describe_drnd_member(ModelRND(64, 3, 0).d_dense_list[0], 64) == (True, True)
    assert describe_drnd_member(ModelRND(128, 3, 0).d_dense_list[0], 128) == (False, True)
    assert describe_drnd_member(LinearLayers(8, 64, 2, None, residual=False), 8) == (False, False)
    refused = {
        'three blocks': LinearLayers(8, 64, 3, None), 'one block': LinearLayers(8, 64, 1, None),
        'a final Linear': LinearLayers(8, 64, 2, 16), 'width 32': LinearLayers(8, 32, 2, None),
        'tanh': LinearLayers(8, 64, 2, None, activation=nn.Tanh), 'dropout': LinearLayers(8, 64, 2, None, dropout=0.1),
        'in 129': LinearLayers(129, 64, 2, None),
    }
    for what, ll in refused.items():
        assert describe_drnd_member(ll, ll.input_size) is None, what
    assert describe_drnd_member(LinearLayers(8, 64, 2, None), 7) is None and describe_drnd_member(nn.Linear(8, 64), 8) is None
    assert describe_rnd_stack(LinearLayers(8, 64, 2, None), 8, 0) is None, 'today\'s callers: unchanged'


def test_header_and_binding_name_the_entry_points():
    from asac_amd import abi, native
    declared = {name for name in abi.functions if name.startswith('asac_drnd_')}
    bound = {name for name in native.EXPORTED_SYMBOLS if name.startswith('asac_drnd_')}
    assert declared == bound == set(ENTRY_POINTS)
    assert all(callable(getattr(native, name)) for name in ('drnd_distill', 'drnd_param_grads', 'drnd_pick', 'drnd_sizes_ok',
                                                            'drnd_table'))
    assert abi.defines['ASAC_DRND_MAX_MEMBERS'] == native.DRND_MAX_MEMBERS == 16
    assert native.drnd_sizes_ok(6, (3,), 10, 1024) and not native.drnd_sizes_ok(6, (3,), 65) and not native.drnd_sizes_ok(6, (9, 8))
    build = (ROOT / 'advanced-soft-actor-critic_amd' / 'csrc' / 'build.py').read_text()
    assert "'drnd.hip'" in build
