"""CPU: the host side of the DQN-like discrete learner on the native path (`hip_config['fused_dqn']`): the float64
restatement the GPU tests compare the `asac_dqn_*` kernels with (tests/dqn_ref.py) against the recorded reference function
(`tests/golden/f16_dqn_y.npz`) and this repository's eager `get_dqn_like_d_y`, the dispatch predicate, the argmax margin
of the three recorded steps, and the three entry points' names in the C header and the binding."""

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401
from tests import dqn_ref as qr
from tests.golden.make_dqn_golden import CASES, MIN_GAP, Y_SHAPES

ENTRY_POINTS = ('asac_dqn_return', 'asac_dqn_q_loss_grad', 'asac_dqn_act')


def _fixture_case(g, c):
    k = lambda name: g[f'c{c}/{name}']      # noqa: E731
    sizes = tuple(int(s) for s in k('sizes'))
    n = k('reward').shape[1]
    gamma = float(k('gamma'))
    # the reference multiplies by float32 gamma^t (torch.logspace) and by torch.pow(gamma, L + 1) in float32
    ratio = torch.logspace(0, n - 1, n, gamma).numpy()
    y = qr.target_y(k('eval'), k('target'), k('sub_n'), k('sub_next'), k('reward'), k('done'), k('last'), k('pad'), ratio,
                    gamma, sizes)
    return sizes, y


@pytest.mark.parametrize('c', range(len(Y_SHAPES)))
def test_restatement_reproduces_the_recorded_reference_function(golden_dir, c):
    """float64 restatement against the reference's float32 `get_dqn_like_d_y`: rtol 2e-5 of the largest entry.  The file
    holds the full member tables and the two subsets; row 0 is wholly masked, row 1 has `done` at L, row 2 has L = 0 and
    row 3 an exact tie across its first branch at L, where the lowest index is the one picked."""
    g = np.load(golden_dir / 'f16_dqn_y.npz')
    B, n, shape_sizes, E, Es = Y_SHAPES[c]
    sizes, y = _fixture_case(g, c)
    want = g[f'c{c}/y'].astype(np.float64).reshape(-1)
    assert sizes == tuple(shape_sizes) and g[f'c{c}/eval'].shape == (E, B, n, sum(sizes)) and len(g[f'c{c}/sub_n']) == Es
    np.testing.assert_allclose(y, want, rtol=0, atol=2e-5 * float(np.abs(want).max()))
    # the rows the fixture promises
    L = qr.last_valid(g[f'c{c}/last'], g[f'c{c}/pad'])
    gone = g[f'c{c}/last'] | g[f'c{c}/pad']
    assert gone[0].all() and L[0] == n - 1
    assert g[f'c{c}/done'][1, L[1]] and L[2] == 0 and L[3] == n - 1
    tied = g[f'c{c}/eval'][g[f'c{c}/sub_n'][0], 3, L[3], :sizes[0]]
    assert (tied == tied[0]).all()
    assert qr.greedy(tied, sizes[:1])[0] == 0 == int(torch.argmax(torch.from_numpy(tied)))


@pytest.mark.parametrize('B,n,sizes,E,Es', [(5, 3, (3, 2), 3, 2), (37, 4, (4,), 1, 1), (16, 7, (3, 2, 5), 8, 5)])
def test_restatement_equals_the_eager_function_on_cpu(B, n, sizes, E, Es):
    """tests/dqn_ref.py in float64 against `SAC_Base.get_dqn_like_d_y` plus the loss and TD lines (float32, CPU tensors):
    the same rule, so they agree to float32 rounding (2e-5 of each tensor's largest entry)"""
    from algorithm.sac_base import SAC_Base
    torch.set_num_threads(1)
    c = qr.make_case(B, n, sizes, E, Es, True, seed=B + n)
    want = qr.all_formulas(qr.to(c, torch.float64, 'cpu'))
    stub = qr.eager_stub(c, 'cpu')
    got = qr.as_numpy(qr.eager(c, lambda *a: SAC_Base.get_dqn_like_d_y(stub, *a)))
    assert set(got) == set(want)
    for name, ref in want.items():
        np.testing.assert_allclose(got[name], ref, rtol=0, atol=2e-5 * float(np.abs(ref).max()), err_msg=name)


def test_the_tie_rule_of_the_restatement_is_torch_argmax():
    c = qr.tie_every_branch(qr.make_case(9, 3, (3, 2, 5), 2, 2, False, seed=1), seed=2)
    for q in c['q_eval']:
        j0 = 0
        for k, s in enumerate(c['sizes']):
            part = q[..., j0:j0 + s]
            assert (part == part.max(-1, keepdim=True).values).sum(-1).max() > 1, 'ties occur'
            np.testing.assert_array_equal(qr.greedy(q.numpy(), c['sizes'])[..., k], torch.argmax(part, dim=-1).numpy())
            j0 += s


# ------------------------------------------------------------------------------------------------
PLAIN = dict(enabled=True, plain_learner=True, d_action_sizes=[3, 2], c_action_size=0, discrete_dqn_like=True,
             offline_loss=False, siamese=False, use_prediction=False, curiosity=False, data_parallel=False,
             float32_on_device=True, ensemble_q_num=2, n_step=3, batch_size=16)


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(d_action_sizes=[64]), True), (dict(d_action_sizes=[1] * 8), True), (dict(ensemble_q_num=8), True),
    (dict(n_step=64), True), (dict(batch_size=1024), True),
    (dict(enabled=False), False),                          # hip_config['fused_dqn'] = False
    (dict(plain_learner=False), False),                    # an OptionBase
    (dict(d_action_sizes=[]), False), (dict(c_action_size=2), False), (dict(discrete_dqn_like=False), False),
    (dict(offline_loss=True), False), (dict(siamese=True), False), (dict(use_prediction=True), False),
    (dict(curiosity=True), False), (dict(data_parallel=True), False), (dict(float32_on_device=False), False),
    (dict(d_action_sizes=[65]), False), (dict(d_action_sizes=[2] * 9), False), (dict(ensemble_q_num=9), False),
    (dict(n_step=65), False), (dict(batch_size=1025), False),
])
def test_dispatch_predicate(change, taken):
    """each excluded condition alone turns the path off"""
    from algorithm.sac_base import fused_dqn_applies
    assert fused_dqn_applies(**{**PLAIN, **change}) is taken


@pytest.mark.parametrize('case', list(CASES))
def test_step_fixtures_keep_the_argmax_margin(golden_dir, case):
    path = golden_dir / f'f6_step_{case}.npz'
    g = np.load(path)
    assert float(g['meta/min_gap']) >= MIN_GAP == 1e-5
    assert path.stat().st_size <= 1 << 20
    assert int(g['n_steps']) == 3 and int(g['step0/n_eps']) == 0


def test_header_and_binding_name_the_three_entry_points():
    from asac_amd import abi, native
    declared = {name for name in abi.functions if name.startswith('asac_dqn_')}
    bound = {name for name in native.EXPORTED_SYMBOLS if name.startswith('asac_dqn_')}
    assert declared == bound == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:       # ... and the Python wrappers of the same names
        assert callable(getattr(native, name[len('asac_'):]))
    assert abi.defines['ASAC_ABI_VERSION'] == native.ABI_VERSION
