"""CPU: the host side of the pure-discrete, policy-based learner on the native path (`hip_config['fused_discrete']`):
the float64 restatements the GPU tests compare the `asac_discrete_*` kernels with (tests/discrete_ref.py) against the
oracle learner, the dispatch predicate, the stock policy's raw discrete head outputs, the three recorded reference steps
(`tests/golden/f6_step_discrete*.npz`) through the oracle bit for bit, and the four entry points' names in the C header and
the binding."""

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401
from oracle import sac_ref
from tests import discrete_ref as dr
from tests import parity_utils as pu
from tests.golden.make_discrete_golden import CASES, SMALL

ENTRY_POINTS = ('asac_discrete_return', 'asac_discrete_q_loss_grad', 'asac_discrete_policy_loss_grad',
                'asac_discrete_alpha_grad')


# ------------------------------------------------------------------------------------------------
# 8. the float64 restatements are the oracle's functions
# ------------------------------------------------------------------------------------------------
class _TableQ:
    """a critic whose discrete head output is a table (the oracle only calls it)"""

    def __init__(self, table):
        self.table = table

    def __call__(self, state, c_action, obs_list):
        return self.table, None


class _TablePolicy(torch.nn.Module):
    """a policy whose logits are a table: its one parameter receives d loss / d logits"""

    def __init__(self, table, sizes):
        super().__init__()
        self.table, self.sizes = torch.nn.Parameter(table.clone()), sizes

    def forward(self, state, obs_list):
        return dr.joint_policy(self.table, self.sizes), None


def _perm(subset, E):
    """a permutation of 0..E-1 that starts with `subset` (the oracle keeps the first E_sample entries)"""
    head = [int(i) for i in subset]
    return np.array(head + [e for e in range(E) if e not in head], dtype=np.int64)


@pytest.mark.parametrize('B,n,sizes,E,Es,use_is', [(5, 3, (3, 2), 3, 2, True), (4, 2, (4,), 2, 2, False),
                                                   (6, 4, (2, 3, 2), 1, 1, True)])
def test_restatements_equal_the_oracle(B, n, sizes, E, Es, use_is):
    """`discrete_ref` in float64 against `SacRef.get_y` / `train_policy` / `train_alpha` (float32) on table-driven policy
    and critic stubs: same formulas, so they agree to float32 rounding (rtol 2e-5 of each tensor's largest entry)."""
    torch.set_num_threads(1)
    c = dr.make_case(B, n, sizes, E, Es, use_is, weights=True, seed=B + n)
    c64 = dr.to(c, torch.float64, 'cpu')
    want = dr.as_numpy(dr.all_formulas(c64))
    agent = sac_ref.SacRef(['vector'], [(6,)], list(sizes), 0, pu.plugin('nn_vec'), ensemble_q_num=E, ensemble_q_sample=Es,
                           n_step=n, batch_size=B, gamma=c['gamma'], v_lambda=0.95, v_rho=c['v_rho'], v_c=c['v_c'],
                           use_n_step_is=use_is, d_policy_entropy_penalty=c['penalty'], target_d_alpha=0.98,
                           replay_config={'capacity': 64})
    with torch.no_grad():
        agent.log_d_alpha.copy_(c['log_alpha'])
    np.testing.assert_array_equal(agent.target_d_alpha.numpy(), c['target'].numpy())
    np.testing.assert_array_equal(agent.lambda_ratio.numpy(), c['lambda_ratio'].numpy())

    def close(got, name):
        got = np.asarray(got.detach().numpy(), dtype=np.float64).reshape(want[name].shape)
        np.testing.assert_allclose(got, want[name], rtol=2e-5, atol=2e-5 * float(np.abs(want[name]).max()), err_msg=name)

    # get_y: the target critics over the window, subset_next drawn before subset_n (sac_base.py:1391-1392)
    agent.model_policy = _TablePolicy(c['logits'], sizes)
    agent.model_target_q_list = [_TableQ(t) for t in c['q_target']]
    agent.noise = sac_ref.RecordedNoise(perm=[_perm(c['sub_next'], E), _perm(c['sub_n'], E)])
    states = torch.zeros(B, n + 1, 6)
    d_y, c_y = agent.get_y(c['last'], c['pad'], [states], states, c['action'][:, :-1], c['reward'].clone(), c['done'],
                           c['mu'] if use_is else None)
    assert c_y is None and not agent.noise.perm
    close(d_y, 'y')

    # train_policy / train_alpha at the step's state
    agent.model_policy = _TablePolicy(c['logits0'], sizes)
    agent.model_q_list = [_TableQ(t) for t in c['q_online']]
    agent.noise = sac_ref.RecordedNoise(perm=[_perm(c['sub_pi'], E)])
    d_ent, c_ent = agent.train_policy([states[:, 0]], states[:, 0], c['action'][:, 0], c['mu0'])
    assert c_ent is None and not agent.noise.perm
    close(agent.last_loss_policy, 'loss_policy')
    close(d_ent, 'd_entropy')
    close(agent.model_policy.table.grad, 'grad_logits')
    agent.train_alpha([states[:, 0]], states[:, 0])
    close(agent.log_d_alpha.grad, 'grad_alpha')


# ------------------------------------------------------------------------------------------------
# 9. the dispatch predicate
# ------------------------------------------------------------------------------------------------
PLAIN = dict(enabled=True, plain_learner=True, d_action_sizes=[3, 2], c_action_size=0, discrete_dqn_like=False,
             offline_loss=False, siamese=False, use_prediction=False, data_parallel=False, float32_on_device=True,
             ensemble_q_num=2, n_step=3, batch_size=16)


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(d_action_sizes=[64]), True), (dict(d_action_sizes=[1] * 8), True), (dict(ensemble_q_num=8), True),
    (dict(n_step=64), True), (dict(batch_size=1024), True),
    (dict(enabled=False), False),                          # hip_config['fused_discrete'] = False
    (dict(c_action_size=2), False),                        # hybrid
    (dict(discrete_dqn_like=True), False),
    (dict(d_action_sizes=[65]), False),                    # D = 65
    (dict(d_action_sizes=[2] * 9), False),                 # nine branches
    (dict(plain_learner=False), False),                    # an OptionBase
    (dict(d_action_sizes=[]), False), (dict(offline_loss=True), False), (dict(siamese=True), False),
    (dict(use_prediction=True), False), (dict(data_parallel=True), False), (dict(float32_on_device=False), False),
    (dict(ensemble_q_num=9), False), (dict(n_step=65), False), (dict(batch_size=1025), False),
])
def test_dispatch_predicate(change, taken):
    from algorithm.sac_base import fused_discrete_applies
    assert fused_discrete_applies(**{**PLAIN, **change}) is taken


# ------------------------------------------------------------------------------------------------
# 10. the stock policy's raw discrete head outputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes,c_size', [((3, 2), 0), ((4,), 0), ((2, 5, 3), 2)])
def test_d_head_raw_gives_the_logits_of_the_policy(sizes, c_size):
    from algorithm.nn_models import ModelPolicy
    torch.manual_seed(sum(sizes))
    policy = ModelPolicy(7, list(sizes), c_size)
    state = torch.randn(5, 3, 7)
    with torch.no_grad():
        raw = policy.d_head_raw(state)
        d_policy, _ = policy(state, [])
    assert raw.shape == (5, 3, sum(sizes))
    probs = torch.cat([torch.softmax(part, dim=-1) for part in raw.split(list(sizes), dim=-1)], dim=-1)
    np.testing.assert_allclose(probs.numpy(), d_policy.probs.numpy(), rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------
# 11. the three recorded reference steps through the oracle, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(CASES))
def test_discrete_fixtures_are_reproduced_by_the_oracle(golden_dir, case):
    """the loop of tests/test_oracle_golden.py::test_f6_full_step on the pure-discrete fixtures (its `STEP_CASES` table is
    not theirs).  Same eager ops on the same host: identical bits — ids, IS weights, both losses, the entropy, the first
    step's gradients, TD error, tree, ring columns, log_d_alpha, and the weights after the steps."""
    torch.set_num_threads(1)
    g = np.load(golden_dir / f'f6_step_{case}.npz')
    plugin_name, kw, d_sizes = CASES[case]
    agent = sac_ref.SacRef(['vector'], [(6,)], list(d_sizes), 0, pu.plugin(plugin_name), batch_size=SMALL['batch_size'],
                           replay_config={'capacity': SMALL['capacity']}, **kw)
    for name, mod in agent.named_modules().items():
        sd = {k[len(f'w0/{name}/'):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(f'w0/{name}/')}
        if sd or list(mod.state_dict()):
            mod.load_state_dict(sd)
    with torch.no_grad():
        agent.log_c_alpha.copy_(torch.from_numpy(g['w0/log_c_alpha']))
        agent.log_d_alpha.copy_(torch.from_numpy(g['w0/log_d_alpha']))
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    exact, tol = True, dict(rtol=0, atol=0)
    n_steps = int(g['n_steps'])
    assert n_steps == 3
    for s in range(n_steps):
        assert int(g[f'step{s}/n_eps']) == 0 and g[f'step{s}/perm'].shape[0] == 5, 'no normal draws, five permutations'
        agent.noise = sac_ref.RecordedNoise(u=[g[f'step{s}/u']], eps=[], perm=list(g[f'step{s}/perm']))
        out = agent.train()
        assert np.array_equal(out['ids'], g[f'step{s}/sample_ids']), f'step {s}: PER index selection'
        assert np.array_equal(out['is_weights'], g[f'step{s}/is_weights'])
        np.testing.assert_allclose(out['loss_q'].numpy(), g[f'step{s}/loss_q'], **tol)
        np.testing.assert_allclose(out['loss_policy'].numpy(), g[f'step{s}/loss_policy'], **tol)
        np.testing.assert_allclose(out['d_entropy'].numpy(), g[f'step{s}/d_entropy'], **tol)
        if s == 0:
            checked = 0
            for oname, opt in agent.named_optimizers().items():
                for j, p in enumerate(opt.param_groups[0]['params']):
                    if f'g0/{oname}/{j}' in g.files:
                        want = g[f'g0/{oname}/{j}']
                        np.testing.assert_allclose(opt.state[p]['exp_avg'].numpy(), want, rtol=tol['rtol'] * 50,
                                                   atol=0 if exact else 1e-6 * np.abs(want).max() + 1e-12,
                                                   err_msg=f'{oname}/{j}')
                        checked += 1
            assert checked > 0
        np.testing.assert_allclose(out['td_error'], g[f'step{s}/td_error'], **tol)
        if exact:
            assert np.array_equal(agent.replay_buffer.tree.tree.view(np.uint32), g[f'step{s}/tree'].view(np.uint32))
        else:
            np.testing.assert_allclose(agent.replay_buffer.tree.tree, g[f'step{s}/tree'], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(agent.replay_buffer.storage.columns['mu_prob'], g[f'step{s}/mu_prob'], **tol)
        np.testing.assert_allclose(agent.replay_buffer.storage.columns['pre_seq_hidden_state'], g[f'step{s}/hidden'], **tol)
        np.testing.assert_allclose(agent.log_d_alpha.detach().numpy(), g[f'step{s}/log_d_alpha'], **tol)
        assert not agent.noise.eps and not agent.noise.perm, 'every recorded draw must be consumed'
    wtol = dict(rtol=0, atol=0) if exact else dict(rtol=1e-4, atol=1e-6)
    for name, mod in agent.named_modules().items():
        for k, v in mod.state_dict().items():
            assert f'w1/{name}/{k}' in g.files
            np.testing.assert_allclose(v.numpy(), g[f'w1/{name}/{k}'], err_msg=f'{name}/{k}', **wtol)
    for path in (golden_dir / f'f6_step_{case}.npz',):
        assert path.stat().st_size <= 1 << 20


# ------------------------------------------------------------------------------------------------
# 12. header and binding name the same four new entry points
# ------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_four_entry_points():
    from asac_amd import abi, native
    declared = {name for name in abi.functions if name.startswith('asac_discrete_')}
    bound = {name for name in native.EXPORTED_SYMBOLS if name.startswith('asac_discrete_')}
    assert declared == bound == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:       # ... and the Python wrappers of the same names
        assert callable(getattr(native, name[len('asac_'):]))
