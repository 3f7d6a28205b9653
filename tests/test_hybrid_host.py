"""CPU: the host side of the hybrid-action-space learner on the native path (`hip_config['fused_hybrid']`): the float64
restatements the GPU tests compare the `asac_hybrid_*` kernels with (tests/hybrid_ref.py) against the oracle learner, the
dispatch predicate, the switch's default, and the four entry points' names in the C header and the binding."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401
from oracle import sac_ref
from tests import discrete_ref as dr
from tests import hybrid_ref as hr
from tests import parity_utils as pu

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ('asac_hybrid_return', 'asac_hybrid_q_loss_grad', 'asac_hybrid_policy_loss_grad', 'asac_hybrid_alpha_grad')


# ------------------------------------------------------------------------------------------------
# the float64 restatements are the oracle's functions
# ------------------------------------------------------------------------------------------------
class _TableQ(torch.nn.Module):
    """a critic whose two head outputs are tables: over the window for a [B, n+1, S] state, at the step's state for a
    [B, S] one (the oracle only calls it); the step's tables are parameters and receive d loss / d (head outputs)"""

    def __init__(self, d_win, c_win, d0, c0):
        super().__init__()
        self.d_win, self.c_win = d_win, c_win
        self.d0, self.c0 = torch.nn.Parameter(d0.clone()), torch.nn.Parameter(c0.clone())

    def forward(self, state, c_action, obs_list):
        if state.dim() == 3:
            return self.d_win, self.c_win.unsqueeze(-1)
        return self.d0, self.c0.unsqueeze(-1)


class _TablePolicy(torch.nn.Module):
    """a policy whose logits and Normal parameters are tables (window / step's state, as above)"""

    def __init__(self, c, sizes):
        super().__init__()
        self.c, self.sizes = c, sizes
        self.logits0 = torch.nn.Parameter(c['logits0'].clone())

    def forward(self, state, obs_list):
        c = self.c
        if state.dim() == 3:
            return (dr.joint_policy(c['logits'], self.sizes),
                    torch.distributions.Normal(c['loc_w'], c['scale_w'], validate_args=False))
        return dr.joint_policy(self.logits0, self.sizes), torch.distributions.Normal(c['loc0'], c['scale0'], validate_args=False)


def _perm(subset, E):
    """a permutation of 0..E-1 that starts with `subset` (the oracle keeps the first E_sample entries)"""
    head = [int(i) for i in subset]
    return np.array(head + [e for e in range(E) if e not in head], dtype=np.int64)


@pytest.mark.parametrize('B,n,sizes,A,E,Es,use_is', [(5, 3, (3, 2), 2, 3, 2, True), (4, 2, (4,), 1, 2, 2, False),
                                                     (6, 4, (2, 3, 2), 5, 1, 1, True)])
def test_restatements_equal_the_oracle(B, n, sizes, A, E, Es, use_is):
    """`hybrid_ref` in float64 against `SacRef.get_y` / `td_error` / `train_rep_q` / `train_policy` / `train_alpha`
    (float32) on table-driven policy and critic stubs: same formulas, so they agree to float32 rounding (rtol 2e-5 of each
    tensor's largest entry).  The oracle's Q step runs its loss on the stubs' tables: their gradients are d (sum_e l_e) / d
    (head outputs, continuous values)."""
    torch.set_num_threads(1)
    c = hr.make_case(B, n, sizes, A, E, Es, use_is, weights=True, seed=B + n)
    if E > 1:       # (an exact tie's gradient goes to an unspecified member under autograd's min: not the oracle's to pin)
        c['c_q_pi'][1, B - 1] += 0.25
    c = hr.to(c, torch.float32, 'cpu')
    want = dr.as_numpy(hr.all_formulas(hr.to(c, torch.float64, 'cpu')))
    agent = sac_ref.SacRef(['vector'], [(6,)], list(sizes), A, pu.plugin('nn_vec'), ensemble_q_num=E, ensemble_q_sample=Es,
                           n_step=n, batch_size=B, gamma=c['gamma'], v_lambda=0.95, v_rho=c['v_rho'], v_c=c['v_c'],
                           use_n_step_is=use_is, d_policy_entropy_penalty=c['penalty'], target_d_alpha=0.98,
                           target_c_alpha=1.0, clip_epsilon=c['clip_eps'], replay_config={'capacity': 64})
    with torch.no_grad():
        agent.log_d_alpha.copy_(c['log_alpha'])
        agent.log_c_alpha.copy_(c['log_c_alpha'])
    np.testing.assert_array_equal(agent.target_d_alpha.numpy(), c['target'].numpy())

    def close(got, name, index=None):
        ref = want[name] if index is None else want[name][index]
        got = np.asarray(got.detach().numpy(), dtype=np.float64).reshape(ref.shape)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * float(np.abs(want[name]).max()), err_msg=name)

    policy = _TablePolicy(c, sizes)
    critics = [_TableQ(c['q_target'][e], c['cq_target'][e], c['q_online'][e], c['c_q_online'][e]) for e in range(E)]
    targets = [_TableQ(c['q_target'][e], c['cq_target'][e], c['q_online'][e], c['c_t_q'][e]) for e in range(E)]
    agent.model_policy, agent.model_q_list, agent.model_target_q_list = policy, critics, targets
    states = torch.zeros(B, n + 1, 6)
    n_actions = c['action_full'][:, :-1]
    window = (c['last'], c['pad'], [states], states, n_actions)
    draws = lambda: [_perm(c[k], E) for k in ('sub_next', 'sub_n', 'sub_cn', 'sub_cnext')]      # noqa: E731  (today's order)

    # get_y and the TD error: the target critics over the window
    agent.noise = sac_ref.RecordedNoise(eps=[c['eps_w']], perm=draws())
    d_y, c_y = agent.get_y(*window, c['reward'].clone(), c['done'], c['mu_full'] if use_is else None)
    assert not agent.noise.perm and not agent.noise.eps
    close(d_y, 'd_y'), close(c_y, 'c_y')
    agent.noise = sac_ref.RecordedNoise(eps=[c['eps_w']], perm=draws())
    td = agent.td_error(c['last'], c['pad'], [states], states[:, 0], states, n_actions, c['reward'].clone(), c['done'],
                        c['mu_full'] if use_is else None)
    close(td, 'td')

    # the Q step's loss on given targets: get_y is replaced by the case's (d_y, c_y)
    agent.get_y = lambda *a, **k: (c['y'], c['c_y'])
    loss_q0 = agent.train_rep_q(*window, c['reward'].clone(), c['done'], None, c['w'])
    close(loss_q0, 'loss_q', index=0)
    close(torch.stack([q.d0.grad for q in critics]), 'grad_qd')
    close(torch.stack([q.c0.grad for q in critics]), 'grad_cq')

    # train_policy / train_alpha at the step's state: the critics' continuous values on the sample are the table c_q_pi
    for q, row in zip(critics, c['c_q_pi']):
        q.c0 = torch.nn.Parameter(row.clone())
    agent.noise = sac_ref.RecordedNoise(eps=[c['eps0']], perm=[_perm(c['sub_pi'], E), _perm(c['sub_pi_c'], E)])
    d_ent, c_ent = agent.train_policy([states[:, 0]], states[:, 0], c['action_full'][:, 0], c['mu0'])
    assert not agent.noise.perm and not agent.noise.eps
    close(agent.last_loss_policy, 'loss_policy')
    close(d_ent, 'd_entropy'), close(c_ent, 'c_entropy')
    close(policy.logits0.grad, 'grad_logits')
    agent.noise = sac_ref.RecordedNoise(eps=[c['eps0']])
    agent.train_alpha([states[:, 0]], states[:, 0])
    close(torch.stack([agent.log_d_alpha.grad, agent.log_c_alpha.grad]), 'grad_alpha')


# ------------------------------------------------------------------------------------------------
# the dispatch predicate and the switch
# ------------------------------------------------------------------------------------------------
PLAIN = dict(enabled=True, plain_learner=True, d_action_sizes=[3, 2], c_action_size=2, discrete_dqn_like=False,
             offline_loss=False, siamese=False, use_prediction=False, data_parallel=False, float32_on_device=True,
             clip_epsilon=0.2, plain_gaussian=True, ensemble_q_num=2, n_step=3, batch_size=16)


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(d_action_sizes=[64]), True), (dict(d_action_sizes=[1] * 8), True), (dict(ensemble_q_num=8), True),
    (dict(n_step=64), True), (dict(batch_size=1024), True), (dict(c_action_size=64), True),
    (dict(enabled=False), False),                          # hip_config['fused_hybrid'] absent or False
    (dict(c_action_size=0), False),                        # pure discrete: `fused_discrete_applies`' ground
    (dict(d_action_sizes=[]), False),                      # no branches
    (dict(discrete_dqn_like=True), False), (dict(offline_loss=True), False), (dict(siamese=True), False),
    (dict(use_prediction=True), False), (dict(data_parallel=True), False), (dict(float32_on_device=False), False),
    (dict(clip_epsilon=0.), False),                        # the reference's doubling quirk stays eager
    (dict(plain_gaussian=False), False),                   # a continuous head (loc, scale) do not fully describe
    (dict(plain_learner=False), False),                    # an OptionBase
    (dict(d_action_sizes=[65]), False),                    # 65 logits
    (dict(d_action_sizes=[2] * 9), False),                 # nine branches
    (dict(ensemble_q_num=9), False), (dict(n_step=65), False), (dict(batch_size=1025), False),
    (dict(c_action_size=65), False),                       # A over ASAC_MAX_ACTION
])
def test_dispatch_predicate(change, taken):
    from algorithm.sac_base import fused_hybrid_applies
    assert fused_hybrid_applies(**{**PLAIN, **change}) is taken


def test_the_pure_discrete_predicate_stays_false_for_hybrid():
    from algorithm.sac_base import fused_discrete_applies
    kw = {k: v for k, v in PLAIN.items() if k not in ('clip_epsilon', 'plain_gaussian')}
    assert fused_discrete_applies(**kw) is False and fused_discrete_applies(**{**kw, 'c_action_size': 0}) is True


def test_the_switch_defaults_to_off():
    """the constructor reads `hip_config['fused_hybrid']` with default False (and the limit the predicate quotes is the
    header's)"""
    from asac_amd import native
    src = (ROOT / 'advanced-soft-actor-critic_amd' / 'algorithm' / 'sac_base.py').read_text()
    assert re.search(r"self\._fused_hybrid = bool\(hip_config\.get\('fused_hybrid', False\)\)", src)
    from asac_amd import abi
    assert abi.defines['ASAC_MAX_ACTION'] == native.MAX_ACTION


def test_header_and_binding_name_the_four_entry_points():
    from asac_amd import abi, native
    declared = {name for name in abi.functions if name.startswith('asac_hybrid_')}
    bound = {name for name in native.EXPORTED_SYMBOLS if name.startswith('asac_hybrid_')}
    assert declared == bound == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:       # ... and the Python wrappers of the same names
        assert callable(getattr(native, name[len('asac_'):]))
