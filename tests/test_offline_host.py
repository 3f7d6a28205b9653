"""CPU: the host side of the offline loss on the native continuous path (`hip_config['fused_offline']`): the dispatch
predicate, the three entry points' bookkeeping, what the Python wrappers refuse before a launch, and the float64
restatement the GPU tests compare the kernels with (tests/offline_ref.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ('asac_mlp_backward_policy_sample_offline', 'asac_policy_step_fused_offline', 'asac_policy_offline_term')

TAKEN = dict(enabled=True, plain_learner=True, offline_loss=True, c_action_size=2, d_action_sizes=[], stock_networks=True,
             data_parallel=False, float32_on_device=True)


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(c_action_size=8), True),
    (dict(enabled=False), False),                   # hip_config['fused_offline'] = False
    (dict(plain_learner=False), False),             # an OptionBase
    (dict(offline_loss=False), False),              # not `offline_enabled and offline_loss`: nothing to ride along
    (dict(c_action_size=0), False),
    (dict(d_action_sizes=[3, 2]), False),           # a hybrid space
    (dict(stock_networks=False), False),            # a plugin critic or policy
    (dict(data_parallel=True), False),
    (dict(float32_on_device=False), False),
])
def test_dispatch_predicate(change, taken):
    """each clause alone flips the answer"""
    from algorithm.sac_base import fused_offline_applies
    assert fused_offline_applies(**{**TAKEN, **change}) is taken


def test_the_switch_is_on_by_default_and_gates_the_stock_path():
    import inspect
    from algorithm.sac_base import SAC_Base
    assert "hip_config.get('fused_offline', True)" in inspect.getsource(SAC_Base.__init__)
    src = inspect.getsource(SAC_Base._stock_c_only)
    assert 'self._offline_fused()' in src and 'self.offline_enabled and self.offline_loss' in src
    assert 'fused_offline_applies(' in inspect.getsource(SAC_Base._offline_fused)
    # the eager branch keeps its term, clamp included
    assert 'torch.atanh(a_tanh.clamp(-0.999999, 0.999999))' in inspect.getsource(SAC_Base._train_policy)


def test_header_binding_and_notes_name_the_three_entry_points():
    from asac_amd import abi, native
    notes = (ROOT / 'INTEGRATION.md').read_text()
    for name in ENTRY_POINTS:
        assert abi.functions[name][0] == 'int', name
        assert name in native.EXPORTED_SYMBOLS
        assert f'| `{name}` |' in notes
        # the binding's argument count is the header's
        assert len(native._SIGNATURES[name][1]) == len(abi.functions[name][1]), name
    for wrapper in ('mlp_backward_policy_sample', 'mlp_backward_policy_sample_offline', 'policy_step_fused',
                    'policy_step_fused_offline', 'policy_offline_term'):
        assert callable(getattr(native, wrapper))
    assert abi.defines['ASAC_ABI_VERSION'] == native.ABI_VERSION
    # the old entry points keep their signatures: the `_offline` ones are the old ones plus (off_action, off_row_stride)
    for old in ('asac_mlp_backward_policy_sample', 'asac_policy_step_fused'):
        assert len(native._SIGNATURES[old + '_offline'][1]) == len(native._SIGNATURES[old][1]) + 2


def test_the_library_exports_the_three_entry_points():
    from asac_amd import native
    lib = native.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None


def _desc(A):
    from asac_amd import native
    d = native.MlpDesc()
    d.head_cols[0] = d.head_cols[1] = A
    return d


def test_stored_actions_with_a_strided_action_dimension_are_refused_in_the_wrapper():
    """`offline` is an [N, A] view whose ROWS may be strided; a non-unit inner stride, a wrong shape or dtype never reaches
    the library (the checks stand in front of every pointer: host tensors are enough to see them)"""
    from asac_amd import native
    N, A = 16, 2
    wide = torch.zeros(N, 2 * A)
    q_desc, pi_desc = _desc(1), _desc(A)
    args = (q_desc, None, 0, pi_desc, None, 0, torch.zeros(N, 6), N, None, torch.zeros(N, A), None, None, None, None, 0)
    with pytest.raises(AssertionError, match='action dimension must be contiguous'):
        native.policy_step_fused(*args, offline=wide[:, ::2])
    with pytest.raises(AssertionError, match='stored actions'):
        native.policy_step_fused(*args, offline=torch.zeros(N, A + 1))
    with pytest.raises(AssertionError, match='stored actions'):
        native.policy_step_fused(*args, offline=torch.zeros(N, A, dtype=torch.float64))
    with pytest.raises(AssertionError, match='action dimension must be contiguous'):
        native.policy_offline_term(torch.zeros(N, 2 * A), torch.zeros(N, A), wide[:, ::2], torch.zeros(()))
    # a window view [N, 3, A][:, 1] passes the shape and stride checks (and stops at the device check that follows them)
    win = torch.zeros(N, 3, A)
    with pytest.raises(AssertionError, match='device memory'):
        native.policy_step_fused(*args, offline=win[:, 1])


def test_the_restatement_is_the_references_expression():
    """tests/offline_ref.py against plain float64 autograd of the reference's lines written out with
    `torch.distributions` (sac_base.py:1883-1903), and: the offline term moves the gradient"""
    import algorithm.nn_models as m
    from tests import offline_ref as ref
    torch.manual_seed(0)
    N, S, A = 9, 6, 2
    pi = m.ModelPolicy(S, [], A).double()
    qs = [m.ModelQ(S, [], A, False).double() for _ in range(3)]
    state, eps = torch.randn(N, S).double(), 3. * torch.randn(N, A).double()
    stored = torch.rand(N, A).double()
    log_alpha = torch.tensor(-0.7).double()
    _, c = pi(state, [None])
    u = c.rsample() * 0 + c.loc + eps * c.scale
    lp = c.log_prob(u) - torch.sum(torch.log(torch.maximum(1 - torch.tanh(u) ** 2, torch.tensor(1e-2, dtype=torch.float64))), -1, keepdim=True)
    logp = torch.where(lp == torch.inf, torch.zeros_like(lp), lp).sum(-1, keepdim=True)
    q = torch.stack([qs[e](state, torch.tanh(u), [None])[1] for e in (2, 0)])
    loss = log_alpha.exp() * logp - q.min(0)[0]
    loss = loss + torch.nn.functional.mse_loss(u, stored, reduction='none').sum(-1, keepdim=True)
    want = torch.autograd.grad(loss.mean(), list(pi.parameters()))
    obj, got = ref.policy_objective(pi, qs, state, eps, stored, log_alpha, subset=(2, 0))
    assert abs(float(obj) - float(loss.mean().detach())) <= 1e-12 * abs(float(obj))
    for a, b in zip(got, want):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-10, atol=1e-14)
    _, plain = ref.policy_objective(pi, qs, state, eps, stored, log_alpha, subset=(2, 0), offline=False)
    assert max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(got, plain)) > 0.1
    term, g_u = ref.offline_grad_u(c.loc, c.scale, eps, stored)
    np.testing.assert_allclose(g_u.numpy(), (2 * (u - stored) / N).detach().numpy(), rtol=1e-12)
    assert float(term) > 0
