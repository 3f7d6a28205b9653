"""CPU: the host side of behaviour cloning (`algorithm/imitation_base.py`): the public surface, the bucket arithmetic and
the loss / gradient formulas `asac_bc_loss_grad` implements, against float64 `torch.distributions.Normal` autograd."""
import inspect
import types

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401

# `ImitationBase.train` of the reference (imitation_base.py:20-24), in order
REFERENCE_TRAIN_PARAMETERS = ['self', 'ep_obses_list', 'ep_actions', 'ep_rewards', 'ep_dones']


def test_public_surface():
    from algorithm.imitation_base import ImitationBase
    assert list(inspect.signature(ImitationBase.train).parameters) == REFERENCE_TRAIN_PARAMETERS
    assert list(inspect.signature(ImitationBase.__init__).parameters) == ['self', 'sac_base']
    for name in ('train_episodes', 'state_dict', 'load_state_dict'):
        assert callable(getattr(ImitationBase, name))


@pytest.mark.parametrize('T,Tp', [(1, 64), (63, 64), (64, 64), (65, 128), (128, 128), (129, 192)])
def test_bucket_length(T, Tp):
    from algorithm.imitation_base import bucket_length
    assert bucket_length(T) == Tp
    assert bucket_length(T, 1) == T       # multiple 1: the unpadded path


def test_bucket_length_refuses_empty_episodes():
    from algorithm.imitation_base import bucket_length
    with pytest.raises(ValueError):
        bucket_length(0)


@pytest.mark.parametrize('T,A,coef', [(1, 1, 0.1), (5, 2, 0.1), (64, 7, 0.1), (33, 3, 0.0), (17, 4, 0.5)])
def test_formulas_against_normal_autograd(T, A, coef):
    from algorithm.imitation_base import bc_loss_terms
    g = torch.Generator().manual_seed(T * 100 + A)
    loc = torch.randn(T, A, generator=g, dtype=torch.float64, requires_grad=True)
    scale = (torch.rand(T, A, generator=g, dtype=torch.float64) * 1.5 + 0.05).requires_grad_(True)
    action = torch.rand(T, A, generator=g, dtype=torch.float64) * 2 - 1
    dist = torch.distributions.Normal(loc, scale)
    want = torch.mean(-dist.log_prob(action) - coef * dist.entropy())
    want.backward()
    with torch.no_grad():
        l, dloc, dscale = bc_loss_terms(loc, scale, action, coef)
    n = T * A
    torch.testing.assert_close(l.sum() / n, want.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dloc / n, loc.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(dscale / n, scale.grad, rtol=1e-11, atol=1e-13)


def test_refuses_a_learner_without_continuous_actions():
    from algorithm.imitation_base import ImitationBase
    sac = types.SimpleNamespace(c_action_size=0, d_action_sizes=[3])
    with pytest.raises(ValueError, match='c_action_size'):
        ImitationBase(sac)


def test_refuses_data_parallel_learners():
    from algorithm.imitation_base import ImitationBase
    sac = types.SimpleNamespace(c_action_size=2, d_action_sizes=[], _dist=object())
    with pytest.raises(ValueError, match='dist'):
        ImitationBase(sac)


def test_fixture_losses_are_finite(golden_dir):
    for case in ('mlp', 'rnn', 'attn', 'hybrid'):
        g = np.load(golden_dir / f'f14_imitation_{case}.npz')
        assert g['loss'].shape == (6,) and np.isfinite(g['loss']).all(), case
        assert int(g['m6/step']) == 6 and bool(g['others_unchanged'])
        lens = [g[f'ep{i}/ep_actions'].shape[1] for i in range(int(g['n_episodes']))]
        assert lens == [5, 63, 64, 65, 130, 17]
