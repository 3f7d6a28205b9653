"""CPU: the host side of the option-critic's per-option learner (`algorithm/oc/option_base.py`): the package imports
without a GPU, the public surface is the reference's, unsupported options are rejected by name before a device is touched,
a CPU device is refused, and the checkpoint keys are the reference's."""
import inspect

import pytest
import torch

import asac_amd  # noqa: F401

# `OptionBase` of the reference (algorithm/oc/option_base.py), public and driven-by-the-selector methods -> parameters
REFERENCE_SIGNATURES = {
    '__init__': ['self', 'option', 'display_name', 'fix_policy', 'random_q', 'args', 'kwargs'],
    'choose_action': ['self', 'obs_list', 'pre_action', 'pre_seq_hidden_state', 'offline_action', 'disable_sample',
                      'force_rnd_if_available'],
    'get_l_states': ['self', 'l_indexes', 'l_padding_masks', 'l_obses_list', 'l_pre_actions', 'l_pre_seq_hidden_states',
                     'is_target'],
    'get_dqn_like_d_y': ['self', 'n_terminations', 'next_n_vs', 'n_last_masks', 'n_padding_masks', 'n_rewards', 'n_dones',
                         'stacked_next_n_d_qs', 'stacked_next_target_n_d_qs'],
    'compute_rep_q_grads': ['self', 'next_n_vs_over_options', 'n_indexes', 'n_last_masks', 'n_padding_masks',
                            'nx_obses_list', 'nx_target_obses_list', 'nx_states', 'nx_target_states', 'n_actions',
                            'n_pre_actions', 'n_rewards', 'n_dones', 'n_mu_probs', 'n_pre_seq_hidden_states',
                            'priority_is'],
    'train_rep_q': ['self'],
    'train_policy_alpha': ['self', 'n_padding_masks', 'n_obses_list', 'nx_states', 'n_actions', 'n_mu_probs'],
    'compute_termination_grads': ['self', 'terminal_entropy', 'obs_list', 'state', 'y', 'v_over_options', 'done',
                                  'priority_is'],
    'train_termination': ['self'],
    '_get_td_error': ['self', 'next_n_vs_over_options', 'n_last_masks', 'n_padding_masks', 'nx_obses_list',
                      'nx_target_obses_list', 'state', 'nx_target_states', 'n_actions', 'n_rewards', 'n_dones',
                      'n_mu_probs'],
    'remove_models': ['self', 'gt'],
    '_update_target_variables': ['self', 'tau'],
}
# the leading parameters of `_get_y` (this class adds keyword-only ones behind them)
REFERENCE_GET_Y = ['self', 'next_n_vs_over_options', 'n_terminations', 'n_last_masks', 'n_padding_masks', 'nx_obses_list',
                   'nx_states', 'n_actions', 'n_rewards', 'n_dones', 'n_mu_probs']
# ckpt_dict of the reference class for a continuous option with a parameter-free representation and two critics
# (sac_base.py:493-566 + option_base.py:55-59)
REFERENCE_CKPT_KEYS = ['global_step', 'model_q_0', 'model_target_q_0', 'optimizer_q_0', 'model_q_1', 'model_target_q_1',
                       'optimizer_q_1', 'model_policy', 'optimizer_policy', 'log_d_alpha', 'log_c_alpha', 'optimizer_alpha',
                       'model_termination', 'model_target_termination']


def _kw(**extra):
    from tests.plugins import nn_oc
    kw = dict(obs_names=['vector'], obs_shapes=[(6,)], d_action_sizes=[], c_action_size=2, model_abs_dir=None, nn=nn_oc,
              device='cpu', batch_size=8)
    kw.update(extra)
    return kw


def test_package_imports_and_surface():
    from algorithm.oc import OptionBase
    from algorithm.oc.option_base import OptionBase as Direct
    from algorithm.sac_base import SAC_Base
    assert OptionBase is Direct and issubclass(OptionBase, SAC_Base)
    for name, params in REFERENCE_SIGNATURES.items():
        assert list(inspect.signature(getattr(OptionBase, name)).parameters) == params, name
    got = inspect.signature(OptionBase._get_y).parameters
    assert list(got)[:len(REFERENCE_GET_Y)] == REFERENCE_GET_Y
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(got.values())[len(REFERENCE_GET_Y):])


def test_cpu_device_is_refused():
    from algorithm.oc import OptionBase
    from asac_amd import native
    with pytest.raises(native.AsacNativeError, match='no CPU fallback'):
        OptionBase(0, 'option_0', False, False, **_kw())


@pytest.mark.parametrize('extra,word', [
    (dict(siamese='ATC'), 'siamese'),
    (dict(use_prediction=True), 'use_prediction'),
    (dict(hip_config={'dist': object()}), 'dist'),
    (dict(seq_encoder='ATTN'), 'ATTN'),
])
def test_unsupported_options_are_rejected_by_name(extra, word):
    from algorithm.oc import OptionBase
    from algorithm.utils.enums import convert_config_to_enum
    extra = dict(extra)
    convert_config_to_enum(extra)
    with pytest.raises(ValueError, match=word):          # (before the device check: a ValueError, not AsacNativeError)
        OptionBase(0, 'option_0', False, False, **_kw(**extra))


def test_unsupported_options_given_positionally():
    """the selector's call sites pass the parent's arguments through `*args`: the rejection reads them there as well"""
    from algorithm.oc import OptionBase
    from tests.plugins import nn_oc
    with pytest.raises(ValueError, match='use_prediction'):
        OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [], 2, None, nn_oc, device='cpu', use_prediction=True)


def test_train_is_not_an_entry_point():
    from algorithm.oc import OptionBase
    opt = OptionBase.__new__(OptionBase)
    with pytest.raises(RuntimeError, match='not an entry point'):
        opt.train()
    with pytest.raises(RuntimeError, match='replay buffer'):
        opt.put_episode()


def test_random_q_environment_switch(monkeypatch):
    from algorithm.oc import option_base
    seen = {}
    monkeypatch.setattr(option_base.SAC_Base, '__init__', lambda self, *a, **k: seen.update(random_q=self.random_q))
    option_base.OptionBase(0, 'o', False, True)
    assert seen['random_q'] is True
    monkeypatch.setenv('DISABLE_RANDOM_Q', '1')
    option_base.OptionBase(0, 'o', False, True)
    assert seen['random_q'] is False


def test_checkpoint_keys_are_the_reference_s():
    """`_build_ckpt` on a stand-in learner (no device): the parent's keys, then the two termination modules"""
    from algorithm.oc import OptionBase
    from algorithm.utils.enums import CURIOSITY  # noqa: F401
    import logging
    lin = lambda: torch.nn.Linear(2, 1)  # noqa: E731
    opt = OptionBase.__new__(OptionBase)
    opt.global_step = torch.tensor(0)
    opt.optimizer_rep = None
    opt.ensemble_q_num = 2
    opt.model_q_list, opt.model_target_q_list, opt.optimizer_q_list = [lin(), lin()], [lin(), lin()], [object(), object()]
    opt.model_policy, opt.optimizer_policy = lin(), object()
    opt.log_d_alpha, opt.log_c_alpha = torch.zeros(1), torch.zeros(1)
    opt.use_auto_alpha, opt.optimizer_alpha = True, object()
    opt.curiosity = opt.siamese = None
    opt.use_prediction = opt.use_rnd = opt.use_normalization = False
    opt.model_termination, opt.model_target_termination = lin(), lin()
    opt._logger = logging.getLogger('option')
    opt._build_ckpt()
    assert list(opt.ckpt_dict) == REFERENCE_CKPT_KEYS
