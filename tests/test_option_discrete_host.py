"""CPU: the host side of the pure-discrete option on the native path (`hip_config['fused_option_discrete']`): which
configurations `fused_option_discrete_applies` takes, and that the entry point is declared, bound and wrapped."""
from pathlib import Path

import pytest
import torch  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent

TAKEN = dict(enabled=True, d_action_sizes=[3, 2], c_action_size=0, discrete_dqn_like=False, float32_on_device=True,
             ensemble_q_num=2, n_step=5, batch_size=1024, num_options=3)


@pytest.mark.parametrize('change,want', [
    (dict(), True),                                        # the toy configurations' shape
    (dict(d_action_sizes=[64]), True),                     # the limits themselves
    (dict(d_action_sizes=[1] * 8), True),
    (dict(ensemble_q_num=8), True),
    (dict(n_step=64), True),
    (dict(batch_size=1024), True),
    (dict(batch_size=1), True),
    (dict(num_options=1), True),
    (dict(num_options=1024), True),
    (dict(enabled=False), False),                          # hip_config['fused_option_discrete'] = False
    (dict(c_action_size=2), False),                        # hybrid
    (dict(d_action_sizes=[]), False),                      # continuous only
    (dict(discrete_dqn_like=True), False),
    (dict(d_action_sizes=[65]), False),
    (dict(d_action_sizes=[1] * 9), False),
    (dict(ensemble_q_num=9), False),
    (dict(n_step=65), False),
    (dict(batch_size=1025), False),
    (dict(float32_on_device=False), False),
    (dict(num_options=1025), False),
    (dict(num_options=0), False),
])
def test_which_options_take_the_launch(change, want):
    import asac_amd  # noqa: F401
    from algorithm.oc.option_base import fused_option_discrete_applies
    assert fused_option_discrete_applies(**{**TAKEN, **change}) is want


def test_the_plain_learner_s_switches_stay_off_for_an_option():
    """`fused_discrete_applies(plain_learner=False)` is still False: the option has a launch and a switch of its own"""
    import asac_amd  # noqa: F401
    from algorithm.sac_base import fused_discrete_applies
    kw = dict(enabled=True, d_action_sizes=[3, 2], c_action_size=0, discrete_dqn_like=False, offline_loss=False,
              siamese=False, use_prediction=False, data_parallel=False, float32_on_device=True, ensemble_q_num=2, n_step=5,
              batch_size=1024)
    assert fused_discrete_applies(plain_learner=True, **kw) and not fused_discrete_applies(plain_learner=False, **kw)


def test_header_binding_and_wrapper_name_the_entry_point():
    from asac_amd import abi, native
    assert 'asac_option_discrete_return' in abi.functions, 'asac_option_discrete_return is not declared'
    assert len(abi.functions['asac_option_discrete_return'][1]) == len(native._SIGNATURES['asac_option_discrete_return'][1]) == 11
    assert 'asac_option_discrete_return' in native.EXPORTED_SYMBOLS and callable(native.option_discrete_return)
    assert abi.defines['ASAC_OPTION_MAX_OPTIONS'] == native.OPTION_MAX_OPTIONS
    assert 'asac_option_discrete_return' in (ROOT / 'INTEGRATION.md').read_text()
