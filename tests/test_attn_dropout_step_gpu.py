"""GPU: a learner whose representation is the episodic attention core as the reference's toy environments configure it for
training (`tests/plugins/nn_attn_dropout.py`: 2 heads, dense q / k / v stacks, dropout 0.005, residual gate) — six `train()`
calls: the eager warm-up steps run the attention-weight dropout inside the core's launches, the step is captured, and every
replay draws afresh (each block's call counter advances by the same amount).  No numbers are compared with the module code
here: the draws differ by construction, and tests/test_attn_dropout_gpu.py carries the numbers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402


def test_learner_with_attention_dropout_trains_captured():
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    from tests.plugins import nn_attn_dropout
    assert seq_layers.FUSED_ATTN_DROPOUT

    torch.manual_seed(13)
    learner = SAC_Base(['vector'], [(6,)], [], 2, None, nn_attn_dropout, device='cuda:0', seq_encoder=SEQ_ENCODER.ATTN,
                       batch_size=32, n_step=3, burn_in_step=4, replay_config={'capacity': 1 << 10})
    assert learner.model_rep.training
    blocks = [mod for mod in learner.model_rep.modules() if isinstance(mod, seq_layers.MultiheadAttention)]
    assert len(blocks) == 2 and all(b.dropout == nn_attn_dropout.DROPOUT for b in blocks)
    rng = np.random.default_rng(5)
    for T in (60, 45, 70, 52):
        learner.put_episode(**pu.synthetic_episode(rng, [(6,)], [], 2, learner.seq_hidden_state_shape, T))

    counters = []
    with native.LaunchProfiler(repeat=1) as prof:
        for _ in range(6):
            learner.train()
            torch.cuda.synchronize()
            counters.append([b.dropout_state()[0] for b in blocks])
        seen = prof.summary()
    eager = learner._eager_steps
    print('attention dropout step', {k: v['calls'] for k, v in seen.items() if 'attention' in k}, 'eager steps', eager, counters)
    # the profiler sees the eager warm-up steps only
    assert seen['asac_attention_mh_dropout_forward']['calls'] > 0 and seen['asac_attention_mh_dropout_backward']['calls'] > 0
    assert 'asac_attention_mh_forward' not in seen and 'asac_attention_mh_backward' not in seen
    assert learner._graph is not None and 0 < eager < 6, 'the step was captured after the warm-up'
    # every block's counter advances by the same positive amount on each replay (and on each eager step)
    steps = np.diff(np.array(counters), axis=0)
    assert (steps[eager:] > 0).all() and (steps[eager:] == steps[eager]).all(), steps
    assert all(b.dropout_state()[1] == 0 for b in blocks), 'arrival words end every launch zero'
    assert torch.isfinite(learner._params.flat).all()
    assert torch.isfinite(learner.replay_buffer._tree).all() and torch.isfinite(learner._td_error).all()
    # acting (an attention learner's `choose_action` is `choose_attn_action`): training mode without gradients drops as well
    n_env, T = 4, 7
    before = [b.dropout_state()[0] for b in blocks]
    act = learner.choose_attn_action(
        np.tile(np.arange(T, dtype=np.int32), (n_env, 1)), np.zeros((n_env, T), dtype=bool),
        [rng.standard_normal((n_env, T, 6)).astype(np.float32)], rng.random((n_env, T, 2)).astype(np.float32),
        rng.standard_normal((n_env, T, *learner.seq_hidden_state_shape)).astype(np.float32), disable_sample=True)
    assert all(np.isfinite(a).all() for a in act)
    assert all(b.dropout_state()[0] > c for b, c in zip(blocks, before))
    learner.close()
