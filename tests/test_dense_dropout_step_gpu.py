"""GPU: the learner of tests/test_attn_dropout_step_gpu.py (`tests/plugins/nn_attn_dropout.py`: 2 heads, dense q / k / v
stacks and a dense output block, dropout 0.005, residual gate) with the dense stacks' dropout inside the row launches — six
`train()` calls: the warm-up steps show the new launches, the step is captured, every replay draws afresh at all three sites
of both blocks, and the captured step draws NO torch random numbers any more, so its replays leave torch's replay path
(`CapturedStep.exec_handle`).  No numbers are compared here: tests/test_dense_dropout_gpu.py carries them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402


def _offset():
    """the device generator's Philox offset"""
    return int(torch.cuda.default_generators[0].get_offset())


def test_learner_with_dense_dropout_trains_captured_without_torch_draws():
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    from tests.plugins import nn_attn_dropout
    assert seq_layers.FUSED_ATTN_DROPOUT and seq_layers.FUSED_DENSE_DROPOUT

    torch.manual_seed(13)
    learner = SAC_Base(['vector'], [(6,)], [], 2, None, nn_attn_dropout, device='cuda:0', seq_encoder=SEQ_ENCODER.ATTN,
                       batch_size=32, n_step=3, burn_in_step=4, replay_config={'capacity': 1 << 10})
    assert learner.model_rep.training
    blocks = [mod for mod in learner.model_rep.modules() if isinstance(mod, seq_layers.MultiheadAttention)]
    assert len(blocks) == 2
    rng = np.random.default_rng(5)
    for T in (60, 45, 70, 52):
        learner.put_episode(**pu.synthetic_episode(rng, [(6,)], [], 2, learner.seq_hidden_state_shape, T))

    def counters():
        return [c for b in blocks for c in (b.dense_dropout_state('qkv')[0], b.dropout_state()[0], b.dense_dropout_state('out')[0])]

    seen_counters = []
    with native.LaunchProfiler(repeat=1) as prof:
        for _ in range(6):
            learner.train()
            torch.cuda.synchronize()
            seen_counters.append(counters())
        seen = prof.summary()
    eager = learner._eager_steps
    print('dense dropout step', {k: v['calls'] for k, v in seen.items() if 'dropout' in k}, 'eager steps', eager, seen_counters)
    # the profiler sees the eager warm-up steps only
    for name in ('asac_rows_dense_proj_dropout', 'asac_rows_resblock_dropout', 'asac_attention_mh_dropout'):
        assert seen[name + '_forward']['calls'] > 0 and seen[name + '_backward']['calls'] > 0, name
    assert learner._graph is not None and 0 < eager < 6, 'the step was captured after the warm-up'
    # the 'qkv', 'out' and core counters of both blocks advance by the same positive amount on every replay
    steps = np.diff(np.array(seen_counters), axis=0)
    assert (steps[eager:] > 0).all() and (steps[eager:] == steps[eager][0]).all(), steps
    for b in blocks:
        assert b.dense_dropout_state('qkv')[1] == b.dense_dropout_state('out')[1] == b.dropout_state()[1] == 0, 'arrival words'
    assert torch.isfinite(learner._params.flat).all()
    assert torch.isfinite(learner.replay_buffer._tree).all() and torch.isfinite(learner._td_error).all()
    # the captured step draws no torch random numbers any more: its replays are launched through the exec handle, and the
    # device generator's offset stays where it is
    assert learner._graph.exec_handle is not None
    before = _offset()
    for _ in range(2):
        learner.train()
    torch.cuda.synchronize()
    assert _offset() == before, (before, _offset())
    assert torch.isfinite(learner._params.flat).all()
    learner.close()
