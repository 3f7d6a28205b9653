"""GPU: a learner whose representation is the ray-sensor encoder (`tests/plugins/nn_ray.py`: `Conv1dLayers(61, 2, 'default')`
of the rays beside a vector) with the convolution stack as one launch per pass (`asac_conv1_*`) against the same learner
running that stack as PyTorch modules (MIOpen / ATen): same seed, same episodes, same noise, six `train()` calls — eager
steps, the capture and hipGraph replays."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402

OBS_SHAPES = [(61, 2), (6,)]


def test_fused_ray_encoder_matches_module_path(monkeypatch):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm import fused_conv
    from algorithm.nn_models.layers import image_layers
    from algorithm.sac_base import SAC_Base
    from tests.plugins import nn_ray

    def agent():
        torch.manual_seed(13)
        return SAC_Base(['ray', 'vector'], OBS_SHAPES, [], 3, None, nn_ray, device='cuda:0', batch_size=32, n_step=3,
                        replay_config={'capacity': 1 << 10})

    monkeypatch.setattr(image_layers, 'FUSED_CONV1D', True)
    fused = agent()
    plain = agent()
    assert torch.equal(plain._params.flat, fused._params.flat)
    rng = np.random.default_rng(5)
    episodes = [pu.synthetic_episode(rng, OBS_SHAPES, [], 3, (0,), T) for T in (40, 31, 52, 45)]
    obs = [rng.standard_normal((4, *s)).astype(np.float32) for s in OBS_SHAPES]
    pre_a = np.zeros((4, 3), np.float32)
    hidden = np.zeros((4, *fused.seq_hidden_state_shape), np.float32)

    def run(learner):
        for ep in episodes:
            learner.put_episode(**ep)
        ids = []
        # (repeat=1: the profiler counts calls here; its timing device, every launch issued `repeat` times, would run each
        # eager step's optimizer launches twenty times, which is not the step whose results are compared below)
        with native.LaunchProfiler(repeat=1) as prof:
            for _ in range(6):
                learner.train()
                ids.append(learner.replay_buffer._ids.clone())
            seen = prof.summary()
        return ids, seen, learner.choose_action(obs, pre_a, hidden, disable_sample=True)

    monkeypatch.setattr(fused_conv, 'conv1d_stack_desc', lambda *a, **k: None)
    plain_ids, plain_seen, plain_act = run(plain)
    assert 'asac_conv1_forward' not in plain_seen and 'asac_conv1_backward' not in plain_seen
    monkeypatch.undo()
    monkeypatch.setattr(image_layers, 'FUSED_CONV1D', True)
    fused_ids, fused_seen, fused_act = run(fused)
    # the profiler sees the eager steps only (the three warm-up steps in front of the capture; nothing is recorded while the
    # step is captured, and a replay issues no launch from Python).  Per eager step, four forward launches: the online and the
    # target pass over the window (both without gradients: a representation without a sequence encoder is differentiated at
    # the one window position the Q loss reads, `_step_rep_and_q`), that one-position pass over the B rays, and the pass
    # under the updated representation; one backward launch, for the one-position pass.
    print('ray step', {k: v['calls'] for k, v in fused_seen.items() if 'conv1' in k}, fused._eager_steps)
    assert fused._eager_steps == 3 and fused._graph is not None, 'the step was captured after the warm-up'
    assert fused_seen['asac_conv1_forward']['calls'] == 3 * 4 and fused_seen['asac_conv1_backward']['calls'] == 3 * 1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(fused_ids, plain_ids)), 'sampled ids differ'
    np.testing.assert_allclose(fused._params.flat.cpu().numpy(), plain._params.flat.cpu().numpy(), rtol=3e-3, atol=5e-5)
    np.testing.assert_allclose(fused.replay_buffer._tree.cpu().numpy(), plain.replay_buffer._tree.cpu().numpy(),
                               rtol=3e-3, atol=2e-5)
    for g, w in zip(fused_act, plain_act):
        assert g.shape == w.shape and np.isfinite(g).all()
        np.testing.assert_allclose(g, w, rtol=2e-4, atol=2e-5)
    fused.close()
    plain.close()
