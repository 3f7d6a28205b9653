"""GPU: `hip_config['head_gather_sidecar']` — the synchronous step whose first network launch reads its rows from the
replay ring and carries the step's own window gather as a rider (8 library launches) against the same step with the
stand-alone gather in front of that launch (9): the learners' whole state stays equal, bit for bit, step after step, eager
and as a replayed hipGraph.  Where the one-launch forward chain does not apply the pending gather is issued on its own
before the first reader of the batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.test_full_size_gpu import _episode  # noqa: E402

CFG = dict(bench.CONFIGS['cfg2'], n_step=4, batch_size=64, capacity=4096, episode_len=37)


def _learner(head, **hip):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    cfg = CFG
    torch.manual_seed(0)
    agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], [], cfg['c_action_size'], None, pu.plugin(cfg['plugin']),
                     device='cuda:0', n_step=cfg['n_step'], burn_in_step=0, batch_size=cfg['batch_size'],
                     ensemble_q_num=cfg['ensemble_q_num'], ensemble_q_sample=cfg['ensemble_q_sample'],
                     replay_config={'capacity': cfg['capacity']},
                     hip_config=dict({'use_graph': True, 'graph_warmup': 4, 'head_gather_sidecar': head}, **hip))
    rng = np.random.default_rng(5)
    for _ in range(3000 // cfg['episode_len']):
        agent.put_episode(**_episode(rng, cfg, cfg['episode_len']))
    rb = agent.replay_buffer
    ids = torch.arange(rb.size, device=rb.device, dtype=torch.int64)
    rb.update(ids, torch.from_numpy(np.abs(rng.standard_normal(rb.size)).astype(np.float32)).to(rb.device))
    return agent


def _state(agent):
    rb = agent.replay_buffer
    return dict(params=agent._params.flat, exp_avg=agent._exp_avg, exp_avg_sq=agent._exp_avg_sq,
                target=agent._target_params.flat, tree=rb._tree, mu_prob=rb._columns['mu_prob'], opt_steps=agent._opt_steps,
                ids=rb._ids, w=rb._w, beta=rb._beta)


def _launches(agent):
    from asac_amd import native
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    torch.cuda.synchronize()
    return {k: len(v) for k, v in prof.records.items()}


def _lockstep(on, off, counts):
    """eight steps side by side: 0 .. 3 eager (the launches of step 1 counted), 4 .. 7 replays of the captured step"""
    for step in range(8):
        if step == 1:
            counts.append((_launches(on), _launches(off)))
        else:
            on.train()
            off.train()
        torch.cuda.synchronize()
        assert (on._graph is not None) == (step >= 4) and (off._graph is not None) == (step >= 4)
        assert on._head_gather is None
        a, b = _state(on), _state(off)
        for k in a:
            assert torch.equal(a[k], b[k]), f'step {step}: {k}'
    assert bool(on.replay_buffer._batch['padding_mask'].any())


def test_gather_rides_in_the_first_network_launch_and_the_learner_stays_equal():
    on, off = _learner(True), _learner(False)
    counts = []
    _lockstep(on, off, counts)
    c_on, c_off = counts[0]
    assert 'asac_window_gather_pad' not in c_on and c_off['asac_window_gather_pad'] == 1, (c_on, c_off)
    assert sum(c_on.values()) == 8 and sum(c_off.values()) == 9, (c_on, c_off)
    on.close()
    off.close()


def test_pending_gather_is_issued_on_its_own_where_the_launch_cannot_take_it():
    # (without the one-launch forward chain there is no launch that reads its rows from the ring)
    on, off = _learner(True, fused_forward_chain=False), _learner(False, fused_forward_chain=False)
    counts = []
    _lockstep(on, off, counts)
    c_on, c_off = counts[0]
    # (the sampler had left the IS weights to the rider too: the gather issued on its own forms them, `window_gather_pad_w`)
    assert c_on.get('asac_window_gather_pad_w') == 1 and c_off.get('asac_window_gather_pad') == 1, (c_on, c_off)
    assert sum(c_on.values()) == sum(c_off.values()), (c_on, c_off)
    on.close()
    off.close()


def test_pending_gather_is_issued_on_its_own_where_the_predicate_refuses_the_ring_job(monkeypatch):
    # No constructor argument reaches this branch: what the predicate refuses of a ring description (keys that are no
    # float32 words, joint layouts) is turned away earlier, where the plan is built.  So the predicate's answer is forced
    # for ring-addressed jobs only: the one-launch forward chain itself (`fused is not None`) still applies, on the
    # gathered batch, with the gather — and the IS weights the sampler left out — issued in front of it.
    from asac_amd import native
    real = native.policy_sample_q_forward_ok
    refused = []

    def ok(job, extra_jobs=None):
        if job.ring.ids:
            refused.append(1)
            return False
        return real(job, extra_jobs)
    monkeypatch.setattr(native, 'policy_sample_q_forward_ok', ok)
    on, off = _learner(True), _learner(False)
    counts = []
    _lockstep(on, off, counts)
    c_on, c_off = counts[0]
    assert refused
    assert c_on.get('asac_window_gather_pad_w') == 1 and c_on.get('asac_step_prologue_sample_partial') == 1, c_on
    assert c_on.get('asac_policy_sample_q_forward') == 2 and sum(c_on.values()) == 9 and sum(c_off.values()) == 9, (c_on, c_off)
    on.close()
    off.close()
