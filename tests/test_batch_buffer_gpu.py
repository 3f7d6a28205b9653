"""GPU: the training mode without a replay buffer (`SAC_Base(use_replay_buffer=False)`, `algorithm/batch_buffer.py`,
csrc/batch.hip) against the reference.

  * `get_batch()` of the HBM batch queue equals the reference BatchBuffer's batches bit for bit (golden
    `f12_batch_buffer.npz`), from NumPy episodes and from device-tensor episodes
  * full train() steps (golden `f13_batch_step_<case>.npz`) under the reference's recorded draws: every draw consumed in
    order, losses / entropy / temperature at the f6 step bounds, first-step gradients, weights after the steps
  * an empty queue trains nothing; the captured step and `train_steps(k)` are the eager steps bit for bit while the
    queue ring wraps and overflow drops occur"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402

LR = 3e-4
BATCH_KEYS = ('bn_indexes', 'bn_last_masks', 'bn_padding_masks', 'bnx_obses', 'bn_actions', 'bn_rewards', 'bn_dones',
              'bn_probs', 'bnx_pre_seq_hidden_states')


def _f12_episode(g, i):
    ep = dict(ep_indexes=g[f'put{i}/ep_indexes'],
              ep_obses_list=[g[f'put{i}/obs_0'], g[f'put{i}/obs_1']],
              ep_actions=g[f'put{i}/ep_actions'], ep_rewards=g[f'put{i}/ep_rewards'], ep_dones=g[f'put{i}/ep_dones'],
              ep_probs=g[f'put{i}/ep_probs'], ep_pre_seq_hidden_states=g[f'put{i}/ep_pre_seq_hidden_states'])
    last = np.zeros_like(ep['ep_indexes'], dtype=bool)
    last[:, -1] = True
    last[ep['ep_indexes'] == -1] = True
    ep['ep_last_masks'] = last
    return ep


def _to_device(ep):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return {k: ([dev(o) for o in v] if isinstance(v, list) else dev(v)) for k, v in ep.items()}


@pytest.mark.parametrize('source', ['numpy', 'device'])
def test_get_batch_bit_exact_against_reference(golden_dir, source):
    import asac_amd  # noqa: F401
    from algorithm.batch_buffer import BatchBuffer
    g = np.load(golden_dir / 'f12_batch_buffer.npz')
    perms = [g[f'put{i}/perm'] for i in range(int(g['n_put']))]
    bb = BatchBuffer(int(g['burn_in']), int(g['n_step']), g['padding_action'], int(g['batch_size']),
                     device=torch.device('cuda:0'), max_size=int(g['max_size']), permutation=lambda n: perms.pop(0))
    n_put = n_get = 0
    for op in g['ops']:
        if op == 0:
            ep = _f12_episode(g, n_put)
            bb.put_episode(**(ep if source == 'numpy' else _to_device(ep)))
            n_put += 1
            continue
        batch = bb.get_batch()
        if bool(g[f'get{n_get}/empty']):
            assert batch is None, f'get {n_get}'
        else:
            assert batch is not None, f'get {n_get}'
            for k, v in zip(BATCH_KEYS, batch):
                if k == 'bnx_obses':
                    for j, o in enumerate(v):
                        want = g[f'get{n_get}/obs_{j}']
                        assert o.dtype == torch.from_numpy(want).dtype and np.array_equal(o.cpu().numpy(), want), \
                            f'get {n_get} obs {j}'
                else:
                    want = g[f'get{n_get}/{k}']
                    got = v.cpu().numpy()
                    assert got.dtype == want.dtype and got.shape == want.shape, (n_get, k, got.dtype, got.shape)
                    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f'get {n_get} {k}'
        n_get += 1
    assert not perms and n_get == int(g['n_get'])


# ------------------------------------------------------------------------------------------------
# full steps against the reference (f13)
# ------------------------------------------------------------------------------------------------
# case -> (plugin, learner keywords, observation / size set, the representation is trained by the step)
F13 = {
    'n1': ('nn_vec', dict(n_step=1, use_priority=False), pu.VEC, False),
    'n4_is': ('nn_vec', dict(n_step=4, use_priority=True, use_n_step_is=True), pu.VEC, False),
    'rnn': ('nn_rnn', dict(n_step=3, burn_in_step=3, seq_encoder='RNN'), pu.VEC, True),
    'conv': ('nn_conv', dict(n_step=3, burn_in_step=5, ensemble_q_num=4, ensemble_q_sample=2), dict(pu.IMG, batch_size=8),
             True),
}
# the f6 step bounds (tests/test_sac_step_gpu.py TOL): observable -> (rtol, atol)
TOL = {'loss_q': (2e-4, 0.), 'loss_policy': (2e-4, 2e-5), 'c_entropy': (2e-4, 2e-5), 'log_c_alpha': (1e-5, 0.),
       'grad0': (2e-3, 2e-5), 'weights': (5e-4, 2e-5)}


def make_batch_agent(plugin_name, kw, io, use_graph=False, hip=None):
    import asac_amd  # noqa: F401
    SAC_Base = pu.hooked_learner()
    from algorithm.utils.enums import convert_config_to_enum
    kw = dict(kw)
    convert_config_to_enum(kw)
    return SAC_Base(io['obs_names'], io['obs_shapes'], [], io['c_action_size'], None, pu.plugin(plugin_name),
                    device='cuda:0', batch_size=io['batch_size'], use_replay_buffer=False,
                    hip_config={'use_graph': use_graph, **(hip or {})}, **kw)


def _close(got, want, rtol, atol, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=rtol, atol=atol,
                               err_msg=what)


@pytest.mark.parametrize('case', list(F13))
def test_batch_steps_vs_reference_golden(golden_dir, case):
    from algorithm.fused import RecordedNoise
    plugin_name, kw, io, trained_rep = F13[case]
    g = np.load(golden_dir / f'f13_batch_step_{case}.npz')
    agent = make_batch_agent(plugin_name, kw, io)
    mods = pu.load_golden_weights(agent, g)
    perms = [g[f'ep{i}/perm'] for i in range(int(g['n_episodes']))]
    agent.batch_buffer.permutation = lambda n: perms.pop(0)
    for ep in pu.golden_episodes(g, len(io['obs_shapes'])):
        agent.put_episode(**ep)
    assert not perms
    step_box = [0]

    def align_with_reference():
        s_ = step_box[0]
        pu.assert_weights_close(mods, g, 1, LR, *TOL['weights'], prefix=f'step{s_}/w_rq', log_key=None)
        pu.load_golden_weights(agent, g, prefix=f'step{s_}/w_rq')

    if trained_rep:
        agent.after_rep_q_update = align_with_reference
    n_steps = int(g['n_steps'])
    for s in range(n_steps):
        step_box[0] = s
        eps = [g[f'step{s}/eps{j}'] for j in range(int(g[f'step{s}/n_eps']))]
        agent.noise = RecordedNoise([], eps, list(g[f'step{s}/perm']))
        alpha_before = agent.log_c_alpha.detach().clone()
        assert agent.train() == s + 1
        assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
        _close(agent._stats['loss_q'].item(), g[f'step{s}/loss_q'], *TOL['loss_q'], f'step {s} loss_q')
        agent._refresh_policy_stats(alpha_before)
        _close(agent._stats['loss_policy'].item(), g[f'step{s}/loss_policy'], *TOL['loss_policy'], f'step {s} loss_policy')
        _close(agent._stats['c_entropy'].item(), g[f'step{s}/c_entropy'], *TOL['c_entropy'], f'step {s} c_entropy')
        _close(agent.log_c_alpha.item(), g[f'step{s}/log_c_alpha'], *TOL['log_c_alpha'], f'step {s} log_c_alpha')
        if s == 0 and any(k.startswith('g0/') for k in g.files):
            pu.assert_first_step_gradients(agent, g, rtol=TOL['grad0'][0], atol_frac=TOL['grad0'][1], log_key=None)
    if any(k.startswith('w1/') for k in g.files):
        pu.assert_weights_close(mods, g, n_steps, LR, *TOL['weights'], log_key=None)
    assert len(agent.batch_buffer) == int(g['queued_after'])
    agent.close()


# ------------------------------------------------------------------------------------------------
# queue behaviour inside the learner
# ------------------------------------------------------------------------------------------------
def _episodes(seed, lens, hidden=(0,)):
    rng = np.random.default_rng(seed)
    return [pu.synthetic_episode(rng, [(6,)], [], 2, hidden, T) for T in lens]


def test_empty_queue_trains_nothing_then_trains_after_a_put():
    torch.manual_seed(3)
    agent = make_batch_agent('nn_vec', dict(n_step=4), pu.VEC)
    before = agent._params.flat.clone()
    assert agent.train() == 0 and agent.get_global_step() == 0
    assert torch.equal(agent._params.flat, before)
    agent.put_episode(**_episodes(1, [20])[0])           # 19 windows < 32: only a rest, still no batch
    assert agent.train() == 0 and torch.equal(agent._params.flat, before)
    agent.put_episode(**_episodes(2, [30])[0])           # 19 + 29 = 48: one batch
    assert agent.train() == 1
    assert not torch.equal(agent._params.flat, before)
    assert agent.train() == 1                            # the queue is empty again
    agent.close()


def _run_schedule(case_kw, hidden, use_graph, runs):
    """puts interleaved with steps: more than max_size + 1 steps, a long episode that overflows the queue"""
    torch.manual_seed(3), np.random.seed(3), random.seed(3)
    agent = make_batch_agent('nn_rnn' if hidden != (0,) else 'nn_vec', case_kw, pu.VEC, use_graph=use_graph)
    eps = _episodes(5, [60, 45, 400, 70, 33, 80, 90], hidden)
    torch.manual_seed(4)
    agent.put_episode(**eps[0])
    agent.put_episode(**eps[1])
    for i in range(2, len(eps)):
        agent.put_episode(**eps[i])
        if runs and i >= 4:
            agent.train_steps(4)
        else:
            for _ in range(4):
                agent.train()
    torch.cuda.synchronize()
    out = (agent.get_global_step(), agent._params.flat.clone(), agent._target_params.flat.clone(),
           agent._opt_steps.clone(), agent.batch_buffer._head.clone(), len(agent.batch_buffer))
    captured = agent._graph is not None
    runs_used = any(c.run is not None and c.run.exec_handle is not None for c in agent._graph_runs.values())
    agent.close()
    return out, captured, runs_used


@pytest.mark.parametrize('case', ['vec', 'rnn'])
def test_graph_replay_is_the_eager_step_bit_for_bit(case):
    kw, hidden = (dict(n_step=4), (0,)) if case == 'vec' else (dict(n_step=3, burn_in_step=3, seq_encoder='RNN'), (2, 8))
    eager, captured_e, _ = _run_schedule(kw, hidden, use_graph=False, runs=False)
    graph, captured_g, _ = _run_schedule(kw, hidden, use_graph=True, runs=False)
    assert not captured_e and captured_g, 'graph capture must succeed for stock models'
    assert eager[0] == graph[0] >= 19 and eager[5] == graph[5]
    for name, a, b in zip(('weights', 'target weights', 'optimizer steps', 'head'), eager[1:5], graph[1:5]):
        assert torch.equal(a, b), name
    assert int(graph[4].item()) > 11, 'the queue ring must wrap'


def test_train_steps_is_the_train_calls_bit_for_bit():
    kw = dict(n_step=4)
    single, _, _ = _run_schedule(kw, (0,), use_graph=True, runs=False)
    multi, captured, runs_used = _run_schedule(kw, (0,), use_graph=True, runs=True)
    assert captured and runs_used, 'train_steps(4) must replay one 4-step graph'
    assert single[0] == multi[0] and single[5] == multi[5]
    for name, a, b in zip(('weights', 'target weights', 'optimizer steps', 'head'), single[1:5], multi[1:5]):
        assert torch.equal(a, b), name


def test_batch_mode_refuses_data_parallel_and_lookahead_is_off():
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    with pytest.raises(ValueError, match='single-GPU'):
        SAC_Base(['vector'], [(6,)], [], 2, None, pu.plugin('nn_vec'), device='cuda:0', batch_size=32,
                 use_replay_buffer=False, hip_config={'dist': object()})
    agent = make_batch_agent('nn_vec', dict(n_step=4), pu.VEC, hip={'lookahead': 1})
    assert agent._lookahead == 0 and not hasattr(agent, 'replay_buffer')
    agent.close()
