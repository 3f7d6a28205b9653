"""GPU: the learner with `use_normalization=True` under `hip_config['fused_normalizer']` — the plugin's own representation
class behind ONE whitening launch a step (`asac_obs_whiten`), the statistics kept by ONE launch an episode
(`asac_normalizer_update`): against the reference's recorded steps (`f6_step_aux_norm.npz`), against the switch-off learner
(the `NormalizedRep` subclass and the eager update), by launch counts, inside the captured step, through a checkpoint.

Recorded tolerances (`norm/...`) live in tests/normalizer_tolerances.json: enforced at 4x the error observed on an MI355X, a
missing key fails, `ASAC_NORMALIZER_RECORD=<file.json>` records under a loose sanity bound instead."""
import json
import math
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402

HERE = Path(__file__).resolve().parent
EPS32 = float(np.finfo(np.float32).eps)
RECORD = os.environ.get('ASAC_NORMALIZER_RECORD')       # path of the JSON file to record into, or unset
_TOL_PATH = HERE / 'normalizer_tolerances.json'
MEASURED = json.loads(_TOL_PATH.read_text()) if _TOL_PATH.exists() else {}
RECORDED = {}
SANITY = 5e-3       # while recording: nothing may be further off than this (relative to the observable's largest value)


def _np(x):
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def ncheck(key, got, want):
    """fixture comparison: 4x the error recorded on an MI355X (not below one float32 rounding), a missing key fails"""
    got, want = _np(got), _np(want)
    got, want = np.broadcast_arrays(got, want)
    assert np.isfinite(got).all(), key
    err = float(np.abs(got - want).max(initial=0.) / max(float(np.abs(want).max(initial=0.)), 1e-30))
    print(f'normalizer parity {key}: {err:.3e}')
    if RECORD:
        RECORDED[key] = max(RECORDED.get(key, 0.), err)
        out = Path(RECORD)
        out.parent.mkdir(parents=True, exist_ok=True)
        old = json.loads(out.read_text()) if out.exists() else {}
        old.update(RECORDED)
        out.write_text(json.dumps(old, indent=1, sort_keys=True))
        assert err <= SANITY, (key, err)
        return
    assert key in MEASURED, (f'{key!r} has no entry in tests/normalizer_tolerances.json '
                             f'(ASAC_NORMALIZER_RECORD=<file.json> records it)')
    assert err <= max(4. * MEASURED[key], EPS32), (key, err, MEASURED[key])


def _calls(fn):
    from asac_amd import native
    with native.LaunchProfiler(repeat=1) as prof:
        fn()
    return {k: v['calls'] for k, v in prof.summary().items()}


def _vec_agent(hip, plugin='nn_vec', **kw):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(0)
    kw = {'use_normalization': True, **kw}
    return SAC_Base(['vector'], [(6,)], [], 2, kw.pop('model_abs_dir', None), pu.plugin(plugin), device='cuda:0', batch_size=16,
                    n_step=3, replay_config={'capacity': 256}, hip_config=hip, **kw)


def _episodes(obs_shapes, c_action_size, lengths=(40, 30, 50), seed=0):
    rng = np.random.default_rng(seed)
    return [pu.synthetic_episode(rng, obs_shapes, [], c_action_size, (0,), T) for T in lengths]


def _expression(agent, obs_list):
    return [torch.clamp((o - m) / torch.sqrt(v / (agent.normalizer_step + 1)), -5, 5)
            for o, m, v in zip(obs_list, agent.running_means, agent.running_variances)]


# ------------------------------------------------------------------------------------------------------------------------
def test_reference_golden_step_with_the_switch_on(golden_dir):
    """the `aux_norm` case of tests/test_sac_aux_gpu.py (same plugin, recorded noise, alignment hook), switch on"""
    import asac_amd  # noqa: F401
    from algorithm.fused import RecordedNoise
    from tests.plugins import nn_vec_full
    SAC_Base = pu.hooked_learner()
    g = np.load(golden_dir / 'f6_step_aux_norm.npz')
    torch.manual_seed(0)
    agent = SAC_Base(['vector'], [(6,)], [], 2, None, nn_vec_full, device='cuda:0', batch_size=16, n_step=3,
                     replay_config={'capacity': 256}, hip_config={'use_graph': False, 'fused_normalizer': True},
                     use_normalization=True)
    assert agent.normalizer is not None and type(agent.model_rep) is nn_vec_full.ModelRep
    with torch.no_grad():
        for name, obj in agent.ckpt_dict.items():
            if isinstance(obj, torch.nn.Module):
                for k, p in obj.state_dict().items():
                    p.copy_(torch.from_numpy(g[f'w0/{name}/{k}'].copy()))
            elif isinstance(obj, torch.Tensor) and f'w0/t/{name}' in g.files:
                obj.copy_(torch.from_numpy(g[f'w0/t/{name}'].copy()))
        agent.log_c_alpha.copy_(torch.from_numpy(g['w0/log_c_alpha'].copy()))
        agent.log_d_alpha.copy_(torch.from_numpy(g['w0/log_d_alpha'].copy()))
    calls = _calls(lambda: [agent.put_episode(**ep) for ep in pu.golden_episodes(g)])
    assert calls.get('asac_normalizer_update') == int(g['n_episodes']), 'the reference pin must reach the launches'
    rb = agent.replay_buffer
    assert agent.normalizer_step.dtype == torch.int32 and int(agent.normalizer_step) == 120
    ncheck('norm/golden/running_means_after_episodes', agent.running_means[0], g['w1/t/running_means_0'])
    ncheck('norm/golden/running_variances_after_episodes', agent.running_variances[0], g['w1/t/running_variances_0'])
    n_steps = int(g['n_steps'])
    mods = {name: m for name, m in agent.ckpt_dict.items() if isinstance(m, torch.nn.Module)}
    step_box = [0]

    def align_with_reference():
        pu.assert_weights_close(mods, g, 1, 3e-4, rtol=1e-3, atol=2e-5, prefix=f'step{step_box[0]}/w_rq')
        pu.load_golden_weights(agent, g, prefix=f'step{step_box[0]}/w_rq')

    if 'step0/w_rq/model_q_0/' + next(iter(agent.model_q_list[0].state_dict())) in g.files:
        agent.after_rep_q_update = align_with_reference
    for s in range(n_steps):
        step_box[0] = s
        eps = [g[f'step{s}/eps{j}'] for j in range(int(g[f'step{s}/n_eps']))]
        agent.noise = RecordedNoise([g[f'step{s}/u']], eps, list(g[f'step{s}/perm']))
        rb.uniform_source = agent.noise
        calls = _calls(lambda: agent.train())
        assert agent.get_global_step() == s + 1 and calls.get('asac_obs_whiten') == 1
        assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
        assert np.array_equal(rb._ids.cpu().numpy(), g[f'step{s}/sample_ids']), f'step {s}: PER index selection'
        ncheck('norm/golden/loss_q', agent._stats['loss_q'].item(), g[f'step{s}/loss_q'])
        ncheck('norm/golden/td_error', agent._td_error.cpu().numpy()[:, None], g[f'step{s}/td_error'])
        ncheck('norm/golden/tree', rb._tree.cpu().numpy(), g[f'step{s}/tree'])
        if s == 0:
            checked = pu.assert_first_step_gradients(agent, g, rtol=2e-3, atol_frac=5e-5)
            assert checked > 0
    pu.assert_weights_close(mods, g, n_steps, 3e-4, rtol=1e-3, atol=2e-5)
    for name, obj in agent.ckpt_dict.items():
        if isinstance(obj, torch.Tensor) and f'w1/t/{name}' in g.files:     # the normalizer's statistics
            if obj.dtype == torch.int32:
                assert int(obj) == int(g[f'w1/t/{name}'])
            else:
                ncheck(f'norm/golden/tensor_{name}', obj, g[f'w1/t/{name}'])
    rb.check_health()
    agent.close()


# ------------------------------------------------------------------------------------------------------------------------
def _derived_bound(T, terms, old):
    from asac_amd import native
    P = native.NORM_ROW_LANES
    return (math.ceil(T / P) + math.log2(P) + 4) * 2. ** -24 * (np.abs(terms).sum(0) + np.abs(old))


def test_on_against_off_statistics_states_and_actions():
    on, off = _vec_agent({'fused_normalizer': True, 'use_graph': False}), _vec_agent({'use_graph': False})
    from algorithm.nn_models.representation import ModelSimpleRep
    assert type(on.model_rep) is ModelSimpleRep and type(off.model_rep) is not ModelSimpleRep
    assert on.model_rep.state_dict().keys() == off.model_rep.state_dict().keys()
    eps = _episodes([(6,)], 2)
    # Each episode, the switch-on learner's new statistics are within the kernel's derived bound of the float64 recurrence
    # from its own previous state.  The two learners are compared with each other under the sum, over the episodes, of that
    # bound plus the same form for ANY summation order of T terms (gamma = (T + 3) 2^-24: torch's sum, whatever its order) —
    # a difference in the mean carries over to the next episode with a factor 1 - T / step <= 1, and into the variance
    # through sum_t |d_t| (first order).
    acc_m, acc_v, step = np.zeros(6), np.zeros(6), 0
    for ep in eps:
        x = ep['ep_obses_list'][0][0].astype(np.float64)
        T = x.shape[0]
        before = [t.double().cpu().numpy() for t in (on.running_means[0], on.running_variances[0])]
        on.put_episode(**ep), off.put_episode(**ep)
        step += T
        assert int(on.normalizer_step) == int(off.normalizer_step) == step
        assert on.normalizer_step.dtype == off.normalizer_step.dtype == torch.int32
        d = x - before[0]
        terms = d / float(step)
        m1 = on.running_means[0].double().cpu().numpy()
        bound_m = _derived_bound(T, terms, before[0])
        assert (np.abs(m1 - (before[0] + terms.sum(0))) <= bound_m).all()
        terms_v = (x - m1) * d
        v1 = on.running_variances[0].double().cpu().numpy()
        bound_v = _derived_bound(T, terms_v, before[1])
        assert (np.abs(v1 - (before[1] + terms_v.sum(0))) <= bound_v).all()
        any_order = (T + 3) * 2. ** -24
        acc_m = acc_m + bound_m + any_order * (np.abs(terms).sum(0) + np.abs(before[0]))
        acc_v = acc_v + bound_v + any_order * (np.abs(terms_v).sum(0) + np.abs(before[1])) + 2 * acc_m * np.abs(d).sum(0)
        for a, b in ((on, off), (off, on)):     # ... each within the bound of the other's float64 value
            assert (np.abs(a.running_means[0].cpu().numpy() - b.running_means[0].double().cpu().numpy()) <= acc_m).all()
            assert (np.abs(a.running_variances[0].cpu().numpy() - b.running_variances[0].double().cpu().numpy()) <= acc_v).all()
    assert float(np.abs(on.running_means[0].cpu().numpy()).max()) > 0
    # equal statistics: equal bits from everything that whitens
    with torch.no_grad():
        on.running_means[0].copy_(off.running_means[0])
        on.running_variances[0].copy_(off.running_variances[0])
        on._params.flat.copy_(off._params.flat)
        on._target_params.flat.copy_(off._target_params.flat)
    gen = torch.Generator().manual_seed(3)
    window = [(torch.randn(16, 4, 6, generator=gen) * 3).cuda()]
    hidden = torch.zeros(16, 4, 0, device='cuda')
    raw = window[0].clone()
    for is_target in (False, True):
        with torch.no_grad():
            s_on, _ = on.get_l_states(None, None, window, None, hidden, is_target=is_target)
            s_off, _ = off.get_l_states(None, None, window, None, hidden, is_target=is_target)
        assert torch.equal(s_on, s_off) and not torch.equal(s_on, raw)
    assert torch.equal(window[0], raw), '`get_l_states` takes raw observations and leaves them raw'
    assert torch.equal(on.whiten_obs(window)[0], _expression(off, window)[0])
    obs = [window[0][:, 0].contiguous()]
    pre_action, pre_hidden = torch.zeros(16, 2, device='cuda'), torch.zeros(16, 0, device='cuda')
    a_on = on.choose_action_device(obs, pre_action, pre_hidden, disable_sample=True)
    a_off = off.choose_action_device(obs, pre_action, pre_hidden, disable_sample=True)
    for x, y in zip(a_on, a_off):
        assert torch.equal(x, y)
    on.close(), off.close()


def test_the_stock_path_is_engaged():
    from algorithm.nn_models.representation import ModelSimpleRep
    eps = _episodes([(6,)], 2)
    seen = {}
    for name, hip, kw in (('on', {'fused_normalizer': True}, {}),
                          ('off', {}, {}),
                          ('plain', {'head_gather_sidecar': False}, {'use_normalization': False})):
        agent = _vec_agent({'use_graph': False, **hip}, **kw)
        for ep in eps:
            agent.put_episode(**ep)
        agent.train()
        seen[name] = _calls(lambda: agent.train())
        if name == 'on':
            assert type(agent.model_rep) is ModelSimpleRep and agent._head_gather_plan(agent.replay_buffer, build=True) is None
        agent.close()
    assert 'asac_obs_whiten' not in seen['off'] and 'asac_obs_whiten' not in seen['plain']
    assert seen['on'] == {**seen['plain'], 'asac_obs_whiten': 1}, (seen['on'], seen['plain'])


@pytest.mark.parametrize('use_replay_buffer', [True, False], ids=['replay', 'batch_queue'])
def test_one_whiten_a_step_one_update_an_episode(use_replay_buffer):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from tests.plugins import nn_conv
    shapes = [(10,), (3, 30, 30)]
    torch.manual_seed(0)
    agent = SAC_Base(['vector', 'image'], shapes, [], 4, None, nn_conv, device='cuda:0', batch_size=16, n_step=3,
                     burn_in_step=2, replay_config={'capacity': 256}, use_normalization=True,
                     use_replay_buffer=use_replay_buffer, hip_config={'use_graph': False, 'fused_normalizer': True})
    rng = np.random.default_rng(1)
    for T in (40, 30):
        ep = pu.synthetic_episode(rng, shapes, [], 4, tuple(agent.seq_hidden_state_shape), T)
        ep['ep_obses_list'][1] = np.abs(ep['ep_obses_list'][1]) % 1.
        calls = _calls(lambda: agent.put_episode(**ep))
        if use_replay_buffer:
            assert calls.get('asac_normalizer_update') == 1, 'one launch for both observations'
        else:
            assert 'asac_normalizer_update' not in calls, 'batch mode does not update (as the reference)'
    assert int(agent.normalizer_step) == (70 if use_replay_buffer else 0)
    for _ in range(2):
        step = agent.get_global_step()
        calls = _calls(lambda: agent.train())
        assert agent.get_global_step() == step + 1
        assert calls.get('asac_obs_whiten') == 1, 'whatever the number of representation passes'
    batch = agent.replay_buffer._batch if use_replay_buffer else agent.batch_buffer._batch
    raw = [batch[f'obs_{n}'] for n in agent.obs_names]
    for got, want in zip(agent.normalizer.whitened, _expression(agent, raw)):
        assert got.shape == want.shape
        torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)
    assert torch.isfinite(agent._params.flat).all()
    agent.close()


@pytest.mark.parametrize('lookahead', [0, 1])
def test_the_captured_step_whitens_with_the_statistics_of_replay_time(lookahead):
    agent = _vec_agent({'fused_normalizer': True, 'lookahead': lookahead})
    eps = _episodes([(6,)], 2, lengths=(40, 30, 50, 45))
    for ep in eps[:3]:
        agent.put_episode(**ep)
    for _ in range(8):
        agent.train()
    assert agent._graph is not None or (lookahead and agent._la_graphs), 'the step is captured'
    before = (int(agent.normalizer_step), agent.normalizer.flat.clone())
    calls = _calls(lambda: agent.put_episode(**eps[3]))
    assert calls.get('asac_normalizer_update') == 1
    assert int(agent.normalizer_step) == before[0] + 45 and not torch.equal(agent.normalizer.flat, before[1])
    n_tables = len(agent.normalizer._tables)
    agent.train()
    torch.cuda.synchronize()
    assert len(agent.normalizer._tables) == n_tables, 'a replayed step builds nothing'
    rb = agent.replay_buffer
    raw = [rb._batch[f'obs_{n}'] for n in agent.obs_names]
    whitened = agent.normalizer.whitened
    assert whitened[0].shape == raw[0].shape
    want = _expression(agent, raw)[0]
    torch.testing.assert_close(whitened[0], want, rtol=0, atol=0, equal_nan=True)
    assert not torch.equal(whitened[0], raw[0])
    # the launch itself, once more on the same static buffers: raw rows are only read
    raw_before = [r.clone() for r in raw]
    whitened[0].zero_()
    assert agent.normalizer.whiten(raw, static=True) is whitened and len(agent.normalizer._tables) == n_tables
    torch.testing.assert_close(whitened[0], want, rtol=0, atol=0, equal_nan=True)
    assert all(torch.equal(a, b) for a, b in zip(raw, raw_before))
    rb.check_health()
    assert torch.isfinite(agent._params.flat).all() and torch.isfinite(agent._target_params.flat).all()
    agent.close()


def test_checkpoints_cross_the_switch(tmp_path):
    eps = _episodes([(6,)], 2)
    layouts = {}
    for src, dst in (('off', 'on'), ('on', 'off')):
        hip = {'off': {'use_graph': False}, 'on': {'use_graph': False, 'fused_normalizer': True}}
        d = tmp_path / src
        a = _vec_agent(hip[src], model_abs_dir=d)
        for ep in eps:
            a.put_episode(**ep)
        layouts[src] = {k: (tuple(v.shape), v.dtype) if isinstance(v, torch.Tensor) else type(v).__name__
                        for k, v in a.ckpt_dict.items()}
        a.save_model()
        b = _vec_agent(hip[dst], model_abs_dir=d, train_mode=False)
        assert (b.normalizer is not None) == (dst == 'on')
        assert int(b.normalizer_step) == int(a.normalizer_step) == 120 and b.normalizer_step.dtype == torch.int32
        assert torch.equal(b.running_means[0], a.running_means[0]) and not (b.running_means[0] == 0).all()
        assert torch.equal(b.running_variances[0], a.running_variances[0])
        a.close(), b.close()
    assert layouts['on'] == layouts['off'], 'ckpt_dict keys, shapes and dtypes do not depend on the switch'
    assert {'normalizer_step', 'running_means_0', 'running_variances_0'} <= set(layouts['on'])
