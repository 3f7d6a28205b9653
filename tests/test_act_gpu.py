"""GPU: policy-based acting on the native path (`hip_config['fused_act']`, csrc/act.hip).

  * the kernel against the float64 restatement (tests/act_ref.py) on the same draws: every one-hot EXACTLY (the draws keep a
    margin of `act_ref.MIN_MARGIN` from every boundary in the reference, asserted), the float outputs within 4x the error
    recorded on an MI355X in `tests/act_tolerances.json` (a missing key fails; `ASAC_ACT_RECORD=<file.json>` records the
    observed errors into that file instead) AND within the bounds the project already enforces on acting
    (tests/test_surface_parity_gpu.py: rtol 1e-5 / atol 2e-6 on actions, rtol 2e-4 / atol 1e-6 on densities)
  * bit equalities with `squash_sample_fwd`, `squash_prob` and `discrete_policy_loss_grad`'s `probs_out`
  * bad arguments are refused without a launch
  * the learner: launch counts, the reference's fixture `tests/golden/f20_act.npz`, recorded draws, switch on against off,
    frequencies, a masking plugin policy, `choose_attn_action`, and what stays on the eager code"""
import functools
import json
import os
import random
import types
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import act_ref as ar  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.golden.make_act_golden import CASES  # noqa: E402

HERE = Path(__file__).resolve().parent
EPS32 = float(np.finfo(np.float32).eps)
RECORD = os.environ.get('ASAC_ACT_RECORD')          # path of the JSON file to record into, or unset
_TOL_PATH = HERE / 'act_tolerances.json'
MEASURED = json.loads(_TOL_PATH.read_text()) if _TOL_PATH.exists() else {}
RECORDED = {}
ACTION_BOUND = dict(rtol=1e-5, atol=2e-6)           # tests/test_surface_parity_gpu.py, acting
DENSITY_BOUND = dict(rtol=2e-4, atol=1e-6)
ACTING_LAUNCHES = ('asac_act_policy', 'asac_squash_sample_fwd', 'asac_squash_prob', 'asac_rnd_pick', 'asac_drnd_pick',
                   'asac_dqn_act')
FLAG = 'fused_act'


def scaled_error(got, want) -> float:
    """max |got - want| over the observable's largest magnitude"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max(initial=0.) / max(float(np.abs(want).max(initial=0.)), 1e-30))


def fcheck(key, got, want, bound=None):
    """4x the error recorded on an MI355X (not below one float32 rounding), a missing key fails; `bound`: the project's
    elementwise bound on this kind of output, held as well"""
    err = scaled_error(got, want)
    print(f'act parity {key}: {err:.3e}')
    if bound is not None:
        np.testing.assert_allclose(got, want, err_msg=key, **bound)
    if RECORD:
        RECORDED[key] = max(RECORDED.get(key, 0.), err)
        out = Path(RECORD)
        out.parent.mkdir(parents=True, exist_ok=True)
        old = json.loads(out.read_text()) if out.exists() else {}
        old.update({k: max(v, old.get(k, 0.)) for k, v in RECORDED.items()})
        out.write_text(json.dumps(old, indent=1, sort_keys=True))
        return
    assert key in MEASURED, f'{key!r} has no entry in tests/act_tolerances.json (ASAC_ACT_RECORD=<file.json> records it)'
    assert err <= max(4. * MEASURED[key], EPS32), (key, err, MEASURED[key])


def test_the_recorded_errors_are_below_the_projects_acting_bounds():
    """every recorded figure (relative to the output's largest value) is below the relative bound the project enforces on
    that kind of output, 4x included"""
    assert MEASURED, 'tests/act_tolerances.json is missing'
    for key, v in MEASURED.items():
        if key.startswith('_'):
            continue
        limit = DENSITY_BOUND['rtol'] if key.endswith(('/density', '/prob')) else ACTION_BOUND['rtol']
        assert 4. * v <= limit, (key, v)


# ------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------
MODES = {'sample': dict(deterministic=False, noise=None), 'deter': dict(deterministic=True, noise=None),
         'noise': dict(deterministic=False, noise=(0.1, 0.9)), 'noise_flat': dict(deterministic=False, noise=(0.5, 0.5)),
         'deter_noise': dict(deterministic=True, noise=(0.1, 0.9))}
# (B, branches, A, head_raw, strided rows): B one past a workgroup, K and D at their limits, A at its limit, no branches
SHAPES = [(1, (3, 2), 0, 0, False), (7, (3, 2), 2, 1, True), (65, (3, 2), 1, 0, True), (7, (1,), 0, 0, True),
          (65, (2,) * 8, 8, 1, False), (7, (64,), 0, 0, False), (65, (64,), 8, 0, True), (1, (), 1, 1, False),
          (7, (), 8, 0, True), (65, (), 2, 1, True), (7, (3, 2), 2, 0, False)]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(a, strided, pad=3):
    """[B, n] array -> device tensor, with `strided` a view of wider rows"""
    if a is None:
        return None
    if not strided:
        return _dev(a)
    wide = torch.full((a.shape[0], a.shape[1] + pad), 9., device='cuda')
    wide[:, :a.shape[1]] = _dev(a)
    return wide[:, :a.shape[1]]


def _launch(case, mode, u, eps, strided=False):
    """the launch on a case's arrays -> (action, prob) as numpy"""
    from asac_amd import native
    sizes, A = case['sizes'], case['A']
    B, D = case['B'], sum(sizes)
    br = native.branches(sizes) if sizes else None
    logits = _rows(case.get('logits'), strided)
    loc = scale = None
    if A:
        if strided:         # the two halves of a [B, 2A] row
            ls = _dev(np.concatenate([case['loc'], case['scale']], axis=1))
            loc, scale = ls[:, :A], ls[:, A:]
        else:
            loc, scale = _dev(case['loc']), _dev(case['scale'])
    action = torch.full((B, D + A), 7., device='cuda')
    prob = torch.full((B, D + A), 7., device='cuda')
    native.act_policy(native.act_job(br, logits, loc, scale, _rows(u, strided), _rows(eps, strided), action, prob,
                                     head_raw=case['head_raw'], deterministic=mode['deterministic'], action_noise=mode['noise']))
    return action.cpu().numpy(), prob.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(B, sizes, A, head_raw, seed=0):
    """float32 inputs of one shape: logits ~ N(0, 1); mean in [-0.5, 0.5] and logstd in [-2, 0.5] (a well-conditioned
    density), handed over raw (`head_raw`) or bounded in float32"""
    rng = np.random.default_rng(1000 * seed + 17 * B + 3 * sum(sizes) + A)
    c = dict(B=B, sizes=tuple(sizes), A=A, head_raw=bool(head_raw))
    if sizes:
        c['logits'] = rng.standard_normal((B, sum(sizes))).astype(np.float32)
    if A:
        mean = rng.uniform(-0.5, 0.5, (B, A)).astype(np.float32)
        logstd = rng.uniform(-2., 0.5, (B, A)).astype(np.float32)
        if head_raw:
            c['loc'], c['scale'] = mean, logstd
        else:
            c['loc'] = (np.tanh(mean / np.float32(5.)) * np.float32(5.)).astype(np.float32)
            c['scale'] = np.exp(logstd).astype(np.float32)
    return c


def _draws(case, mode, seed):
    """(u, eps, the reference's result): the uniforms keep `act_ref.MIN_MARGIN` from every boundary they are compared with;
    under noise the sampling normals stay in [-1, 1], so that `atanh` of the action before the noise is well conditioned"""
    sizes, A, B = case['sizes'], case['A'], case['B']
    noise = mode['noise']
    nu, ne = ar.draw_columns(len(sizes), A, mode['deterministic'], noise is not None)
    rng = np.random.default_rng(seed)
    eps = None
    if ne:
        eps = rng.standard_normal((B, ne)).astype(np.float32)
        if noise is not None and not mode['deterministic']:
            eps[:, :A] = np.clip(eps[:, :A], -1., 1.)
    kw = dict(sizes=sizes, logits=case.get('logits'), loc=case.get('loc'), scale=case.get('scale'), head_raw=case['head_raw'],
              eps=eps, deterministic=mode['deterministic'], noise=noise)
    if not nu:
        return None, eps, ar.act(u=None, **kw)
    u, ref = ar.redraw_close(rng, lambda r: r.random((B, nu)).astype(np.float32), **kw)
    return u, eps, ref


def _compare(key, case, ref, action, prob):
    sizes, A = case['sizes'], case['A']
    D = sum(sizes)
    if sizes:
        assert ref['margin'] >= ar.MIN_MARGIN, 'the reference side keeps the margin'
        np.testing.assert_array_equal(action[:, :D], ref['onehot'], err_msg=f'{key}: every one-hot, no row left out')
        fcheck(f'{key}/p', prob[:, :D], ref['p'], DENSITY_BOUND)
    if A:
        fcheck(f'{key}/a', action[:, D:], ref['a'], ACTION_BOUND)
        fcheck(f'{key}/density', prob[:, D:], ar.density(action[:, D:], ref['loc'], ref['scale']), DENSITY_BOUND)


@pytest.mark.parametrize('B,sizes,A,head_raw,strided', SHAPES)
def test_kernel_against_float64(B, sizes, A, head_raw, strided):
    case = _case(B, sizes, A, head_raw)
    for i, (name, mode) in enumerate(MODES.items()):
        u, eps, ref = _draws(case, mode, seed=100 + i)
        action, prob = _launch(case, mode, u, eps, strided)
        _compare(f'kernel/{name}', case, ref, action, prob)
        if mode['noise'] is not None and sizes:
            gate = 0 if mode['deterministic'] else len(sizes)
            opened = u[:, gate] < ref['level']
            assert B < 7 or (opened.any() and not opened.all()), 'both sides of the gate occur'


def test_noise_levels_on_the_device_are_torch_linspace():
    """the rows' noise levels, read off the launch: a gate uniform exactly AT the level stays shut, one float32 below opens"""
    for B in (1, 2, 7, 65):
        case = dict(B=B, sizes=(2,), A=0, head_raw=False, logits=np.tile(np.float32([5., -5.]), (B, 1)))
        level = torch.linspace(0.1, 0.9, B).numpy()
        for below, want in ((False, 0), (True, 1)):
            u = np.zeros((B, 2), dtype=np.float32)          # deterministic + noise: (gate | index)
            u[:, 0] = np.nextafter(level, np.float32(0)) if below else level
            u[:, 1] = 0.75                                   # floor(0.75 * 2) = 1: the entry the greedy rule never takes
            action, _ = _launch(case, MODES['deter_noise'], u, None)
            assert (action[:, 1] == want).all(), (B, below)


def test_ties_zero_uniforms_and_masked_entries():
    """equal logits: the lowest index wins (deterministic); u == 0 takes the first entry of positive probability; a branch
    whose last entries are -inf never returns them, u one float32 below 1 included, and their `prob` is exactly 0"""
    ninf, under1 = -np.inf, np.nextafter(np.float32(1), np.float32(0))
    logits = np.float32([[1., 1., 0.5, 2., 2., -1.],           # ties in both branches
                         [ninf, 0.3, 0.2, 0.1, ninf, ninf],    # masked head and tail
                         [0.5, ninf, ninf, 0.2, 0.1, ninf]])
    case = dict(B=3, sizes=(3, 3), A=0, head_raw=False, logits=logits)
    action, prob = _launch(case, MODES['deter'], None, None)
    np.testing.assert_array_equal(action, ar.act(sizes=(3, 3), logits=logits, deterministic=True)['onehot'])
    assert action[0].tolist() == [1, 0, 0, 1, 0, 0]
    for u in (np.zeros((3, 2), dtype=np.float32), np.full((3, 2), under1, dtype=np.float32)):
        action, prob = _launch(case, MODES['sample'], u, None)
        ref = ar.act(sizes=(3, 3), logits=logits, u=u)
        np.testing.assert_array_equal(action, ref['onehot'])
        masked = ~np.isfinite(logits)
        assert not action[masked].any() and not prob[masked].any(), 'a masked entry is never chosen and has probability 0'
        np.testing.assert_allclose(prob, ref['p'], rtol=1e-6)
    assert action[1].tolist() == [0, 0, 1, 1, 0, 0] and action[2].tolist() == [1, 0, 0, 0, 1, 0]      # (u just under 1)


def test_a_saturated_action_under_noise_follows_the_composition():
    """tanh saturates to exactly 1 in float32, atanh(1) is inf, and the noisy action stays 1 (the reference's composition,
    infinities included); the density stays finite (the clamp)"""
    case = dict(B=2, sizes=(), A=1, head_raw=False, loc=np.float32([[20.], [-20.]]), scale=np.float32([[1.], [1.]]))
    eps = np.float32([[0.1, -3.], [0.2, 3.]])
    action, prob = _launch(case, MODES['noise_flat'], None, eps)
    assert action.tolist() == [[1.], [-1.]] and np.isfinite(prob).all()


def test_bit_equalities_with_the_librarys_other_launches():
    """without noise `a` is `squash_sample_fwd`'s `a_tanh`, the continuous `prob` is `squash_prob` on the returned action
    (with and without noise), the discrete `prob` is `discrete_policy_loss_grad`'s `probs_out`"""
    from asac_amd import native
    B, sizes, A = 65, (3, 2), 2
    D = sum(sizes)
    case = _case(B, sizes, A, 0, seed=1)
    for name in ('sample', 'noise'):
        mode = MODES[name]
        u, eps, _ = _draws(case, mode, seed=7)
        action, prob = _launch(case, mode, u, eps)
        loc, scale = _dev(case['loc']), _dev(case['scale'])
        if name == 'sample':
            a = torch.empty(B, A, device='cuda')
            native.squash_sample_fwd(loc, scale, _dev(eps), a, torch.empty(B, device='cuda'))
            np.testing.assert_array_equal(action[:, D:], a.cpu().numpy())
        dens = torch.empty(B, A, device='cuda')
        win = lambda t: t.as_strided((B, 1, A), (t.stride(0), t.stride(0), 1))      # noqa: E731
        native.squash_prob(win(loc), win(scale), win(_dev(action[:, D:])), 0, win(dens), 0)
        np.testing.assert_array_equal(prob[:, D:], dens.cpu().numpy())
        probs = torch.empty(B, D, device='cuda')
        f = lambda *s: torch.zeros(*s, device='cuda')      # noqa: E731
        native.discrete_policy_loss_grad(native.branches(sizes), _dev(case['logits']), [torch.randn(B, D, device='cuda')], None, 1,
                                         torch.rand(B, D, device='cuda'), f(1), 0., f(1), f(B, D), f(1), probs_out=probs)
        np.testing.assert_array_equal(prob[:, :D], probs.cpu().numpy())


def test_entry_point_refuses_bad_arguments():
    """null outputs, a branch table that does not add up, sizes over the limits, neither part present, a missing input or
    draw buffer the mode needs, noise_lo > noise_hi, negative noise, B < 0: `AsacNativeError`, the outputs untouched; B == 0
    launches nothing; the good job then runs"""
    from asac_amd import native
    B, sizes, A = 4, (3, 2), 2
    D, K = sum(sizes), len(sizes)
    logits, ls = torch.randn(B, D, device='cuda'), torch.rand(B, 2 * A, device='cuda') + 0.1
    u, eps = torch.rand(B, 2 * K + 1, device='cuda'), torch.randn(B, 2 * A, device='cuda')
    action, prob = torch.full((B, D + A), 7., device='cuda'), torch.full((B, D + A), 7., device='cuda')

    def job(**over):
        j = native.act_job(native.branches(sizes), logits, ls[:, :A], ls[:, A:], u, eps, action, prob, action_noise=(0.1, 0.9))
        for k, v in over.items():
            setattr(j, k, v)
        return j

    def table(**over):
        br = native.branches(sizes)
        for k, v in over.items():
            setattr(br, k, v)
        return br

    nine = native.Branches()
    nine.K, nine.D = 9, 9
    for k in range(8):
        nine.size[k] = 1
    none = native.Branches()
    bad = [job(action_out=None), job(prob_out=None), job(branches=table(D=D + 1)), job(branches=table(D=65)), job(branches=nine),
           job(A=9), job(A=-1), job(branches=none, A=0), job(logits=None), job(loc=None), job(scale=None), job(u=None),
           job(eps=None), job(noise_lo=0.9, noise_hi=0.1), job(noise_lo=-0.1), job(noise_lo=float('nan')), job(B=-1)]
    for j in bad:
        with pytest.raises(native.AsacNativeError):
            native.act_policy(j)
    native.act_policy(job(B=0))
    torch.cuda.synchronize()
    assert (action == 7.).all() and (prob == 7.).all(), 'no launch'
    # what a mode does not need may be missing: deterministic without noise reads no draws
    native.act_policy(job(u=None, eps=None, deterministic=1, use_noise=0))
    native.act_policy(job())
    torch.cuda.synchronize()
    assert torch.isfinite(action).all() and torch.isfinite(prob).all() and not (action == 7.).any()


# ------------------------------------------------------------------------------------------------------------------------
# the learner
# ------------------------------------------------------------------------------------------------------------------------
def _learner(d_sizes=(3, 2), c_size=0, plugin='nn_vec', seed=0, hip=None, **kw):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    torch.manual_seed(seed), np.random.seed(seed), random.seed(seed)
    nn = pu.plugin(plugin) if isinstance(plugin, str) else plugin
    kw = dict(kw)
    convert_config_to_enum(kw)
    return SAC_Base(['vector'], [(6,)], list(d_sizes), c_size, None, nn, device='cuda:0', n_step=3, batch_size=16,
                    replay_config={'capacity': 256}, hip_config={'use_graph': False, **(hip or {})}, **kw)


def _inputs(agent, batch=7, seed=3):
    rng = np.random.default_rng(seed)
    obs = [rng.standard_normal((batch, 6)).astype(np.float32)]
    pre_action = np.zeros((batch, agent.d_action_summed_size + agent.c_action_size), dtype=np.float32)
    hidden = np.zeros((batch, *agent.seq_hidden_state_shape), dtype=np.float32)
    return obs, pre_action, hidden


def _acting_calls(prof):
    return {k: v['calls'] for k, v in prof.summary().items() if k in ACTING_LAUNCHES}


def _is_one_hot(action, sizes):
    parts = np.split(action, np.cumsum(sizes)[:-1], axis=-1)
    return all(((p == 0) | (p == 1)).all() and (p.sum(-1) == 1).all() for p in parts)


COUNTED = {
    'discrete': dict(d=(3, 2), c=0),
    'hybrid': dict(d=(3, 2), c=2),
    'continuous_noise': dict(d=(), c=2, kw=dict(action_noise=[0., 1.])),
    'discrete_deter': dict(d=(3, 2), c=0, acting=dict(disable_sample=True)),
}


@pytest.mark.parametrize('case', list(COUNTED))
def test_launch_counts(case):
    """with the switch on one `choose_action` issues exactly one `asac_act_policy` and none of the other acting launches,
    with the switch off none at all.  (Fails without the launch.)"""
    from asac_amd import native
    cfg = COUNTED[case]
    for fused in (True, False):
        agent = _learner(cfg['d'], cfg['c'], hip={FLAG: fused}, **cfg.get('kw', {}))
        with native.LaunchProfiler(repeat=1) as prof:
            action, prob, _ = agent.choose_action(*_inputs(agent), **cfg.get('acting', {}))
        assert _acting_calls(prof) == ({'asac_act_policy': 1} if fused else {})
        D = sum(cfg['d'])
        assert action.shape == prob.shape == (7, D + cfg['c']) and np.isfinite(action).all() and np.isfinite(prob).all()
        assert not D or _is_one_hot(action[:, :D], cfg['d'])
        agent.close()


def test_a_stock_continuous_learner_without_noise_keeps_its_path():
    from asac_amd import native
    for fused in (True, False):
        agent = _learner((), 2, hip={FLAG: fused})
        with native.LaunchProfiler(repeat=1) as prof:
            agent.choose_action(*_inputs(agent))
        assert _acting_calls(prof) == {'asac_squash_sample_fwd': 1, 'asac_squash_prob': 1}
        agent.close()


@pytest.mark.parametrize('case', list(CASES))
def test_fixture_through_choose_action(golden_dir, case):
    """the reference's own `_choose_action` (disable_sample, no noise) on its weights and inputs: the one-hots exactly, the
    continuous action, the probabilities and the next hidden state within the recorded tolerances"""
    from asac_amd import native
    g = np.load(golden_dir / 'f20_act.npz')
    plugin, sizes, A, kw = CASES[case]
    D = sum(sizes)
    agent = _learner(sizes, A, plugin=plugin, **{k: v for k, v in kw.items() if k != 'n_step'})
    pu.load_golden_weights(agent, g, prefix=f'{case}/w0')
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, hidden = agent.choose_action([g[f'{case}/in/obs_list'].copy()], g[f'{case}/in/pre_action'].copy(),
                                                   g[f'{case}/in/pre_seq_hidden_state'].copy(), disable_sample=True)
    assert _acting_calls(prof) == {'asac_act_policy': 1}
    np.testing.assert_array_equal(action[:, :D], g[f'{case}/action'][:, :D])
    fcheck(f'fixture/{case}/p', prob[:, :D], g[f'{case}/prob'][:, :D], DENSITY_BOUND)
    if A:
        fcheck(f'fixture/{case}/a', action[:, D:], g[f'{case}/action'][:, D:], ACTION_BOUND)
        fcheck(f'fixture/{case}/density', prob[:, D:], g[f'{case}/prob'][:, D:], DENSITY_BOUND)
    if hidden.size:
        assert case == 'discrete_rnn', 'the recurrent representation ran'
        fcheck(f'fixture/{case}/hidden', hidden, g[f'{case}/hidden'], ACTION_BOUND)
    agent.close()


def _state(agent, obs, pre_action, hidden):
    """the state `choose_action` forms for these inputs"""
    dev = lambda x: torch.from_numpy(x).to(agent.device)      # noqa: E731
    with torch.no_grad():
        state, _ = agent.model_rep([dev(o).unsqueeze(1) for o in obs], dev(pre_action).unsqueeze(1), dev(hidden).unsqueeze(1))
    return state.squeeze(1)


def _heads(agent, obs, pre_action, hidden):
    """the stock policy's raw head outputs at that state, as numpy (None for an absent part)"""
    with torch.no_grad():
        heads = agent.model_policy.heads_raw(_state(agent, obs, pre_action, hidden))
    return [None if h is None else h.cpu().numpy() for h in heads]


@pytest.mark.parametrize('d,c,disable_sample,noise', [((3, 2), 2, False, (0.1, 0.9)), ((3, 2), 0, False, None),
                                                      ((3, 2), 2, True, (0.1, 0.9)), ((3, 2), 2, False, None)])
def test_recorded_draws(d, c, disable_sample, noise):
    """`RecordedNoise(u=[..], eps=[..])` asserts the buffers' shapes: at most one `uniform_` and one `normal_` per call, in
    the documented column layout; the result is `act_ref` on the same draws, and the noise is used up"""
    from algorithm.fused import RecordedNoise
    agent = _learner(d, c, seed=2, action_noise=None if noise is None else list(noise))
    inputs = _inputs(agent)
    logits, mean, logstd = _heads(agent, *inputs)
    case = dict(B=7, sizes=tuple(d), A=c, head_raw=True, logits=logits, loc=mean, scale=logstd)
    mode = dict(deterministic=disable_sample, noise=noise)
    u, eps, ref = _draws(case, mode, seed=11)
    nu, ne = ar.draw_columns(len(d), c, disable_sample, noise is not None)
    assert (u is None) == (nu == 0) and (eps is None) == (ne == 0)
    agent.noise = RecordedNoise([u.astype(np.float64)] if nu else [], [eps] if ne else [], ())
    action, prob, _ = agent.choose_action(*inputs, disable_sample=disable_sample)
    assert agent.noise.exhausted()
    _compare('learner/recorded', case, ref, action, prob)
    agent.close()


def test_continuous_noise_draws_one_gaussian_buffer():
    """a stock continuous learner with `action_noise`: one `normal_` of [batch, 2A] (sampling | noise columns), no
    `uniform_`; the action is `act_ref`'s on the eager policy's (loc, scale) within the recorded tolerance"""
    from algorithm.fused import RecordedNoise
    agent = _learner((), 2, seed=4, action_noise=[0., 1.])
    inputs = _inputs(agent)
    with torch.no_grad():
        c_policy = agent.model_policy(_state(agent, *inputs), None)[1]
    case = dict(B=7, sizes=(), A=2, head_raw=False, loc=c_policy.loc.cpu().numpy(), scale=c_policy.scale.cpu().numpy())
    mode = dict(deterministic=False, noise=(0., 1.))
    _, eps, ref = _draws(case, mode, seed=12)
    agent.noise = RecordedNoise((), [eps], ())
    action, prob, _ = agent.choose_action(*inputs)
    assert agent.noise.exhausted() and eps.shape == (7, 4)
    fcheck('learner/continuous_noise/a', action, ref['a'], ACTION_BOUND)
    fcheck('learner/continuous_noise/density', prob, ar.density(action, ref['loc'], ref['scale']), DENSITY_BOUND)
    agent.close()


def test_switch_on_against_off():
    """deterministic, no noise, hybrid: equal one-hots, floats within the recorded tolerances"""
    out = {}
    for fused in (True, False):
        agent = _learner((3, 2), 2, seed=5, hip={FLAG: fused})
        out[fused] = agent.choose_action(*_inputs(agent), disable_sample=True)
        agent.close()
    (a1, p1, _), (a0, p0, _) = out[True], out[False]
    np.testing.assert_array_equal(a1[:, :5], a0[:, :5])
    fcheck('onoff/p', p1[:, :5], p0[:, :5], DENSITY_BOUND)
    fcheck('onoff/a', a1[:, 5:], a0[:, 5:], ACTION_BOUND)
    fcheck('onoff/density', p1[:, 5:], p0[:, 5:], DENSITY_BOUND)


def test_frequencies_follow_the_softmax_and_the_noise():
    """4 096 identical rows, draws on the device: the per-entry counts lie within 5 sigma of B p; with action_noise
    [1, 1] every row's gate opens and they lie within 5 sigma of uniform"""
    B, sizes = 4096, (3, 2)
    for noise in (None, [1., 1.]):
        agent = _learner(sizes, 0, seed=6, action_noise=noise)
        obs, pre_action, hidden = _inputs(agent, batch=1)
        torch.manual_seed(60)
        agent.noise = type(agent.noise)()
        action, prob, _ = agent.choose_action([np.repeat(obs[0], B, axis=0)], np.repeat(pre_action, B, axis=0),
                                              np.repeat(hidden, B, axis=0))
        assert _is_one_hot(action, sizes)
        np.testing.assert_allclose(prob, np.broadcast_to(prob[0], prob.shape), rtol=1e-6)
        p = prob[0].astype(np.float64) if noise is None else np.repeat(1. / np.asarray(sizes), sizes)
        counts = action.sum(0)
        sigma = np.sqrt(B * p * (1. - p))
        assert (np.abs(counts - B * p) <= 5. * sigma).all(), (counts, B * p, sigma)
        agent.close()


def _masking_plugin():
    """nn_vec_full with a policy that subclasses the stock `ModelPolicy` but has its own `forward`: the first entry of
    every branch is forbidden and the other logits are scaled (the construction of tests/test_drnd_gpu.py)"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    base = pu.plugin('nn_vec_full')

    class ModelPolicy(m.ModelPolicy):
        def forward(self, state, obs_list):
            h = self.dense(state)
            dists = []
            for head in self.d_dense_list:
                z = 3. * head(h)
                z[..., 0] = -torch.inf
                dists.append(torch.distributions.OneHotCategorical(logits=z, validate_args=False))
            return m.JointOneHotCategorical(dists), None

    ns = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if k.startswith('Model')})
    ns.ModelPolicy = ModelPolicy
    return ns


def test_a_masking_plugin_policy_acts_on_its_own_logits():
    """the launch takes the logits of the distribution the plugin's `forward` returns: over 64 rows no forbidden entry is
    chosen, its `prob` is 0, and the probabilities equal the switch-off path's"""
    from asac_amd import native
    sizes, out = (3, 2), {}
    for fused in (True, False):
        agent = _learner(sizes, 0, plugin=_masking_plugin(), seed=7, hip={FLAG: fused})
        with native.LaunchProfiler(repeat=1) as prof:
            action, prob, _ = agent.choose_action(*_inputs(agent, batch=64))
        assert _acting_calls(prof) == ({'asac_act_policy': 1} if fused else {})
        assert _is_one_hot(action, sizes) and not action[:, 0].any() and not action[:, 3].any(), 'a forbidden entry was chosen'
        assert not prob[:, 0].any() and not prob[:, 3].any() and (prob[:, 4] == 1).all()
        out[fused] = prob
        agent.close()
    np.testing.assert_allclose(out[True], out[False], rtol=1e-5, atol=1e-7)
    assert (out[True][:, 1:3] > 0).all() and out[True][:, 1].std() > 0, 'the probabilities follow the states'


def test_choose_attn_action_takes_the_launch():
    from asac_amd import native
    agent = _learner((3, 2), 0, plugin='nn_attn', seed=8, seq_encoder='ATTN', burn_in_step=4)
    rng = np.random.default_rng(8)
    n_env, T, hs = 5, 7, tuple(agent.seq_hidden_state_shape)
    pre = np.concatenate([np.eye(s, dtype=np.float32)[rng.integers(0, s, (n_env, T))] for s in (3, 2)], axis=-1)
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, state = agent.choose_attn_action(
            np.tile(np.arange(T, dtype=np.int32), (n_env, 1)), np.zeros((n_env, T), dtype=bool),
            [rng.standard_normal((n_env, T, 6)).astype(np.float32)], pre,
            rng.standard_normal((n_env, T, *hs)).astype(np.float32))
    assert _acting_calls(prof) == {'asac_act_policy': 1}
    assert action.shape == prob.shape == (n_env, 5) and _is_one_hot(action, (3, 2)) and np.isfinite(prob).all()
    np.testing.assert_allclose(prob[:, :3].sum(-1), 1., rtol=1e-6)
    agent.close()


FALLBACKS = {
    'dqn_like': dict(d=(3, 2), kw=dict(discrete_dqn_like=True)),
    'offline_action': dict(d=(3, 2), c=2, offline=True),
    'rnd_in_effect_hybrid': dict(d=(3,), c=2, plugin='nn_vec_full', kw=dict(use_rnd=True)),
    'sizes_65': dict(d=(65,)),
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_what_the_path_does_not_cover_runs_todays_code(case):
    """each of these, with the switch ON, issues no `asac_act_policy` and still acts with finite outputs"""
    from asac_amd import native
    cfg = FALLBACKS[case]
    d, c = cfg['d'], cfg.get('c', 0)
    agent = _learner(d, c, plugin=cfg.get('plugin', 'nn_vec'), hip={FLAG: True}, **cfg.get('kw', {}))
    extra = {}
    if cfg.get('offline'):
        rng = np.random.default_rng(1)
        extra['offline_action'] = np.concatenate([np.eye(s, dtype=np.float32)[rng.integers(0, s, 7)] for s in d]
                                                 + [rng.uniform(-0.9, 0.9, (7, c)).astype(np.float32)], axis=-1)
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, _ = agent.choose_action(*_inputs(agent), **extra)
    assert 'asac_act_policy' not in _acting_calls(prof)
    assert action.shape == prob.shape == (7, sum(d) + c) and np.isfinite(action).all() and np.isfinite(prob).all()
    agent.close()


def test_an_option_runs_todays_code():
    import asac_amd  # noqa: F401
    from algorithm.oc.option_base import OptionBase
    from asac_amd import native
    torch.manual_seed(0)
    opt = OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [3], 0, None, pu.plugin('nn_oc'), device='cuda:0',
                     batch_size=16, summary_path=None, n_step=3, hip_config={FLAG: True})
    dev = opt.device
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, _, _ = opt.choose_action([torch.randn(7, 6, device=dev)], torch.zeros(7, 3, device=dev),
                                               torch.zeros(7, *opt.seq_hidden_state_shape, device=dev))
    assert 'asac_act_policy' not in _acting_calls(prof)
    assert torch.isfinite(action).all() and torch.isfinite(prob).all()
    opt.close()
