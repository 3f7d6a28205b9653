"""GPU: the discrete learners' networks on the head-bank launches (`hip_config['fused_discrete_nets']`, default off;
`algorithm/fused_heads.py`, csrc/head_bank.hip): launch counts of one step, the captured step, what keeps the module code,
the widths the reference's plugins build, acting."""
import json
import random
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402
from tests.golden import make_discrete_golden, make_dqn_golden  # noqa: E402

CASES = {'discrete': make_discrete_golden, 'dqn': make_dqn_golden}
TOLERANCES = json.loads((Path(__file__).parent / 'head_bank_tolerances.json').read_text())


def _learner(case, golden_dir=None, **hip):
    """the fixture learner of tests/test_discrete_gpu.py / test_dqn_gpu.py (`f6_step_discrete`, `f6_step_dqn`: three critics
    of branches (3, 2), 32-wide heads — zero-padded tiles of 64) with the fixture's weights and episodes"""
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    mod = CASES[case]
    plugin_name, kw, d_sizes = mod.CASES[case]
    kw = dict(kw)
    convert_config_to_enum(kw)
    agent = SAC_Base(['vector'], [(6,)], list(d_sizes), 0, None, pu.plugin(plugin_name), device='cuda:0',
                     batch_size=mod.SMALL['batch_size'], replay_config={'capacity': mod.SMALL['capacity']},
                     hip_config=hip, **kw)
    if golden_dir is None:
        return agent, None
    g = np.load(golden_dir / f'f6_step_{case}.npz')
    pu.load_golden_weights(agent, g)
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    return agent, g


def _bank_calls(summary):
    """{entry point: calls} of the head-bank launches in a `LaunchProfiler.summary()` or in a {name: calls} table"""
    return {k: (v['calls'] if isinstance(v, dict) else v) for k, v in summary.items() if k.startswith('asac_head_bank_')}


# One eager step with the switch on, one row per call site: (forward launches, backward calls).
BANK_CALLS = {
    'discrete': [
        ('_train_rep_q: the E online critics on the state, with grad', 1, 1),
        ('_get_y (target): the E target critics on the window', 1, 0),
        ('_get_y (target): the policy on the window', 1, 0),
        ('_train_policy: the policy on the state, with grad', 1, 1),
        ('_train_policy: the E online critics on the state, no grad', 1, 0),
        ('_train_alpha: the policy on the state, no grad', 1, 0),
        ('_get_td_error: the E online critics on the state', 1, 0),
        ('_get_td_error -> _get_y: the E target critics and the policy on the window', 2, 0),
        ("the step's tail: the policy on the window once more (the stored mu_prob refresh)", 1, 0),
    ],
    'dqn': [
        ('_train_rep_q: the E online critics on the state, with grad', 1, 1),
        ('_dqn_target_job (loss): the E target critics on the window, the E online critics on its tail', 2, 0),
        ('_get_td_error: the E online critics on the state', 1, 0),
        ('_dqn_target_job (TD error): the E target critics on the window, the E online critics on its tail', 2, 0),
        ('_train_policy: the policy once, for the logged d_entropy', 1, 0),
    ],
}
# ... and with the switch off: every native launch of that step by name — what the step issued before the switch existed
OFF_CALLS = json.loads((Path(__file__).parent / 'head_bank_tolerances.json').read_text())['launches_with_the_switch_off']


@pytest.mark.parametrize('case', list(CASES))
def test_one_step_issues_the_bank_launches_of_the_design(golden_dir, case):
    """one eager step of the fixture learner: with the switch on, `asac_head_bank_forward` / `_backward` as often as the
    table above adds up to, and every other native launch as before; with the switch off none, and exactly the native
    launches, name by name, of the step before the switch existed"""
    from asac_amd import native
    seen = {}
    for on in (True, False):
        agent, _ = _learner(case, golden_dir, use_graph=False, fused_discrete_nets=on)
        assert (agent._q_bank is not None) == on and (agent._tq_bank is not None) == on
        torch.manual_seed(0)
        with native.LaunchProfiler(repeat=1) as prof:
            agent.train()
        seen[on] = {k: v['calls'] for k, v in prof.summary().items()}
        agent.close()
    print(case, json.dumps(seen, sort_keys=True))
    want = {'asac_head_bank_forward': sum(r[1] for r in BANK_CALLS[case]),
            'asac_head_bank_backward': sum(r[2] for r in BANK_CALLS[case])}
    assert _bank_calls(seen[True]) == want
    assert not _bank_calls(seen[False])
    assert seen[False] == OFF_CALLS[case]
    others = {k: v for k, v in seen[True].items() if not k.startswith('asac_head_bank_')}
    assert others == {k: v for k, v in OFF_CALLS[case].items()}, 'the launches around the networks stay'


def _plain_learner(d_sizes=(3, 2), seed=0, use_graph=False, hip=None, plugin='nn_vec', **kw):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(seed), np.random.seed(seed), random.seed(seed)
    return SAC_Base(['vector'], [(6,)], list(d_sizes), 0, None, pu.plugin(plugin), device='cuda:0', n_step=3,
                    batch_size=16, replay_config={'capacity': 256}, hip_config={'use_graph': use_graph, **(hip or {})}, **kw)


def _episodes(d_sizes):
    rng = np.random.default_rng(1)
    return [pu.synthetic_episode(rng, [(6,)], list(d_sizes), 0, (0,), T_) for T_ in (60, 45, 70)]


@pytest.mark.parametrize('dqn_like', [False, True])
def test_captured_step_matches_eager(dqn_like):
    """three `train()` calls with the switch on — eager, and capture + replay + replay with host work in between — leave
    the same parameters, tree and TD errors: the launches allocate nothing and synchronise nothing"""
    from asac_amd import native
    episodes = _episodes((3, 2))
    results = []
    for use_graph in (False, True):
        agent = _plain_learner(seed=3, use_graph=use_graph, hip=dict(graph_warmup=1, fused_discrete_nets=True),
                               ensemble_q_num=3, ensemble_q_sample=2, discrete_dqn_like=dqn_like)
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        launches = 0
        for i in range(3):
            if i == 0:
                with native.LaunchProfiler(repeat=1) as prof:
                    agent.train()
                launches = sum(_bank_calls(prof.summary()).values())
            else:
                agent.train()
            torch.cuda.synchronize()
            np.sort(np.random.default_rng(i).standard_normal(1 << 14))         # host work between the replays
        assert launches > 0, 'the step runs the bank launches'
        assert (agent._graph is not None) == use_graph, 'the step must capture'
        results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                        agent._td_error.cpu().numpy().copy()))
        agent.close()
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)


FALLBACKS = {
    'switch_off': dict(hip=dict(fused_discrete_nets=False), banks=0),
    # the critics keep the module code; the policy's own bank runs the policy's passes of the step (BANK_CALLS['discrete'])
    'dropout': dict(plugin='nn_vec_q_dropout', banks={'asac_head_bank_forward': 5, 'asac_head_bank_backward': 1}),
    'trunk': dict(plugin='nn_vec_trunk', banks=0),
    'width_65': dict(d=(65,), banks=0),
    # the policy keeps its code; the critics' banks run the critics' passes of the step (BANK_CALLS['discrete'])
    'own_forward': dict(plugin='nn_vec_pi_forward', banks={'asac_head_bank_forward': 5, 'asac_head_bank_backward': 1}),
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_what_the_banks_do_not_cover_runs_todays_code(case):
    """switch off; critics with `dropout=0.2`; a trunk that is not the identity; a branch of 65 logits; a policy with its
    own `forward`: the network concerned issues no `asac_head_bank_*` launch and the learner still trains.  Where no
    network is left with a bank the step issues none at all; where the other network keeps its bank (banks are attached
    per network) the step issues exactly that network's launches: the policy's five forwards and one backward of
    BANK_CALLS['discrete'] for `dropout`, the critics' five and one for `own_forward` — a network that slipped onto a bank
    would show in the count"""
    from asac_amd import native
    cfg = FALLBACKS[case]
    d = cfg.get('d', (3, 2))
    agent = _plain_learner(d, hip=cfg.get('hip', dict(fused_discrete_nets=True)), plugin=cfg.get('plugin', 'nn_vec'))
    for ep in _episodes(d):
        agent.put_episode(**ep)
    if case in ('dropout', 'switch_off', 'trunk', 'width_65'):
        assert agent._q_bank is None and agent._tq_bank is None
        assert all(getattr(q, '_head_bank', None) is None for q in agent.model_q_list + agent.model_target_q_list)
    if case != 'dropout':
        assert getattr(agent.model_policy, '_head_bank', None) is None
    before = agent._params.flat.clone()
    with native.LaunchProfiler(repeat=1) as prof:
        assert agent.train() == 1
    calls = _bank_calls(prof.summary())
    print(case, calls)
    assert calls == (cfg['banks'] or {}), calls
    q0, pi = slice(*agent._params.segments['q_0']), slice(*agent._params.segments['policy'])
    assert torch.isfinite(agent._params.flat).all() and torch.isfinite(agent._td_error).all()
    assert not torch.equal(before[q0], agent._params.flat[q0]) and not torch.equal(before[pi], agent._params.flat[pi])
    agent.close()


def test_the_widths_the_reference_plugins_use():
    """critics 128 x 2 and policy 128 x 1 (tests/plugins/nn_vec_d128.py): three steps with the switch on and off from the
    same seed; every parameter within the recorded ABSOLUTE tolerance of the switch-off path's — 4 x the largest
    difference observed on MI355X between the two paths (tests/head_bank_tolerances.json; the parameters
    reach 2.3, which is printed beside the difference)"""
    from asac_amd import native
    flats, calls = {}, {}
    for on in (True, False):
        agent = _plain_learner(seed=5, hip=dict(fused_discrete_nets=on), plugin='nn_vec_d128', ensemble_q_num=2)
        for ep in _episodes((3, 2)):
            agent.put_episode(**ep)
        torch.manual_seed(6)
        with native.LaunchProfiler(repeat=1) as prof:
            for _ in range(3):
                agent.train()
        calls[on] = _bank_calls(prof.summary())
        flats[on] = agent._params.flat.cpu().numpy().copy()
        agent.close()
    assert calls[True] and not calls[False]
    diff = float(np.abs(flats[True] - flats[False]).max())
    scale = float(np.abs(flats[False]).max())
    print(f'128-wide heads, three steps: largest parameter difference {diff:.3e} at scale {scale:.3e}')
    assert np.isfinite(flats[True]).all()
    assert diff <= TOLERANCES['nn_vec_d128_three_steps']['atol'], diff


def test_acting_issues_one_forward_in_front_of_the_acting_launch():
    """`choose_action` on a pure-discrete learner: the same one-hot actions with the switch on and off for the same draws,
    one `asac_head_bank_forward` in front of `asac_act_policy`, and the probabilities within the kernel bound of
    tests/test_head_bank_gpu.py: against the float64 branch softmax of the float64 policy stacks (tests/head_bank_ref.py)
    the switch-on path's error may be at most twice the switch-off path's, floor 4 units in the last place"""
    from asac_amd import native
    from tests import head_bank_ref as hr
    from tests.discrete_ref import over_the_bound
    rng = np.random.default_rng(3)
    obs = [rng.standard_normal((7, 6)).astype(np.float32)]
    pre_action = np.zeros((7, 5), dtype=np.float32)
    results, stacks = {}, {}
    for on in (True, False):
        agent = _plain_learner(hip=dict(fused_discrete_nets=on))
        hidden = np.zeros((7, *agent.seq_hidden_state_shape), dtype=np.float32)
        stacks[on] = [[q.detach().double().cpu().numpy() for q in m.parameters()] for m in agent.model_policy.d_dense_list]
        torch.manual_seed(9)
        with native.LaunchProfiler(repeat=1) as prof:
            results[on] = agent.choose_action(obs, pre_action, hidden)
        seen = {k: v['calls'] for k, v in prof.summary().items()}
        assert seen.get('asac_act_policy') == 1, seen
        assert _bank_calls(seen) == ({'asac_head_bank_forward': 1} if on else {}), seen
        agent.close()
    (a_on, p_on, _), (a_off, p_off, _) = results[True], results[False]
    assert np.array_equal(a_on, a_off)
    assert all(np.array_equal(a, b) for x, y in zip(stacks[True], stacks[False]) for a, b in zip(x, y)), 'one seed, one policy'
    # the stock plugin's state IS the vector observation (ModelSimpleRep); LinearLayers(6, 64, 3, size) per branch
    logits = hr.bank_forward(obs[0].astype(np.float64), stacks[False], hr.residual_flags(6, 64, 3), (3, 2), 1)[0]
    want = []
    for z in np.split(logits, [3], axis=1):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        want.append(e / e.sum(axis=1, keepdims=True))
    bad, _ = over_the_bound('acting', {'prob': np.concatenate(want, axis=1)}, {'prob': p_on.astype(np.float64)},
                            {'prob': p_off.astype(np.float64)})
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# the recorded reference steps
# ------------------------------------------------------------------------------------------------
ULP = 2.0 ** -23
FIXTURES = ['discrete', 'discrete_is', 'dqn', 'hybrid']


def _fixture_learner(case, golden_dir, **hip):
    """the learner of `f6_step_<case>` (a hooked subclass, tests/parity_utils.py) with the fixture's weights and episodes,
    and the observables with the call-site defaults the case's own test file holds it to"""
    import asac_amd  # noqa: F401
    from algorithm.utils.enums import convert_config_to_enum
    from tests import test_discrete_gpu, test_dqn_gpu, test_hybrid_gpu
    if case == 'hybrid':
        plugin_name, kw, d_sizes, io = pu.STEP_CASES['hybrid']
        observables = test_hybrid_gpu.OBSERVABLES
    else:
        mod = make_dqn_golden if case == 'dqn' else make_discrete_golden
        plugin_name, kw, d_sizes = mod.CASES[case]
        io = dict(obs_names=['vector'], obs_shapes=[(6,)], c_action_size=0, batch_size=mod.SMALL['batch_size'],
                  capacity=mod.SMALL['capacity'])
        observables = test_dqn_gpu.OBSERVABLES if case == 'dqn' else test_discrete_gpu.OBSERVABLES
    kw = dict(kw)
    convert_config_to_enum(kw)
    agent = pu.hooked_learner()(io['obs_names'], io['obs_shapes'], list(d_sizes), io['c_action_size'], None,
                                pu.plugin(plugin_name), device='cuda:0', batch_size=io['batch_size'],
                                replay_config={'capacity': io['capacity']}, hip_config=hip, **kw)
    g = np.load(golden_dir / f'f6_step_{case}.npz')
    pu.load_golden_weights(agent, g)
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    return agent, g, observables


def _gradient_error(agent, g):
    """the first step's gradients against the reference's (Adam's first moment, `pu.assert_first_step_gradients`): the worst
    entry error relative to its tensor's largest entry (or the optimizer's rounding floor, for analytically zero tensors)"""
    moments, opt_scale, worst = pu.product_first_moments(agent), pu._optimizer_scales(g), 0.
    for key in g.files:
        if key.startswith('g0/'):
            _, oname, j = key.split('/')
            want = g[key]
            err = np.abs(moments[oname][int(j)].cpu().numpy().astype(np.float64) - want)
            worst = max(worst, float(err.max()) / max(float(np.abs(want).max()), pu.ZERO_GRAD_REL * opt_scale[oname], 1e-300))
    return worst


def _weight_error(mods, g):
    """the weights after the steps against the reference's: the worst entry error relative to its tensor's largest entry,
    over the entries `pu.assert_weights_close` holds strictly (an entry whose reference gradient is at rounding level moves
    by +- lr with a device-dependent sign in both paths)"""
    zero, worst = set(pu.zero_gradient_tensors(g, mods)), 0.
    for name, mod in mods.items():
        params = [k for k, _ in mod.named_parameters()]
        oname = pu.OPTIMIZER_OF.get(name) or ('optimizer_q_' + name.rsplit('_', 1)[1] if name.startswith('model_q_') else None)
        for k, v in mod.state_dict().items():
            key, gkey = f'w1/{name}/{k}', (f'g0/{oname}/{params.index(k)}' if oname is not None and k in params else None)
            if key not in g.files or f'{name}/{k}' in zero:
                continue
            want = g[key]
            strict = np.ones(want.shape, dtype=bool)
            if gkey is not None and gkey in g.files:
                g0 = np.abs(g[gkey])
                strict = g0 >= 1e-3 * max(float(g0.max()), 1e-30)
            if strict.any():
                err = np.abs(v.detach().cpu().numpy().astype(np.float64) - want)
                worst = max(worst, float(err[strict].max()) / max(float(np.abs(want).max()), 1e-300))
    return worst


def _run_fixture(case, golden_dir, on):
    """the fixture's steps through the learner its defaults build, with the switch `on` or off -> ({observable: (|error|,
    scale)}: step 0's observables, the first step's gradients, the weights after the steps; [what missed the call-site
    defaults])"""
    from algorithm.fused import RecordedNoise
    from asac_amd import native
    agent, g, observables = _fixture_learner(case, golden_dir, use_graph=False, fused_discrete_nets=on)
    rb = agent.replay_buffer
    mods = {name: m for name, m in agent.ckpt_dict.items() if isinstance(m, torch.nn.Module)}
    n_steps = int(g['n_steps'])
    step_box, failures, errors = [0], [], {}

    def soft(fn, what):
        try:
            fn()
        except AssertionError as e:
            failures.append(f'{what}: {" ".join(str(e).split())[:300]}')

    def align_with_reference():     # see tests/test_sac_step_gpu.py: compare the fresh update, then align
        s = step_box[0]
        soft(lambda: pu.assert_weights_close(mods, g, 1, 3e-4, rtol=1e-3, atol=2e-5, prefix=f'step{s}/w_rq'), f'step {s} w_rq')
        pu.load_golden_weights(agent, g, prefix=f'step{s}/w_rq')

    if 'step0/w_rq/model_q_0/' + next(iter(agent.model_q_list[0].state_dict())) in g.files:
        agent.after_rep_q_update = align_with_reference
    for s in range(n_steps):
        step_box[0] = s
        n_eps = int(g[f'step{s}/n_eps']) if f'step{s}/n_eps' in g.files else 0
        agent.noise = RecordedNoise([g[f'step{s}/u']], [g[f'step{s}/eps{j}'] for j in range(n_eps)], list(g[f'step{s}/perm']))
        rb.uniform_source = agent.noise
        with native.LaunchProfiler(repeat=1) as prof:
            assert agent.train() == s + 1
        assert (sum(_bank_calls(prof.summary()).values()) > 0) == on
        assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
        assert np.array_equal(rb._ids.cpu().numpy(), g[f'step{s}/sample_ids']), f'step {s}: PER index selection'
        for name, tol in observables.items():
            if name == 'td_error':
                got = agent._td_error.cpu().numpy()[:, None]
            elif name == 'tree':
                got = rb._tree.cpu().numpy()
            elif name.startswith('log_'):
                got = getattr(agent, name).item()
            else:
                got = agent._stats[name].item()
            want = g[f'step{s}/{name}']
            err = np.abs(np.asarray(got, dtype=np.float64) - want)
            if s == 0:
                errors[name] = (float(err.max()), float(np.abs(want).max()))
            soft(lambda: np.testing.assert_allclose(got, want, err_msg=name, **tol), f'step {s} {name}')
        if s == 0:
            errors['gradients'] = (_gradient_error(agent, g), 1.)
            soft(lambda: pu.assert_first_step_gradients(agent, g, rtol=2e-3, atol_frac=5e-5), 'first-step gradients')
    errors['weights'] = (_weight_error(mods, g), 1.)
    soft(lambda: pu.assert_weights_close(mods, g, n_steps, 3e-4, rtol=1e-3, atol=2e-5), 'weights')
    rb.check_health()
    agent.close()
    return errors, failures


@pytest.mark.parametrize('case', FIXTURES)
def test_step_against_the_reference_fixture(golden_dir, case):
    """The recorded reference steps (`f6_step_discrete`, `_discrete_is`, `_dqn`, `_hybrid`) through the learner its defaults
    build, with `RecordedNoise`, as tests/test_dqn_gpu.py::test_step_against_the_reference_fixture runs them: PER ids
    bit-exact, every recorded draw consumed.  With the switch on and off: the case's observables (its own test file's
    table), the first step's gradients and the weights after the steps under that file's call-site defaults — the switch-off
    path must meet them by itself.  Each observable's error against the recorded reference under the switch (step 0's
    observables; the gradients and the weights relative to their tensor's largest entry) may be at most twice that of the
    switch-off path, floor 4 units in the last place.  The hybrid learner (a bank beside `c_dense` in each critic, the
    policy's split path) and the importance-sampling learner run the switch here.  Largest share of the bound observed on
    MI355X: NOTES.md, "Discrete-nets round"."""
    on_err, on_failures = _run_fixture(case, golden_dir, True)
    off_err, off_failures = _run_fixture(case, golden_dir, False)
    bad, share = [], 0.
    for name in on_err:
        (e_on, scale), (e_off, _) = on_err[name], off_err[name]
        floor = 4 * ULP * scale
        bound = max(2 * e_off, floor)
        share = max(share, e_on / bound)
        print(f'{case} {name}: switch on {e_on:.3e}  switch off {e_off:.3e}  floor {floor:.3e}  share {e_on / bound:.2f}')
        if e_on > bound:
            bad.append((name, e_on, e_off, floor))
    print(f'{case}: largest share of the bound {share:.2f}')
    assert not off_failures, ('the switch-off path misses its own defaults', off_failures)
    assert not on_failures, on_failures
    assert not bad, bad
