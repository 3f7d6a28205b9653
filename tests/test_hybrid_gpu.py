"""GPU: the policy-based learner on a hybrid action space on the native path (`hip_config['fused_hybrid']`,
csrc/hybrid.hip): the four `asac_hybrid_*` kernels against float64 and against the float32 eager composition, the bits they
share with the single-head launches, the recorded reference steps (`tests/golden/f6_step_hybrid.npz`) through the learner
with and without the launches, launch counts, the captured step, the fallbacks and the refused arguments."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import discrete_ref as dr  # noqa: E402
from tests import hybrid_ref as hr  # noqa: E402
from tests import parity_utils as pu  # noqa: E402

ULP = 2.0 ** -23
MAX_ACTION = 64     # ASAC_MAX_ACTION
# (B, n, branches, A): a single row; two branches; rows that do not fill a workgroup and A = 5 (past vtrace_step_load's
# A <= 4 path); a long window, three branches; more rows than one pass of 256 lanes; the width limits
SHAPES = [(1, 1, (2,), 1), (5, 3, (3, 2), 2), (37, 4, (4,), 5), (16, 40, (3, 2, 5), 2), (300, 2, (17,), 1),
          (3, 1, (64,), MAX_ACTION)]
ENSEMBLES = [(1, 1), (2, 2), (3, 2), (6, 5)]        # E_sample = 5: past vtrace_step_load's E_sample <= 4 path
EXCLUDED = ('asac_vtrace_return_direct', 'asac_vtrace_return_min', 'asac_q_loss_fwd_bwd', 'asac_policy_loss_fwd_bwd',
            'asac_alpha_grad')


def _common_args(c, y_out):
    from asac_amd import native
    a = native.VtraceArgs()
    a.reward, a.reward_stride = c['reward'].data_ptr(), c['reward'].stride(0)
    a.done, a.last_mask, a.padding_mask = c['done'].data_ptr(), c['last'].data_ptr(), c['pad'].data_ptr()
    assert c['done'].stride(0) == c['last'].stride(0) == c['pad'].stride(0)
    a.mask_stride = c['done'].stride(0)
    a.gamma_ratio, a.lambda_ratio = c['gamma_ratio'].data_ptr(), c['lambda_ratio'].data_ptr()
    a.gamma, a.v_rho, a.v_c = c['gamma'], c['v_rho'], c['v_c']
    a.use_n_step_is, a.B, a.n = int(c['use_is']), c['B'], c['n']
    a.E_sample = c['Es']
    if c['use_is']:
        a.mu_prob, a.mu_stride_b, a.mu_stride_t = c['mu_full'].data_ptr(), c['mu_full'].stride(0), c['mu_full'].stride(1)
    a.y_out = y_out.data_ptr()
    return a


def _d_args(c, y_out):
    a = _common_args(c, y_out)
    a.subset_n, a.subset_next, a.log_alpha = c['sub_n'].data_ptr(), c['sub_next'].data_ptr(), c['log_alpha'].data_ptr()
    return a


def _c_args(c, y_out):
    a = _common_args(c, y_out)
    q = c['cq_target']
    a.q, a.q_stride_e, a.q_stride_b, a.q_stride_t = q.data_ptr(), q.stride(0), q.stride(1), q.stride(2)
    a.subset_n, a.subset_next = c['sub_cn'].data_ptr(), c['sub_cnext'].data_ptr()
    a.logp, a.log_alpha = c['logp_w'].data_ptr(), c['log_c_alpha'].data_ptr()
    a.A, a.mu_offset = c['A'], c['D']
    if c['use_is']:
        a.pi_prob, a.pi_stride_b, a.pi_stride_t = c['c_pi'].data_ptr(), c['c_pi'].stride(0), c['c_pi'].stride(1)
    return a


def _device_case(c):
    """the case as strided float32 device views, plus what the learner's sampling launches hand on: log pi of the window's
    sample and pi(stored continuous actions) (`asac_squash_sample_fwd`), log pi of the temperature step's sample"""
    from asac_amd import native
    d = hr.to(c, torch.float32, 'cuda', strided=True)
    B, n, A, D = c['B'], c['n'], c['A'], c['D']
    assert d['logits'].stride(1) == D + 5 and d['action_full'].stride(1) == D + A + 5 and d['done'].stride(0) == n + 2
    f32 = dict(dtype=torch.float32, device='cuda')
    d['logp_w'], d['c_pi'] = torch.empty(B, n + 1, **f32), torch.empty(B, n + 1, A, **f32)
    native.squash_sample_fwd(d['loc_w'], d['scale_w'], d['eps_w'], torch.empty(B, n + 1, A, **f32), d['logp_w'],
                             action=d['action_full'], action_offset=D, prob_out=d['c_pi'])
    d['logp0'] = torch.empty(B, **f32)
    native.squash_sample_fwd(d['loc0'], d['scale0'], d['eps0'], torch.empty(B, A, **f32), d['logp0'])
    return d


def _outputs(c, alloc=None):
    B, D, E = c['B'], c['D'], c['E']
    nan = alloc or (lambda *shape: torch.full(shape, float('nan'), device='cuda'))
    return {'d_y': nan(B), 'c_y': nan(B), 'td': nan(B), 'loss_q': nan(E), 'grad_qd': nan(E, B, D), 'grad_cq': nan(E, B),
            'loss_policy': nan(), 'grad_logits': nan(B, D), 'grad_logp': nan(B), 'grad_cq_pi': nan(E, B), 'd_entropy': nan(),
            'c_entropy': nan(), 'grad_alpha': nan(2)}


def _kernels(c, alloc=None):
    """the four launches on the case's (strided, device) tensors, outputs pre-filled with NaN (`alloc`: another allocator
    of NaN-filled outputs, `discrete_ref.Guarded`) -> {name: tensor}"""
    from asac_amd import native
    br, out = native.branches(c['sizes']), _outputs(c, alloc)
    native.hybrid_return(_d_args(c, out['d_y']), _c_args(c, out['c_y']), br, c['q_target'], c['logits'],
                         action=c['action_full'], q_online=c['q_online'], c_q_online=c['c_q_online'], td_out=out['td'])
    native.hybrid_q_loss_grad(br, c['q_online'], c['action_full'][:, 0], c['c_q_online'], c['c_t_q'], c['y'], c['c_y'],
                              c['w'], c['clip_eps'], out['loss_q'], out['grad_qd'], out['grad_cq'])
    native.hybrid_policy_loss_grad(br, c['logits0'], c['q_online'], c['sub_pi'], c['mu0'], c['log_alpha'], c['penalty'],
                                   c['logp0'], c['c_q_pi'], c['sub_pi_c'], c['Es'], c['log_c_alpha'], c['scale0'],
                                   out['loss_policy'], out['grad_logits'], out['grad_logp'], out['grad_cq_pi'],
                                   out['d_entropy'], out['c_entropy'])
    native.hybrid_alpha_grad(br, c['logits0'], c['target'], c['logp0'], c['target_c'], out['grad_alpha'])
    return out


def _eager(c):
    """today's float32 code on the same device and inputs: the discrete V as torch ops and the scan through
    `asac_vtrace_return_direct`, the continuous return through `asac_vtrace_return_min`, the rest as torch ops"""
    from asac_amd import native
    v_n, v_next, pi, mu = dr.values(c)
    d_y, c_y = torch.empty(c['B'], device='cuda'), torch.empty(c['B'], device='cuda')
    cont = lambda t: None if t is None else t.contiguous()      # noqa: E731
    native.vtrace_return_direct(_d_args(c, d_y), v_n.contiguous(), v_next.contiguous(), cont(pi), cont(mu))
    native.vtrace_return_min(_c_args(c, c_y))
    out = {'d_y': d_y, 'c_y': c_y, 'td': hr.td_error(c, d_y, c_y)}
    for f in (hr.q_loss, hr.policy_loss, hr.alpha_grad):
        out.update(f(c))
    return out


def _compare(tag, c, alloc=None):
    """kernel and eager float32 against float64 -> [(tensor, kernel error, eager error, floor)] of the tensors over the
    bound (`discrete_ref.over_the_bound`); prints every figure"""
    want = dr.as_numpy(hr.all_formulas(hr.to(c, torch.float64, 'cpu')))
    dev = _device_case(c)
    kernel, eager = dr.as_numpy(_kernels(dev, alloc)), dr.as_numpy(_eager(dev))
    return dr.over_the_bound(tag, want, kernel, eager)[0]


@pytest.mark.parametrize('use_is', [False, True], ids=['plain', 'is'])
@pytest.mark.parametrize('E,Es', ENSEMBLES)
@pytest.mark.parametrize('B,n,sizes,A', SHAPES)
def test_kernels_against_float64_and_the_eager_composition(B, n, sizes, A, E, Es, use_is):
    """The four entry points on strided views, outputs pre-filled with NaN, against the float64 restatement of the
    oracle's formulas (tests/hybrid_ref.py; tests/test_hybrid_host.py pins it to the oracle).  Planted rows: `make_case`.
    Bound (the rule of tests/test_discrete_gpu.py): per tensor the kernel's largest absolute error against float64 may be
    at most twice that of the float32 eager composition — today's code on the same device and inputs — against the same
    float64 values, with a floor of 4 units in the last place at the tensor's largest magnitude.  Both pipelines take log
    pi of the samples and pi(stored continuous actions) from the learner's sampling launch; float64 forms them itself.  With
    and without IS weights.  Observed on MI355X: DESIGN.md section 5."""
    import asac_amd  # noqa: F401
    bad = []
    for weights in (False, True):
        c = hr.make_case(B, n, sizes, A, E, Es, use_is, weights, seed=B + 7 * n + len(sizes) + E)
        bad += _compare(f'{(B, n, sizes, A)} E {E}/{Es} is={use_is} w={weights}', c)
    assert not bad, bad


def test_the_planted_rows_are_what_they_claim():
    """on the (5, 3, (3, 2), 2) case in float64: both sides of +-eps and the inside occur among `cq - tq`, the stored
    continuous action sits at +-1, a behaviour probability is 0, and the policy step's first two critics tie"""
    c = hr.to(hr.make_case(5, 3, (3, 2), 2, 3, 2, True, True, seed=1), torch.float64, 'cpu')
    delta = c['c_q_online'] - c['c_t_q']
    assert bool((delta > c['clip_eps']).any()) and bool((delta < -c['clip_eps']).any()) and bool((delta.abs() < c['clip_eps']).any())
    assert float(c['action_full'][3, 0, c['D']:].min()) == 1. and float(c['action_full'][3, 2, c['D']:].max()) == -1.
    assert float((c['mu_full'][4, 0, :c['D']] * c['action'][4, 0]).sum()) == 0. and float(c['mu_full'][4, 2, c['D']]) == 0.
    assert float(c['c_q_pi'][0, 4]) == float(c['c_q_pi'][1, 4]) == float(c['c_q_pi'][:, 4].min())
    assert bool(c['pad'][0].all()) and bool(c['done'][1, 0]) and float(c['action'][2, 0].abs().sum()) == 0.


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_is', [False, True], ids=['plain', 'is'])
@pytest.mark.parametrize('B,n,sizes,A,E,Es', [(5, 3, (3, 2), 2, 3, 2), (37, 4, (4,), 5, 6, 5), (16, 40, (3, 2, 5), 2, 2, 2),
                                              (300, 2, (17,), 1, 1, 1)])
def test_the_launches_share_the_single_head_launches_bits(B, n, sizes, A, E, Es, use_is):
    """on the same inputs: d_y is `asac_discrete_return`'s, c_y `asac_vtrace_return_min`'s, the two temperature slots
    `asac_discrete_alpha_grad`'s and `asac_alpha_grad`'s, the policy launch's grad_cq / grad_logp
    `asac_policy_loss_fwd_bwd`'s, the Q launch's grad_cq `asac_q_loss_fwd_bwd`'s, the policy launch's grad_logits /
    d_entropy `asac_discrete_policy_loss_grad`'s and the Q launch's grad_qd `asac_discrete_q_loss_grad`'s — bit for bit"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    c = _device_case(hr.make_case(B, n, sizes, A, E, Es, use_is, True, seed=B + n))
    got, br = _kernels(c), native.branches(sizes)
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')      # noqa: E731
    d_y, c_y = nan(B), nan(B)
    native.discrete_return(_d_args(c, d_y), br, c['q_target'], c['logits'], action=c['action_full'])
    native.vtrace_return_min(_c_args(c, c_y))
    assert torch.isfinite(d_y).all() and torch.equal(got['d_y'], d_y)
    assert torch.isfinite(c_y).all() and torch.equal(got['c_y'], c_y)
    slot_d, slot_c = nan(1), nan(1)
    native.discrete_alpha_grad(br, c['logits0'], c['target'], slot_d)
    native.alpha_grad(c['logp0'], c['target_c'], slot_c)
    assert torch.equal(got['grad_alpha'], torch.cat([slot_d, slot_c]))
    grad_logp, grad_cq = nan(B), nan(E, B)
    native.policy_loss_fwd_bwd(c['logp0'], c['c_q_pi'], c['sub_pi_c'], Es, c['log_c_alpha'], c['scale0'], nan(1), grad_logp,
                               grad_cq, nan(1))
    assert torch.equal(got['grad_logp'], grad_logp) and torch.equal(got['grad_cq_pi'], grad_cq)
    grad_q = nan(E, B)
    native.q_loss_fwd_bwd(c['c_q_online'], c['c_t_q'], c['c_y'].reshape(-1).contiguous(), c['w'].reshape(-1).contiguous(),
                          c['clip_eps'], nan(E), grad_q)
    assert torch.isfinite(grad_q).all() and torch.equal(got['grad_cq'], grad_q)
    # the discrete rows (csrc/asac_discrete_rows.h): the policy launch's grad_logits and d_entropy against
    # `asac_discrete_policy_loss_grad`, the Q launch's grad_qd against `asac_discrete_q_loss_grad`.  (c_entropy is not
    # `asac_policy_loss_fwd_bwd`'s: one divides by B, the other multiplies by 1 / B.)
    grad_logits, d_entropy = nan(B, c['D']), nan(1)
    native.discrete_policy_loss_grad(br, c['logits0'], c['q_online'], c['sub_pi'], Es, c['mu0'], c['log_alpha'],
                                     c['penalty'], nan(1), grad_logits, d_entropy)
    assert torch.isfinite(grad_logits).all() and torch.equal(got['grad_logits'], grad_logits)
    assert torch.isfinite(d_entropy).all() and torch.equal(got['d_entropy'].reshape(1), d_entropy)
    grad_qd = nan(E, B, c['D'])
    native.discrete_q_loss_grad(br, c['q_online'], c['action_full'][:, 0], c['y'], c['w'], nan(E), grad_qd)
    assert torch.isfinite(grad_qd).all() and torch.equal(got['grad_qd'], grad_qd)


# ------------------------------------------------------------------------------------------------
# the step
# ------------------------------------------------------------------------------------------------
def _hybrid_calls(summary):
    return {k: v['calls'] for k, v in summary.items() if k.startswith('asac_hybrid_')}


ONE_STEP = {'asac_hybrid_return': 2, 'asac_hybrid_q_loss_grad': 1, 'asac_hybrid_policy_loss_grad': 1,
            'asac_hybrid_alpha_grad': 1}


def _golden_learner(golden_dir, **hip):
    """the `hybrid` case of `pu.STEP_CASES` with the fixture's weights and episodes -> (agent, fixture)"""
    import asac_amd  # noqa: F401
    from algorithm.utils.enums import convert_config_to_enum
    plugin_name, kw, d_sizes, io = pu.STEP_CASES['hybrid']
    kw = dict(kw)
    convert_config_to_enum(kw)
    agent = pu.hooked_learner()(io['obs_names'], io['obs_shapes'], list(d_sizes), io['c_action_size'], None,
                                pu.plugin(plugin_name), device='cuda:0', batch_size=io['batch_size'],
                                replay_config={'capacity': io['capacity']}, hip_config=hip, **kw)
    g = np.load(golden_dir / 'f6_step_hybrid.npz')
    pu.load_golden_weights(agent, g)
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    return agent, g


# the call-site defaults of tests/test_discrete_gpu.py; c_entropy on d_entropy's terms, log_c_alpha on log_d_alpha's
OBSERVABLES = {'loss_q': dict(rtol=2e-4, atol=0.), 'loss_policy': dict(rtol=2e-4, atol=2e-5),
               'd_entropy': dict(rtol=2e-4, atol=2e-5), 'c_entropy': dict(rtol=2e-4, atol=2e-5),
               'td_error': dict(rtol=2e-4, atol=2e-5), 'tree': dict(rtol=2e-4, atol=1e-6),
               'log_c_alpha': dict(rtol=2e-4, atol=2e-5)}


def _run_fixture(golden_dir, fused):
    """the fixture's steps through the learner -> ({observable: (|error|, scale) of step 0}, [failures])"""
    from algorithm.fused import RecordedNoise
    from asac_amd import native
    agent, g = _golden_learner(golden_dir, use_graph=False, fused_hybrid=fused)
    rb = agent.replay_buffer
    mods = {name: m for name, m in agent.ckpt_dict.items() if isinstance(m, torch.nn.Module)}
    n_steps = int(g['n_steps'])
    failures, errors0 = [], {}

    def soft(fn, what):
        try:
            fn()
        except AssertionError as e:
            failures.append(f'{what}: {" ".join(str(e).split())[:300]}')

    for s in range(n_steps):
        eps = [g[f'step{s}/eps{j}'] for j in range(int(g[f'step{s}/n_eps']))]
        agent.noise = RecordedNoise([g[f'step{s}/u']], eps, list(g[f'step{s}/perm']))
        rb.uniform_source = agent.noise
        with native.LaunchProfiler(repeat=1) as prof:
            assert agent.train() == s + 1
        seen = prof.summary()
        assert _hybrid_calls(seen) == (ONE_STEP if fused else {}), _hybrid_calls(seen)
        assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
        assert np.array_equal(rb._ids.cpu().numpy(), g[f'step{s}/sample_ids']), f'step {s}: PER index selection'
        got = {'loss_q': agent._stats['loss_q'].item(), 'loss_policy': agent._stats['loss_policy'].item(),
               'd_entropy': agent._stats['d_entropy'].item(), 'c_entropy': agent._stats['c_entropy'].item(),
               'td_error': agent._td_error.cpu().numpy()[:, None], 'tree': rb._tree.cpu().numpy(),
               'log_c_alpha': agent.log_c_alpha.item()}
        for name, tol in OBSERVABLES.items():
            want = g[f'step{s}/{name}']
            err = np.abs(np.asarray(got[name], dtype=np.float64) - want)
            print(f'hybrid fused={fused} step {s} {name}: max error {float(err.max()):.3e} at scale {float(np.abs(want).max()):.3e}')
            if s == 0:
                errors0[name] = (float(err.max()), float(np.abs(want).max()))
            soft(lambda: np.testing.assert_allclose(got[name], want, err_msg=name, **tol), f'step {s} {name}')
        if s == 0:
            soft(lambda: pu.assert_first_step_gradients(agent, g, rtol=2e-3, atol_frac=5e-5), 'first-step gradients')
    soft(lambda: pu.assert_weights_close(mods, g, n_steps, 3e-4, rtol=1e-3, atol=2e-5), 'weights')
    rb.check_health()
    agent.close()
    return errors0, failures


def test_step_against_the_reference_fixture(golden_dir):
    """The recorded reference steps of the `hybrid` case through `SAC_Base(..., hip_config={'use_graph': False,
    'fused_hybrid': ...})` with `RecordedNoise`: PER ids bit-exact, every recorded draw consumed, exactly the five launches a
    step; loss_q, loss_policy, d_entropy, c_entropy, td_error, tree and log_c_alpha, the first step's gradients and the
    weights after the steps under the call-site defaults of tests/test_discrete_gpu.py.  The same steps run with the
    switch off; for step 0 each observable's error against the fixture under the launches may be at most twice that of
    the eager path, floor 4 units in the last place at the observable's largest magnitude.  The eager run must pass its own
    defaults: otherwise the test says so rather than blaming the launches."""
    fused_err, fused_failures = _run_fixture(golden_dir, True)
    eager_err, eager_failures = _run_fixture(golden_dir, False)
    bad = []
    for name in OBSERVABLES:
        (e_f, scale), (e_e, _) = fused_err[name], eager_err[name]
        floor = 4 * ULP * scale
        print(f'hybrid step 0 {name}: fused {e_f:.3e}  eager {e_e:.3e}  floor {floor:.3e}')
        if e_f > max(2 * e_e, floor):
            bad.append((name, e_f, e_e, floor))
    assert not eager_failures, ('the eager hybrid path misses its own defaults', eager_failures)
    assert not fused_failures, fused_failures
    assert not bad, bad


def test_one_step_issues_one_launch_per_item(golden_dir):
    """one eager step with the switch on: two returns (target and TD error), one launch per loss and for the temperatures,
    and none of the launches they replace"""
    from asac_amd import native
    agent, _ = _golden_learner(golden_dir, use_graph=False, fused_hybrid=True)
    torch.manual_seed(0)
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    seen = prof.summary()
    agent.close()
    assert _hybrid_calls(seen) == ONE_STEP
    assert not [k for k in seen if k in EXCLUDED or k.startswith('asac_discrete_')], sorted(seen)


def _episodes(d_sizes, c_size, hidden=(0,)):
    rng = np.random.default_rng(1)
    return [pu.synthetic_episode(rng, [(6,)], list(d_sizes), c_size, hidden, T_) for T_ in (60, 45, 70)]


def test_captured_step_matches_eager():
    """the pattern of tests/test_discrete_gpu.py::test_captured_step_matches_eager: three `train()` calls — eager, and
    capture + replay + replay with host work in between — leave the same parameters, tree and TD errors (the hybrid
    launches allocate nothing and synchronise nothing, so they are nodes of the step's graph)"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.sac_base import SAC_Base
    episodes = _episodes((3, 2), 2)
    results = []
    for use_graph in (False, True):
        torch.manual_seed(3), np.random.seed(3), random.seed(3)
        agent = SAC_Base(['vector'], [(6,)], [3, 2], 2, None, pu.plugin('nn_vec'), device='cuda:0', n_step=3,
                         ensemble_q_num=3, ensemble_q_sample=2, batch_size=16, replay_config={'capacity': 256},
                         hip_config={'use_graph': use_graph, 'graph_warmup': 1, 'fused_hybrid': True})
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        launches = 0
        for i in range(3):
            if i == 0:
                with native.LaunchProfiler(repeat=1) as prof:
                    agent.train()
                launches = sum(_hybrid_calls(prof.summary()).values())
            else:
                agent.train()
            torch.cuda.synchronize()
            np.sort(np.random.default_rng(i).standard_normal(1 << 14))         # host work between the replays
        assert launches == 5, 'the step runs the one-launch hybrid arithmetic'
        assert (agent._graph is not None) == use_graph, 'the hybrid step must capture'
        results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                        agent._td_error.cpu().numpy().copy()))
        agent.close()
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)


ON = dict(fused_hybrid=True)
FALLBACKS = {
    'default': dict(d=(3, 2), c=2, hip={}),
    'dqn_like': dict(d=(3, 2), c=2, hip=ON, kw=dict(discrete_dqn_like=True)),
    'offline_loss': dict(d=(3, 2), c=2, hip=ON, kw=dict(offline_enabled=True, offline_loss=True)),
    'clip_epsilon_0': dict(d=(3, 2), c=2, hip=ON, kw=dict(clip_epsilon=0.)),
    'width_65': dict(d=(65,), c=2, hip=ON),
    'nine_branches': dict(d=(2,) * 9, c=2, hip=ON),
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_what_the_path_does_not_cover_runs_todays_code(case):
    """each of these issues no `asac_hybrid_*` launch and still trains"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.sac_base import SAC_Base
    cfg = FALLBACKS[case]
    torch.manual_seed(0)
    agent = SAC_Base(['vector'], [(6,)], list(cfg['d']), cfg['c'], None, pu.plugin('nn_vec'), device='cuda:0', n_step=3,
                     batch_size=16, replay_config={'capacity': 256}, hip_config={'use_graph': False, **cfg['hip']},
                     **cfg.get('kw', {}))
    assert agent._fused_hybrid is bool(cfg['hip'])
    for ep in _episodes(cfg['d'], cfg['c']):
        agent.put_episode(**ep)
    before = agent._params.flat.clone()
    with native.LaunchProfiler(repeat=1) as prof:
        assert agent.train() == 1
    assert not _hybrid_calls(prof.summary())
    q0 = slice(*agent._params.segments['q_0'])
    assert torch.isfinite(agent._params.flat).all() and not torch.equal(before[q0], agent._params.flat[q0])
    assert torch.isfinite(agent._td_error).all()
    agent.close()


def test_an_option_runs_todays_code():
    """an `OptionBase` with the switch on: its policy and temperature steps (the parent's `_train_policy` /
    `_train_alpha`) issue no `asac_hybrid_*` launch and still train"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.oc import OptionBase
    torch.manual_seed(0)
    B, n, D, A = 16, 3, 5, 2
    opt = OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [3, 2], A, None, pu.plugin('nn_oc_small'),
                     device='cuda:0', batch_size=B, summary_path=None, n_step=n, hip_config={'fused_hybrid': True})
    assert opt._fused_hybrid is True and not opt._hybrid_fused(B)
    gen = torch.Generator().manual_seed(1)
    ep = pu.synthetic_episode(np.random.default_rng(2), [(6,)], [3, 2], A, (0,), B * n)
    actions = torch.from_numpy(ep['ep_actions']).view(B, n, D + A).cuda()
    obs = torch.randn(B, n, 6, generator=gen).cuda()
    states = torch.randn(B, n + 1, opt.state_size, generator=gen).cuda()
    mu = torch.rand(B, n, D + A, generator=gen).cuda()
    seg = slice(*opt._params.segments['policy'])
    before = opt._params.flat[seg].clone()
    with native.LaunchProfiler(repeat=1) as prof:
        opt.train_policy_alpha(torch.zeros(B, n, dtype=torch.bool, device='cuda'), [obs], states, actions, mu)
    assert not _hybrid_calls(prof.summary())
    assert torch.isfinite(opt._params.flat).all() and not torch.equal(before, opt._params.flat[seg])
    opt.close()


# ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    """mismatched B or n between the two blocks, `td_error_out` inside a block, a branch table that does not add up,
    E_sample > E, clip_eps <= 0, B = 1025 for the three single-workgroup launches, A = 0: hipErrorInvalidValue and no
    launch"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    B, n, sizes, A, E = 8, 3, (3, 2), 2, 2
    c = _device_case(hr.make_case(B, n, sizes, A, E, E, True, True, seed=5))
    D = c['D']
    lib, s, bad = native.load(), native._stream(), 1      # hipErrorInvalidValue
    marker = lambda *shape: torch.full(shape, 7., device='cuda')      # noqa: E731
    d_y, c_y, td, loss_q, grad_qd, grad_cq = marker(B), marker(B), marker(B), marker(E), marker(E, B, D), marker(E, B)
    loss_pi, grad_z, grad_lp, grad_cq_pi, d_ent, c_ent, slots = (marker(1), marker(B, D), marker(B), marker(E, B), marker(1),
                                                                 marker(1), marker(2))
    outputs = (d_y, c_y, td, loss_q, grad_qd, grad_cq, loss_pi, grad_z, grad_lp, grad_cq_pi, d_ent, c_ent, slots)
    p = native._p

    def job(sizes_=sizes):
        j = native._discrete_return_job(_d_args(c, d_y), native.branches(sizes), c['q_target'], c['logits'],
                                        c['action_full'], c['q_online'])
        j.branches = native.branches(sizes_)
        return j

    def blocks():
        ca = _c_args(c, c_y)
        ca.q_online, ca.E_online = c['c_q_online'].data_ptr(), E
        return _d_args(c, d_y), ca

    def ret(d, ca, j=None, td_=td):
        return lib.asac_hybrid_return(C.byref(d), C.byref(ca), C.byref(j or job()), p(td_), s)

    def q_loss(br, B_=B, eps=0.2):
        return lib.asac_hybrid_q_loss_grad(
            C.byref(br), C.byref(native.members(c['q_online'], D)), p(c['action_full'][:, 0]), c['action_full'].stride(0),
            p(c['c_q_online']), p(c['c_t_q']), p(c['y']), c['y'].stride(0), p(c['c_y']), c['c_y'].stride(0), None, 0, B_, eps,
            p(loss_q), p(grad_qd), p(grad_cq), s)

    def pi_loss(br, Es=E, B_=B, A_=A):
        return lib.asac_hybrid_policy_loss_grad(
            C.byref(br), p(c['logits0']), c['logits0'].stride(0), C.byref(native.members(c['q_online'], D)), None,
            p(c['mu0']), c['mu0'].stride(0), p(c['log_alpha']), 0.5, p(c['logp0']), p(c['c_q_pi']), None, Es,
            p(c['log_c_alpha']), p(c['scale0']), c['scale0'].stride(0), A_, B_, p(loss_pi), p(grad_z), D, p(grad_lp),
            p(grad_cq_pi), p(d_ent), p(c_ent), s)

    def alpha(br, B_=B):
        return lib.asac_hybrid_alpha_grad(C.byref(br), p(c['logits0']), c['logits0'].stride(0), p(c['target']), p(c['logp0']),
                                          -float(A), B_, p(slots), s)

    ok_br, uneven = native.branches(sizes), native.branches(sizes)
    uneven.D = D + 1
    uneven_job = job()
    uneven_job.branches = uneven
    (d_b, c_b), (d_n, c_n), (d_td, c_td), (d_td2, c_td2), (d_es, c_es), (d_ces, c_ces), (d_a0, c_a0) = (blocks() for _ in range(7))
    c_b.B, d_n.n = B - 1, n - 1
    d_td.td_error_out, c_td2.td_error_out = td.data_ptr(), td.data_ptr()
    d_es.E_sample, c_ces.E_sample, c_a0.A = E + 1, E + 1, 0
    refused = [ret(d_b, c_b), ret(d_n, c_n), ret(d_td, c_td), ret(d_td2, c_td2), ret(*blocks(), j=uneven_job),
               ret(d_es, c_es), ret(d_ces, c_ces), ret(d_a0, c_a0),
               q_loss(ok_br, eps=0.), q_loss(ok_br, eps=-0.1), q_loss(ok_br, B_=1025), q_loss(uneven),
               pi_loss(ok_br, Es=E + 1), pi_loss(ok_br, B_=1025), pi_loss(ok_br, A_=0), pi_loss(uneven),
               alpha(ok_br, B_=1025), alpha(uneven)]
    assert refused == [bad] * len(refused), refused
    # no rows: nothing to launch, no error
    d_0, c_0 = blocks()
    d_0.B = c_0.B = 0
    assert [ret(d_0, c_0), q_loss(ok_br, B_=0), pi_loss(ok_br, B_=0), alpha(ok_br, B_=0)] == [0, 0, 0, 0]
    torch.cuda.synchronize()
    for t in outputs:
        assert (t == 7.).all(), 'nothing was launched'
    # ... and the same calls with good arguments run
    assert [ret(*blocks()), q_loss(ok_br), pi_loss(ok_br), alpha(ok_br)] == [0, 0, 0, 0]
    torch.cuda.synchronize()
    for t in outputs:
        assert torch.isfinite(t).all() and not (t == 7.).all()
