"""GPU: the pure-discrete, policy-based learner on the native path (`hip_config['fused_discrete']`, csrc/discrete.hip):
the four `asac_discrete_*` kernels against float64 and against the float32 eager composition, the bits the kernels share,
three recorded reference steps (`tests/golden/f6_step_discrete*.npz`) through the learner with and without the launches,
launch counts, the captured step, the fallbacks and the refused arguments."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import discrete_ref as dr  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.golden.make_discrete_golden import CASES, SMALL  # noqa: E402

ULP = 2.0 ** -23
# (B, n, branches): a single row; two branches; rows that do not fill a workgroup, one branch; a long window, three branches;
# more rows than one pass of 256 lanes; the width limit
SHAPES = [(1, 1, (2,)), (5, 3, (3, 2)), (37, 4, (4,)), (16, 40, (3, 2, 5)), (300, 2, (17,)), (3, 1, (64,))]
ENSEMBLES = [(1, 1), (2, 2), (3, 2)]


def _vtrace_args(c, y_out, td_out=None):
    from asac_amd import native
    a = native.VtraceArgs()
    a.reward, a.reward_stride = c['reward'].data_ptr(), c['reward'].stride(0)
    a.done, a.last_mask, a.padding_mask = c['done'].data_ptr(), c['last'].data_ptr(), c['pad'].data_ptr()
    assert c['done'].stride(0) == c['last'].stride(0) == c['pad'].stride(0)
    a.mask_stride = c['done'].stride(0)
    a.gamma_ratio, a.lambda_ratio = c['gamma_ratio'].data_ptr(), c['lambda_ratio'].data_ptr()
    a.gamma, a.v_rho, a.v_c = c['gamma'], c['v_rho'], c['v_c']
    a.use_n_step_is, a.B, a.n = int(c['use_is']), c['B'], c['n']
    a.subset_n, a.subset_next, a.E_sample = c['sub_n'].data_ptr(), c['sub_next'].data_ptr(), c['Es']
    a.log_alpha = c['log_alpha'].data_ptr()
    if c['use_is']:
        a.mu_prob, a.mu_stride_b, a.mu_stride_t = c['mu'].data_ptr(), c['mu'].stride(0), c['mu'].stride(1)
    a.y_out = y_out.data_ptr()
    if td_out is not None:
        a.td_error_out = td_out.data_ptr()
    return a


def _kernels(c, alloc=None):
    """the four launches on the case's (strided, device) tensors, outputs pre-filled with NaN (`alloc`: another allocator
    of NaN-filled outputs, `discrete_ref.Guarded`) -> {name: tensor}"""
    from asac_amd import native
    B, D, E = c['B'], c['D'], c['E']
    nan = alloc or (lambda *shape: torch.full(shape, float('nan'), device='cuda'))
    br = native.branches(c['sizes'])
    out = {'y': nan(B), 'td': nan(B), 'loss_q': nan(E), 'grad_q': nan(E, B, D), 'loss_policy': nan(), 'grad_logits': nan(B, D),
           'd_entropy': nan(), 'p': nan(B, D), 'h_pi': nan(B), 'grad_alpha': nan(1)}
    native.discrete_return(_vtrace_args(c, out['y'], out['td']), br, c['q_target'], c['logits'], action=c['action'],
                           q_online=c['q_online'])
    native.discrete_q_loss_grad(br, c['q_online'], c['action'][:, 0], c['y'], c['w'], out['loss_q'], out['grad_q'])
    native.discrete_policy_loss_grad(br, c['logits0'], c['q_online'], c['sub_pi'], c['Es'], c['mu0'], c['log_alpha'],
                                     c['penalty'], out['loss_policy'], out['grad_logits'], out['d_entropy'], out['p'],
                                     out['h_pi'])
    native.discrete_alpha_grad(br, c['logits0'], c['target'], out['grad_alpha'])
    out['grad_alpha'] = out['grad_alpha'][0]
    return out


def _eager(c):
    """today's float32 torch code on the same device and inputs (the scan through `asac_vtrace_return_direct`, as the
    learner issues it)"""
    from asac_amd import native
    v_n, v_next, pi, mu = dr.values(c)
    y = torch.empty(c['B'], device='cuda')
    cont = lambda t: None if t is None else t.contiguous()      # noqa: E731
    native.vtrace_return_direct(_vtrace_args(c, y), v_n.contiguous(), v_next.contiguous(), cont(pi), cont(mu))
    out = {'y': y, 'td': dr.td_error(c, y)}
    for f in (dr.q_loss, dr.policy_loss, dr.alpha_grad):
        out.update(f(c))
    return out


def _compare(tag, c, alloc=None):
    """kernel and eager float32 against float64 -> [(tensor, kernel error, eager error, floor)] of the tensors over the
    bound (`discrete_ref.over_the_bound`); prints every figure"""
    want = dr.as_numpy(dr.all_formulas(dr.to(c, torch.float64, 'cpu')))
    dev = dr.to(c, torch.float32, 'cuda', strided=True)
    assert dev['logits'].stride(1) == c['D'] + 5 and dev['q_target'][0].stride(1) == c['D'] + 5      # strided views
    assert dev['done'].stride(0) == c['n'] + 2 and dev['reward'].stride(0) == c['n'] + 5
    kernel, eager = dr.as_numpy(_kernels(dev, alloc)), dr.as_numpy(_eager(dev))
    return dr.over_the_bound(tag, want, kernel, eager)[0]


@pytest.mark.parametrize('use_is', [False, True], ids=['plain', 'is'])
@pytest.mark.parametrize('E,Es', ENSEMBLES)
@pytest.mark.parametrize('B,n,sizes', SHAPES)
def test_kernels_against_float64_and_the_eager_composition(B, n, sizes, E, Es, use_is):
    """The four entry points on strided views, outputs pre-filled with NaN, against the float64 restatement of the
    oracle's formulas (tests/discrete_ref.py; tests/test_discrete_host.py pins it to the oracle).  Row 0 is wholly padded,
    row 1 has `done` at t = 0, row 2's stored action at t = 0 is all zeros.  Bound (the rule of tests/test_fused_gate_gpu.py):
    per tensor the kernel's largest absolute error against float64 may be at most twice that of the float32 eager
    composition — today's torch code on the same device and inputs — against the same float64 values, with a floor of 4
    units in the last place at the tensor's largest magnitude: both are float32 sums over the same terms in another
    order.  With and without IS weights.  Observed on MI355X: DESIGN.md section 5."""
    import asac_amd  # noqa: F401
    bad = []
    for weights in (False, True):
        c = dr.make_case(B, n, sizes, E, Es, use_is, weights, seed=B + 7 * n + len(sizes) + E)
        bad += _compare(f'{(B, n, sizes)} E {E}/{Es} is={use_is} w={weights}', c)
    assert not bad, bad


@pytest.mark.parametrize('B,n,sizes', [(5, 3, (3, 2)), (16, 40, (3, 2, 5)), (3, 1, (64,))])
def test_saturated_logits_on_both_sides_of_the_clamp(B, n, sizes):
    """logits spread by +-30: probabilities on both sides of the 1e-8 clamp, every one of them above 1e-6 or below 1e-12
    in float64, so float32 and float64 agree on the side of each entry; same bound as above"""
    import asac_amd  # noqa: F401
    c = dr.saturate(dr.make_case(B, n, sizes, 3, 2, True, True, seed=B + n), seed=n)
    probs = dr.clamp_sides(dr.to(c, torch.float64, 'cpu'))
    assert bool(((probs > 1e-6) | (probs < 1e-12)).all())
    assert bool((probs > 1e-6).any()) and bool((probs < 1e-12).any()), 'both sides of the clamp occur'
    bad = _compare(f'saturated {(B, n, sizes)}', c)
    assert not bad, bad


@pytest.mark.parametrize('B,n,sizes', SHAPES)
def test_policy_and_temperature_kernels_form_the_same_bits(B, n, sizes):
    """p and the entropy at the step's state come from one implementation (csrc/asac_categorical.h): the policy-loss
    launch and the temperature launch write the same bits for the same logits"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    c = dr.to(dr.make_case(B, n, sizes, 2, 2, False, False, seed=B), torch.float32, 'cuda', strided=True)
    D, br = c['D'], native.branches(sizes)
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')      # noqa: E731
    p_pi, h_pi, p_al, h_al = nan(B, D), nan(B), nan(B, D), nan(B)
    native.discrete_policy_loss_grad(br, c['logits0'], c['q_online'], None, 2, c['mu0'], c['log_alpha'], c['penalty'],
                                     nan(), nan(B, D), nan(), p_pi, h_pi)
    native.discrete_alpha_grad(br, c['logits0'], c['target'], nan(1), p_al, h_al)
    assert torch.isfinite(p_pi).all() and torch.isfinite(h_pi).all()
    assert torch.equal(p_pi, p_al) and torch.equal(h_pi, h_al)


# ------------------------------------------------------------------------------------------------
# the step
# ------------------------------------------------------------------------------------------------
def _learner(case, golden_dir=None, cls=None, **hip):
    """the case's learner (tests/golden/make_discrete_golden.CASES) with the fixture's weights and episodes if
    `golden_dir` is given -> (agent, fixture | None)"""
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    plugin_name, kw, d_sizes = CASES[case]
    kw = dict(kw)
    convert_config_to_enum(kw)
    agent = (cls or SAC_Base)(['vector'], [(6,)], list(d_sizes), 0, None, pu.plugin(plugin_name), device='cuda:0',
                              batch_size=SMALL['batch_size'], replay_config={'capacity': SMALL['capacity']},
                              hip_config=hip, **kw)
    if golden_dir is None:
        return agent, None
    g = np.load(golden_dir / f'f6_step_{case}.npz')
    pu.load_golden_weights(agent, g)
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    return agent, g


def _discrete_calls(summary):
    return {k: v['calls'] for k, v in summary.items() if k.startswith('asac_discrete_')}


# the call-site defaults of tests/test_sac_aux_gpu.py (loss_q, td_error, tree); the policy objective and the entropy are
# means of O(1) terms like the Q loss and may pass through zero, so they take the TD error's absolute term too; log_d_alpha
# moves by +-lr = 3e-4 per step: rtol 2e-4 of |-2.3| stays below one step taken with the wrong sign
OBSERVABLES = {'loss_q': dict(rtol=2e-4, atol=0.), 'loss_policy': dict(rtol=2e-4, atol=2e-5),
               'd_entropy': dict(rtol=2e-4, atol=2e-5), 'td_error': dict(rtol=2e-4, atol=2e-5),
               'tree': dict(rtol=2e-4, atol=1e-6), 'log_d_alpha': dict(rtol=2e-4, atol=2e-5)}


ONE_STEP = {'asac_discrete_return': 2, 'asac_discrete_q_loss_grad': 1, 'asac_discrete_policy_loss_grad': 1,
            'asac_discrete_alpha_grad': 1}


def _run_fixture(case, golden_dir, fused):
    """the fixture's steps through the learner -> ({observable: |error| array of step 0}, [failures])"""
    from algorithm.fused import RecordedNoise
    agent, g = _learner(case, golden_dir, cls=pu.hooked_learner(), use_graph=False, fused_discrete=fused)
    rb = agent.replay_buffer
    mods = {name: m for name, m in agent.ckpt_dict.items() if isinstance(m, torch.nn.Module)}
    n_steps = int(g['n_steps'])
    step_box, failures, errors0 = [0], [], {}

    def soft(fn, what):
        try:
            fn()
        except AssertionError as e:
            failures.append(f'{what}: {str(e).strip().splitlines()[0] if str(e).strip() else "assertion"}'
                            f' | {" ".join(str(e).split())[:300]}')

    def align_with_reference():     # see tests/test_sac_step_gpu.py: compare the fresh update, then align
        s = step_box[0]
        soft(lambda: pu.assert_weights_close(mods, g, 1, 3e-4, rtol=1e-3, atol=2e-5, prefix=f'step{s}/w_rq'), f'step {s} w_rq')
        pu.load_golden_weights(agent, g, prefix=f'step{s}/w_rq')

    if 'step0/w_rq/model_q_0/' + next(iter(agent.model_q_list[0].state_dict())) in g.files:
        agent.after_rep_q_update = align_with_reference
    from asac_amd import native
    for s in range(n_steps):
        step_box[0] = s
        agent.noise = RecordedNoise([g[f'step{s}/u']], [], list(g[f'step{s}/perm']))
        rb.uniform_source = agent.noise
        with native.LaunchProfiler(repeat=1) as prof:
            assert agent.train() == s + 1
        calls = _discrete_calls(prof.summary())
        assert (sum(calls.values()) > 0) == fused, calls
        assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
        assert np.array_equal(rb._ids.cpu().numpy(), g[f'step{s}/sample_ids']), f'step {s}: PER index selection'
        got = {'loss_q': agent._stats['loss_q'].item(), 'loss_policy': agent._stats['loss_policy'].item(),
               'd_entropy': agent._stats['d_entropy'].item(), 'td_error': agent._td_error.cpu().numpy()[:, None],
               'tree': rb._tree.cpu().numpy(), 'log_d_alpha': agent.log_d_alpha.item()}
        for name, tol in OBSERVABLES.items():
            want = g[f'step{s}/{name}']
            err = np.abs(np.asarray(got[name], dtype=np.float64) - want)
            print(f'{case} fused={fused} step {s} {name}: max error {float(err.max()):.3e} at scale {float(np.abs(want).max()):.3e}')
            if s == 0:
                errors0[name] = (float(err.max()), float(np.abs(want).max()))
            soft(lambda: np.testing.assert_allclose(got[name], want, err_msg=name, **tol), f'step {s} {name}')
        if s == 0:
            soft(lambda: pu.assert_first_step_gradients(agent, g, rtol=2e-3, atol_frac=5e-5), 'first-step gradients')
    soft(lambda: pu.assert_weights_close(mods, g, n_steps, 3e-4, rtol=1e-3, atol=2e-5), 'weights')
    rb.check_health()
    agent.close()
    return errors0, failures


@pytest.mark.parametrize('case', list(CASES))
def test_step_against_the_reference_fixture(golden_dir, case):
    """The recorded reference steps through `SAC_Base(..., hip_config={'use_graph': False})` with `RecordedNoise`, as
    tests/test_sac_aux_gpu.py does: PER ids bit-exact, every recorded draw consumed; loss_q, loss_policy, d_entropy,
    td_error, tree and log_d_alpha, the first step's gradients and the weights after the steps under that file's call-site
    defaults (no tolerance-table entries).  The same steps run with `fused_discrete=False`; for step 0 each observable's
    error against the fixture under the launches may be at most twice that of the eager path, floor 4 units in the last
    place at the observable's largest magnitude."""
    fused_err, fused_failures = _run_fixture(case, golden_dir, True)
    eager_err, eager_failures = _run_fixture(case, golden_dir, False)
    bad = []
    for name in OBSERVABLES:
        (e_f, scale), (e_e, _) = fused_err[name], eager_err[name]
        floor = 4 * ULP * scale
        print(f'{case} step 0 {name}: fused {e_f:.3e}  eager {e_e:.3e}  floor {floor:.3e}')
        if e_f > max(2 * e_e, floor):
            bad.append((name, e_f, e_e, floor))
    assert not eager_failures, ('the eager pure-discrete path misses its own defaults', eager_failures)
    assert not fused_failures, fused_failures
    assert not bad, bad


def test_one_step_issues_one_launch_per_item(golden_dir):
    """one eager step of the `discrete` case: two returns (target and TD error), one launch per loss and for the
    temperature, and no `asac_vtrace_return_direct`"""
    from asac_amd import native
    agent, _ = _learner('discrete', golden_dir, use_graph=False)
    torch.manual_seed(0)
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    seen = prof.summary()
    agent.close()
    assert _discrete_calls(seen) == ONE_STEP
    assert 'asac_vtrace_return_direct' not in seen


def _episodes(d_sizes, c_size, hidden=(0,)):
    rng = np.random.default_rng(1)
    return [pu.synthetic_episode(rng, [(6,)], list(d_sizes), c_size, hidden, T_) for T_ in (60, 45, 70)]


def test_captured_step_matches_eager():
    """the pattern of test_captured_step_with_a_rotary_representation_matches_eager: three `train()` calls — eager, and
    capture + replay + replay with host work in between — leave the same parameters, tree and TD errors (the discrete
    launches allocate nothing and synchronise nothing, so they are nodes of the step's graph)"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.sac_base import SAC_Base
    episodes = _episodes((3, 2), 0)
    results = []
    for use_graph in (False, True):
        torch.manual_seed(3), np.random.seed(3), random.seed(3)
        agent = SAC_Base(['vector'], [(6,)], [3, 2], 0, None, pu.plugin('nn_vec'), device='cuda:0', n_step=3,
                         ensemble_q_num=3, ensemble_q_sample=2, batch_size=16, replay_config={'capacity': 256},
                         hip_config={'use_graph': use_graph, 'graph_warmup': 1})
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        launches = 0
        for i in range(3):
            if i == 0:
                with native.LaunchProfiler(repeat=1) as prof:
                    agent.train()
                launches = sum(_discrete_calls(prof.summary()).values())
            else:
                agent.train()
            torch.cuda.synchronize()
            np.sort(np.random.default_rng(i).standard_normal(1 << 14))         # host work between the replays
        assert launches == 5, 'the step runs the one-launch discrete arithmetic'
        assert (agent._graph is not None) == use_graph, 'the discrete step must capture'
        results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                        agent._td_error.cpu().numpy().copy()))
        agent.close()
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)


FALLBACKS = {
    'flag_off': dict(d=(3, 2), c=0, hip=dict(fused_discrete=False)),
    'hybrid': dict(d=(3, 2), c=2),
    'dqn_like': dict(d=(3, 2), c=0, kw=dict(discrete_dqn_like=True)),
    'width_65': dict(d=(65,), c=0),
    'nine_branches': dict(d=(2,) * 9, c=0),
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_what_the_path_does_not_cover_runs_todays_code(case):
    """each of these issues no `asac_discrete_*` launch and still trains"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.sac_base import SAC_Base
    cfg = FALLBACKS[case]
    torch.manual_seed(0)
    agent = SAC_Base(['vector'], [(6,)], list(cfg['d']), cfg['c'], None, pu.plugin('nn_vec'), device='cuda:0', n_step=3,
                     batch_size=16, replay_config={'capacity': 256}, hip_config={'use_graph': False, **cfg.get('hip', {})},
                     **cfg.get('kw', {}))
    for ep in _episodes(cfg['d'], cfg['c']):
        agent.put_episode(**ep)
    before = agent._params.flat.clone()
    with native.LaunchProfiler(repeat=1) as prof:
        assert agent.train() == 1
    assert not _discrete_calls(prof.summary())
    q0 = slice(*agent._params.segments['q_0'])
    assert torch.isfinite(agent._params.flat).all() and not torch.equal(before[q0], agent._params.flat[q0])
    assert torch.isfinite(agent._td_error).all()
    agent.close()


def test_an_option_runs_todays_code():
    """`OptionBase` switches the path off in its constructor: its policy and temperature steps (the parent's
    `_train_policy` / `_train_alpha`) issue no `asac_discrete_*` launch and still train"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.oc import OptionBase
    torch.manual_seed(0)
    B, n, D = 16, 3, 5
    opt = OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [3, 2], 0, None, pu.plugin('nn_oc_small'),
                     device='cuda:0', batch_size=B, summary_path=None, n_step=n)
    assert opt._fused_discrete is False
    gen = torch.Generator().manual_seed(1)
    ep = pu.synthetic_episode(np.random.default_rng(2), [(6,)], [3, 2], 0, (0,), B * n)
    actions = torch.from_numpy(ep['ep_actions']).view(B, n, D).cuda()
    obs = torch.randn(B, n, 6, generator=gen).cuda()
    states = torch.randn(B, n + 1, opt.state_size, generator=gen).cuda()
    mu = torch.rand(B, n, D, generator=gen).cuda()
    seg = slice(*opt._params.segments['policy'])
    before = opt._params.flat[seg].clone()
    with native.LaunchProfiler(repeat=1) as prof:
        opt.train_policy_alpha(torch.zeros(B, n, dtype=torch.bool, device='cuda'), [obs], states, actions, mu)
    assert not _discrete_calls(prof.summary())
    assert torch.isfinite(opt._params.flat).all() and not torch.equal(before, opt._params.flat[seg])
    opt.close()


# ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    """null outputs, E_sample > E, D > 64, a branch table that does not add up, B > 1024 for the single-workgroup
    reductions, n > 64: hipErrorInvalidValue and no launch"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    B, n, sizes, E = 8, 3, (3, 2), 2
    c = dr.to(dr.make_case(B, n, sizes, E, E, True, True, seed=5), torch.float32, 'cuda', strided=True)
    D = c['D']
    lib, s, bad = native.load(), native._stream(), 1      # hipErrorInvalidValue
    marker = lambda *shape: torch.full(shape, 7., device='cuda')      # noqa: E731
    y, td, loss_q, grad_q = marker(B), marker(B), marker(E), marker(E, B, D)
    loss_pi, grad_z, ent, slot = marker(1), marker(B, D), marker(1), marker(1)
    outputs = (y, td, loss_q, grad_q, loss_pi, grad_z, ent, slot)
    p = native._p

    def job(sizes_=sizes, q_target=c['q_target'], q_online=c['q_online']):
        j = native.DiscreteReturn()
        j.branches = native.branches(sizes_)
        j.q_target, j.q_online = native.members(list(q_target), D), native.members(list(q_online), D)
        j.logits, j.logits_stride_b, j.logits_stride_t = c['logits'].data_ptr(), c['logits'].stride(0), c['logits'].stride(1)
        j.action, j.action_stride_b, j.action_stride_t = c['action'].data_ptr(), c['action'].stride(0), c['action'].stride(1)
        return j

    def ret(a, j):
        return lib.asac_discrete_return(C.byref(a), C.byref(j), s)

    def q_loss(br, B_=B, loss=loss_q, grad=grad_q):
        return lib.asac_discrete_q_loss_grad(C.byref(br), C.byref(native.members(c['q_online'], D)), p(c['action'][:, 0]),
                                             c['action'].stride(0), p(c['y']), c['y'].stride(0), None, 0, B_, p(loss),
                                             p(grad), s)

    def pi_loss(br, Es=E, B_=B, loss=loss_pi, grad=grad_z):
        return lib.asac_discrete_policy_loss_grad(
            C.byref(br), p(c['logits0']), c['logits0'].stride(0), C.byref(native.members(c['q_online'], D)), None, Es,
            p(c['mu0']), c['mu0'].stride(0), p(c['log_alpha']), 0.5, B_, p(loss), p(grad), D, p(ent), None, None, s)

    def alpha(br, B_=B, out=slot):
        return lib.asac_discrete_alpha_grad(C.byref(br), p(c['logits0']), c['logits0'].stride(0), p(c['target']), B_,
                                            p(out), None, None, s)

    ok_br, wide, uneven = native.branches(sizes), native.branches((65,)), native.branches(sizes)
    uneven.D = D + 1
    a_null, a_es, a_n = _vtrace_args(c, y, td), _vtrace_args(c, y, td), _vtrace_args(c, y, td)
    a_null.y_out, a_es.E_sample, a_n.n = None, E + 1, 65
    wide_job, uneven_job = job(), job()
    wide_job.branches, uneven_job.branches = wide, uneven
    refused = [ret(a_null, job()), ret(a_es, job()), ret(a_n, job()), ret(_vtrace_args(c, y, td), wide_job),
               ret(_vtrace_args(c, y, td), uneven_job),
               q_loss(ok_br, loss=None), q_loss(ok_br, grad=None), q_loss(wide), q_loss(ok_br, B_=1025),
               pi_loss(ok_br, loss=None), pi_loss(ok_br, grad=None), pi_loss(ok_br, Es=E + 1), pi_loss(wide),
               pi_loss(ok_br, B_=1025), alpha(ok_br, out=None), alpha(wide), alpha(ok_br, B_=1025)]
    assert refused == [bad] * len(refused), refused
    with pytest.raises(native.AsacNativeError):
        native.discrete_policy_loss_grad(ok_br, c['logits0'], c['q_online'], None, E + 1, c['mu0'], c['log_alpha'], 0.5,
                                         loss_pi, grad_z, ent)
    torch.cuda.synchronize()
    for t in outputs:
        assert (t == 7.).all(), 'nothing was launched'
    # ... and the same calls with good arguments run
    assert [ret(_vtrace_args(c, y, td), job()), q_loss(ok_br), pi_loss(ok_br), alpha(ok_br)] == [0, 0, 0, 0]
    torch.cuda.synchronize()
    for t in outputs:
        assert torch.isfinite(t).all() and not (t == 7.).all()
