"""GPU: the DQN-like discrete learner on the native path (`hip_config['fused_dqn']`, csrc/dqn.hip): the target / loss
kernels against float64 and against the float32 eager composition, ties, the bits the two target-forming launches share,
the acting kernel, the learner's acting, three recorded reference steps (`tests/golden/f6_step_dqn*.npz`) through the
learner with and without the launches, launch counts, the captured step, the fallbacks and the refused arguments."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import dqn_ref as qr  # noqa: E402
from tests.discrete_ref import over_the_bound  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.golden.make_dqn_golden import CASES, SMALL  # noqa: E402

ULP = 2.0 ** -23
# (B, n, branches): a single row; two branches; rows that do not fill a workgroup, one branch; the longest window, three
# branches; more rows than one pass of 256 lanes (and than four workgroups of 64); the width limit
SHAPES = [(1, 1, (2,)), (5, 3, (3, 2)), (37, 4, (4,)), (16, 64, (3, 2, 5)), (300, 2, (17,)), (3, 1, (64,))]
# (E, E_sample): both sides of the two-slot / eight-slot kernels' threshold (E_sample <= 2), a sampled subset, the limit
ENSEMBLES = [(1, 1), (2, 2), (3, 2), (8, 5)]


def _vtrace_args(c, y_out, td_out=None):
    from asac_amd import native
    a = native.VtraceArgs()
    a.reward, a.reward_stride = c['reward'].data_ptr(), c['reward'].stride(0)
    a.done, a.last_mask, a.padding_mask = c['done'].data_ptr(), c['last'].data_ptr(), c['pad'].data_ptr()
    assert c['done'].stride(0) == c['last'].stride(0) == c['pad'].stride(0)
    a.mask_stride = c['done'].stride(0)
    a.gamma_ratio, a.gamma = c['gamma_ratio'].data_ptr(), c['gamma']
    a.B, a.n = c['B'], c['n']
    a.subset_n, a.subset_next, a.E_sample = c['sub_n'].data_ptr(), c['sub_next'].data_ptr(), c['Es']
    a.y_out = y_out.data_ptr() if y_out is not None else None
    if td_out is not None:
        a.td_error_out = td_out.data_ptr()
    return a


def _job(c, online=True):
    from asac_amd import native
    return native.dqn_job(native.branches(c['sizes']), c['q_eval'], c['q_target'], action=c['action'],
                          q_online=c['q_online'] if online else None)


def _kernels(c, alloc=None):
    """the two launches on the case's (strided, device) tensors, outputs pre-filled with NaN (`alloc`: another allocator
    of NaN-filled outputs, `discrete_ref.Guarded`) -> {name: tensor}"""
    from asac_amd import native
    B, D, E = c['B'], c['D'], c['E']
    nan = alloc or (lambda *shape: torch.full(shape, float('nan'), device='cuda'))
    out = {'y': nan(B), 'td': nan(B), 'loss_q': nan(E), 'grad_q': nan(E, B, D), 'y_loss': nan(B)}
    native.dqn_return(_vtrace_args(c, out['y'], out['td']), _job(c))
    native.dqn_q_loss_grad(_vtrace_args(c, out['y_loss']), _job(c), c['w'], out['loss_q'], out['grad_q'])
    return out


def _eager(c):
    """today's float32 torch code on the same device and inputs: `get_dqn_like_d_y` plus the loss and TD lines"""
    from algorithm.sac_base import SAC_Base
    stub = qr.eager_stub(c, 'cuda')
    return qr.eager(c, lambda *a: SAC_Base.get_dqn_like_d_y(stub, *a))


def _compare(tag, c, alloc=None):
    """kernel and eager float32 against float64 -> ([(tensor, kernel error, eager error, floor)] of the tensors over the
    bound, the largest share of the bound) (`discrete_ref.over_the_bound`); prints every figure"""
    want = qr.all_formulas(qr.to(c, torch.float64, 'cpu'))
    dev = qr.to(c, torch.float32, 'cuda', strided=True)
    assert dev['q_eval'][0].stride(1) == c['D'] + 5 and dev['q_target'][0].stride(1) == c['D'] + 5      # strided views
    assert dev['done'].stride(0) == c['n'] + 2 and dev['reward'].stride(0) == c['n'] + 5
    kernel, eager = qr.as_numpy(_kernels(dev, alloc)), qr.as_numpy(_eager(dev))
    assert np.array_equal(kernel.pop('y_loss'), kernel['y']), 'the loss launch stores the return launch\'s y'
    return over_the_bound(tag, want, kernel, eager)


@pytest.mark.parametrize('E,Es', ENSEMBLES)
@pytest.mark.parametrize('B,n,sizes', SHAPES)
def test_kernels_against_float64_and_the_eager_composition(B, n, sizes, E, Es):
    """`asac_dqn_return` and `asac_dqn_q_loss_grad` on strided views, outputs pre-filled with NaN, against the float64
    restatement (tests/dqn_ref.py; tests/test_dqn_host.py pins it to the recorded reference function).  Row 0 is wholly
    masked, row 1 has `done` at L, row 2 has L = 0, row 3's stored action is all zeros.  Bound (the rule of
    tests/test_discrete_gpu.py): per tensor the kernel's largest absolute error against float64 may be at most twice that
    of the float32 eager composition — `get_dqn_like_d_y` plus today's loss and TD lines on the same device and inputs —
    with a floor of 4 units in the last place at the tensor's largest magnitude.  With and without IS weights.  Observed
    on MI355X: NOTES.md, "DQN-like"."""
    import asac_amd  # noqa: F401
    bad, share = [], 0.
    for weights in (False, True):
        c = qr.make_case(B, n, sizes, E, Es, weights, seed=B + 7 * n + len(sizes) + E)
        b_, s_ = _compare(f'{(B, n, sizes)} E {E}/{Es} w={weights}', c)
        bad, share = bad + b_, max(share, s_)
    print(f'{(B, n, sizes)} E {E}/{Es}: largest share of the bound {share:.2f}')
    assert not bad, bad


# E_sample 1 and 2: the two-slot instantiation of the target; 3 and 5: the eight-slot one
@pytest.mark.parametrize('B,n,sizes,E,Es', [(5, 3, (3, 2), 1, 1), (37, 4, (4,), 2, 2), (9, 2, (3, 2, 5), 4, 3),
                                            (37, 3, (3, 2, 5), 8, 5)])
def test_ties_pick_the_index_torch_argmax_picks_on_the_cpu(B, n, sizes, E, Es):
    """exact ties in every branch of the eval values and of the acting kernel's heads.  Every target table holds powers of
    two by column, rewards are zero, gamma one and nothing done, so K * v_i is the sum of 2^(column member i picked) and
    names the indices; y is the smallest of them.  The acting kernel sees the tied heads greedy, with uniforms under
    epsilon 0, and with some rows replaced."""
    import asac_amd  # noqa: F401
    from asac_amd import native
    K, D = len(sizes), sum(sizes)
    c = qr.tie_every_branch(qr.make_case(B, n, sizes, E, Es, False, seed=B), seed=n)
    c['gamma'], c['gamma_ratio'] = 1., torch.ones(n)
    c['reward'].zero_()
    c['done'].zero_()
    for t in c['q_target']:
        t.copy_((2. ** torch.arange(D)).expand(B, n + 1, D))
    L = qr.last_valid(c['last'].numpy(), c['pad'].numpy())
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    want = np.full(B, np.inf, dtype=np.float32)
    ties = 0
    for b in range(B):
        for e in c['sub_n'].tolist():
            row, j0, v = c['q_eval'][e][b, L[b]], 0, np.float32(0.)
            for k, s in enumerate(sizes):
                part = row[j0:j0 + s]
                ties += int((part == part.max()).sum() > 1)
                v += np.float32(2. ** (starts[k] + int(torch.argmax(part))))
                j0 += s
            want[b] = min(want[b], v / np.float32(K))
    assert ties > 0
    dev = qr.to(c, torch.float32, 'cuda', strided=True)
    y = torch.full((B,), float('nan'), device='cuda')
    native.dqn_return(_vtrace_args(dev, y), _job(dev, online=False))
    assert np.array_equal(y.cpu().numpy(), want)
    # the acting kernel on the tied heads of one position
    q = c['q_eval'][0][:, 0].contiguous()
    u = torch.rand(B, 1 + K, generator=torch.Generator().manual_seed(B + n))
    br = native.branches(sizes)
    cpu = torch.cat([torch.nn.functional.one_hot(torch.argmax(part, dim=-1), s).float()
                     for part, s in zip(q.split(list(sizes), dim=-1), sizes)], dim=-1)
    for u_, eps in ((None, 0.5), (u, 0.), (u, 0.5)):
        act = torch.full((B, D), float('nan'), device='cuda')
        native.dqn_act(br, q.cuda(), None if u_ is None else u_.cuda(), eps, act)
        if u_ is None or eps == 0.:
            assert torch.equal(act.cpu(), cpu)
        else:
            rows = u[:, 0] >= 0.5                # the rows that stay greedy keep the CPU's index
            assert torch.equal(act.cpu()[rows], cpu[rows])
            assert np.array_equal(act.cpu().numpy(), qr.act(q.numpy(), u.numpy(), eps, sizes))


@pytest.mark.parametrize('B,n,sizes,E,Es', [(37, 4, (4,), 2, 2), (300, 2, (17,), 3, 2), (16, 64, (3, 2, 5), 8, 5)])
def test_the_loss_launch_stores_the_bits_of_the_return_launch(B, n, sizes, E, Es):
    """one implementation of the row's target (csrc/asac_dqn.h): `asac_dqn_q_loss_grad`'s `y_out` is `torch.equal` to
    `asac_dqn_return`'s y on the same inputs"""
    import asac_amd  # noqa: F401
    out = _kernels(qr.to(qr.make_case(B, n, sizes, E, Es, True, seed=B), torch.float32, 'cuda', strided=True))
    assert torch.isfinite(out['y']).all() and torch.equal(out['y'], out['y_loss'])


def test_the_loss_launch_shares_the_discrete_q_loss_launchs_bits():
    """one implementation of the Q step's row (`disc_dot`, csrc/asac_discrete_rows.h `disc_q_grad_row`): on the smallest
    case with two branches, `asac_discrete_q_loss_grad` given the y `asac_dqn_q_loss_grad` stored and the same weights
    returns its loss and its gradient, `torch.equal`"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    c = qr.to(qr.make_case(5, 3, (3, 2), 3, 2, True, seed=5), torch.float32, 'cuda', strided=True)
    out = _kernels(c)
    assert c['w'] is not None and torch.isfinite(out['y_loss']).all()
    loss, grad = torch.full_like(out['loss_q'], float('nan')), torch.full_like(out['grad_q'], float('nan'))
    native.discrete_q_loss_grad(native.branches(c['sizes']), c['q_online'], c['action'], out['y_loss'], c['w'], loss, grad)
    assert torch.isfinite(loss).all() and torch.equal(out['loss_q'], loss)
    assert torch.isfinite(grad).all() and torch.equal(out['grad_q'], grad)


# ------------------------------------------------------------------------------------------------
# acting
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 37, 300])
def test_acting_kernel_against_the_host_rule(B):
    """exact equality with tests/dqn_ref.act on the same uniforms; `u = None` and `epsilon = 0` are greedy, `epsilon = 1`
    replaces every row; strided heads and output, the output pre-filled with NaN"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    sizes = (3, 2, 5)
    K, D = len(sizes), sum(sizes)
    gen = torch.Generator().manual_seed(B)
    q = qr._strided(torch.randn(B, D, generator=gen).cuda())
    u = qr._strided(torch.rand(B, 1 + K, generator=gen).cuda())
    u[B // 2, 1:] = 0.99999994          # the largest float32 below one: the index stays inside the branch
    br = native.branches(sizes)

    def run(u_, eps):
        out = qr._strided(torch.full((B, D), float('nan'), device='cuda'))
        native.dqn_act(br, q, u_, eps, out)
        return out.cpu().numpy()
    greedy = qr.act(q.cpu().numpy(), None, 0., sizes)
    assert np.array_equal(run(None, 0.3), greedy)
    assert np.array_equal(run(u, 0.), greedy)
    assert np.array_equal(run(u, 0.3), qr.act(q.cpu().numpy(), u.cpu().numpy(), 0.3, sizes))
    every = run(u, 1.)
    assert np.array_equal(every, qr.act(q.cpu().numpy(), u.cpu().numpy(), 1., sizes))
    j0 = 0
    for k, s in enumerate(sizes):      # ... and every row follows its uniforms
        idx = np.minimum(np.floor(u[:, 1 + k].cpu().numpy() * np.float32(s)).astype(np.int64), s - 1)
        assert np.array_equal(every[:, j0:j0 + s].argmax(-1), idx) and (every[:, j0:j0 + s].sum(-1) == 1.).all()
        j0 += s
    if B > 1:
        assert 0 < (u[:, 0] < 0.3).sum().item() < B or B < 8


def test_random_actions_are_uniform_over_each_branch():
    """`epsilon = 1`, 4096 rows, uniforms from `DeviceNoise`: the count of each index of each branch is binomial(B, 1/s):
    within five standard deviations of B / s"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused import DeviceNoise
    torch.manual_seed(11)
    B, sizes = 4096, (3, 2, 5)
    D = sum(sizes)
    u = torch.empty(B, 1 + len(sizes), device='cuda')
    DeviceNoise(seed=5).uniform_(u)
    out = torch.full((B, D), float('nan'), device='cuda')
    native.dqn_act(native.branches(sizes), torch.randn(B, D, device='cuda'), u, 1., out)
    counts = out.sum(0).cpu().numpy()
    j0 = 0
    for s in sizes:
        sigma = np.sqrt(B * (1. / s) * (1. - 1. / s))
        print(f'branch of {s}: counts {counts[j0:j0 + s]}, expected {B / s:.1f} +- {sigma:.1f}')
        assert counts[j0:j0 + s].sum() == B
        assert (np.abs(counts[j0:j0 + s] - B / s) <= 5 * sigma).all()
        j0 += s


def _plain_learner(d_sizes=(3, 2), c_size=0, seed=0, use_graph=False, hip=None, plugin='nn_vec', **kw):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(seed), np.random.seed(seed), random.seed(seed)
    kw.setdefault('discrete_dqn_like', True)
    return SAC_Base(['vector'], [(6,)], list(d_sizes), c_size, None, pu.plugin(plugin), device='cuda:0', n_step=3,
                    batch_size=16, replay_config={'capacity': 256}, hip_config={'use_graph': use_graph, **(hip or {})}, **kw)


def test_learner_acting_with_and_without_the_launch():
    """`choose_action` outside train mode is identical with the flag on and off; in train mode it issues exactly one
    `asac_dqn_act` (and the eager code none)"""
    from asac_amd import native
    rng = np.random.default_rng(3)
    obs = [rng.standard_normal((7, 6)).astype(np.float32)]
    pre_action = np.zeros((7, 5), dtype=np.float32)
    results = {}
    for fused in (True, False):
        agent = _plain_learner(hip=dict(fused_dqn=fused))
        hidden = np.zeros((7, *agent.seq_hidden_state_shape), dtype=np.float32)
        with native.LaunchProfiler(repeat=1) as prof:
            a_train, p_train, _ = agent.choose_action(obs, pre_action, hidden)
        calls = {k: v['calls'] for k, v in prof.summary().items() if k.startswith('asac_dqn_')}
        assert calls == ({'asac_dqn_act': 1} if fused else {}), calls
        assert a_train.shape == (7, 5) and (a_train[:, :3].sum(-1) == 1).all() and (a_train[:, 3:].sum(-1) == 1).all()
        assert (p_train == 1.).all()
        agent.set_train_mode(False)
        results[fused] = agent.choose_action(obs, pre_action, hidden)
        agent.close()
    for a, b in zip(results[True], results[False]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------
# the step
# ------------------------------------------------------------------------------------------------
def _learner(case, golden_dir=None, cls=None, **hip):
    """the case's learner (tests/golden/make_dqn_golden.CASES) with the fixture's weights and episodes if `golden_dir` is
    given -> (agent, fixture | None)"""
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


def _calls(summary, prefix='asac_dqn_'):
    return {k: v['calls'] for k, v in summary.items() if k.startswith(prefix)}


# the call-site defaults of tests/test_sac_aux_gpu.py, as tests/test_discrete_gpu.py states them (no policy objective and
# no temperature in this mode)
OBSERVABLES = {'loss_q': dict(rtol=2e-4, atol=0.), 'td_error': dict(rtol=2e-4, atol=2e-5), 'tree': dict(rtol=2e-4, atol=1e-6)}


ONE_STEP = {'asac_dqn_q_loss_grad': 1, 'asac_dqn_return': 1}


def _run_fixture(case, golden_dir, fused):
    """the fixture's steps through the learner -> ({observable: (|error|, scale) of step 0}, [failures])"""
    from algorithm.fused import RecordedNoise
    from asac_amd import native
    agent, g = _learner(case, golden_dir, cls=pu.hooked_learner(), use_graph=False, fused_dqn=fused)
    rb = agent.replay_buffer
    mods = {name: m for name, m in agent.ckpt_dict.items() if isinstance(m, torch.nn.Module)}
    n_steps = int(g['n_steps'])
    step_box, failures, errors0 = [0], [], {}

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
        agent.noise = RecordedNoise([g[f'step{s}/u']], [], list(g[f'step{s}/perm']))
        rb.uniform_source = agent.noise
        with native.LaunchProfiler(repeat=1) as prof:
            assert agent.train() == s + 1
        calls = _calls(prof.summary())
        assert (sum(calls.values()) > 0) == fused, calls
        assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
        assert np.array_equal(rb._ids.cpu().numpy(), g[f'step{s}/sample_ids']), f'step {s}: PER index selection'
        got = {'loss_q': agent._stats['loss_q'].item(), 'td_error': agent._td_error.cpu().numpy()[:, None],
               'tree': rb._tree.cpu().numpy()}
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
    tests/test_discrete_gpu.py does: PER ids bit-exact, every recorded draw consumed (the target subset is drawn before
    the eval subset); loss_q, td_error and tree, the first step's gradients and the weights after the steps under the
    call-site defaults (no tolerance-table entries).  The same steps run with `fused_dqn=False`, which must meet the
    defaults by itself; for step 0 each observable's error under the launches may be at most twice that of the eager
    path, floor 4 units in the last place at the observable's largest magnitude."""
    fused_err, fused_failures = _run_fixture(case, golden_dir, True)
    eager_err, eager_failures = _run_fixture(case, golden_dir, False)
    bad = []
    for name in OBSERVABLES:
        (e_f, scale), (e_e, _) = fused_err[name], eager_err[name]
        floor = 4 * ULP * scale
        print(f'{case} step 0 {name}: fused {e_f:.3e}  eager {e_e:.3e}  floor {floor:.3e}')
        if e_f > max(2 * e_e, floor):
            bad.append((name, e_f, e_e, floor))
    assert not eager_failures, ('the eager DQN-like path misses its own defaults', eager_failures)
    assert not fused_failures, fused_failures
    assert not bad, bad


def test_one_step_issues_one_launch_per_item(golden_dir):
    """one eager step of the `dqn` case: the loss launch (which forms the target) and the TD error's return launch, and
    nothing of the policy-based path"""
    from asac_amd import native
    agent, _ = _learner('dqn', golden_dir, use_graph=False)
    torch.manual_seed(0)
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    seen = prof.summary()
    agent.close()
    assert _calls(seen) == ONE_STEP
    assert not _calls(seen, 'asac_discrete_')


def _episodes(d_sizes, c_size, hidden=(0,)):
    rng = np.random.default_rng(1)
    return [pu.synthetic_episode(rng, [(6,)], list(d_sizes), c_size, hidden, T_) for T_ in (60, 45, 70)]


def test_captured_step_matches_eager():
    """the pattern of tests/test_discrete_gpu.py::test_captured_step_matches_eager: three `train()` calls — eager, and
    capture + replay + replay with host work in between — leave the same parameters, tree and TD errors (the launches
    allocate nothing and synchronise nothing, so they are nodes of the step's graph)"""
    from asac_amd import native
    episodes = _episodes((3, 2), 0)
    results = []
    for use_graph in (False, True):
        agent = _plain_learner(seed=3, use_graph=use_graph, hip=dict(graph_warmup=1), ensemble_q_num=3, ensemble_q_sample=2)
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        launches = 0
        for i in range(3):
            if i == 0:
                with native.LaunchProfiler(repeat=1) as prof:
                    agent.train()
                launches = sum(_calls(prof.summary()).values())
            else:
                agent.train()
            torch.cuda.synchronize()
            np.sort(np.random.default_rng(i).standard_normal(1 << 14))         # host work between the replays
        assert launches == 2, 'the step runs the DQN-like launches'
        assert (agent._graph is not None) == use_graph, 'the DQN-like step must capture'
        results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                        agent._td_error.cpu().numpy().copy()))
        agent.close()
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)


FALLBACKS = {
    'flag_off': dict(d=(3, 2), c=0, hip=dict(fused_dqn=False)),
    'hybrid': dict(d=(3, 2), c=2),
    'width_65': dict(d=(65,), c=0),
    'curiosity': dict(d=(3, 2), c=0, kw=dict(curiosity='FORWARD'), plugin='nn_vec_full'),
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_what_the_path_does_not_cover_runs_todays_code(case):
    """each of these issues no `asac_dqn_*` launch and still trains"""
    from asac_amd import native
    from algorithm.utils.enums import convert_config_to_enum
    cfg = FALLBACKS[case]
    kw = dict(cfg.get('kw', {}))
    convert_config_to_enum(kw)
    agent = _plain_learner(cfg['d'], cfg['c'], hip=cfg.get('hip'), plugin=cfg.get('plugin', 'nn_vec'), **kw)
    for ep in _episodes(cfg['d'], cfg['c']):
        agent.put_episode(**ep)
    before = agent._params.flat.clone()
    with native.LaunchProfiler(repeat=1) as prof:
        assert agent.train() == 1
    assert not _calls(prof.summary())
    q0 = slice(*agent._params.segments['q_0'])
    assert torch.isfinite(agent._params.flat).all() and not torch.equal(before[q0], agent._params.flat[q0])
    assert torch.isfinite(agent._td_error).all()
    agent.close()


def test_an_option_runs_todays_code(golden_dir):
    """`OptionBase` switches the path off in its constructor (its own `get_dqn_like_d_y` mixes the termination in): the
    recorded DQN-like option sequence of tests/test_option_gpu.py issues no `asac_dqn_*` launch and still trains (that
    sequence compares the updated weights with the reference's)"""
    from asac_amd import native
    from tests.test_option_gpu import run_sequence
    with native.LaunchProfiler(repeat=1) as prof:
        opt, _, _ = run_sequence('dqn', golden_dir)
    assert opt._fused_dqn is False and opt.discrete_dqn_like
    assert not _calls(prof.summary())
    opt.close()


# ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    """null outputs, E_sample > E, D > 64, K > 8, a branch table that does not add up, n > 64, B > 1024 for the loss:
    hipErrorInvalidValue and no launch; B == 0 is accepted and launches nothing"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    B, n, sizes, E = 8, 3, (3, 2), 2
    c = qr.to(qr.make_case(B, n, sizes, E, E, True, seed=5), torch.float32, 'cuda', strided=True)
    D, K = c['D'], c['K']
    lib, s, bad = native.load(), native._stream(), 1      # hipErrorInvalidValue
    marker = lambda *shape: torch.full(shape, 7., device='cuda')      # noqa: E731
    y, td, loss_q, grad_q, act = marker(B), marker(B), marker(E), marker(E, B, D), marker(B, D)
    outputs = (y, td, loss_q, grad_q, act)
    u = torch.rand(B, 1 + K, device='cuda')
    p = native._p

    def ret(a, j):
        return lib.asac_dqn_return(C.byref(a), C.byref(j), s)

    def q_loss(a, j, loss=loss_q, grad=grad_q):
        return lib.asac_dqn_q_loss_grad(C.byref(a), C.byref(j), None, 0, p(loss), p(grad), s)

    def acting(br, out=act, B_=B):
        return lib.asac_dqn_act(C.byref(br), p(c['q_online'][0]), c['q_online'][0].stride(0), p(u), u.stride(0), 0.5, p(out),
                                D, B_, s)

    def args(**change):
        a = _vtrace_args(c, y, td)
        for k, v in change.items():
            setattr(a, k, v)
        return a

    def job(**change):
        j = _job(c)
        for k, v in change.items():
            setattr(j, k, v)
        return j

    ok_br, wide, nine, uneven = native.branches(sizes), native.branches((65,)), native.branches(sizes), native.branches(sizes)
    nine.K = 9
    uneven.D = D + 1
    bad_jobs = [job(branches=wide), job(branches=nine), job(branches=uneven)]
    refused = [ret(args(y_out=None), job()), ret(args(E_sample=E + 1), job()), ret(args(n=65), job())]
    refused += [ret(args(), j) for j in bad_jobs]
    refused += [q_loss(args(), job(), loss=None), q_loss(args(), job(), grad=None), q_loss(args(E_sample=E + 1), job()),
                q_loss(args(n=65), job()), q_loss(args(B=1025), job())]
    refused += [q_loss(args(), j) for j in bad_jobs]
    refused += [acting(ok_br, out=None), acting(wide), acting(nine), acting(uneven)]
    assert refused == [bad] * len(refused), refused
    assert [ret(args(B=0), job()), q_loss(args(B=0), job()), acting(ok_br, B_=0)] == [0, 0, 0]
    with pytest.raises(native.AsacNativeError):
        native.dqn_return(args(E_sample=E + 1), job())
    torch.cuda.synchronize()
    for t in outputs:
        assert (t == 7.).all(), 'nothing was launched'
    # ... and the same calls with good arguments run
    assert [ret(args(), job()), q_loss(args(), job()), acting(ok_br)] == [0, 0, 0]
    torch.cuda.synchronize()
    for t in outputs:
        assert torch.isfinite(t).all() and not (t == 7.).all()
