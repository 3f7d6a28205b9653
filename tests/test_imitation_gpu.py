"""GPU: behaviour cloning (`algorithm/imitation_base.ImitationBase`, csrc/imitation.hip).

  * `asac_bc_loss_grad` alone against float64 `torch.distributions.Normal` autograd: value, gradients, exact zeros behind
    `t_valid`, bit-identical repeats, the raw-head form against the stock policy's head in float64
  * every reference fixture `f14_imitation_<case>.npz`: six steps from the recorded weights — every loss, the step-1 and
    step-6 parameters, Adam's moments — at the f6 full-step bounds of tests/test_sac_step_gpu.py (`TOL`); an observable
    that has no bound there, or whose step-2-to-6 error does not hold it, is bounded by 4x the error recorded on the
    MI355X (`tests/imitation_tolerances.json`)
  * captured against eager, the buckets and their graphs, padded against unpadded, what an imitation step must leave
    alone, a SAC step after an imitation step, persistence of the optimizer state"""
import io
import json
import random
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402

LR = 3e-4
# the f6 step bounds (tests/test_sac_step_gpu.py TOL): observable -> (rtol, atol)
TOL = {'loss_policy': (2e-4, 2e-5), 'grad0': (2e-3, 2e-5), 'weights': (5e-4, 2e-5)}
# case -> (plugin under tests.plugins, learner keywords, discrete action sizes)
F14 = {
    'mlp': ('nn_vec', {}, ()),
    'rnn': ('nn_rnn', dict(seq_encoder='RNN'), ()),
    'attn': ('nn_attn_tanh', dict(seq_encoder='ATTN'), ()),
    'hybrid': ('nn_vec', {}, (3, 2)),
}
MEASURED = json.loads((Path(__file__).resolve().parent / 'imitation_tolerances.json').read_text())


def make_learner(case, use_graph=False, hip=None):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    plugin_name, kw, d_sizes = F14[case]
    kw = dict(kw)
    convert_config_to_enum(kw)
    return SAC_Base(['vector'], [(6,)], list(d_sizes), 2, None, pu.plugin(plugin_name), device='cuda:0', batch_size=32,
                    replay_config={'capacity': 512}, hip_config={'use_graph': use_graph, **(hip or {})}, **kw)


def fixture_episodes(g):
    return [([g[f'ep{i}/obs_0']], g[f'ep{i}/ep_actions'], g[f'ep{i}/ep_rewards'], g[f'ep{i}/ep_dones'])
            for i in range(int(g['n_episodes']))]


def reference_autograd(loc, scale, action, dsum, tv, coef):
    """float64 Normal autograd over the first tv rows -> (loss, dloc [Tp, A], dscale [Tp, A])"""
    A = loc.shape[1]
    l64 = loc[:tv].double().cpu().requires_grad_(True)
    s64 = scale[:tv].double().cpu().requires_grad_(True)
    dist = torch.distributions.Normal(l64, s64)
    loss = torch.mean(-dist.log_prob(action[:tv, dsum:dsum + A].double().cpu()) - coef * dist.entropy())
    loss.backward()
    pad = torch.zeros(loc.shape[0] - tv, A, dtype=torch.float64)
    return loss.detach(), torch.cat([l64.grad, pad]), torch.cat([s64.grad, pad])


# ------------------------------------------------------------------------------------------------
# the kernel alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dsum', [0, 3])
@pytest.mark.parametrize('A', [1, 2, 7])
@pytest.mark.parametrize('T', [1, 5, 64, 1000, 4096])
def test_kernel_against_float64_normal_autograd(T, A, dsum):
    from asac_amd import native
    from algorithm.imitation_base import bucket_length
    Tp = bucket_length(T)
    g = torch.Generator().manual_seed(T * 31 + A * 7 + dsum)
    loc = torch.randn(Tp, A, generator=g).cuda()
    scale = (torch.rand(Tp, A, generator=g) * 1.5 + 0.05).cuda()
    action = (torch.rand(Tp, dsum + A, generator=g) * 2 - 1).cuda()
    for tv in sorted({T, max(1, T // 2), Tp}):
        t_valid = torch.tensor([tv], dtype=torch.int32, device='cuda')
        outs = []
        for _ in range(2):
            loss = torch.full((1,), float('nan'), device='cuda')
            dloc, dscale = torch.full_like(loc, float('nan')), torch.full_like(scale, float('nan'))
            native.bc_loss_grad(loc, scale, action, dsum, t_valid, 0.1, loss, dloc, dscale)
            outs.append((loss.cpu(), dloc.cpu(), dscale.cpu()))
        for a, b in zip(*outs):       # same input, same bits
            assert torch.equal(a, b)
        loss, dloc, dscale = outs[0]
        assert (dloc[tv:] == 0).all() and (dscale[tv:] == 0).all()
        want, wl, ws = reference_autograd(loc, scale, action, dsum, tv, 0.1)
        # f32 arithmetic on f32 inputs against f64: a few ulp per element, sqrt(n) growth of the sum at most
        torch.testing.assert_close(loss.double()[0], want, rtol=2e-5, atol=1e-6)
        torch.testing.assert_close(dloc.double(), wl, rtol=2e-5, atol=1e-9)
        torch.testing.assert_close(dscale.double(), ws, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize('T,A', [(5, 2), (300, 4)])
def test_kernel_raw_head_form(T, A):
    """(mean | logstd) halves of one [Tp, 2A] buffer: the head of nn_models/policy.py:169 inside the launch, clamp edges
    included; gradients with respect to the raw values, written into the halves of one [Tp, 2A] buffer"""
    from asac_amd import native
    from algorithm.imitation_base import bucket_length
    Tp = bucket_length(T)
    g = torch.Generator().manual_seed(T + A)
    raw = torch.randn(Tp, 2 * A, generator=g) * 2
    raw[0, A] = 0.9           # log-std above the clamp: no gradient
    raw[1 % T, A] = -25.      # ... and below
    action = torch.rand(Tp, A, generator=g) * 2 - 1
    raw_d, action_d = raw.cuda(), action.cuda()
    t_valid = torch.tensor([T], dtype=torch.int32, device='cuda')
    loss, grad = torch.empty(1, device='cuda'), torch.full_like(raw_d, float('nan'))
    native.bc_loss_grad(raw_d[:, :A], raw_d[:, A:], action_d, 0, t_valid, 0.1, loss, grad[:, :A], grad[:, A:], raw_head=True)
    r64 = raw[:T].double().requires_grad_(True)
    dist = torch.distributions.Normal(torch.tanh(r64[:, :A] / 5.) * 5., torch.exp(torch.clamp(r64[:, A:], -20, 0.5)))
    want = torch.mean(-dist.log_prob(action[:T].double()) - 0.1 * dist.entropy())
    want.backward()
    torch.testing.assert_close(loss.cpu().double()[0], want.detach(), rtol=2e-5, atol=1e-6)
    got = grad.cpu().double()
    assert (got[T:] == 0).all()
    # exp(-20) as a scale puts 1e17-sized terms into that row's gradient: relative comparison only
    torch.testing.assert_close(got[:T], r64.grad, rtol=5e-5, atol=1e-9)
    assert got[0, A] == 0 and got[1 % T, A] == 0


def test_autograd_function_behind_a_plain_normal():
    from algorithm.imitation_base import bc_loss
    g = torch.Generator().manual_seed(9)
    loc = torch.randn(1, 64, 3, generator=g).cuda().requires_grad_(True)
    log_s = torch.randn(1, 64, 3, generator=g).cuda().requires_grad_(True)
    action = torch.rand(1, 64, 5, generator=g).cuda()
    dist = torch.distributions.Normal(loc, torch.exp(log_s))
    t_valid = torch.tensor([40], dtype=torch.int32, device='cuda')
    (bc_loss(dist.loc, dist.scale, action, 2, t_valid) * 3.).backward()
    l64, s64 = loc.detach().double().cpu().requires_grad_(True), log_s.detach().double().cpu().requires_grad_(True)
    d64 = torch.distributions.Normal(l64[:, :40], torch.exp(s64[:, :40]))
    (torch.mean(-d64.log_prob(action[:, :40, 2:].double().cpu()) - 0.1 * d64.entropy()) * 3.).backward()
    torch.testing.assert_close(loc.grad.double().cpu(), l64.grad, rtol=2e-5, atol=1e-9)
    torch.testing.assert_close(log_s.grad.double().cpu(), s64.grad, rtol=2e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------
# the reference's six steps
# ------------------------------------------------------------------------------------------------
def run_fixture(case, g, use_graph=False, hip=None, n=None, on_step=None):
    from algorithm.imitation_base import ImitationBase
    sac = make_learner(case, use_graph, hip)
    mods = pu.load_golden_weights(sac, g)
    imit = ImitationBase(sac)
    losses = []
    for i, ep in enumerate(fixture_episodes(g)[:n]):
        assert imit.train(*ep) == i + 1
        losses.append(float(imit.last_loss.item()))
        if on_step is not None:
            on_step(i, sac, imit, mods)
    return sac, imit, mods, losses


def bound(key, default):
    """the f6 bound, or 4x the error recorded on the MI355X where the observable has none / does not hold it"""
    rec = MEASURED.get(key)
    return default if rec is None else (rec['rtol'], rec['atol'])


def moment_errors(imit, g, which):
    """worst |got - want| / (atol + rtol |want|) in the `grad0` norm of parity_utils.assert_first_step_gradients"""
    state = imit.state_dict()['state']
    wants = [g[f'm6/{which}/{j}'] for j in range(len(state))]
    floor = pu.ZERO_GRAD_REL * max(float(np.abs(w).max()) for w in wants)
    rtol, atol_frac = TOL['grad0']
    worst = 0.
    for j, want in enumerate(wants):
        got = state[j][which].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        tol_ = atol_frac * float(np.abs(want).max()) + floor + rtol * np.abs(want)
        worst = max(worst, float((np.abs(got - want) / np.maximum(tol_, 1e-300)).max()))
    return worst


@pytest.mark.parametrize('case', list(F14))
def test_six_steps_against_the_reference(golden_dir, case):
    g = np.load(golden_dir / f'f14_imitation_{case}.npz')
    trained = tuple(n for n in ('model_rep', 'model_policy') if any(k.startswith(f'w1/{n}/') for k in g.files))
    first = {}

    def after(i, sac, imit, mods):
        if i == 0:
            try:
                pu.assert_weights_close(mods, g, 1, LR, *TOL['weights'], prefix='w_s1', only=trained)
            except AssertionError as e:
                first['error'] = e
    sac, imit, mods, losses = run_fixture(case, g, on_step=after)
    want = g['loss']
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, want)]
    print(f'\n[f14 {case}] loss relative errors: ' + ' '.join(f'{r:.3g}' for r in rel))
    m1, m2 = moment_errors(imit, g, 'exp_avg'), moment_errors(imit, g, 'exp_avg_sq')
    print(f'[f14 {case}] moments, fraction of the grad0 bound used: exp_avg {m1:.3g} exp_avg_sq {m2:.3g}')
    worst_w = 0.
    for name in trained:
        for k, v in mods[name].state_dict().items():
            w = g[f'w1/{name}/{k}']
            worst_w = max(worst_w, float(np.abs(v.detach().cpu().numpy() - w).max()))
    print(f'[f14 {case}] step-6 weights: worst |got - want| = {worst_w:.3g} (lr = {LR})')
    assert 'error' not in first, first.get('error')
    for i, (a, b) in enumerate(zip(losses, want)):
        rtol, atol = bound(f'{case}/loss/step{i}', TOL['loss_policy'])
        assert abs(a - b) <= atol + rtol * abs(b), (case, i, a, float(b))
    wr, wa = bound(f'{case}/weights6', TOL['weights'])
    pu.assert_weights_close(mods, g, 6, LR, wr, wa, only=trained)
    scale = bound(f'{case}/moments6', (1., 0.))[0]       # multiples of the grad0 bound
    assert m1 <= scale and m2 <= scale, (m1, m2, scale)
    assert int(imit.opt.steps_done.item()) == int(g['m6/step']) == 6
    # the critics and the target networks are the recorded initial ones, bit for bit
    for name, mod in mods.items():
        if name not in trained:
            for k, v in mod.state_dict().items():
                assert np.array_equal(v.detach().cpu().numpy(), g[f'w0/{name}/{k}']), (name, k)
    sac.close()


# ------------------------------------------------------------------------------------------------
# graphs, buckets, isolation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(F14))
def test_captured_steps_are_the_eager_steps_bit_for_bit(golden_dir, case):
    g = np.load(golden_dir / f'f14_imitation_{case}.npz')
    flats, moments = [], []
    for use_graph in (False, True):
        sac, imit, _, _ = run_fixture(case, g, use_graph)
        # lengths 5, 63, 64, 17 share the 64 bucket (one capture, three replays), 65 has 128, 130 has 192
        assert imit.captures == (3 if use_graph else 0)
        flats.append(sac._params.flat.clone())
        moments.append((imit.opt.exp_avg.clone(), imit.opt.exp_avg_sq.clone()))
        sac.close()
    assert torch.equal(flats[0], flats[1])
    assert torch.equal(moments[0][0], moments[1][0]) and torch.equal(moments[0][1], moments[1][1])


def test_buckets_share_and_split_graphs(golden_dir):
    from algorithm.imitation_base import ImitationBase
    g = np.load(golden_dir / 'f14_imitation_mlp.npz')
    eps = {ep[1].shape[1]: ep for ep in fixture_episodes(g)}
    sac = make_learner('mlp', use_graph=True)
    imit = ImitationBase(sac)
    imit.train(*eps[5])
    imit.train(*eps[63])
    assert imit.captures == 1 and len(imit._buckets) == 1, '5 and 63 share the 64 bucket'
    imit.train(*eps[64])
    assert imit.captures == 1
    imit.train(*eps[65])
    imit.train(*eps[65])
    assert imit.captures == 2 and len(imit._buckets) == 2, '64 and 65 use two graphs'
    sac.close()
    # the cap: the oldest bucket goes first
    sac = make_learner('mlp', use_graph=True, hip={'imitation_max_graphs': 2})
    imit = ImitationBase(sac)
    for T in (5, 65, 130):
        imit.train(*eps[T])
    assert list(imit._buckets) == [128, 192]
    sac.close()


class _AsGolden:
    """weights of one run under `prefix/`, beside the fixture's `g0/` entries: what `pu.assert_weights_close` reads"""

    def __init__(self, g, prefix, mods, names):
        self.data = {k: g[k] for k in g.files if k.startswith('g0/')}
        for n in names:
            for k, v in mods[n].state_dict().items():
                self.data[f'{prefix}/{n}/{k}'] = v.detach().cpu().numpy().copy()
        self.files = list(self.data)

    def __getitem__(self, k):
        return self.data[k]


@pytest.mark.parametrize('case', list(F14))
def test_padding_does_not_change_the_valid_rows(golden_dir, case):
    """the length-65 episode padded to 128 (captured path) against the eager unpadded path, for every representation: the
    weight bound of the reference comparison through the same helper (entries whose gradient is analytically zero —
    the attention's key-projection bias — take sign-like Adam steps from rounding noise and get the helper's 2.2 lr per
    step); bit-equality for `mlp`"""
    from algorithm.imitation_base import ImitationBase
    g = np.load(golden_dir / f'f14_imitation_{case}.npz')
    ep = [e for e in fixture_episodes(g) if e[1].shape[1] == 65][0]
    unpadded = None
    for hip, use_graph in (({'imitation_bucket': 1}, False), ({}, True)):
        sac = make_learner(case, use_graph, hip)
        mods = pu.load_golden_weights(sac, g)
        names = [n for n in ('model_rep', 'model_policy') if n in mods]
        imit = ImitationBase(sac)
        imit.train(*ep)
        imit.train(*ep)      # (the second one replays the captured graph)
        assert list(imit._buckets) == ([65] if not use_graph else [128])
        assert imit.captures == int(use_graph)
        if unpadded is None:
            unpadded = _AsGolden(g, 'pad', mods, names)
        else:
            worst = max(float(np.abs(v.detach().cpu().numpy() - unpadded[f'pad/{n}/{k}']).max())
                        for n in names for k, v in mods[n].state_dict().items())
            print(f'\n[f14 {case}] padded against unpadded: worst weight difference {worst:.3g}')
            if case == 'mlp':
                assert worst == 0.
            pu.assert_weights_close(mods, unpadded, 2, LR, *TOL['weights'], prefix='pad', only=names)
        sac.close()


def test_isolation_and_global_step(golden_dir):
    g = np.load(golden_dir / 'f14_imitation_rnn.npz')
    from algorithm.imitation_base import ImitationBase
    sac = make_learner('rnn', use_graph=True)
    pu.load_golden_weights(sac, g)
    sac._exp_avg.normal_(), sac._exp_avg_sq.uniform_(), sac._opt_steps.fill_(11)      # (anything recognisable)
    seg = sac._params.segments
    keep = [n for n in seg if n not in ('rep', 'policy')]
    before = {n: sac._params.flat[seg[n][0]:seg[n][1]].clone() for n in keep}
    target, m, v = sac._target_params.flat.clone(), sac._exp_avg.clone(), sac._exp_avg_sq.clone()
    imit = ImitationBase(sac)
    assert imit.train_episodes(fixture_episodes(g)) == 6 and sac.get_global_step() == 6
    for n in keep:          # critics, temperature
        assert torch.equal(sac._params.flat[seg[n][0]:seg[n][1]], before[n]), n
    assert torch.equal(sac._target_params.flat, target)
    assert torch.equal(sac._exp_avg, m) and torch.equal(sac._exp_avg_sq, v) and int(sac._opt_steps.item()) == 11
    assert int(imit.opt.steps_done.item()) == 6
    sac.close()


@pytest.mark.parametrize('fused_head,demo_len', [(True, 50), (False, 50), (True, 700), (False, 700)])
def test_sac_steps_after_an_imitation_step(golden_dir, fused_head, demo_len):
    """the f6_step_cfg2 inputs: SAC steps (captured after three eager ones), imitation steps, SAC steps again — the
    replayed graph reads the parameters the imitation steps left, and its own buffers are where it captured them: the
    700-step episode has more rows than the SAC step's 32 x 5, so a policy workspace sized by rows would have to grow —
    the learner's must not (a captured step holds its address).  Against the eager run of the same sequence at the
    bounds of test_sac_step_gpu.py::test_graph_replay_matches_eager"""
    from tests.test_sac_step_gpu import make_agent
    from algorithm.imitation_base import ImitationBase
    g = np.load(golden_dir / 'f6_step_cfg2.npz')
    demo = pu.synthetic_episode(np.random.default_rng(5), [(6,)], [], 2, (0,), demo_len)
    results = []
    for use_graph in (False, True):
        torch.manual_seed(3), np.random.seed(3), random.seed(3)
        agent = make_agent('cfg2', use_graph=use_graph, hip={'imitation_fused_head': fused_head})
        pu.load_golden_weights(agent, g)
        for ep in pu.golden_episodes(g):
            agent.put_episode(**ep)
        imit = ImitationBase(agent)
        assert (imit._fpi_raw is not None) == fused_head and (imit._fpi_ls is not None) == (not fused_head)
        for _ in range(5):
            agent.train()
        assert (agent._graph is not None) == use_graph
        held = {id(m): (m._workspace, m._workspace.data_ptr()) for m in (agent._fpi, agent._fq) if m._workspace is not None}
        policy_before = agent._params.flat[slice(*agent._params.span('policy'))].clone()
        for _ in range(2):
            imit.train(demo['ep_obses_list'], demo['ep_actions'], demo['ep_rewards'], demo['ep_dones'])
        assert not torch.equal(agent._params.flat[slice(*agent._params.span('policy'))], policy_before)
        for m in (agent._fpi, agent._fq):       # the learner's cached workspaces: same tensors, same addresses
            if id(m) in held:
                assert m._workspace is held[id(m)][0] and m._workspace.data_ptr() == held[id(m)][1]
        for _ in range(3):
            agent.train()
        assert agent.get_global_step() == 10
        results.append((agent.replay_buffer._tree.cpu().numpy().copy(), agent._params.flat.cpu().numpy().copy()))
        assert np.isfinite(results[-1][1]).all()
        agent.close()
    for a, b in zip(*results):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6)


def test_eviction_between_replays(golden_dir):
    """two live graphs at most: buckets are replayed, evicted and captured again in turn — the eager sequence bit for bit"""
    from algorithm.imitation_base import ImitationBase
    g = np.load(golden_dir / 'f14_imitation_rnn.npz')
    eps = {ep[1].shape[1]: ep for ep in fixture_episodes(g)}
    order = (5, 63, 65, 65, 130, 130, 17, 64, 65, 65, 130)
    flats = []
    for use_graph in (False, True):
        sac = make_learner('rnn', use_graph, hip={'imitation_max_graphs': 2})
        pu.load_golden_weights(sac, g)
        imit = ImitationBase(sac)
        for T in order:
            imit.train(*eps[T])
            assert len(imit._buckets) <= 2
        # 64, 128, 192 captured; 64 evicted by 192, captured again (evicting 128); 128 again; 192 again
        assert imit.captures == (6 if use_graph else 0) and imit.capture_failures == 0
        assert list(imit._buckets) == [128, 192]
        flats.append(sac._params.flat.clone())
        sac.close()
    assert torch.equal(flats[0], flats[1])


def test_two_observations_with_an_image(golden_dir):
    """a vector and a float image observation (the convolution plugin): every observation is staged and padded, the
    captured steps are the eager ones bit for bit and follow the PyTorch composition of the reference's lines; 8-bit
    observations are refused (the reference hands them to the representation unwidened)"""
    import asac_amd  # noqa: F401
    from itertools import chain
    from algorithm.imitation_base import ImitationBase
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.operators import gen_n_pre_actions
    io_ = pu.IMG
    rng = np.random.default_rng(8)
    eps = []
    for T in (20, 70, 33):
        ep = pu.synthetic_episode(rng, [(10,)], [], io_['c_action_size'], (0,), T)
        img = (rng.integers(0, 256, (1, T, 3, 30, 30)).astype(np.float32) / np.float32(255.))
        eps.append(([ep['ep_obses_list'][0], img], ep['ep_actions'], ep['ep_rewards'], ep['ep_dones']))

    def learner(use_graph):
        torch.manual_seed(21)
        return SAC_Base(io_['obs_names'], io_['obs_shapes'], [], io_['c_action_size'], None, pu.plugin('nn_conv'),
                        device='cuda:0', batch_size=8, replay_config={'capacity': 128}, hip_config={'use_graph': use_graph})
    flats, losses = [], []
    for use_graph in (False, True):
        sac = learner(use_graph)
        imit = ImitationBase(sac)
        for ep in eps + eps[:1]:
            imit.train(*ep)
            losses.append(float(imit.last_loss.item()))
        assert imit.captures == (2 if use_graph else 0) and imit.capture_failures == 0
        flats.append(sac._params.flat.clone())
        if use_graph:
            with pytest.raises(TypeError, match='float32'):
                imit.train([eps[0][0][0], (eps[0][0][1] * 255).astype(np.uint8)], *eps[0][1:])
        sac.close()
    assert torch.equal(flats[0], flats[1]) and np.isfinite(losses).all()
    # the reference's lines on the same modules (plain autograd, unpadded, torch.optim.Adam)
    sac = learner(False)
    opt = torch.optim.Adam(chain(sac.model_rep.parameters(), sac.model_policy.parameters()), lr=sac.learning_rate)
    want = []
    for obses, actions, _, _ in eps + eps[:1]:
        obses, actions = [torch.from_numpy(o).cuda() for o in obses], torch.from_numpy(actions).cuda()
        T = actions.shape[1]
        idx = torch.arange(T, dtype=torch.int32, device='cuda').unsqueeze(0)
        pad = torch.zeros_like(idx, dtype=torch.bool)
        pad[:, -1] = True
        hidden = sac.get_initial_seq_hidden_state(1, get_numpy=False).unsqueeze(1).repeat_interleave(T, dim=1)
        states, _ = sac.get_l_states(idx, pad, obses, gen_n_pre_actions(actions, keep_last_action=False), hidden)
        _, c_policy = sac.model_policy(states, obses)
        loss = torch.mean(-c_policy.log_prob(actions) - 0.1 * c_policy.entropy())
        opt.zero_grad(), loss.backward(), opt.step()
        want.append(float(loss.item()))
    sac.close()
    print('\n[conv] losses', losses[:4], 'composition', want)
    rtol, atol = TOL['loss_policy']
    for a, b in zip(losses[:4], want):
        assert abs(a - b) <= atol + rtol * abs(b), (losses[:4], want)


def test_state_dict_round_trip_continues_bit_for_bit(golden_dir):
    from algorithm.imitation_base import ImitationBase
    g = np.load(golden_dir / 'f14_imitation_rnn.npz')
    eps = fixture_episodes(g)
    sac, imit, _, _ = run_fixture('rnn', g, n=3)
    buf = io.BytesIO()
    torch.save(imit.state_dict(), buf)
    flat3 = sac._params.flat.clone()
    imit.train(*eps[3])
    want = sac._params.flat.clone()
    sac.close()
    sac2 = make_learner('rnn')
    sac2._params.flat.copy_(flat3)
    imit2 = ImitationBase(sac2)
    buf.seek(0)
    imit2.load_state_dict(torch.load(buf, weights_only=False))
    assert int(imit2.opt.steps_done.item()) == 3
    imit2.train(*eps[3])
    assert torch.equal(sac2._params.flat, want)
    # the reference's optimizer type loads the same file
    buf.seek(0)
    params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in imit2.opt._param_list()]
    torch.optim.Adam(params, lr=LR).load_state_dict(torch.load(buf, weights_only=False))
    sac2.close()


def test_fused_head_equals_the_general_path(golden_dir):
    """the stock policy: head transform inside the loss launch against `asac_bc_loss_grad` behind the fused network's
    (loc | scale) output — two roundings apart at most, so the weight bound applies"""
    g = np.load(golden_dir / 'f14_imitation_mlp.npz')
    flats = []
    for fused in (True, False):
        sac, imit, _, _ = run_fixture('mlp', g, hip={'imitation_fused_head': fused}, n=2)
        assert (imit._fpi_raw is not None) == fused
        flats.append(sac._params.flat.cpu().numpy().copy())
        sac.close()
    rtol, atol = TOL['weights']
    assert (np.abs(flats[0] - flats[1]) <= atol + rtol * np.abs(flats[1])).all()
