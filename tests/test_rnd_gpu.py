"""GPU: random network distillation with continuous actions on the native path (`hip_config['fused_rnd']`, csrc/rnd.hip):
both kernels against float64 (tests/rnd_ref.py) and against the float32 eager composition, ties, NaN, the bits shared with
the squash launches, the recorded reference function (`tests/golden/f17_rnd_pick.npz`), two recorded reference steps
(`tests/golden/f6_step_rnd_c*.npz`) through the learner with and without the launches, launch counts, the captured step, the
fallbacks, the acting statistics and the refused arguments."""
import ctypes as C
import functools
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402
from tests import rnd_ref as rr  # noqa: E402
from tests.golden.make_rnd_golden import CASES, MIN_GAP, PICK_SHAPES, SMALL  # noqa: E402

ULP = 2.0 ** -23
F = torch.nn.functional
# (B, n, S, A): a single row; rows that do not fill a tile of 16; several tiles with a ragged last one and an odd input
# width; many workgroups with the residual first block (S + A == 64); the widest input (two stacks: 101 KB of LDS)
SHAPES = [(1, 1, 6, 2), (5, 3, 6, 2), (37, 4, 7, 2), (300, 2, 61, 3), (16, 64, 100, 28)]


def _stacks(c, dev='cuda'):
    """(RndDesc, predictor RndStack, target RndStack, (device parameter tensors))"""
    from asac_amd import native
    pred = tuple(t.to(dev).contiguous() for t in c['pred'])
    targ = tuple(t.to(dev).contiguous() for t in c['targ'])
    desc = native.rnd_desc(c['S'], c['A'], rr.residual_flags(c['S'] + c['A']))
    return desc, native.rnd_stack(*pred), native.rnd_stack(*targ), pred + targ


def _stack_eager(x, w1, b1, w2, b2, r1):
    """the module code's arithmetic (`LinearLayers` of two `ResBlock`s: Linear, GELU, + input where the widths agree)"""
    z1 = F.linear(x, w1, b1)
    h1 = F.gelu(z1) + x if r1 else F.gelu(z1)
    z2 = F.linear(h1, w2, b2)
    return F.gelu(z2) + h1, h1, z1, z2


# ------------------------------------------------------------------------------------------------
# asac_rnd_distill
# ------------------------------------------------------------------------------------------------
def _distill_kernel(c, dev, masked):
    """the launch and the `xty_multi` pair on the case's strided device views, outputs pre-filled with NaN"""
    from asac_amd import native
    desc, pred, targ, keep = _stacks(c)
    N, K = c['B'] * c['n'], c['S'] + c['A']
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')      # noqa: E731
    out = dict(x_cat=nan(N, K), h1=nan(N, 64), gz1=nan(N, 64), gz2=nan(N, 64), loss=nan(1), dw1=nan(64, K), db1=nan(64),
               dw2=nan(64, 64), db2=nan(64))
    native.rnd_distill(desc, pred, targ, dev['state'], dev['action'], dev['pad'] if masked else None, out['x_cat'], out['h1'],
                       out['gz1'], out['gz2'], out['loss'])
    native.xty_multi([(out['gz2'], out['h1'], out['dw2'], out['db2']), (out['gz1'], out['x_cat'], out['dw1'], out['db1'])],
                     accumulate=False)
    out['loss'] = out['loss'].view(())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _distill_eager(c, dev, masked):
    """today's `_train_rnd` lines in float32 on the same device tensors: `torch.cat`, the stacks' module arithmetic, the
    masked MSE chain, gradients by autograd"""
    w1, b1, w2, b2 = (t.cuda().clone().requires_grad_() for t in c['pred'])
    r1 = c['S'] + c['A'] == 64
    x = torch.cat([dev['state'], dev['action']], dim=-1)
    p, h1, z1, z2 = _stack_eager(x, w1, b1, w2, b2, r1)
    with torch.no_grad():
        t = _stack_eager(x, *(q.cuda() for q in c['targ']), r1)[0]
    keep = ~(dev['pad'] if masked else torch.zeros_like(dev['pad'])).unsqueeze(-1)
    loss = torch.mean(F.mse_loss(p, t, reduction='none') * keep)
    dw1, db1, dw2, db2, gz1, gz2 = torch.autograd.grad(loss, [w1, b1, w2, b2, z1, z2])
    N = c['B'] * c['n']
    out = dict(loss=loss.detach(), h1=h1.detach().reshape(N, 64), gz1=gz1.reshape(N, 64), gz2=gz2.reshape(N, 64),
               dw1=dw1, db1=db1, dw2=dw2, db2=db2)
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _distill_case(B, n, S, A):
    """the case and its float64 reference with and without the mask (computed once)"""
    c = rr.make_distill_case(B, n, S, A, seed=B + 7 * n + S + A)
    p64, t64 = (tuple(t.double().numpy() for t in c[k]) for k in ('pred', 'targ'))
    ref = {m: rr.distill(c['state'].numpy(), c['action'].numpy(), c['pad'].numpy() if m else None, p64, t64) for m in (False, True)}
    return c, ref


def _share(tag, name, kernel, eager, ref, bad):
    assert np.isfinite(kernel).all(), f'{tag} {name}: an element was not written'
    assert kernel.shape == ref.shape, (tag, name)
    e_k, e_m = float(np.abs(kernel - ref).max()), float(np.abs(eager - ref).max())
    floor = 4 * ULP * float(np.abs(ref).max())
    bound = max(2 * e_m, floor)
    share = e_k / bound if bound > 0 else 0.
    print(f'{tag} {name}: kernel {e_k:.3e}  eager {e_m:.3e}  floor {floor:.3e}  share {share:.2f}')
    if e_k > bound:
        bad.append((tag, name, e_k, e_m, floor))
    return share


CHECKED = ('loss', 'gz1', 'gz2', 'h1', 'dw1', 'db1', 'dw2', 'db2')


@pytest.mark.parametrize('B,n,S,A', SHAPES)
def test_distill_against_float64_and_the_eager_composition(B, n, S, A):
    """`asac_rnd_distill` plus the `xty_multi` pair on strided window views, outputs pre-filled with NaN, against the float64
    restatement (tests/rnd_ref.py; tests/test_rnd_host.py pins it to float64 autograd on the module code).  One batch entry
    is wholly padded; with and without the mask.  Bound (the rule of tests/test_discrete_gpu.py): per tensor the kernel's
    largest absolute error against float64 may be at most twice that of the float32 eager composition — today's
    `_train_rnd` lines on the same device tensors, gradients by autograd — with a floor of 4 units in the last place at the
    tensor's largest magnitude.  Tensors: loss, gz1, gz2, h1 and the four parameter gradients.  Observed on MI355X:
    NOTES.md, "RND"."""
    import asac_amd  # noqa: F401
    c, refs = _distill_case(B, n, S, A)
    dev = dict(state=rr.strided(c['state'].cuda()), action=rr.strided(c['action'].cuda(), 5), pad=rr.strided(c['pad'].cuda(), 2))
    assert dev['state'].stride(1) == S + 3 and dev['action'].stride(1) == A + 5 and dev['pad'].stride(0) == n + 2
    bad, share = [], 0.
    for masked in (False, True):
        kernel, eager, ref = _distill_kernel(c, dev, masked), _distill_eager(c, dev, masked), refs[masked]
        assert np.array_equal(kernel['x_cat'], np.concatenate([c['state'].numpy(), c['action'].numpy()], -1).reshape(B * n, S + A))
        for name in CHECKED:
            share = max(share, _share(f'{(B, n, S, A)} mask={masked}', name, kernel[name], eager[name], ref[name], bad))
        if masked:      # the wholly padded entry has no cotangent
            rows = slice(B // 2 * n, B // 2 * n + n)
            assert not kernel['gz1'][rows].any() and not kernel['gz2'][rows].any()
    print(f'{(B, n, S, A)}: largest share of the bound {share:.2f}')
    assert not bad, bad


def test_distill_with_every_row_padded():
    """loss 0, every cotangent and gradient 0, nothing NaN; the hidden activations are still the forward's"""
    import asac_amd  # noqa: F401
    c, _ = _distill_case(5, 3, 6, 2)
    dev = dict(state=rr.strided(c['state'].cuda()), action=rr.strided(c['action'].cuda()), pad=torch.ones(5, 3, dtype=torch.bool, device='cuda'))
    out = _distill_kernel(c, dev, True)
    for name in ('loss', 'gz1', 'gz2', 'dw1', 'db1', 'dw2', 'db2'):
        assert not out[name].any() and np.isfinite(out[name]).all(), name
    assert np.isfinite(out['h1']).all() and out['h1'].any()


def test_distill_twice_gives_the_same_bits_and_leaves_its_workspace_zero():
    import asac_amd  # noqa: F401
    from asac_amd import native
    c, _ = _distill_case(300, 2, 61, 3)
    dev = dict(state=c['state'].cuda(), action=c['action'].cuda(), pad=c['pad'].cuda())
    a, b = _distill_kernel(c, dev, True), _distill_kernel(c, dev, True)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    ws = native.rnd_distill_workspace(torch.device('cuda', torch.cuda.current_device()), 600)
    assert ws.numel() == 38 + 1 and not ws[-1:].view(torch.int32).any(), 'the arrival counter is left at zero'


# ------------------------------------------------------------------------------------------------
# asac_rnd_pick
# ------------------------------------------------------------------------------------------------
def _pick_case(batch, k, S, A, seed):
    gen = torch.Generator().manual_seed(seed)
    c = dict(S=S, A=A, batch=batch, k=k)
    c['state'] = torch.randn(batch, S, generator=gen)
    ls = torch.cat([0.5 * torch.randn(batch, A, generator=gen), 0.2 + torch.rand(batch, A, generator=gen)], dim=-1)
    c['ls'], c['eps'] = ls, torch.randn(batch, k, A, generator=gen)
    c['pred'], c['targ'] = rr.make_stack(S, A, gen), rr.make_stack(S, A, gen)
    return c


def _pick_kernel(c, eps=None, state=None):
    from asac_amd import native
    desc, pred, targ, keep = _stacks(c)
    batch, k, A = c['batch'], c['k'], c['A']
    ls = c['ls'].cuda()
    eps = (c['eps'] if eps is None else eps).cuda()
    state = rr.strided(c['state'].cuda()) if state is None else state
    out = dict(action=torch.full((batch, A), float('nan'), device='cuda'), prob=torch.full((batch, A), float('nan'), device='cuda'),
               err=torch.full((batch, k), float('nan'), device='cuda'), index=torch.full((batch,), -1, dtype=torch.int32, device='cuda'))
    native.rnd_pick(desc, pred, targ, state, ls[:, :A], ls[:, A:], eps, out['action'], out['prob'], out['err'], out['index'])
    return out


def _pick_eager_err(c):
    """today's `rnd_sample_c_action` lines in float32 on the device: tanh of the candidates, `repeat_interleave`, the two
    stacks' module arithmetic on the concatenation, `pow` / `sum`"""
    A, k = c['A'], c['k']
    ls, eps = c['ls'].cuda(), c['eps'].cuda()
    acts = torch.tanh(ls[:, None, :A] + ls[:, None, A:] * eps)
    x = torch.cat([torch.repeat_interleave(c['state'].cuda().unsqueeze(1), k, dim=1), acts], dim=-1)
    r1 = c['S'] + A == 64
    p = _stack_eager(x, *(t.cuda() for t in c['pred']), r1)[0]
    t = _stack_eager(x, *(t.cuda() for t in c['targ']), r1)[0]
    return torch.sum(torch.pow(p - t, 2), dim=-1).cpu().numpy()


def _squash_launches(ls, eps, A):
    """`native.squash_sample_fwd` + `native.squash_prob`, as `_choose_action`'s fast path issues them"""
    from asac_amd import native
    batch = ls.shape[0]
    loc, scale = ls[:, :A], ls[:, A:]
    a, prob = torch.empty(batch, A, device='cuda'), torch.empty(batch, A, device='cuda')
    native.squash_sample_fwd(loc, scale, eps, a, torch.empty(batch, device='cuda'))
    win = lambda t: t.as_strided((batch, 1, A), (t.stride(0), t.stride(0), 1))  # noqa: E731
    native.squash_prob(win(loc), win(scale), win(a), 0, win(prob), 0)
    return a, prob


def _prob_of(c, action):
    from asac_amd import native
    batch, A = action.shape
    ls = c['ls'].cuda()
    prob = torch.empty(batch, A, device='cuda')
    win = lambda t: t.as_strided((batch, 1, A), (t.stride(0), t.stride(0), 1))  # noqa: E731
    native.squash_prob(win(ls[:, :A]), win(ls[:, A:]), win(action.contiguous()), 0, win(prob), 0)
    return prob


@pytest.mark.parametrize('k', [1, 10, 50])
@pytest.mark.parametrize('batch', [1, 37, 300])
def test_pick_against_float64_and_the_eager_composition(batch, k):
    """`asac_rnd_pick` at the headline widths (S 6, A 2), strided states, loc / scale the halves of one [batch, 2A] tensor,
    outputs pre-filled.  The candidates' errors under the bound of the distillation test (eager: today's
    `rnd_sample_c_action` lines on the device).  Where the float64 margin between a row's two largest errors is at least
    `MIN_GAP` of the largest, the index equals tests/rnd_ref.pick's and the action is its candidate to 1e-6 (tanhf and the
    rounding of loc + scale * eps: a few units in the last place of a value below one).  The probability carries the bits
    of `asac_squash_prob` on the chosen action; with k = 1 action and probability are bit-equal to
    `native.squash_sample_fwd` + `native.squash_prob` on the same eps.  Two runs are bit-identical."""
    import asac_amd  # noqa: F401
    S, A = 6, 2
    c = _pick_case(batch, k, S, A, seed=batch + k)
    p64, t64 = (tuple(t.double().numpy() for t in c[name]) for name in ('pred', 'targ'))
    ref = rr.pick(c['state'].numpy(), c['ls'][:, :A].numpy(), c['ls'][:, A:].numpy(), c['eps'].numpy(), p64, t64)
    out, again = _pick_kernel(c), _pick_kernel(c)
    for name in out:
        assert torch.equal(out[name], again[name]), f'{name}: two runs differ'
    bad = []
    share = _share(f'pick {(batch, k)}', 'err', out['err'].cpu().numpy(), _pick_eager_err(c), ref['err'], bad)
    print(f'pick {(batch, k)}: share of the bound {share:.2f}')
    assert not bad, bad
    index = out['index'].cpu().numpy().astype(np.int64)
    assert ((index >= 0) & (index < k)).all()
    safe = rr.margin(ref['err']) >= MIN_GAP
    assert safe.mean() > 0.9 or k == 1
    assert np.array_equal(index[safe], ref['index'][safe])
    np.testing.assert_allclose(out['action'].cpu().numpy()[safe], ref['action'][safe], rtol=0, atol=1e-6)
    # the chosen action IS one of the device's candidates, and its probability asac_squash_prob's
    assert torch.equal(out['prob'], _prob_of(c, out['action']))
    # first maximum of the device's own errors
    err = out['err'].cpu()
    assert torch.equal(torch.argmax(err, dim=1).to(torch.int32), out['index'].cpu())
    if k == 1:
        a, prob = _squash_launches(c['ls'].cuda(), c['eps'].cuda()[:, 0].contiguous(), A)
        assert torch.equal(out['action'], a) and torch.equal(out['prob'], prob)


@pytest.mark.parametrize('c_id', range(len(PICK_SHAPES)))
def test_pick_replays_the_recorded_reference_function(golden_dir, c_id):
    """`tests/golden/f17_rnd_pick.npz` (the reference's own `rnd_sample_c_action`; every row keeps the margin): the indices
    are equal, errors and actions agree to float32 rounding.  The third case has S + A == 64 (residual first block)."""
    import asac_amd  # noqa: F401
    from tests.test_rnd_host import fixture_stacks
    g = np.load(golden_dir / 'f17_rnd_pick.npz')
    batch, k, S, A = PICK_SHAPES[c_id]
    pred, targ = fixture_stacks(g, c_id)
    k_ = lambda name: torch.from_numpy(g[f'c{c_id}/{name}'])      # noqa: E731
    c = dict(S=S, A=A, batch=batch, k=k, state=k_('state'), ls=torch.cat([k_('loc'), k_('scale')], dim=-1), eps=k_('eps'),
             pred=tuple(torch.from_numpy(p).float() for p in pred), targ=tuple(torch.from_numpy(p).float() for p in targ))
    out = _pick_kernel(c)
    assert np.array_equal(out['index'].cpu().numpy().astype(np.int64), g[f'c{c_id}/index'])
    want = g[f'c{c_id}/err']
    np.testing.assert_allclose(out['err'].cpu().numpy(), want, rtol=0, atol=2e-5 * float(np.abs(want).max()))
    np.testing.assert_allclose(out['action'].cpu().numpy(), g[f'c{c_id}/action'], rtol=0, atol=1e-6)


def test_pick_ties_and_nan():
    """two identical candidates placed at the maximum: the lower index wins; a NaN candidate wins over every finite error,
    the first of two NaN candidates over the second (`torch.argmax`)"""
    import asac_amd  # noqa: F401
    batch, k, S, A = 37, 10, 6, 2
    c = _pick_case(batch, k, S, A, seed=5)
    first = _pick_kernel(c)['index'].cpu().long()
    eps = c['eps'].clone()
    other = (first + 3) % k
    rows = torch.arange(batch)
    eps[rows, other] = eps[rows, first]
    out = _pick_kernel(c, eps=eps)
    err = out['err'].cpu()
    assert torch.equal(err[rows, other], err[rows, first]), 'equal candidates give equal bits wherever they lie in a tile'
    assert torch.equal(out['index'].cpu().long(), torch.minimum(first, other))
    assert (other < first).any() and (other > first).any()
    # NaN
    eps = c['eps'].clone()
    where = torch.arange(batch) % k
    eps[rows, where, 0] = float('nan')
    eps[0, k - 1, 1] = float('nan')          # row 0: a second NaN candidate behind the first
    out = _pick_kernel(c, eps=eps)
    assert torch.equal(out['index'].cpu().long(), where)
    assert torch.isnan(out['action'][:, 0]).all() and torch.isnan(out['err'].cpu()[rows, where]).all()


def test_acting_statistics():
    """batch 4096, k = 10, draws from `DeviceNoise`: the chosen index is not uniformly 0, every index occurs, and the chosen
    action is candidate `index` of `native.squash_sample_fwd` on the same draws, bit for bit"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused import DeviceNoise
    batch, k, S, A = 4096, 10, 6, 2
    c = _pick_case(batch, k, S, A, seed=9)
    eps = torch.empty(batch, k, A, device='cuda')
    DeviceNoise(seed=5).normal_(eps)
    out = _pick_kernel(c, eps=eps)
    index = out['index'].cpu().long()
    counts = np.bincount(index.numpy(), minlength=k)
    print('chosen index counts', counts)
    assert (counts > 0).all() and counts[0] < batch // 2
    ls = c['ls'].cuda()
    rep = torch.repeat_interleave(ls, k, dim=0)                    # [batch * k, 2A]
    cand = torch.empty(batch * k, A, device='cuda')
    native.squash_sample_fwd(rep[:, :A], rep[:, A:], eps.view(batch * k, A), cand, torch.empty(batch * k, device='cuda'))
    assert torch.equal(out['action'].cpu(), cand.view(batch, k, A).cpu()[torch.arange(batch), index])


# ------------------------------------------------------------------------------------------------
# the learner
# ------------------------------------------------------------------------------------------------
def _learner(case, golden_dir=None, cls=None, **hip):
    """the case's learner (tests/golden/make_rnd_golden.CASES) with the fixture's weights and episodes if `golden_dir` is
    given -> (agent, fixture | None)"""
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    plugin_name, kw = CASES[case]
    kw = dict(kw)
    convert_config_to_enum(kw)
    agent = (cls or SAC_Base)(['vector'], [(6,)], [], 2, None, pu.plugin(plugin_name), device='cuda:0',
                              batch_size=SMALL['batch_size'], replay_config={'capacity': SMALL['capacity']},
                              hip_config=hip, **kw)
    if golden_dir is None:
        return agent, None
    g = np.load(golden_dir / f'f6_step_{case}.npz')
    pu.load_golden_weights(agent, g)
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    return agent, g


def _calls(summary, prefix='asac_rnd_'):
    return {k: v['calls'] for k, v in summary.items() if k.startswith(prefix)}


# the call-site defaults of tests/test_sac_aux_gpu.py
OBSERVABLES = {'loss_q': dict(rtol=2e-4, atol=0.), 'td_error': dict(rtol=2e-4, atol=2e-5), 'tree': dict(rtol=2e-4, atol=1e-6)}


def _s_dense_state(agent):
    """bit copies of the predictor's `s_dense` weights and of their Adam moments"""
    opt, out = agent.optimizer_rnd, []
    for p in agent.model_rnd.s_dense.parameters():
        off = (p.data_ptr() - agent._params.flat.data_ptr()) // 4
        out += [p.detach().clone(), opt.exp_avg[off:off + p.numel()].clone(), opt.exp_avg_sq[off:off + p.numel()].clone()]
    return out


def _run_fixture(case, golden_dir, fused):
    """the fixture's steps through the learner -> ({observable: (|error|, scale) of step 0}, [failures])"""
    from algorithm.fused import RecordedNoise
    from asac_amd import native
    agent, g = _learner(case, golden_dir, cls=pu.hooked_learner(), use_graph=False, fused_rnd=fused)
    rb = agent.replay_buffer
    mods = {name: m for name, m in agent.ckpt_dict.items() if isinstance(m, torch.nn.Module)}
    n_steps = int(g['n_steps'])
    step_box, failures, errors0 = [0], [], {}
    s_dense0 = _s_dense_state(agent)

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
        eps = [g[f'step{s}/eps{j}'] for j in range(int(g[f'step{s}/n_eps']))]
        agent.noise = RecordedNoise([g[f'step{s}/u']], eps, list(g[f'step{s}/perm']))
        rb.uniform_source = agent.noise
        with native.LaunchProfiler(repeat=1) as prof:
            assert agent.train() == s + 1
        calls = _calls(prof.summary())
        assert calls == ({'asac_rnd_distill': 1} if fused else {}), calls
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
            assert any(k.startswith('g0/optimizer_rnd/') for k in g.files)       # the `rnd` span is among the gradients checked
            soft(lambda: pu.assert_first_step_gradients(agent, g, rtol=2e-3, atol_frac=5e-5), 'first-step gradients')
    soft(lambda: pu.assert_weights_close(mods, g, n_steps, 3e-4, rtol=1e-3, atol=2e-5), 'weights')
    for a, b in zip(s_dense0, _s_dense_state(agent)):
        assert torch.equal(a, b), 's_dense: weights and moments stay bit-unchanged'
    c0 = agent.model_rnd.c_dense.dense[0].linear.weight
    assert not np.array_equal(c0.detach().cpu().numpy(), g['w0/model_rnd/c_dense.dense.0.linear.weight']), 'c_dense trains'
    rb.check_health()
    agent.close()
    return errors0, failures


@pytest.mark.parametrize('case', list(CASES))
def test_step_against_the_reference_fixture(golden_dir, case):
    """The recorded reference steps through `SAC_Base(..., hip_config={'use_graph': False})` with `RecordedNoise`, as
    tests/test_dqn_gpu.py does: PER ids bit-exact, every recorded draw consumed; loss_q, td_error and tree, the first
    step's gradients (the `rnd` span among them) and the weights after the steps under the call-site defaults of
    tests/test_sac_aux_gpu.py.  The same steps run with `fused_rnd=False`, which must meet the defaults by itself; for step
    0 each observable's error under the launches may be at most twice that of the eager path, floor 4 units in the last
    place at the observable's largest magnitude.  `s_dense` weights and Adam moments stay bit-unchanged."""
    fused_err, fused_failures = _run_fixture(case, golden_dir, True)
    eager_err, eager_failures = _run_fixture(case, golden_dir, False)
    bad = []
    for name in OBSERVABLES:
        (e_f, scale), (e_e, _) = fused_err[name], eager_err[name]
        floor = 4 * ULP * scale
        print(f'{case} step 0 {name}: fused {e_f:.3e}  eager {e_e:.3e}  floor {floor:.3e}')
        if e_f > max(2 * e_e, floor):
            bad.append((name, e_f, e_e, floor))
    assert not eager_failures, ('the eager RND path misses its own defaults', eager_failures)
    assert not fused_failures, fused_failures
    assert not bad, bad


def _acting_inputs(agent, batch=7, seed=3):
    rng = np.random.default_rng(seed)
    obs = [rng.standard_normal((batch, 6)).astype(np.float32)]
    pre_action = np.zeros((batch, agent.d_action_summed_size + agent.c_action_size), dtype=np.float32)
    hidden = np.zeros((batch, *agent.seq_hidden_state_shape), dtype=np.float32)
    return obs, pre_action, hidden


def test_launch_counts(golden_dir):
    """one eager step records exactly one `asac_rnd_distill` and exactly one `xty_multi` call inside `_train_rnd`; one
    `choose_action` in train mode exactly one `asac_rnd_pick` behind one policy forward; with the flag off no
    `asac_rnd_*` call at all.  (Fails without the launches.)"""
    from asac_amd import native
    for fused in (True, False):
        agent, _ = _learner('rnd_c', golden_dir, use_graph=False, fused_rnd=fused)
        inner = {}
        train_rnd = agent._train_rnd

        def spy(*a, **k):
            before = {name: len(v) for name, v in prof.records.items()}
            out = train_rnd(*a, **k)
            inner.update({name: len(v) - before.get(name, 0) for name, v in prof.records.items()})
            return out

        agent._train_rnd = spy
        torch.manual_seed(0)
        with native.LaunchProfiler(repeat=1) as prof:
            agent.train()
        seen = prof.summary()
        assert _calls(seen) == ({'asac_rnd_distill': 1} if fused else {}), seen.keys()
        inner = {k: v for k, v in inner.items() if v}
        if fused:       # the distillation launch, ONE xty_multi call, the optimizer's launch and nothing else
            assert inner.pop('asac_rnd_distill') == 1 and inner.pop('asac_xty_multi') == 1, inner
            assert set(inner) <= {'asac_adam_step'}, inner
        else:
            assert not any(k.startswith('asac_rnd_') for k in inner)
        with native.LaunchProfiler(repeat=1) as prof:
            action, prob, _ = agent.choose_action(*_acting_inputs(agent))
        seen = prof.summary()
        assert _calls(seen) == ({'asac_rnd_pick': 1} if fused else {}), seen.keys()
        if fused:
            assert seen['asac_mlp_forward']['calls'] == 1 and not any(k.startswith('asac_squash') for k in seen)
        assert action.shape == (7, 2) and prob.shape == (7, 2) and np.isfinite(action).all() and (np.abs(action) <= 1).all()
        assert np.isfinite(prob).all() and (prob > 0).all()
        agent.set_train_mode(False)         # outside train mode RND plays no part: the squash launches, flag on or off
        with native.LaunchProfiler(repeat=1) as prof:
            agent.choose_action(*_acting_inputs(agent))
        assert not _calls(prof.summary())
        with native.LaunchProfiler(repeat=1) as prof:
            agent.choose_action(*_acting_inputs(agent), force_rnd_if_available=True)
        assert _calls(prof.summary()) == ({'asac_rnd_pick': 1} if fused else {})
        agent.close()


def _plain_learner(d_sizes=(), c_size=2, seed=0, use_graph=False, hip=None, plugin='nn_vec_full', **kw):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(seed), np.random.seed(seed), random.seed(seed)
    kw.setdefault('use_rnd', True)
    nn = pu.plugin(plugin) if isinstance(plugin, str) else plugin
    return SAC_Base(['vector'], [(6,)], list(d_sizes), c_size, None, nn, device='cuda:0', n_step=3,
                    batch_size=16, replay_config={'capacity': 256}, hip_config={'use_graph': use_graph, **(hip or {})}, **kw)


def _headline_plugin():
    """nn_vec (the headline learner: concatenated-vector state, stock critics and policy) with the stock `ModelRND`"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    return types.SimpleNamespace(ModelRep=m.ModelSimpleRep, ModelQ=m.ModelQ, ModelPolicy=m.ModelPolicy, ModelRND=m.ModelRND)


def _episodes(d_sizes, c_size, hidden=(0,)):
    rng = np.random.default_rng(1)
    return [pu.synthetic_episode(rng, [(6,)], list(d_sizes), c_size, hidden, T_) for T_ in (60, 45, 70)]


def test_captured_step_matches_eager():
    """the pattern of tests/test_dqn_gpu.py::test_captured_step_matches_eager: three `train()` calls — eager, and capture +
    replay + replay with host work in between — leave the same parameters, tree and TD errors (the launches allocate
    nothing once their buffers exist and synchronise nothing, so they are nodes of the step's graph)"""
    from asac_amd import native
    episodes = _episodes((), 2)
    results = []
    for use_graph in (False, True):
        agent = _plain_learner(seed=3, use_graph=use_graph, hip=dict(graph_warmup=1), plugin=_headline_plugin())
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
        assert launches == 1, 'the step runs the distillation launch'
        assert (agent._graph is not None) == use_graph, 'the RND step must capture'
        results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                        agent._td_error.cpu().numpy().copy()))
        agent.close()
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)


def _narrow_plugin():
    """nn_vec_full with a `ModelRND` of width 32 (a plugin's `_build_model` override)"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    base = pu.plugin('nn_vec_full')

    class ModelRND(m.ModelRND):
        def _build_model(self):
            return super()._build_model(dense_n=32)

    ns = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if k.startswith('Model')})
    ns.ModelRND = ModelRND
    return ns


FALLBACKS = {
    'flag_off': dict(hip=dict(fused_rnd=False)),
    'hybrid': dict(d=(3,), c=2),
    'pure_discrete': dict(d=(3, 2), c=0),
    'dqn_like': dict(d=(3, 2), c=0, kw=dict(discrete_dqn_like=True)),
    'n_sample_65': dict(kw=dict(rnd_n_sample=65)),
    'width_32': dict(plugin=_narrow_plugin),
    'action_noise': dict(kw=dict(action_noise=[0.1, 0.2]), acting_only=True),
    'disable_sample': dict(acting=dict(disable_sample=True), acting_only=True),
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_what_the_path_does_not_cover_runs_todays_code(case):
    """each of these issues no `asac_rnd_*` launch where it applies (`acting_only`: in `choose_action`; the others in the
    step as well) and still trains and acts"""
    from asac_amd import native
    cfg = FALLBACKS[case]
    d, c = cfg.get('d', ()), cfg.get('c', 2)
    plugin = cfg.get('plugin', 'nn_vec_full')
    agent = _plain_learner(d, c, hip=cfg.get('hip'), plugin=plugin() if callable(plugin) else plugin, **cfg.get('kw', {}))
    for ep in _episodes(d, c):
        agent.put_episode(**ep)
    rnd0 = slice(*agent._params.segments['rnd'])
    before = agent._params.flat.clone()
    with native.LaunchProfiler(repeat=1) as prof:
        assert agent.train() == 1
    calls = _calls(prof.summary())
    assert calls == ({'asac_rnd_distill': 1} if cfg.get('acting_only') else {}), calls
    assert torch.isfinite(agent._params.flat).all() and not torch.equal(before[rnd0], agent._params.flat[rnd0])
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, _ = agent.choose_action(*_acting_inputs(agent), **cfg.get('acting', {}))
    assert not _calls(prof.summary())
    assert np.isfinite(action).all() and np.isfinite(prob).all()
    agent.close()


def test_an_option_runs_todays_code():
    """an `OptionBase` (`_plain_learner = False`) with `use_rnd=True` and continuous actions: neither its acting nor its
    `_train_rnd` issues an `asac_rnd_*` launch"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    from algorithm.oc.option_base import OptionBase
    from asac_amd import native
    base = pu.plugin('nn_oc')
    ns = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if k.startswith('Model')})
    ns.ModelRND = m.ModelRND
    torch.manual_seed(0)
    opt = OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [], 2, None, ns, device='cuda:0', batch_size=16,
                     summary_path=None, n_step=3, use_rnd=True)
    assert opt._rnd_fused(rows=48) is None and type(opt)._plain_learner is False
    dev = opt.device
    obs = [torch.randn(7, 6, device=dev)]
    before = opt.model_rnd.c_dense.dense[0].linear.weight.detach().clone()
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, _, _ = opt.choose_action(obs, torch.zeros(7, 2, device=dev),
                                               torch.zeros(7, *opt.seq_hidden_state_shape, device=dev))
        opt._train_rnd(torch.zeros(16, 3, dtype=torch.bool, device=dev), torch.randn(16, 3, opt.state_size, device=dev),
                       torch.rand(16, 3, 2, device=dev))
    assert not _calls(prof.summary())
    assert torch.isfinite(action).all() and torch.isfinite(prob).all()
    assert not torch.equal(before, opt.model_rnd.c_dense.dense[0].linear.weight)
    opt.close()


# ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    """misaligned parameters, k = 0 or k = 65, in = 129, a residual first block at another width, a NULL required pointer:
    hipErrorInvalidValue and no launch; B == 0 / batch == 0 are accepted and launch nothing"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    B, n, S, A, k = 4, 3, 6, 2, 5
    c = rr.make_distill_case(B, n, S, A, seed=1)
    desc, pred, targ, keep = _stacks(c)
    lib, s, bad, p = native.load(), native._stream(), 1, native._p      # 1: hipErrorInvalidValue
    N, K = B * n, S + A
    marker = lambda *shape: torch.full(shape, 7., device='cuda')      # noqa: E731
    x_cat, h1, gz1, gz2, loss = marker(N, K), marker(N, 64), marker(N, 64), marker(N, 64), marker(1)
    action, prob, err = marker(B, A), marker(B, A), marker(B, k)
    outputs = (x_cat, h1, gz1, gz2, loss, action, prob, err)
    state, act, pad = c['state'].cuda(), c['action'].cuda(), c['pad'].cuda()
    ls = torch.cat([torch.randn(B, A), torch.rand(B, A) + 0.2], -1).cuda()
    eps = torch.randn(B, k, A, device='cuda')
    ws = torch.zeros(8, device='cuda')
    # a predictor whose first matrix starts 4 bytes off a 16-byte boundary
    off = torch.zeros(64 * K + 1, device='cuda')[1:].view(64, K)
    skew = native.RndStack()
    skew.w1, skew.b1, skew.w2, skew.b2 = off.data_ptr(), pred.b1, pred.w2, pred.b2
    null = native.RndStack()
    null.w1, null.b1, null.w2, null.b2 = pred.w1, None, pred.w2, pred.b2

    def distill(d=desc, pr=pred, tg=targ, st=state, B_=B, x=x_cat, h=h1, lo=loss, w=ws):
        return lib.asac_rnd_distill(C.byref(d), C.byref(pr), C.byref(tg), p(st), st.stride(0), st.stride(1), p(act), act.stride(0),
                                    act.stride(1), p(pad), pad.stride(0), pad.stride(1), B_, n, p(x), p(h), p(gz1), p(gz2),
                                    p(lo) if lo is not None else None, p(w) if w is not None else None, s)

    def pick(d=desc, pr=pred, tg=targ, k_=k, batch=B, a=action, e=eps):
        return lib.asac_rnd_pick(C.byref(d), C.byref(pr), C.byref(tg), p(state[:, 0]), state.stride(0), p(ls[:, :A]), p(ls[:, A:]),
                                 ls.stride(0), p(e) if e is not None else None, k_, batch, p(a) if a is not None else None,
                                 p(prob), p(err), None, s)

    wide, res = native.rnd_desc(125, 4), native.rnd_desc(S, A, (True, True))
    h_off = torch.zeros(N * 64 + 1, device='cuda')[1:]
    refused = [distill(pr=skew), distill(tg=skew), distill(pr=null), distill(d=wide), distill(d=res), distill(lo=None),
               distill(w=None), distill(h=h_off), distill(d=native.rnd_desc(S, 65)), distill(B_=-1)]
    refused += [pick(pr=skew), pick(tg=null), pick(k_=0), pick(k_=65), pick(d=wide), pick(d=res), pick(a=None), pick(e=None)]
    assert refused == [bad] * len(refused), refused
    assert [distill(B_=0), pick(batch=0)] == [0, 0]
    assert not native.rnd_sizes_ok(125, 4) and not native.rnd_sizes_ok(S, A, 65) and not native.rnd_sizes_ok(S, A, 0)
    torch.cuda.synchronize()
    for t in outputs:
        assert (t == 7.).all(), 'nothing was launched'
    assert [distill(), pick()] == [0, 0]          # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    for t in outputs:
        assert torch.isfinite(t).all() and not (t == 7.).all()
    assert not ws.view(torch.int32)[1:2].any(), 'the arrival counter (behind one workgroup sum) is zero again'
