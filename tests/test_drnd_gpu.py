"""GPU: random network distillation of a pure-discrete, policy-based learner on the native path
(`hip_config['fused_rnd_discrete']`, csrc/drnd.hip): the three kernels against float64 (tests/drnd_ref.py) and against the
float32 eager composition, padding, unselected members, ties, NaN, two runs, the bits shared with the discrete policy launch,
the recorded reference function (`tests/golden/f18_drnd_pick.npz`), three recorded reference steps
(`tests/golden/f6_step_rnd_d*.npz`) through the learner with and without the launches, launch counts, the captured step, the
fallbacks, the acting statistics and the refused arguments."""
import ctypes as C
import functools
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import drnd_ref as dr  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests import rnd_ref as rr  # noqa: E402
from tests.golden.make_drnd_golden import CASES, MIN_GAP, PICK_SHAPES, SMALL  # noqa: E402
# what the two RND paths' tests share: the module code's stack arithmetic, the "twice the eager error, floor 4 ulp" report, the
# call-site defaults of the step fixtures, `s_dense`'s bit copies, acting inputs, synthetic episodes, the width-32 plugin
from tests.test_rnd_gpu import (CHECKED, OBSERVABLES, ULP, _acting_inputs, _episodes, _narrow_plugin, _s_dense_state,  # noqa: E402
                                _share, _stack_eager)

F = torch.nn.functional
# (B, n, S, sizes): one row; less than a tile; two branches, a ragged last tile and an odd S; many workgroups and the
# residual first block (S == 64); the widest S with D = 16 members in five branches
SHAPES = [(1, 1, 6, (3,)), (5, 3, 6, (3,)), (37, 4, 7, (2, 3)), (300, 2, 64, (4,)), (16, 8, 128, (5, 4, 3, 2, 2))]


def _tables(c):
    """(Branches, residual flags, predictor table, target table, the device tensors the tables point into)"""
    from asac_amd import native
    pred = [tuple(t.cuda().contiguous() for t in m) for m in c['pred']]
    targ = [tuple(t.cuda().contiguous() for t in m) for m in c['targ']]
    return native.branches(c['sizes']), dr.residual_flags(c['S']), native.drnd_table(pred), native.drnd_table(targ), (pred, targ)


# ------------------------------------------------------------------------------------------------
# asac_drnd_distill + asac_drnd_param_grads
# ------------------------------------------------------------------------------------------------
def _distill_kernel(c, dev, masked):
    """both launches on the case's strided device views, outputs pre-filled with NaN (sel with -7)"""
    from asac_amd import native
    br, flags, pred, targ, keep = _tables(c)
    N, S, K, D = c['B'] * c['n'], c['S'], br.K, br.D
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')      # noqa: E731
    out = dict(x=nan(N, S), h1=nan(N, K, 64), gz1=nan(N, K, 64), gz2=nan(N, K, 64), loss=nan(1),
               sel=torch.full((N, K), -7, dtype=torch.int32, device='cuda'))
    grads = [(nan(64, S), nan(64), nan(64, 64), nan(64)) for _ in range(D)]
    native.drnd_distill(br, flags, pred, targ, dev['state'], dev['action'], dev['pad'] if masked else None, out['sel'], out['x'],
                        out['h1'], out['gz1'], out['gz2'], out['loss'])
    native.drnd_param_grads(br, S, out['sel'], out['x'], out['h1'], out['gz1'], out['gz2'], native.drnd_table(grads))
    out['loss'] = out['loss'].view(())
    for i, name in enumerate(('dw1', 'db1', 'dw2', 'db2')):
        out[name] = torch.stack([g[i] for g in grads])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _distill_eager(c, dev, masked, sel):
    """today's `_train_rnd` lines in float32 on the same device tensors: `cal_d_rnd` of both models (every member's module
    arithmetic and a `torch.stack`), the broadcast multiply by the stored action and the sum over members, the masked MSE
    chain, gradients by autograd; the records are read out at the members `sel` names"""
    D, N, r1 = len(c['pred']), c['B'] * c['n'], c['S'] == 64
    params = [[t.cuda().clone().requires_grad_() for t in m] for m in c['pred']]
    x = dev['state']
    fwd = [_stack_eager(x, *m, r1) for m in params]
    with torch.no_grad():
        tgt = torch.stack([_stack_eager(x, *(q.cuda() for q in m), r1)[0] for m in c['targ']], dim=-2)
    a = dev['action'].unsqueeze(-1)
    d = (a * torch.stack([f[0] for f in fwd], dim=-2)).sum(-2)
    t = (a * tgt).sum(-2)
    keep = ~(dev['pad'] if masked else torch.zeros_like(dev['pad'])).unsqueeze(-1)
    loss = torch.mean(F.mse_loss(d, t, reduction='none') * keep)
    flat = [p for m in params for p in m] + [f[2] for f in fwd] + [f[3] for f in fwd]
    g = torch.autograd.grad(loss, flat)
    gp, gz1, gz2 = g[:4 * D], g[4 * D:5 * D], g[5 * D:]
    out = dict(loss=loss.detach())
    for i, name in enumerate(('dw1', 'db1', 'dw2', 'db2')):
        out[name] = torch.stack([gp[4 * m + i] for m in range(D)])
    rec = lambda per_member: torch.stack([t_.reshape(N, 64) for t_ in per_member], dim=1)      # noqa: E731  [N, D, 64]
    idx = torch.as_tensor(sel, device='cuda').clamp(min=0).long()
    live = torch.as_tensor(sel >= 0, device='cuda').unsqueeze(-1)
    for name, per_member in (('h1', [f[1].detach() for f in fwd]), ('gz1', gz1), ('gz2', gz2)):
        full = rec(per_member)
        out[name] = torch.gather(full, 1, idx.unsqueeze(-1).expand(-1, -1, 64)) * live
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _distill_case(B, n, S, sizes):
    """the case and its float64 reference with and without the mask (computed once)"""
    c = dr.make_distill_case(B, n, S, sizes, seed=B + 7 * n + S + sum(sizes))
    p64, t64 = dr.as64(c['pred']), dr.as64(c['targ'])
    ref = {m: dr.distill(c['state'].numpy(), c['action'].numpy(), c['pad'].numpy() if m else None, sizes, p64, t64) for m in (False, True)}
    return c, ref


def _dev(c):
    return dict(state=rr.strided(c['state'].cuda()), action=rr.strided(c['action'].cuda(), 5), pad=rr.strided(c['pad'].cuda(), 2))


@pytest.mark.parametrize('B,n,S,sizes', SHAPES)
def test_distill_against_float64_and_the_eager_composition(B, n, S, sizes):
    """`asac_drnd_distill` + `asac_drnd_param_grads` on strided window views, outputs pre-filled with NaN, against the float64
    restatement (tests/drnd_ref.py; tests/test_drnd_host.py pins it to float64 autograd on the module code), with and without
    the mask.  Every case with B > 1 holds one wholly padded batch entry whose action rows are all zero and one live row with
    an all-zero branch (the B == 1 case is one live row), and every case one member no row selects: that member's four gradients are exact zeros, padded rows' records are
    exact zeros.  Bound (the rule of tests/test_rnd_gpu.py): per tensor the kernels' largest absolute error against float64
    may be at most twice that of the float32 eager composition — today's `_train_rnd` lines on the same device tensors,
    gradients by autograd — with a floor of 4 units in the last place at the tensor's largest magnitude.  Tensors: loss, the
    records gz1 / gz2 / h1 and all 4 D parameter gradients.  Observed on MI355X: NOTES.md, "discrete RND"."""
    import asac_amd  # noqa: F401
    c, refs = _distill_case(B, n, S, sizes)
    D, K = sum(sizes), len(sizes)
    dev = _dev(c)
    assert dev['state'].stride(1) == S + 3 and dev['action'].stride(1) == D + 5 and dev['pad'].stride(0) == n + 2
    bad, share = [], 0.
    for masked in (False, True):
        ref = refs[masked]
        kernel = _distill_kernel(c, dev, masked)
        assert np.array_equal(kernel['sel'], ref['sel']), 'the selected members'
        assert np.array_equal(kernel['x'], c['state'].numpy().reshape(B * n, S))
        eager = _distill_eager(c, dev, masked, ref['sel'])
        for name in CHECKED:
            share = max(share, _share(f'{(B, n, S, sizes)} mask={masked}', name, kernel[name], eager[name], ref[name], bad))
        assert not (ref['sel'] == D - 1).any(), 'the case: nobody selects the last member'
        for name in ('dw1', 'db1', 'dw2', 'db2'):
            assert not kernel[name][D - 1].any(), f'{name}: exact zeros for the member nobody selected'
        rows = slice(B // 2 * n, B // 2 * n + n) if B > 1 else slice(0, 0)     # the wholly padded entry (all-zero action rows)
        for name in ('h1', 'gz1', 'gz2'):
            assert not kernel[name][rows].any(), name
            assert not kernel[name][kernel['sel'] < 0].any(), f'{name}: a pair that selected nothing has a zero record'
        if B == 1:
            assert (kernel['sel'] >= 0).all() and kernel['loss'] > 0 and kernel['gz1'].any(), 'the single row is live'
        if masked:
            padded = c['pad'].numpy().reshape(-1)
            assert (kernel['sel'][padded] == -1).all() and not kernel['gz1'][padded].any() and not kernel['gz2'][padded].any()
        if B > 1:
            r = ((B // 2 + 1) % B) * n
            assert kernel['sel'][r, 0] == -1 and (K == 1 or kernel['sel'][r, 1] >= 0), 'the live row with an all-zero branch'
    print(f'{(B, n, S, sizes)}: largest share of the bound {share:.2f}')
    assert not bad, bad


def test_distill_with_every_row_padded():
    """loss 0, every record and every gradient 0, nothing NaN"""
    import asac_amd  # noqa: F401
    c, _ = _distill_case(5, 3, 6, (3,))
    dev = dict(state=rr.strided(c['state'].cuda()), action=rr.strided(c['action'].cuda()), pad=torch.ones(5, 3, dtype=torch.bool, device='cuda'))
    out = _distill_kernel(c, dev, True)
    for name in ('loss', 'h1', 'gz1', 'gz2', 'dw1', 'db1', 'dw2', 'db2'):
        assert not out[name].any() and np.isfinite(out[name]).all(), name
    assert (out['sel'] == -1).all()


def test_distill_twice_gives_the_same_bits_and_leaves_its_workspace_zero():
    """(300, 2, 64, (4,)): 38 workgroups in the distillation, ten row chunks a member in the gradient launch"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    c, _ = _distill_case(300, 2, 64, (4,))
    dev = dict(state=c['state'].cuda(), action=c['action'].cuda(), pad=c['pad'].cuda())
    a, b = _distill_kernel(c, dev, True), _distill_kernel(c, dev, True)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    device = torch.device('cuda', torch.cuda.current_device())
    ws = native.drnd_distill_workspace(device, 600)
    assert ws.numel() == 38 + 1 and not ws[-1:].view(torch.int32).any(), 'the arrival counter is left at zero'
    wg = native.drnd_param_grads_workspace(device, 600, 64, 4)
    assert wg.numel() == 10 * 4 * (64 * 64 + 64 * 64 + 128) + 16
    assert not wg[-16:].view(torch.int32).any(), 'the members\' arrival counters are left at zero'


# ------------------------------------------------------------------------------------------------
# asac_drnd_pick
# ------------------------------------------------------------------------------------------------
def _pick_kernel(c, u=None, state=None, logits=None):
    from asac_amd import native
    br, flags, pred, targ, keep = _tables(c)
    batch, k, K, D = c['batch'], c['k'], br.K, br.D
    u = (c['u'] if u is None else u).cuda()
    state = rr.strided(c['state'].cuda()) if state is None else state
    logits = rr.strided(c['logits'].cuda(), 2) if logits is None else logits
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')      # noqa: E731
    out = dict(action=nan(batch, D), prob=nan(batch, D), err=nan(batch, k),
               cand=torch.full((batch, k, K), -1, dtype=torch.int32, device='cuda'),
               index=torch.full((batch,), -1, dtype=torch.int32, device='cuda'))
    native.drnd_pick(br, flags, pred, targ, state, logits, u, out['action'], out['prob'], out['err'], out['cand'], out['index'])
    return out


def _pick_eager_err(c, cand):
    """today's `rnd_sample_d_action` lines in float32 on the device, on the given candidates: `cal_d_rnd` of both models, the
    two broadcast products and sums, `pow` / `sum`"""
    r1 = c['S'] == 64
    x = c['state'].cuda()
    acts = torch.as_tensor(dr.one_hot(cand, c['sizes']), dtype=torch.float32, device='cuda')      # [batch, k, D]
    sel = acts.unsqueeze(-1)
    p = torch.stack([_stack_eager(x, *(t.cuda() for t in m), r1)[0] for m in c['pred']], dim=-2)
    t = torch.stack([_stack_eager(x, *(t.cuda() for t in m), r1)[0] for m in c['targ']], dim=-2)
    d = (sel * p.unsqueeze(1)).sum(-2)
    tt = (sel * t.unsqueeze(1)).sum(-2)
    return torch.sum(torch.pow(d - tt, 2), dim=-1).cpu().numpy()


# ... and the launch at its LDS limit: S = 128 and D = 16 (one staged stack, 16 members' differences: 141 KB), two workgroups
PICK_CASES = ([(batch, k, 6, (3,)) for batch in (1, 37, 300) for k in (1, 10, 50)] + [(37, 10, 64, (3, 2))]
              + [(17, 3, 128, (5, 4, 3, 2, 2))])


@functools.lru_cache(maxsize=None)
def _pick_case(batch, k, S, sizes):
    c = dr.make_pick_case(batch, k, S, sizes, seed=1000 + batch + 3 * k + S)
    ref = dr.pick(c['state'].numpy(), c['logits'].numpy(), c['u'].numpy(), sizes, dr.as64(c['pred']), dr.as64(c['targ']))
    return c, ref


def _discrete_probs(logits, sizes):
    """`asac_discrete_policy_loss_grad`'s probs_out on these logits (one zero critic; nothing else of it is read)"""
    from asac_amd import native
    B, D = logits.shape
    z = lambda *shape: torch.zeros(shape, device='cuda')      # noqa: E731
    probs = torch.full((B, D), float('nan'), device='cuda')
    native.discrete_policy_loss_grad(native.branches(sizes), logits.contiguous(), [z(B, D)], None, 1, torch.ones(B, D, device='cuda'),
                                     z(1), 0., z(1), z(B, D), z(1), probs)
    return probs


@pytest.mark.parametrize('batch,k,S,sizes', PICK_CASES)
def test_pick_against_float64(batch, k, S, sizes):
    """candidate indices equal the host rule's; the candidates' errors under the distillation test's bound (at most twice the
    float32 eager composition's error against float64, floor 4 ulp at the largest error); index and one-hot action equal
    where the float64 margin over candidates with another action is at least MIN_GAP (at most a tenth of the rows may miss
    it: tests/test_drnd_host.py checks that of the reference alone); argmax of the device's own errors is the index; prob
    has the bits of `asac_discrete_policy_loss_grad`'s probs_out"""
    import asac_amd  # noqa: F401
    c, ref = _pick_case(batch, k, S, sizes)
    out = {name: v.cpu().numpy() for name, v in _pick_kernel(c).items()}
    assert np.array_equal(out['cand'], ref['cand']), 'candidate indices'
    bad = []
    share = _share(f'pick {(batch, k, S, sizes)}', 'err', out['err'], _pick_eager_err(c, ref['cand']), ref['err'], bad)
    print(f'pick {(batch, k, S, sizes)}: share of the bound {share:.2f}')
    assert not bad, bad
    clear = dr.margin(ref['err'], ref['cand']) >= MIN_GAP
    assert clear.mean() > 0.9
    assert np.array_equal(out['index'][clear], ref['index'][clear])
    assert np.array_equal(out['action'][clear], ref['action'][clear])
    assert np.array_equal(out['index'], torch.argmax(torch.as_tensor(out['err']), dim=1).numpy())
    assert np.array_equal(out['action'], dr.one_hot(out['cand'][np.arange(batch), out['index']], sizes))
    if batch <= 1024:
        want = _discrete_probs(c['logits'].cuda(), sizes).cpu().numpy()
        assert np.array_equal(out['prob'], want), 'prob: the bits of the discrete policy launch'
    np.testing.assert_allclose(out['prob'], ref['prob'], rtol=4 * ULP, atol=0)


def test_pick_duplicates_nan_and_two_runs():
    """duplicated candidates have equal error bits and the lower index wins; a NaN state row gives index 0; two runs give the
    same bits"""
    import asac_amd  # noqa: F401
    c, _ = _pick_case(37, 10, 6, (3,))
    u = c['u'].clone()
    u[:, 5:] = u[:, :5]                      # candidates 5..9 repeat 0..4
    a, b = _pick_kernel(c, u=u), _pick_kernel(c, u=u)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    err = a['err'].cpu()
    assert torch.equal(err[:, 5:], err[:, :5]) and (a['index'].cpu() < 5).all()
    state = rr.strided(c['state'].cuda())
    state[3] = float('nan')
    out = _pick_kernel(c, state=state)
    assert out['index'][3].item() == 0 and torch.isnan(out['err'][3]).all()
    assert torch.isfinite(out['action']).all() and torch.isfinite(out['prob']).all()
    assert torch.equal(out['action'][3].cpu(), torch.as_tensor(dr.one_hot(out['cand'][3, 0].cpu().numpy(), (3,)), dtype=torch.float32))


def test_pick_frequencies_follow_the_softmax():
    """batch 4096, identical logits, k = 1, `DeviceNoise` uniforms: each action's frequency within 5 sqrt(p (1 - p) / 4096) of
    its softmax probability"""
    import asac_amd  # noqa: F401
    from algorithm.fused import DeviceNoise
    sizes, batch = (3, 2), 4096
    c = dr.make_pick_case(1, 1, 6, sizes, seed=5)
    c['batch'] = batch
    c['state'] = torch.randn(batch, 6, generator=torch.Generator().manual_seed(6))
    logits = torch.tensor([0.3, -0.9, 1.1, 0.5, -0.2]).repeat(batch, 1).cuda()
    u = torch.empty(batch, 1, 2, device='cuda')
    DeviceNoise(seed=11).uniform_(u)
    out = _pick_kernel(c, u=u, logits=logits)
    freq = out['action'].double().mean(0).cpu().numpy()
    p = dr.branch_probs(logits[:1].cpu().numpy(), sizes)[0]
    print('frequencies', freq, 'softmax', p)
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / batch)).all()
    assert (out['index'] == 0).all()


def fixture_members(g, c_id, D):
    """the D members of predictor and target of case `c_id` of f18_drnd_pick.npz -> two lists of float64 (w1, b1, w2, b2)"""
    sd = lambda name: {k.split('/', 2)[2]: g[k] for k in g.files if k.startswith(f'c{c_id}/{name}/')}      # noqa: E731
    return tuple([rr.stack_params(sd(name), f'd_dense_list.{m}.') for m in range(D)] for name in ('rnd', 'target'))


@pytest.mark.parametrize('c_id', range(len(PICK_SHAPES)))
def test_pick_replays_the_recorded_reference_function(golden_dir, c_id):
    """`tests/golden/f18_drnd_pick.npz` (the reference's own `rnd_sample_d_action` on recorded candidates; every row keeps
    the margin): the uniforms are the midpoints of the recorded candidates' CDF intervals; candidate and chosen indices and
    the action are equal, errors agree to 2e-5 of the largest.  The third case has S == 64 (residual first block) and two
    branches."""
    import asac_amd  # noqa: F401
    g = np.load(golden_dir / 'f18_drnd_pick.npz')
    batch, k, S, sizes = PICK_SHAPES[c_id]
    pred, targ = fixture_members(g, c_id, sum(sizes))
    k_ = lambda name: g[f'c{c_id}/{name}']      # noqa: E731
    u, narrow = dr.midpoint_uniforms(k_('logits'), sizes, k_('cand'))
    assert narrow > 1e-3
    f32 = lambda members: [tuple(torch.from_numpy(p).float() for p in m) for m in members]      # noqa: E731
    c = dict(S=S, sizes=sizes, batch=batch, k=k, state=torch.from_numpy(k_('state')), logits=torch.from_numpy(k_('logits')),
             u=torch.from_numpy(u), pred=f32(pred), targ=f32(targ))
    out = {name: v.cpu().numpy() for name, v in _pick_kernel(c).items()}
    assert np.array_equal(out['cand'], k_('cand'))
    assert np.array_equal(out['index'].astype(np.int64), k_('index'))
    want = k_('err')
    np.testing.assert_allclose(out['err'], want, rtol=0, atol=2e-5 * float(np.abs(want).max()))
    assert np.array_equal(out['action'], k_('action'))


# ------------------------------------------------------------------------------------------------
# the learner
# ------------------------------------------------------------------------------------------------
FLAG = 'fused_rnd_discrete'


def _learner(case, golden_dir=None, cls=None, **hip):
    """the case's learner (tests/golden/make_drnd_golden.CASES) with the fixture's weights and episodes if `golden_dir` is
    given -> (agent, fixture | None)"""
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    from tests.golden.make_drnd_golden import Fixture
    plugin_name, sizes, kw = CASES[case]
    kw = dict(kw)
    convert_config_to_enum(kw)
    agent = (cls or SAC_Base)(['vector'], [(6,)], list(sizes), 0, None, pu.plugin(plugin_name), device='cuda:0',
                              batch_size=SMALL['batch_size'], replay_config={'capacity': SMALL['capacity']},
                              hip_config=hip, **kw)
    if golden_dir is None:
        return agent, None
    g = Fixture(golden_dir / f'f6_step_{case}.npz')
    pu.load_golden_weights(agent, g)
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    return agent, g


def _calls(summary, prefix='asac_drnd_'):
    return {k: v['calls'] for k, v in summary.items() if k.startswith(prefix)}


STEP_CALLS = {'asac_drnd_distill': 1, 'asac_drnd_param_grads': 1}
def _run_fixture(case, golden_dir, fused):
    """the fixture's steps through the learner -> ({observable: (|error|, scale) of step 0}, [failures])"""
    from algorithm.fused import RecordedNoise
    from asac_amd import native
    agent, g = _learner(case, golden_dir, cls=pu.hooked_learner(), use_graph=False, **{FLAG: fused})
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
        assert calls == (STEP_CALLS if fused else {}), calls
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
    trained = [not np.array_equal(m.dense[0].linear.weight.detach().cpu().numpy(),
                                  g[f'w0/model_rnd/d_dense_list.{i}.dense.0.linear.weight'])
               for i, m in enumerate(agent.model_rnd.d_dense_list)]
    assert any(trained), 'd_dense_list trains'
    rb.check_health()
    agent.close()
    return errors0, failures


@pytest.mark.parametrize('case', list(CASES))
def test_step_against_the_reference_fixture(golden_dir, case):
    """The recorded reference steps through `SAC_Base(..., hip_config={'use_graph': False})` with `RecordedNoise`, as
    tests/test_rnd_gpu.py does: PER ids bit-exact, every recorded draw consumed; loss_q, td_error and tree, the first
    step's gradients (the `rnd` span among them) and the weights after the steps under the call-site defaults of
    tests/test_sac_aux_gpu.py.  The same steps run with the flag off, which must meet the defaults by itself; for step 0
    each observable's error under the launches may be at most twice that of the eager path, floor 4 units in the last
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


def _is_one_hot(action, sizes):
    parts = np.split(action, np.cumsum(sizes)[:-1], axis=-1)
    return all(((p == 0) | (p == 1)).all() and (p.sum(-1) == 1).all() for p in parts)


def test_launch_counts(golden_dir):
    """inside `_train_rnd` of one eager step: exactly one `asac_drnd_distill`, at most one other `asac_drnd_*` call and
    otherwise only `asac_adam_step`; one `choose_action` in train mode exactly one `asac_drnd_pick`, none outside train mode
    but one with `force_rnd_if_available`; with the flag off no `asac_drnd_*` call at all.  (Fails without the launches.)"""
    from asac_amd import native
    sizes = CASES['rnd_d2'][1]
    for fused in (True, False):
        agent, _ = _learner('rnd_d2', golden_dir, use_graph=False, **{FLAG: fused})
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
        assert _calls(seen) == (STEP_CALLS if fused else {}), seen.keys()
        assert not _calls(seen, 'asac_rnd_')
        inner = {k: v for k, v in inner.items() if v}
        if fused:
            assert inner.pop('asac_drnd_distill') == 1, inner
            assert sum(v for k, v in inner.items() if k.startswith('asac_drnd_')) <= 1, inner
            assert {k for k in inner if not k.startswith('asac_drnd_')} <= {'asac_adam_step'}, inner
        else:
            assert not any(k.startswith('asac_drnd_') for k in inner)
        with native.LaunchProfiler(repeat=1) as prof:
            action, prob, _ = agent.choose_action(*_acting_inputs(agent))
        assert _calls(prof.summary()) == ({'asac_drnd_pick': 1} if fused else {}), prof.summary().keys()
        assert action.shape == (7, 5) and prob.shape == (7, 5) and _is_one_hot(action, sizes)
        assert np.isfinite(prob).all() and (prob > 0).all()
        np.testing.assert_allclose(prob[:, :3].sum(-1), 1., rtol=1e-6)
        np.testing.assert_allclose(prob[:, 3:].sum(-1), 1., rtol=1e-6)
        agent.set_train_mode(False)         # outside train mode RND plays no part
        with native.LaunchProfiler(repeat=1) as prof:
            agent.choose_action(*_acting_inputs(agent))
        assert not _calls(prof.summary())
        with native.LaunchProfiler(repeat=1) as prof:
            agent.choose_action(*_acting_inputs(agent), force_rnd_if_available=True)
        assert _calls(prof.summary()) == ({'asac_drnd_pick': 1} if fused else {})
        agent.close()


def _plain_learner(d_sizes=(3,), c_size=0, seed=0, use_graph=False, hip=None, plugin='nn_vec_full', **kw):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(seed), np.random.seed(seed), random.seed(seed)
    kw.setdefault('use_rnd', True)
    nn = pu.plugin(plugin) if isinstance(plugin, str) else plugin
    return SAC_Base(['vector'], [(6,)], list(d_sizes), c_size, None, nn, device='cuda:0', n_step=3,
                    batch_size=16, replay_config={'capacity': 256},
                    hip_config={'use_graph': use_graph, FLAG: True, **(hip or {})}, **kw)


def test_captured_step_matches_eager():
    """the pattern of tests/test_rnd_gpu.py::test_captured_step_matches_eager: three `train()` calls — eager, and capture +
    replay + replay with host work in between — leave the same parameters, tree and TD errors (the launches allocate
    nothing once their buffers exist and synchronise nothing, so they are nodes of the step's graph)"""
    from asac_amd import native
    episodes = _episodes((3, 2), 0)
    results = []
    for use_graph in (False, True):
        agent = _plain_learner((3, 2), seed=3, use_graph=use_graph, hip=dict(graph_warmup=1))
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        launches = {}
        for i in range(3):
            if i == 0:
                with native.LaunchProfiler(repeat=1) as prof:
                    agent.train()
                launches = _calls(prof.summary())
            else:
                agent.train()
            torch.cuda.synchronize()
            np.sort(np.random.default_rng(i).standard_normal(1 << 14))         # host work between the replays
        assert launches == STEP_CALLS, 'the step runs the two launches'
        assert (agent._graph is not None) == use_graph, 'the RND step must capture'
        results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                        agent._td_error.cpu().numpy().copy()))
        agent.close()
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)


FALLBACKS = {
    'flag_off': dict(hip={FLAG: False}),
    'hybrid': dict(d=(3,), c=2),
    'dqn_like': dict(d=(3, 2), kw=dict(discrete_dqn_like=True)),
    'n_sample_65': dict(kw=dict(rnd_n_sample=65)),
    'sizes_sum_17': dict(d=(9, 8)),
    'width_32': dict(plugin=_narrow_plugin),
    'action_noise': dict(kw=dict(action_noise=[0.1, 0.2]), acting_only=True),
    'disable_sample': dict(acting=dict(disable_sample=True), acting_only=True),
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_what_the_path_does_not_cover_runs_todays_code(case):
    """each of these, with the flag ON, issues no `asac_drnd_*` launch where it applies (`acting_only`: in `choose_action`;
    the others in the step as well) and still trains and acts"""
    from asac_amd import native
    cfg = FALLBACKS[case]
    d, c = cfg.get('d', (3,)), cfg.get('c', 0)
    plugin = cfg.get('plugin', 'nn_vec_full')
    agent = _plain_learner(d, c, hip=cfg.get('hip'), plugin=plugin() if callable(plugin) else plugin, **cfg.get('kw', {}))
    for ep in _episodes(d, c):
        agent.put_episode(**ep)
    rnd0 = slice(*agent._params.segments['rnd'])
    before = agent._params.flat.clone()
    with native.LaunchProfiler(repeat=1) as prof:
        assert agent.train() == 1
    calls = _calls(prof.summary())
    assert calls == (STEP_CALLS if cfg.get('acting_only') else {}), calls
    assert torch.isfinite(agent._params.flat).all() and not torch.equal(before[rnd0], agent._params.flat[rnd0])
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, _ = agent.choose_action(*_acting_inputs(agent), **cfg.get('acting', {}))
    assert not _calls(prof.summary())
    assert np.isfinite(action).all() and np.isfinite(prob).all()
    agent.close()


def _masking_plugin():
    """nn_vec_full with a policy that subclasses the stock `ModelPolicy` (and so inherits `d_head_raw`) but has its own
    `forward`: the first entry of every branch is forbidden and the other logits are scaled"""
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


def test_a_policy_with_its_own_forward_acts_on_its_own_logits():
    """a plugin policy that overrides `forward` inherits `d_head_raw`, whose raw head outputs its `forward` never produces:
    the acting launch takes the logits of the distribution `forward` returns (`SAC_Base._discrete_logits`).  The returned
    probability equals the flag-off path's (`d_policy.probs`) to float32 rounding, is zero at every forbidden entry and
    no forbidden entry is ever chosen"""
    from asac_amd import native
    sizes, out = (3, 2), {}
    inputs = None
    for fused in (True, False):
        agent = _plain_learner(sizes, seed=5, hip={FLAG: fused}, plugin=_masking_plugin(), rnd_n_sample=10)
        inputs = _acting_inputs(agent, batch=64)
        with native.LaunchProfiler(repeat=1) as prof:
            action, prob, _ = agent.choose_action(*inputs)
        assert _calls(prof.summary()) == ({'asac_drnd_pick': 1} if fused else {})
        assert _is_one_hot(action, sizes) and not action[:, 0].any() and not action[:, 3].any(), 'a forbidden entry was chosen'
        assert not prob[:, 0].any() and not prob[:, 3].any() and (prob[:, 4] == 1).all()
        out[fused] = prob
        agent.close()
    np.testing.assert_allclose(out[True], out[False], rtol=1e-5, atol=1e-7)
    assert (out[True][:, 1:3] > 0).all() and out[True][:, 1].std() > 0, 'the probabilities follow the states'


def test_an_option_runs_todays_code():
    """an `OptionBase` (`_plain_learner = False`) with `use_rnd=True` and discrete branches: neither its acting nor its
    `_train_rnd` issues an `asac_drnd_*` launch, flag on"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    from algorithm.oc.option_base import OptionBase
    from asac_amd import native
    base = pu.plugin('nn_oc')
    ns = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if k.startswith('Model')})
    ns.ModelRND = m.ModelRND
    torch.manual_seed(0)
    opt = OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [3], 0, None, ns, device='cuda:0', batch_size=16,
                     summary_path=None, n_step=3, use_rnd=True, hip_config={FLAG: True})
    assert opt._drnd_fused(rows=48) is None and type(opt)._plain_learner is False
    dev = opt.device
    obs = [torch.randn(7, 6, device=dev)]
    before = opt.model_rnd.d_dense_list[0].dense[0].linear.weight.detach().clone()
    actions = torch.zeros(16, 3, 3, device=dev)
    actions[..., 0] = 1.
    with native.LaunchProfiler(repeat=1) as prof:
        action, prob, _, _ = opt.choose_action(obs, torch.zeros(7, 3, device=dev),
                                               torch.zeros(7, *opt.seq_hidden_state_shape, device=dev))
        opt._train_rnd(torch.zeros(16, 3, dtype=torch.bool, device=dev), torch.randn(16, 3, opt.state_size, device=dev), actions)
    assert not _calls(prof.summary())
    assert torch.isfinite(action).all() and torch.isfinite(prob).all()
    assert not torch.equal(before, opt.model_rnd.d_dense_list[0].dense[0].linear.weight)
    opt.close()


# ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    """a misaligned member pointer (refused where the table is built: the entry points see only the table), a NULL or
    misaligned table, k = 0 or 65, D = 17, S = 129, a residual first block at S != 64, a NULL required pointer:
    hipErrorInvalidValue and no launch, the marker buffers untouched; B == 0 / batch == 0 launch nothing; the same calls with
    good arguments then run"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    B, n, S, sizes, k = 4, 3, 6, (3, 2), 5
    c = dr.make_distill_case(B, n, S, sizes, seed=1)
    br, flags, pred, targ, keep = _tables(c)
    lib, s, bad, p = native.load(), native._stream(), 1, native._p      # 1: hipErrorInvalidValue
    stacks, gstacks = (lambda t: native._table_p(t, native.RndStack)), (lambda t: native._table_p(t, native.RndGrads))
    N, K, D = B * n, br.K, br.D
    marker = lambda *shape: torch.full(shape, 7., device='cuda')      # noqa: E731
    x, h1, gz1, gz2, loss = marker(N, S), marker(N, K, 64), marker(N, K, 64), marker(N, K, 64), marker(1)
    sel = torch.full((N, K), 7, dtype=torch.int32, device='cuda')
    gtens = [(marker(64, S), marker(64), marker(64, 64), marker(64)) for _ in range(D)]
    grads = native.drnd_table(gtens)
    action, prob, err = marker(B, D), marker(B, D), marker(B, k)
    outputs = (x, h1, gz1, gz2, loss, action, prob, err, *(t for g_ in gtens for t in g_))
    state, act, pad = c['state'].cuda(), c['action'].cuda(), c['pad'].cuda()
    logits, u = torch.randn(B, D, device='cuda'), torch.rand(B, k, K, device='cuda')
    ws, wg = torch.zeros(8, device='cuda'), torch.zeros(native.drnd_param_grads_workspace_floats(N, S, D), device='cuda')
    # a member whose first matrix starts 4 bytes off a 16-byte boundary: the table is not built
    off = torch.zeros(64 * S + 1, device='cuda')[1:].view(64, S)
    with pytest.raises(native.AsacNativeError):
        native.drnd_table([(off, *keep[0][0][1:])] + keep[0][1:])
    with pytest.raises(native.AsacNativeError):
        native.drnd_table(keep[0] * 4)                 # 20 members
    skew = torch.zeros(4 * D + 1, dtype=torch.int64, device='cuda')[1:]       # a table 8 bytes off
    res = lambda r1, r2: (C.c_int32 * 2)(r1, r2)      # noqa: E731
    ok_res = res(*map(int, flags))

    def distill(b=br, S_=S, r=ok_res, pr=pred, tg=targ, B_=B, h=h1, lo=loss, w=ws):
        return lib.asac_drnd_distill(C.byref(b), S_, r, stacks(pr), stacks(tg), p(state), state.stride(0), state.stride(1), p(act),
                                     act.stride(0), act.stride(1), p(pad), pad.stride(0), pad.stride(1), B_, n, p(sel), p(x), p(h),
                                     p(gz1), p(gz2), p(lo), p(w), s)

    def param_grads(b=br, S_=S, g_=grads, rows=N, h=h1, w=wg):
        return lib.asac_drnd_param_grads(C.byref(b), S_, p(sel), p(x), p(h), p(gz1), p(gz2), rows, gstacks(g_), p(w), s)

    def pick(b=br, S_=S, r=ok_res, pr=pred, tg=targ, k_=k, batch=B, a=action, u_=u):
        return lib.asac_drnd_pick(C.byref(b), S_, r, stacks(pr), stacks(tg), p(state[:, 0]), state.stride(0), p(logits),
                                  logits.stride(0), p(u_), k_, batch, p(a), p(prob), p(err), None, None, s)

    wide, sum_off = native.branches((9, 8)), native.branches(sizes)
    sum_off.D = D + 1
    h_off = torch.zeros(N * K * 64 + 1, device='cuda')[1:]
    refused = [distill(pr=None), distill(tg=None), distill(pr=skew), distill(b=wide), distill(b=sum_off), distill(S_=129),
               distill(r=res(1, 1)), distill(lo=None), distill(w=None), distill(h=h_off), distill(B_=-1)]
    refused += [param_grads(g_=None), param_grads(g_=skew), param_grads(b=wide), param_grads(S_=129), param_grads(h=h_off),
                param_grads(w=None), param_grads(rows=-1)]
    refused += [pick(pr=None), pick(tg=skew), pick(k_=0), pick(k_=65), pick(b=wide), pick(S_=129), pick(r=res(1, 1)),
                pick(a=None), pick(u_=None)]
    assert refused == [bad] * len(refused), refused
    assert [distill(B_=0), param_grads(rows=0), pick(batch=0)] == [0, 0, 0]
    assert not native.drnd_sizes_ok(129, sizes) and not native.drnd_sizes_ok(S, (9, 8)) and not native.drnd_sizes_ok(S, sizes, 65)
    assert not native.drnd_sizes_ok(S, sizes, 0) and not native.drnd_sizes_ok(S, (1,) * 9) and native.drnd_sizes_ok(S, sizes, 64)
    torch.cuda.synchronize()
    for t in outputs:
        assert (t == 7.).all(), 'nothing was launched'
    assert (sel == 7).all()
    assert [distill(), param_grads(), pick()] == [0, 0, 0]          # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    for t in outputs:
        assert torch.isfinite(t).all() and not (t == 7.).all()
    assert not ws.view(torch.int32)[1:2].any(), 'the arrival counter (behind one workgroup sum) is zero again'
