"""GPU: the one-launch siamese losses (`asac_siamese_atc_loss_grad` / `asac_siamese_byol_loss_grad`, csrc/siamese.hip)
against float64 copies of the eager arithmetic they replace (`SacAux._train_siamese_representation_learning`), and the
learner with `hip_config['fused_siamese']` on: launch accounting, the reference's recorded step, the captured step.

Yardstick, as in tests/test_fused_conv1d_gpu.py: for each output, err(a) = max|a - ref64| / max|ref64|; e_mod is the larger
of that error of the SAME eager code in float32 on the device and on the CPU, computed here on every run; the kernel must hold
err <= max(4 e_mod, sqrt(k) 2^-24) with k the number of terms of the output's longest sum (4x: DESIGN.md section 5; the second
term is the random-walk rounding of any float32 summation order).  k: the ATC loss and g_W = e^T dl te sum over all N^2 logits,
g_e = dl te W^T over N E terms; the BYOL loss over N P products, a row of g_pred over the P terms of its norms and dot product.
The figures observed on the MI355X are recorded in tests/siamese_tolerances.json (not read by the tests).

At P = 1 the cosine is +-1 whatever pred is: d cos / d pred is identically zero, formed as the difference of two terms of
size pad_i / (N |pred_i|).  A relative error against max|ref64| = 0 means nothing there; for that case alone the error of
g_pred is taken relative to the largest of those cancelling terms, for the kernel and for e_mod alike."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch
from torch.nn import functional

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402
from tests.plugins import nn_vec_full  # noqa: E402

# (batch, n, E) -> (pad: 'blocks' = random 0 / 1 with whole blocks zero | 'ones', scale of e)
ATC_CASES = {
    (16, 3, 16): ('blocks', 1.0),      # the existing aux test's N = 48, under one tile
    (5, 1, 8): ('blocks', 1.0),        # n = 1: the labels are the identity
    (7, 3, 16): ('blocks', 1.0),       # N = 21, a ragged tile
    (40, 3, 16): ('blocks', 1.0),      # blocks of 3 straddle every power-of-two tile edge; several row and column tiles
    (3, 64, 32): ('blocks', 1.0),      # a block larger than a tile
    (9, 4, 10): ('ones', 1.0),         # E not a multiple of 4; all rows count
    (33, 3, 1): ('blocks', 1.0),       # E = 1
    (64, 5, 128): ('blocks', 1.0),     # E at its limit
    (256, 3, 16): ('blocks', 1.0),     # usv_search itself
    (16, 3, 17): ('blocks', 3.5),      # |l| reaches ~50: the stable form of the BCE (and E one past a block of 16)
}
ATC_NAMES = ('loss', 'g_e', 'g_w')
# (N, P) -> which input gets an all-zero row
BYOL_CASES = {(48, 14): 'pred', (21, 6): 't_proj', (768, 14): None, (130, 256): None, (1, 1): None}


def _err(a, ref, floor=0.):
    return float((a - ref).abs().max() / max(float(ref.abs().max()), floor))


def _atc_inputs(case):
    batch, n, E = case
    pad_mode, scale = ATC_CASES[case]
    N = batch * n
    gen = torch.Generator().manual_seed(1000 * batch + 10 * n + E)
    e = torch.randn(N, E, generator=gen) * scale
    te = torch.randn(N, E, generator=gen)
    w = torch.randn(E, E, generator=gen) / math.sqrt(E)
    if pad_mode == 'ones':
        pad = torch.ones(N)
    else:
        pad = (torch.rand(N, generator=gen) < 0.7).float().reshape(batch, n)
        pad[torch.arange(batch) % 4 == 1] = 0.         # whole blocks without weight
        pad[0, 0] = 1.
        pad = pad.reshape(N)
    return e, te, w, pad


def _atc_eager(e, te, w, pad, batch, n):
    """[loss, d loss / d e, d loss / d W] of the eager branch on the operands' device in their dtype (as float64 on the host)"""
    e, w = e.clone().requires_grad_(), w.clone().requires_grad_()
    logits = torch.mm(torch.mm(e, w), te.t())
    labels = torch.block_diag(*torch.ones(batch, n, n, dtype=e.dtype, device=e.device))
    loss = (functional.binary_cross_entropy_with_logits(logits, labels, reduction='none') * pad.reshape(batch * n, 1)).mean()
    loss.backward()
    return [t.detach().double().cpu() for t in (loss, e.grad, w.grad)], float(logits.detach().abs().max())


@functools.lru_cache(maxsize=None)
def _atc_reference(case):
    """-> (ref64 outputs, e_mod per output, max |logit|); computed once per case"""
    batch, n, _ = case
    ins = _atc_inputs(case)
    want, l_max = _atc_eager(*[t.double() for t in ins], batch, n)
    cpu32, _ = _atc_eager(*ins, batch, n)
    dev32, _ = _atc_eager(*[t.cuda() for t in ins], batch, n)
    return want, [max(_err(a, r), _err(b, r)) for a, b, r in zip(cpu32, dev32, want)], l_max


def _atc_launch(e, te, w, pad, n, fill=None):
    from asac_amd import native
    N, E = e.shape
    ws = torch.zeros(native.siamese_atc_workspace_floats(N, E), device='cuda')
    make = (lambda *s: torch.full(s, fill, device='cuda')) if fill is not None else (lambda *s: torch.empty(s, device='cuda'))
    loss, g_e, g_w = make(), make(N, E), make(E, E)
    native.siamese_atc_loss_grad(e, te, w, pad, n, loss, g_e, g_w, ws)
    return [loss, g_e, g_w], ws


@pytest.mark.parametrize('case', list(ATC_CASES), ids=lambda c: 'x'.join(map(str, c)))
def test_atc_kernel_matches_the_float64_eager_arithmetic(case):
    import asac_amd  # noqa: F401
    from asac_amd import native
    batch, n, E = case
    N = batch * n
    ins = _atc_inputs(case)
    want, e_mod, l_max = _atc_reference(case)
    if ATC_CASES[case][1] != 1.0:
        assert l_max > 40., f'the saturating case must reach large logits (max |l| = {l_max:.3g})'
    with native.LaunchProfiler(repeat=1) as prof:
        outs, _ = _atc_launch(*[t.cuda() for t in ins], n, fill=float('nan'))
    assert prof.summary()['asac_siamese_atc_loss_grad']['calls'] == 1
    terms = {'loss': N * N, 'g_e': N * E, 'g_w': N * N}
    figures, failed = {}, []
    for name, a, r, em in zip(ATC_NAMES, outs, want, e_mod):
        a = a.double().cpu()
        assert a.shape == r.shape and torch.isfinite(a).all(), name
        err, bound = _err(a, r), max(4.0 * em, math.sqrt(terms[name]) * 2.0 ** -24)
        figures[name] = {'observed': err, 'e_mod': em, 'bound': bound}
        if not err <= bound:
            failed.append(name)
    print('SIAMESE_TOL', json.dumps({'kernel': 'atc', 'case': 'x'.join(map(str, case)), 'max_abs_logit': l_max, **figures}))
    assert not failed, (failed, figures)


@pytest.mark.parametrize('case', [(40, 3, 16), (256, 3, 16), (64, 5, 128)], ids=lambda c: 'x'.join(map(str, c)))
def test_atc_kernel_exact_cases(case):
    """zero weights give exact zeros; equal inputs give equal bits; every output element is written"""
    import asac_amd  # noqa: F401
    batch, n, E = case
    e, te, w, pad = [t.cuda() for t in _atc_inputs(case)]
    (loss, g_e, g_w), ws = _atc_launch(e, te, w, torch.zeros_like(pad), n, fill=float('nan'))
    assert float(loss) == 0. and torch.equal(g_e, torch.zeros_like(g_e)) and torch.equal(g_w, torch.zeros_like(g_w))
    first, ws = _atc_launch(e, te, w, pad, n, fill=float('nan'))
    assert all(torch.isfinite(t).all() for t in first) and float(first[1].abs().max()) > 0
    again, _ = _atc_launch(e, te, w, pad, n, fill=float('nan'))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # ... also on a workspace a launch has used before (it leaves its counters ready)
    from asac_amd import native
    outs = [torch.full_like(t, float('nan')) for t in first]
    native.siamese_atc_loss_grad(e, te, w, pad, n, *outs, ws)
    assert all(torch.equal(a, b) for a, b in zip(first, outs))


def _byol_inputs(case):
    N, P = case
    gen = torch.Generator().manual_seed(100 * N + P)
    pred, t_proj = torch.randn(N, P, generator=gen), torch.randn(N, P, generator=gen)
    pad = (torch.rand(N, generator=gen) < 0.7).float()
    pad[0] = 1.
    zero_row = BYOL_CASES[case]
    if zero_row == 'pred':
        pred[5] = 0.
        pad[5] = 1.
    elif zero_row == 't_proj':
        t_proj[5] = 0.
        pad[5] = 1.
    return pred, t_proj, pad


def _byol_eager(pred, t_proj, pad):
    pred = pred.clone().requires_grad_()
    loss = (functional.cosine_similarity(pred, t_proj) * pad).mean()
    loss.backward()
    return [t.detach().double().cpu() for t in (loss, pred.grad)]


def _byol_floor(case, pred, pad):
    """the size of the terms that cancel in d cos / d pred at P = 1 (module docstring); 0 elsewhere"""
    if case[1] != 1:
        return 0.
    return float((pad.double() / (case[0] * pred.double().abs().reshape(-1))).max())


def _byol_rows(case):
    """-> (all rows, the rows without the zero row: next to its gradient of size 1 / eps nothing else would be seen)"""
    keep = torch.ones(case[0], dtype=torch.bool)
    if BYOL_CASES[case] is not None:
        keep[5] = False
    return torch.ones(case[0], dtype=torch.bool), keep


@functools.lru_cache(maxsize=None)
def _byol_reference(case):
    """-> (ref64 outputs, e_mod of the loss, e_mod of g_pred over all rows and over the rows without the zero row)"""
    ins = _byol_inputs(case)
    floor = _byol_floor(case, ins[0], ins[2])
    want = _byol_eager(*[t.double() for t in ins])
    cpu32, dev32 = _byol_eager(*ins), _byol_eager(*[t.cuda() for t in ins])
    e_loss = max(_err(cpu32[0], want[0]), _err(dev32[0], want[0]))
    e_g = [max(_err(cpu32[1][rows], want[1][rows], floor), _err(dev32[1][rows], want[1][rows], floor)) for rows in _byol_rows(case)]
    # float32 torch on the CPU stays within the bound the kernel is held to (the clamp does not blow its rounding up)
    assert torch.isfinite(cpu32[1]).all()
    assert _err(cpu32[0], want[0]) <= max(4.0 * e_loss, math.sqrt(case[0] * case[1]) * 2.0 ** -24)
    for rows, em in zip(_byol_rows(case), e_g):
        assert _err(cpu32[1][rows], want[1][rows], floor) <= max(4.0 * em, math.sqrt(case[1]) * 2.0 ** -24)
    return want, e_loss, e_g


@pytest.mark.parametrize('case', list(BYOL_CASES), ids=lambda c: 'x'.join(map(str, c)))
def test_byol_kernel_matches_float64_cosine_similarity(case):
    import asac_amd  # noqa: F401
    from asac_amd import native
    N, P = case
    pred, t_proj, pad = _byol_inputs(case)
    want, e_loss, e_g = _byol_reference(case)
    floor = _byol_floor(case, pred, pad)
    ws = torch.zeros(native.SIAMESE_BYOL_WORKSPACE_FLOATS, device='cuda')
    loss, g_pred = torch.full((), float('nan'), device='cuda'), torch.full((N, P), float('nan'), device='cuda')
    with native.LaunchProfiler(repeat=1) as prof:
        native.siamese_byol_loss_grad(pred.cuda(), t_proj.cuda(), pad.cuda(), loss, g_pred, ws)
    assert prof.summary()['asac_siamese_byol_loss_grad']['calls'] == 1
    loss2, g2 = torch.full_like(loss, float('nan')), torch.full_like(g_pred, float('nan'))
    native.siamese_byol_loss_grad(pred.cuda(), t_proj.cuda(), pad.cuda(), loss2, g2, ws)
    assert torch.equal(loss, loss2) and torch.equal(g_pred, g2) and torch.isfinite(g_pred).all() and torch.isfinite(loss)
    got_loss, got_g = loss.double().cpu(), g_pred.double().cpu()
    figures = {'loss': {'observed': _err(got_loss, want[0]), 'e_mod': e_loss,
                        'bound': max(4.0 * e_loss, math.sqrt(N * P) * 2.0 ** -24)}}
    for tag, rows, em in zip(('g_pred', 'g_pred_other_rows'), _byol_rows(case), e_g):
        figures[tag] = {'observed': _err(got_g[rows], want[1][rows], floor), 'e_mod': em,
                        'bound': max(4.0 * em, math.sqrt(P) * 2.0 ** -24)}
    print('SIAMESE_TOL', json.dumps({'kernel': 'byol', 'case': 'x'.join(map(str, case)), **figures}))
    failed = [k for k, f in figures.items() if not f['observed'] <= f['bound']]
    assert not failed, (failed, figures)
    if BYOL_CASES[case] == 't_proj':     # a zero target row: the cosine and its gradient are exact zeros
        assert torch.equal(g_pred[5], torch.zeros(P, device='cuda'))
    # zero weights: exact zeros
    native.siamese_byol_loss_grad(pred.cuda(), t_proj.cuda(), torch.zeros(N, device='cuda'), loss2, g2, ws)
    assert float(loss2) == 0. and torch.equal(g2, torch.zeros_like(g2))


def test_entry_points_refuse_bad_arguments_without_a_launch():
    import asac_amd  # noqa: F401
    from asac_amd import native
    lib, bad = native.load(), 1         # hipErrorInvalidValue
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')      # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731
    big = torch.zeros(66 * 130, device='cuda')
    e, w, pad = big, torch.zeros(130 * 130, device='cuda'), torch.ones(256, device='cuda')
    loss, g_e, g_w, ws = nan(1), nan(66 * 130), nan(130 * 130), torch.zeros(1 << 16, device='cuda')

    def atc(N, E, n, null=None):
        args = [p(e), p(e), p(w), p(pad), N, E, n, p(loss), p(g_e), p(g_w), p(ws)]
        if null is not None:
            args[null] = None
        return lib.asac_siamese_atc_loss_grad(*args, None)

    assert atc(48, 129, 3) == bad             # E beyond the limit
    assert atc(48, 0, 3) == bad
    assert atc(50, 16, 3) == bad              # n does not divide N
    assert atc(65, 16, 65) == bad             # n beyond the limit
    assert atc(48, 16, 0) == bad
    assert atc(0, 16, 3) == bad               # no rows
    assert atc(16384 + 4, 16, 4) == bad
    for null in (0, 1, 2, 3, 7, 8, 9, 10):
        assert atc(48, 16, 3, null) == bad
    assert native.siamese_atc_workspace_floats(48, 129) == -1 and native.siamese_atc_workspace_floats(0, 16) == -1

    def byol(N, P, null=None):
        args = [p(e), p(e), p(pad), N, P, p(loss), p(g_e), p(ws)]
        if null is not None:
            args[null] = None
        return lib.asac_siamese_byol_loss_grad(*args, None)

    assert byol(16, 257) == bad and byol(16, 0) == bad and byol(0, 14) == bad and byol((1 << 20) + 1, 14) == bad
    for null in (0, 1, 2, 5, 6, 7):
        assert byol(16, 14, null) == bad
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (loss, g_e, g_w)), 'a refused call wrote an output'
    assert not ws.any(), 'a refused call touched the workspace'
    with pytest.raises(native.AsacNativeError):
        native.siamese_atc_loss_grad(torch.zeros(50, 16, device='cuda'), torch.zeros(50, 16, device='cuda'),
                                     torch.zeros(16, 16, device='cuda'), torch.ones(50, device='cuda'), 3, nan(1), nan(50, 16),
                                     nan(16, 16), ws)


def _learner(siamese, use_q, adaptive, hip_config, **kw):
    import asac_amd  # noqa: F401
    from algorithm.utils.enums import convert_config_to_enum
    SAC_Base = pu.hooked_learner()
    cfg = dict(siamese=siamese, siamese_use_q=use_q, siamese_use_adaptive=adaptive, burn_in_step=2)
    convert_config_to_enum(cfg)
    torch.manual_seed(0)
    return SAC_Base(['vector'], [(6,)], [], 2, None, nn_vec_full, device='cuda:0', batch_size=16, n_step=3,
                    replay_config={'capacity': 256}, hip_config=hip_config, **cfg, **kw)


def _feed(agent, lengths=(40, 30, 50)):
    rng = np.random.default_rng(0)
    for T in lengths:
        agent.put_episode(**pu.synthetic_episode(rng, [(6,)], [], 2, (0,), T))


LAUNCH = {'ATC': 'asac_siamese_atc_loss_grad', 'BYOL': 'asac_siamese_byol_loss_grad'}


@pytest.mark.parametrize('use_q,adaptive', [(False, False), (True, False), (False, True), (True, True)],
                         ids=['plain', 'q', 'adaptive', 'q_adaptive'])
@pytest.mark.parametrize('siamese', ['ATC', 'BYOL'])
def test_one_launch_per_encoder_with_the_switch_on(siamese, use_q, adaptive):
    from asac_amd import native
    agent = _learner(siamese, use_q, adaptive, {'use_graph': False, 'fused_siamese': True})
    _feed(agent)
    encoders = len(agent.contrastive_weight_list) if siamese == 'ATC' else len(agent.model_rep_prediction_list)
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    seen = prof.summary()
    assert encoders >= 1 and seen[LAUNCH[siamese]]['calls'] == encoders
    assert LAUNCH['BYOL' if siamese == 'ATC' else 'ATC'] not in seen
    assert torch.isfinite(agent._params.flat).all()
    agent.close()


@pytest.mark.parametrize('hip_config', [{'use_graph': False, 'fused_siamese': False}, {'use_graph': False}], ids=['off', 'absent'])
@pytest.mark.parametrize('siamese', ['ATC', 'BYOL'])
def test_no_siamese_launch_with_the_switch_off(siamese, hip_config):
    from asac_amd import native
    agent = _learner(siamese, True, siamese == 'BYOL', hip_config)
    _feed(agent)
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    seen = prof.summary()
    assert LAUNCH['ATC'] not in seen and LAUNCH['BYOL'] not in seen
    agent.close()


GOLDEN = {'aux_atc': dict(siamese='ATC', siamese_use_q=True, burn_in_step=2),
          'aux_byol': dict(siamese='BYOL', siamese_use_q=True, siamese_use_adaptive=True, burn_in_step=2)}


@pytest.mark.parametrize('case', list(GOLDEN))
def test_first_step_with_the_switch_on_vs_reference_golden(golden_dir, case):
    """the set-up of tests/test_sac_aux_gpu.py with `fused_siamese=True`: the first step's gradients of every optimizer
    against the reference's within that test's DEFAULT bounds (no entry of tests/parity_tolerances.json is read)"""
    import asac_amd  # noqa: F401
    from algorithm.fused import RecordedNoise
    from algorithm.utils.enums import convert_config_to_enum
    from asac_amd import native
    SAC_Base = pu.hooked_learner()
    g = np.load(golden_dir / f'f6_step_{case}.npz')
    kw = dict(GOLDEN[case])
    convert_config_to_enum(kw)
    torch.manual_seed(0)
    agent = SAC_Base(['vector'], [(6,)], [], 2, None, nn_vec_full, device='cuda:0', batch_size=16, n_step=3,
                     replay_config={'capacity': 256}, hip_config={'use_graph': False, 'fused_siamese': True}, **kw)
    with torch.no_grad():
        for name, obj in agent.ckpt_dict.items():
            if isinstance(obj, torch.nn.Module):
                for k, p in obj.state_dict().items():
                    p.copy_(torch.from_numpy(g[f'w0/{name}/{k}'].copy()))
            elif isinstance(obj, torch.Tensor) and f'w0/t/{name}' in g.files:
                obj.copy_(torch.from_numpy(g[f'w0/t/{name}'].copy()))
        agent.log_c_alpha.copy_(torch.from_numpy(g['w0/log_c_alpha'].copy()))
        agent.log_d_alpha.copy_(torch.from_numpy(g['w0/log_d_alpha'].copy()))
    for ep in pu.golden_episodes(g):
        agent.put_episode(**ep)
    rb = agent.replay_buffer
    if 'step0/w_rq/model_q_0/' + next(iter(agent.model_q_list[0].state_dict())) in g.files:
        agent.after_rep_q_update = lambda: pu.load_golden_weights(agent, g, prefix='step0/w_rq')
    eps = [g[f'step0/eps{j}'] for j in range(int(g['step0/n_eps']))]
    agent.noise = RecordedNoise([g['step0/u']], eps, list(g['step0/perm']))
    rb.uniform_source = agent.noise
    with native.LaunchProfiler(repeat=1) as prof:
        assert agent.train() == 1
    assert prof.summary()[LAUNCH[kw['siamese'].name]]['calls'] >= 1
    assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
    assert np.array_equal(rb._ids.cpu().numpy(), g['step0/sample_ids']), 'PER index selection'
    np.testing.assert_allclose(agent._stats['loss_q'].item(), g['step0/loss_q'], rtol=2e-4)
    np.testing.assert_allclose(agent._td_error.cpu().numpy()[:, None], g['step0/td_error'], rtol=2e-4, atol=2e-5)
    checked = pu.assert_first_step_gradients(agent, g, rtol=2e-3, atol_frac=5e-5, log_key=None)
    assert checked > 0
    agent.close()


@pytest.mark.parametrize('siamese', ['ATC', 'BYOL'])
def test_siamese_inside_the_captured_step(siamese):
    """graphs on (the default): six steps with the switch on train the head, stay finite, and the step is captured
    exactly when it is with the switch off"""
    captured = {}
    for fused in (False, True):
        agent = _learner(siamese, True, True, {'fused_siamese': fused})
        # (the losses weigh a row by its padding mask, as the reference's do: short episodes put padded rows into every batch)
        _feed(agent, (40, 30, 50, 7, 8, 9, 7, 8, 9))
        before = agent._params.flat.clone()
        for _ in range(6):
            agent.train()
        seg = agent._params.segments['siamese']
        assert not torch.equal(before[seg[0]:seg[1]], agent._params.flat[seg[0]:seg[1]])
        assert torch.isfinite(agent._params.flat).all()
        captured[fused] = agent._graph is not None
        agent.close()
    assert captured[True] == captured[False]
