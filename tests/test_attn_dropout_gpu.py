"""GPU: attention-weight dropout inside the multi-head attention launches (`asac_attention_mh_dropout_forward/backward`,
csrc/attn_mh.hip, csrc/asac_dropout.h) through `MultiheadAttention` in training mode, against the float64 restatement of
tests/attn_dropout_ref.py fed the RESTATED mask of the call counter the launch reports.  Nothing here is compared with torch's
own dropout draws.

The output stack of the modules under test is `out_dense_depth=1`: a ResBlock and an `nn.Dropout(p)`.  That `nn.Dropout` is
ATen's (out of scope) and draws from torch's generator, so the tests switch IT off (`.eval()` on that one
sub-module; the attention module itself stays in training mode) to have values a restatement can reproduce.

Tolerances: tests/attn_dropout_tolerances.json holds, per p and output, 4 x the error observed on the MI355X as
a FRACTION of the cap — the cap being 1 / (1 - p) times what tests/test_fused_attn_mh_gpu.py holds this kernel to at p = 0
(rtol 3e-4, atol 3e-5 for outputs and input gradients; its parameter-gradient formula for the rest); no fraction exceeds 1."""
import copy
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

from tests import attn_dropout_ref as ref

pytestmark = pytest.mark.gpu

TOL = json.loads((Path(__file__).resolve().parent / 'attn_dropout_tolerances.json').read_text())
NAMES = ('out', 'weights', 'dq', 'dk', 'dv')

SHAPES = [
    (3, 7, 5, 24, 2),        # Lk % 4 != 0: a Philox block hangs over the window's edge; ragged head width 12
    (4, 20, 27, 40, 8),      # both tile pairs, ragged; a wave walks two heads; head width 5
    (7, 32, 32, 128, 2),     # full tiles; head width 64
    (5, 1, 32, 64, 1),       # one query; one head
    (70, 9, 18, 12, 2),      # toy_queue's widths; more workgroups than leaf arrival words
    (1, 9, 9, 64, 8),        # a single workgroup is first and last arriver
]
SEED, INSTANCE = 20240229, 77


def _mask(kind, B, Lq, Lk, gen):
    """the masks of tests/test_fused_attn_mh_gpu.py::_mask ('batch': dead rows, a dead batch entry; 'none')"""
    if kind == 'none':
        return None, None
    m = torch.rand(B, Lq, Lk, generator=gen) < 0.4
    m[0, 0] = True                       # a dead row
    if B > 1:
        m[1] = True                      # a dead batch entry
    kpm = torch.rand(B, Lk, generator=gen) < 0.3
    return m, kpm


def _switch_off_output_dropout(layer):
    for mod in layer.out_proj.modules():
        if isinstance(mod, nn.Dropout):
            mod.eval()
    return layer


@functools.lru_cache(maxsize=None)
def _case(B, Lq, Lk, E, H, kind, p, row_mask=False):
    """(CPU module, inputs) of a case: built once, shared, never modified"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    torch.manual_seed(0)
    layer = _switch_off_output_dropout(m.MultiheadAttention(E, H, out_dense_depth=1, dropout=p))
    gen = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, L, E, generator=gen) for L in (Lq, Lk, Lk))
    mask, kpm = _mask(kind, B, Lq, Lk, gen)
    g_out, g_w = torch.randn(B, Lq, E, generator=gen), torch.randn(B, Lq, Lk, generator=gen) * 0.2
    rz = (torch.rand(B, Lq, generator=gen) < 0.3) if row_mask else None
    return layer, dict(q=q, k=k, v=v, mask=mask, kpm=kpm, g_out=g_out, g_w=g_w, rz=rz)


def _cuda(t):
    return None if t is None else t.cuda()


def _run_device(dev, c, need=(True, True, True)):
    """forward + backward of the device module -> [out, w, dq, dk, dv, parameter gradients...] (None where not asked for)"""
    qd, kd, vd = (c[n].clone().cuda().requires_grad_(r) for n, r in zip('qkv', need))
    for p_ in dev.parameters():
        p_.grad = None
    out, w = dev(qd, kd, vd, key_padding_mask=_cuda(c['kpm']), attn_mask=_cuda(c['mask']), out_row_mask=_cuda(c['rz']))
    ((out * c['g_out'].cuda()).sum() + (w * c['g_w'].cuda()).sum()).backward()
    grads = [None if t.grad is None else t.grad.cpu().numpy() for t in (qd, kd, vd)]
    return [out.detach().cpu().numpy(), w.detach().cpu().numpy(), *grads, *(p_.grad.cpu().numpy() for p_ in dev.parameters())]


def _run_restated(layer, c, counter, p, seed=SEED, instance=INSTANCE):
    B, Lq, E = c['q'].shape
    Lk, H = c['k'].shape[1], layer.num_heads
    kept = ref.mask(seed, instance, counter, B, H, Lq, Lk, p)
    l64 = copy.deepcopy(layer).double()
    q, k, v = (c[n].double().requires_grad_(True) for n in 'qkv')
    out, w = ref.module_forward(l64, q, k, v, kept, p, c['mask'], c['kpm'], c['rz'])
    ((out * c['g_out'].double()).sum() + (w * c['g_w'].double()).sum()).backward()
    return [t.detach().numpy() for t in (out, w, q.grad, k.grad, v.grad, *(p_.grad for p_ in l64.parameters()))], kept


def _fraction_of_cap(got, want, n_, p, B, Lq):
    """max over the entries of |got - want| / (rtol |want| + atol) with the CAP's rtol and atol: <= 1 is inside the cap"""
    s = 1.0 / (1.0 - p)
    atol = 3e-5 if n_ < 5 else 2e-7 * B * Lq * max(1.0, float(np.abs(want).max()) ** 0.5) + 3e-5
    return float((np.abs(got - want) / (s * (3e-4 * np.abs(want) + atol))).max())


def _assert_close(got, want, p, B, Lq, only=None, label=''):
    tol = TOL[f'p={p}']
    for n_, (a, b) in enumerate(zip(got, want)):
        name = NAMES[n_] if n_ < 5 else 'parameter_gradients'
        if a is None or (only is not None and name not in only):
            continue
        assert np.isfinite(a).all(), name
        frac = _fraction_of_cap(a, b, n_, p, B, Lq)
        print(f'attn dropout {label} p={p} {name}[{n_}]: {frac:.4f} of the cap (tolerance {tol[name]:.4f})')
        assert tol[name] <= 1.0
        assert frac <= tol[name], f'{name} (output {n_}): {frac:.4f} of the cap, tolerance {tol[name]:.4f}'


def _device_layer(layer, counter=0):
    return copy.deepcopy(layer).cuda().reseed(SEED, counter=counter, instance_id=INSTANCE)


@pytest.mark.parametrize('kind', ['batch', 'none'])
@pytest.mark.parametrize('B,Lq,Lk,E,H', SHAPES)
def test_zeros_of_the_weights_are_the_restated_mask(B, Lq, Lk, E, H, kind):
    p = 0.5
    layer, c = _case(B, Lq, Lk, E, H, kind, p)
    dev = _device_layer(layer, counter=5)
    with torch.no_grad():
        _, w = dev(c['q'].cuda(), c['k'].cuda(), c['v'].cuda(), key_padding_mask=_cuda(c['kpm']), attn_mask=_cuda(c['mask']))
    assert dev.dropout_drawn() == 5
    kept = ref.mask(SEED, INSTANCE, 5, B, H, Lq, Lk, p)
    blocked = ref.blocked_mask(B, Lq, Lk, c['mask'], c['kpm'])
    expect_zero = ~kept.any(axis=1)                                   # every head dropped it
    live = np.ones((B, Lq, Lk), bool)
    if blocked is not None:
        dead = blocked.all(-1, keepdim=True)
        live = (~blocked & ~dead).numpy()                             # (a dead row attends unmasked and is zeroed by keep)
        expect_zero = expect_zero | ~live
    got_zero = w.cpu().numpy() == 0
    assert (got_zero == expect_zero).all(), f'{int((got_zero != expect_zero).sum())} entries differ'
    # the test cannot pass with an empty (or a full) mask
    dropped = 1.0 - kept.transpose(0, 2, 3, 1)[live].mean()
    assert 0.25 <= dropped <= 0.75
    if H == 1:
        assert 0.25 <= got_zero[live].mean() <= 0.75
    else:
        assert got_zero[live].any() or 0.5 ** H * live.sum() < 4


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('kind', ['batch', 'none'])
@pytest.mark.parametrize('B,Lq,Lk,E,H', SHAPES)
def test_values_match_the_restatement(B, Lq, Lk, E, H, kind, p):
    from asac_amd import native
    row_mask = (B, Lq, Lk, E, H, kind) == (4, 20, 27, 40, 8, 'batch')      # one shape also runs with `out_row_mask`
    layer, c = _case(B, Lq, Lk, E, H, kind, p, row_mask)
    dev = _device_layer(layer, counter=3)
    with native.LaunchProfiler() as prof:      # (every launch issued 20 times: the repetitions draw alike and count once)
        got = _run_device(dev, c)
    seen = prof.summary()
    assert seen['asac_attention_mh_dropout_forward']['calls'] == 1 and seen['asac_attention_mh_dropout_backward']['calls'] == 1
    assert 'asac_attention_mh_forward' not in seen and 'asac_attention_mh_backward' not in seen
    assert dev.dropout_drawn() == 3 and dev.dropout_state() == (4, 0)
    want, _ = _run_restated(layer, c, 3, p)
    _assert_close(got, want, p, B, Lq, label=f'{(B, Lq, Lk, E, H)} {kind}')


@pytest.mark.parametrize('which', ['dv', 'dk'])
def test_turned_tiles_hold_the_right_weights(which):
    """the products over the queries read two tiles turned through LDS: dV's holds the DROPPED weights Pd, dK's holds dS.
    Each gradient alone, against the restatement — and far from what the other tile's content would give."""
    B, Lq, Lk, E, H, p = 4, 20, 27, 40, 8, 0.5
    layer, c = _case(B, Lq, Lk, E, H, 'batch', p)
    dev = _device_layer(layer, counter=11)
    got = _run_device(dev, c, need=(False, which == 'dk', which == 'dv'))
    want, kept = _run_restated(layer, c, 11, p)
    n_ = NAMES.index(which)
    assert got[n_] is not None and all(got[j] is None for j in (2, 3, 4) if j != n_)
    _assert_close(got, want, p, B, Lq, only=(which,), label=f'only {which}')
    # the same gradient with ANOTHER mask (what a tile holding P instead of Pd, or a mask of another call, amounts to) is far
    # away: the comparison above can tell them apart
    other, _ = _run_restated(layer, c, 12, p)
    assert np.abs(other[n_] - want[n_]).max() > 100 * 3e-5


def test_counter_protocol():
    B, Lq, Lk, E, H, p = 70, 9, 18, 12, 2, 0.5
    layer, c = _case(B, Lq, Lk, E, H, 'none', p)
    dev = _device_layer(layer, counter=100)
    assert dev.dropout_state() is None, 'the state is created at the first dropout launch'
    q, k, v = (c[n].cuda() for n in 'qkv')

    def acting():
        with torch.no_grad():      # training mode without gradients (acting) drops and advances as well
            return dev(q, k, v)[1].cpu().numpy()

    ws = [acting() for _ in range(4)]
    assert dev.dropout_drawn() == 103 and dev.dropout_state() == (104, 0), 'n calls advance by n; arrival words zero'
    for n, w in enumerate(ws):
        kept = ref.mask(SEED, INSTANCE, 100 + n, B, H, Lq, Lk, p)
        assert ((w == 0) == ~kept.any(axis=1)).all()
    assert all((ws[0] != w).any() for w in ws[1:]), 'different counters give different masks'
    # with gradients: the same counter advances, the backward follows its forward
    got = _run_device(dev, c)
    assert dev.dropout_drawn() == 104 and dev.dropout_state()[0] == 105
    want, _ = _run_restated(layer, c, 104, p)
    _assert_close(got, want, p, B, Lq, label='counter 104')
    # the same (seed, instance, counter) gives the same bits twice
    dev.reseed(SEED, counter=101, instance_id=INSTANCE)
    again = acting()
    assert dev.dropout_drawn() == 101 and np.array_equal(again, ws[1])
    dev.reseed(SEED + 1, counter=101, instance_id=INSTANCE)
    assert not np.array_equal(acting(), ws[1])
    # a copy made BEFORE the first launch has an instance id of its own
    a, b = copy.deepcopy(layer).cuda(), copy.deepcopy(layer).cuda()
    torch.manual_seed(9)
    with torch.no_grad():
        wa, wb = a(q, k, v)[1], b(q, k, v)[1]
    assert a._drop_instance != b._drop_instance and a._drop_seed == b._drop_seed == 9 and not torch.equal(wa, wb)
    assert set(a.state_dict()) == set(layer.state_dict())


def test_a_module_applied_twice_keeps_both_counters():
    """two forwards of one module before their backwards (observations and next observations): each backward regenerates
    the mask of ITS forward"""
    B, Lq, Lk, E, H, p = 3, 7, 5, 24, 2, 0.5
    layer, c = _case(B, Lq, Lk, E, H, 'batch', p)
    dev = _device_layer(layer, counter=40)
    q1, q2 = (c['q'].clone().cuda().requires_grad_(True) for _ in range(2))
    k, v, am, kpm = c['k'].cuda(), c['v'].cuda(), c['mask'].cuda(), c['kpm'].cuda()
    o1, w1 = dev(q1, k, v, attn_mask=am, key_padding_mask=kpm)
    o2, w2 = dev(q2, k, v, attn_mask=am, key_padding_mask=kpm)
    g_out, g_w = c['g_out'].cuda(), c['g_w'].cuda()
    ((o1 * g_out).sum() + (w1 * g_w).sum() + (o2 * g_out).sum() + (w2 * g_w).sum()).backward()
    for counter, qd in ((40, q1), (41, q2)):
        want, _ = _run_restated(layer, c, counter, p)
        _assert_close([None, None, qd.grad.cpu().numpy()], want, p, B, Lq, label=f'applied twice, counter {counter}')


def test_captured_block_draws_afresh_on_every_replay():
    from algorithm.captured_step import CapturedStep
    B, Lq, Lk, E, H, p = 4, 20, 27, 40, 8, 0.5
    layer, c = _case(B, Lq, Lk, E, H, 'batch', p)
    dev = _device_layer(layer, counter=0)
    xq, xk, xv = (c[n].clone().cuda().requires_grad_(True) for n in 'qkv')
    am, kpm, g_out, g_w = (c[n].cuda() for n in ('mask', 'kpm', 'g_out', 'g_w'))

    def step():
        xq.grad = xk.grad = xv.grad = None
        out, w = dev(xq, xk, xv, attn_mask=am, key_padding_mask=kpm)
        ((out * g_out).sum() + (w * g_w).sum()).backward()
        return out.detach(), w.detach(), xq.grad, xk.grad, xv.grad

    step()                                                  # eager: creates the state (counter 0 -> 1)
    torch.cuda.synchronize()
    captured = CapturedStep.capture(step, torch.device('cuda:0'))
    torch.cuda.synchronize()
    first = dev.dropout_state()[0]
    assert first == 1, 'capturing launches nothing'
    outs = []
    for n in range(3):
        captured.replay(direct=False)
        torch.cuda.synchronize()
        assert dev.dropout_drawn() == first + n
        got = [t.cpu().numpy() for t in captured.payload]
        want, _ = _run_restated(layer, c, first + n, p)
        _assert_close(got, want[:5], p, B, Lq, label=f'replay {n}')
        outs.append(got[0])
    assert dev.dropout_state() == (first + 3, 0)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2]) and not np.array_equal(outs[0], outs[2])


def test_first_call_under_capture_runs_the_module_code():
    from algorithm.captured_step import CapturedStep
    B, Lq, Lk, E, H, p = 3, 7, 5, 24, 2, 0.5
    layer, c = _case(B, Lq, Lk, E, H, 'none', p)
    dev = copy.deepcopy(layer).cuda()
    q, k, v = (c[n].cuda() for n in 'qkv')

    def step():
        with torch.no_grad():
            return dev(q, k, v)

    captured = CapturedStep.capture(step, torch.device('cuda:0'))      # allocating and seeding are not part of a capture
    captured.replay(direct=False)
    torch.cuda.synchronize()
    assert dev.dropout_state() is None
    out, w = captured.payload
    assert torch.isfinite(out).all() and 0.05 < float((w == 0).float().mean()) < 0.6


def test_paths_without_active_dropout_do_not_move(monkeypatch):
    from asac_amd import native
    from algorithm import fused_attention
    from algorithm.nn_models.layers import seq_layers
    B, Lq, Lk, E, H = 4, 20, 27, 40, 8
    layer, c = _case(B, Lq, Lk, E, H, 'batch', 0.5)
    args = dict(key_padding_mask=c['kpm'].cuda(), attn_mask=c['mask'].cuda())
    g_out, g_w = c['g_out'].cuda(), c['g_w'].cuda()

    def run(dev):
        qd, kd, vd = (c[n].clone().cuda().requires_grad_(True) for n in 'qkv')
        with native.LaunchProfiler(repeat=1) as prof:
            out, w = dev(qd, kd, vd, **args)
            ((out * g_out).sum() + (w * g_w).sum()).backward()
        return [out.detach(), w.detach(), qd.grad, kd.grad, vd.grad], prof.summary()

    # the launch the parent makes, called directly: q / k / v projections by the module, then `_AttnMhFn`
    import algorithm.nn_models as m
    torch.manual_seed(0)
    zero = m.MultiheadAttention(E, H, out_dense_depth=1, dropout=0.).cuda()      # dropout = 0 in training mode
    zero.load_state_dict(layer.state_dict())
    evald = copy.deepcopy(layer).cuda().eval()                                   # dropout = 0.5 under .eval()
    for name, dev in (('dropout=0', zero), ('eval', evald)):
        got, seen = run(dev)
        assert seen['asac_attention_mh_forward']['calls'] == 1 and seen['asac_attention_mh_backward']['calls'] == 1, name
        assert not any('dropout' in k for k in seen), name
        assert dev.dropout_state() is None and dev._drop_used is None, f'{name}: no state is created'
        qp, kp, vp = (proj(c[n].cuda()) for proj, n in zip((dev.q_proj, dev.k_proj, dev.v_proj), 'qkv'))
        mask3 = torch.logical_or(c['mask'].cuda(), c['kpm'].cuda().unsqueeze(1))
        o_core, w_core, *_ = fused_attention._AttnMhFn.apply(qp.detach(), kp.detach(), vp.detach(), mask3, H, None)
        assert torch.equal(got[1], w_core), f'{name}: the weights are the plain launch\'s, bit for bit'
    got_zero, got_eval = run(zero)[0], run(evald)[0]
    # (the output stack differs — a fused ResBlock launch without its nn.Dropout, module code with it — the core does not)
    assert torch.equal(got_zero[1], got_eval[1])
    for a, b in zip(got_zero, got_eval):
        torch.testing.assert_close(a, b, rtol=3e-4, atol=3e-5)
    # the switch off: a training module runs the module code (torch's draws; nothing of the dropout launch)
    monkeypatch.setattr(seq_layers, 'FUSED_ATTN_DROPOUT', False)
    dev = copy.deepcopy(layer).cuda()
    got, seen = run(dev)
    assert not any('attention_mh' in k for k in seen) and dev.dropout_state() is None
    assert all(torch.isfinite(t).all() for t in got)
    # p = 1 is outside the launch's envelope whatever the switch says: module code (everything dropped)
    monkeypatch.setattr(seq_layers, 'FUSED_ATTN_DROPOUT', True)
    torch.manual_seed(0)
    ones = m.MultiheadAttention(E, H, dropout=1.).cuda()
    got, seen = run(ones)
    assert not any('attention_mh' in k for k in seen) and ones.dropout_state() is None
    assert float(got[1].abs().max()) == 0.
