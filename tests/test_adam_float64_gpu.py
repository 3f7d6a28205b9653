"""GPU: every Adam launch against one float64 step of torch's single-tensor Adam from an arbitrary state
(`adam_ref.step64`, itself held to `torch.optim.Adam` in float64 by tests/test_adam_ref_host.py): `asac_adam_step` (float4
path, scalar tail, wholly scalar path of misaligned views, grid-stride rounds), `asac_adam_step_partials` (tile sums on both
sides of sixteen, first-parameter path and the loop behind it) and `asac_alpha_adam_step` (the `i >= 256` tail, the counter)
with its hosted forms.  Parameters AND both moments are compared, under the rule of the categorical kernels
(`discrete_ref.over_the_bound`): per tensor the kernel's largest absolute error may be at most twice that of
`torch.optim.Adam` in float32 on the device, floor 4 units in the last place at the tensor's largest magnitude.  Every
tensor of a case is of one magnitude (one gradient scale per case, p = 0 where the update itself is to be seen), so that a
relative error in small elements cannot hide under large ones.

Worst share of the bound per entry point (kernel error / bound; 1 = at the bound), MI355X, measured 2026-10-21:
  asac_adam_step            0.48  (param at steps_done = 0, scale 1, p = 0, lr 0.1: kernel 2.30e-08, eager 2.13e-08, floor 4.77e-08)
  asac_adam_step_partials   0.58  (grad at E = 3, stride 1000, 33 tiles: kernel 3.19e-07, eager 1.25e-07, floor 5.47e-07)
  asac_alpha_adam_step      0.52  (exp_avg_sq at B = 255, n = 2, steps_done = 0: kernel 3.32e-09, eager 3.20e-09, floor 5.93e-09)
With the step count off by one in `adam_bias_terms` the p = 0 cases of `asac_adam_step` at steps_done 0, 1, 9 and 999 stand
at 560 to 700 000 times the bound (later ones cannot tell: both powers have vanished), with eps inside the bias division of
`adam1` those at gradient scale 1e-6 at 39 000 to 1.4 million times (scratch builds, same date)."""
import numpy as np
import pytest
import torch

from tests import adam_ref as ar
from tests import discrete_ref as dr

pytestmark = pytest.mark.gpu

NAMES = ('param', 'exp_avg', 'exp_avg_sq')


@pytest.fixture(scope='module')
def nat():
    from asac_amd import native
    native.load()
    assert torch.cuda.is_available()
    return native


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _same_bits(t, array):
    return np.array_equal(t.detach().cpu().numpy().view(np.uint32), np.ascontiguousarray(array, dtype=np.float32).view(np.uint32))


def _report(entry, bad, share):
    print(f'{entry}: worst share of the bound {share:.3f}')
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- asac_adam_step

def adam_step_case(nat, tag, state, done, hyper, shifts=(0, 0, 0, 0)):
    """one launch on guarded views of `state` = (p, g, m, v) -> (tensors over the bound, share)"""
    p, g, m, v = state
    guard = ar.GuardedViews()
    dp, dg, dm, dv = (guard(x, s) for x, s in zip(state, shifts))
    steps = torch.tensor([done], dtype=torch.int64, device='cuda')
    nat.adam_step(dp, dg, dm, dv, *hyper, steps)
    torch.cuda.synchronize()
    guard.check()
    assert _same_bits(dg, g), f'{tag}: the gradient was written'
    assert int(steps.item()) == done, f'{tag}: the counter was written'
    want = dict(zip(NAMES, ar.step64(p, g, m, v, done + 1, *hyper)))
    kernel = dict(zip(NAMES, (_f64(dp), _f64(dm), _f64(dv))))
    yardstick = dict(zip(NAMES, ar.eager(p, g, m, v, done + 1, *hyper)))
    return dr.over_the_bound(tag, want, kernel, yardstick)


def test_adam_step_values_against_float64(nat):
    """n = 10007: every step count x gradient scale x (p drawn, p = 0) x hyper-parameter set, and g = m = v = 0"""
    rng = np.random.default_rng(3)
    bad, share = [], 0.
    for done, scale, p_zero, hyper, all_zero in ar.value_cases():
        tag = f'adam_step done={done} scale={scale:g} p={"0" if p_zero else "N(0,1)"} lr={hyper[0]:g}' + (' all-zero' if all_zero else '')
        state = ar.make_state(rng, 10007, done, scale, p_zero, all_zero)
        b, s = adam_step_case(nat, tag, state, done, hyper)
        bad += [(tag, *x) for x in b]
        share = max(share, s)
    _report('asac_adam_step values', bad, share)


@pytest.mark.parametrize('shifts', [(0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 1)], ids=['aligned', 'all-shifted', 'exp_avg_sq-shifted'])
def test_adam_step_shapes_and_alignment_against_float64(nat, shifts):
    """steps_done = 9, default hyper-parameters: sizes around the float4 width and the workgroup, all four views 16-byte
    aligned / all one float off / only exp_avg_sq off (the scalar path for everything), p drawn and p = 0"""
    rng = np.random.default_rng(4)
    bad, share = [], 0.
    for n in (1, 3, 4, 5, 255, 1023, 10007):
        for p_zero in (False, True):
            tag = f'adam_step n={n} shifts={shifts} p={"0" if p_zero else "N(0,1)"}'
            b, s = adam_step_case(nat, tag, ar.make_state(rng, n, 9, 1., p_zero), 9, ar.HYPER_DEFAULT, shifts)
            bad += [(tag, *x) for x in b]
            share = max(share, s)
    _report(f'asac_adam_step shapes {shifts}', bad, share)


def test_adam_step_second_round_of_the_float4_loop_against_float64(nat):
    """n = 2 * 2^21 + 7, aligned: 2^20 + 1 float4 items for the 2048 * 256 threads of the capped grid (a second and a
    third round of the loop) and a scalar tail of 3"""
    n = 2 * 2 ** 21 + 7
    state = ar.make_state(np.random.default_rng(5), n, 9, 1., True)
    _report('asac_adam_step large', *adam_step_case(nat, f'adam_step n={n}', state, 9, ar.HYPER_DEFAULT))


# ---------------------------------------------------------------------------------------------- asac_adam_step_partials

LOSS_ROWS = 96


def partials_case(nat, tag, rng, E, ms, used, tiles, accumulate, with_loss, p_zero, done=9, hyper=ar.HYPER_DEFAULT):
    """one launch.  Every parameter's partials (and its stored gradient) share a sign, so that no tile sum cancels: Adam
    normalises the gradient, and a cancelled one would make p' measure the summation order (asserted below in float64);
    the partials are 1 / tiles in size, so that the summed and the kept gradients are of one magnitude"""
    n = E * ms
    sign = np.where(rng.random(n) < 0.5, -1., 1.)

    def size(*shape):
        return np.clip(np.abs(rng.standard_normal(shape)), 0.1, 10.)
    partial = (sign.reshape(1, E, ms) * size(tiles, E, ms) / tiles).astype(np.float32)
    grad = (sign * size(n)).astype(np.float32)
    p = np.zeros(n, np.float32) if p_zero else rng.standard_normal(n).astype(np.float32)
    m, v = ar.draw(rng, n, 1.), ar.draw(rng, n, 1.) ** 2
    loss_partial = (rng.random((tiles, E)) + 0.5).astype(np.float32)
    workspace = ar.partials_workspace(partial, loss_partial if with_loss else None)

    guard = ar.GuardedViews()
    dp, dg, dm, dv, dws = (guard(x) for x in (p, grad, m, v, workspace))
    loss_out = guard(np.full(E, np.nan, np.float32)) if with_loss else None
    steps = torch.tensor([done], dtype=torch.int64, device='cuda')
    nat.adam_step_partials(dp, dg, dm, dv, *hyper, steps, dws, tiles, E, ms, used, accumulate, loss_out,
                           LOSS_ROWS if with_loss else 0)
    torch.cuda.synchronize()
    guard.check()
    assert _same_bits(dws, workspace), f'{tag}: the workspace was written'
    assert int(steps.item()) == done, f'{tag}: the counter was written'

    partial64, grad64 = partial.astype(np.float64), grad.astype(np.float64)
    g64 = ar.partials_gradient(np, partial64, grad64, used, accumulate)
    terms = np.abs(partial64).sum(0).reshape(-1) + (np.abs(grad64) if accumulate else 0.)
    summed = np.arange(n) % ms < used
    assert (np.abs(g64[summed]) >= 0.999 * terms[summed]).all(), 'a tile sum cancels'
    want = dict(zip(NAMES, ar.step64(p, g64, m, v, done + 1, *hyper)), grad=g64)
    kernel = dict(zip(NAMES, (_f64(dp), _f64(dm), _f64(dv))), grad=_f64(dg))
    g32 = ar.partials_gradient(torch, torch.from_numpy(partial).cuda(), torch.from_numpy(grad).cuda(), used, accumulate)
    g32 = g32.cpu().numpy()
    assert g32.dtype == np.float32
    yardstick = dict(zip(NAMES, ar.eager(p, g32, m, v, done + 1, *hyper)), grad=g32.astype(np.float64))
    if with_loss:
        want['loss'] = loss_partial.astype(np.float64).sum(0) / LOSS_ROWS
        kernel['loss'] = _f64(loss_out)
        yardstick['loss'] = _f64(torch.from_numpy(loss_partial).cuda().sum(0) / LOSS_ROWS)
    kept = ~summed
    assert np.array_equal(kernel['grad'][kept], grad64[kept]), f'{tag}: a gradient past `used` was written'
    return dr.over_the_bound(tag, want, kernel, yardstick)


@pytest.mark.parametrize('E', [1, 3])
def test_adam_step_partials_against_float64(nat, E):
    """(member_stride, used) x tiles on both sides of sixteen x accumulate x with / without the loss sums; p = 0 in the cases
    with the loss sums, drawn in the others"""
    rng = np.random.default_rng(6 + E)
    bad, share = [], 0.
    for ms, used in ((5, 5), (5, 2), (1000, 1000), (1000, 997)):
        for tiles in (1, 15, 16, 17, 33):
            for accumulate in (0, 1):
                for with_loss in (False, True):
                    tag = f'adam_partials E={E} stride={ms} used={used} tiles={tiles} acc={accumulate} loss={int(with_loss)}'
                    b, s = partials_case(nat, tag, rng, E, ms, used, tiles, accumulate, with_loss, p_zero=with_loss)
                    bad += [(tag, *x) for x in b]
                    share = max(share, s)
    _report(f'asac_adam_step_partials E={E}', bad, share)


def test_adam_step_partials_grid_stride_loop_against_float64(nat):
    """E = 3, member_stride = 200 000: n = 600 000 > 2048 * 256 threads, so the loop behind the first-parameter path runs
    (across a member boundary), here with an unused tail, accumulation and the loss sums"""
    rng = np.random.default_rng(9)
    _report('asac_adam_step_partials large',
            *partials_case(nat, 'adam_partials E=3 stride=200000 used=199997 tiles=2 acc=1 loss=1', rng, 3, 200000, 199997, 2, 1,
                           True, p_zero=True))


# ---------------------------------------------------------------------------------------------- asac_alpha_adam_step

TARGET = -2.


def alpha_inputs(rng, B, n, done, p_zero):
    """logp around -1.5 +- 1, so that the terms -logp - target are around 3.5 and their mean does not cancel; the stored
    gradients and the moments at that scale"""
    logp = (rng.standard_normal(B) - 1.5).astype(np.float32)
    p = np.zeros(n, np.float32) if p_zero else rng.standard_normal(n).astype(np.float32)
    grad = ar.draw(rng, n, 3.)
    if done == 0:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m, v = ar.draw(rng, n, 3.), ar.draw(rng, n, 3.) ** 2
    return logp, p, grad, m, v


def alpha_case(nat, tag, rng, B, n, slot, advance, done, p_zero, hyper=ar.HYPER_DEFAULT):
    logp, p, grad, m, v = alpha_inputs(rng, B, n, done, p_zero)
    guard = ar.GuardedViews()
    dlogp, dp, dg, dm, dv = (guard(x) for x in (logp, p, grad, m, v))
    steps = torch.tensor([done], dtype=torch.int64, device='cuda')
    nat.alpha_adam_step(dlogp, TARGET, slot, dp, dg, dm, dv, *hyper, steps, advance_counter=advance)
    torch.cuda.synchronize()
    guard.check()
    assert _same_bits(dlogp, logp), f'{tag}: logp was written'
    assert int(steps.item()) == done + int(advance), f'{tag}: the counter'

    # grad[slot] = mean(-logp) - target: one scalar from a sum that may cancel, so its floor is 4 units in the last place
    # at the size of what is summed, mean |term| (tests/test_option_gpu.py does the same for its returns)
    terms = -logp.astype(np.float64) - np.float64(np.float32(TARGET))
    g_slot, size = terms.sum() / B, np.abs(terms).mean()
    assert abs(g_slot) >= 0.1 * size, 'the mean cancels: the step of the slot would be ill-conditioned'
    g_eager = (-torch.from_numpy(logp).cuda() - TARGET).mean().cpu().numpy()
    assert g_eager.dtype == np.float32
    got = _f64(dg)
    e_k, e_m, floor = abs(got[slot] - g_slot), abs(float(g_eager) - g_slot), 4 * dr.ULP * size
    bound = max(2 * e_m, floor)
    print(f'{tag} grad[slot]: kernel {e_k:.3e}  eager {e_m:.3e}  floor {floor:.3e}  share {e_k / bound:.2f}')
    bad = [('grad[slot]', e_k, e_m, floor)] if not e_k <= bound else []
    others = np.arange(n) != slot
    assert np.array_equal(dg.cpu().numpy().view(np.uint32)[others], grad.view(np.uint32)[others]), f'{tag}: another gradient was written'

    # the slot steps with the new gradient, the others with their stored ones
    g64, g32 = grad.astype(np.float64), grad.copy()
    g64[slot], g32[slot] = g_slot, g_eager
    want = dict(zip(NAMES, ar.step64(p, g64, m, v, done + 1, *hyper)))
    kernel = dict(zip(NAMES, (_f64(dp), _f64(dm), _f64(dv))))
    yardstick = dict(zip(NAMES, ar.eager(p, g32, m, v, done + 1, *hyper)))
    b, share = dr.over_the_bound(tag, want, kernel, yardstick)
    return bad + b, max(share, e_k / bound)


def alpha_slots(n):
    return sorted({0, n - 1} | ({256} if n > 256 else set()))


@pytest.mark.parametrize('B', [1, 255, 256, 257, 1000])
def test_alpha_adam_step_against_float64(nat, B):
    """segment sizes up to the `i >= 256` tail with the slot in front, at the end and in the tail, the counter advanced or
    not, from zero state and after 999 steps, p drawn and p = 0"""
    rng = np.random.default_rng(10 + B)
    bad, share = [], 0.
    for n in (1, 2, 3, 257, 600):
        for slot in alpha_slots(n):
            for advance in (False, True):
                for done in (0, 999):
                    for p_zero in (False, True):
                        tag = f'alpha_adam B={B} n={n} slot={slot} advance={int(advance)} done={done} p={"0" if p_zero else "N(0,1)"}'
                        b, s = alpha_case(nat, tag, rng, B, n, slot, advance, done, p_zero)
                        bad += [(tag, *x) for x in b]
                        share = max(share, s)
    _report(f'asac_alpha_adam_step B={B}', bad, share)


@pytest.mark.parametrize('B,n,slot', [(255, 2, 1), (257, 257, 256), (1000, 600, 256)])
def test_hosted_temperature_steps_have_alpha_adam_step_s_bits(nat, B, n, slot):
    """The hosted forms of the temperature step — the sidecar of `sumtree_update` behind a `vtrace_return_min` that only
    previews it (`pending_alpha`: nothing written), and `alpha_step` of `td_update` — leave the bits of `alpha_adam_step`
    in the parameters, the gradients, both moments and the counter (the arrangement of tests/test_kernels_gpu.py
    `test_return_with_the_pending_temperature_step`, at segments with an `i >= 256` tail and the slot in it); the hosts
    want `slot` to be the temperature their return reads."""
    from tests.test_kernels_gpu import _vtrace_args
    rng = np.random.default_rng(B)
    done, hyper, steps_ret, E, C = 999, ar.HYPER_DEFAULT, 3, 2, 2048
    logp_a, p, grad, m, v = alpha_inputs(rng, B, n, done, False)
    gen = torch.Generator().manual_seed(B)
    f = dict(device='cuda')

    def rand(*shape):
        return torch.randn(*shape, generator=gen).cuda()
    q, logp, reward, q_on = rand(E, B, steps_ret + 1), rand(B, steps_ret + 1), rand(B, steps_ret), rand(E, B)
    done_m, last, pad = (torch.rand(B, steps_ret, generator=gen).cuda() < x for x in (0.1, 0.05, 0.1))
    gr, lr = torch.logspace(0, steps_ret - 1, steps_ret, 0.99).cuda(), torch.logspace(0, steps_ret - 1, steps_ret, 0.95).cuda()
    ids = torch.from_numpy(rng.permutation(C)[:B].astype(np.int64)).cuda()

    def run(form):
        guard = ar.GuardedViews()
        dlogp, dp, dg, dm, dv = (guard(x) for x in (logp_a, p, grad, m, v))
        steps = torch.tensor([done], dtype=torch.int64, device='cuda')
        tree, slot_ids = torch.zeros(2 * C - 1, **f), torch.arange(C, dtype=torch.int64, device='cuda')
        winner, nan_flag = torch.full((C + 2 * 4096,), -1, dtype=torch.int32, **f), torch.zeros(1, dtype=torch.int32, **f)
        y, td = torch.zeros(B, **f), torch.zeros(B, **f)
        a = _vtrace_args(nat, q=q, logp=logp, log_alpha=dp[slot:], reward=reward, done=done_m, last=last, pad=pad, mu=None,
                         pi=None, A=1, gamma_ratio=gr, lambda_ratio=lr, gamma=0.99, rho=1.0, c=1.0, use_is=False, y=y,
                         q_online=q_on, td=td)
        job = nat.sidecar_alpha_adam(dlogp, TARGET, slot, dp, dg, dm, dv, *hyper, steps, advance_counter=True)
        if form == 'plain':
            nat.alpha_adam_step(dlogp, TARGET, slot, dp, dg, dm, dv, *hyper, steps, advance_counter=True)
            nat.vtrace_return_min(a)
            nat.sumtree_update(tree, C, ids, slot_ids, td, 0.9, 0.01, 1.0, 0, winner, nan_flag)
        elif form == 'pending + sidecar':
            nat.vtrace_return_min(a, pending_alpha=job)
            torch.cuda.synchronize()
            for name, t, before in zip(('param', 'grad', 'exp_avg', 'exp_avg_sq'), (dp, dg, dm, dv), (p, grad, m, v)):
                assert _same_bits(t, before), f'the return launch only previews the step: {name} written'
            assert int(steps.item()) == done
            nat.sumtree_update(tree, C, ids, slot_ids, td, 0.9, 0.01, 1.0, 0, winner, nan_flag, sidecars=[job])
        else:
            nat.td_update(a, tree, C, ids, slot_ids, 0.9, 0.01, 1.0, winner, nan_flag, alpha_step=job)
        torch.cuda.synchronize()
        guard.check()
        assert int(nan_flag.item()) == 0
        return [dp, dg, dm, dv, steps, y, td, tree]

    want = run('plain')
    assert int(want[4].item()) == done + 1 and not _same_bits(want[0][slot:slot + 1], p[slot:slot + 1])
    for form in ('pending + sidecar', 'td_update'):
        for name, w_, g_ in zip(('param', 'grad', 'exp_avg', 'exp_avg_sq', 'steps', 'y', 'td', 'tree'), want, run(form)):
            assert torch.equal(w_, g_), (form, name)
