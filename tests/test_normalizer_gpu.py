"""GPU: the two launches of observation normalization (csrc/normalize.hip) through their owner
(`algorithm/normalizer.Normalizer`).

Whiten: against `torch.clamp((o - m) / torch.sqrt(v / (step + 1)), -5, 5)` evaluated on the device, BIT FOR BIT (NaN equal
to NaN): the launch is the same IEEE operations in the same order, without contraction.

Update: against the reference recurrence in float64.  The mean's sum is checked on its own; the variance's sum is
evaluated in float64 from the kernel's own float32 `mean'`.  Per column the bound is gamma * (sum_t |term_t| + |old value|),
gamma = (ceil(T / P) + log2 P + 4) * 2^-24 with P = `native.NORM_ROW_LANES`: the kernel's longest addition chain (a lane's
rows, then the tree) plus the roundings of the term itself (difference, quotient or product, the final addition to the
old value).  Derived, not measured; a dropped row is about 1 / T of sum |term|, far outside it."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _normalizer(shapes, step=0, seed=0):
    import asac_amd  # noqa: F401
    from algorithm.normalizer import Normalizer
    nz = Normalizer(shapes, torch.device('cuda:0'))
    gen = torch.Generator().manual_seed(seed)
    for m, v in zip(nz.running_means, nz.running_variances):
        m.copy_(torch.randn(m.shape, generator=gen))
        v.copy_(torch.rand(v.shape, generator=gen) * 50 + 0.5)
    nz.normalizer_step.fill_(step)
    return nz


def _expression(nz, obs_list):
    return [torch.clamp((o - m) / torch.sqrt(v / (nz.normalizer_step + 1)), -5, 5)
            for o, m, v in zip(obs_list, nz.running_means, nz.running_variances)]


def _launches(fn):
    from asac_amd import native
    with native.LaunchProfiler(repeat=1) as prof:
        out = fn()
    return out, {k: v['calls'] for k, v in prof.summary().items()}


def _same_bits(got, want):
    torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------
# whiten
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', [0, 119, 2 ** 24 + 1])
@pytest.mark.parametrize('rows,shape', [(1, (1,)), (6, (6,)), (5, (67,)), (4, (3, 5, 7)), (3, (4096 + 4,))])
def test_whiten_equals_the_module_expression_bit_for_bit(rows, shape, step):
    nz = _normalizer([shape], step, seed=rows)
    gen = torch.Generator().manual_seed(17)
    x = (torch.randn((rows, *shape), generator=gen) * 30).cuda()       # (values beyond both clamp edges)
    (got,), calls = _launches(lambda: nz.whiten([x]))
    assert calls == {'asac_obs_whiten': 1}
    want, = _expression(nz, [x])
    assert (want.abs() == 5).any() or rows * math.prod(shape) < 4
    _same_bits(got, want)
    # two leading dimensions ([B, L, *shape], as the learner's window) fold into rows
    x3 = x.unsqueeze(0).expand(2, *x.shape).contiguous()
    _same_bits(nz.whiten([x3])[0], _expression(nz, [x3])[0])


def test_whiten_clamp_edges_zero_variance_and_nan():
    nz = _normalizer([(8,)], 119)
    nz.running_variances[0][:4] = 0.
    x = torch.randn(6, 8).cuda() * 100
    x[0, :2] = nz.running_means[0][:2]            # x == mean at zero variance: 0 / 0
    x[1, 5] = float('nan')
    x[2, 6], x[3, 6] = float('inf'), float('-inf')
    got, want = nz.whiten([x])[0], _expression(nz, [x])[0]
    assert torch.isnan(want[0, :2]).all() and torch.isnan(want[1, 5])
    assert set(want[1:, :4].flatten().tolist()) == {-5., 5.}          # +-inf, then the clamp
    assert (want[:, 4:] == 5).any() and (want[:, 4:] == -5).any()
    _same_bits(got, want)


def test_whiten_views_inside_a_pitch_and_in_place():
    nz = _normalizer([(6,)], 7)
    src_buf, dst_buf = torch.randn(5, 3, 8).cuda() * 4, torch.full((5, 3, 8), 77., device='cuda')
    src, dst = src_buf[..., :6], dst_buf[..., 1:7]                     # D = 6 in a pitch of 8 floats, both sides
    want, = _expression(nz, [src])
    raw = src_buf.clone()
    out, calls = _launches(lambda: nz.whiten([src], out=[dst]))
    assert calls == {'asac_obs_whiten': 1} and out[0] is dst
    _same_bits(dst, want)
    assert torch.equal(src_buf, raw), 'the source is only read'
    assert (dst_buf[..., 0] == 77).all() and (dst_buf[..., 7] == 77).all(), 'nothing outside the view is written'
    # in place, dense and inside the pitch
    for x in (torch.randn(7, 6).cuda() * 4, src):
        want, = _expression(nz, [x])
        _, calls = _launches(lambda: nz.whiten([x], out=[x]))
        assert calls == {'asac_obs_whiten': 1}
        _same_bits(x, want)
    assert torch.equal(src_buf[..., 6:], raw[..., 6:])


def test_whiten_refuses_overlapping_buffers():
    from asac_amd import native
    nz = _normalizer([(6,)], 7)
    buf = torch.randn(40).cuda()
    src, dst = buf[:24].view(4, 6), buf[6:30].view(4, 6)
    jobs = native.whiten_jobs([(src, dst, nz.running_means[0], nz.running_variances[0])])
    with pytest.raises(native.AsacNativeError, match='overlap'):
        native.obs_whiten(jobs, nz.normalizer_step)


@pytest.mark.parametrize('n_jobs', [2, 8, 9])
def test_whiten_several_observations_in_one_launch(n_jobs):
    shapes = [(1,), (6,), (67,), (3, 5, 7), (4100,), (4,), (2, 2), (33,), (5,)][:n_jobs]
    nz = _normalizer(shapes, 119)
    obs = [(torch.randn(3, 2, *s) * 10).cuda() for s in shapes]
    got, calls = _launches(lambda: nz.whiten(obs))
    if n_jobs <= 8:
        assert calls == {'asac_obs_whiten': 1}
    else:
        assert 'asac_obs_whiten' not in calls, 'nine observations: the module expression'
    for g, w in zip(got, _expression(nz, obs)):
        _same_bits(g, w)


def test_whiten_static_buffers_are_built_once_and_follow_the_statistics():
    nz = _normalizer([(6,), (3, 4)], 10)
    obs = [torch.randn(4, 3, 6).cuda(), torch.randn(4, 3, 3, 4).cuda()]
    first = nz.whiten(obs, static=True)
    assert nz.whitened is first
    obs[0].normal_()
    nz.running_means[0].add_(1.)
    nz.normalizer_step.add_(50)
    again = nz.whiten(obs, static=True)
    assert all(a is b for a, b in zip(first, again)) and len(nz._tables) == 1
    for g, w in zip(again, _expression(nz, obs)):
        _same_bits(g, w)


# ------------------------------------------------------------------------------------------------------------------------
# update
# ------------------------------------------------------------------------------------------------------------------------
def _gamma(T):
    from asac_amd import native
    P = native.NORM_ROW_LANES
    return (math.ceil(T / P) + math.log2(P) + 4) * 2. ** -24


def _check_update(x, mean0, var0, step0, mean1, var1):
    """x [T, D] as the kernel took it (float32 or uint8), statistics before and after, flat per column"""
    T = x.shape[0]
    x64 = x.double().reshape(T, -1).cpu().numpy()
    m0, v0 = mean0.double().reshape(-1).cpu().numpy(), var0.double().reshape(-1).cpu().numpy()
    m1, v1 = mean1.double().reshape(-1).cpu().numpy(), var1.double().reshape(-1).cpu().numpy()
    g = _gamma(T)
    d = x64 - m0
    terms = d / float(step0 + T)
    bound_m = g * (np.abs(terms).sum(0) + np.abs(m0))
    err_m = np.abs(m1 - (m0 + terms.sum(0)))
    print(f'normalizer update T={T} D={x64.shape[1]}: mean error / bound {float((err_m / bound_m).max()):.3f}')
    assert (err_m <= bound_m).all(), float((err_m / bound_m).max())
    terms = (x64 - m1) * d                   # (from the kernel's own float32 mean')
    bound_v = g * (np.abs(terms).sum(0) + np.abs(v0))
    err_v = np.abs(v1 - (v0 + terms.sum(0)))
    print(f'normalizer update T={T} D={x64.shape[1]}: variance error / bound {float((err_v / bound_v).max()):.3f}')
    assert (err_v <= bound_v).all(), float((err_v / bound_v).max())


@pytest.mark.parametrize('shape', [(1,), (6,), (67,), (3, 5, 7)])
@pytest.mark.parametrize('T', [1, 2, 65, 257, 1000])
def test_update_against_the_float64_recurrence(T, shape):
    nz = _normalizer([shape], 37, seed=T)
    gen = torch.Generator().manual_seed(T * 131 + len(shape))
    x = (torch.randn((T, *shape), generator=gen) * 3 + 1.5).cuda()
    m0, v0 = nz.running_means[0].clone(), nz.running_variances[0].clone()
    _, calls = _launches(lambda: nz.update([x]))
    assert calls == {'asac_normalizer_update': 1}
    assert nz.normalizer_step.dtype == torch.int32 and int(nz.normalizer_step) == 37 + T
    assert int(nz._counter) == 0
    _check_update(x, m0, v0, 37, nz.running_means[0], nz.running_variances[0])


def test_update_takes_uint8_as_its_integer_value():
    nz = _normalizer([(3, 5, 7)], 37)
    x = torch.randint(0, 256, (65, 3, 5, 7), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    m0, v0 = nz.running_means[0].clone(), nz.running_variances[0].clone()
    _, calls = _launches(lambda: nz.update([x]))
    assert calls == {'asac_normalizer_update': 1} and int(nz.normalizer_step) == 102 and int(nz._counter) == 0
    _check_update(x, m0, v0, 37, nz.running_means[0], nz.running_variances[0])


def test_update_other_dtypes_keep_the_eager_code():
    nz = _normalizer([(6,)], 37)
    x = torch.randn(40, 6, dtype=torch.float64).cuda()
    _, calls = _launches(lambda: nz.update([x]))
    assert 'asac_normalizer_update' not in calls and int(nz.normalizer_step) == 77


def test_update_two_observations_two_calls_and_equal_bits():
    shapes = [(6,), (3, 30, 30)]
    gen = torch.Generator().manual_seed(5)
    ep = [[(torch.randn((T, *s), generator=gen) * 2).cuda() for s in shapes] for T in (40, 30)]

    def run():
        nz = _normalizer(shapes, 37)
        before = [[t.clone() for t in nz.running_means + nz.running_variances]]
        for obs in ep:
            _, calls = _launches(lambda: nz.update(obs))
            assert calls == {'asac_normalizer_update': 1}, 'one launch for all observations'
            assert int(nz._counter) == 0
            before.append([t.clone() for t in nz.running_means + nz.running_variances])
        return nz, before

    nz, hist = run()
    assert int(nz.normalizer_step) == 37 + 40 + 30 and nz.normalizer_step.dtype == torch.int32
    step = 37
    for obs, b, a in zip(ep, hist[:-1], hist[1:]):
        for i in range(2):
            _check_update(obs[i], b[i], b[2 + i], step, a[i], a[2 + i])
        step += obs[0].shape[0]
    nz2, hist2 = run()                       # equal state, equal input: equal bits
    assert torch.equal(nz.flat, nz2.flat) and int(nz2.normalizer_step) == int(nz.normalizer_step)


def test_update_under_the_repeat_knob_counts_the_episode_once():
    from asac_amd import native
    shapes = [(6,), (3, 5, 7)]
    gen = torch.Generator().manual_seed(9)
    obs = [(torch.randn((257, *s), generator=gen)).cuda() for s in shapes]
    plain, repeated = _normalizer(shapes, 37), _normalizer(shapes, 37)
    plain.update(obs)
    with native.LaunchProfiler(repeat=20):
        repeated.update(obs)
    assert int(repeated.normalizer_step) == 37 + 257 == int(plain.normalizer_step)
    assert torch.equal(plain.flat, repeated.flat)
    assert int(repeated._counter) == 0 and int(plain._counter) == 0
