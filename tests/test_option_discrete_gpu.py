"""GPU: the pure-discrete, policy-based option on the native path (`hip_config['fused_option_discrete']`,
`asac_option_discrete_return` in csrc/discrete.hip; `algorithm/oc/option_base.py` `_get_y` / `_get_td_error` /
`compute_rep_q_grads`).

  * the launch alone against a float64 NumPy restatement of the reference lines (option_base.py:287, 333-373 + _v_trace)
    written here; the bound of a case is 4x the error the float32 PyTorch-ROCm composition of the same lines (the eager
    branch of `OptionBase._get_y`, restated here) shows against float64, pooled over the case's (n, IS) family and
    measured per row against the size of what the row sums; no floor (the scheme and the margin of
    tests/test_option_gpu.py::test_option_return_against_float64; 4x: DESIGN.md s.5)
  * beta == 0 and E_sample == 1: the bits of `asac_discrete_return`
  * step t pairs with position t + 1: what beta == 1 / beta == 0 must hide stays hidden
  * bad arguments are refused without a launch
  * the reference's own numbers: `_get_y` on tables (`f19_option_discrete_get_y.npz`) and two full call sequences
    (`f19_option_discrete_pd32.npz`, `..._pd4_n1.npz`), switch on and off, the off path's error measured in the same run
  * launch accounting, and `d_y` a fresh tensor per call"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import discrete_ref as dr  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.test_option_gpu import (EPS32, OPTIMIZER_OF, UNDETERMINED_ABS, UNDETERMINED_MAX_SHARE,  # noqa: E402
                                   UNDETERMINED_SHARE, _np, first_moments, scaled_error)

GAMMA, V_RHO, V_C, LAMBDA = 0.99, 1.0, 0.9, 0.95


# ------------------------------------------------------------------------------------------------------------------------
# one case of the launch: host arrays (float32 / bool / int32) and their device tensors
# ------------------------------------------------------------------------------------------------------------------------
def make_case(B, n, sizes, O, E, Es, use_is, seed, beta=None):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    D = sum(sizes)
    b = rng.random((B, n)).astype(np.float32)       # spread over (0, 1) with exact zeros and ones
    b.reshape(-1)[::5] = 0.
    b.reshape(-1)[2::7] = 1.
    if beta is not None:
        b[:] = beta
    action = np.concatenate([np.eye(s, dtype=np.float32)[rng.integers(0, s, (B, n))] for s in sizes], -1)
    c = dict(B=B, n=n, sizes=tuple(sizes), K=len(sizes), D=D, O=O, E=E, Es=Es, use_is=use_is,
             logits=f(B, n + 1, D) * 2, q_target=f(E, B, n + 1, D), q_online=f(E, B, D), beta=b, v_opt=f(B, n, O),
             action=action, mu=(rng.random((B, n, D)) * 0.95 + 0.05).astype(np.float32), reward=f(B, n),
             done=rng.random((B, n)) < 0.3, last=rng.random((B, n)) < 0.15, pad=rng.random((B, n)) < 0.2,
             sub_n=rng.permutation(E)[:Es].astype(np.int32), sub_next=rng.permutation(E)[:Es].astype(np.int32),
             log_alpha=np.float32(rng.uniform(-3, 0)),
             gamma_ratio=(GAMMA ** np.arange(n)).astype(np.float32), lambda_ratio=(LAMBDA ** np.arange(n)).astype(np.float32))
    if B > 2:
        c['action'][2, 0] = 0.      # a stored action of zeros: every mu * a is 0 -> 1, the first entry is the maximum
    return c


def _gapped(t):
    """the same values as a view of a wider buffer: NaN in front of and behind every row of the last dimension"""
    big = torch.full((*t.shape[:-1], t.shape[-1] + 5), float('nan'), device=t.device)
    big[..., 3:3 + t.shape[-1]] = t
    return big[..., 3:3 + t.shape[-1]]


def to_device(c, strided=False):
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d = {k: cu(v) if isinstance(v, np.ndarray) and v.ndim > 0 else v for k, v in c.items()}
    d['log_alpha'] = torch.tensor([float(c['log_alpha'])], device='cuda')
    d['q_target'], d['q_online'] = list(d['q_target'].unbind(0)), list(d['q_online'].unbind(0))
    if strided:     # beta a column block of a wider buffer, the options' values transposed and padded, logits gapped rows
        d['beta'], d['logits'] = _gapped(d['beta']), _gapped(d['logits'])
        O, B, n = c['O'], c['B'], c['n']
        vt = torch.full((O + 2, B, n), float('nan'), device='cuda')
        vt[1:O + 1] = d['v_opt'].permute(2, 0, 1)
        d['v_opt'] = vt[1:O + 1].permute(1, 2, 0)
        assert not d['logits'].is_contiguous() and (B * n == 1 or O == 1 or not d['v_opt'].is_contiguous())
    return d


def vtrace_args(d, y, td=None):
    from asac_amd import native
    a = native.VtraceArgs()
    n = d['n']
    a.reward, a.reward_stride = d['reward'].data_ptr(), n
    a.done, a.last_mask, a.padding_mask, a.mask_stride = d['done'].data_ptr(), d['last'].data_ptr(), d['pad'].data_ptr(), n
    a.gamma_ratio, a.lambda_ratio = d['gamma_ratio'].data_ptr(), d['lambda_ratio'].data_ptr()
    a.gamma, a.v_rho, a.v_c = GAMMA, V_RHO, V_C
    a.use_n_step_is, a.B, a.n = int(d['use_is']), d['B'], n
    a.subset_n, a.subset_next, a.E_sample = d['sub_n'].data_ptr(), d['sub_next'].data_ptr(), d['Es']
    a.log_alpha = d['log_alpha'].data_ptr()
    if d['use_is']:
        a.mu_prob, a.mu_stride_b, a.mu_stride_t = d['mu'].data_ptr(), d['mu'].stride(0), d['mu'].stride(1)
    a.y_out = y.data_ptr()
    if td is not None:
        a.td_error_out = td.data_ptr()
    return a


def launch(d, with_td=True):
    """-> (y, td) of `asac_option_discrete_return`, outputs pre-filled with NaN"""
    from asac_amd import native
    y, td = torch.full((d['B'],), float('nan'), device='cuda'), torch.full((d['B'],), float('nan'), device='cuda')
    native.option_discrete_return(vtrace_args(d, y, td if with_td else None), native.branches(d['sizes']), d['q_target'],
                                  d['logits'], d['beta'], d['v_opt'], action=d['action'],
                                  q_online=d['q_online'] if with_td else None)
    return y, td


# ------------------------------------------------------------------------------------------------------------------------
# float64 arbiter (NumPy) and the float32 composition (torch on the device) of the same lines
# ------------------------------------------------------------------------------------------------------------------------
def ref64(c):
    """-> (y [B], td [B], scale_y [B], scale_td [B]): the issue's formulas in float64, and per row the size of what the
    row sums (before any cancellation)"""
    f8 = lambda k: c[k].astype(np.float64)  # noqa: E731
    sizes, K, n = c['sizes'], c['K'], c['n']
    z, q, beta, reward = f8('logits'), f8('q_target'), f8('beta'), f8('reward')
    alpha = np.exp(np.float64(c['log_alpha']))
    p, lp = np.empty_like(z), np.empty_like(z)
    j0 = 0
    for s in sizes:
        zz = z[..., j0:j0 + s]
        m = zz.max(-1, keepdims=True)
        lse = np.log(np.exp(zz - m).sum(-1, keepdims=True)) + m
        lp[..., j0:j0 + s] = zz - lse
        p[..., j0:j0 + s] = np.exp(zz - lse)
        j0 += s
    cl = alpha * np.log(np.maximum(p, 1e-8))
    qn, qx = q[c['sub_n'].astype(np.int64)].min(0), q[c['sub_next'].astype(np.int64)].min(0)
    vbar, vbar_mag = f8('v_opt').mean(-1), np.abs(f8('v_opt')).mean(-1)
    bb = beta[..., None]
    vn = (p[:, :-1] * (qn[:, :-1] - cl[:, :-1])).sum(-1) / K
    vx = (p[:, 1:] * ((1 - bb) * (qx[:, 1:] - cl[:, 1:]) + bb * vbar[..., None])).sum(-1) / K
    vn_mag = (p[:, :-1] * (np.abs(qn[:, :-1]) + np.abs(cl[:, :-1]))).sum(-1) / K
    vx_mag = (p[:, 1:] * (np.abs(1 - bb) * (np.abs(qx[:, 1:]) + np.abs(cl[:, 1:])) + bb * vbar_mag[..., None])).sum(-1) / K
    keep = ~(c['last'] | c['pad'])
    g = GAMMA * ~c['done']
    td = f8('gamma_ratio') * (reward + g * vx - vn)
    mag = f8('gamma_ratio') * (np.abs(reward) + g * vx_mag + vn_mag)
    if c['use_is']:
        a = f8('action')
        mu = f8('mu') * a
        mu = np.where(mu == 0., 1., mu).prod(-1)
        lpa = np.zeros(a.shape[:2])
        j0 = 0
        for s in sizes:
            arg = a[..., j0:j0 + s].argmax(-1)          # the first maximum
            lpa += np.take_along_axis(lp[:, :n, j0:j0 + s], arg[..., None], -1)[..., 0]
            j0 += s
        ratio = np.exp(lpa) / np.maximum(mu, 1e-8)
        rho, cc = np.minimum(ratio, V_RHO), np.minimum(ratio, V_C)
        cc = np.cumprod(np.concatenate([np.ones_like(cc[:, :1]), cc[:, :-1]], 1), 1)
        w = cc * rho * f8('lambda_ratio')
        td, mag = w * td, w * mag
    y = vn[:, 0] + (td * keep).sum(1)
    scale_y = vn_mag[:, 0] + (mag * keep).sum(1)
    a0, qo = f8('action')[:, 0], f8('q_online')
    qs = (a0[None] * qo).sum(-1) / K                                   # [E, B]
    err = np.abs(qs - y[None]).mean(0)
    scale_td = (np.abs(a0[None] * qo).sum(-1) / K).mean(0) + scale_y
    return y, err, np.maximum(scale_y, 1e-30), np.maximum(scale_td, 1e-30)


def composition32(d):
    """the eager branch of `OptionBase._get_y` / `_get_td_error` (float32 torch ops on the device, the scan through
    `asac_vtrace_return_direct`, as the option issues it) on contiguous tensors -> (y, td)"""
    from asac_amd import native
    K, D, B = d['K'], d['D'], d['B']
    stacked = torch.stack(d['q_target'])
    next_target = stacked[:, :, 1:].index_select(0, d['sub_next'].long())
    min_n = stacked[:, :, :-1].index_select(0, d['sub_n'].long()).min(0)[0]
    min_next = next_target.min(0)[0]
    vbar = d['v_opt'].mean(-1)
    d_policy = dr.joint_policy(d['logits'].contiguous(), d['sizes'])
    probs = d_policy.probs
    n_p, next_p = probs[:, :-1], probs[:, 1:]
    alpha = torch.exp(d['log_alpha'])
    beta = d['beta'].unsqueeze(-1)
    tmp_n = min_n - alpha * torch.log(n_p.clamp(min=1e-8))
    tmp_next = (1 - beta) * (min_next - alpha * torch.log(next_p.clamp(min=1e-8))) + beta * vbar.unsqueeze(-1)
    v_n = torch.sum(n_p * tmp_n, dim=-1) / K
    v_next = torch.sum(next_p * tmp_next, dim=-1) / K
    pi = mu = None
    if d['use_is']:
        nx_actions = torch.cat([d['action'], torch.zeros_like(d['action'][:, :1])], dim=1)
        mu = d['mu'][..., :D] * nx_actions[:, :-1, :D]
        mu = torch.where(mu == 0., torch.ones_like(mu), mu).prod(-1).contiguous()
        pi = torch.exp(d_policy.log_prob(nx_actions[..., :D]).sum(-1))[:, :-1].contiguous()
    y = torch.empty(B, device='cuda')
    native.vtrace_return_direct(vtrace_args(d, y), v_n.contiguous(), v_next.contiguous(), pi, mu)
    a0 = d['action'][:, 0]
    qs = torch.stack([torch.sum(a0 * q, dim=-1) / K for q in d['q_online']])
    return y, torch.abs(qs - y.unsqueeze(0)).mean(0)


BS, NS, OS = (1, 33, 256), (1, 4, 64), (1, 3, 16)
SIZES = ((2,), (3, 2), (64,), (1,) * 8, (5, 7, 9, 11))
ENSEMBLES = ((1, 1), (3, 2), (8, 8))


def return_cases():
    """every (B, n, branch sizes) with and without importance sampling; the options, the ensemble and the layout cycle
    through their values along the list, out of step with each other (every value of every axis occurs, every (n, IS)
    family holds every B and every branch table)"""
    out = []
    for i, (B, n, sizes) in enumerate(itertools.product(BS, NS, SIZES)):
        for use_is in (True, False):
            k = i + int(use_is)
            out.append((B, n, sizes, OS[k % 3], *ENSEMBLES[(k // 3 + i // 5) % 3], use_is, bool((k + i // 15) % 2)))
    return out


def test_the_list_of_cases_covers_every_axis():
    cases = return_cases()
    for axis, values in enumerate((BS, NS, SIZES, OS)):
        assert {c[axis] for c in cases} == set(values)
    assert {(c[4], c[5]) for c in cases} == set(ENSEMBLES)
    assert {c[6] for c in cases} == {True, False} and {c[7] for c in cases} == {True, False}


def test_option_discrete_return_against_float64():
    """one launch per case on contiguous or strided views (NaN in the gaps), outputs pre-filled with NaN; the TD error
    rides along"""
    import asac_amd  # noqa: F401
    errors = {}     # (n, IS) -> [(case, kernel y, composition y, kernel td, composition td)]
    for i, (B, n, sizes, O, E, Es, use_is, strided) in enumerate(return_cases()):
        c = make_case(B, n, sizes, O, E, Es, use_is, seed=1900 + i)
        want_y, want_td, scale_y, scale_td = ref64(c)
        y, td = launch(to_device(c, strided=strided))
        comp_y, comp_td = composition32(to_device(c))
        assert torch.isfinite(y).all() and torch.isfinite(td).all(), 'an element was not written'
        rel = lambda got, want, scale: float((np.abs(_np(got) - want) / scale).max())  # noqa: E731
        errors.setdefault((n, use_is), []).append(
            ((B, n, sizes, O, E, Es, use_is, strided), rel(y, want_y, scale_y), rel(comp_y, want_y, scale_y),
             rel(td, want_td, scale_td), rel(comp_td, want_td, scale_td)))
    for family, rows in sorted(errors.items()):
        pooled_y, pooled_td = max(r[2] for r in rows), max(r[4] for r in rows)
        worst = max(rows, key=lambda r: r[1])
        print(f'option_discrete_return n={family[0]} IS={family[1]}: composition y {pooled_y:.3e} td {pooled_td:.3e}; '
              f'kernel at worst y {worst[1]:.3e} {worst[0]}, td {max(r[3] for r in rows):.3e}')
        for tag, e_y, _, e_td, _ in rows:
            assert e_y <= 4. * pooled_y, (tag, e_y, pooled_y)
            assert e_td <= 4. * pooled_td, (tag, e_td, pooled_td)


@pytest.mark.parametrize('use_is', [True, False], ids=['is', 'plain'])
@pytest.mark.parametrize('B,n,sizes', [(1, 1, (2,)), (33, 4, (3, 2)), (256, 64, (64,))])
def test_zero_beta_and_one_sampled_member_give_the_plain_return_s_bits(B, n, sizes, use_is):
    """the minimum and the mean of one member are the same number, and (1 - 0) * x + 0 * vbar is x"""
    from asac_amd import native
    d = to_device(make_case(B, n, sizes, 3, 2, 1, use_is, seed=B + n, beta=0.))
    y0, td0 = torch.full((B,), float('nan'), device='cuda'), torch.full((B,), float('nan'), device='cuda')
    native.discrete_return(vtrace_args(d, y0, td0), native.branches(sizes), d['q_target'], d['logits'], action=d['action'],
                           q_online=d['q_online'])
    y1, td1 = launch(d)
    assert torch.isfinite(y0).all() and torch.isfinite(td0).all()
    assert torch.equal(y0, y1) and torch.equal(td0, td1)


@pytest.mark.parametrize('use_is', [True, False], ids=['is', 'plain'])
def test_a_step_s_beta_and_option_values_pair_with_the_next_position(use_is):
    """beta and vbar of step t act on position t + 1: an off-by-one shows as a dependence that must not exist"""
    B, n, sizes, O = 33, 4, (3, 2), 3
    base = make_case(B, n, sizes, O, 2, 2, use_is, seed=77)
    base['done'][:], base['last'][:], base['pad'][:] = False, False, False

    def y_of(beta_last, **change):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        c['beta'][:, n - 1] = beta_last
        for k, fn in change.items():
            fn(c[k])
        return launch(to_device(c), with_td=False)[0]

    def other_q(q):
        q[:, :, n, :] += 3.

    def other_v(v):
        v[:, n - 1, :] -= 2.
    assert torch.equal(y_of(1.), y_of(1., q_target=other_q))        # beta = 1 hides the last position's critics
    assert torch.equal(y_of(0.), y_of(0., v_opt=other_v))           # beta = 0 hides the last step's option values
    # ... which beta = 1 shows (no step is masked: in every row, unless a row's importance weights round the change away)
    some = torch.any if use_is else torch.all
    assert some(y_of(1.) != y_of(1., v_opt=other_v))
    assert some(y_of(0.) != y_of(0., q_target=other_q))


def test_entry_point_refuses_bad_arguments():
    """every rejection of include/asac_hip.h: hipErrorInvalidValue, no launch, the marker-filled outputs untouched;
    B == 0 is accepted and launches nothing; the good call then runs"""
    from asac_amd import native
    B, n, sizes, O, E = 8, 3, (3, 2), 3, 2
    d = to_device(make_case(B, n, sizes, O, E, E, True, seed=5))
    D = d['D']
    lib, s, bad, p = native.load(), native._stream(), 1, native._p      # 1: hipErrorInvalidValue
    y, td = torch.full((B,), 7., device='cuda'), torch.full((B,), 7., device='cuda')

    def args(**change):
        a = vtrace_args(d, y, td)
        for k, v in change.items():
            setattr(a, k, v)
        return a

    def job(sizes_=sizes, q_online=d['q_online'], action=d['action']):
        j = native.DiscreteReturn()
        j.branches = native.branches(sizes_)
        j.q_target, j.q_online = native.members(d['q_target'], D), native.members(list(q_online), D)
        j.logits, j.logits_stride_b, j.logits_stride_t = d['logits'].data_ptr(), (n + 1) * D, D
        if action is not None:
            j.action, j.action_stride_b, j.action_stride_t = action.data_ptr(), n * D, D
        return j

    def call(a, j, beta=d['beta'], v=d['v_opt'], O_=O):
        return lib.asac_option_discrete_return(C.byref(a), C.byref(j), p(beta), n, 1, p(v), n * O, O, 1, O_, s)
    uneven = job()
    uneven.branches.size[1] = 3                                         # 3 + 3 != D
    refused = [call(args(), job(), beta=None), call(args(), job(), v=None), call(args(), job(), O_=0),
               call(args(), job(), O_=-2), call(args(), job(), O_=native.OPTION_MAX_OPTIONS + 1), call(args(), uneven),
               call(args(E_sample=E + 1), job()), call(args(mu_prob=None), job()), call(args(), job(action=None)),
               call(args(), job(q_online=[])), call(args(use_n_step_is=0), job(action=None)),
               call(args(n=65), job()), call(args(y_out=None), job()), call(args(B=-1), job())]
    assert refused == [bad] * len(refused), refused
    assert call(args(B=0), job()) == 0
    torch.cuda.synchronize()
    assert (y == 7.).all() and (td == 7.).all()                         # nothing was launched
    with pytest.raises(native.AsacNativeError):
        native.option_discrete_return(args(), native.branches(sizes), d['q_target'], d['logits'], None, None,
                                      action=d['action'], q_online=d['q_online'])
    assert call(args(), job()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and not (y == 7.).any() and not (td == 7.).any()


# ------------------------------------------------------------------------------------------------------------------------
# the class against the reference's fixtures
# ------------------------------------------------------------------------------------------------------------------------
IS = dict(gamma=GAMMA, v_lambda=LAMBDA, v_rho=V_RHO, v_c=V_C)
F19 = {     # case -> (learner keywords, discrete action sizes)
    'pd32': (dict(n_step=3, ensemble_q_num=3, ensemble_q_sample=2, use_n_step_is=True, **IS), (3, 2)),
    'pd4_n1': (dict(n_step=1, use_n_step_is=False), (4,)),
}


def make_option(d_sizes, c_size=0, fused=True, batch_size=16, plugin='nn_oc_small', **kw):
    import asac_amd  # noqa: F401
    from algorithm.oc import OptionBase
    return OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], list(d_sizes), c_size, None, pu.plugin(plugin),
                      device='cuda:0', batch_size=batch_size, summary_path=None,
                      hip_config={'fused_option_discrete': fused}, **kw)


class TablePolicy(torch.nn.Module):
    """a policy that returns one OneHotCategorical per branch over recorded logits, whatever the state"""

    def __init__(self, logits, sizes):
        super().__init__()
        self.table, self.sizes = logits, sizes

    def forward(self, state, obs_list):
        return dr.joint_policy(self.table, self.sizes), None


def test_get_y_against_the_reference_s_tables(golden_dir):
    """`OptionBase._get_y` with policy and target critics replaced by the fixture's tables, the recorded draws replayed:
    switch on against the reference's `d_y`, bounded by 4x what the eager branch (switch off) shows in this run over the
    fixture's cases, not below one float32 rounding at the observable's largest magnitude"""
    from algorithm.fused import RecordedNoise
    from asac_amd import native
    g = np.load(golden_dir / 'f19_option_discrete_get_y.npz')
    errors = {}
    for tag in ('n4_s32', 'n3_s253_e4s2', 'n40_s4', 'n1_s32_nois'):
        n, E, Es, use_is = (int(x) for x in g[f'{tag}_cfg'])
        sizes = tuple(int(x) for x in g[f'{tag}_sizes'])
        gamma, lam, v_rho, v_c = (float(x) for x in g[f'{tag}_params'])
        cu = lambda k: torch.from_numpy(np.ascontiguousarray(g[f'{tag}_{k}'])).cuda()  # noqa: E731
        B = cu('logits').shape[0]
        opt = make_option(sizes, batch_size=B, n_step=n, ensemble_q_num=E, ensemble_q_sample=Es,
                          use_n_step_is=bool(use_is), gamma=gamma, v_lambda=lam, v_rho=v_rho, v_c=v_c)
        opt.model_policy = TablePolicy(cu('logits'), sizes)
        opt.model_target_q_list = [(lambda s, a, o, t=t: (t, None)) for t in cu('q').unbind(0)]
        with torch.no_grad():
            opt.log_d_alpha.fill_(float(g[f'{tag}_log_alpha'].reshape(-1)[0]))
        states = torch.zeros((B, n + 1, 6), device='cuda')
        for fused in (True, False):
            opt._fused_option_discrete = fused
            opt.noise = RecordedNoise(perm=list(g[f'{tag}_perm']))
            with native.LaunchProfiler(repeat=1) as prof:
                d_y, c_y = opt._get_y(cu('next_n_vs_over_options'), cu('n_terminations'), cu('n_last_masks'),
                                      cu('n_padding_masks'), [states], states, cu('n_actions'), cu('n_rewards'),
                                      cu('n_dones'), cu('n_mu_probs') if use_is else None)
            assert c_y is None and d_y.shape == (B, 1) and opt.noise.exhausted()
            assert ('asac_option_discrete_return' in prof.summary()) == fused      # the run that claims the launch took it
            assert ('asac_vtrace_return_direct' in prof.summary()) == (not fused)
            errors[tag, fused] = scaled_error(d_y, g[f'{tag}_y'])
        opt.close()
    pooled = max(e for (_, fused), e in errors.items() if not fused)
    print('get_y against the reference:', {f'{t}/{"on" if f else "off"}': f'{e:.3e}' for (t, f), e in errors.items()})
    for (tag, fused), err in errors.items():
        if fused:
            assert err <= max(4. * pooled, EPS32), (tag, err, pooled)


def _updates(case, g, mods, prefix, g0_prefix='g0', lr=3e-4):
    """{observable: scaled error} of the weights under `prefix`, compared as updates (weight - w0) in EVERY entry; entries
    whose recorded first moment does not determine the sign of the Adam step (tests/test_option_gpu.py `check_weights`)
    may differ by up to two steps and are taken out of the figure"""
    out = {}
    for name, mod in mods.items():
        oname = OPTIMIZER_OF.get(name, name.replace('model_', 'optimizer_'))
        param_index = {k: j for j, (k, _) in enumerate(mod.named_parameters())}
        for k, v in mod.state_dict().items():
            key = f'{prefix}/{name}/{k}'
            if key not in g.files:
                continue
            base = g[f'w0/{name}/{k}'].astype(np.float64)
            got, want = _np(v) - base, g[key].astype(np.float64) - base
            gkey = f'{g0_prefix}/{oname}/{param_index.get(k, -1)}'
            if gkey in g.files:
                g0 = np.abs(g[gkey].astype(np.float64))
                loose = (g0 > 0) & (g0 < max(UNDETERMINED_SHARE * float(g0.max(initial=0.)), UNDETERMINED_ABS))
                assert loose.sum() <= max(2, UNDETERMINED_MAX_SHARE * loose.size), (key, int(loose.sum()), loose.size)
                assert (np.abs(got[loose] - want[loose]) <= 2 * lr * (1 + 1e-3)).all(), key
                got = np.where(loose, want, got)
            obs = f'{prefix}/{name}'
            out[obs] = max(out.get(obs, 0.), scaled_error(got, want))
    return out


def run_sequence(case, golden_dir, fused):
    """the call order of tests/test_option_gpu.py `run_sequence` on a pure-discrete option -> (option, {observable:
    scaled error against the fixture}, the policy's and the termination head's weights afterwards)"""
    from algorithm.fused import RecordedNoise
    g = np.load(golden_dir / f'f19_option_discrete_{case}.npz')
    kw, d_sizes = F19[case]
    opt = make_option(d_sizes, fused=fused, **kw)
    mods = pu.load_golden_weights(opt, g)
    assert int(g['n_eps']) == 0
    opt.noise = RecordedNoise(perm=[g[f'perm/{i}'] for i in range(int(g['n_perm']))])
    t = {k[3:]: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in g.files if k.startswith('in/') and g[k].ndim > 0}
    priority_is = t['priority_is'] if bool(g['in/with_priority_is']) else None
    B, n = t['n_rewards'].shape
    nx_obses_list = [t['nx_obs']]
    nx_actions = torch.cat([t['n_actions'], torch.zeros_like(t['n_actions'][:, :1])], dim=1)
    nx_pre_actions = torch.cat([torch.zeros_like(nx_actions[:, :1]), nx_actions[:, :-1]], dim=1)
    nx_indexes = torch.arange(n + 1, dtype=torch.int32, device='cuda').repeat(B, 1)
    nx_pad = torch.cat([t['n_padding_masks'], t['n_padding_masks'][:, -1:]], dim=1)
    states = lambda tgt: opt.get_l_states(nx_indexes, nx_pad, nx_obses_list, nx_pre_actions,  # noqa: E731
                                          t['nx_pre_seq_hidden_states'], is_target=tgt)[0]
    with torch.no_grad():
        nx_target_states = states(True)
    nx_states = states(False)
    err = {}

    d_y, c_y = opt.compute_rep_q_grads(
        t['next_n_vs_over_options'], nx_indexes[:, :-1], t['n_last_masks'], t['n_padding_masks'], nx_obses_list,
        nx_obses_list, nx_states, nx_target_states, t['n_actions'], nx_pre_actions[:, :-1], t['n_rewards'].clone(),
        t['n_dones'], t['n_mu_probs'].clone(), t['nx_pre_seq_hidden_states'][:, :-1], priority_is=priority_is)
    assert c_y is None
    err['d_y'] = scaled_error(d_y, g['d_y'])
    opt.train_rep_q()

    def moments(names):
        fm = first_moments(opt)
        for oname in names:
            for j, view in enumerate(fm.get(oname, [])):
                key = f'g0/{oname}/{j}'
                if key in g.files and np.abs(g[key]).max() > 0:
                    err[f'g0/{oname}'] = max(err.get(f'g0/{oname}', 0.), scaled_error(view, g[key]))
                elif key in g.files:
                    assert float(view.abs().max()) == 0., key
    moments(['optimizer_rep'] + [f'optimizer_q_{i}' for i in range(opt.ensemble_q_num)])
    err.update(_updates(case, g, mods, 'w_rq'))
    assert any(k.startswith('w_rq/model_q_') for k in err) and any(k.startswith('g0/optimizer_q_') for k in err)

    nx_states_d = nx_states.detach()
    opt.train_policy_alpha(t['n_padding_masks'], [t['nx_obs'][:, :-1]], nx_states_d, t['n_actions'], t['n_mu_probs'].clone())
    moments(['optimizer_policy'])
    err.update(_updates(case, g, mods, 'w_pi'))
    opt.compute_termination_grads(float(g['in/terminal_entropy']), [t['nx_obs'][:, 0]], nx_states_d[:, 0], d_y.detach(),
                                  t['v_over_options'], t['done'], priority_is)
    opt.train_termination()
    err['loss_termination'] = scaled_error(opt._loss_termination[0], g['loss_termination'])
    moments(['optimizer_termination'])
    err.update(_updates(case, g, mods, 'w_term'))
    assert 'w_pi/model_policy' in err and 'w_term/model_termination' in err

    td = opt._get_td_error(t['next_n_vs_over_options'], t['n_last_masks'], t['n_padding_masks'], nx_obses_list,
                           nx_obses_list, nx_states_d[:, 0], nx_target_states, t['n_actions'], t['n_rewards'].clone(),
                           t['n_dones'], t['n_mu_probs'].clone())
    err['td_error'] = scaled_error(td, g['td_error'])
    assert opt.noise.exhausted()
    opt._update_target_variables(float(g['in/tau']))
    err.update(_updates(case, g, mods, 'w_tgt'))
    return opt, err


@pytest.mark.parametrize('case', list(F19))
def test_sequence_against_the_reference_fixture(case, golden_dir):
    """one full call sequence from the recorded weights, switch on and switch off (today's code): every observable of the
    fused run is within 4x the eager run's error against the fixture, not below one float32 rounding.  The policy,
    temperature and termination steps are the same code in both runs; their weights are held to the same bound."""
    from asac_amd import native
    with native.LaunchProfiler(repeat=1) as prof:
        on, err_on = run_sequence(case, golden_dir, True)
    seen = {k: v['calls'] for k, v in prof.summary().items()}
    assert seen.get('asac_option_discrete_return') == 2 and seen.get('asac_discrete_q_loss_grad') == 1, seen
    off, err_off = run_sequence(case, golden_dir, False)
    assert on._fused_option_discrete and not off._fused_option_discrete and not on._fused_discrete
    assert set(err_on) == set(err_off)
    for key in sorted(err_on):
        print(f'{case} {key}: on {err_on[key]:.3e} off {err_off[key]:.3e}')
    held = ('d_y', 'td_error', 'g0/optimizer_rep', 'g0/optimizer_q_', 'w_rq/', 'w_pi/', 'w_term/')
    bad = {k: (err_on[k], err_off[k]) for k in err_on if k.startswith(held) and err_on[k] > max(4. * err_off[k], EPS32)}
    assert not bad, bad
    on.close(), off.close()


# ------------------------------------------------------------------------------------------------------------------------
def _random_call_args(opt, B, n, d_sizes, c_size, O=3, seed=3):
    """seeded tensors for `compute_rep_q_grads` / `_get_td_error` on the plugin's pass-through representation"""
    rng = np.random.default_rng(seed)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    parts = [np.eye(s, dtype=np.float32)[rng.integers(0, s, (B, n))] for s in d_sizes]
    if c_size:
        parts.append(rng.uniform(-0.9, 0.9, (B, n, c_size)).astype(np.float32))
    A = sum(d_sizes) + c_size
    last, pad = rng.random((B, n)) < 0.15, rng.random((B, n)) < 0.2
    last[:, 0] = pad[:, 0] = False
    return dict(v=cu(rng.standard_normal((B, n, O)).astype(np.float32)), last=cu(last), pad=cu(pad),
                nx=cu(rng.standard_normal((B, n + 1, 6)).astype(np.float32)), actions=cu(np.concatenate(parts, -1)),
                rewards=cu(rng.standard_normal((B, n)).astype(np.float32)), dones=cu(rng.random((B, n)) < 0.3),
                mu=cu((rng.random((B, n, A)) * 0.9 + 0.1).astype(np.float32)))


def _rep_q(opt, a):
    return opt.compute_rep_q_grads(a['v'], None, a['last'], a['pad'], [a['nx']], [a['nx']], a['nx'], a['nx'], a['actions'],
                                   None, a['rewards'].clone(), a['dones'], a['mu'].clone(), None)


def _td(opt, a):
    return opt._get_td_error(a['v'], a['last'], a['pad'], [a['nx']], [a['nx']], a['nx'][:, 0], a['nx'], a['actions'],
                             a['rewards'].clone(), a['dones'], a['mu'].clone())


OURS = ('asac_option_discrete_', 'asac_discrete_')
VARIANTS = {    # name -> (discrete sizes, continuous size, switch, learner keywords, the launches expected per call)
    'on': ((3, 2), 0, True, dict(), True),
    'off': ((3, 2), 0, False, dict(), False),
    'hybrid': ((3, 2), 2, True, dict(), False),
    'dqn': ((3, 2), 0, True, dict(discrete_dqn_like=True), False),
    'nine_members': ((3, 2), 0, True, dict(ensemble_q_num=9), False),
}


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_launch_accounting(variant):
    """switch on, a (3, 2) option: `compute_rep_q_grads` is one `asac_option_discrete_return` and one
    `asac_discrete_q_loss_grad`, `_get_td_error` one `asac_option_discrete_return`, no `asac_vtrace_return_direct`; with the
    switch off, a hybrid or DQN-like option or nine critics none of them appears and the calls still train the critics;
    `train_policy_alpha` issues none of them either way"""
    from asac_amd import native
    d_sizes, c_size, fused, kw, expect = VARIANTS[variant]
    B, n = 16, 3
    torch.manual_seed(0)
    opt = make_option(d_sizes, c_size, fused, n_step=n, **kw)
    a = _random_call_args(opt, B, n, d_sizes, c_size)
    ours = lambda prof: {k: v['calls'] for k, v in prof.summary().items() if k.startswith(OURS)}  # noqa: E731
    q0 = slice(*opt._params.segments['q_0'])
    before = opt._params.flat[q0].clone()
    with native.LaunchProfiler(repeat=1) as prof:
        d_y, _ = _rep_q(opt, a)
    assert ours(prof) == ({'asac_option_discrete_return': 1, 'asac_discrete_q_loss_grad': 1} if expect else {})
    assert ('asac_vtrace_return_direct' in prof.summary()) == (not expect and not kw.get('discrete_dqn_like', False))
    opt.train_rep_q()
    assert torch.isfinite(opt._params.flat).all() and not torch.equal(before, opt._params.flat[q0])
    with native.LaunchProfiler(repeat=1) as prof:
        td = _td(opt, a)
    assert ours(prof) == ({'asac_option_discrete_return': 1} if expect else {})
    assert ('asac_vtrace_return_direct' in prof.summary()) == (not expect and not kw.get('discrete_dqn_like', False))
    assert td.shape == (B, 1) and torch.isfinite(td).all() and torch.isfinite(d_y).all()
    with native.LaunchProfiler(repeat=1) as prof:
        opt.train_policy_alpha(a['pad'], [a['nx'][:, :-1]], a['nx'], a['actions'], a['mu'].clone())
    assert not ours(prof)
    opt.close()


def test_d_y_is_a_fresh_tensor_per_call():
    """the selector keeps the returned y for the termination step: a second call must not write into it"""
    B, n = 16, 3
    torch.manual_seed(0)
    opt = make_option((3, 2), n_step=n)
    a = _random_call_args(opt, B, n, (3, 2), 0)
    beta = torch.rand(B, n, device='cuda')

    def get_y(rewards):
        return opt._get_y(a['v'], beta, a['last'], a['pad'], [a['nx']], a['nx'], a['actions'], rewards, a['dones'],
                          a['mu'] if opt.use_n_step_is else None)[0]
    first = get_y(a['rewards'])
    kept = first.clone()
    second = get_y(a['rewards'] + 1.)
    assert first.data_ptr() != second.data_ptr()
    assert first.untyped_storage().data_ptr() != second.untyped_storage().data_ptr()
    assert torch.equal(first, kept) and not torch.equal(first, second)
    opt.close()
