"""GPU: the option-critic's per-option learner (`algorithm/oc/option_base.OptionBase`, csrc/option.hip).

  * `asac_option_return` and `asac_termination_loss_grad` alone against float64 NumPy restatements of the reference lines
    written here; the bound of each comparison is 4x the error the PyTorch-ROCm float32 composition of the same lines shows
    against float64 on the same inputs (measured in the test), the composition's error taken over the family of cases that
    share the arithmetic (same n and IS for the return, same weighting and done pattern for the termination loss): a
    one-row case is held to what the composition shows on the family's large cases, there is no floor.  The factor 4 is the project's margin for reduction-order differences.
  * `asac_option_return` with beta == 0: the bits of `asac_vtrace_return_min`; its TD error: mean_e |q_e - y| of its own y
  * `asac_option_return` against the reference's own numbers (`f15_option_get_y.npz`, recorded draws replayed)
  * every reference fixture `f15_option_<case>.npz`: one full call sequence from the recorded weights; each observable is
    bounded by 4x the error recorded on an MI355X in `tests/option_tolerances.json` (a missing key fails;
    `ASAC_OPTION_RECORD=<file.json>` records the observed errors into that file under a loose sanity bound instead)
  * `fix_policy` leaves representation and policy bit-equal, checkpoints round-trip, a reference-layout `.pth` loads,
    bad arguments are refused without a launch"""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_utils as pu  # noqa: E402

HERE = Path(__file__).resolve().parent
EPS32 = float(np.finfo(np.float32).eps)
RECORD = os.environ.get('ASAC_OPTION_RECORD')       # path of the JSON file to record into, or unset
_TOL_PATH = HERE / 'option_tolerances.json'
MEASURED = json.loads(_TOL_PATH.read_text()) if _TOL_PATH.exists() else {}
RECORDED = {}
SANITY = 5e-3       # while recording: nothing may be further off than this (relative to the observable's largest value)


def _np(x):
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def scaled_error(got, want) -> float:
    """max |got - want| over the observable's largest magnitude"""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max(initial=0.) / max(float(np.abs(want).max(initial=0.)), 1e-30))


def ocheck(key, got, want):
    """fixture comparison: 4x the error recorded on an MI355X (not below one float32 rounding), a missing key fails"""
    err = scaled_error(got, want)
    print(f'option parity {key}: {err:.3e}')
    if RECORD:
        RECORDED[key] = max(RECORDED.get(key, 0.), err)
        out = Path(RECORD)
        out.parent.mkdir(parents=True, exist_ok=True)
        old = json.loads(out.read_text()) if out.exists() else {}
        old.update(RECORDED)
        out.write_text(json.dumps(old, indent=1, sort_keys=True))
        assert err <= SANITY, (key, err)
        return
    assert key in MEASURED, f'{key!r} has no entry in tests/option_tolerances.json (ASAC_OPTION_RECORD=<file.json> records it)'
    assert err <= max(4. * MEASURED[key], EPS32), (key, err, MEASURED[key])


# ------------------------------------------------------------------------------------------------------------------------
# float64 restatements (reference option_base.py:287, 376-427, sac_base.py:1244-1295, operators.py:27-31)
# ------------------------------------------------------------------------------------------------------------------------
def ref_option_return(xp, q, sub_n, sub_next, logp, alpha, beta, v_opt, reward, done, last, pad, pi, mu, gamma_ratio,
                      lambda_ratio, gamma, v_rho, v_c, use_is, scale_out=None):
    """`xp`: numpy (float64 arbiter) or torch (float32 composition on the device); q [E, B, n+1], logp [B, n+1],
    beta [B, n], v_opt [B, n, O], pi / mu per-dimension probabilities [B, n, A]"""
    mn = (lambda x: x.min(0)) if xp is np else (lambda x: x.min(0)[0])
    min_n, min_next = mn(q[sub_n][:, :, :-1]), mn(q[sub_next][:, :, 1:])
    vbar = v_opt.mean(-1)
    n_vs = min_n - alpha * logp[:, :-1]
    next_n_vs = (1 - beta) * (min_next - alpha * logp[:, 1:]) + beta * vbar
    td = reward + gamma * ~done * next_n_vs - n_vs
    if scale_out is not None:       # the size of what a step adds up, before any cancellation
        ab = np.abs
        n_mag = ab(min_n) + alpha * ab(logp[:, :-1])
        next_mag = ab(1 - beta) * (ab(min_next) + alpha * ab(logp[:, 1:])) + ab(beta) * ab(v_opt).mean(-1)
        mag = ab(reward) + gamma * ~done * next_mag + n_mag
        mag = gamma_ratio * mag
    td = gamma_ratio * td
    if use_is:
        td = lambda_ratio * td
        ratio = pi.prod(-1) / (xp.clip(mu.prod(-1), 1e-8, None) if xp is np else mu.prod(-1).clamp(min=1e-8))
        rho = xp.minimum(ratio, xp.asarray(v_rho, dtype=ratio.dtype) if xp is np else torch.tensor(v_rho, dtype=ratio.dtype, device=ratio.device))
        c = xp.minimum(ratio, xp.asarray(v_c, dtype=ratio.dtype) if xp is np else torch.tensor(v_c, dtype=ratio.dtype, device=ratio.device))
        ones = xp.ones_like(c[:, :1])
        c = (np.concatenate if xp is np else torch.cat)([ones, c[:, :-1]], 1)
        c = np.cumprod(c, 1) if xp is np else torch.cumprod(c, 1)
        td = c * rho * td
        if scale_out is not None:
            mag = c * rho * lambda_ratio * mag
    td = td * ~(last | pad)
    if scale_out is not None:       # per row: |Q| + alpha |log pi| of V(s_0), plus every step's summands with its weight
        scale_out.append(n_mag[:, 0] + (mag * ~(last | pad)).sum(1))
    return n_vs[:, 0] + td.sum(1)


def make_return_inputs(B, n, O, E, Es, A, use_is, seed, beta_zero=False, strided=False):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    beta = rng.random((B, n)).astype(np.float32)
    beta.reshape(-1)[::5] = 0.
    beta.reshape(-1)[2::7] = 1.
    if beta_zero:
        beta[:] = 0.
    d = dict(q=f(E, B, n + 1), logp=f(B, n + 1), beta=beta, v_opt=f(B, n, O), reward=f(B, n),
             done=rng.random((B, n)) < 0.3, last=rng.random((B, n)) < 0.15, pad=rng.random((B, n)) < 0.2,
             pi=(rng.random((B, n + 1, A)) * 2).astype(np.float32), mu=(rng.random((B, n, A)) * 2 + 0.05).astype(np.float32),
             q_online=f(E, B), log_alpha=np.float32(rng.uniform(-3, 0)),
             sub_n=rng.permutation(E)[:Es].astype(np.int32), sub_next=rng.permutation(E)[:Es].astype(np.int32))
    d['gamma_ratio'] = (0.99 ** np.arange(n)).astype(np.float32)
    d['lambda_ratio'] = (0.95 ** np.arange(n)).astype(np.float32)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v for k, v in d.items()}
    if strided:     # non-contiguous views: beta a column block of a wider buffer, V a transposed / padded one
        wide = torch.full((B, n + 3), float('nan'), device='cuda')
        wide[:, 1:n + 1] = dev['beta']
        dev['beta'] = wide[:, 1:n + 1]
        vt = torch.full((O + 2, B, n), float('nan'), device='cuda')
        vt[1:O + 1] = dev['v_opt'].permute(2, 0, 1)
        dev['v_opt'] = vt[1:O + 1].permute(1, 2, 0)
        assert B == 1 or not (dev['beta'].is_contiguous() or dev['v_opt'].is_contiguous())
    return d, dev


def vtrace_args(dev, B, n, E, Es, A, use_is, y, td=None):
    from asac_amd import native
    a = native.VtraceArgs()
    q = dev['q']
    a.q, a.q_stride_e, a.q_stride_b, a.q_stride_t = q.data_ptr(), q.stride(0), q.stride(1), q.stride(2)
    if Es != E:
        a.subset_n, a.subset_next = dev['sub_n'].data_ptr(), dev['sub_next'].data_ptr()
    a.E_sample = Es
    dev['_log_alpha'] = torch.tensor([float(dev['log_alpha'])], device='cuda')
    a.logp, a.log_alpha = dev['logp'].data_ptr(), dev['_log_alpha'].data_ptr()
    a.reward, a.reward_stride = dev['reward'].data_ptr(), n
    a.done, a.last_mask, a.padding_mask, a.mask_stride = dev['done'].data_ptr(), dev['last'].data_ptr(), dev['pad'].data_ptr(), n
    if use_is:
        a.mu_prob, a.mu_stride_b, a.mu_stride_t, a.mu_offset = dev['mu'].data_ptr(), n * A, A, 0
        a.pi_prob, a.pi_stride_b, a.pi_stride_t, a.A = dev['pi'].data_ptr(), (n + 1) * A, A, A
    a.gamma_ratio, a.lambda_ratio = dev['gamma_ratio'].data_ptr(), dev['lambda_ratio'].data_ptr()
    a.gamma, a.v_rho, a.v_c, a.use_n_step_is, a.B, a.n = 0.99, 1.0, 0.9, int(use_is), B, n
    a.y_out = y.data_ptr()
    if td is not None:
        a.q_online, a.E_online, a.td_error_out = dev['q_online'].data_ptr(), E, td.data_ptr()
    return a


def subsets(d, E, Es):
    if Es == E:
        return np.arange(E), np.arange(E)
    return d['sub_n'].astype(np.int64), d['sub_next'].astype(np.int64)


RETURN_CASES = [(B, n, O, E, Es, use_is, strided)
                for B in (1, 33, 256, 4096) for n in (1, 4, 40) for O in (1, 3, 16)
                for (E, Es) in ((2, 2), (4, 2), (4, 4)) for use_is in (True, False)
                for strided in ((False, True) if (O == 3 and E == 2) else (False,))]


def test_option_return_against_float64():
    """every (B, n, O, E, subset, IS, layout) combination, one launch each; bit-equality with the plain return at beta == 0
    and the TD error of its own y ride along"""
    from asac_amd import native
    errors = {}     # (n, IS) -> [(case, the kernel's error, the composition's error)]
    for case_i, (B, n, O, E, Es, use_is, strided) in enumerate(RETURN_CASES):
        A = 2
        d, dev = make_return_inputs(B, n, O, E, Es, A, use_is, seed=1000 + case_i, strided=strided)
        y, td = torch.full((B,), float('nan'), device='cuda'), torch.full((B,), float('nan'), device='cuda')
        native.option_return(vtrace_args(dev, B, n, E, Es, A, use_is, y, td), dev['beta'], dev['v_opt'])
        sn, sx = subsets(d, E, Es)
        common = dict(gamma=0.99, v_rho=1.0, v_c=0.9, use_is=use_is)
        terms = []
        d64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in d.items()}
        want = ref_option_return(np, d64['q'], sn, sx, d64['logp'], np.exp(np.float64(d['log_alpha'])),
                                 d64['beta'], d64['v_opt'], d64['reward'], d['done'], d['last'], d['pad'],
                                 d64['pi'][:, :-1], d64['mu'], d64['gamma_ratio'], d64['lambda_ratio'], scale_out=terms,
                                 **common)
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items() if isinstance(v, np.ndarray)}
        comp = ref_option_return(torch, t['q'], torch.from_numpy(sn).cuda(), torch.from_numpy(sx).cuda(), t['logp'],
                                 torch.exp(torch.tensor(float(d['log_alpha']), device='cuda')), t['beta'], t['v_opt'],
                                 t['reward'], t['done'], t['last'], t['pad'], t['pi'][:, :-1], t['mu'], t['gamma_ratio'],
                                 t['lambda_ratio'], **common)
        # errors are measured per row against the size of what that row sums (a return whose terms cancel is small, its
        # rounding error is not)
        scale = np.maximum(terms[0], 1e-30)
        tag = (B, n, O, E, Es, use_is, strided)
        errors.setdefault((n, use_is), []).append(
            (tag, float((np.abs(_np(y) - want) / scale).max()), float((np.abs(_np(comp) - want) / scale).max())))
        # the TD error is formed from the launch's own y
        want_td = (dev['q_online'] - y.unsqueeze(0)).abs()
        want_td = sum(want_td[e] for e in range(E)) / E if E <= 4 else want_td.mean(0)
        assert torch.equal(td, want_td), tag
    # The bound of every case is 4x the composition's error over its (n, IS) family — the same arithmetic on the same kind
    # of input at every B, O and ensemble of the list: a one-row case is held to what the composition shows over the
    # family's 4 096-row cases, not to its own single error, which can be zero by chance.  No floor.
    for family, rows in sorted(errors.items()):
        pooled = max(comp for _, _, comp in rows)
        worst = max(rows, key=lambda r: r[1])
        print(f'option_return n={family[0]} IS={family[1]}: composition {pooled:.3e}, kernel at worst {worst[1]:.3e} {worst[0]}')
        for tag, err_kernel, _ in rows:
            assert err_kernel <= 4. * pooled, (tag, err_kernel, pooled)


@pytest.mark.parametrize('B,n,O,E,Es,use_is', [(1, 1, 1, 2, 2, False), (33, 4, 3, 2, 2, True), (256, 40, 16, 4, 2, True),
                                               (4096, 4, 3, 4, 4, True), (4096, 40, 3, 2, 2, False), (33, 1, 3, 4, 2, True)])
def test_option_return_with_zero_beta_has_the_plain_return_s_bits(B, n, O, E, Es, use_is):
    from asac_amd import native
    A = 2
    d, dev = make_return_inputs(B, n, O, E, Es, A, use_is, seed=B + n + O, beta_zero=True)
    y0, y1 = torch.full((B,), float('nan'), device='cuda'), torch.full((B,), float('nan'), device='cuda')
    td0, td1 = torch.zeros(B, device='cuda'), torch.zeros(B, device='cuda')
    native.vtrace_return_min(vtrace_args(dev, B, n, E, Es, A, use_is, y0, td0))
    native.option_return(vtrace_args(dev, B, n, E, Es, A, use_is, y1, td1), dev['beta'], dev['v_opt'])
    assert torch.isfinite(y0).all()
    assert torch.equal(y0, y1) and torch.equal(td0, td1)


def test_option_return_against_the_reference_s_get_y(golden_dir):
    """OptionBase._get_y of the reference with table-driven policy / critics; the recorded draws replayed"""
    from asac_amd import native
    g = np.load(golden_dir / 'f15_option_get_y.npz')
    for tag in ('n4_e2', 'n3_e4s2', 'n40_e2', 'n1_e2_nois'):
        n, E, Es, A, use_is = (int(x) for x in g[f'{tag}_cfg'])
        gamma, lam, v_rho, v_c = (float(x) for x in g[f'{tag}_params'])
        cu = lambda k: torch.from_numpy(np.ascontiguousarray(g[f'{tag}_{k}'])).cuda()  # noqa: E731
        loc, scale, eps = cu('loc'), cu('scale'), cu('eps')
        B = loc.shape[0]
        nx_actions = torch.cat([cu('n_actions'), torch.zeros((B, 1, A), device='cuda')], 1)
        a_tanh, logp = torch.empty_like(loc), torch.empty((B, n + 1), device='cuda')
        c_pi = torch.empty_like(loc)
        native.squash_sample_fwd(loc, scale, eps, a_tanh, logp, None, nx_actions, 0, c_pi, 0)
        perm = g[f'{tag}_perm']
        dev = dict(q=cu('q').squeeze(-1).contiguous(), logp=logp, reward=cu('n_rewards'), done=cu('n_dones'),
                   last=cu('n_last_masks'), pad=cu('n_padding_masks'), pi=c_pi, mu=cu('n_mu_probs'),
                   log_alpha=float(g[f'{tag}_log_alpha'].reshape(-1)[0]),
                   sub_n=torch.from_numpy(perm[0][:Es].astype(np.int32)).cuda(),
                   sub_next=torch.from_numpy(perm[1][:Es].astype(np.int32)).cuda(),
                   gamma_ratio=torch.from_numpy((gamma ** np.arange(n)).astype(np.float32)).cuda(),
                   lambda_ratio=torch.from_numpy((lam ** np.arange(n)).astype(np.float32)).cuda())
        y = torch.full((B,), float('nan'), device='cuda')
        a = vtrace_args(dev, B, n, E, Es, A, use_is, y)
        a.gamma, a.v_rho, a.v_c = gamma, v_rho, v_c
        native.option_return(a, cu('n_terminations'), cu('next_n_vs_over_options'))
        ocheck(f'get_y/{tag}', y, g[f'{tag}_y'].reshape(-1))


def test_option_return_refuses_bad_arguments():
    from asac_amd import native
    B, n, O, E, A = 8, 4, 3, 2, 2
    d, dev = make_return_inputs(B, n, O, E, E, A, True, seed=3)
    y = torch.full((B,), 7., device='cuda')
    ok = lambda **k: vtrace_args(dev, B, n, E, E, A, k.get('use_is', True), y)  # noqa: E731
    lib = native.load()
    import ctypes as C
    s = native._stream()

    def call(a, beta, v, O_):
        return lib.asac_option_return(C.byref(a), native._p(beta), n, 1, native._p(v), n * O, O, 1, O_, s)
    assert call(ok(), dev['beta'], dev['v_opt'], O) == 0
    bad = 1     # hipErrorInvalidValue
    assert call(ok(), None, dev['v_opt'], O) == bad
    assert call(ok(), dev['beta'], None, O) == bad
    assert call(ok(), dev['beta'], dev['v_opt'], 0) == bad
    assert call(ok(), dev['beta'], dev['v_opt'], -2) == bad
    a = ok()
    a.pi_prob = None                                      # importance sampling without probabilities
    assert call(a, dev['beta'], dev['v_opt'], O) == bad
    a = ok()
    a.n = 20000                                           # one row's two slabs no longer fit 64 KB of LDS
    assert call(a, dev['beta'], dev['v_opt'], O) == bad
    with pytest.raises(native.AsacNativeError):
        native.option_return(a, None, None)
    torch.cuda.synchronize()
    y.fill_(7.)
    assert call(ok(), None, dev['v_opt'], O) == bad
    torch.cuda.synchronize()
    assert (y == 7.).all()                                # nothing was launched


# ------------------------------------------------------------------------------------------------------------------------
TERM_B = (1, 64, 257, 10000)


@pytest.mark.parametrize('done_mode', ['none', 'mixed', 'all'])
@pytest.mark.parametrize('with_is', [False, True])
def test_termination_loss_grad_against_float64(with_is, done_mode):
    from asac_amd import native
    O, te = 3, 0.05
    cu = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    rows = []       # (B, kernel loss error, composition loss error, kernel gradient error, composition gradient error)
    for B in TERM_B:
        rng = np.random.default_rng(B * 7 + with_is)
        beta = rng.random((B, 1)).astype(np.float32)
        y = rng.standard_normal((B, 1)).astype(np.float32)
        v = rng.standard_normal((B, O)).astype(np.float32)
        w = (rng.random((B, 1)) + 0.5).astype(np.float32)
        done = {'none': np.zeros(B, bool), 'mixed': rng.random(B) < 0.4, 'all': np.ones(B, bool)}[done_mode]
        outs = []
        for _ in range(2):
            loss, g = torch.full((1,), float('nan'), device='cuda'), torch.full((B,), float('nan'), device='cuda')
            native.termination_loss_grad(cu(beta), cu(y), cu(v), cu(done), cu(w) if with_is else None, te, loss, g)
            outs.append((loss.cpu(), g.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])      # same input, same bits
        loss, g = outs[0]
        assert (g[torch.from_numpy(done)] == 0).all()
        if done_mode == 'all':
            assert float(loss) == 0. and (g == 0).all()
            continue
        keep = (~done)[:, None].astype(np.float64)
        adv = y.astype(np.float64) - v.astype(np.float64).mean(-1, keepdims=True) + te
        w64 = w.astype(np.float64) if with_is else 1.
        want_loss = float((beta.astype(np.float64) * adv * keep * w64).mean())
        want_g = (adv * keep * w64 / B).reshape(-1)
        # the PyTorch-ROCm float32 composition of option_base.py:693-703 on the same inputs
        tb = cu(beta).requires_grad_(True)
        l32 = tb * (cu(y) - cu(v).mean(-1, keepdim=True) + te) * ~cu(done).unsqueeze(-1)
        if with_is:
            l32 = l32 * cu(w)
        l32 = torch.mean(l32)
        l32.backward()
        # the loss is a mean of B signed terms: its error is measured against the terms' size, not against a sum that
        # cancels; a gradient entry against the row's advantage / B
        lscale = float(np.abs(beta * adv * keep * w64).mean()) + 1e-30
        gscale = np.abs(adv * w64 / B).reshape(-1) + 1e-30
        rows.append((B, abs(float(loss) - want_loss) / lscale, abs(float(l32.detach()) - want_loss) / lscale,
                     float((np.abs(_np(g) - want_g) / gscale).max()),
                     float((np.abs(_np(tb.grad).reshape(-1) - want_g) / gscale).max())))
    if done_mode == 'all':
        return
    # 4x the composition's error over the family (every B of this weighting and done pattern); no floor
    pooled_loss, pooled_g = max(r[2] for r in rows), max(r[4] for r in rows)
    print(f'termination_loss_grad is={with_is} done={done_mode}: composition loss {pooled_loss:.3e} grad {pooled_g:.3e}; '
          + ' '.join(f'B={r[0]}: {r[1]:.2e}/{r[3]:.2e}' for r in rows))
    for B, e_loss, _, e_g, _ in rows:
        assert e_loss <= 4. * pooled_loss, (B, e_loss, pooled_loss)
        assert e_g <= 4. * pooled_g, (B, e_g, pooled_g)


def test_termination_loss_grad_takes_strided_views():
    from asac_amd import native
    B, O = 300, 4
    rng = np.random.default_rng(5)
    wide = torch.from_numpy(rng.standard_normal((B, 6)).astype(np.float32)).cuda()
    vt = torch.from_numpy(rng.standard_normal((O, B)).astype(np.float32)).cuda()
    done = torch.from_numpy(rng.random(B) < 0.3).cuda()
    res = []
    for contiguous in (False, True):
        beta, y, w, v = wide[:, 1:2], wide[:, 3:4], wide[:, 5:6], vt.t()
        if contiguous:
            beta, y, w, v = (x.contiguous() for x in (beta, y, w, v))
        loss, g = torch.empty(1, device='cuda'), torch.empty(B, device='cuda')
        native.termination_loss_grad(beta, y, v, done, w, -0.1, loss, g)
        res.append((loss.cpu(), g.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------------------------------
# the class against the reference's fixtures
# ------------------------------------------------------------------------------------------------------------------------
IS = dict(gamma=0.99, v_lambda=0.95, v_rho=1.0, v_c=0.9)
F15 = {     # case -> (plugin under tests.plugins, learner keywords, discrete action sizes, continuous size, fix_policy)
    'mlp': ('nn_oc', dict(n_step=4, use_n_step_is=True, **IS), (), 2, False),
    'mlp_n1': ('nn_oc', dict(n_step=1, use_n_step_is=False, clip_epsilon=0.2), (), 2, False),
    'rnn': ('nn_oc_rnn', dict(n_step=3, seq_encoder='RNN', **IS), (), 2, False),
    'hybrid': ('nn_oc_small', dict(n_step=3, ensemble_q_num=3, ensemble_q_sample=2, **IS), (3, 2), 2, False),
    'dqn': ('nn_oc_small', dict(n_step=3, discrete_dqn_like=True, ensemble_q_num=3, ensemble_q_sample=2), (3, 2), 0, False),
    'fix_policy': ('nn_oc', dict(n_step=4, use_n_step_is=True, **IS), (), 2, True),
}


def make_option(case, model_abs_dir=None, **extra):
    import asac_amd  # noqa: F401
    from algorithm.oc import OptionBase
    from algorithm.utils.enums import convert_config_to_enum
    plugin_name, kw, d_sizes, c_size, fix_policy = F15[case]
    kw = dict(kw)
    convert_config_to_enum(kw)
    return OptionBase(0, 'option_0', fix_policy, False, ['vector'], [(6,)], list(d_sizes), c_size, model_abs_dir,
                      pu.plugin(plugin_name), device='cuda:0', batch_size=16, summary_path=None, **kw, **extra)


def first_moments(opt) -> dict:
    """{optimizer name: [Adam first-moment view per parameter]} with the reference's optimizer names"""
    out = {}
    names = {'optimizer_rep': opt.optimizer_rep, 'optimizer_policy': opt.optimizer_policy}
    names.update({f'optimizer_q_{i}': o for i, o in enumerate(opt.optimizer_q_list)})
    for name, o in names.items():
        if o is None:
            continue
        views = []
        for seg in o.names:
            off = o.group.segments[seg][0]
            for p in o.group.params[seg]:
                views.append(o.exp_avg[off:off + p.numel()].view(p.shape))
                off += p.numel()
        out[name] = views
    t = opt.optimizer_termination
    out['optimizer_termination'] = [t.exp_avg[off:off + p.numel()].view(p.shape) for p, off in t._param_slots()]
    return out


OPTIMIZER_OF = {'model_rep': 'optimizer_rep', 'model_policy': 'optimizer_policy', 'model_termination': 'optimizer_termination'}
# Where is the sign of an Adam step from zero moments, lr * g / (|g| + 1e-8), not determined by the fixture?  Only where the
# recorded gradient is within float32 rounding of zero: an entry is a sum of a few dozen products (16 rows, up to 64 inputs),
# so 16 roundings of the tensor's largest entry; or where |g| is within a hundred of Adam's eps (first moment 0.1 g < 1e-7),
# where the step's size depends on g itself.  Fixed here, independent of tests/option_tolerances.json; which entries these
# are is a property of the fixture alone (the recorded gradients), and a tensor with more than 1 in 100 of them fails.
UNDETERMINED_SHARE, UNDETERMINED_ABS, UNDETERMINED_MAX_SHARE = 16 * EPS32, 1e-7, 1e-2


def check_weights(case, g, mods, prefix, lr=3e-4, want_prefix=None, g0_prefix='g0'):
    """EVERY entry of the weights after a step is compared, as an update (weight - w0: an update is ~1e-4 of a weight).
    Entries whose recorded first moment is non-zero but undetermined in sign (see above) may differ by up to two steps;
    they are counted, and more than UNDETERMINED_MAX_SHARE of a tensor (at least 2 entries) fails."""
    seen = 0
    for name, mod in mods.items():
        oname = OPTIMIZER_OF.get(name, name.replace('model_', 'optimizer_'))
        param_index = {k: j for j, (k, _) in enumerate(mod.named_parameters())}
        for k, v in mod.state_dict().items():
            key = f'{want_prefix or prefix}/{name}/{k}'
            if key not in g.files:
                continue
            base = g[f'w0/{name}/{k}'].astype(np.float64)
            got, want = _np(v) - base, g[key].astype(np.float64) - base
            gkey = f'{g0_prefix}/{oname}/{param_index.get(k, -1)}'
            if prefix != 'w_tgt' and gkey in g.files:
                g0 = np.abs(g[gkey].astype(np.float64))
                loose = (g0 > 0) & (g0 < max(UNDETERMINED_SHARE * float(g0.max(initial=0.)), UNDETERMINED_ABS))
                assert loose.sum() <= max(2, UNDETERMINED_MAX_SHARE * loose.size), (key, int(loose.sum()), loose.size)
                assert (np.abs(got[loose] - want[loose]) <= 2 * lr * (1 + 1e-3)).all(), key
                got = np.where(loose, want, got)
            ocheck(f'{case}/{prefix}/{name}', got, want)
            seen += 1
    return seen


def run_sequence(case, golden_dir):
    from algorithm.fused import RecordedNoise
    g = np.load(golden_dir / f'f15_option_{case}.npz')
    opt = make_option(case)
    mods = pu.load_golden_weights(opt, g)
    opt.noise = RecordedNoise(eps=[g[f'eps/{i}'] for i in range(int(g['n_eps']))],
                              perm=[g[f'perm/{i}'] for i in range(int(g['n_perm']))])
    t = {k[3:]: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in g.files
         if k.startswith('in/') and g[k].ndim > 0}
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

    d_y, c_y = opt.compute_rep_q_grads(
        t['next_n_vs_over_options'], nx_indexes[:, :-1], t['n_last_masks'], t['n_padding_masks'], nx_obses_list,
        nx_obses_list, nx_states, nx_target_states, t['n_actions'], nx_pre_actions[:, :-1], t['n_rewards'].clone(),
        t['n_dones'], t['n_mu_probs'].clone(), t['nx_pre_seq_hidden_states'][:, :-1], priority_is=priority_is)
    for name, val in (('d_y', d_y), ('c_y', c_y)):
        assert (val is not None) == (name in g.files), name
        if val is not None:
            ocheck(f'{case}/{name}', val, g[name])
    opt.train_rep_q()
    fm = first_moments(opt)

    def check_moments(names):
        for oname in names:
            for j, view in enumerate(fm.get(oname, [])):
                key = f'g0/{oname}/{j}'
                if key in g.files and np.abs(g[key]).max() > 0:
                    ocheck(f'{case}/g0/{oname}', view, g[key])
                elif key in g.files:
                    assert float(view.abs().max()) == 0., key
    check_moments(['optimizer_rep'] + [f'optimizer_q_{i}' for i in range(opt.ensemble_q_num)])
    assert check_weights(case, g, mods, 'w_rq') > 0

    nx_states_d = nx_states.detach()
    opt.train_policy_alpha(t['n_padding_masks'], [t['nx_obs'][:, :-1]], nx_states_d, t['n_actions'], t['n_mu_probs'].clone())
    if 'g0_f64/optimizer_policy/0' in g.files:
        # continuous cases: the fixture holds the policy step evaluated in float64 (the reference's float32 gradient is
        # itself up to 1e-3 off it at a policy scale of 1e-4, `ref32_error/`): first moments and weights are compared
        # with those, and the first moments must also be within 4x the reference's own error (its largest over the policy's
        # tensors) of float64
        views = fm['optimizer_policy']
        ref_own = max(float(g[f'ref32_error/optimizer_policy/{j}']) for j in range(len(views)))
        for j, view in enumerate(views):
            want = g[f'g0_f64/optimizer_policy/{j}']
            ocheck(f'{case}/g0/optimizer_policy', view, want)
            assert scaled_error(view, want) <= 4. * ref_own, (case, j, ref_own)
        check_weights(case, g, {'model_policy': mods['model_policy']}, 'w_pi', want_prefix='w_pi_f64', g0_prefix='g0_f64')
    else:
        if not opt.fix_policy and not (opt.discrete_dqn_like and not opt.c_action_size):
            check_moments(['optimizer_policy'])
        check_weights(case, g, mods, 'w_pi')

    y = c_y if c_y is not None else d_y
    opt.compute_termination_grads(float(g['in/terminal_entropy']), [t['nx_obs'][:, 0]], nx_states_d[:, 0], y.detach(),
                                  t['v_over_options'], t['done'], priority_is)
    opt.train_termination()
    ocheck(f'{case}/loss_termination', opt._loss_termination[0], g['loss_termination'])
    fm = first_moments(opt)
    check_moments(['optimizer_termination'])
    assert check_weights(case, g, mods, 'w_term') > 0

    td = opt._get_td_error(t['next_n_vs_over_options'], t['n_last_masks'], t['n_padding_masks'], nx_obses_list,
                           nx_obses_list, nx_states_d[:, 0], nx_target_states, t['n_actions'], t['n_rewards'].clone(),
                           t['n_dones'], t['n_mu_probs'].clone())
    ocheck(f'{case}/td_error', td, g['td_error'])
    assert opt.noise.exhausted()

    opt._update_target_variables(float(g['in/tau']))
    assert check_weights(case, g, mods, 'w_tgt') > 0
    opt.set_train_mode(False)
    action, prob, hidden, termination = opt.choose_action([t['act_obs']], t['act_pre_action'], t['act_pre_hidden'],
                                                          disable_sample=True)
    for name, val in (('action', action), ('prob', prob), ('hidden', hidden), ('termination', termination)):
        if g[f'act/{name}'].size:
            ocheck(f'{case}/act/{name}', val, g[f'act/{name}'])
        else:
            assert val.numel() == 0
    return opt, g, mods


@pytest.mark.parametrize('case', list(F15))
def test_option_against_reference_fixture(case, golden_dir):
    opt, g, mods = run_sequence(case, golden_dir)
    if case == 'fix_policy':        # representation and policy: the recorded bits, after the whole sequence
        for name in ('model_rep', 'model_policy'):
            mod = mods.get(name) or getattr(opt, name)
            for k, v in mod.state_dict().items():
                if f'w0/{name}/{k}' in g.files:
                    assert np.array_equal(v.cpu().numpy(), g[f'w0/{name}/{k}']), (name, k)
        assert int(opt._steps_pi) == 0
    opt.close()


def test_checkpoint_round_trip_and_reference_layout(tmp_path, golden_dir):
    g = np.load(golden_dir / 'f15_option_mlp.npz')
    a = make_option('mlp', model_abs_dir=tmp_path / 'a')
    pu.load_golden_weights(a, g, prefix='w_tgt')
    pu.load_golden_weights(a, g, prefix='w_term')
    a.set_global_step(7)
    a.save_model()
    b = make_option('mlp', model_abs_dir=tmp_path / 'a')
    assert b.get_global_step() == 7
    for name, mod in a.ckpt_dict.items():
        if isinstance(mod, torch.nn.Module):
            for (k, x), (_, y) in zip(mod.state_dict().items(), b.ckpt_dict[name].state_dict().items()):
                assert torch.equal(x, y), (name, k)
    # restored weights live in the flat buffers the kernels read
    s, e = b._params.span('termination')
    flat = torch.cat([p.reshape(-1) for p in b.model_termination.parameters()])
    assert torch.equal(b._params.flat[s:s + flat.numel()], flat)
    tflat = torch.cat([p.reshape(-1) for p in b.model_target_termination.parameters()])
    assert torch.equal(b._target_termination_params.flat[:tflat.numel()], tflat)
    b.remove_models(3)
    assert not list((tmp_path / 'a' / 'model').glob('*.pth'))
    a.close(), b.close()

    # a checkpoint in the reference's layout: module state dicts under the reference's keys, no optimizers
    names = sorted({k.split('/')[1] for k in g.files if k.startswith('w0/model_')})
    ck = {name: {k.split('/', 2)[2]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(f'w0/{name}/')}
          for name in names}
    ck['log_d_alpha'], ck['log_c_alpha'] = torch.from_numpy(g['w0/log_d_alpha'].copy()), torch.from_numpy(g['w0/log_c_alpha'].copy())
    ck['global_step'] = torch.tensor(11)
    (tmp_path / 'r' / 'model').mkdir(parents=True)
    torch.save(ck, tmp_path / 'r' / 'model' / '11.pth')
    c = make_option('mlp', model_abs_dir=tmp_path / 'r')
    assert c.get_global_step() == 11 and 'model_termination' in names and 'model_target_termination' in names
    for name in names:
        for k, v in c.ckpt_dict[name].state_dict().items():
            assert np.array_equal(v.cpu().numpy(), g[f'w0/{name}/{k}']), (name, k)
    c.close()


def test_termination_optimizer_state_is_adam_s_format(golden_dir):
    opt, g, _ = run_sequence('mlp_n1', golden_dir)
    sd = opt.optimizer_termination.state_dict()
    ref = torch.optim.Adam([torch.nn.Parameter(p.detach().cpu().clone()) for p in opt.model_termination.parameters()],
                           lr=opt.learning_rate)
    ref.load_state_dict(sd)         # torch's own loader accepts it
    assert int(float(sd['state'][0]['step'])) == 1 and int(opt._steps_rep_q) == 1 and int(opt._steps_pi) == 1
    opt.close()


def test_second_sequence_steps_adam_with_its_own_counters(golden_dir):
    """a second pass over the same option: the gradients each pass leaves are fed to torch.optim.Adam on the host, and the
    critics' and the termination head's weights after two passes must be what Adam gives (bias correction with the step
    counts of the separate optimizer groups, gradient buffers zeroed between passes)"""
    from algorithm.fused import RecordedNoise
    g = np.load(golden_dir / 'f15_option_mlp_n1.npz')
    opt = make_option('mlp_n1')
    pu.load_golden_weights(opt, g)
    t = {k[3:]: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in g.files if k.startswith('in/') and g[k].ndim > 0}
    obs = [t['nx_obs']]
    groups = {'q': (opt.model_q_list[0], 'q_0'), 'term': (opt.model_termination, 'termination')}
    host = {k: [torch.nn.Parameter(p.detach().cpu().clone()) for p in m.parameters()] for k, (m, _) in groups.items()}
    adam = {k: torch.optim.Adam(ps, lr=opt.learning_rate) for k, ps in host.items()}

    def grads_of(seg):
        s, _ = opt._params.span(seg)
        out = []
        for p in opt._params.params[seg]:
            out.append(opt._params.grad[s:s + p.numel()].view(p.shape).detach().cpu().clone())
            s += p.numel()
        return out

    def host_step(k, seg):
        for p, gr in zip(host[k], grads_of(seg)):
            p.grad = gr
        adam[k].step()
    for rep in range(2):
        eps = [g[f'eps/{i}'] for i in range(int(g['n_eps']))]
        opt.noise = RecordedNoise(eps=eps, perm=[g[f'perm/{i}'] for i in range(int(g['n_perm']))])
        nx = t['nx_obs']
        _, c_y = opt.compute_rep_q_grads(t['next_n_vs_over_options'], None, t['n_last_masks'], t['n_padding_masks'], obs, obs,
                                         nx, nx, t['n_actions'], None, t['n_rewards'].clone(), t['n_dones'],
                                         t['n_mu_probs'].clone(), None, priority_is=t['priority_is'])
        host_step('q', 'q_0')
        opt.train_rep_q()
        opt.train_policy_alpha(t['n_padding_masks'], [nx[:, :-1]], nx, t['n_actions'], t['n_mu_probs'].clone())
        opt.compute_termination_grads(0.05, [nx[:, 0]], nx[:, 0], c_y, t['v_over_options'], t['done'], t['priority_is'])
        host_step('term', 'termination')
        opt.train_termination()
        opt._get_td_error(t['next_n_vs_over_options'], t['n_last_masks'], t['n_padding_masks'], obs, obs, nx[:, 0], nx,
                          t['n_actions'], t['n_rewards'].clone(), t['n_dones'], t['n_mu_probs'].clone())
    assert int(opt._steps_rep_q) == 2 and int(opt._steps_pi) == 2 and int(opt.optimizer_termination.steps_done) == 2
    for k, (m, _) in groups.items():
        for p, h in zip(m.parameters(), host[k]):
            # same gradients, same Adam: float32 rounding of the update (two steps of 3e-4) only
            np.testing.assert_allclose(p.detach().cpu().numpy(), h.detach().numpy(), rtol=0, atol=2 * 3e-4 * 1e-4)
    opt.close()


def test_batch_must_be_the_learner_s():
    opt = make_option('mlp_n1')
    z = lambda *s: torch.zeros(s, device='cuda')  # noqa: E731
    m = lambda *s: torch.zeros(s, dtype=torch.bool, device='cuda')  # noqa: E731
    with pytest.raises(ValueError, match='batch_size'):
        opt.compute_rep_q_grads(z(8, 1, 3), None, m(8, 1), m(8, 1), [z(8, 2, 6)], [z(8, 2, 6)], z(8, 2, 6), z(8, 2, 6),
                                z(8, 1, 2), None, z(8, 1), m(8, 1), z(8, 1, 2), None)
    opt.close()


def test_random_q_reinitialises_the_critics_and_copies_the_targets():
    torch.manual_seed(3)
    a = make_option('mlp_n1')
    torch.manual_seed(3)
    from algorithm.oc import OptionBase
    b = OptionBase(0, 'option_0', False, True, ['vector'], [(6,)], [], 2, None, pu.plugin('nn_oc'), device='cuda:0',
                   batch_size=16, summary_path=None, n_step=1, use_n_step_is=False)
    for qa, qb, tb in zip(a.model_q_list, b.model_q_list, b.model_target_q_list):
        for pa, pb, pt in zip(qa.parameters(), qb.parameters(), tb.parameters()):
            assert not torch.equal(pa, pb) and torch.equal(pb, pt)
            assert pb.data_ptr() >= b._params.flat.data_ptr()      # still a view of the flat buffer
        biases = [p for p in qb.parameters() if p.dim() == 1]
        assert max(float(p.abs().max()) for p in biases) > 0.5       # normal(0, 1), not the zero / small default
    for pa, pb in zip(a.model_policy.parameters(), b.model_policy.parameters()):
        assert torch.equal(pa, pb)
    a.close(), b.close()
