"""GPU: the offline loss (`offline_enabled and offline_loss`, reference sac_base.py:1899-1900) inside the policy-step
launches (`hip_config['fused_offline']`, csrc/mlp.hip, csrc/returns.hip).

Kernel level
  * the policy gradient of `backward_policy_sample(..., offline=a)` and of `policy_step_fused(..., offline=a)` (action given
    and sampled inside) and the objective of `policy_loss_fwd_bwd` + `policy_offline_term` against the float64 restatement
    tests/offline_ref.py, per key within max(4 x the error recorded on an MI355X in tests/offline_tolerances.json, one float32
    rounding) — a missing key fails, `ASAC_OFFLINE_RECORD=<file.json>` (`=1`: tests/offline_tolerances.recorded.json) records
    instead — and, for gradients, within the 2e-4 that tests/test_fused_mlp_gpu.py::test_policy_step_fused_backwards_match_the_kernel_chain holds this chain to
  * bit equalities: one launch (given) == one launch (sampled inside) == chain with the term on; an `_offline` entry point
    fed the sample itself as the stored action (a term of exactly zero) == the plain entry point
  * the term is really in, bad arguments are refused without a launch
Learner level
  * the reference's own fixture tests/golden/f6_step_offline.npz replayed with the switch on and off under the bounds of
    tests/test_sac_step_gpu.py::TOL (`parity_utils.check`, keys under `offline/`), launch multiset, graph replay == eager,
    the plain-Gaussian autograd path with a plugin critic, and what stays on the eager branch"""
import collections
import json
import os
import random
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import offline_ref as ref  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.golden import make_offline_golden as mog  # noqa: E402
from tests.test_sac_step_gpu import LR, TOL  # noqa: E402

HERE = Path(__file__).resolve().parent
EPS32 = float(np.finfo(np.float32).eps)
GRAD_BOUND = 2e-4           # a gradient error above this is a defect to find, not a number to record
_TOL_PATH = HERE / 'offline_tolerances.json'
_record = os.environ.get('ASAC_OFFLINE_RECORD')
RECORD = None if not _record else (HERE / 'offline_tolerances.recorded.json' if _record == '1' else Path(_record))
_TABLE = json.loads(_TOL_PATH.read_text()) if _TOL_PATH.exists() else {}
MEASURED = _TABLE.get('float64', {})           # key -> max |got - want| / max |want| against tests/offline_ref.py
PARITY = _TABLE.get('parity', {})              # `parity_utils.check` keys under offline/ -> {'used_of_default': ...}
RECORDED = {'float64': {}, 'parity': {}}


def _write_record():
    RECORD.parent.mkdir(parents=True, exist_ok=True)
    old = json.loads(RECORD.read_text()) if RECORD.exists() else {}
    out = {'float64': dict(old.get('float64', {})), 'parity': dict(old.get('parity', {}))}
    for k, v in RECORDED['float64'].items():
        out['float64'][k] = max(v, out['float64'].get(k, 0.))
    for k, v in RECORDED['parity'].items():
        out['parity'][k] = {'used_of_default': max(v, out['parity'].get(k, {}).get('used_of_default', 0.))}
    RECORD.write_text(json.dumps(out, indent=1, sort_keys=True))


def scaled_error(got, want) -> float:
    """max |got - want| over the largest magnitude of `want`"""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max(initial=0.) / max(float(np.abs(want).max(initial=0.)), 1e-300))


def enforced(key) -> float:
    """the bound `fcheck` holds `key` to: 4 x the recorded error, not below one float32 rounding"""
    if RECORD:
        return GRAD_BOUND
    assert key in MEASURED, f'{key!r} has no entry in tests/offline_tolerances.json (ASAC_OFFLINE_RECORD=1 records it)'
    return max(4. * MEASURED[key], EPS32)


def fcheck(key, err, gradient=True):
    print(f'offline parity {key}: {err:.3e}')
    if gradient:
        assert err <= GRAD_BOUND, (key, err)
    if RECORD:
        RECORDED['float64'][key] = max(RECORDED['float64'].get(key, 0.), err)
        _write_record()
        return
    assert err <= enforced(key), (key, err, MEASURED[key])


def grads_error(got_flat, want_tensors, scale=1.) -> float:
    """worst `scaled_error` over the policy's parameter tensors; `got_flat`: `scale` times the flat gradient, the tensors
    back to back in `parameters()` order (FlatParamGroup; only the segment's end is padded)"""
    worst, off = 0., 0
    for w in want_tensors:
        n = w.numel()
        worst = max(worst, scaled_error(got_flat[off:off + n].view(w.shape).double() / scale, w))
        off += n
    assert off <= got_flat.numel() < off + 4
    return worst


def test_the_recorded_gradient_errors_are_below_the_chains_bound():
    assert MEASURED, 'tests/offline_tolerances.json is missing'
    for key, v in MEASURED.items():
        if not key.startswith(('objective/', 'term/')):
            assert v <= GRAD_BOUND, (key, v)


# ------------------------------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------------------------------
def _setup(E, state, A, policy=False, seed=0):
    """tests/test_fused_mlp_gpu.py::_setup: E stock critics (or the stock policy) in flat buffers -> (modules, group, StockMLP)"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_mlp import StockMLP, describe_policy, describe_q
    torch.manual_seed(seed)
    if policy:
        mods = [m.ModelPolicy(state, [], A).cuda()]
        desc = describe_policy(mods[0])
    else:
        mods = [m.ModelQ(state, [], A, False).cuda() for _ in range(E)]
        desc = describe_q(mods[0])
    assert desc is not None
    with torch.no_grad():      # non-trivial biases
        for mod in mods:
            for p in mod.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.3)
    group = FlatParamGroup([(f'm{i}', list(mod.parameters())) for i, mod in enumerate(mods)], 'cuda')
    stride = group.segments['m0'][1] - group.segments['m0'][0]
    mlp = StockMLP(desc, group.flat, group.grad, 0, stride, len(mods), torch.device('cuda'))
    return mods, group, mlp


SHAPES = [(6, 1), (6, 2), (61, 3), (8, 8)]          # (S, A); A = 8: the head's limit, 2 A = 16
ROWS = [1, 16, 17, 45, 256]                         # a partial 16-row tile, an exact one, one row more, many tiles
CRITICS = [(2, None), (4, (2, 0)), (4, (1, 3))]     # (E, the two members the objective samples)


def _case(N, S, A):
    """the networks and inputs of one shape.  Stored actions: a [N, 3, A] window read at position 1 (row stride 3 A, base
    offset A); states: strided rows too; eps scaled by 3, and its first element set so that u = 8 there: |u| passes 7.25 —
    where the eager branch's atanh(clamp(tanh(u))) saturates — in every shape"""
    pmods, pgroup, fpi = _setup(1, S, A, policy=True)
    critics = {E: _setup(E, S, A, seed=E) for E in (2, 4)}
    gen = torch.Generator().manual_seed(1000 * N + 10 * S + A)
    x = torch.randn(N, 3, S, generator=gen).cuda()[:, 1]
    eps = (3. * torch.randn(N, A, generator=gen)).cuda()
    ls = fpi._launch_forward(x, None)[0]
    eps[0, 0] = (8. - ls[0, 0]) / ls[0, A]
    stored = torch.rand(N, 3, A, generator=gen).cuda()[:, 1]
    assert stored.stride(0) == 3 * A and stored.storage_offset() == A and x.stride(0) == 3 * S
    log_alpha = torch.tensor(-0.7, device='cuda')
    return dict(N=N, S=S, A=A, pi=pmods[0], pgroup=pgroup, fpi=fpi, critics=critics, x=x, eps=eps, stored=stored,
                log_alpha=log_alpha)


def _reference(c, E, subset, offline=True):
    qs = [ref.double_copy(q) for q in c['critics'][E][0]]
    return ref.policy_objective(ref.double_copy(c['pi']), qs, c['x'], c['eps'], c['stored'], c['log_alpha'],
                                subset=subset, offline=offline)


def _sub(subset):
    return None if subset is None else torch.tensor(subset, dtype=torch.int32, device='cuda')


def _sample(c):
    """policy forward + sampling launch -> (ls [N, 2A], a_tanh, logp)"""
    from asac_amd import native
    N, A = c['N'], c['A']
    ls = c['fpi']._launch_forward(c['x'], None)[0]
    a, logp = torch.empty(N, A, device='cuda'), torch.empty(N, device='cuda')
    native.squash_sample_fwd(ls[:, :A], ls[:, A:], c['eps'], a, logp)
    return ls, a, logp


def _chain(c, E, subset, a, offline, defer=False):
    """critics forward + backward_policy_q + backward_policy_sample -> the value table"""
    fq, fpi, N = c['critics'][E][2], c['fpi'], c['N']
    q = fq._launch_forward(c['x'], a)
    ga = fq.backward_policy_q(c['x'], a, q.view(E, N), _sub(subset), 2)
    fpi.backward_policy_sample(c['x'], c['eps'], ga, c['log_alpha'], defer=defer, offline=offline)
    return q


def _partials(fpi, N):
    from asac_amd import native
    tiles, used = native.mlp_backward_tiles(N, 1), native.mlp_param_extent(fpi.desc)
    return fpi._workspace[:tiles * fpi.member_stride].view(tiles, -1)[:, :used].clone()


def _adam(pgroup):
    from algorithm.fused import FlatAdam
    steps = torch.zeros(1, dtype=torch.int64, device='cuda')
    return FlatAdam(pgroup, ['m0'], 1e-3, steps, torch.zeros_like(pgroup.flat), torch.zeros_like(pgroup.flat))


@pytest.mark.parametrize('S,A', SHAPES)
@pytest.mark.parametrize('N', ROWS)
def test_policy_step_with_the_offline_term_against_float64(N, S, A):
    """every policy parameter's gradient from the chain and from the one-launch step (action given / sampled inside), in
    the three reduce modes, against float64 autograd; the three forms bit for bit; the term really in"""
    from asac_amd import native
    c = _case(N, S, A)
    fpi, pgroup, x, eps, stored, la = c['fpi'], c['pgroup'], c['x'], c['eps'], c['stored'], c['log_alpha']
    ls, a, logp = _sample(c)
    u = ls[:, :A].double() + eps.double() * ls[:, A:].double()
    assert float(u.abs().max()) > 7.25, 'the shapes are to pass the eager branch\'s clamp'
    shape = f'N{N}_S{S}_A{A}'
    flat0 = pgroup.flat.clone()
    used = native.mlp_param_extent(fpi.desc)
    grad = lambda: pgroup.grad[:used].clone()  # noqa: E731
    for E, subset in CRITICS:
        fq, qgroup = c['critics'][E][2], c['critics'][E][1]
        assert fpi.policy_step_fused_ok(fq, N)
        _, want = _reference(c, E, subset)
        _, plain = _reference(c, E, subset, offline=False)
        sub = _sub(subset)
        # ---- the chain: overwrite (a filled buffer), accumulate (onto the gradient itself: exactly twice it), defer + Adam
        fpi.accumulate = False
        pgroup.grad.fill_(7.)
        q = _chain(c, E, subset, a, stored)
        g_chain = grad()
        fcheck(f'sample/{shape}', grads_error(g_chain, want))
        fpi.accumulate = True
        _chain(c, E, subset, a, stored)
        assert torch.equal(grad(), 2. * g_chain), 'accumulate'
        fpi.accumulate = False
        pgroup.grad.zero_()
        _chain(c, E, subset, a, stored, defer=True)
        p_chain = _partials(fpi, N)
        assert pgroup.grad.count_nonzero() == 0
        fpi.adam_partials(_adam(pgroup))
        assert torch.equal(grad(), g_chain), 'partials summed by the Adam launch == reduced in the backward launch'
        pgroup.flat.copy_(flat0)
        # ---- one launch, action given
        q_out = torch.zeros(E, N, 1, device='cuda')
        pgroup.grad.fill_(7.)
        fpi.policy_step_fused(fq, x, a, eps, la, q_out=q_out, subset=sub, offline=stored)
        g_given = grad()
        fcheck(f'fused_given/{shape}', grads_error(g_given, want))
        assert torch.equal(g_given, g_chain), 'one launch (given) == chain: reduced gradient'
        for e in (subset or (0, 1)):
            assert torch.equal(q_out[e], q[e]), 'value table'
        fpi.accumulate = True
        fpi.policy_step_fused(fq, x, a, eps, la, subset=sub, offline=stored)
        assert torch.equal(grad(), 2. * g_chain), 'accumulate'
        fpi.accumulate = False
        fpi._workspace.fill_(float('nan'))
        pgroup.grad.zero_()
        fpi.policy_step_fused(fq, x, a, eps, la, defer=True, subset=sub, offline=stored)
        assert torch.equal(_partials(fpi, N), p_chain), 'one launch (given) == chain: per-tile partials'
        fpi.adam_partials(_adam(pgroup))
        assert torch.equal(grad(), g_chain)
        pgroup.flat.copy_(flat0)
        # ---- one launch, action sampled inside
        out = (torch.zeros(N, A, device='cuda'), torch.zeros(N, device='cuda'), torch.zeros(N, 2 * A, device='cuda'))
        q_out.zero_()
        pgroup.grad.fill_(7.)
        fpi.policy_step_fused(fq, x, None, eps, la, q_out=q_out, subset=sub, sample_out=out, offline=stored)
        g_inside = grad()
        fcheck(f'fused_inside/{shape}', grads_error(g_inside, want))
        assert torch.equal(out[0], a) and torch.equal(out[1], logp) and torch.equal(out[2], ls), 'sampled on chip'
        assert torch.equal(g_inside, g_chain), 'one launch (sampled inside) == chain: reduced gradient'
        for e in (subset or (0, 1)):
            assert torch.equal(q_out[e], q[e])
        fpi._workspace.fill_(float('nan'))
        pgroup.grad.zero_()
        fpi.policy_step_fused(fq, x, None, eps, la, defer=True, subset=sub, sample_out=out, offline=stored)
        assert torch.equal(_partials(fpi, N), p_chain), 'one launch (sampled inside) == chain: per-tile partials'
        fpi.adam_partials(_adam(pgroup))
        assert torch.equal(grad(), g_chain)
        pgroup.flat.copy_(flat0)
        assert qgroup.grad.count_nonzero() == 0, 'the critics get no gradient from the policy step'
        # ---- the term is really in: without it the float64 gradient is at least 100 bounds away
        moved = max(scaled_error(p, w) for p, w in zip(plain, want))
        for kind in ('sample', 'fused_given', 'fused_inside'):
            assert moved >= 100. * enforced(f'{kind}/{shape}'), (kind, moved)


@pytest.mark.parametrize('S,A', [(6, 2), (8, 8)])
def test_backward_policy_sample_on_32_row_tiles(S, A):
    """4 097 rows: 32-row tiles, where the one-launch step refuses and the learner keeps the chain"""
    N, (E, subset) = 4097, CRITICS[1]
    c = _case(N, S, A)
    fpi, pgroup = c['fpi'], c['pgroup']
    assert not fpi.policy_step_fused_ok(c['critics'][E][2], N)
    _, a, _ = _sample(c)
    _, want = _reference(c, E, subset)
    _, plain = _reference(c, E, subset, offline=False)
    key = f'sample/N{N}_S{S}_A{A}'
    from asac_amd import native
    used = native.mlp_param_extent(fpi.desc)
    fpi.accumulate = False
    pgroup.grad.fill_(7.)
    _chain(c, E, subset, a, c['stored'])
    g = pgroup.grad[:used].clone()
    fcheck(key, grads_error(g, want))
    fpi.accumulate = True
    _chain(c, E, subset, a, c['stored'])
    assert torch.equal(pgroup.grad[:used], 2. * g), 'accumulate'
    fpi.accumulate = False
    pgroup.grad.zero_()
    _chain(c, E, subset, a, c['stored'], defer=True)
    fpi.adam_partials(_adam(pgroup))
    # (129 tiles: the backward launch's reduction sums them in slices, the Adam launch in tile order — two orders, one bound)
    fcheck(key, grads_error(pgroup.grad[:used].clone(), want))
    assert max(scaled_error(p, w) for p, w in zip(plain, want)) >= 100. * enforced(key)


@pytest.mark.parametrize('N,S,A', [(1, 6, 1), (17, 6, 2), (45, 61, 3), (256, 8, 8)])
def test_a_zero_term_is_the_plain_entry_point_bit_for_bit(N, S, A):
    """the `_offline` entry points fed the pre-tanh sample itself as the stored action add a term of exactly zero: gradient,
    partials and value table of the plain entry points (`offline=None`), bit for bit, in every form"""
    c = _case(N, S, A)
    fpi, pgroup, x, eps, la = c['fpi'], c['pgroup'], c['x'], c['eps'], c['log_alpha']
    E, subset = CRITICS[0]
    fq, qgroup = c['critics'][E][2], c['critics'][E][1]
    ls, a, _ = _sample(c)
    wide = torch.zeros(N, 3, A, device='cuda')
    wide[:, 1] = ls[:, :A] + eps * ls[:, A:]             # u, in the kernels' evaluation order (no contraction there)
    u = wide[:, 1]
    fpi.accumulate = False
    results = []
    for offline in (None, u):
        pgroup.grad.fill_(7.)
        q = _chain(c, E, subset, a, offline)
        g_chain = pgroup.grad.clone()
        _chain(c, E, subset, a, offline, defer=True)
        p_chain = _partials(fpi, N)
        q_out = torch.zeros(E, N, 1, device='cuda')
        pgroup.grad.fill_(7.)
        fpi.policy_step_fused(fq, x, a, eps, la, q_out=q_out, offline=offline)
        g_given = pgroup.grad.clone()
        out = (torch.zeros(N, A, device='cuda'), torch.zeros(N, device='cuda'), torch.zeros(N, 2 * A, device='cuda'))
        q_in = torch.zeros(E, N, 1, device='cuda')
        pgroup.grad.fill_(7.)
        fpi.policy_step_fused(fq, x, None, eps, la, q_out=q_in, sample_out=out, offline=offline)
        g_inside = pgroup.grad.clone()
        fpi._deferred_rows = None
        results.append((q, g_chain, p_chain, q_out, g_given, q_in, g_inside))
    for name, old, new in zip(('q', 'chain', 'partials', 'q given', 'given', 'q inside', 'inside'), *results):
        assert torch.equal(old, new), name
    assert qgroup.grad.count_nonzero() == 0


@pytest.mark.parametrize('N,S,A', [(N, S, A) for N in ROWS for S, A in SHAPES] + [(4097, 6, 2), (4097, 8, 8)])
def test_offline_term_value_and_gradient(N, S, A):
    """`policy_loss_fwd_bwd` + `policy_offline_term`: the objective against float64, the term's gradient against
    2 (u - a) / N in float64"""
    from asac_amd import native
    c = _case(N, S, A)
    E, subset = CRITICS[1]
    fq = c['critics'][E][2]
    ls, a, logp = _sample(c)
    q = fq._launch_forward(c['x'], a)
    loss, ent = torch.zeros((), device='cuda'), torch.zeros((), device='cuda')
    native.policy_loss_fwd_bwd(logp, q.view(E, N), _sub(subset), 2, c['log_alpha'], ls[:, A:], loss,
                               torch.empty(N, device='cuda'), torch.empty(E, N, device='cuda'), ent)
    before = loss.clone()
    g_u = torch.full((N, A), 7., device='cuda')
    native.policy_offline_term(ls, c['eps'], c['stored'], loss, g_u)
    want_obj, _ = _reference(c, E, subset)
    shape = f'N{N}_S{S}_A{A}'
    fcheck(f'objective/{shape}', scaled_error(loss, want_obj), gradient=False)
    want_term, want_g = ref.offline_grad_u(ls[:, :A], ls[:, A:], c['eps'], c['stored'])
    fcheck(f'term/{shape}', scaled_error(loss.double() - before.double(), want_term), gradient=False)
    fcheck(f'term_grad/{shape}', scaled_error(g_u, want_g))
    again = before.clone()
    native.policy_offline_term(ls, c['eps'], c['stored'], again)          # without the gradient: the same sum
    assert torch.equal(again, loss)


def test_entry_points_refuse_bad_arguments():
    """no stored actions, a row stride below A: hipErrorInvalidValue and no launch (the buffers keep their fill)"""
    import ctypes as C
    from asac_amd import native
    N, S, A = 16, 6, 2
    c = _case(N, S, A)
    fpi, pgroup = c['fpi'], c['pgroup']
    fq = c['critics'][2][2]
    _, a, _ = _sample(c)
    pgroup.grad.fill_(7.)
    lib, p = native.load(), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ws = fpi._workspace_for(N)
    x0, rs0, _ = native._rows_view(c['x'])
    for off, stride in ((None, 3 * A), (p(c['stored']), A - 1)):
        rc = lib.asac_policy_step_fused_offline(C.byref(fq.desc), p(fq.params), fq.member_stride, C.byref(fpi.desc),
                                                p(fpi.params), fpi.member_stride, x0, rs0, N, p(a), p(c['eps']),
                                                p(c['log_alpha']), None, off, stride, None, None, None, None,
                                                p(fpi.grad_params), p(ws), native.MLP_REDUCE_OVERWRITE, None)
        assert rc != 0
        ga = torch.zeros(2, N, A, device='cuda')
        rc = lib.asac_mlp_backward_policy_sample_offline(C.byref(fpi._pass(c['x'], None)), p(c['eps']), p(ga), 2,
                                                         p(c['log_alpha']), off, stride, p(fpi.grad_params), p(ws),
                                                         native.MLP_REDUCE_OVERWRITE, None)
        assert rc != 0
        loss = torch.full((), 7., device='cuda')
        ls = torch.ones(N, 2 * A, device='cuda')
        rc = lib.asac_policy_offline_term(p(ls), C.c_void_p(ls.data_ptr() + 4 * A), 2 * A, p(c['eps']), off, stride, N, A,
                                          p(loss), None, None)
        assert rc != 0 and float(loss) == 7.
    torch.cuda.synchronize()
    assert bool((pgroup.grad == 7.).all())


# ------------------------------------------------------------------------------------------------------------------------
# the learner
# ------------------------------------------------------------------------------------------------------------------------
SMALL = dict(batch_size=mog.SMALL['batch_size'], replay_config={'capacity': mog.SMALL['capacity']})


def _learner(plugin='nn_vec', use_graph=False, hip=None, cls=None, d_sizes=(), seed=None, **kw):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    if seed is not None:
        torch.manual_seed(seed), np.random.seed(seed), random.seed(seed)
    nn = pu.plugin(plugin) if isinstance(plugin, str) else plugin
    kw = {**mog.KW, **kw}
    return (cls or SAC_Base)(['vector'], [(6,)], list(d_sizes), mog.C_ACTION_SIZE, None, nn, device='cuda:0',
                             hip_config={'use_graph': use_graph, **(hip or {})}, **SMALL, **kw)


class _parity_defaults:
    """while recording, `parity_utils.check` runs under the call sites' default bounds; otherwise it finds the `offline/`
    keys of tests/offline_tolerances.json beside its own table (tests/parity_tolerances.json is not touched)"""

    def __enter__(self):
        self.old = os.environ.get('ASAC_PARITY_RECORD')
        if RECORD:
            os.environ['ASAC_PARITY_RECORD'] = '1'
        else:
            try:
                pu._tolerance_scale('offline/', 1.)        # (loads the table)
            except AssertionError:
                pass
            if pu._TOL_TABLE is not None:
                pu._TOL_TABLE.update({k: v for k, v in PARITY.items() if k.startswith('offline/')})

    def __exit__(self, *exc):
        if RECORD:
            if self.old is None:
                os.environ.pop('ASAC_PARITY_RECORD', None)
            else:
                os.environ['ASAC_PARITY_RECORD'] = self.old
            for k, rec in pu.PARITY_LOG.items():
                if k.startswith('offline/'):
                    RECORDED['parity'][k] = max(RECORDED['parity'].get(k, 0.), rec['used_of_default'])
            _write_record()
        return False


@pytest.mark.parametrize('fused', [True, False])
def test_reference_fixture_replayed(golden_dir, fused):
    """the reference's own steps with the offline loss (tests/golden/f6_step_offline.npz), recorded draws: PER ids equal,
    observables, first-step gradients and final weights under the bounds of tests/test_sac_step_gpu.py — with the term in
    the launches, and on the eager branch (`fused_offline` off; the fixture's samples stay clear of its clamp)"""
    from algorithm.fused import RecordedNoise
    g = np.load(golden_dir / f'f6_step_{mog.CASE}.npz')
    agent = _learner(hip={'fused_offline': fused}, cls=pu.hooked_learner())
    assert agent._stock_c_only() is fused and agent._offline_fused() is fused
    windows = []
    views = agent._window_views
    agent._window_views = lambda *a, **k: windows.append(views(*a, **k)) or windows[-1]
    mods = pu.load_golden_weights(agent, g)
    for ep in pu.golden_episodes(g, 1):
        agent.put_episode(**ep)
    rb, n_steps = agent.replay_buffer, int(g['n_steps'])
    K = f'offline/{"on" if fused else "off"}'

    missed = []

    def soft(fn, what):         # every observable of every step is looked at; what missed is raised together at the end
        try:
            fn()
        except AssertionError as e:
            missed.append(f'{what}: {str(e).strip()[:600]}')

    def chk(observable, got, want):
        soft(lambda: pu.check(f'{K}/{observable}', got, want, *TOL[observable]), f'step {s} {observable}')

    with _parity_defaults():
        for s in range(n_steps):
            eps = [g[f'step{s}/eps{j}'] for j in range(int(g[f'step{s}/n_eps']))]
            agent.noise = RecordedNoise([g[f'step{s}/u']], eps, list(g[f'step{s}/perm']))
            rb.uniform_source = agent.noise
            alpha_before = agent.log_c_alpha.detach().clone()
            assert agent.train() == s + 1
            assert agent.noise.exhausted(), 'every recorded draw must be consumed, in order'
            assert windows[-1].stock is fused
            assert np.array_equal(rb._ids.cpu().numpy(), g[f'step{s}/sample_ids']), f'step {s}: PER index selection'
            chk('is_weights', rb._w.cpu().numpy()[:, None], g[f'step{s}/is_weights'])
            chk('loss_q', agent._stats['loss_q'].item(), g[f'step{s}/loss_q'])
            agent._refresh_policy_stats(alpha_before)
            chk('loss_policy', agent._stats['loss_policy'].item(), g[f'step{s}/loss_policy'])
            chk('c_entropy', agent._stats['c_entropy'].item(), g[f'step{s}/c_entropy'])
            if s == 0:
                soft(lambda: pu.assert_first_step_gradients(agent, g, rtol=TOL['grad0'][0], atol_frac=TOL['grad0'][1],
                                                            log_key=f'{K}/grad0'), 'first-step gradients')
            chk('td_error', agent._td_error.cpu().numpy()[:, None], g[f'step{s}/td_error'])
            chk('tree', rb._tree.cpu().numpy(), g[f'step{s}/tree'])
            chk('mu_prob', rb._columns['mu_prob'].cpu().numpy(), g[f'step{s}/mu_prob'])
            chk('log_c_alpha', agent.log_c_alpha.item(), g[f'step{s}/log_c_alpha'])
        soft(lambda: pu.assert_weights_close(mods, g, n_steps, LR, *TOL['weights'], log_key=f'{K}/weights'), 'weights')
    assert not missed, '\n'.join(missed)
    # the term is in the recorded objective: without it the logged value is far off
    if fused:
        agent._pi_stats_src = agent._pi_stats_src[:2]
        agent._refresh_policy_stats(alpha_before)
        want = float(g[f'step{n_steps - 1}/loss_policy'])
        assert abs(agent._stats['loss_policy'].item() - want) > 0.1 * abs(want)
    rb.check_health()
    assert rb.check_tree_invariant() == 0
    agent.close()


def _episodes(d_sizes=(), hidden=(0,)):
    rng = np.random.default_rng(1)
    return [pu.synthetic_episode(rng, [(6,)], list(d_sizes), mog.C_ACTION_SIZE, hidden, T_) for T_ in (60, 45, 70)]


def _calls(agent, warm=2):
    """the multiset of entry-point calls of one eager `train()` (after `warm` steps)"""
    from asac_amd import native
    for ep in _episodes():
        agent.put_episode(**ep)
    for _ in range(warm):
        agent.train()
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    torch.cuda.synchronize()
    return collections.Counter({name: len(v) for name, v in prof.records.items()})


@pytest.mark.parametrize('plugin,kw,sibling', [
    ('nn_vec', {}, ('asac_policy_step_fused', 'asac_policy_step_fused_offline')),
    # `fused_policy_step` off: the chain (critics forward, backward_policy_q, backward_policy_sample)
    ('nn_vec', dict(hip={'fused_policy_step': False}), ('asac_mlp_backward_policy_sample', 'asac_mlp_backward_policy_sample_offline')),
])
def test_the_step_issues_the_launches_of_the_learner_without_the_loss(plugin, kw, sibling):
    """one eager `train()` of the offline learner issues the multiset of entry-point calls of the same learner with
    `offline_loss=False`, the policy step's entry point renamed to its `_offline` sibling: as many launches, and no ATen
    fallback for the policy step"""
    hip = kw.get('hip', {})
    with_loss = _learner(plugin, hip=hip, seed=3)
    assert with_loss._stock_c_only()
    got = _calls(with_loss)
    with_loss.close()
    without = _learner(plugin, hip=hip, seed=3, offline_loss=False)
    want = _calls(without)
    without.close()
    old, new = sibling
    assert want[old] == 1 and old not in got and new not in want
    want[new] = want.pop(old)
    assert got == want, (sorted(got.items()), sorted(want.items()))
    # ... while the switch off takes the learner off the native policy step altogether
    eager = _learner(plugin, hip={**hip, 'fused_offline': False}, seed=3)
    assert not eager._stock_c_only()
    off = _calls(eager)
    eager.close()
    assert not any(k.startswith(('asac_policy_step_fused', 'asac_mlp_backward_policy_sample')) for k in off)


@pytest.mark.parametrize('plugin,kw,hidden', [('nn_vec', {}, (0,)),
                                              ('nn_rnn', dict(n_step=3, burn_in_step=3, seq_encoder='RNN'), (2, 8))])
def test_graph_replay_matches_eager(plugin, kw, hidden):
    """the pattern of tests/test_sac_step_gpu.py::test_graph_replay_matches_eager on the offline learner (stock networks on
    a fixed state: the action given; a trained GRU representation: the action sampled inside the launch): twin learners on
    device-drawn noise, one eager, one replaying its captured step after three warm-up steps — tree, parameters, written
    back probabilities and the logged objective equal bit for bit"""
    from algorithm.utils.enums import convert_config_to_enum
    kw = dict(kw)
    convert_config_to_enum(kw)
    episodes = _episodes(hidden=hidden)
    results = []
    for use_graph in (False, True):
        agent = _learner(plugin, use_graph=use_graph, hip=dict(graph_warmup=3), seed=3, **kw)
        assert agent._stock_c_only()
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        for _ in range(8):
            agent.train()
        assert (agent._graph is not None) == use_graph, 'the offline step must capture'
        agent._refresh_policy_stats()
        results.append((agent.replay_buffer._tree.clone(), agent._params.flat.clone(),
                        agent.replay_buffer._columns['mu_prob'].clone(), agent._stats['loss_policy'].clone()))
        assert len(agent._pi_stats_src) == 5, 'the payload carries the term\'s inputs'
        agent.close()
    for name, a, b in zip(('tree', 'parameters', 'mu_prob', 'loss_policy'), *results):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), name


def test_plain_gaussian_path_with_a_plugin_critic(golden_dir):
    """a non-stock critic (tests/plugins/nn_oc_small.py: 32 wide, two layers) with the stock policy: the autograd fast
    branch stays, the term's value and gradient come from `asac_policy_offline_term`; the policy gradient of the first
    step against float64 autograd on the learner's own modules, the logged objective with the term"""
    from asac_amd import native
    agent = _learner('nn_oc_small', seed=5)
    assert agent._fq is None and agent._fpi is not None and not agent._stock_c_only() and agent._offline_plain()
    for ep in _episodes():
        agent.put_episode(**ep)
    box, orig = {}, agent._train_policy

    def spy(obs_list, state, action, mu, ls=None):
        box.update(state=state.detach().clone(), stored=action.detach().clone(), pi=ref.double_copy(agent.model_policy),
                   qs=[ref.double_copy(q) for q in agent.model_q_list], log_alpha=agent.log_c_alpha.detach().clone())
        return orig(obs_list, state, action, mu, ls=ls)

    agent._train_policy = spy
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    torch.cuda.synchronize()
    assert len(prof.records['asac_policy_offline_term']) == 1 and len(prof.records['asac_policy_loss_fwd_bwd']) == 1
    E = agent.ensemble_q_num
    subset = None if agent.ensemble_q_sample == E else agent._subsets['pi_c'].cpu().tolist()
    want_obj, want = ref.policy_objective(box['pi'], box['qs'], box['state'], agent._eps_pi, box['stored'], box['log_alpha'],
                                          subset=subset)
    _, plain = ref.policy_objective(box['pi'], box['qs'], box['state'], agent._eps_pi, box['stored'], box['log_alpha'],
                                    subset=subset, offline=False)
    got = [m / 0.1 for m in pu.product_first_moments(agent)['optimizer_policy']]       # Adam's first moment, first step
    assert len(got) == len(want)
    err = max(scaled_error(a, b) for a, b in zip(got, want))
    fcheck('plain/grad', err)
    fcheck('plain/objective', scaled_error(agent._stats['loss_policy'], want_obj), gradient=False)
    assert max(scaled_error(p, w) for p, w in zip(plain, want)) >= 100. * enforced('plain/grad')
    agent.close()


def test_what_stays_on_the_eager_branch():
    """a hybrid space, a data-parallel context and an `OptionBase` with the offline loss construct, answer the predicate
    with no, and (hybrid) train on the eager branch as before"""
    from asac_amd import native
    from algorithm.oc import OptionBase
    hybrid = _learner(d_sizes=(3, 2), seed=0)
    assert not hybrid._offline_fused() and not hybrid._stock_c_only()
    for ep in _episodes(d_sizes=(3, 2)):
        hybrid.put_episode(**ep)
    with native.LaunchProfiler(repeat=1) as prof:
        assert hybrid.train() == 1
    assert not any(k.endswith('_offline') or k == 'asac_policy_offline_term' for k in prof.records)
    assert torch.isfinite(hybrid._params.flat).all()
    hybrid.close()
    plain = _learner(seed=0)
    assert plain._offline_fused() and plain._stock_c_only()
    plain._dist = object()              # (the predicate only: a data-parallel context in place)
    assert not plain._offline_fused() and not plain._stock_c_only() and not plain._offline_plain()
    plain._dist = None
    plain.close()
    opt = OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [], mog.C_ACTION_SIZE, None, pu.plugin('nn_oc'),
                     device='cuda:0', batch_size=16, summary_path=None, n_step=3, offline_enabled=True, offline_loss=True)
    assert opt._fq is not None and opt._fpi is not None, 'stock networks: only the learner\'s kind says no'
    assert not opt._offline_fused() and not opt._stock_c_only() and not opt._offline_plain()
    opt.close()
