"""GPU: the kernels over a categorical head (csrc/asac_categorical.h, asac_discrete_rows.h: discrete.hip, hybrid.hip,
dqn.hip) on the near side of their documented limits (include/asac_hip.h ASAC_DISCRETE_MAX_*, ASAC_MAX_ACTION), against
the float64 restatements of tests/discrete_ref.py, hybrid_ref.py and dqn_ref.py under the rule of
`discrete_ref.over_the_bound` (the bound of tests/test_discrete_gpu.py, unchanged).  The far side of every limit is
refused or falls back in those modules (`test_entry_points_refuse_bad_arguments`, `FALLBACKS`).  Every output of the
comparisons is a NaN-filled view between two bands of 64 sentinel floats whose bits must survive the launches
(`discrete_ref.Guarded`).

limit -> test id (each a float64 comparison of every entry point the limit applies to)

| limit | entry points | test id |
|---|---|---|
| D = 64, K = 8 | all | `test_return_corner[*-b8x8-*]`, `[*-uneven-*]`, `test_reduction_corner[*-b8x8-*]`, `[*-uneven-*]` |
| D = 64 in one branch | all | `test_return_corner[*-b64-*]`, `test_reduction_corner[*-b64-*]` |
| E = 8 (E_sample 8 and 5) | all | every id of `test_return_corner` and `test_reduction_corner` |
| n = 64 | `asac_discrete_return`, `asac_hybrid_return`, `asac_dqn_return`, `asac_dqn_q_loss_grad` | `test_return_corner[*-n64-*]` |
| B = 1024 (and 1023, 769) | the `*_q_loss_grad`, `*_policy_loss_grad`, `*_alpha_grad` entry points | `test_reduction_corner[*-B1024-*]`, `[*-B1023-*]`, `[*-B769-*]`, `test_saturated_logits_at_the_corner` |
| A = 64 | the `asac_hybrid_*` entry points | `test_return_corner[hybrid_a64-*]`, `test_reduction_corner[hybrid_a64-*]` |
| more than 64 KiB of LDS | `k_hybrid_return`, `k_discrete_return<false>` | `test_lds_ceiling_in_both_orders`, `test_return_corner[discrete-*-n64-*-is]`, `[hybrid_a*-*-n64-*-is]` at D = 64 |
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import discrete_ref as dr  # noqa: E402
from tests import dqn_ref as qr  # noqa: E402
from tests import hybrid_ref as hr  # noqa: E402
from tests import test_discrete_gpu as tdg  # noqa: E402
from tests import test_dqn_gpu as tqg  # noqa: E402
from tests import test_hybrid_gpu as thg  # noqa: E402

UNEVEN = (1, 2, 3, 5, 8, 13, 15, 17)        # K = 8, D = 64, a branch of size 1
TABLES = {'b8x8': (8,) * 8, 'b64': (64,), 'uneven': UNEVEN, 'ones': (1,) * 8}
ENSEMBLES = [(8, 8), (8, 5)]                # every slot of cat_member_mean live; a sampled subset past the 4-slot loads
# (B, n, branches): the window and width limits together, one row a workgroup at D = 64 (five workgroups); and one short
# of both, where Dp = D | 1 and pitch = (n + 1) | 1 take their other parity
WINDOWS = [(5, 64, sizes) for sizes in TABLES.values()] + [(3, 63, (63,))]
# a full last pass of the 256 lanes, one lane short of it, a partly filled fourth pass
ROWS = [1024, 1023, 769]
HEADS = ['discrete', 'hybrid_a64', 'hybrid_a1', 'dqn']


def _table_id(sizes):
    return next((k for k, v in TABLES.items() if v == sizes), 'b' + 'x'.join(map(str, sizes)))


def _case(head, B, n, sizes, E, Es, use_is, weights, seed):
    if head == 'discrete':
        return dr.make_case(B, n, sizes, E, Es, use_is, weights, seed)
    if head == 'dqn':
        return qr.make_case(B, n, sizes, E, Es, weights, seed)
    return hr.make_case(B, n, sizes, int(head[len('hybrid_a'):]), E, Es, use_is, weights, seed)


def _compare_guarded(head, tag, c):
    """the head's `_compare` with every output between sentinels -> the tensors over the bound"""
    guard = dr.Guarded()
    if head == 'discrete':
        bad = tdg._compare(tag, c, guard)
    elif head == 'dqn':
        bad = tqg._compare(tag, c, guard)[0]
    else:
        bad = thg._compare(tag, c, guard)
    guard.check()
    return bad


# ------------------------------------------------------------------------------------------------
def _return_only(head, dev):
    """the return launch alone on a device case -> {name: tensor} of its outputs (NaN-filled before)"""
    from asac_amd import native
    B, br = dev['B'], native.branches(dev['sizes'])
    nan = lambda: torch.full((B,), float('nan'), device='cuda')      # noqa: E731
    if head == 'discrete':
        out = {'y': nan(), 'td': nan()}
        native.discrete_return(tdg._vtrace_args(dev, out['y'], out['td']), br, dev['q_target'], dev['logits'],
                               action=dev['action'], q_online=dev['q_online'])
    else:
        out = {'d_y': nan(), 'c_y': nan(), 'td': nan()}
        native.hybrid_return(thg._d_args(dev, out['d_y']), thg._c_args(dev, out['c_y']), br, dev['q_target'], dev['logits'],
                             action=dev['action_full'], q_online=dev['q_online'], c_q_online=dev['c_q_online'],
                             td_out=out['td'])
    return out


@pytest.mark.parametrize('head', ['hybrid_a64', 'discrete'])
def test_lds_ceiling_in_both_orders(head):
    """`disc_return_geometry` raises a kernel's dynamic-LDS ceiling to 96 KiB once, behind a flag, when a workgroup needs
    more than 64 KiB: n = 64, D = 64 under importance sampling (86 784 B for `k_hybrid_return`, 86 224 B for
    `k_discrete_return<false>`).  A small launch (n 3, D 5), the corner, the small one again, the corner again — the flag's
    first and later uses, and a launch under 64 KiB after the ceiling was raised: all four against float64 under the
    bound, the two small results bit-equal and the two corner results bit-equal.  (First in this module: no launch of
    these kernels above 64 KiB comes before it in the process.)"""
    import asac_amd  # noqa: F401
    small = _case(head.replace('a64', 'a2'), 7, 3, (3, 2), 3, 2, True, True, seed=3)
    corner = _case(head, 5, 64, (64,), 8, 5, True, True, seed=4)
    results, bad = {}, []
    for i, (name, c) in enumerate([('small', small), ('corner', corner)] * 2):
        if head == 'discrete':
            want = dr.as_numpy(dr.ret(dr.to(c, torch.float64, 'cpu')))
            dev = dr.to(c, torch.float32, 'cuda', strided=True)
            eager = tdg._eager(dev)
        else:
            want = dr.as_numpy(hr.ret(hr.to(c, torch.float64, 'cpu')))
            dev = thg._device_case(c)
            eager = thg._eager(dev)
        got = _return_only(head, dev)
        torch.cuda.synchronize()
        eager = dr.as_numpy({k: eager[k] for k in want})
        bad += dr.over_the_bound(f'{head} launch {i} ({name})', want, dr.as_numpy(got), eager)[0]
        results.setdefault(name, []).append(got)
    for name, (first, second) in results.items():
        for k in first:
            assert torch.equal(first[k], second[k]), f'{name} {k}: the second launch differs from the first'
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# the DQN-like target has no importance sampling
RETURN_CASES = [(head, B, n, sizes, E, Es, use_is) for head in HEADS for B, n, sizes in WINDOWS for E, Es in ENSEMBLES
                for use_is in ((False,) if head == 'dqn' else (False, True))]


@pytest.mark.parametrize('head,B,n,sizes,E,Es,use_is', RETURN_CASES,
                         ids=[f'{h}-{_table_id(s)}-n{n}-{E}-{Es}-{"is" if i else "plain"}' for h, _, n, s, E, Es, i in RETURN_CASES])
def test_return_corner(head, B, n, sizes, E, Es, use_is):
    """The return entry points (`asac_discrete_return`, `asac_hybrid_return` with A = 64 and A = 1, `asac_dqn_return` and
    the target inside `asac_dqn_q_loss_grad`) at n = 64 with every branch table of the width limit and eight members, with
    and without importance sampling, the TD error included; the planted rows of `make_case`, strided views, with and
    without IS weights.  The other launches of the head run on the same case."""
    import asac_amd  # noqa: F401
    bad = []
    for weights in (False, True):
        c = _case(head, B, n, sizes, E, Es, use_is, weights, seed=B + 7 * n + len(sizes) + E + Es)
        bad += _compare_guarded(head, f'{head} {(B, n, sizes)} E {E}/{Es} is={use_is} w={weights}', c)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E,Es', ENSEMBLES)
@pytest.mark.parametrize('sizes', list(TABLES.values()), ids=list(TABLES))
@pytest.mark.parametrize('B', ROWS, ids=[f'B{b}' for b in ROWS])
@pytest.mark.parametrize('head', ['discrete', 'hybrid_a64', 'dqn'])
def test_reduction_corner(head, B, sizes, E, Es):
    """The single-workgroup launches (`asac_discrete_q_loss_grad` / `_policy_loss_grad` / `_alpha_grad`, the three
    `asac_hybrid_*` ones with A = 64, `asac_dqn_q_loss_grad`) where every one of the 256 lanes walks four rows (a lane
    reuses its `DiscPolicyKeep` entries row after row, all eight of them at K = 8), with and without IS weights; n = 2,
    importance sampling on, so the return launches run on the same rows.

    What `[discrete-B769-uneven-8-5]` (and its hybrid twin, the same bits) showed: y of row 242 was off by 5.385e-07
    from float64 (the eager composition 1.309e-07, floor 4.859e-07: 1.11 of the bound).  The row's pi(stored action)
    is 2.9e-06, the sum of eight log-probabilities -12.8, where float32 steps are 9.5e-07, and exp turned the sum's
    rounding into a relative error of 1e-06 of an unclamped ratio of 0.97, times a TD term of -0.54.
    `disc_return_values` forms that sum in double now: 1.300e-07, 0.27 of the bound."""
    import asac_amd  # noqa: F401
    bad = []
    for weights in (False, True):
        c = _case(head, B, 2, sizes, E, Es, True, weights, seed=B + len(sizes) + E + Es)
        bad += _compare_guarded(head, f'{head} {(B, 2, sizes)} E {E}/{Es} w={weights}', c)
    assert not bad, bad


def test_shared_bits_at_the_row_limit():
    """the bit-sharing assertions of tests/test_discrete_gpu.py (p and the row entropy of the policy and the temperature
    launch) and tests/test_dqn_gpu.py (the loss launch's y and the return launch's) at B = 1024 with K = 8, D = 64"""
    tdg.test_policy_and_temperature_kernels_form_the_same_bits(1024, 2, UNEVEN)
    tqg.test_the_loss_launch_stores_the_bits_of_the_return_launch(1024, 2, UNEVEN, 8, 5)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('head', ['discrete', 'hybrid_a64'])
def test_saturated_logits_at_the_corner(head):
    """`discrete_ref.saturate` (logits 0 or -30 per entry: both sides of the 1e-8 clamp) on B = 1024, eight branches of
    eight, eight members; the precondition of tests/test_discrete_gpu.py on the inputs, in float64: every probability is
    above 1e-6 or below 1e-12 and both sides occur; same bound"""
    import asac_amd  # noqa: F401
    B, n, sizes = 1024, 2, TABLES['b8x8']
    c = dr.saturate(_case(head, B, n, sizes, 8, 8, True, True, seed=B + n), seed=n)
    probs = dr.clamp_sides((dr if head == 'discrete' else hr).to(c, torch.float64, 'cpu'))
    assert bool(((probs > 1e-6) | (probs < 1e-12)).all())
    assert bool((probs > 1e-6).any()) and bool((probs < 1e-12).any()), 'both sides of the clamp occur'
    bad = _compare_guarded(head, f'{head} saturated {(B, n, sizes)}', c)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [TABLES['ones'], UNEVEN], ids=['ones', 'uneven'])
def test_exact_facts_of_branches_of_size_one(sizes):
    """A branch of one entry has p = 1, log p = 0 and H = 0 whatever its logit.  Of those entries, in the discrete and in
    the hybrid policy launch: `grad_logits` is exactly 0; `probs_out` exactly 1 (the discrete launch; the hybrid one has no
    such output).  Their addend to the row entropy is exactly 0: with every branch of size one `row_entropy_out` and both
    launches' mean entropy are exactly 0; in the uneven table the row entropy (1/8) sum_k H_k, times 8 and divided by 7
    in float32 (both the kernel's divisions are correctly rounded), has the bits of a launch on the seven other branches
    alone, and the hybrid launch's mean entropy the bits of the discrete launch's.  B = 300: a lane's second row too."""
    import asac_amd  # noqa: F401
    from asac_amd import native
    B, E, Es = 300, 8, 5
    ones = [j for j, s in zip(np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes) if s == 1]
    assert ones
    c = thg._device_case(hr.make_case(B, 2, sizes, 3, E, Es, True, True, seed=11))
    d_out, h_out = tdg._kernels(c), thg._kernels(c)
    torch.cuda.synchronize()
    for name, grad in (('discrete', d_out['grad_logits']), ('hybrid', h_out['grad_logits'])):
        assert torch.isfinite(grad).all() and bool((grad[:, ones] == 0.).all()), f'{name}: grad_logits of a size-1 branch'
    assert bool((d_out['p'][:, ones] == 1.).all())
    assert torch.equal(h_out['d_entropy'].reshape(1), d_out['d_entropy'].reshape(1))
    if all(s == 1 for s in sizes):
        assert bool((d_out['h_pi'] == 0.).all()) and float(d_out['d_entropy']) == 0. and float(h_out['d_entropy']) == 0.
        return
    assert ones == [0] and len(sizes) == 8
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')      # noqa: E731
    h_rest = nan(B)
    native.discrete_policy_loss_grad(native.branches(sizes[1:]), c['logits0'][:, 1:], [q[:, 1:] for q in c['q_online']],
                                     c['sub_pi'], Es, c['mu0'][:, 1:], c['log_alpha'], c['penalty'], nan(1),
                                     nan(B, c['D'] - 1), nan(1), None, h_rest)
    with_one = d_out['h_pi'].cpu().numpy() * np.float32(8.) / np.float32(7.)
    assert with_one.dtype == np.float32 and bool((with_one > 0.).all())
    assert np.array_equal(with_one, h_rest.cpu().numpy())


# ------------------------------------------------------------------------------------------------
# the step
# ------------------------------------------------------------------------------------------------
def _observables(agent, names):
    rb = agent.replay_buffer
    get = {'loss_q': lambda: agent._stats['loss_q'].item(), 'loss_policy': lambda: agent._stats['loss_policy'].item(),
           'd_entropy': lambda: agent._stats['d_entropy'].item(), 'c_entropy': lambda: agent._stats['c_entropy'].item(),
           'td_error': lambda: agent._td_error.cpu().numpy()[:, None], 'tree': lambda: rb._tree.cpu().numpy(),
           'log_d_alpha': lambda: agent.log_d_alpha.item(), 'log_c_alpha': lambda: agent.log_c_alpha.item()}
    return {name: np.asarray(get[name](), dtype=np.float64) for name in names}


LEARNERS = {
    'discrete': dict(c=0, dqn_like=False, flag='fused_discrete', module=tdg, calls=tdg._discrete_calls),
    'hybrid': dict(c=2, dqn_like=False, flag='fused_hybrid', module=thg, calls=thg._hybrid_calls),
    'dqn': dict(c=0, dqn_like=True, flag='fused_dqn', module=tqg, calls=tqg._calls),
}


@pytest.mark.parametrize('sizes', [TABLES['b8x8'], TABLES['b64']], ids=['b8x8', 'b64'])
@pytest.mark.parametrize('kind', list(LEARNERS))
def test_the_learner_takes_the_path_at_the_limit(kind, sizes):
    """the counterpart of the modules' `FALLBACKS` (`width_65`, `nine_branches`): a learner with 64 logits in eight
    branches or in one and eight critics, five of them sampled, issues with its switch on exactly the launches
    `test_one_step_issues_one_launch_per_item` counts and with it off none of them; one step of the two leaves the same
    observables under the module's `OBSERVABLES` bounds and the same first-step gradients (Adam's first moments) under
    the bound of its `assert_first_step_gradients` call: rtol 2e-3, plus 5e-5 of the tensor's largest entry, plus
    `ZERO_GRAD_REL` of the optimizer's largest gradient"""
    from asac_amd import native
    from tests import parity_utils as pu
    cfg = LEARNERS[kind]
    mod = cfg['module']
    episodes = tqg._episodes(sizes, cfg['c'])
    seen = {}
    for fused in (True, False):
        agent = tqg._plain_learner(sizes, cfg['c'], seed=3, hip={cfg['flag']: fused}, discrete_dqn_like=cfg['dqn_like'],
                                   ensemble_q_num=8, ensemble_q_sample=5)
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        with native.LaunchProfiler(repeat=1) as prof:
            assert agent.train() == 1
        assert cfg['calls'](prof.summary()) == (mod.ONE_STEP if fused else {}), cfg['calls'](prof.summary())
        assert torch.isfinite(agent._params.flat).all()
        moments = {name: [m.cpu().numpy().astype(np.float64) for m in views]
                   for name, views in pu.product_first_moments(agent).items()}
        seen[fused] = (_observables(agent, mod.OBSERVABLES), moments)
        agent.close()
    (obs_on, mom_on), (obs_off, mom_off) = seen[True], seen[False]
    for name, tol in mod.OBSERVABLES.items():
        err = float(np.abs(obs_on[name] - obs_off[name]).max())
        print(f'{kind} {sizes} {name}: switch on against off {err:.3e} at scale {float(np.abs(obs_off[name]).max()):.3e}')
        np.testing.assert_allclose(obs_on[name], obs_off[name], err_msg=name, **tol)
    assert set(mom_on) == set(mom_off) and any(np.abs(v).max() > 0. for views in mom_off.values() for v in views)
    for name, views in mom_off.items():
        scale = max(float(np.abs(v).max()) for v in views)      # (0 for the policy of a DQN-like learner: never trained)
        for j, (got, want) in enumerate(zip(mom_on[name], views)):
            atol = 5e-5 * float(np.abs(want).max()) + pu.ZERO_GRAD_REL * scale
            np.testing.assert_allclose(got, want, rtol=2e-3, atol=atol, err_msg=f'{name}/{j}')
