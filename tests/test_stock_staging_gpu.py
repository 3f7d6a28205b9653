"""GPU: the staging of the stock (fixed-shape) networks — `net_fetch_fixed` / `net_put_fixed` in csrc/mlp.hip request every
word once: the first layer's 64 x K0 matrix flat and scattered into its padded tile, the biases by the first 192 threads,
the head bias by the first 16; the loaded backwards leave the first layer, the biases and the head bias out.  Nothing a
launch computes may change, so every comparison here is `torch.equal`, against the GENERIC instantiations of the same
entry points (`net_fetch` / `net_put`, which the change does not touch), reached as tests/test_backward_chain_gpu.py reaches
them: the same parameters at an address that is not 16-byte aligned.

First-layer widths K0 = in0 + in1: the edges of 64 K0 words against 256 / 512 / 1 024 threads (4 | 8 | 16 and their
neighbours), of `round4` (1, 3, 4, 5), one word (1) and the full tile (63, 64).  Rows: one, an exact tile, a one-row tail,
two tiles and a tail; the forward and the Q-loss backward also at 2 065 rows (the policy: 4 113), where they take 32-row
tiles on 512 threads.  Kernels covered: the
fixed-shape forward on four and eight waves, the policy-sample-Q forward (it hosts the critic rider), the Q-loss backward
(y given, return formed inside, forward loaded), the one-launch policy step (action given, sampled inside, policy forward
loaded) and the two riders.

A padding word of the first layer's tile that a launch leaves unwritten reads whatever the CU's LDS held.  Every case
therefore runs twice with launches in between that leave NON-ZERO words in those places on every CU: the same entry
points on decoy networks of 64 inputs whose every parameter is 7 (their first-layer tiles have no padding at all), over
enough rows for every CU."""
import pytest
import torch

from tests.test_policy_forward_rider_gpu import _loss_partials, _ret_args, _slabs

pytestmark = pytest.mark.gpu

F = dict(device='cuda')
CLIP = 0.2
WIDTHS = [1, 3, 4, 5, 8, 15, 16, 17, 33, 63, 64]
ROWS = [1, 16, 17, 40]
HEADS = [(1, 2), (2, 3), (4, 2)]                  # (A, E)


def _pair(S, A, residual, policy, E=2, seed=7):
    """(the stock kernels' StockMLP, its misaligned twin on the same numbers: the generic kernels)"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_mlp import StockMLP, describe_policy, describe_q
    torch.manual_seed(seed)
    mods = [m.ModelPolicy(S, [], A).cuda()] if policy else [m.ModelQ(S, [], A, False).cuda() for _ in range(E)]
    desc = describe_policy(mods[0]) if policy else describe_q(mods[0])
    assert desc is not None
    with torch.no_grad():
        for mod in mods:
            for p in mod.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.3)
    for l in (1, 2):
        desc.residual[l] = int(residual)
    group = FlatParamGroup([(f'm{i}', list(mod.parameters())) for i, mod in enumerate(mods)], 'cuda')
    stride = group.segments['m0'][1] - group.segments['m0'][0]
    n, dev = len(mods), torch.device('cuda')
    mlp = StockMLP(desc, group.flat, group.grad, 0, stride, n, dev)
    flat1 = torch.zeros(1 + n * stride, **F)
    flat1[1:] = group.flat[:n * stride]
    twin = StockMLP(desc, flat1, torch.zeros_like(flat1), 1, stride, n, dev)
    assert mlp.params.data_ptr() % 16 == 0 and twin.params.data_ptr() % 16 == 4
    mlp.accumulate = twin.accumulate = False
    return mlp, twin


_decoys = {}


def _soil_lds():
    """non-zero words into the LDS of every CU, where the staged networks lie: the forward, the Q-loss backward and the
    policy step of networks on 64 inputs whose parameters are all 7 (results: whatever; nobody reads them)"""
    from asac_amd import native as nat
    if not _decoys:
        A = 2
        fq, _ = _pair(64 - A, A, True, policy=False, seed=1)
        fpi, _ = _pair(64 - A, A, True, policy=True, seed=1)
        with torch.no_grad():
            fq.params.fill_(7.)
            fpi.params.fill_(7.)
        N = 16 * torch.cuda.get_device_properties(0).multi_processor_count
        _decoys.update(fq=fq, fpi=fpi, N=N, x=torch.ones(N, 64 - A, **F), a=torch.ones(N, A, **F), eps=torch.ones(N, A, **F),
                       tq=torch.ones(2, N, **F), y=torch.ones(N, **F), loss=torch.zeros(2, **F),
                       la=torch.tensor(0., **F))
    d = _decoys
    d['fq']._launch_forward(d['x'], d['a'])
    d['fpi']._launch_forward(d['x'], None)
    d['fq'].backward_qloss(d['x'], d['a'], d['tq'], d['y'], None, CLIP, d['loss'], defer=True, state_grads=True)
    r, keep = _ret_args(nat, d['N'], 1, 2, 2, d['y'].clone())
    d['fq'].backward_qloss_return(d['x'], d['a'], d['tq'], r, None, CLIP, d['loss'], defer=True)
    d['fpi'].policy_step_fused(d['fq'], d['x'], d['a'], d['eps'], d['la'], defer=True)
    torch.cuda.synchronize()


def _twice(run):
    """`run()` -> a tuple of tensors / None; executed twice with the decoys in between and in front: equal, and returned"""
    _soil_lds()
    first = run()
    _soil_lds()
    second = run()
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b), 'two launches of one case differ'
    return first


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            continue
        if g.dim() == 3 and g.shape == w.shape and i == 0:      # partial slabs: tile by tile
            for t in range(g.shape[0]):
                assert torch.equal(g[t], w[t]), f'{what}: output {i}, tile {t}'
        else:
            assert torch.equal(g, w), f'{what}: output {i}'


# ---- the forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('K0', WIDTHS)
def test_fixed_shape_forward_is_the_generic_forward(K0, residual):
    nets = [(_pair(K0, 2, residual, policy=True), K0, 0)]
    nets += [(_pair(K0 - A, A, residual, policy=False, E=E), K0 - A, A) for A, E in HEADS if K0 > A]
    for (mlp, twin), S, A in nets:
        for N in ROWS + [2065 if A else 4113]:            # (32-row tiles: more than 256 (tile, member) pairs)
            torch.manual_seed(N + K0)
            x = torch.randn(N, 2, S, **F)[:, 1]                  # strided rows
            a = torch.randn(N, A, **F).tanh() if A else None
            want = twin._launch_forward(x, a)
            want = want if isinstance(want, (tuple, list)) else (want,)
            assert all(torch.isfinite(w).all() for w in want)

            def run():
                out = mlp._launch_forward(x, a)
                torch.cuda.synchronize()
                return tuple(o.clone() for o in (out if isinstance(out, (tuple, list)) else (out,)))
            _same(_twice(run), want, f'forward, in0 {S}, in1 {A}, E {mlp.E}, N {N}')


# ---- the Q-loss backward ------------------------------------------------------------------------------------------------
def _subset3(r, keep, E):
    if E == 3:                       # a device subset for the return: the two members its minimum is taken over
        keep['sn'] = torch.tensor([2, 0], dtype=torch.int32, device='cuda')
        keep['sx'] = torch.tensor([1, 2], dtype=torch.int32, device='cuda')
        r.subset_n, r.subset_next = keep['sn'].data_ptr(), keep['sx'].data_ptr()


@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('K0', WIDTHS)
def test_q_loss_backwards_are_the_generic_backward(K0, residual):
    from asac_amd import native as nat
    from tests.test_critic_forward_rider_gpu import _forward
    n = 4
    for A, E in HEADS:
        S = K0 - A
        if S < 1:
            continue
        fq, twin = _pair(S, A, residual, policy=False, E=E)
        ftq, ttq = _pair(S, A, residual, policy=False, E=E, seed=8)
        fpi, tpi = _pair(S, A, residual, policy=True)
        for N in ROWS + [2065]:                          # (2 065 rows: the four-wave form on 32-row tiles; nothing is loaded there)
            torch.manual_seed(100 * N + K0)
            x, a = torch.randn(N, 3, S, **F)[:, 1], torch.randn(N, A, **F).tanh()
            tq, w = torch.randn(E, N, **F) * 0.3, torch.rand(N, **F) + 0.5
            eps = torch.randn(N, A, **F)
            y = torch.zeros(N, **F)
            r, keep = _ret_args(nat, N, n, A, E, y)
            _subset3(r, keep, E)
            nat.vtrace_return_min(r)                      # the return launch: y for the yardstick
            loss = torch.zeros(E, **F)

            def backward(mlp, form, saved=None):
                def run():
                    mlp._workspace_for(N).fill_(float('nan'))
                    y_in = y
                    if form == 'plain':
                        g0 = mlp.backward_qloss(x, a, tq, y, w, CLIP, loss, defer=True, state_grads=True)
                    else:
                        y_in = torch.full((N,), float('nan'), **F)
                        r_in, keep_in = _ret_args(nat, N, n, A, E, y_in)
                        _subset3(r_in, keep_in, E)
                        assert mlp.backward_qloss_return_ok(N, r_in)
                        if saved is not None:
                            assert mlp.backward_qloss_return_loaded_ok(N, r_in, saved)
                        g0 = mlp.backward_qloss_return(x, a, tq, r_in, w, CLIP, loss, defer=True,
                                                       state_grads=saved is None, critic_saved=saved)
                    torch.cuda.synchronize()
                    out = (_slabs(mlp, N).clone(), _loss_partials(mlp, N).clone(), y_in.clone(), g0)
                    assert all(o is None or torch.isfinite(o).all() for o in out), 'a live output word was not written'
                    return out
                return run

            want = backward(twin, 'plain')()
            what = f'in0 {S}, in1 {A}, E {E}, N {N}'
            _same(_twice(backward(fq, 'plain')), want, 'y given, ' + what)
            _same(_twice(backward(fq, 'return')), want, 'return inside, ' + what)
            if N > 2048:
                continue
            # the first network launch with the critic rider (k_pi_sample_q stages three networks itself), then the
            # backward that loads what it saved
            save = fq.critic_save_buffer(N)
            plain_f = _forward(nat, fpi, ftq, fq, x, x, a, eps, 1)
            save.fill_(float('nan'))
            _soil_lds()
            got_f = _forward(nat, fpi, ftq, fq, x, x, a, eps, 1, save=save)
            for k, v in plain_f.items():
                assert torch.equal(got_f[k], v), f'hosting launch {k}, ' + what
            assert torch.isfinite(save).all()
            assert torch.equal(plain_f['x'], ttq._launch_forward(x, a)), 'stored pair job, ' + what
            assert torch.equal(plain_f['ls'].reshape(N, -1), tpi._launch_forward(x, None)[0]), 'policy of the hosting launch, ' + what
            _same(_twice(backward(fq, 'return', saved=save)), want[:3] + (None,), 'forward loaded, ' + what)


# ---- the policy step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('K0', WIDTHS)
def test_policy_steps_are_the_generic_chain(K0, residual):
    from asac_amd import native as nat
    n = 4
    for A, E in HEADS:
        S = K0 - A
        if S < 1:
            continue
        fq, tq_ = _pair(S, A, residual, policy=False, E=E)
        fpi, tpi = _pair(S, A, residual, policy=True)
        sub = torch.tensor([2, 0], dtype=torch.int32, device='cuda') if E == 3 else None
        for N in ROWS:
            torch.manual_seed(100 * N + K0 + 1)
            x = torch.randn(N, 3, S, **F)[:, 1]
            eps = torch.randn(N, A, **F)
            log_alpha = torch.tensor(-0.7, **F)
            what = f'in0 {S}, A {A}, E {E}, N {N}'
            # ---- the yardstick: generic forward, sampling launch, generic backwards
            ls = tpi._launch_forward(x, None)[0]
            a, logp = torch.empty(N, A, **F), torch.empty(N, **F)
            nat.squash_sample_fwd(ls[:, :A], ls[:, A:], eps, a, logp)
            q = tq_._launch_forward(x, a)
            ga = tq_.backward_policy_q(x, a, q.view(E, N), sub, 2)
            tpi._workspace_for(N).fill_(float('nan'))
            tpi.backward_policy_sample(x, eps, ga, log_alpha, defer=True)
            torch.cuda.synchronize()
            want_s = _slabs(tpi, N).clone()
            assert torch.isfinite(want_s).all()
            members = [2, 0] if E == 3 else [0, 1]
            assert fpi.policy_step_fused_ok(fq, N)
            # ---- the saved policy forward: the rider of the Q-loss backward launch
            save = fpi.forward_save_buffer(N)
            save.fill_(float('nan'))
            y = torch.zeros(N, **F)
            r, keep = _ret_args(nat, N, n, A, E, y)
            if E == 3:
                keep['sn'] = torch.tensor([2, 0], dtype=torch.int32, device='cuda')
                keep['sx'] = torch.tensor([1, 2], dtype=torch.int32, device='cuda')
                r.subset_n, r.subset_next = keep['sn'].data_ptr(), keep['sx'].data_ptr()
            a0, tq, w = torch.randn(N, A, **F).tanh(), torch.randn(E, N, **F) * 0.3, torch.rand(N, **F) + 0.5
            assert fq.backward_qloss_return_rider_ok(N, r, fpi, x, save)
            _soil_lds()
            fq.backward_qloss_return_rider(x, a0, tq, r, w, CLIP, torch.zeros(E, **F), fpi, x, save, defer=True)
            torch.cuda.synchronize()
            assert torch.isfinite(save).all()

            def step(form):
                def run():
                    q_out = torch.full((E, N, 1), -7.0, **F)
                    out = (torch.zeros(N, A, **F), torch.zeros(N, **F), torch.zeros(N, 2 * A, **F))
                    fpi._workspace_for(N).fill_(float('nan'))
                    if form == 'loaded':
                        fpi.policy_step_fused_loaded(fq, x, a, eps, log_alpha, save, q_out=q_out, defer=True, subset=sub)
                    else:
                        fpi.policy_step_fused(fq, x, None if form == 'sampled' else a, eps, log_alpha, q_out=q_out,
                                              defer=True, subset=sub, sample_out=out if form == 'sampled' else None)
                    torch.cuda.synchronize()
                    return (_slabs(fpi, N).clone(), q_out) + (out if form == 'sampled' else ())
                return run

            for form in ('given', 'sampled', 'loaded'):
                got = _twice(step(form))
                _same(got[:1], (want_s,), f'{form}: partial slabs, ' + what)
                for m in members:
                    assert torch.equal(got[1][m], q.view(E, N, 1)[m]), f'{form}: value table of member {m}, ' + what
                if form == 'sampled':
                    assert torch.equal(got[2], a) and torch.equal(got[3], logp) and torch.equal(got[4], ls), what
