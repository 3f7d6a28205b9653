"""GPU: the wave roles of `asac_policy_sample_q_forward` in a workgroup that runs one tile.  Waves 0..3 form the action and
go on into the critic's layers; waves 4..6 form the side outputs (the main sample's log-probability, the stored actions'
probabilities, the second sample) beside them; a wave without a job retires.  Nothing changes a value: every case
compares the one launch with the chain policy forward -> `squash_multi` -> critics forward through `torch.equal` on every
output.  The shapes sit on the edges of the roles — one live row, a last partial tile, a second workgroup with one live
row, two items per lane (A = 8), writer and non-writer workgroups (E > 1), every subset of the side jobs — not on size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_fused_mlp_gpu import _setup  # noqa: E402

S = 6
SHAPES = [(1, 1), (3, 5), (16, 1), (17, 1), (7, 5)]      # (B, T): rows N = B T = 1, 15, 16, 17, 35
SIDES = ['none', 'stored', 'second@0', 'second@last', 'both']
_NETS = {}


def _nets(E, A):
    """-> (policy, critics): built once per (E, A) and left unchanged"""
    if (E, A) not in _NETS:
        _NETS[(E, A)] = (_setup(1, S, A, policy=True)[2], _setup(E, S, A)[2])
    return _NETS[(E, A)]


def _side(side, T):
    """-> (stored actions scored, second sample drawn, its window row)"""
    return side in ('stored', 'both'), side.startswith('second') or side == 'both', 0 if side == 'second@0' else T - 1


def _buffers(B, T, A):
    f = dict(device='cuda')
    return dict(a=torch.full((B, T, A), 7., **f), logp=torch.full((B, T), 7., **f), pr=torch.zeros(B, T, A, **f),
                a2=torch.full((B, A), 7., **f), logp2=torch.full((B,), 7., **f))


def _chain(native, fpi, fq, xs, B, T, A, eps, eps2, stored, side, extra=None):
    """policy forward -> squash_multi -> critics forward (+ the plain job on its own)"""
    with_stored, with_second, t2 = _side(side, T)
    N = B * T
    ls = fpi._launch_forward(xs, None)[0].view(B, T, 2 * A)
    o = _buffers(B, T, A)
    jobs = [native.squash_job(ls[..., :A], ls[..., A:], eps, o['a'], o['logp'], stored if with_stored else None, 1,
                              o['pr'] if with_stored else None, 0)]
    if with_second:
        jobs.append(native.squash_job(ls[:, t2, :A], ls[:, t2, A:], eps2, o['a2'], o['logp2']))
    native.squash_multi(jobs)
    o['ls'] = ls.clone()
    o['q'] = fq._launch_forward(xs, o['a'].view(N, A))
    if extra is not None:
        o['x'] = fq._launch_forward(*extra)
    return o


def _one_launch(native, fpi, fq, xs, B, T, A, eps, eps2, stored, side, extra=None, ring=None, sidecars=None, out=None):
    with_stored, with_second, t2 = _side(side, T)
    N = B * T
    o = out if out is not None else _buffers(B, T, A)
    job_pi, ls = fpi.job(xs, None)
    job_q, o['q'] = fq.job(xs, o['a'].view(N, A))
    extras = []
    if extra is not None:
        job_x, o['x'] = fq.job(*extra)
        extras.append(job_x)
    kw = {}
    if with_stored:
        kw.update(action=stored, action_offset=1, prob_out=o['pr'])
    if with_second:
        kw.update(eps2=eps2, t2=t2, a2_out=o['a2'], logp2_out=o['logp2'])
    job = native.pi_q_job(job_pi, job_q, eps, o['a'], o['logp'], T, **kw)
    if ring is not None:
        job = native.pi_q_ring_rows(job, **ring)
    assert native.policy_sample_q_forward_ok(job, extras)
    native.policy_sample_q_forward(job, extras, sidecars=sidecars)
    o['ls'] = ls[0].view(B, T, 2 * A)
    return o


def _same(got, want, what):
    # (outputs a case does not ask for keep their fill value on both sides: a stray store shows)
    for k, v in want.items():
        assert torch.equal(got[k], v), (what, k)


def _inputs(B, T, A, window, seed):
    from asac_amd import native
    torch.manual_seed(seed)
    N = B * T
    if window:      # [B, T, S] view of a longer window, read in place
        base = torch.randn(B, T + 2, S, device='cuda')
        xs = native.WindowRows(base[:, 2:])
    else:
        xs = torch.randn(N, S, device='cuda')
    eps, eps2 = torch.randn(N, A, device='cuda'), torch.randn(B, A, device='cuda')
    stored = torch.rand(B, T, A + 1, device='cuda') * 1.9 - 0.95       # stored actions behind one discrete column
    return xs, eps, eps2, stored


@pytest.mark.parametrize('E', [1, 2, 3])
@pytest.mark.parametrize('A', [1, 2, 8])
def test_single_tile_workgroups_equal_the_chain(A, E):
    """plain rows: every shape x every subset of the side jobs (A = 8: 128 items a tile, two per lane; E > 1: the
    non-writer workgroups form the action for their critic and store no side output)"""
    from asac_amd import native
    fpi, fq = _nets(E, A)
    for B, T in SHAPES:
        xs, eps, eps2, stored = _inputs(B, T, A, False, 100 * B + T)
        for side in SIDES:
            want = _chain(native, fpi, fq, xs, B, T, A, eps, eps2, stored, side)
            got = _one_launch(native, fpi, fq, xs, B, T, A, eps, eps2, stored, side)
            _same(got, want, (B, T, side))


@pytest.mark.parametrize('A,E', [(1, 2), (2, 1), (8, 3)])
def test_window_rows_equal_the_chain(A, E):
    from asac_amd import native
    fpi, fq = _nets(E, A)
    for B, T in [(3, 5), (7, 5), (17, 1)]:
        xs, eps, eps2, stored = _inputs(B, T, A, True, 200 * B + T)
        for side in ('none', 'both', 'second@0'):
            want = _chain(native, fpi, fq, xs, B, T, A, eps, eps2, stored, side)
            got = _one_launch(native, fpi, fq, xs, B, T, A, eps, eps2, stored, side)
            _same(got, want, (B, T, side))


# ---- ring-addressed rows ------------------------------------------------------------------------------------------------
C_RING, EPISODE, PREV_N, POST_N = 1024, 37, 2, 4
L_WIN = PREV_N + 1 + POST_N


def _ring(native, B, A, seed):
    """a full ring of capacity 1 024 with hand-placed ids: windows over the ring's end and its start, ids several wraps
    on, one from beyond 2^32 (long overwritten: only its slot counts), one on the last row of an episode (its later rows
    are padding) -> (gathered batch, specs, ring description)"""
    rng = np.random.default_rng(seed)
    obs_ring = torch.from_numpy(rng.standard_normal((C_RING, S)).astype(np.float32)).cuda()
    act_ring = torch.from_numpy(np.tanh(rng.standard_normal((C_RING, A))).astype(np.float32)).cuda()
    index_ring = torch.from_numpy((np.arange(C_RING) % EPISODE).astype(np.int32)).cuda()
    fixed = [C_RING - 2, 0, C_RING - 1, 3 * C_RING + 5, 2 ** 33 + 7, EPISODE - 1, 1]
    ids_h = np.concatenate([fixed, rng.integers(0, 4 * C_RING, max(B - len(fixed), 0))])[:B].astype(np.int64)
    ids = torch.from_numpy(ids_h).cuda()
    pad_row = torch.from_numpy(rng.uniform(-0.9, 0.9, A).astype(np.float32)).cuda()
    batch = dict(obs_vec=torch.zeros(B, L_WIN, S, device='cuda'), action=torch.zeros(B, L_WIN, A, device='cuda'))
    obs_spec = dict(src=obs_ring, dst=batch['obs_vec'], row_bytes=S * 4, pad_mode=native.PAD_KEEP)
    act_spec = dict(src=act_ring, dst=batch['action'], row_bytes=A * 4, pad_mode=native.PAD_ROW, pad_row=pad_row)
    specs = [obs_spec, act_spec]
    ring = dict(ids=ids, index_ring=index_ring, capacity=C_RING, prev_n=PREV_N, L=L_WIN, j0=PREV_N,
                x0_key=native.ring_key(obs_spec), action_key=native.ring_key(act_spec))
    return batch, specs, ring


def _ring_case(native, A, E, B, T, sides, rider=False):
    from algorithm.fused_mlp import StockMLP
    fpi, fq = _nets(E, A)
    batch, specs, ring = _ring(native, B, A, 7 * B + T)
    keys = native.make_gather_keys(specs)
    native.window_gather_pad(keys, ring['ids'], B, PREV_N, POST_N, C_RING, ring['index_ring'])
    torch.cuda.synchronize()
    want_batch = {k: v.clone() for k, v in batch.items()}
    obs, act = batch['obs_vec'][:, PREV_N:PREV_N + T], batch['action'][:, PREV_N:PREV_N + T]
    xs = StockMLP._rows_in_place(obs, S)
    torch.manual_seed(B + T)
    eps, eps2 = torch.randn(B * T, A, device='cuda'), torch.randn(B, A, device='cuda')

    def stored_chain(side):      # (the chain's stored actions sit behind one column, the ring's at offset 0)
        return torch.cat([torch.zeros(B, T, 1, device='cuda'), act], dim=2) if _side(side, T)[0] else None

    extra = (StockMLP._rows(obs[:, 0], S), StockMLP._rows(act[:, 0], A)) if rider else None
    wants = {side: _chain(native, fpi, fq, xs, B, T, A, eps, eps2, stored_chain(side), side, extra) for side in sides}
    torch.cuda.synchronize()
    for v in batch.values():       # nothing of the gathered batch is left for the ring-addressed launch to read
        v.fill_(float('nan'))
    for side in sides:
        with_stored, with_second, t2 = _side(side, T)
        o = _buffers(B, T, A)
        job_pi, ls = fpi.job(xs, None)
        job_q, o['q'] = fq.job(xs, o['a'].view(B * T, A))
        kw, extras, sidecars = {}, [], None
        if with_stored:
            kw.update(action=act, prob_out=o['pr'])
        if with_second:
            kw.update(eps2=eps2, t2=t2, a2_out=o['a2'], logp2_out=o['logp2'])
        job = native.pi_q_job(job_pi, job_q, eps, o['a'], o['logp'], T, **kw)
        r = dict(ring)
        if rider:       # a plain forward job reading its rows from the ring, and the batch's gather as a sidecar
            job_x, o['x'] = fq.job(*extra)
            extras, r['x_j0'] = [job_x], PREV_N
            sidecars = [native.sidecar_window_gather(keys, ring['ids'], B, PREV_N, POST_N, C_RING, ring['index_ring'])]
        job = native.pi_q_ring_rows(job, **r)
        assert native.policy_sample_q_forward_ok(job, extras)
        native.policy_sample_q_forward(job, extras, sidecars=sidecars)
        torch.cuda.synchronize()
        o['ls'] = ls[0].view(B, T, 2 * A)
        _same(o, wants[side], ('ring', B, T, side))
        if rider:
            for k, v in want_batch.items():
                assert torch.equal(batch[k], v), k
            for v in batch.values():
                v.fill_(float('nan'))


@pytest.mark.parametrize('A,E', [(1, 1), (2, 2), (8, 2), (2, 3)])
def test_ring_addressed_rows_equal_gather_then_chain(A, E):
    """`k_pi_sample_q_ring`: the stored actions wave 5 scores were requested by every wave at the head of the tile (two per
    lane at A = 8)"""
    from asac_amd import native
    for B, T in SHAPES:
        _ring_case(native, A, E, B, T, SIDES if (B, T) in ((3, 5), (17, 1)) else ('none', 'both'))


def test_riders_leave_beside_the_side_waves():
    """a plain forward job and a sidecar in the launch: their workgroups let waves 4..7 go at the kernel's entry, the fused
    job's workgroups retire the waves without a side job behind the policy head (all four in a non-writer workgroup) —
    plain rows and ring-addressed rows"""
    from asac_amd import native
    A, E, B, T = 2, 2, 17, 5
    _ring_case(native, A, E, B, T, ('both', 'stored'), rider=True)
    fpi, fq = _nets(E, A)
    xs, eps, eps2, stored = _inputs(B, T, A, False, 5)
    extra = (torch.randn(B, S, device='cuda'), torch.randn(B, A, device='cuda').tanh())
    want = _chain(native, fpi, fq, xs, B, T, A, eps, eps2, stored, 'both', extra)
    _same(_one_launch(native, fpi, fq, xs, B, T, A, eps, eps2, stored, 'both', extra), want, 'plain rider')


def test_looping_workgroups_keep_their_path():
    """E = 3: 85 tile groups a launch, so 86 tiles — N = 85 * 16 + 1 = 1 361 rows — is the smallest launch in which a
    workgroup (the first group's) takes a second tile: the launch runs the looping instantiation"""
    from asac_amd import native
    A, E, B, T = 2, 3, 1361, 1
    fpi, fq = _nets(E, A)
    xs, eps, eps2, stored = _inputs(B, T, A, False, 9)
    want = _chain(native, fpi, fq, xs, B, T, A, eps, eps2, stored, 'both')
    _same(_one_launch(native, fpi, fq, xs, B, T, A, eps, eps2, stored, 'both'), want, 'looping')
    # ... and one tile fewer: every workgroup on the single-tile path
    B = 1360
    xs, eps, eps2, stored = _inputs(B, T, A, False, 10)
    want = _chain(native, fpi, fq, xs, B, T, A, eps, eps2, stored, 'both')
    _same(_one_launch(native, fpi, fq, xs, B, T, A, eps, eps2, stored, 'both'), want, 'last single-tile size')


@pytest.mark.parametrize('A,E,B,T', [(2, 2, 7, 5), (8, 1, 17, 1)])
def test_back_to_back_launches_keep_their_own_outputs(A, E, B, T):
    """the same launch twice on one stream, into the same buffers, with different noise and no host synchronisation
    between them: a side wave of the first launch whose stores were still in flight at the kernel's end would overwrite
    the second's outputs"""
    from asac_amd import native
    fpi, fq = _nets(E, A)
    xs, eps_a, eps2_a, stored = _inputs(B, T, A, False, 11)
    eps_b, eps2_b = torch.randn_like(eps_a), torch.randn_like(eps2_a)
    want_a = _chain(native, fpi, fq, xs, B, T, A, eps_a, eps2_a, stored, 'both')
    want_b = _chain(native, fpi, fq, xs, B, T, A, eps_b, eps2_b, stored, 'both')
    assert not torch.equal(want_a['a'], want_b['a'])
    torch.cuda.synchronize()
    out = _buffers(B, T, A)
    first = _one_launch(native, fpi, fq, xs, B, T, A, eps_a, eps2_a, stored, 'both', out=out)
    got_a = {k: v.clone() for k, v in first.items() if k != 'q'}
    q_a = first['q']
    got_b = _one_launch(native, fpi, fq, xs, B, T, A, eps_b, eps2_b, stored, 'both', out=out)
    torch.cuda.synchronize()
    got_a['q'] = q_a
    _same(got_a, want_a, 'first launch')
    _same(got_b, want_b, 'second launch')
