"""GPU: ring slots by mask.  Every kernel that turns a row id into a ring slot — the window gather, the write-back
scatter, the ring-addressed first network launch, the TD-error / priority update — takes `id & (capacity - 1)` when the
capacity is a power of two and the signed 64-bit remainder otherwise.  The ids here are the ones at which the two forms,
or a wrong one, part: 0 and 1 (negative window neighbours), the ring's end, ids beyond one wrap and beyond 2^32.  The
expected values are NumPy restatements (`np.mod` on int64) or the stand-alone launches; every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_head_gather_gpu import A, S, _f32_bits, _launch, nets  # noqa: E402,F401
from tests.test_kernels_gpu import DevTree, _vtrace_args, nat  # noqa: E402,F401

CAPACITIES = [16, 1024, 24, 1000]        # mask, mask, generic, generic
PREV_N, POST_N, BATCH = 3, 4, 12
L = PREV_N + 1 + POST_N


def _ids(C, rng):
    """the ids the issue names, a duplicate, an overlapping window, the rest random over several wraps"""
    fixed = [0, 1, C - 1, C, 3 * C + 5, 2 ** 33 + 7, 3 * C + 5, 3 * C + 6]
    rest = rng.integers(0, 5 * C, BATCH - len(fixed))
    return np.array(fixed + list(rest), np.int64)


def _window_valid(ids, index, C):
    """-> slot [B, L], valid [B, L]: `asac_gather.h: index_run` — a window row belongs to the centre row's episode iff the
    stored step indexes run on from the centre's (the centre itself always)"""
    off = np.arange(L, dtype=np.int64) - PREV_N
    slot = np.mod(ids[:, None] + off[None, :], np.int64(C))
    idx_c = index[np.mod(ids, np.int64(C))].astype(np.int64)
    valid = (index[slot].astype(np.int64) - idx_c[:, None]) == off[None, :]
    valid[:, PREV_N] = True
    return slot, valid


@pytest.mark.parametrize('C', CAPACITIES)
def test_window_gather_slots_equal_numpy_mod(nat, C):
    rng = np.random.default_rng(C)
    ids = _ids(C, rng)
    index = (np.arange(C) % 5).astype(np.int32)               # episodes of 5 rows: every window crosses one
    rings = {'wide': rng.standard_normal((C, 8)).astype(np.float32),          # 32-byte rows: 16-byte units
             'words': rng.standard_normal((C, 6)).astype(np.float32),         # 24-byte rows: 4-byte units
             'bytes': rng.integers(0, 255, (C, 3)).astype(np.uint8)}          # 3-byte rows: 1-byte units
    pad_row = rng.standard_normal(8).astype(np.float32)
    pad_word, pad_byte = np.float32(-0.75), 0xAB
    slot, valid = _window_valid(ids, index, C)
    assert valid.any() and not valid.all() and valid[:, :PREV_N].any() and not valid[:, :PREV_N].all()
    want = {'wide': np.where(valid[..., None], rings['wide'][slot], pad_row),
            'words': np.where(valid[..., None], rings['words'][slot], pad_word),
            'bytes': np.where(valid[..., None], rings['bytes'][slot], np.uint8(pad_byte)),
            'mask': (~valid).astype(np.uint8)}

    d_ring = {k: torch.from_numpy(v).cuda() for k, v in rings.items()}
    d_pad_row = torch.from_numpy(pad_row).cuda()
    out = {k: torch.zeros((BATCH, L) + v.shape[1:], dtype=v.dtype, device='cuda') for k, v in d_ring.items()}
    out['mask'] = torch.full((BATCH, L), 7, dtype=torch.uint8, device='cuda')
    specs = [dict(src=d_ring['wide'], dst=out['wide'], row_bytes=32, pad_mode=nat.PAD_ROW, pad_row=d_pad_row),
             dict(src=d_ring['words'], dst=out['words'], row_bytes=24, pad_mode=nat.PAD_WORD, pad_word=_f32_bits(pad_word)),
             dict(src=d_ring['bytes'], dst=out['bytes'], row_bytes=3, pad_mode=nat.PAD_BYTE, pad_word=pad_byte),
             dict(src=None, dst=out['mask'], pad_mode=nat.PAD_EMIT_MASK)]
    keys = nat.make_gather_keys(specs)
    nat.window_gather_pad(keys, torch.from_numpy(ids).cuda(), BATCH, PREV_N, POST_N, C, torch.from_numpy(index).cuda())
    torch.cuda.synchronize()
    for k, w in want.items():
        got = out[k].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(w.astype(got.dtype)).view(np.uint8)), k


@pytest.mark.parametrize('C', CAPACITIES)
def test_scatter_rows_slots_equal_numpy_mod(nat, C):
    rng = np.random.default_rng(100 + C)
    ids = _ids(C, rng)
    count, first_off, W = PREV_N + POST_N, -PREV_N, 4
    tgt = ids[:, None] + first_off + np.arange(count, dtype=np.int64)[None, :]         # [B, count], negative for ids 0, 1
    slot = np.mod(tgt, np.int64(C))
    # the id map: every slot holds one of the ids aimed at it (the first in row-major order), so that other ids aimed at
    # the same slot — a wrap earlier or later — must be refused; one slot is stale for everybody
    slot_ids = np.full(C, -(2 ** 40), np.int64)
    for t, s in zip(tgt.reshape(-1)[::-1], slot.reshape(-1)[::-1]):
        slot_ids[s] = t
    stale = slot[4, 2]
    slot_ids[stale] += C
    pad = rng.random((BATCH, count + 1)) < 0.2
    new = rng.standard_normal((BATCH, count, W)).astype(np.float32)
    ring = rng.standard_normal((C, W)).astype(np.float32)
    want = ring.copy()
    written = 0
    for s in range(BATCH):                                    # row-major order: the last writer wins
        for j in range(count):
            if not pad[s, j] and slot_ids[slot[s, j]] == tgt[s, j]:
                want[slot[s, j]] = new[s, j]
                written += 1
    assert written > 0 and np.array_equal(want[stale], ring[stale])
    d_ring = torch.from_numpy(ring).cuda()
    winner = torch.full((C,), -1, dtype=torch.int32, device='cuda')
    nat.scatter_rows_if_id_match(d_ring, W * 4, C, torch.from_numpy(ids).cuda(), BATCH, first_off, count,
                                 torch.from_numpy(slot_ids).cuda(), torch.from_numpy(pad).cuda(), count + 1,
                                 torch.from_numpy(new).cuda(), count * W * 4, W * 4, winner)
    torch.cuda.synchronize()
    assert np.array_equal(d_ring.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert bool((winner == -1).all())


# ---- the ring-addressed first network launch -------------------------------------------------------------------------
C_SMALL, EPISODE = 64, 37


def _small_ring(batch, prev_n, post_n):
    import asac_amd  # noqa: F401
    from algorithm.replay_buffer import PrioritizedReplayBuffer
    gen = np.random.default_rng(0)
    n = C_SMALL         # a full ring
    data = dict(index=(np.arange(n) % EPISODE).astype(np.int32), obs_vec=gen.standard_normal((n, S)).astype(np.float32),
                action=np.tanh(gen.standard_normal((n, A))).astype(np.float32),
                reward=gen.standard_normal(n).astype(np.float32), done=np.zeros(n, bool), last_mask=np.zeros(n, bool),
                mu_prob=np.ones((n, A), np.float32), pre_seq_hidden_state=gen.standard_normal((n, 2)).astype(np.float32))
    rb = PrioritizedReplayBuffer(batch_size=batch, capacity=C_SMALL, sample_prev_n=prev_n, sample_post_n=post_n, device='cuda')
    rb.set_window_padding(torch.tensor([0.25, -0.5, 0.75]))
    rb.add(data)
    rb.sample()
    # the first id (burn-in rows before slot 0), the ring's last slot (the window continues at slot 0), ids beyond one
    # and several wraps, one past 2^32
    rb._ids[:6] = torch.tensor([0, C_SMALL - 1, C_SMALL + 20, 3 * C_SMALL + 5, 1, 2 ** 33 + 7], device='cuda')
    return rb


def test_ring_addressed_launch_at_the_ring_ends_equals_gather_then_launch(nets):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused_mlp import StockMLP
    B, prev_n, post_n, T = 16, 2, 4, 5                     # n-step 4: five rows from the centre on
    rb = _small_ring(B, prev_n, post_n)
    batch, specs = rb._window_specs(B)
    obs_spec = next(s for s in specs if s.get('dst') is batch['obs_vec'])
    act_spec = next(s for s in specs if s.get('dst') is batch['action'])
    keys = native.make_gather_keys(specs)
    ids, index_ring = rb._ids, rb._index_ring()
    eps, eps2 = torch.randn(B * T, A, device='cuda'), torch.randn(B, A, device='cuda')

    native.window_gather_pad(keys, ids, B, prev_n, post_n, C_SMALL, index_ring)
    torch.cuda.synchronize()
    assert bool(batch['padding_mask'].any()) and not bool(batch['padding_mask'].all())
    want_batch = {k: v.clone() for k, v in batch.items()}
    want = _launch(native, StockMLP, nets, batch, B, T, prev_n, eps, eps2)

    for v in batch.values():
        v.fill_(float('nan')) if v.is_floating_point() else v.zero_()
    rider = native.sidecar_window_gather(keys, ids, B, prev_n, post_n, C_SMALL, index_ring)
    ring = dict(ids=ids, index_ring=index_ring, capacity=C_SMALL, prev_n=prev_n, L=prev_n + 1 + post_n, j0=prev_n,
                x0_key=native.ring_key(obs_spec), action_key=native.ring_key(act_spec))
    got = _launch(native, StockMLP, nets, batch, B, T, prev_n, eps, eps2, ring=ring, sidecars=[rider])
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for k, v in want_batch.items():
        assert torch.equal(batch[k], v), k


def test_ring_form_is_refused_for_a_capacity_that_is_no_power_of_two(nets):
    """capacity 1 000: `policy_sample_q_forward_ok` says no (what SAC_Base._head_ring_job asks: it then returns None and
    the step keeps the stand-alone gather), the launch itself refuses, and the fallback — the gather at that capacity,
    then the plain launch on the gathered batch — runs and delivers the rows NumPy's `%` picks."""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused_mlp import StockMLP
    fpi, ftq = nets
    C, B, prev_n, post_n, T = 1000, 16, 2, 4, 5
    Lw = prev_n + 1 + post_n
    rng = np.random.default_rng(3)
    obs_ring = torch.from_numpy(rng.standard_normal((C, S)).astype(np.float32)).cuda()
    act_ring = torch.from_numpy(np.tanh(rng.standard_normal((C, A))).astype(np.float32)).cuda()
    index = (np.arange(C) % EPISODE).astype(np.int32)
    index_ring = torch.from_numpy(index).cuda()
    ids_h = np.concatenate([[0, C - 1, C + 20, 3 * C + 5, 1, 2 ** 33 + 7], rng.integers(0, 4 * C, B - 6)]).astype(np.int64)
    ids = torch.from_numpy(ids_h).cuda()
    pad_row = torch.tensor([0.25, -0.5, 0.75], device='cuda')
    batch = dict(obs_vec=torch.zeros(B, Lw, S, device='cuda'), action=torch.zeros(B, Lw, A, device='cuda'))
    obs_spec = dict(src=obs_ring, dst=batch['obs_vec'], row_bytes=S * 4, pad_mode=native.PAD_KEEP)
    act_spec = dict(src=act_ring, dst=batch['action'], row_bytes=A * 4, pad_mode=native.PAD_ROW, pad_row=pad_row)

    f32 = dict(dtype=torch.float32, device='cuda')
    obs, act = batch['obs_vec'][:, prev_n:], batch['action'][:, prev_n:]
    rows = StockMLP._rows_in_place(obs, S)
    job_pi, _ = fpi.job(rows, None)
    a_y, logp_y, c_pi = torch.zeros((B, T, A), **f32), torch.zeros((B, T), **f32), torch.zeros((B, T, A), **f32)
    job_q, _ = ftq.job(rows, a_y.view(-1, A))
    job_tq, _ = ftq.job(StockMLP._rows(obs[:, 0], S), StockMLP._rows(act[:, 0], A))
    eps = torch.randn(B * T, A, device='cuda')
    fused = native.pi_q_job(job_pi, job_q, eps, a_y, logp_y, T, action=act, prob_out=c_pi)
    ring = dict(ids=ids, index_ring=index_ring, prev_n=prev_n, L=Lw, j0=prev_n, x0_key=native.ring_key(obs_spec),
                action_key=native.ring_key(act_spec), x_j0=prev_n)
    assert native.policy_sample_q_forward_ok(fused, [job_tq])
    assert native.policy_sample_q_forward_ok(native.pi_q_ring_rows(fused, capacity=1024, **ring), [job_tq])
    refused = native.pi_q_ring_rows(fused, capacity=C, **ring)
    assert not native.policy_sample_q_forward_ok(refused, [job_tq])
    assert not native.policy_sample_q_forward_ok(refused)
    with pytest.raises(native.AsacNativeError):
        native.policy_sample_q_forward(refused, [job_tq])

    # the fallback
    native.window_gather_pad(native.make_gather_keys([obs_spec, act_spec]), ids, B, prev_n, post_n, C, index_ring)
    native.policy_sample_q_forward(fused, [job_tq])
    torch.cuda.synchronize()
    off = np.arange(Lw, dtype=np.int64) - prev_n
    slot = np.mod(ids_h[:, None] + off[None, :], np.int64(C))
    valid = (index[slot].astype(np.int64) - index[np.mod(ids_h, np.int64(C))].astype(np.int64)[:, None]) == off[None, :]
    valid[:, prev_n] = True
    assert np.array_equal(batch['obs_vec'].cpu().numpy(), obs_ring.cpu().numpy()[slot])
    assert np.array_equal(batch['action'].cpu().numpy(),
                          np.where(valid[..., None], act_ring.cpu().numpy()[slot], pad_row.cpu().numpy()))
    assert bool(torch.isfinite(a_y).all()) and bool((a_y != 0).any())


# ---- the TD errors' return + priority update ---------------------------------------------------------------------------
def _td_update_case(nat, B, n):
    torch.manual_seed(B * 31 + n)
    rng = np.random.default_rng(B * 31 + n)
    E, An, C = 3, 2, 256
    f = dict(device='cuda')
    q = torch.randn(E, B, n + 1, **f)
    logp, log_alpha = torch.randn(B, n + 1, **f), torch.tensor([-1.2], **f)
    reward, done = torch.randn(B, n, **f), torch.rand(B, n, **f) < 0.1
    last, pad = torch.rand(B, n, **f) < 0.05, torch.rand(B, n, **f) < 0.1
    mu, pi = torch.rand(B, n, An, **f) + 0.05, torch.rand(B, n + 1, An, **f) + 0.05
    gr, lr = torch.logspace(0, n - 1, n, 0.99).cuda(), torch.logspace(0, n - 1, n, 0.95).cuda()
    q_on = torch.randn(E, B, **f)
    slots = np.sort(rng.choice(C, B, replace=False))
    slots[1] = slots[0]                                       # a duplicate: the last writer wins
    wraps = rng.integers(1, 4, B)
    wraps[1] = wraps[0]
    wraps[2] = 2 ** 25                                        # an id beyond 2^32
    ids_h = (slots + wraps * C).astype(np.int64)
    slot_h = np.arange(C, dtype=np.int64)
    slot_h[slots] = ids_h
    gone = 3
    slot_h[slots[gone]] += C                                  # overwritten since it was sampled: skipped
    ids, slot0 = torch.from_numpy(ids_h).cuda(), torch.from_numpy(slot_h).cuda()
    assert np.array_equal(np.mod(ids_h, np.int64(C)), slots) and int(ids_h.min()) >= C
    start = DevTree(nat, C)
    start.set_priorities(np.arange(C), rng.random(C).astype(np.float32) + 0.01)
    base_tree = start.tree

    def run(merged):
        tree = base_tree.clone()
        winner, nan_flag = torch.full((C,), -1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
        y, td = torch.zeros(B, **f), torch.zeros(B, **f)
        a = _vtrace_args(nat, q=q, logp=logp, log_alpha=log_alpha, reward=reward, done=done, last=last, pad=pad, mu=mu, pi=pi,
                         A=An, gamma_ratio=gr, lambda_ratio=lr, gamma=0.99, rho=1.0, c=1.0, use_is=True, y=y,
                         q_online=q_on, td=td)
        if merged:
            nat.td_update(a, tree, C, ids, slot0, 0.9, 0.01, 1.0, winner, nan_flag)
        else:
            nat.vtrace_return_min(a)
            nat.sumtree_update(tree, C, ids, slot0, td, 0.9, 0.01, 1.0, 0, winner, nan_flag)
        assert int(nan_flag) == 0 and bool((winner == -1).all())
        chk = torch.zeros(1, dtype=torch.int32, device='cuda')
        nat.sumtree_check(tree, C, chk)                      # parent == left + right everywhere
        assert int(chk) == 0
        return y, td, tree

    want, got = run(False), run(True)
    for name, w_, g_ in zip(('y', 'td', 'tree'), want, got):
        assert torch.equal(w_, g_), name
    # the leaves: p = clip(td)^0.9 at id % capacity of every resident id (the duplicate: its last item), nothing else
    td_h = got[1].cpu().numpy()
    leaves = base_tree[C - 1:].cpu().numpy().copy()
    for i in range(B):
        if i != gone:
            leaves[slots[i]] = np.float32(np.power(np.clip(td_h[i], np.float32(0.01), np.float32(1.0)), 0.9))
    got_leaves = got[2][C - 1:].cpu().numpy()
    touched = np.zeros(C, bool)
    touched[np.delete(slots, gone)] = True
    assert np.array_equal(got_leaves[~touched], leaves[~touched])
    np.testing.assert_allclose(got_leaves[touched], leaves[touched], rtol=2e-7, atol=0)      # (pow: one ulp of float32)


@pytest.mark.parametrize('B,n', [(5, 1), (5, 4), (70, 1), (70, 4)])
def test_td_update_with_ids_beyond_a_wrap(nat, B, n):
    """asac_td_update == asac_vtrace_return_min + asac_sumtree_update bit for bit with ids >= capacity (the ring has
    wrapped) and one id whose slot has been overwritten; the leaves that change are the ones NumPy's `%` names."""
    _td_update_case(nat, B, n)


# ---- a divisor the host knows, as multiply-shift (asac_common.h: fastdiv; k_td_update's item -> (row, step) split) ----
# kernel-level: the quotient picks the addresses every output is read from, so a wrong one shows in the exact comparison
# with the launch that keeps its own division (asac_vtrace_return_min: `/ n` per item).  n = 1 has no multiplier (the
# kernel's own division runs), 3 and 40 are no powers of two, 64 is the longest window the workgroup's LDS takes at B = 37.
@pytest.mark.parametrize('n', [1, 3, 4, 40, 64])
def test_td_update_item_split_by_multiply_shift(nat, n):
    _td_update_case(nat, 37, n)


# the ring tile's row -> (sample, window row) split keeps its division (a multiply-shift form did not pay: NOTES.md); the
# window lengths it was tried at stay as cases of the ring-addressed launch against gather + plain launch
@pytest.mark.parametrize('T', [1, 2, 5, 41, 81])
def test_ring_tile_row_split_at_short_and_long_windows(nets, T):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused_mlp import StockMLP
    from tests.test_head_gather_gpu import C_RING, _ring
    B, prev_n, post_n = (40 if T <= 5 else 7), 0, max(T - 1, 1)          # (the replay wants a window of two rows at least)
    rb = _ring(B, prev_n, post_n)
    batch, specs = rb._window_specs(B)
    obs_spec = next(s for s in specs if s.get('dst') is batch['obs_vec'])
    act_spec = next(s for s in specs if s.get('dst') is batch['action'])
    keys = native.make_gather_keys(specs)
    ids, index_ring = rb._ids, rb._index_ring()
    eps, eps2 = torch.randn(B * T, A, device='cuda'), torch.randn(B, A, device='cuda')
    native.window_gather_pad(keys, ids, B, prev_n, post_n, C_RING, index_ring)
    torch.cuda.synchronize()
    want = _launch(native, StockMLP, nets, batch, B, T, prev_n, eps, eps2)
    ring = dict(ids=ids, index_ring=index_ring, capacity=C_RING, prev_n=prev_n, L=prev_n + 1 + post_n, j0=prev_n,
                x0_key=native.ring_key(obs_spec), action_key=native.ring_key(act_spec))
    got = _launch(native, StockMLP, nets, batch, B, T, prev_n, eps, eps2, ring=ring)
    for k, v in want.items():
        assert torch.equal(got[k], v), (T, k)
