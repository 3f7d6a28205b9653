"""GPU: the step's first network launch (`asac_policy_sample_q_forward`) reading its rows where they lie in the replay ring
(`native.pi_q_ring_rows`) with the batch's own window gather riding in it as a sidecar job — against the stand-alone
`asac_window_gather_pad` followed by the same launch on the gathered batch.  Nothing changes an operation or an order:
every comparison is `torch.equal`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_fused_mlp_gpu import _setup  # noqa: E402

C_RING, EPISODE, S, A, E = 4096, 37, 6, 3, 2


def _f32_bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.fixture(scope='module')
def nets():
    _, _, ftq = _setup(E, S, A)
    _, _, fpi = _setup(1, S, A, policy=True)
    return fpi, ftq


def _ring(batch, prev_n, post_n):
    import asac_amd  # noqa: F401
    from algorithm.replay_buffer import PrioritizedReplayBuffer
    gen = np.random.default_rng(0)
    n = C_RING          # a full ring: a window past its last slot continues at slot 0
    data = dict(index=(np.arange(n) % EPISODE).astype(np.int32), obs_vec=gen.standard_normal((n, S)).astype(np.float32),
                action=np.tanh(gen.standard_normal((n, A))).astype(np.float32),
                reward=gen.standard_normal(n).astype(np.float32), done=np.zeros(n, bool), last_mask=np.zeros(n, bool),
                mu_prob=np.ones((n, A), np.float32), pre_seq_hidden_state=gen.standard_normal((n, 2)).astype(np.float32))
    rb = PrioritizedReplayBuffer(batch_size=batch, capacity=C_RING, sample_prev_n=prev_n, sample_post_n=post_n, device='cuda')
    rb.set_window_padding(torch.tensor([0.25, -0.5, 0.75]))
    rb.add(data)
    rb.sample()
    # ids placed by hand: a window that runs over the ring's end, one that starts on the last row of an episode, one whose
    # burn-in rows lie before slot 0, one that starts an episode (burn-in rows in another episode)
    rb._ids[:4] = torch.tensor([C_RING - 2, EPISODE - 1, 0, 3 * EPISODE], device='cuda')
    return rb


def _launch(native, StockMLP, nets, batch, B, T, j0, eps, eps2, ring=None, sidecars=None):
    """policy -> sample (+ pi(stored action), + second sample) -> critics over window rows j0.. of `batch`, the target Q
    of the stored pair at row j0 riding along -> every output of the launch"""
    fpi, ftq = nets
    f32 = dict(dtype=torch.float32, device='cuda')
    obs, act = batch['obs_vec'][:, j0:j0 + T], batch['action'][:, j0:j0 + T]
    rows = StockMLP._rows_in_place(obs, S)
    job_pi, ls = fpi.job(rows, None)
    a_y, logp_y, c_pi = torch.zeros((B, T, A), **f32), torch.zeros((B, T), **f32), torch.zeros((B, T, A), **f32)
    a2, logp2 = torch.zeros((B, A), **f32), torch.zeros(B, **f32)
    job_q, q_tab = ftq.job(rows, a_y.view(-1, A))
    job_tq, tq = ftq.job(StockMLP._rows(obs[:, 0], S), StockMLP._rows(act[:, 0], A))
    fused = native.pi_q_job(job_pi, job_q, eps, a_y, logp_y, T, action=act, prob_out=c_pi, eps2=eps2, t2=0, a2_out=a2,
                            logp2_out=logp2)
    if ring is not None:
        fused = native.pi_q_ring_rows(fused, x_j0=j0, **ring)
    assert native.policy_sample_q_forward_ok(fused)
    native.policy_sample_q_forward(fused, [job_tq], sidecars=sidecars)
    torch.cuda.synchronize()
    return dict(a=a_y, logp=logp_y, pi_stored=c_pi, ls=ls, q=q_tab, a2=a2, logp2=logp2, tq=tq)


# B = 40: 200 rows, a partial 16-row tile; prev_n = 2: burn-in rows in front (j0 = 2); the observation key padded with a
# word (the replay's own table keeps observation rows: ASAC_PAD_KEEP) beside the action key's pad row
@pytest.mark.parametrize('B,prev_n,obs_pad_word', [(40, 0, False), (40, 0, True), (256, 2, False), (256, 2, True)])
def test_ring_addressed_launch_with_gather_rider_equals_gather_then_launch(nets, B, prev_n, obs_pad_word):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused_mlp import StockMLP
    T, post_n = 5, 4
    rb = _ring(B, prev_n, post_n)
    batch, specs = rb._window_specs(B)
    obs_spec = next(s for s in specs if s.get('dst') is batch['obs_vec'])
    act_spec = next(s for s in specs if s.get('dst') is batch['action'])
    assert act_spec['pad_mode'] == native.PAD_ROW
    if obs_pad_word:
        obs_spec['pad_mode'], obs_spec['pad_word'] = native.PAD_WORD, _f32_bits(0.5)
    keys = native.make_gather_keys(specs)
    ids, index_ring = rb._ids, rb._index_ring()
    eps, eps2 = torch.randn(B * T, A, device='cuda'), torch.randn(B, A, device='cuda')

    native.window_gather_pad(keys, ids, B, prev_n, post_n, C_RING, index_ring)
    torch.cuda.synchronize()
    assert bool(batch['padding_mask'].any()) and not bool(batch['padding_mask'].all())
    want_batch = {k: v.clone() for k, v in batch.items()}
    want = _launch(native, StockMLP, nets, batch, B, T, prev_n, eps, eps2)

    for v in batch.values():       # nothing of the gathered batch is left for the ring-addressed launch to read
        v.fill_(float('nan')) if v.is_floating_point() else v.zero_()
    rider = native.sidecar_window_gather(keys, ids, B, prev_n, post_n, C_RING, index_ring)
    ring = dict(ids=ids, index_ring=index_ring, capacity=C_RING, prev_n=prev_n, L=prev_n + 1 + post_n, j0=prev_n,
                x0_key=native.ring_key(obs_spec), action_key=native.ring_key(act_spec))
    got = _launch(native, StockMLP, nets, batch, B, T, prev_n, eps, eps2, ring=ring, sidecars=[rider])
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    for k, v in want_batch.items():
        assert torch.equal(batch[k], v), k


def test_ring_addressing_refuses_what_it_does_not_cover(nets):
    import asac_amd  # noqa: F401
    from asac_amd import native
    rb = _ring(40, 0, 4)
    batch, specs = rb._window_specs(40)
    by_dst = {k: next(s for s in specs if s.get('dst') is v) for k, v in batch.items()}
    assert native.ring_key(by_dst['done']) is None and native.ring_key(by_dst['padding_mask']) is None     # 8-bit, a mask
    assert native.ring_key(dict(by_dst['obs_vec'], derive=native.DERIVE_PREVIOUS)) is None
    assert native.ring_key(dict(by_dst['obs_vec'], convert=native.CVT_U8_TO_F32_UNIT)) is None
    assert native.ring_key(by_dst['obs_vec']) is not None


# the IS weights (K2) off the sampler's path: the prologue's sampler in its partial form (ids, leaves, p, the minimum) plus one
# rider workgroup of the ring-addressed launch (minimum, beta, the f64 powers) against `step_prologue_sample`, which does
# all of it in the sampler workgroup — the same operations in the same order
@pytest.mark.parametrize('B', [40, 256])
def test_is_weights_ride_in_the_first_network_launch(nets, B):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused import DeviceNoise
    from algorithm.fused_mlp import StockMLP
    T = 5
    rbs = [_ring(B, 0, T - 1) for _ in range(2)]
    td = torch.rand(C_RING, device='cuda') + 0.01
    ids_all = torch.arange(C_RING, device='cuda', dtype=torch.int64)
    step = torch.zeros(1, dtype=torch.int64, device='cuda')
    flat = torch.zeros(64, device='cuda')
    for rb in rbs:
        rb.update(ids_all, td)
        rb.uniform_source = DeviceNoise(1234)
    whole, part = rbs
    assert torch.equal(whole._tree, part._tree) and torch.equal(whole._beta, part._beta)
    head = part.head_gather('obs_vec', build=True)
    assert head is not None
    eps, eps2 = torch.randn(B * T, A, device='cuda'), torch.randn(B, A, device='cuda')
    for draw in range(2):
        step.fill_(draw)
        assert whole.uniform_source.begin_step_with_sample(step, whole, flat) == 1
        assert part.uniform_source.begin_step_with_sample(step, part, flat, defer_weights=True, defer_small=True) == 3
        ring = dict(ids=part._ids, index_ring=head['index_ring'], capacity=C_RING, prev_n=0, L=T, j0=0, x0_key=head['x0'],
                    action_key=head['action'])
        _launch(native, StockMLP, nets, part._batch, B, T, 0, eps, eps2, ring=ring, sidecars=[head['sidecar_w']])
        torch.cuda.synchronize()
        for k in ('_ids', '_leaf', '_p', '_w', '_beta', '_u'):
            assert torch.equal(getattr(whole, k), getattr(part, k)), (draw, k)
        assert torch.equal(whole._min_p[:1], part._min_p[:1]), draw
        assert float(part._beta) > 0 and bool((part._w != 1).any())
    # ... and the rider's gather delivered the batch of the ids drawn last
    whole.sample_into_static(sampled=1)
    torch.cuda.synchronize()
    for k, v in whole._batch.items():
        assert torch.equal(part._batch[k], v), k
