"""GPU: `hip_config['policy_forward_rider']` — the policy's forward on the policy step's rows rides in the Q-loss backward
launch (`asac_mlp_backward_qloss_return_rider`, further workgroups of `k_mlp_bwd`) and the one-launch policy step LOADS it
(`asac_policy_step_fused_loaded`, `k_policy_step<.., LOADED>`) instead of running it again behind the critics.  Nothing
may change: the partial slabs of every tile, the value table and every output of the hosting launch are compared bit for
bit with today's launches, at the smallest shapes at which these kernels can go wrong (a single ragged tile, an exact
tile, a ragged second tile, three tiles); the learners' whole state with the switch on and off, eager and as a replayed
captured step.

State widths: 6 (the first layer's K rounded up to 8) and 64 - A — the widest a stock critic on (state | action) admits
(`asac_policy_step_fused_ok` wants both networks on <= 64 inputs and the policy on the critics' state width), where the
critics' first layer takes the full-width MFMA loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CLIP = 0.2
F = dict(device='cuda')
SAVE_X, SAVE_ZP, SAVE_HEAD, SAVE_TILE = 0, 3072, 6144, 6400        # float offsets inside one saved tile


def _nets(S, A, residual, policy, E=2):
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_mlp import StockMLP, describe_policy, describe_q
    torch.manual_seed(7)
    mods = [m.ModelPolicy(S, [], A).cuda()] if policy else [m.ModelQ(S, [], A, False).cuda() for _ in range(E)]
    desc = describe_policy(mods[0]) if policy else describe_q(mods[0])
    assert desc is not None
    with torch.no_grad():
        for mod in mods:
            for p in mod.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.3)
    for l in (1, 2):            # (the first block maps S (+ A) inputs to 64 and cannot have one)
        desc.residual[l] = int(residual)
    group = FlatParamGroup([(f'm{i}', list(mod.parameters())) for i, mod in enumerate(mods)], 'cuda')
    stride = group.segments['m0'][1] - group.segments['m0'][0]
    mlp = StockMLP(desc, group.flat, group.grad, 0, stride, len(mods), torch.device('cuda'))
    assert mlp.params.data_ptr() % 16 == 0
    mlp.accumulate = False
    return mlp


def _slabs(mlp, N):
    from asac_amd import native
    tiles, used = native.mlp_backward_tiles(N, mlp.E), native.mlp_param_extent(mlp.desc)
    return mlp._workspace[:tiles * mlp.E * mlp.member_stride].view(tiles, mlp.E, -1)[:, :, :used]


def _loss_partials(mlp, N):
    from asac_amd import native
    tiles = native.mlp_backward_tiles(N, mlp.E)
    base = tiles * mlp.E * mlp.member_stride
    return mlp._workspace[base:base + tiles * mlp.E].view(tiles, mlp.E)


def _ret_args(nat, N, n, A, E, y):
    g = torch.Generator(device='cuda').manual_seed(N * 31 + n)
    r = nat.VtraceArgs()
    t = dict(q=torch.randn(E, N, n + 1, generator=g, **F), logp=torch.randn(N, n + 1, generator=g, **F),
             log_alpha=torch.tensor([-1.2], **F), reward=torch.randn(N, n, generator=g, **F),
             done=torch.rand(N, n, generator=g, **F) < 0.1, last=torch.rand(N, n, generator=g, **F) < 0.05,
             pad=torch.rand(N, n, generator=g, **F) < 0.1, mu=torch.rand(N, n, A, generator=g, **F) + 0.05,
             pi=torch.rand(N, n + 1, A, generator=g, **F) + 0.05,
             gr=torch.logspace(0, n - 1, n, 0.99).cuda(), lr=torch.logspace(0, n - 1, n, 0.95).cuda())
    r.q = t['q'].data_ptr()
    r.q_stride_e, r.q_stride_b, r.q_stride_t = t['q'].stride(0), t['q'].stride(1), t['q'].stride(2)
    r.logp, r.log_alpha, r.E_sample = t['logp'].data_ptr(), t['log_alpha'].data_ptr(), min(E, 2)
    r.reward, r.reward_stride = t['reward'].data_ptr(), t['reward'].stride(0)
    r.done, r.last_mask, r.padding_mask, r.mask_stride = (t['done'].data_ptr(), t['last'].data_ptr(), t['pad'].data_ptr(),
                                                          t['done'].stride(0))
    r.mu_prob, r.mu_stride_b, r.mu_stride_t, r.mu_offset = t['mu'].data_ptr(), t['mu'].stride(0), t['mu'].stride(1), 0
    r.pi_prob, r.pi_stride_b, r.pi_stride_t, r.A = t['pi'].data_ptr(), t['pi'].stride(0), t['pi'].stride(1), A
    r.gamma_ratio, r.lambda_ratio = t['gr'].data_ptr(), t['lr'].data_ptr()
    r.gamma, r.v_rho, r.v_c, r.use_n_step_is, r.B, r.n = 0.99, 1.0, 1.0, 1, N, n
    r.y_out = y.data_ptr()
    return r, t          # (t keeps the tensors alive)


def _q_backward(fq, fpi, x, a0, tq, w, N, n, A, rider_rows=None, save=None):
    """the Q-loss backward forming its return, into NaN-filled outputs -> (slabs, loss partials, y, state gradients)"""
    from asac_amd import native as nat
    y = torch.full((N,), float('nan'), **F)
    r, keep = _ret_args(nat, N, n, A, fq.E, y)
    loss = torch.zeros(fq.E, **F)
    fq._workspace_for(N).fill_(float('nan'))
    assert fq.backward_qloss_return_ok(N, r)
    if rider_rows is None:
        g0 = fq.backward_qloss_return(x, a0, tq, r, w, CLIP, loss, defer=True, state_grads=True)
    else:
        assert fq.backward_qloss_return_rider_ok(N, r, fpi, rider_rows, save)
        g0 = fq.backward_qloss_return_rider(x, a0, tq, r, w, CLIP, loss, fpi, rider_rows, save, defer=True, state_grads=True)
    torch.cuda.synchronize()
    out = (_slabs(fq, N).clone(), _loss_partials(fq, N).clone(), y, g0)
    assert all(torch.isfinite(o).all() for o in out), 'a live output word of the hosting launch was not written'
    return out


def _case(N, A, S, residual, offline, E=2, subset=None, n=4):
    from asac_amd import native
    fq = _nets(S, A, residual, policy=False, E=E)
    fpi = _nets(S, A, residual, policy=True)
    torch.manual_seed(100 * N + A)
    x = torch.randn(N, 3, S, **F)[:, 1]                  # strided rows
    eps = torch.randn(N, A, **F)
    log_alpha = torch.tensor(-0.7, **F)
    off = torch.randn(N, 2, A, **F)[:, 1] if offline else None
    sub = torch.tensor(subset, dtype=torch.int32, device='cuda') if subset is not None else None
    ls = fpi._launch_forward(x, None)[0]
    a, logp = torch.empty(N, A, **F), torch.empty(N, **F)
    native.squash_sample_fwd(ls[:, :A], ls[:, A:], eps, a, logp)
    assert fpi.policy_step_fused_ok(fq, N)

    def step(saved):
        q_out = torch.full((E, N, 1), -7.0, **F)         # (rows of members the objective does not sample stay as they are)
        fpi._workspace_for(N).fill_(float('nan'))
        if saved is None:
            fpi.policy_step_fused(fq, x, a, eps, log_alpha, q_out=q_out, defer=True, subset=sub, offline=off)
        else:
            fpi.policy_step_fused_loaded(fq, x, a, eps, log_alpha, saved, q_out=q_out, defer=True, subset=sub, offline=off)
        torch.cuda.synchronize()
        return _slabs(fpi, N).clone(), q_out

    want_s, want_q = step(None)
    assert torch.isfinite(want_s).all()
    # ---- the hosting launch, without and with the rider
    a0, tq, w = torch.randn(N, A, **F).tanh(), torch.randn(E, N, **F) * 0.3, torch.rand(N, **F) + 0.5
    plain = _q_backward(fq, fpi, x, a0, tq, w, N, n, A)
    save = fpi.forward_save_buffer(N)
    assert save.numel() == (N + 15) // 16 * SAVE_TILE
    save.fill_(float('nan'))
    hosted = _q_backward(fq, fpi, x, a0, tq, w, N, n, A, rider_rows=x, save=save)
    for got, want, what in zip(hosted, plain, ('partial slabs', 'loss partials', 'y', 'state gradients')):
        assert torch.equal(got, want), f'hosting launch: {what}'
    assert torch.isfinite(save).all(), 'a word of a saved tile (dead rows included) was not written'
    # ---- the saved raw head, through the head transform, is the forward's (loc | scale)
    tiles = save.view(-1, SAVE_TILE)
    raw = tiles[:, SAVE_HEAD:].reshape(-1, 16)[:N, :2 * A].contiguous()
    loc, scale = torch.empty(N, A, **F), torch.empty(N, A, **F)
    native.gauss_head_fwd(raw, A, loc, scale)
    assert torch.equal(torch.cat([loc, scale], dim=1), ls), 'saved head'
    # ---- the loaded policy step, twice
    assert native.policy_step_fused_loaded_ok(fq.desc, fq.params, fq.member_stride, fpi.desc, fpi.params, fpi.member_stride,
                                              N, save)
    for _ in range(2):
        got_s, got_q = step(save)
        for t in range(got_s.shape[0]):
            assert torch.equal(got_s[t], want_s[t]), f'partial slab of tile {t}'
        assert torch.equal(got_q, want_q), 'value table'


@pytest.mark.parametrize('offline', [False, True])
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('wide_state', [False, True])
@pytest.mark.parametrize('A', [1, 2, 4])
@pytest.mark.parametrize('N', [1, 16, 17, 40])
def test_rider_then_loaded_policy_step_is_todays_policy_step_bit_for_bit(N, A, wide_state, residual, offline):
    _case(N, A, 64 - A if wide_state else 6, residual, offline)


@pytest.mark.parametrize('offline', [False, True])
@pytest.mark.parametrize('N', [17, 40])
def test_an_ensemble_of_three_with_a_device_subset(N, offline):
    """the two members the objective samples are named on the device; the third row of the value table stays unwritten"""
    _case(N, 2, 6, True, offline, E=3, subset=[2, 0])


@pytest.mark.parametrize('n', [1, 4])
@pytest.mark.parametrize('N', [17, 40])
def test_hosting_launch_is_unchanged_for_its_own_job(N, n):
    A, S = 2, 6
    fq = _nets(S, A, True, policy=False)
    fpi = _nets(S, A, True, policy=True)
    torch.manual_seed(N + n)
    x = torch.randn(N, S, **F)
    a0, tq, w = torch.randn(N, A, **F).tanh(), torch.randn(2, N, **F) * 0.3, torch.rand(N, **F) + 0.5
    plain = _q_backward(fq, fpi, x, a0, tq, w, N, n, A)
    save = fpi.forward_save_buffer(N)
    for _ in range(2):
        hosted = _q_backward(fq, fpi, x, a0, tq, w, N, n, A, rider_rows=x, save=save)
        for got, want, what in zip(hosted, plain, ('partial slabs', 'loss partials', 'y', 'state gradients')):
            assert torch.equal(got, want), what


# ---- step level -----------------------------------------------------------------------------------------------------
import bench  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.test_full_size_gpu import _episode  # noqa: E402

VEC = dict(bench.CONFIGS['cfg2'], n_step=2, batch_size=32, capacity=1024, episode_len=37)
RNN = dict(bench.CONFIGS['cfg3'], n_step=3, burn_in_step=3, batch_size=32, capacity=1024, episode_len=37)


def _learner(cfg, rider, use_graph=False):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    torch.manual_seed(0)
    agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], [], cfg['c_action_size'], None, pu.plugin(cfg['plugin']),
                     device='cuda:0', n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'], batch_size=cfg['batch_size'],
                     ensemble_q_num=cfg['ensemble_q_num'], ensemble_q_sample=cfg['ensemble_q_sample'],
                     seq_encoder=SEQ_ENCODER[cfg['seq_encoder']] if cfg['seq_encoder'] else None,
                     replay_config={'capacity': cfg['capacity']},
                     hip_config={'use_graph': use_graph, 'graph_warmup': 2, 'policy_forward_rider': rider})
    rng = np.random.default_rng(5)
    for _ in range(800 // cfg['episode_len']):
        agent.put_episode(**_episode(rng, cfg, cfg['episode_len']))
    rb = agent.replay_buffer
    ids = torch.arange(rb.size, device=rb.device, dtype=torch.int64)
    rb.update(ids, torch.from_numpy(np.abs(rng.standard_normal(rb.size)).astype(np.float32)).to(rb.device))
    return agent


def _state(agent):
    rb = agent.replay_buffer
    return dict(params=agent._params.flat, exp_avg=agent._exp_avg, exp_avg_sq=agent._exp_avg_sq,
                target=agent._target_params.flat, tree=rb._tree, mu_prob=rb._columns['mu_prob'])


def _names(agent):
    from asac_amd import native
    with native.LaunchProfiler(repeat=1) as prof:
        agent.train()
    torch.cuda.synchronize()
    return {k: len(v) for k, v in prof.records.items()}


def _spy(monkeypatch):
    """counts the calls that reach the two new wrappers"""
    from algorithm.fused_mlp import StockMLP
    calls = dict(rider=0, loaded=0)
    real_r, real_l = StockMLP.backward_qloss_return_rider, StockMLP.policy_step_fused_loaded

    def rider(self, *a, **k):
        calls['rider'] += 1
        return real_r(self, *a, **k)

    def loaded(self, *a, **k):
        calls['loaded'] += 1
        return real_l(self, *a, **k)
    monkeypatch.setattr(StockMLP, 'backward_qloss_return_rider', rider)
    monkeypatch.setattr(StockMLP, 'policy_step_fused_loaded', loaded)
    return calls


def test_learners_with_the_switch_on_and_off_stay_equal_eager(monkeypatch):
    calls = _spy(monkeypatch)
    on, off = _learner(VEC, True), _learner(VEC, False)
    for step in range(5):
        if step == 1:
            n_on, before = _names(on), dict(calls)
            n_off = _names(off)
            assert n_on == n_off, 'the profiler names of a step'
            assert calls == dict(rider=before['rider'], loaded=before['loaded']), 'the switch off reached a new wrapper'
        else:
            on.train()
            off.train()
        torch.cuda.synchronize()
        a, b = _state(on), _state(off)
        for k in a:
            assert torch.equal(a[k], b[k]), f'step {step}: {k}'
    assert calls == dict(rider=5, loaded=5), calls
    on.close()
    off.close()


def test_a_replayed_captured_step_with_the_switch_on_equals_eager_steps_with_it_off(monkeypatch):
    calls = _spy(monkeypatch)
    on, off = _learner(VEC, True, use_graph=True), _learner(VEC, False)
    for step in range(2 + 3):           # the warm-up, then three replays
        on.train()
        off.train()
        torch.cuda.synchronize()
        assert (on._graph is not None) == (step >= 2)
        a, b = _state(on), _state(off)
        for k in a:
            assert torch.equal(a[k], b[k]), f'step {step}: {k}'
    assert calls['rider'] >= 1 and calls['rider'] == calls['loaded'], calls
    on.close()
    off.close()


def test_a_trainable_representation_takes_todays_launches(monkeypatch):
    calls = _spy(monkeypatch)
    on, off = _learner(RNN, True), _learner(RNN, False)
    for step in range(2):
        n_on, n_off = _names(on), _names(off)
        assert n_on == n_off
        a, b = _state(on), _state(off)
        for k in a:
            assert torch.equal(a[k], b[k]), f'step {step}: {k}'
    assert calls == dict(rider=0, loaded=0), calls
    on.close()
    off.close()
