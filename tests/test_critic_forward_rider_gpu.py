"""GPU: `hip_config['critic_forward_rider']` — the ONLINE critics' forward on the stored pair rides in the step's first
network launch (`asac_policy_sample_q_forward_saving`, four-wave workgroups behind the extra jobs of `k_pi_sample_q` /
`k_pi_sample_q_ring`) and the Q-loss backward LOADS it (`asac_mlp_backward_qloss_return_loaded` / `_rider_loaded`,
`k_mlp_bwd<.., LOADED>`) instead of recomputing it.  The rider executes the recompute's statements in the recompute's order,
so the tolerance is zero: every partial slab, the loss partials, y, the reduced gradients and every output of the hosting
launch are compared with `torch.equal` against today's launches — kernel level at one row, one full tile, a tile with one
live row and a ragged third tile; ring-addressed rows against the gathered batch; the learners' whole state with the switch
on and off, eager and as a replayed captured step."""
import numpy as np
import pytest
import torch

from tests.test_policy_forward_rider_gpu import _loss_partials, _nets, _ret_args, _slabs

pytestmark = pytest.mark.gpu

CLIP = 0.2
F = dict(device='cuda')
SAVE_TILE = 6160                     # floats of a saved (tile, member): x_1..x_3 3072 | fragments 3072 | raw q 16


def _target_like(fq, S, A, residual):
    """a second ensemble (the target critics of the hosting launch's extra job) with other parameters"""
    ftq = _nets(S, A, residual, policy=False, E=fq.E)
    with torch.no_grad():
        ftq.params.mul_(0.9)
    return ftq


def _forward(native, fpi, ftq, fq, xs, x0, a0, eps, T, save=None, ring=None, sidecars=None):
    """the first network launch: policy -> sample -> target critics over `xs`, the target critics on the stored pair as
    extra job 0; with `save` the online critics `fq` ride on the stored pair -> every output of the launch"""
    N, A = eps.shape
    o = dict(a=torch.full((N, A), 7., **F), logp=torch.full((N,), 7., **F))
    job_pi, ls = fpi.job(xs, None)
    job_q, o['q'] = ftq.job(xs, o['a'])
    job_x, o['x'] = ftq.job(x0, a0)
    ls.fill_(7.), o['q'].fill_(7.), o['x'].fill_(7.)
    job = native.pi_q_job(job_pi, job_q, eps, o['a'], o['logp'], T)
    if ring is not None:
        job = native.pi_q_ring_rows(job, **ring)
    assert native.policy_sample_q_forward_ok(job, [job_x])
    if save is None:
        native.policy_sample_q_forward(job, [job_x], sidecars=sidecars)
    else:
        online = fq._pass(x0, a0)
        assert native.policy_sample_q_forward_saving_ok(job, [job_x], sidecars, online, save)
        native.policy_sample_q_forward_saving(job, [job_x], sidecars, online, save)
    torch.cuda.synchronize()
    o['ls'] = ls
    return o


def _backward(fq, x0, a0, tq, w, n, A, saved=None, fpi=None, pi_save=None, defer=True):
    """the Q-loss backward forming its return, into NaN-filled outputs -> slabs, loss partials, y (deferred) or the reduced
    gradients, the loss and y"""
    from asac_amd import native as nat
    N = x0.shape[0]
    y = torch.full((N,), float('nan'), **F)
    r, keep = _ret_args(nat, N, n, A, fq.E, y)
    if fq.E == 3:                    # a device subset for the return: the two members its minimum is taken over
        keep['sn'] = torch.tensor([2, 0], dtype=torch.int32, device='cuda')
        keep['sx'] = torch.tensor([1, 2], dtype=torch.int32, device='cuda')
        r.subset_n, r.subset_next = keep['sn'].data_ptr(), keep['sx'].data_ptr()
    loss = torch.full((fq.E,), float('nan'), **F)
    fq._workspace_for(N).fill_(float('nan'))
    fq.grad_params.fill_(float('nan'))
    assert fq.backward_qloss_return_ok(N, r)
    if saved is not None:
        assert fq.backward_qloss_return_loaded_ok(N, r, saved, *((fpi, x0, pi_save) if fpi is not None else ()))
    if fpi is None:
        fq.backward_qloss_return(x0, a0, tq, r, w, CLIP, loss, defer=defer, critic_saved=saved)
    else:
        assert fq.backward_qloss_return_rider_ok(N, r, fpi, x0, pi_save)
        fq.backward_qloss_return_rider(x0, a0, tq, r, w, CLIP, loss, fpi, x0, pi_save, defer=defer, critic_saved=saved)
    torch.cuda.synchronize()
    if defer:
        out = dict(slabs=_slabs(fq, N).clone(), loss_partial=_loss_partials(fq, N).clone(), y=y)
    else:
        from asac_amd import native
        out = dict(grads=fq.grad_params[:fq.E * fq.member_stride].view(fq.E, -1)[:, :native.mlp_param_extent(fq.desc)].clone(),
                   loss=loss, y=y)
    assert all(torch.isfinite(v).all() for v in out.values()), 'a live output word of the backward was not written'
    return out


def _same(got, want, what):
    for k, v in want.items():
        if k == 'slabs':
            for t in range(v.shape[0]):
                assert torch.equal(got[k][t], v[t]), (what, f'partial slab of tile {t}')
        else:
            assert torch.equal(got[k], v), (what, k)


def _case(N, A, S, residual, ns, weights, E=2, policy_rider=False):
    from asac_amd import native
    fq = _nets(S, A, residual, policy=False, E=E)
    ftq = _target_like(fq, S, A, residual)
    fpi = _nets(S, A, residual, policy=True)
    torch.manual_seed(100 * N + 10 * A)
    x0 = torch.randn(N, 3, S, **F)[:, 1]                  # strided rows
    a0 = torch.randn(N, 2, A, **F)[:, 1].tanh()
    eps = torch.randn(N, A, **F)
    tq, w = torch.randn(E, N, **F) * 0.3, (torch.rand(N, **F) + 0.5) if weights else None
    pi_save = fpi.forward_save_buffer(N) if policy_rider else None
    host = (fpi, pi_save) if policy_rider else (None, None)
    # ---- the hosting launch, without and with the rider
    want_f = _forward(native, fpi, ftq, fq, x0, x0, a0, eps, 1)
    save = fq.critic_save_buffer(N)
    assert save.numel() == (N + 15) // 16 * E * SAVE_TILE and save.data_ptr() % 16 == 0
    save.fill_(float('nan'))
    got_f = _forward(native, fpi, ftq, fq, x0, x0, a0, eps, 1, save=save)
    _same(got_f, want_f, 'hosting launch')
    assert torch.isfinite(save).all(), 'a word of a saved tile (dead rows included) was not written'
    # ---- the saved raw q is the online critics' forward
    q_online = fq._launch_forward(x0, a0)
    tiles = save.view(-1, E, SAVE_TILE)
    for e in range(E):
        assert torch.equal(tiles[:, e, 6144:].reshape(-1)[:N], q_online[e].reshape(-1)), f'saved q of member {e}'
    # ---- the loaded backward, twice, deferred (tile by tile) and reduced
    for n, defer in [(n, defer) for n in ns for defer in (True, False)]:
        want = _backward(fq, x0, a0, tq, w, n, A, fpi=host[0], pi_save=host[1], defer=defer)
        want_pi = pi_save.clone() if policy_rider else None
        for _ in range(2):
            if policy_rider:
                pi_save.fill_(float('nan'))
            got = _backward(fq, x0, a0, tq, w, n, A, saved=save, fpi=host[0], pi_save=host[1], defer=defer)
            _same(got, want, f'loaded backward (defer={defer})')
            if policy_rider:
                assert torch.equal(pi_save, want_pi), 'the policy rider beside the loaded backward'


@pytest.mark.parametrize('weights', [True, False])
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('wide_state', [False, True])
@pytest.mark.parametrize('A', [1, 2, 4])
@pytest.mark.parametrize('N', [1, 16, 17, 40])
def test_rider_then_loaded_backward_is_todays_backward_bit_for_bit(N, A, wide_state, residual, weights):
    _case(N, A, 64 - A if wide_state else 6, residual, (1, 4), weights)


@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('A', [1, 2, 4])
@pytest.mark.parametrize('N', [1, 16, 17, 40])
def test_with_the_policy_rider_on_its_second_plane(N, A, residual):
    _case(N, A, 6, residual, (1, 4), True, policy_rider=True)


@pytest.mark.parametrize('policy_rider', [False, True])
@pytest.mark.parametrize('N', [17, 40])
def test_an_ensemble_of_three_with_a_device_subset_for_the_return(N, policy_rider):
    _case(N, 2, 6, True, (4,), True, E=3, policy_rider=policy_rider)


# ---- ring-addressed rows ------------------------------------------------------------------------------------------------
from tests.test_piq_wave_roles_gpu import C_RING, POST_N, PREV_N, S as S_RING, _ring  # noqa: E402


@pytest.mark.parametrize('A,E', [(2, 2), (4, 3)])
def test_ring_rows_save_what_the_gathered_batch_saves(A, E):
    """capacity 1 024; the ids (`_ring`) include the first rows of an episode (window neighbours in front are padding), windows
    that cross the ring's wrap, and ids whose id-map entry is stale (several wraps on, beyond 2^32).  The saved tiles must
    equal what the rider stores when it is given the gathered static batch instead; the hosting launch's outputs and the
    gather riding in it stay what they are."""
    from algorithm.fused_mlp import StockMLP
    from asac_amd import native
    B, T = 40, 3
    fq = _nets(S_RING, A, True, policy=False, E=E)
    ftq = _target_like(fq, S_RING, A, True)
    fpi = _nets(S_RING, A, True, policy=True)
    batch, specs, ring = _ring(native, B, A, 11)
    keys = native.make_gather_keys(specs)
    native.window_gather_pad(keys, ring['ids'], B, PREV_N, POST_N, C_RING, ring['index_ring'])
    torch.cuda.synchronize()
    want_batch = {k: v.clone() for k, v in batch.items()}
    obs, act = batch['obs_vec'][:, PREV_N:PREV_N + T], batch['action'][:, PREV_N:PREV_N + T]
    xs = StockMLP._rows_in_place(obs, S_RING)
    x0, a0 = StockMLP._rows(obs[:, 0], S_RING), StockMLP._rows(act[:, 0], A)
    eps = torch.randn(B * T, A, **F)
    # the rider on the gathered static batch (plain host)
    save = fq.critic_save_buffer(B)
    save.fill_(float('nan'))
    want_f = _forward(native, fpi, ftq, fq, xs, x0, a0, eps, T, save=save)
    want_save = save.clone()
    assert torch.isfinite(want_save).all()
    # ... and through the ring, the batch's gather riding as a sidecar of the same launch
    for v in batch.values():
        v.fill_(float('nan'))
    save.fill_(float('nan'))
    r = dict(ring, x_j0=PREV_N)
    sidecars = [native.sidecar_window_gather(keys, ring['ids'], B, PREV_N, POST_N, C_RING, ring['index_ring'])]
    got_f = _forward(native, fpi, ftq, fq, xs, x0, a0, eps, T, save=save, ring=r, sidecars=sidecars)
    _same(got_f, want_f, 'ring host')
    assert torch.equal(save, want_save), 'saved tiles: ring rows against the gathered batch'
    for k, v in want_batch.items():
        assert torch.equal(batch[k], v), k
    # ... and without the rider the ring host computes the same
    plain_f = _forward(native, fpi, ftq, fq, xs, x0, a0, eps, T, ring=r, sidecars=sidecars)
    _same(plain_f, want_f, 'ring host without the rider')


def test_a_grid_beyond_the_cu_count_is_refused():
    """the launch holds one workgroup per CU and dispatches in block order: with more workgroups in front of the sidecars
    (chain, stored pair, rider) than CUs the rider would wait for a second round, so `_ok` says no (and the entry point
    refuses) while the plain launch still qualifies.  (Sidecar workgroups follow the rider in the grid and are not counted:
    the headline launch carries 76 gather workgroups beside 192 of its own on 256 CUs already.)"""
    from asac_amd import native
    A, S, E = 2, 6, 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fq = _nets(S, A, True, policy=False, E=E)
    ftq = _target_like(fq, S, A, True)
    fpi = _nets(S, A, True, policy=True)
    B = 128                                       # 8 tiles x 2 members: 16 rider and 16 stored-pair workgroups
    T_fit = max((cus - 32) // 16 - 1, 1)          # the chain's 8 T x 2 workgroups beside them: inside / beyond the CUs
    T_over = (cus - 32) // 16 + 1
    for T, fits in ((T_fit, True), (T_over, False)):
        if T * B > 256 * 16 // E:                 # (the fused job itself caps its workgroups at 256)
            continue
        xs = torch.randn(B * T, S, **F)
        x0, a0 = torch.randn(B, S, **F), torch.randn(B, A, **F).tanh()
        eps = torch.randn(B * T, A, **F)
        o = dict(a=torch.empty(B * T, A, **F), logp=torch.empty(B * T, **F))
        job_pi, _ = fpi.job(xs, None)
        job_q, _ = ftq.job(xs, o['a'])
        job_x, _ = ftq.job(x0, a0)
        job = native.pi_q_job(job_pi, job_q, eps, o['a'], o['logp'], T)
        save = fq.critic_save_buffer(B)
        assert native.policy_sample_q_forward_ok(job, [job_x])
        assert native.policy_sample_q_forward_saving_ok(job, [job_x], None, fq._pass(x0, a0), save) == fits, (T, cus)
        if not fits:
            with pytest.raises(native.AsacNativeError):
                native.policy_sample_q_forward_saving(job, [job_x], None, fq._pass(x0, a0), save)
    torch.cuda.synchronize()


# ---- step level -----------------------------------------------------------------------------------------------------
import bench  # noqa: E402
from tests import parity_utils as pu  # noqa: E402
from tests.test_full_size_gpu import _episode  # noqa: E402
from tests.test_policy_forward_rider_gpu import RNN, VEC, _names, _state  # noqa: E402


def _learner(cfg, rider, use_graph=False, **hip):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    torch.manual_seed(0)
    agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], [], cfg['c_action_size'], None, pu.plugin(cfg['plugin']),
                     device='cuda:0', n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'], batch_size=cfg['batch_size'],
                     ensemble_q_num=cfg['ensemble_q_num'], ensemble_q_sample=cfg['ensemble_q_sample'],
                     seq_encoder=SEQ_ENCODER[cfg['seq_encoder']] if cfg['seq_encoder'] else None,
                     replay_config={'capacity': cfg['capacity']},
                     hip_config=dict({'use_graph': use_graph, 'graph_warmup': 2, 'critic_forward_rider': rider}, **hip))
    rng = np.random.default_rng(5)
    for _ in range(800 // cfg['episode_len']):
        agent.put_episode(**_episode(rng, cfg, cfg['episode_len']))
    rb = agent.replay_buffer
    ids = torch.arange(rb.size, device=rb.device, dtype=torch.int64)
    rb.update(ids, torch.from_numpy(np.abs(rng.standard_normal(rb.size)).astype(np.float32)).to(rb.device))
    return agent


def _spy(monkeypatch):
    """counts the launches that reach the two new wrappers (and whether the ring host carried the rider)"""
    from asac_amd import native
    calls = dict(saving=0, loaded=0, ring=0)
    real_s, real_l = native.policy_sample_q_forward_saving, native.mlp_backward_qloss_return_loaded

    def saving(job, *a, **k):
        calls['saving'] += 1
        calls['ring'] += bool(job.ring.ids)
        return real_s(job, *a, **k)

    def loaded(*a, **k):
        calls['loaded'] += 1
        return real_l(*a, **k)
    monkeypatch.setattr(native, 'policy_sample_q_forward_saving', saving)
    monkeypatch.setattr(native, 'mlp_backward_qloss_return_loaded', loaded)
    return calls


def _equal_states(on, off, step):
    a, b = _state(on), _state(off)
    for k in a:
        assert torch.equal(a[k], b[k]), f'step {step}: {k}'


@pytest.mark.parametrize('head_gather', [True, False])
def test_learners_with_the_switch_on_and_off_stay_equal_eager(monkeypatch, head_gather):
    """five eager steps; the first of a static set plans (today's launches), the other four carry the rider — through the
    ring host, or with `head_gather_sidecar: false` through the plain kernel"""
    calls = _spy(monkeypatch)
    on = _learner(VEC, True, head_gather_sidecar=head_gather)
    off = _learner(VEC, False, head_gather_sidecar=head_gather)
    for step in range(5):
        if step == 2:
            before = dict(calls)
            n_on, n_off = _names(on), _names(off)
            assert n_on == n_off, 'the profiler names of a step'
            assert calls['saving'] == before['saving'] + 1 and calls['loaded'] == before['loaded'] + 1, 'switch off reached a wrapper'
        else:
            on.train()
            off.train()
        torch.cuda.synchronize()
        _equal_states(on, off, step)
    assert calls['saving'] == 4 and calls['loaded'] == 4, calls
    assert calls['ring'] == (4 if head_gather else 0), calls
    on.close()
    off.close()


def test_a_replayed_captured_step_with_the_switch_on_equals_eager_steps_with_it_off(monkeypatch):
    calls = _spy(monkeypatch)
    on, off = _learner(VEC, True, use_graph=True), _learner(VEC, False)
    for step in range(2 + 3):           # the warm-up, then three replays
        before = dict(calls)
        on.train()
        off.train()
        torch.cuda.synchronize()
        assert (on._graph is not None) == (step >= 2)
        _equal_states(on, off, step)
        if step == 2:       # the capturing step issues both new launches into the graph; a replay issues none from here
            assert calls['saving'] == before['saving'] + 1 and calls['loaded'] == before['loaded'] + 1, (before, calls)
            captured = dict(calls)
    assert calls == captured and calls['ring'] == calls['saving'] == 2, calls
    on.close()
    off.close()


def test_a_learner_with_one_batch_in_flight_takes_the_rider_through_the_plain_kernel(monkeypatch):
    """`lookahead: 1`: the step's batch was gathered a step ahead, so the first network launch is the plain kernel and
    hosts the rider there"""
    calls = _spy(monkeypatch)
    states = {}
    for rider in (True, False):         # one learner at a time: a batch in flight belongs to the learner that sampled it
        agent = _learner(VEC, rider, lookahead=1)
        states[rider] = []
        for step in range(6):
            agent.train()
            torch.cuda.synchronize()
            states[rider].append({k: v.clone() for k, v in _state(agent).items()})
        agent.close()
        if rider:       # (every static set plans in its first step and rides from its second)
            taken = dict(calls)
            assert calls['saving'] >= 2 and calls['loaded'] == calls['saving'] and calls['ring'] == 0, calls
    assert calls == taken, 'the switch off reached a new wrapper'
    for step, (a, b) in enumerate(zip(states[True], states[False])):
        for k in a:
            assert torch.equal(a[k], b[k]), f'step {step}: {k}'


def test_a_batch_whose_launch_has_no_cus_for_the_rider_takes_todays_launches(monkeypatch):
    """batch 512, window 3: 192 chain + 64 stored-pair workgroups fill the CUs, the rider's 64 would not fit — the real
    predicate says no at every step, the learner issues today's launches by name and stays bit-equal"""
    from asac_amd import native
    cfg = dict(VEC, batch_size=512)
    fits = 2 * (512 * 3 // 16) + 2 * 2 * (512 // 16) <= torch.cuda.get_device_properties(0).multi_processor_count
    calls = _spy(monkeypatch)
    asked = []
    real_ok = native.policy_sample_q_forward_saving_ok
    monkeypatch.setattr(native, 'policy_sample_q_forward_saving_ok', lambda *a, **k: asked.append(real_ok(*a, **k)) or asked[-1])
    on, off = _learner(cfg, True), _learner(cfg, False)
    for step in range(3):
        n_on, n_off = _names(on), _names(off)
        assert n_on == n_off
        _equal_states(on, off, step)
    assert asked == [fits, fits], asked            # (asked from the second step on: the first one plans)
    assert not fits, 'a device with more than 320 CUs: choose a larger batch for this test'
    assert calls == dict(saving=0, loaded=0, ring=0), calls
    on.close()
    off.close()


def test_a_trainable_representation_takes_todays_launches(monkeypatch):
    calls = _spy(monkeypatch)
    on, off = _learner(RNN, True), _learner(RNN, False)
    for step in range(3):
        n_on, n_off = _names(on), _names(off)
        assert n_on == n_off
        _equal_states(on, off, step)
    assert calls == dict(saving=0, loaded=0, ring=0), calls
    on.close()
    off.close()


def test_a_refusing_predicate_leaves_todays_launches(monkeypatch):
    """the forward's `_ok` says no (as it does when the grid would exceed the CU count): the learner issues today's launches,
    launch for launch, and stays bit-equal"""
    from asac_amd import native
    calls = _spy(monkeypatch)
    monkeypatch.setattr(native, 'policy_sample_q_forward_saving_ok', lambda *a, **k: False)
    on, off = _learner(VEC, True), _learner(VEC, False)
    for step in range(3):
        n_on, n_off = _names(on), _names(off)
        assert n_on == n_off
        _equal_states(on, off, step)
    assert calls == dict(saving=0, loaded=0, ring=0), calls
    on.close()
    off.close()
