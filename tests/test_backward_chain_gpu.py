"""GPU: the headline step's two backward launches — `asac_policy_step_fused` (`k_policy_step`) and the 16-wave Q-loss
backward (`k_mlp_bwd<16, false, 3, RET, 16>`) — against a yardstick their source does not share a line of control flow
with: the GENERIC four-wave `k_mlp_bwd` chain (`asac_mlp_forward` -> `asac_mlp_backward_policy_q` ->
`asac_mlp_backward_policy_sample`, and `asac_mlp_backward_qloss`).  The generic form is reached for stock shapes by
handing the entry points the same parameters at an address that is not 16-byte aligned (`stock3` in csrc/mlp.hip then
says no and the launch takes `k_mlp_bwd<16, false, 0>`).  Everything the next launch reads must be bit-identical: the
per-tile partial slabs slab by slab, the value table, the loss partials, y, the input gradients.  A float64 restatement
of the same networks catches a yardstick and a kernel that are wrong together, at the bounds tests/test_fused_mlp_gpu.py
uses for the same quantities.  Shapes: the smallest at which these kernels can go wrong — no full tile, an exact tile, a
one-row tail, two tiles and a tail.  Residual flags: off everywhere / on wherever the widths allow (blocks 1 and 2; the
first block maps 6 + A inputs to 64 and cannot have one)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, E, CLIP = 6, 2, 0.2
SHAPES = [(N, A) for N in (1, 16, 17, 33) for A in (1, 2)] + [(17, 4)]
F = dict(device='cuda')


def _nets(A, residual, policy):
    """(aligned StockMLP: the stock kernels, misaligned twin on the same numbers: the generic ones, group)"""
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
    for l in (1, 2):
        desc.residual[l] = int(residual)
    group = FlatParamGroup([(f'm{i}', list(mod.parameters())) for i, mod in enumerate(mods)], 'cuda')
    stride = group.segments['m0'][1] - group.segments['m0'][0]
    n = len(mods)
    dev = torch.device('cuda')
    mlp = StockMLP(desc, group.flat, group.grad, 0, stride, n, dev)
    flat1 = torch.zeros(1 + n * stride, **F)
    flat1[1:] = group.flat[:n * stride]
    twin = StockMLP(desc, flat1, torch.zeros_like(flat1), 1, stride, n, dev)
    assert mlp.params.data_ptr() % 16 == 0 and twin.params.data_ptr() % 16 == 4
    mlp.accumulate = twin.accumulate = False
    return mlp, twin


def _gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _net64(P, desc, x):
    """the network of `desc` on float64 parameters P (one member) -> the raw head columns [N, O]"""
    h, K = x, desc.in0 + desc.in1
    for l in range(desc.n_blocks):
        W = desc.width[l]
        w = P[desc.w_off[l]:desc.w_off[l] + W * K].view(W, K)
        y = _gelu64(h @ w.T + P[desc.b_off[l]:desc.b_off[l] + W])
        h = y + h if desc.residual[l] else y
        K = W
    outs = []
    for k in range(2):
        O = desc.head_cols[k]
        if O:
            w = P[desc.head_w_off[k]:desc.head_w_off[k] + O * K].view(O, K)
            outs.append(h @ w.T + P[desc.head_b_off[k]:desc.head_b_off[k] + O])
    return torch.cat(outs, dim=1)


def _slabs(mlp, N):
    from asac_amd import native
    tiles, used = native.mlp_backward_tiles(N, mlp.E), native.mlp_param_extent(mlp.desc)
    return mlp._workspace[:tiles * mlp.E * mlp.member_stride].view(tiles, mlp.E, -1)[:, :, :used]


def _loss_partials(mlp, N):
    from asac_amd import native
    tiles = native.mlp_backward_tiles(N, mlp.E)
    base = tiles * mlp.E * mlp.member_stride
    return mlp._workspace[base:base + tiles * mlp.E].view(tiles, mlp.E)


def _close(got, want, rtol, atol, what):
    np.testing.assert_allclose(got.double().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=what)


@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('N,A', SHAPES)
def test_policy_step_in_one_launch_is_the_generic_four_wave_chain_bit_for_bit(N, A, residual):
    from asac_amd import native
    fq, tq_ = _nets(A, residual, policy=False)
    fpi, tpi = _nets(A, residual, policy=True)
    torch.manual_seed(100 * N + A)
    x = torch.randn(N, 3, S, **F)[:, 1]                  # strided rows
    eps = torch.randn(N, A, **F)
    log_alpha = torch.tensor(-0.7, **F)
    # ---- the yardstick: generic forward, sampling launch, generic backwards
    ls = tpi._launch_forward(x, None)[0]
    a, logp = torch.empty(N, A, **F), torch.empty(N, **F)
    native.squash_sample_fwd(ls[:, :A], ls[:, A:], eps, a, logp)
    q = tq_._launch_forward(x, a)
    ga = tq_.backward_policy_q(x, a, q.view(E, N), None, E)
    tpi._workspace_for(N).fill_(float('nan'))
    tpi.backward_policy_sample(x, eps, ga, log_alpha, defer=True)
    want = _slabs(tpi, N).clone()
    assert torch.isfinite(want).all()
    # ---- one launch, the action given and the action sampled inside; twice each into NaN-filled slabs
    assert fpi.policy_step_fused_ok(fq, N)
    for sampled in (False, True):
        runs = []
        for _ in range(2):
            q_out = torch.full((E, N, 1), float('nan'), **F)
            out = (torch.zeros(N, A, **F), torch.zeros(N, **F), torch.zeros(N, 2 * A, **F))
            fpi._workspace_for(N).fill_(float('nan'))
            fpi.policy_step_fused(fq, x, None if sampled else a, eps, log_alpha, q_out=q_out, defer=True,
                                  sample_out=out if sampled else None)
            runs.append((_slabs(fpi, N).clone(), q_out, out))
        (got, q_out, out), (again, q_again, _) = runs
        assert torch.isfinite(got).all(), 'a slab word of a live parameter was not written'
        assert torch.equal(got, again) and torch.equal(q_out, q_again), 'two launches differ'
        for t in range(got.shape[0]):
            assert torch.equal(got[t], want[t]), f'partial slab of tile {t} (sampled inside: {sampled})'
        assert torch.equal(q_out, q), 'value table'
        if sampled:
            assert torch.equal(out[0], a) and torch.equal(out[1], logp) and torch.equal(out[2], ls)
    # ---- float64 restatement of the same step
    dq, dp = fq.desc, fpi.desc
    Pq = [fq.params[e * fq.member_stride:(e + 1) * fq.member_stride].double() for e in range(E)]
    Pp = fpi.params.double().requires_grad_()
    x64, eps64, gl = x.double(), eps.double(), math.exp(-0.7) / N
    raw = _net64(Pp, dp, x64)
    loc, sc = 5.0 * torch.tanh(raw[:, :A] / 5.0), torch.exp(raw[:, A:].clamp(-20.0, 0.5))
    u = loc + eps64 * sc
    a64 = torch.tanh(u).detach().requires_grad_()
    q64 = torch.stack([_net64(Pq[e], dq, torch.cat([x64, a64], dim=1))[:, 0] for e in range(E)])
    (-q64.min(dim=0).values.sum() / N).backward()
    t = a64.detach()
    one_m = 1.0 - t * t
    gx = a64.grad * one_m + torch.where(one_m > 1e-2, gl * (A * 2.0 * t), torch.zeros_like(t))
    ((gx * u).sum() - gl * torch.log(sc).sum()).backward()
    _close(q_out[:, :, 0], q64, 2e-5, 2e-6, 'value table against float64')
    gp_scale = max(1.0, float(Pp.grad.abs().max()))
    used = want.shape[-1]
    _close(want.double().sum(dim=0)[0], Pp.grad[:used], 1e-4, 2e-5 * gp_scale, 'policy gradient against float64')


def _ret_args(nat, N, n, A, y):
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
    r.logp, r.log_alpha, r.E_sample = t['logp'].data_ptr(), t['log_alpha'].data_ptr(), E
    r.reward, r.reward_stride = t['reward'].data_ptr(), t['reward'].stride(0)
    r.done, r.last_mask, r.padding_mask, r.mask_stride = (t['done'].data_ptr(), t['last'].data_ptr(), t['pad'].data_ptr(),
                                                          t['done'].stride(0))
    r.mu_prob, r.mu_stride_b, r.mu_stride_t, r.mu_offset = t['mu'].data_ptr(), t['mu'].stride(0), t['mu'].stride(1), 0
    r.pi_prob, r.pi_stride_b, r.pi_stride_t, r.A = t['pi'].data_ptr(), t['pi'].stride(0), t['pi'].stride(1), A
    r.gamma_ratio, r.lambda_ratio = t['gr'].data_ptr(), t['lr'].data_ptr()
    r.gamma, r.v_rho, r.v_c, r.use_n_step_is, r.B, r.n = 0.99, 1.0, 1.0, 1, N, n
    r.y_out = y.data_ptr()
    return r, t          # (t keeps the tensors alive)


@pytest.mark.parametrize('state_grads', [False, True])
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('N,A', SHAPES)
def test_sixteen_wave_q_loss_backward_is_the_generic_four_wave_one_bit_for_bit(N, A, residual, state_grads):
    from asac_amd import native as nat
    fq, twin = _nets(A, residual, policy=False)
    torch.manual_seed(100 * N + A + 1)
    x, a = torch.randn(N, S, **F), torch.randn(N, A, **F).tanh()
    tq = torch.randn(E, N, **F) * 0.3
    w = torch.rand(N, **F) + 0.5
    n = 4
    y = torch.zeros(N, **F)
    r, keep = _ret_args(nat, N, n, A, y)
    nat.vtrace_return_min(r)                              # the return launch: y for the yardstick
    loss = torch.zeros(E, **F)

    def run(mlp, formed_inside):
        out = []
        for _ in range(2):
            mlp._workspace_for(N).fill_(float('nan'))
            if formed_inside:
                y_in = torch.full((N,), float('nan'), **F)
                r_in, keep_in = _ret_args(nat, N, n, A, y_in)
                assert mlp.backward_qloss_return_ok(N, r_in)
                g0 = mlp.backward_qloss_return(x, a, tq, r_in, w, CLIP, loss, defer=True, state_grads=state_grads)
            else:
                y_in = y
                g0 = mlp.backward_qloss(x, a, tq, y, w, CLIP, loss, defer=True, state_grads=state_grads)
            out.append((_slabs(mlp, N).clone(), _loss_partials(mlp, N).clone(), y_in.clone(), g0))
        (s0, l0, y0, g0), (s1, l1, y1, g1) = out
        assert torch.isfinite(s0).all() and torch.isfinite(l0).all(), 'a live slab / loss word was not written'
        assert torch.equal(s0, s1) and torch.equal(l0, l1) and torch.equal(y0, y1), 'two launches differ'
        assert g0 is None or torch.equal(g0, g1)
        return s0, l0, y0, g0

    want_s, want_l, _, want_g = run(twin, False)
    for formed_inside in (False, True):
        got_s, got_l, got_y, got_g = run(fq, formed_inside)
        for t in range(got_s.shape[0]):
            assert torch.equal(got_s[t], want_s[t]), f'partial slabs of tile {t} (return inside: {formed_inside})'
        assert torch.equal(got_l, want_l), 'loss partials'
        assert torch.equal(got_y, y), 'y'
        if state_grads:
            assert torch.equal(got_g, want_g), 'input gradients'
        else:
            assert got_g is None
    # ---- float64 restatement
    d = fq.desc
    x64 = x.double().requires_grad_()
    Ps = [fq.params[e * fq.member_stride:(e + 1) * fq.member_stride].double().requires_grad_() for e in range(E)]
    losses = []
    for e in range(E):
        q = _net64(Ps[e], d, torch.cat([x64, a.double()], dim=1))[:, 0]
        t64 = tq[e].double()
        l = torch.maximum((t64 + (q - t64).clamp(-CLIP, CLIP) - y.double()) ** 2, (q - y.double()) ** 2) * w.double()
        losses.append(l.mean())
    gx = [torch.autograd.grad(losses[e], x64, retain_graph=True)[0] for e in range(E)]
    torch.stack(losses).sum().backward()
    _close(want_l.double().sum(dim=0) / N, torch.stack(losses), 2e-5, 1e-6, 'loss against float64')
    used = want_s.shape[-1]
    for e in range(E):
        _close(want_s.double().sum(dim=0)[e], Ps[e].grad[:used], 2e-4, 2e-6, f'member {e} gradient against float64')
        if state_grads:
            _close(want_g[e], gx[e], 1e-4, 1e-5, f'member {e} input gradient against float64')
