"""The ordered cross-workgroup finish (csrc/asac_ordered_finish.h) of the six last-arriver kernels, checked through the
words it leaves behind: after a launch the workspace still holds every workgroup's partial, so the test owns a zeroed
workspace, reads the partials back and redoes the finish in NumPy float32 in the documented order.  The kernel's result must
have the same BITS: a partial the last arriver saw stale, a changed collection order or a missed workgroup all fail, and
nothing depends on how a transcendental rounds.  Every case also checks that the counter word is zero after the launch,
that a second launch on the same workspace gives the same bits, and that a hipGraph replay does (three replays, the outputs
reset in between).

`mse_mean_grad`: [128, 4, 2700] has 338 workgroups (a partly filled lane group of eight, lanes past the grid adding
zeros); the grid cap of 2 048 needs more than 2 047 * 4 096 floats, which [784, 4, 2700] has."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope='module')
def nat():
    from asac_amd import native
    native.load()
    assert torch.cuda.is_available()
    return native


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


def rnd(*shape, seed, lo=None, hi=None):
    g = torch.Generator(device='cuda').manual_seed(seed)
    if lo is None:
        return torch.randn(*shape, generator=g, device='cuda')
    return torch.rand(*shape, generator=g, device='cuda') * (hi - lo) + lo


def seq_sum(p):
    """p[0] + p[1] + ... in that order, every add rounded to float32"""
    s = F(0)
    for x in np.asarray(p, dtype=F):
        s = F(s + x)
    return s


def exercise(launch, outs, ws, counter_at, result, expected, reset=None):
    """launch(): one call of the entry point on `ws`; outs: every tensor it writes; result(): the tensor the finish wrote;
    expected(words): that result from the workspace's float32 words; reset(): the outputs' state before a launch"""
    if reset is None:
        def reset():
            for o in outs:
                o.zero_()
    reset()
    launch()
    torch.cuda.synchronize()
    words = ws.cpu().numpy()
    assert words.view(np.uint32)[counter_at] == 0, 'the arrival counter is left at zero'
    got, want = result().cpu().numpy(), expected(words)
    print('finish:', got.ravel()[:4], 'redone:', np.asarray(want).ravel()[:4])
    np.testing.assert_array_equal(bits(got), bits(want))
    first = [o.clone() for o in outs]

    def same():
        torch.cuda.synchronize()
        assert ws.cpu().numpy().view(np.uint32)[counter_at] == 0
        for o, f in zip(outs, first):
            np.testing.assert_array_equal(bits(o.cpu().numpy()), bits(f.cpu().numpy()))
    reset()
    launch()                                                 # the same workspace again
    same()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            launch()
        for _ in range(3):
            reset()
            graph.replay()
            same()
    torch.cuda.current_stream().wait_stream(stream)


B3, T3, K3 = 33, 7, 80                                       # 18 480 elements: 10 workgroups of 2 048


def test_masked_mse(nat):
    n = B3 * T3 * K3
    pred = rnd(B3, T3, K3, seed=1)
    target = rnd(B3, T3 + 5, K3, seed=2)[:, 5:]              # a strided slice of a window batch
    mask = rnd(B3, T3, seed=3, lo=0., hi=1.) < 0.25
    grad, loss = torch.empty_like(pred), torch.zeros((), device='cuda')
    ws = torch.zeros(nat.load().asac_masked_mse_workspace(n), device='cuda')
    nb = ws.numel() - 1
    assert nb == 10
    exercise(lambda: nat.masked_mse(pred, target, mask, grad, loss, workspace=ws), [loss, grad], ws, nb, lambda: loss,
             lambda w: F(seq_sum(w[:nb]) / F(n)))


@pytest.mark.parametrize('logstd', [False, True])
def test_normal_nll_kl(nat, logstd):
    n, kl_w = B3 * T3 * K3, 0.37
    target = rnd(B3, T3 + 5, K3, seed=4)[:, 5:]
    out = torch.zeros(2, device='cuda')
    ws = torch.zeros(nat.load().asac_normal_nll_kl_workspace(n), device='cuda')
    nb = (ws.numel() - 1) // 3
    assert nb == 10
    if logstd:
        raw = rnd(B3, T3, 2 * K3, seed=5)
        g_raw = torch.empty_like(raw)
        outs = [out, g_raw]

        def launch():
            nat.normal_nll_kl_logstd(raw, 0.1, 2.0, target, kl_w, g_raw, out, workspace=ws)
    else:
        loc, scale = rnd(B3, T3, K3, seed=6), rnd(B3, T3, K3, seed=7, lo=0.3, hi=2.0)
        g_loc, g_scale = torch.empty_like(loc), torch.empty_like(loc)
        outs = [out, g_loc, g_scale]

        def launch():
            nat.normal_nll_kl(loc, scale, target, kl_w, g_loc, g_scale, out, workspace=ws)

    def expected(w):
        inv_n = F(1) / F(n)
        a, b, e = (seq_sum(w[q:3 * nb:3]) for q in range(3))
        return np.array([F(-F(a * inv_n)) + F(F(kl_w) * F(b * inv_n)), F(e * inv_n)], dtype=F)
    exercise(launch, outs, ws, 3 * nb, lambda: out, expected)


@pytest.mark.parametrize('B, grid', [(16, 43), (128, 338), (784, 2048)])
def test_mse_mean_grad(nat, B, grid):
    T, K = 4, 2700
    n = B * T * K
    cap = nat.mse_mean_grad_workspace() - 1
    assert cap == 2048 and min(-(-(n // 4) // 1024), cap) == grid and (grid < cap or n // 4 > (cap - 1) * 1024)
    pred = rnd(B, T, K, seed=8)
    target = rnd(B, T + 5, K, seed=9)[:, 5:]
    grad, loss = torch.empty_like(pred), torch.zeros((), device='cuda')
    ws = torch.zeros(cap + 1, device='cuda')

    def expected(w):
        p = np.zeros(cap, dtype=F)
        p[:grid] = w[:grid]
        per = p.reshape(256, cap // 256)                     # lane t: partials 8 t .. 8 t + 7 in order
        red = np.zeros(256, dtype=F)
        for j in range(per.shape[1]):
            red = red + per[:, j]
        h = 128
        while h > 0:                                         # red[i] += red[i + h], h = 128, 64, .., 1
            red[:h] = red[:h] + red[h:2 * h]
            h //= 2
        return F(red[0] * (F(1) / F(n)))
    exercise(lambda: nat.mse_mean_grad(pred, target, grad, loss, ws), [loss, grad], ws, cap, lambda: loss, expected)


@pytest.mark.parametrize('Tp, A, grid', [(4096, 7, 28), (16384, 5, 64)])
@pytest.mark.parametrize('half', [False, True])
def test_bc_loss_grad(nat, Tp, A, grid, half):
    tv = Tp // 2 if half else Tp
    loc, scale = rnd(Tp, A, seed=10), rnd(Tp, A, seed=11, lo=0.3, hi=2.0)
    action = rnd(Tp, A + 2, seed=12)
    t_valid = torch.tensor([tv], dtype=torch.int32, device='cuda')
    loss, dloc, dscale = torch.zeros(1, device='cuda'), torch.empty_like(loc), torch.empty_like(loc)
    ws = torch.zeros(nat.load().asac_bc_loss_grad_workspace(), device='cuda')
    cap = ws.numel() - 4
    assert min(-(-(Tp * A) // 1024), cap) == grid
    exercise(lambda: nat.bc_loss_grad(loc, scale, action, 2, t_valid, 0.01, loss, dloc, dscale, workspace=ws),
             [loss, dloc, dscale], ws, cap, lambda: loss, lambda w: F(seq_sum(w[:grid]) / F(F(tv) * F(A))))


@pytest.mark.parametrize('B, grid', [(10000, 10), (70000, 64)])
@pytest.mark.parametrize('weighted', [False, True])
def test_termination_loss_grad(nat, B, grid, weighted):
    O = 4
    beta, y, v = rnd(B, 1, seed=13, lo=0., hi=1.), rnd(B, 1, seed=14), rnd(B, O, seed=15)
    done = rnd(B, seed=16, lo=0., hi=1.) < 0.2
    w_is = rnd(B, 1, seed=17, lo=0.2, hi=1.) if weighted else None
    loss, dbeta = torch.zeros(1, device='cuda'), torch.empty(B, device='cuda')
    ws = torch.zeros(nat.load().asac_termination_loss_grad_workspace(), device='cuda')
    cap = ws.numel() - 4
    assert min(-(-B // 1024), cap) == grid
    exercise(lambda: nat.termination_loss_grad(beta, y, v, done, w_is, 0.01, loss, dbeta, workspace=ws), [loss, dbeta], ws,
             cap, lambda: loss, lambda w: F(seq_sum(w[:grid]) / F(B)))


@pytest.mark.parametrize('accumulate', [False, True])
def test_linear_tanh_backward(nat, accumulate):
    N, K, O = 643, 18, 8                                     # 11 workgroups of 64 rows, 152 floats each: the in-launch tail
    nb, P = 11, O * (K + 1)
    x, weight, bias = rnd(N, K, seed=18), rnd(O, K, seed=19) * 0.3, rnd(O, seed=20) * 0.1
    y, grad_y = torch.empty(N, O, device='cuda'), rnd(N, O, seed=21)
    nat.linear_tanh_forward(x, weight, bias, y)
    grad_x, grad_p = torch.empty(N, K, device='cuda'), torch.empty(P, device='cuda')
    base = rnd(P, seed=22) if accumulate else torch.zeros(P, device='cuda')
    ws = torch.zeros(nat.linear_tanh_workspace(N, K, O), device='cuda')
    assert ws.numel() == nb * P + 1

    def reset():
        grad_x.zero_()
        grad_p.copy_(base)

    def expected(w):
        s = np.zeros(P, dtype=F)
        for slab in w[:nb * P].reshape(nb, P):               # one sum per gradient element, workgroups in order
            s = s + slab
        return base.cpu().numpy() + s if accumulate else s
    exercise(lambda: nat.linear_tanh_backward(x, weight, y, grad_y, grad_x, grad_p, accumulate, ws), [grad_p, grad_x], ws,
             nb * P, lambda: grad_p, expected, reset)
