"""One step of torch's single-tensor Adam (torch/optim/adam.py `_single_tensor_adam`, no weight decay, no amsgrad) from an
arbitrary state, restated twice, and the inputs both are run on; shared by tests/test_adam_ref_host.py (CPU: `step64`
against `torch.optim.Adam` in float64) and tests/test_adam_float64_gpu.py (GPU: the float64 reference of `asac_adam_step`,
`asac_adam_step_partials` and `asac_alpha_adam_step`, and `eager` — `torch.optim.Adam` itself in float32 on the device —
the yardstick of `discrete_ref.over_the_bound`)."""
import numpy as np
import torch

from tests.discrete_ref import GUARD, SENTINEL

HYPER_DEFAULT = (3e-4, 0.9, 0.999, 1e-8)        # (lr, beta1, beta2, eps)
HYPER_COARSE = (0.1, 0.5, 0.9, 1e-3)
HYPERS = (HYPER_DEFAULT, HYPER_COARSE)
STEPS_DONE = (0, 1, 9, 999, 10 ** 6 - 1, 2 ** 24, 2 ** 31 + 4)
SCALES = (1e-6, 1., 1e4)


def as_float32(hyper):
    """the hyper-parameters as the C ABI receives them (float arguments), as Python floats"""
    return tuple(float(np.float32(x)) for x in hyper)


def step64(p, g, m, v, t, lr, b1, b2, eps):
    """float32 (or float64) arrays p, g, m, v; `t` the step being taken (steps done + 1) -> (p', m', v') in float64"""
    lr, b1, b2, eps = (np.float64(x) for x in as_float32((lr, b1, b2, eps)))
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    t = int(t)
    m1 = m + (1. - b1) * (g - m)
    v1 = b2 * v + (1. - b2) * g * g
    step_size = lr / (1. - b1 ** t)
    p1 = p - step_size * m1 / (np.sqrt(v1) / np.sqrt(1. - b2 ** t) + eps)
    return p1, m1, v1


def torch_adam(p, g, m, v, t, lr, b1, b2, eps, dtype, device):
    """the same step by `torch.optim.Adam([P], foreach=False)` in `dtype` on `device`, the state injected; the hyper-
    parameters are the float32-rounded ones.  The counter is injected as a float64 tensor: torch's own float32 one cannot
    hold 2^24 + 1.  -> (P, exp_avg, exp_avg_sq) afterwards as float64 numpy arrays"""
    lr, b1, b2, eps = as_float32((lr, b1, b2, eps))

    def tensor(x):
        return torch.as_tensor(np.ascontiguousarray(x)).to(device=device, dtype=dtype).clone()
    P = tensor(p).requires_grad_()
    P.grad = tensor(g)
    opt = torch.optim.Adam([P], lr=lr, betas=(b1, b2), eps=eps, foreach=False, fused=False, capturable=False)
    opt.state[P] = {'step': torch.tensor(float(t - 1), dtype=torch.float64), 'exp_avg': tensor(m), 'exp_avg_sq': tensor(v)}
    opt.step()
    state = opt.state[P]
    assert float(state['step']) == float(t)
    return tuple(x.detach().double().cpu().numpy() for x in (P, state['exp_avg'], state['exp_avg_sq']))


def eager(p, g, m, v, t, lr, b1, b2, eps):
    """the float32 yardstick: torch's own Adam on the device"""
    return torch_adam(p, g, m, v, t, lr, b1, b2, eps, torch.float32, 'cuda')


def draw(rng, n, scale):
    """n float32 values of one magnitude: sign * clip(|standard normal|, 0.1, 10) * scale.  Clipped from below so that no
    element is small beside its neighbours (Adam divides by sqrt(v): an element with g and v both near zero is ill-
    conditioned and would measure the inputs, not the kernel), from above so that 1e4 stays under 1e5"""
    x = rng.standard_normal(n)
    return (np.sign(x) * np.clip(np.abs(x), 0.1, 10.) * scale).astype(np.float32)


def make_state(rng, n, steps_done, scale, p_zero, all_zero=False):
    """(p, g, m, v) float32 of one case: g at `scale` with a few exact zeros, the moments zero at steps_done == 0 and at
    the gradient's scale otherwise (v as squares); `all_zero`: g = m = v = 0 throughout"""
    p = np.zeros(n, np.float32) if p_zero else rng.standard_normal(n).astype(np.float32)
    if all_zero:
        return p, np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    g = draw(rng, n, scale)
    g[rng.integers(0, n, size=min(5, n // 2))] = 0.
    if steps_done == 0:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m, v = draw(rng, n, scale), draw(rng, n, scale) ** 2
    nz = np.abs(g[g != 0])
    assert nz.size == 0 or (nz.min() >= 1e-7 and nz.max() <= 1e5)
    return p, g, m, v


def value_cases():
    """the section-3 value cases: (steps_done, scale, p_zero, hyper, all_zero)"""
    cases = [(done, scale, p_zero, hyper, False)
             for done in STEPS_DONE for scale in SCALES for p_zero in (False, True) for hyper in HYPERS]
    cases.append((9, 1., False, HYPER_DEFAULT, True))
    return cases


def partials_workspace(partial, loss_partial=None):
    """`asac_adam_step_partials`' workspace from partial [tiles, E, member_stride] (and loss_partial [tiles, E]): the
    parameter partials at [t E member_stride + e member_stride + local], the loss partials behind them at [t E + e]"""
    flat = np.ascontiguousarray(partial, dtype=np.float32).reshape(-1)
    if loss_partial is None:
        return flat
    assert loss_partial.shape == partial.shape[:2]
    return np.concatenate([flat, np.ascontiguousarray(loss_partial, dtype=np.float32).reshape(-1)])


def partials_gradient(xp, partial, grad, used, accumulate):
    """the gradient `asac_adam_step_partials` steps with and stores (csrc/optim.hip `k_adam_partials`): for local < used
    the tile sum (+ the stored gradient with `accumulate`), the stored gradient elsewhere; `xp`: numpy on float64 arrays
    (the reference) or torch on float32 device tensors (the eager composition).  partial [tiles, E, member_stride],
    grad [E member_stride]"""
    tiles, E, ms = partial.shape
    total = partial.sum(0).reshape(-1)
    if accumulate:
        total = grad + total
    local = xp.arange(E * ms) % ms
    if xp is torch:
        local = local.to(grad.device)
    return xp.where(local < used, total, grad)


class GuardedViews:
    """float32 device views with chosen contents, each inside a larger buffer with GUARD sentinels in front and behind
    (`discrete_ref.Guarded` for tensors that go in with values), `shift` floats further in than the 16-byte aligned place
    (shift = 1: a view no float4 access may touch); `check()`: every sentinel still has its bits"""

    def __init__(self):
        self.buffers = []

    def __call__(self, values, shift=0):
        values = torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32))
        n = values.numel()
        buf = torch.full((GUARD + shift + n + GUARD,), SENTINEL, device='cuda')
        view = buf[GUARD + shift:GUARD + shift + n]
        view.copy_(values.reshape(-1))
        assert view.data_ptr() % 16 == (4 * shift) % 16
        self.buffers.append((buf, GUARD + shift, n))
        return view

    def check(self):
        assert self.buffers
        bits = torch.tensor(SENTINEL).view(torch.int32).item()
        for i, (buf, lead, n) in enumerate(self.buffers):
            words = buf.view(torch.int32)
            assert bool((words[:lead] == bits).all()), f'buffer {i} ({n} floats): written in front of the view'
            assert bool((words[lead + n:] == bits).all()), f'buffer {i} ({n} floats): written behind the view'
