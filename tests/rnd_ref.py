"""Restatements of the two random-network-distillation launches (`asac_rnd_distill`, `asac_rnd_pick`: include/asac_hip.h,
the RND section) in float64 on explicit arrays, shared by tests/test_rnd_host.py (CPU: against the recorded reference
function `tests/golden/f17_rnd_pick.npz` and float64 autograd on the module code) and tests/test_rnd_gpu.py (GPU: the float64
reference of the kernels).  Written row by row and feature by feature from the formulas, not with the module code's tensor
operations: a second statement of the same rule, not a copy of the first."""
import math

import numpy as np
import torch

WIDTH = 64
_erf = np.frompyfunc(math.erf, 1, 1)


def gelu(z):
    """z Phi(z), the erf form, elementwise on a float64 array"""
    z = np.asarray(z, dtype=np.float64)
    return z * 0.5 * (1. + _erf(z / math.sqrt(2.)).astype(np.float64))


def gelu_grad(z):
    z = np.asarray(z, dtype=np.float64)
    return 0.5 * (1. + _erf(z / math.sqrt(2.)).astype(np.float64)) + z * np.exp(-0.5 * z * z) / math.sqrt(2. * math.pi)


def stack_params(state_dict, prefix='c_dense.'):
    """the four parameter arrays of `ModelRND.c_dense` out of a state dict (tensors or arrays) -> float64 (w1, b1, w2, b2)"""
    get = lambda k: np.asarray(state_dict[prefix + k], dtype=np.float64)      # noqa: E731
    return (get('dense.0.linear.weight'), get('dense.0.linear.bias'), get('dense.2.linear.weight'), get('dense.2.linear.bias'))


def residual_flags(in_width):
    """(r1, r2) of the stock stack: a ResBlock adds its input whenever the widths agree"""
    return in_width == WIDTH, True


def stack_row(params, x, flags):
    """one row through one stack -> (p, h1, z1, z2)"""
    w1, b1, w2, b2 = params
    r1, r2 = flags
    z1 = np.array([b1[f] + np.dot(w1[f], x) for f in range(WIDTH)])
    h1 = gelu(z1) + (x if r1 else 0.)
    z2 = np.array([b2[f] + np.dot(w2[f], h1) for f in range(WIDTH)])
    p = gelu(z2) + (h1 if r2 else 0.)
    return p, h1, z1, z2


def distill(state, action, pad, pred, targ, flags=None):
    """state [B, n, S], action [B, n, A], pad [B, n] bool or None, the two stacks' float64 parameters ->
    dict(loss, h1, gz1, gz2 [N, 64], x_cat [N, S + A], dw1, db1, dw2, db2)"""
    state, action = np.asarray(state, dtype=np.float64), np.asarray(action, dtype=np.float64)
    B, n, S = state.shape
    A = action.shape[2]
    N, K = B * n, S + A
    flags = residual_flags(K) if flags is None else flags
    out = dict(x_cat=np.zeros((N, K)), h1=np.zeros((N, WIDTH)), gz1=np.zeros((N, WIDTH)), gz2=np.zeros((N, WIDTH)))
    w2 = pred[2]
    total = 0.
    for b in range(B):
        for t in range(n):
            r = b * n + t
            x = np.concatenate([state[b, t], action[b, t]])
            p, h1, z1, z2 = stack_row(pred, x, flags)
            tp = stack_row(targ, x, flags)[0]
            keep = 0. if (pad is not None and bool(pad[b, t])) else 1.
            d = (p - tp) * keep
            total += float(np.sum(d * d))
            g = 2. * d / (N * WIDTH)
            gz2 = g * gelu_grad(z2)
            gh1 = (g if flags[1] else 0.) + np.array([np.dot(gz2, w2[:, k]) for k in range(WIDTH)])
            gz1 = gh1 * gelu_grad(z1)
            out['x_cat'][r], out['h1'][r], out['gz1'][r], out['gz2'][r] = x, h1, gz1, gz2
    out['loss'] = np.array(total / (N * WIDTH))
    # the predictor's gradients: products over the rows
    out['dw2'] = np.array([[np.dot(out['gz2'][:, f], out['h1'][:, k]) for k in range(WIDTH)] for f in range(WIDTH)])
    out['db2'] = out['gz2'].sum(0)
    out['dw1'] = np.array([[np.dot(out['gz1'][:, f], out['x_cat'][:, k]) for k in range(K)] for f in range(WIDTH)])
    out['db1'] = out['gz1'].sum(0)
    return out


def candidates(loc, scale, eps):
    """[batch, A], [batch, A], [batch, k, A] -> tanh(loc + scale * eps_j) [batch, k, A] (float64)"""
    loc, scale, eps = (np.asarray(t, dtype=np.float64) for t in (loc, scale, eps))
    return np.tanh(loc[:, None, :] + scale[:, None, :] * eps)


def first_argmax(v):
    """torch.argmax on a 1-D array: the lowest index of the maximum, NaN the largest value"""
    best = 0
    for j in range(1, len(v)):
        if v[j] > v[best] or (np.isnan(v[j]) and not np.isnan(v[best])):
            best = j
    return best


def squash_prob(loc, scale, a):
    """the squash-corrected density of one action row under Normal(loc, scale):
    exp(N(x_d).log_prob) / prod_e max(1 - tanh(x_e)^2, 1e-2),  x = atanh(clamp(a, +-0.999))"""
    x = np.arctanh(np.clip(np.asarray(a, dtype=np.float64), -0.999, 0.999))
    jac = 1.
    for e in range(len(x)):
        jac *= max(1. - math.tanh(x[e]) ** 2, 1e-2)
    logp = -((x - loc) ** 2) / (2. * scale ** 2) - np.log(scale) - math.log(math.sqrt(2. * math.pi))
    return np.exp(logp) / jac


def pick(state, loc, scale, eps, pred, targ, flags=None, cand=None):
    """-> dict(err [batch, k], index [batch], action [batch, A], prob [batch, A]); `cand`: the candidates' squashed actions
    where they are given (float32 values of the device) instead of formed here"""
    state, loc, scale = (np.asarray(t, dtype=np.float64) for t in (state, loc, scale))
    batch, k, A = np.asarray(eps).shape
    flags = residual_flags(state.shape[1] + A) if flags is None else flags
    cand = candidates(loc, scale, eps) if cand is None else np.asarray(cand, dtype=np.float64)
    err = np.zeros((batch, k))
    for b in range(batch):
        for j in range(k):
            x = np.concatenate([state[b], cand[b, j]])
            d = stack_row(pred, x, flags)[0] - stack_row(targ, x, flags)[0]
            err[b, j] = float(np.sum(d * d))
    index = np.array([first_argmax(err[b]) for b in range(batch)], dtype=np.int64)
    action = cand[np.arange(batch), index]
    prob = np.stack([squash_prob(loc[b], scale[b], action[b]) for b in range(batch)])
    return dict(err=err, index=index, action=action, prob=prob)


def margin(err):
    """per row, (largest - second largest error) / largest; inf for a single candidate"""
    err = np.asarray(err, dtype=np.float64)
    if err.shape[1] < 2:
        return np.full(err.shape[0], np.inf)
    top = np.sort(err, axis=1)
    return (top[:, -1] - top[:, -2]) / top[:, -1]


# ------------------------------------------------------------------------------------------------
# cases for the kernels
# ------------------------------------------------------------------------------------------------
def make_stack(S, A, gen, scale=1.):
    """float32 parameters of one stock stack, Kaiming-uniform-like weights and non-zero biases -> (w1, b1, w2, b2)"""
    K = S + A
    u = lambda *shape: torch.rand(*shape, generator=gen) * 2. - 1.       # noqa: E731
    return (u(WIDTH, K) * math.sqrt(6. / K) * scale, 0.1 * u(WIDTH), u(WIDTH, WIDTH) * math.sqrt(6. / WIDTH) * scale,
            0.1 * u(WIDTH))


def make_distill_case(B, n, S, A, seed):
    """float32 CPU tensors: state, action, pad (one wholly padded row of B, other entries padded at random), the two stacks"""
    gen = torch.Generator().manual_seed(seed)
    c = dict(B=B, n=n, S=S, A=A)
    c['state'] = torch.randn(B, n, S, generator=gen)
    c['action'] = torch.tanh(torch.randn(B, n, A, generator=gen))
    c['pad'] = torch.rand(B, n, generator=gen) < 0.2
    c['pad'][B // 2] = True                        # one wholly padded row
    c['pred'], c['targ'] = make_stack(S, A, gen), make_stack(S, A, gen)
    return c


def strided(t, extra=3):
    """a view of `t` whose rows lie `extra` elements further apart than they need to (last dim dense)"""
    big = torch.full((*t.shape[:-1], t.shape[-1] + extra), float('nan') if t.is_floating_point() else 1, dtype=t.dtype,
                     device=t.device)
    big[..., :t.shape[-1]] = t
    return big[..., :t.shape[-1]]
