"""A float64 restatement of the acting launch `asac_act_policy` (include/asac_hip.h, the section on acting; reference
sac_base.py `_choose_action` 931-966 and `_random_action` 858-880, operators.py `squash_correction_prob` 17-19) on explicit
arrays and explicit draws, shared by tests/test_act_host.py (CPU: against the recorded reference `tests/golden/f20_act.npz`
and `torch.linspace`) and tests/test_act_gpu.py (GPU: the reference of the kernel and of the learner's acting).  Written row
by row and branch by branch, not with the eager code's tensor operations: a second statement of the rule, not a copy.

Draw buffers (the layout of the header, mirrored by `native.act_draw_columns`), a group being absent when its condition fails:
    u    [K sampling columns: not deterministic] [1 gate column, K index columns: noise]        none without branches
    eps  [A sampling columns: not deterministic] [A noise columns: noise]                      none when A == 0
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
CLAMP = float(F32(0.999))            # torch.clamp(c_action, -0.999, 0.999) on a float32 tensor
SQUASH_FLOOR = float(F32(1e-2))
LOG_SQRT_2PI = 0.91893853320467274178


def draw_columns(K, A, deterministic, noise):
    nu = ((0 if deterministic else K) + ((1 + K) if noise else 0)) if K else 0
    ne = (0 if deterministic else A) + (A if noise else 0)
    return nu, ne


def _round_f32(x: Fraction) -> np.float32:
    """the float32 nearest to an exact rational (ties to even)"""
    d = F32(float(x))
    cands = [np.nextafter(d, F32(-np.inf)), d, np.nextafter(d, F32(np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(F32(c).view(np.uint32)) & 1))


def _fma_f32(a, b, c) -> np.float32:
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def noise_levels(lo, hi, B) -> np.ndarray:
    """`torch.linspace(lo, hi, B)` in float32, element by element: step = (hi - lo) / (B - 1); the lower half counts up from
    lo, the upper half down from hi, each with ONE rounding (a fused multiply-add); lo alone at B == 1"""
    lo, hi = F32(lo), F32(hi)
    if B == 1:
        return np.array([lo], dtype=F32)
    step = F32(F32(hi - lo) / F32(B - 1))
    out = np.empty(B, dtype=F32)
    for b in range(B):
        out[b] = _fma_f32(step, F32(b), lo) if b < B // 2 else _fma_f32(-step, F32(B - 1 - b), hi)
    return out


def head_bounding(mean, logstd):
    """the stock policy's (mean, logstd) -> (loc, scale) (reference nn_models/policy.py:170-172)"""
    mean, logstd = np.asarray(mean, dtype=np.float64), np.asarray(logstd, dtype=np.float64)
    return np.tanh(mean / 5.) * 5., np.exp(np.clip(logstd, -20., 0.5))


def softmax_branches(logits, sizes):
    """[B, D] -> the per-branch softmax [B, D], float64 (a -inf logit has probability exactly 0)"""
    z = np.asarray(logits, dtype=np.float64)
    p, j0 = np.zeros_like(z), 0
    for s in sizes:
        for b in range(z.shape[0]):
            row = z[b, j0:j0 + s]
            e = np.exp(row - row.max())
            p[b, j0:j0 + s] = e / e.sum()
        j0 += s
    return p


def density(action, loc, scale):
    """`squash_correction_prob` at the float32 action it is handed: x = atanh(clamp(a, +-0.999)),
    exp(N(loc, scale).log_prob(x_d)) / prod_e max(1 - tanh(x_e)^2, 1e-2); float64 [B, A]"""
    a = np.asarray(action, dtype=np.float64)
    loc, scale = np.asarray(loc, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    x = np.arctanh(np.clip(a, -CLAMP, CLAMP))
    jac = np.prod(np.maximum(1. - np.tanh(x) ** 2, SQUASH_FLOOR), axis=-1, keepdims=True)
    logp = -((x - loc) ** 2) / (2. * scale ** 2) - np.log(scale) - LOG_SQRT_2PI
    return np.exp(logp) / jac


def act(*, sizes=(), logits=None, loc=None, scale=None, head_raw=False, u=None, eps=None, deterministic=False, noise=None):
    """One call of the launch on arrays.  `sizes`: the discrete branches (may be empty) with logits [B, D]; loc, scale
    [B, A] or None (`head_raw`: they hold (mean, logstd)); u, eps: float32 draws in the layout above; noise: None or
    (lo, hi).  -> dict:
        index [B, K] int64, onehot [B, D] float32, p [B, D] float64, a [B, A] float64, loc / scale [B, A] float64,
        level [B] float32 (the rows' noise levels),
        margin: the smallest distance of any uniform that decided an index from the boundary it was compared with (a CDF
                boundary, the row's noise level, a multiple of 1 / s_k), `close` [B] bool the rows below `MIN_MARGIN`.
    The continuous action under noise passes through float32 before `atanh`, as the reference's does (`_random_action`
    is handed the float32 action): a = tanh(atanh(float32(a)) + eps_noise * level)."""
    sizes = tuple(int(s) for s in sizes)
    K, D = len(sizes), sum(sizes)
    A = 0 if loc is None else np.asarray(loc).shape[1]
    B = np.asarray(logits).shape[0] if K else np.asarray(loc).shape[0]
    nu, ne = draw_columns(K, A, deterministic, noise is not None)
    if nu:
        u = np.asarray(u, dtype=F32)
        assert u.shape == (B, nu), (u.shape, (B, nu))
    if ne:
        eps = np.asarray(eps, dtype=F32)
        assert eps.shape == (B, ne), (eps.shape, (B, ne))
    level = noise_levels(noise[0], noise[1], B) if noise is not None else np.zeros(B, dtype=F32)
    out = dict(level=level, margin=np.inf, close=np.zeros(B, dtype=bool))

    def near(b, dist):
        out['margin'] = min(out['margin'], float(dist))
        if dist < MIN_MARGIN:
            out['close'][b] = True

    if K:
        z = np.asarray(logits, dtype=np.float64)
        p = softmax_branches(z, sizes)
        index = np.zeros((B, K), dtype=np.int64)
        gate = 0 if deterministic else K
        for b in range(B):
            random = False
            if noise is not None:
                random = bool(u[b, gate] < level[b])
                near(b, abs(float(u[b, gate]) - float(level[b])))
            j0 = 0
            for k, s in enumerate(sizes):
                if random:
                    v = float(u[b, gate + 1 + k])
                    index[b, k] = min(int(np.floor(v * s)), s - 1)
                    if s > 1:
                        near(b, min(abs(v - i / s) for i in range(1, s)))
                elif deterministic:
                    index[b, k] = int(np.argmax(z[b, j0:j0 + s]))        # numpy argmax: the first maximum
                else:
                    v, pk = float(u[b, k]), p[b, j0:j0 + s]
                    c = np.cumsum(pk)
                    idx = int(sum(1 for i in range(s - 1) if c[i] <= v))
                    last = max(i for i in range(s) if pk[i] > 0.)
                    index[b, k] = min(idx, last)
                    # the boundaries that can move the index: not a running sum of exactly 0 (masked leading entries: every
                    # u >= 0 passes it on both sides), not those from the last positive entry on (the clamp decides there)
                    edges = [c[i] for i in range(last) if c[i] > 0.]
                    if edges:
                        near(b, min(abs(v - e) for e in edges))
                j0 += s
        onehot, j0 = np.zeros((B, D), dtype=F32), 0
        for k, s in enumerate(sizes):
            onehot[np.arange(B), j0 + index[:, k]] = 1.
            j0 += s
        out.update(index=index, onehot=onehot, p=p)
    if A:
        l, sc = (head_bounding(loc, scale) if head_raw else
                 (np.asarray(loc, dtype=np.float64), np.asarray(scale, dtype=np.float64)))
        a = np.tanh(l) if deterministic else np.tanh(l + eps[:, :A].astype(np.float64) * sc)
        if noise is not None:
            en = eps[:, (0 if deterministic else A):].astype(np.float64)
            with np.errstate(divide='ignore'):
                a = np.tanh(np.arctanh(a.astype(F32).astype(np.float64)) + en * level.astype(np.float64)[:, None])
        out.update(a=a, loc=l, scale=sc)
    return out


MIN_MARGIN = 1e-5


def redraw_close(rng, make_u, **case):
    """uniforms for `case` that keep every deciding comparison at least `MIN_MARGIN` from its boundary in the float64
    reference: rows that do not are drawn again (never the other rows) -> (u, the reference's result on it)"""
    u = make_u(rng)
    for _ in range(100):
        ref = act(u=u, **case)
        if not ref['close'].any():
            return u, ref
        fresh = make_u(rng)
        u[ref['close']] = fresh[ref['close']]
    raise AssertionError('no draw keeps the margin')
