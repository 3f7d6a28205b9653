"""Restatements of the three launches of random network distillation for a pure-discrete, policy-based learner
(`asac_drnd_distill`, `asac_drnd_param_grads`, `asac_drnd_pick`: include/asac_hip.h) in float64 on explicit arrays, shared
by tests/test_drnd_host.py (CPU: against float64 autograd on the module code and the recorded reference function
`tests/golden/f18_drnd_pick.npz`) and tests/test_drnd_gpu.py (GPU: the float64 reference of the kernels).  Written row by
row from the formulas; one stack is tests/rnd_ref.py's `stack_row` (in = S, no action columns).

The action contract: per row and branch the selected member is the FIRST non-zero element of the branch, its value the
weight w; a branch without a non-zero element selects nothing.

The candidate rule, shared with the device: a candidate's index in a branch of s entries is #{i < s - 1 : c_i <= u} with
c_i the running FLOAT32 sum of the branch softmax in index order."""
import numpy as np
import torch

from tests import rnd_ref as rr

WIDTH = rr.WIDTH


def offsets(sizes):
    return [int(sum(sizes[:j])) for j in range(len(sizes))]


def residual_flags(S):
    return rr.residual_flags(S)


def select(action_row, sizes):
    """one action row [>= D] -> [(member, weight) | (-1, 0.)] per branch"""
    out = []
    for first, s in zip(offsets(sizes), sizes):
        hit = (-1, 0.)
        for i in range(s):
            if action_row[first + i] != 0:
                hit = (first + i, float(action_row[first + i]))
                break
        out.append(hit)
    return out


def distill(state, action, pad, sizes, preds, targs, flags=None):
    """state [B, n, S], action [B, n, D], pad [B, n] bool or None, the D members' float64 parameters of predictor and target
    -> dict(loss, sel [N, K], x [N, S], h1 / gz1 / gz2 [N, K, 64], dw1 [D, 64, S], db1 [D, 64], dw2 [D, 64, 64], db2 [D, 64]).
    Padded rows select nothing."""
    state, action = np.asarray(state, dtype=np.float64), np.asarray(action, dtype=np.float64)
    B, n, S = state.shape
    K, D, N = len(sizes), int(sum(sizes)), B * n
    flags = residual_flags(S) if flags is None else flags
    out = dict(sel=np.full((N, K), -1, dtype=np.int64), x=np.zeros((N, S)), h1=np.zeros((N, K, WIDTH)),
               gz1=np.zeros((N, K, WIDTH)), gz2=np.zeros((N, K, WIDTH)))
    total = 0.
    for b in range(B):
        for t in range(n):
            r = b * n + t
            x = state[b, t]
            out['x'][r] = x
            if pad is not None and bool(pad[b, t]):
                continue
            chosen = select(action[b, t], sizes)
            d, fwd = np.zeros(WIDTH), {}
            for j, (m, w) in enumerate(chosen):
                if m < 0:
                    continue
                fwd[j] = rr.stack_row(preds[m], x, flags)
                d = d + w * (fwd[j][0] - rr.stack_row(targs[m], x, flags)[0])
            total += float(np.sum(d * d))
            for j, (m, w) in enumerate(chosen):
                if m < 0:
                    continue
                _, h1, z1, z2 = fwd[j]
                g = w * (2. * d / (N * WIDTH))
                gz2 = g * rr.gelu_grad(z2)
                gh1 = (g if flags[1] else 0.) + gz2 @ preds[m][2]
                out['sel'][r, j], out['h1'][r, j], out['gz2'][r, j], out['gz1'][r, j] = m, h1, gz2, gh1 * rr.gelu_grad(z1)
    out['loss'] = np.array(total / (N * WIDTH))
    out.update(param_grads(out['sel'], out['x'], out['h1'], out['gz1'], out['gz2'], sizes))
    return out


def param_grads(sel, x, h1, gz1, gz2, sizes):
    """the records -> the D members' gradients (sums over the rows that selected the member)"""
    D, S = int(sum(sizes)), x.shape[1]
    out = dict(dw1=np.zeros((D, WIDTH, S)), db1=np.zeros((D, WIDTH)), dw2=np.zeros((D, WIDTH, WIDTH)), db2=np.zeros((D, WIDTH)))
    for j, (first, s) in enumerate(zip(offsets(sizes), sizes)):
        for m in range(first, first + s):
            rows = np.nonzero(sel[:, j] == m)[0]
            a2, a1 = np.asarray(gz2, dtype=np.float64)[rows, j], np.asarray(gz1, dtype=np.float64)[rows, j]
            out['dw2'][m], out['db2'][m] = a2.T @ np.asarray(h1, dtype=np.float64)[rows, j], a2.sum(0)
            out['dw1'][m], out['db1'][m] = a1.T @ np.asarray(x, dtype=np.float64)[rows], a1.sum(0)
    return out


# ------------------------------------------------------------------------------------------------
def branch_probs(logits, sizes, dtype=np.float64):
    """the branch softmax [batch, D]: exp(z - max) / sum, per branch"""
    z = np.asarray(logits, dtype=dtype)
    out = np.zeros_like(z)
    for first, s in zip(offsets(sizes), sizes):
        part = z[:, first:first + s]
        e = np.exp(part - part.max(axis=1, keepdims=True))
        out[:, first:first + s] = e / e.sum(axis=1, keepdims=True, dtype=dtype)
    return out


def inverse_cdf(p, u):
    """p: one branch's probabilities; -> #{i < s - 1 : c_i <= u}, c the running float32 sum"""
    c, idx = np.float32(0.), 0
    for i in range(len(p) - 1):
        c = np.float32(c + np.float32(p[i]))
        idx += 1 if c <= np.float32(u) else 0
    return idx


def candidate_indices(logits, sizes, u):
    """logits [batch, D], u [batch, k, K] -> the candidates' index per branch [batch, k, K]"""
    p = branch_probs(logits, sizes, np.float32)
    batch, k, K = np.asarray(u).shape
    out = np.zeros((batch, k, K), dtype=np.int64)
    for b in range(batch):
        for j, (first, s) in enumerate(zip(offsets(sizes), sizes)):
            for c in range(k):
                out[b, c, j] = inverse_cdf(p[b, first:first + s], u[b, c, j])
    return out


def midpoint_uniforms(logits, sizes, cand):
    """the uniforms that reproduce recorded candidate indices: the midpoint of each index's CDF interval (float64) ->
    (u [batch, k, K] float32, the narrowest interval used)"""
    p = branch_probs(logits, sizes)
    batch, k, K = cand.shape
    u, narrow = np.zeros((batch, k, K), dtype=np.float32), 1.
    for j, (first, s) in enumerate(zip(offsets(sizes), sizes)):
        edges = np.concatenate([np.zeros((batch, 1)), np.cumsum(p[:, first:first + s], axis=1)], axis=1)
        edges[:, -1] = 1.
        for b in range(batch):
            for c in range(k):
                i = int(cand[b, c, j])
                u[b, c, j] = 0.5 * (edges[b, i] + edges[b, i + 1])
                narrow = min(narrow, float(edges[b, i + 1] - edges[b, i]))
    return u, narrow


def member_diffs(state, preds, targs, flags=None):
    """state [batch, S] -> E [batch, D, 64] = P_m(x) - T_m(x)"""
    state = np.asarray(state, dtype=np.float64)
    flags = residual_flags(state.shape[1]) if flags is None else flags
    return np.array([[rr.stack_row(p, x, flags)[0] - rr.stack_row(t, x, flags)[0] for p, t in zip(preds, targs)] for x in state])


def one_hot(idx, sizes):
    """[..., K] indices -> [..., D] one-hot per branch"""
    idx = np.asarray(idx)
    out = np.zeros((*idx.shape[:-1], int(sum(sizes))))
    for j, first in enumerate(offsets(sizes)):
        np.put_along_axis(out, (first + idx[..., j])[..., None], 1., axis=-1)
    return out


def pick(state, logits, u, sizes, preds, targs, flags=None, cand=None):
    """-> dict(cand [batch, k, K], err [batch, k], index [batch], action [batch, D], prob [batch, D]); `cand`: the
    candidates' indices where they are given (recorded) instead of formed from `u`"""
    cand = candidate_indices(logits, sizes, u) if cand is None else np.asarray(cand, dtype=np.int64)
    batch, k, K = cand.shape
    E = member_diffs(state, preds, targs, flags)
    off = np.asarray(offsets(sizes))
    err = np.zeros((batch, k))
    for b in range(batch):
        for c in range(k):
            s = np.zeros(WIDTH)
            for j in range(K):
                s = s + E[b, off[j] + cand[b, c, j]]
            err[b, c] = float(np.sum(s * s))
    index = np.array([rr.first_argmax(err[b]) for b in range(batch)], dtype=np.int64)
    action = one_hot(cand[np.arange(batch), index], sizes)
    return dict(cand=cand, err=err, index=index, action=action, prob=branch_probs(logits, sizes))


def margin(err, cand):
    """per row, (largest error - largest error among the candidates with ANOTHER action) / largest error; inf where every
    candidate is the same action (identical candidates tie exactly and the first wins)"""
    err, cand = np.asarray(err, dtype=np.float64), np.asarray(cand)
    out = np.full(err.shape[0], np.inf)
    for b in range(err.shape[0]):
        best = rr.first_argmax(err[b])
        other = [err[b, c] for c in range(err.shape[1]) if not np.array_equal(cand[b, c], cand[b, best])]
        if other:
            out[b] = (err[b, best] - max(other)) / err[b, best]
    return out


# ------------------------------------------------------------------------------------------------
# cases for the kernels
# ------------------------------------------------------------------------------------------------
def make_members(S, D, gen):
    """float32 parameters of D stock stacks  S -> 64 -> 64"""
    return [rr.make_stack(S, 0, gen) for _ in range(D)]


def as64(members):
    return [tuple(t.double().numpy() for t in m) for m in members]


def make_distill_case(B, n, S, sizes, seed):
    """float32 CPU tensors: state, one-hot action, pad, both member lists.  With B > 1 entry B // 2 is wholly padded and its
    action rows are all zero, and one live row ((B // 2 + 1) % B, 0) has an all-zero first branch; with B == 1 the only
    entry is live at every position (a single live row is computed); no row selects the last member."""
    gen = torch.Generator().manual_seed(seed)
    K, D = len(sizes), int(sum(sizes))
    c = dict(B=B, n=n, S=S, sizes=tuple(sizes))
    c['state'] = torch.randn(B, n, S, generator=gen)
    idx = torch.stack([torch.randint(0, max(1, s - 1) if j == K - 1 else s, (B, n), generator=gen) for j, s in enumerate(sizes)], -1)
    c['action'] = torch.from_numpy(one_hot(idx.numpy(), sizes)).float()
    c['pad'] = torch.rand(B, n, generator=gen) < 0.2
    if B == 1:
        c['pad'][:] = False
    else:
        c['pad'][B // 2] = True
        c['action'][B // 2] = 0.
        b = (B // 2 + 1) % B
        c['pad'][b, 0] = False
        c['action'][b, 0, :sizes[0]] = 0.
    c['pred'], c['targ'] = make_members(S, D, gen), make_members(S, D, gen)
    return c


def make_pick_case(batch, k, S, sizes, seed, guard=1e-4):
    """state, logits, uniforms, both member lists; a uniform closer than `guard` to an edge of its branch's CDF (float64) is
    moved to the middle of its interval, so float32 rounding of the running sum cannot move a candidate"""
    gen = torch.Generator().manual_seed(seed)
    K, D = len(sizes), int(sum(sizes))
    c = dict(batch=batch, k=k, S=S, sizes=tuple(sizes))
    c['state'] = torch.randn(batch, S, generator=gen)
    c['logits'] = 1.5 * torch.randn(batch, D, generator=gen)
    u = torch.rand(batch, k, K, generator=gen).numpy().astype(np.float64)
    p = branch_probs(c['logits'].numpy(), sizes)
    for j, (first, s) in enumerate(zip(offsets(sizes), sizes)):
        edges = np.concatenate([np.zeros((batch, 1)), np.cumsum(p[:, first:first + s], axis=1)], axis=1)
        edges[:, -1] = 1.
        for b in range(batch):
            for cc in range(k):
                if np.abs(edges[b] - u[b, cc, j]).min() < guard:
                    i = int(np.searchsorted(edges[b], u[b, cc, j], side='right')) - 1
                    i = min(max(i, 0), s - 1)
                    u[b, cc, j] = 0.5 * (edges[b, i] + edges[b, i + 1])
    c['u'] = torch.from_numpy(u.astype(np.float32))
    c['pred'], c['targ'] = make_members(S, D, gen), make_members(S, D, gen)
    return c
