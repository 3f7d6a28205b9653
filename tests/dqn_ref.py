"""Restatements of the DQN-like discrete learner's arithmetic on explicit tensors, shared by tests/test_dqn_host.py (CPU:
against the recorded reference function `tests/golden/f16_dqn_y.npz` and this repository's eager `get_dqn_like_d_y`) and
tests/test_dqn_gpu.py (GPU: the float64 reference of the `asac_dqn_*` kernels).  Formulas: include/asac_hip.h, the
section of the DQN-like learner.  Written index by index, not with the eager code's tensor operations: a second statement
of the same rule, not a copy of the first."""
import numpy as np
import torch

from tests.discrete_ref import _strided, as_numpy  # noqa: F401


def make_case(B, n, sizes, E, Es, weights, seed):
    """float32 CPU tensors of one case (`to(..., strided=True)` turns them into strided views).  Row 0 (B > 1) is wholly
    masked, row 1 has `done` at its L, row 2 has L = 0, row 3's stored action is all zeros.  Every L in [0, n) can occur
    among the other rows; `gamma` is a float32 value, so every path is handed the same number."""
    gen = torch.Generator().manual_seed(seed)
    K, D = len(sizes), sum(sizes)
    c = dict(B=B, n=n, sizes=tuple(sizes), K=K, D=D, E=E, Es=Es)

    def view(*shape):
        return torch.randn(*shape, generator=gen)
    c['q_eval'] = [view(B, n, D) for _ in range(E)]
    c['q_target'] = [view(B, n + 1, D) for _ in range(E)]
    c['q_online'] = [view(B, D) for _ in range(E)]
    c['action'] = torch.cat([torch.eye(s)[torch.randint(0, s, (B,), generator=gen)] for s in sizes], dim=-1)
    c['reward'] = view(B, n)
    c['done'], c['last'], c['pad'] = (m.clone() for m in torch.rand(3, B, n, generator=gen) < 0.25)
    if B > 1:
        c['pad'][0] = True
        c['last'][1], c['pad'][1] = False, False
        c['done'][1, n - 1] = True
    if B > 2:
        c['last'][2], c['pad'][2] = False, False
        c['pad'][2, 1:] = True
    if B > 3:
        c['action'][3] = 0.
    c['sub_n'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    c['sub_next'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    c['w'] = (torch.rand(B, 1, generator=gen) + 0.5) if weights else None
    c['gamma'] = float(np.float32(0.97))
    c['gamma_ratio'] = torch.logspace(0, n - 1, n, c['gamma'])
    return c


def tie_every_branch(c, seed):
    """exact ties in every branch of the eval values at every position: two or more equal maxima (values on a grid of
    three levels), so that the greedy index depends on the tie rule alone"""
    gen = torch.Generator().manual_seed(seed)
    for q in c['q_eval']:
        q.copy_(torch.randint(0, 3, q.shape, generator=gen).float() * 0.5)
    return c


def to(c, dtype, device, strided=False):
    """the case on `device` with its floating-point tensors as `dtype`; `strided`: every tensor with rows a strided view"""
    wrap = _strided if strided else (lambda t: t)
    out = {}
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            out[k] = wrap(v.to(device=device, dtype=dtype if v.is_floating_point() else v.dtype))
        elif isinstance(v, list):
            out[k] = [wrap(t.to(device=device, dtype=dtype)) for t in v]
        else:
            out[k] = v
    if strided:
        out['gamma_ratio'] = out['gamma_ratio'].contiguous()
    return out


def last_valid(last, pad):
    """[B, n] bool arrays -> L [B]: the largest t with !(last | pad), n - 1 where there is none"""
    gone = np.asarray(last) | np.asarray(pad)
    B, n = gone.shape
    L = np.full(B, n - 1, dtype=np.int64)
    for b in range(B):
        for t in range(n):
            if not gone[b, t]:
                L[b] = t
    return L


def greedy(values, sizes):
    """values [..., D] -> the index of the first maximum of each branch [..., K] (numpy argmax: the lowest index)"""
    values = np.asarray(values)
    out, j0 = [], 0
    for s in sizes:
        out.append(np.argmax(values[..., j0:j0 + s], axis=-1))
        j0 += s
    return np.stack(out, axis=-1)


def target_y(q_eval, q_target, sub_n, sub_next, reward, done, last, pad, gamma_ratio, gamma, sizes):
    """float64 y [B] of the double-DQN n-step target; q_eval [E, B, n, D], q_target [E, B, n+1, D] as arrays, the subsets
    index them and pair by position"""
    q_eval, q_target = np.asarray(q_eval, dtype=np.float64), np.asarray(q_target, dtype=np.float64)
    reward, gamma_ratio = np.asarray(reward, dtype=np.float64), np.asarray(gamma_ratio, dtype=np.float64)
    done = np.asarray(done)
    B, K = reward.shape[0], len(sizes)
    L = last_valid(last, pad)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    y = np.zeros(B)
    for b in range(B):
        v = np.inf
        for e_n, e_next in zip(np.asarray(sub_n), np.asarray(sub_next)):
            pick = greedy(q_eval[e_n, b, L[b]], sizes)
            v = min(v, sum(q_target[e_next, b, L[b] + 1, starts[k] + pick[k]] for k in range(K)) / K)
        y[b] = (gamma_ratio * reward[b]).sum() + float(gamma) ** int(L[b] + 1) * v * (0. if done[b, L[b]] else 1.)
    return y


def all_formulas(c):
    """the case (any dtype, CPU) -> float64 {'y' [B], 'td' [B], 'loss_q' [E], 'grad_q' [E, B, D]}"""
    f64 = lambda t: np.asarray(t.detach().cpu().double().numpy())    # noqa: E731
    B, K, E = c['B'], c['K'], c['E']
    y = target_y(np.stack([f64(t) for t in c['q_eval']]), np.stack([f64(t) for t in c['q_target']]),
                 c['sub_n'].cpu().numpy(), c['sub_next'].cpu().numpy(), f64(c['reward']), c['done'].cpu().numpy(),
                 c['last'].cpu().numpy(), c['pad'].cpu().numpy(), f64(c['gamma_ratio']), c['gamma'], c['sizes'])
    a = f64(c['action'])
    qs = np.stack([(a * f64(q)).sum(-1) / K for q in c['q_online']])              # [E, B]
    w = f64(c['w']).reshape(-1) if c['w'] is not None else np.ones(B)
    diff = qs - y[None, :]
    return {'y': y, 'td': np.abs(diff).mean(0), 'loss_q': (w[None, :] * diff ** 2).mean(1),
            'grad_q': (2. * w[None, :] * diff / (K * B))[:, :, None] * a[None, :, :] * np.ones((E, 1, 1))}


def eager(c, get_dqn_like_d_y):
    """today's torch code on the case's device and dtype: `get_dqn_like_d_y` (bound to a learner or a stand-in) plus the
    loss and TD lines of `_train_rep_q` / `_get_td_error` -> {'y', 'td', 'loss_q', 'grad_q'}"""
    K = c['K']
    ev = torch.stack(c['q_eval']).index_select(0, c['sub_n'].long())
    tg = torch.stack([t[:, 1:] for t in c['q_target']]).index_select(0, c['sub_next'].long())
    d_y = get_dqn_like_d_y(c['last'], c['pad'], c['reward'], c['done'], ev, tg)           # [B, 1]
    heads = [q.detach().clone().requires_grad_(True) for q in c['q_online']]
    qs = torch.stack([torch.sum(c['action'] * q, dim=-1, keepdim=True) / K for q in heads])
    losses = torch.nn.functional.mse_loss(qs, d_y.expand_as(qs), reduction='none')
    if c['w'] is not None:
        losses = losses * c['w'].unsqueeze(0)
    per_member = losses.mean(dim=(1, 2))
    per_member.sum().backward()
    td = torch.abs(qs.detach() - d_y).mean(dim=0).reshape(-1)
    return {'y': d_y.reshape(-1), 'td': td, 'loss_q': per_member.detach(), 'grad_q': torch.stack([h.grad for h in heads])}


def eager_stub(c, device):
    """what the eager `get_dqn_like_d_y` reads of its learner"""
    import types
    return types.SimpleNamespace(device=device, d_action_sizes=list(c['sizes']), d_action_branch_size=c['K'],
                                 gamma=c['gamma'], _gamma_ratio=c['gamma_ratio'])


def act(q, u, epsilon, sizes):
    """the acting rule on arrays: q [B, D] float32, u [B, 1+K] float32 or None -> the one-hot action [B, D] float32.
    Greedy: the first maximum per branch; rows with u[b, 0] < float32(epsilon): index min(floor(u[b, 1+k] * s_k), s_k - 1),
    the product formed in float32 as the kernel forms it."""
    q = np.asarray(q, dtype=np.float32)
    B, D = q.shape
    pick = greedy(q, sizes)
    if u is not None:
        u = np.asarray(u, dtype=np.float32)
        rows = u[:, 0] < np.float32(epsilon)
        for k, s in enumerate(sizes):
            rnd = np.minimum(np.floor(u[:, 1 + k] * np.float32(s)).astype(np.int64), s - 1)
            pick[:, k] = np.where(rows, rnd, pick[:, k])
    out, j0 = np.zeros((B, D), dtype=np.float32), 0
    for k, s in enumerate(sizes):
        out[np.arange(B), j0 + pick[:, k]] = 1.
        j0 += s
    return out
