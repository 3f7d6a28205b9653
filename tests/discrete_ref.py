"""Restatements of the pure-discrete, policy-based learner's arithmetic on explicit tensors, shared by
tests/test_discrete_host.py (CPU: against `oracle.sac_ref.SacRef`) and tests/test_discrete_gpu.py (GPU: the float64
reference of the `asac_discrete_*` kernels, and — the same torch code in float32 on the device — the eager composition
the learner runs without them).  Formulas: oracle/sac_ref.py:334-348 (`get_y`), 379-382 (`train_rep_q`), 459-468
(`train_policy`), 491-494 (`train_alpha`), 547-548 (`td_error`), 106-121 (`v_trace`)."""
import numpy as np
import torch

from algorithm.nn_models.policy import JointOneHotCategorical


def joint_policy(logits, sizes):
    return JointOneHotCategorical([torch.distributions.OneHotCategorical(logits=part, validate_args=False)
                                   for part in logits.split(list(sizes), dim=-1)])


def make_case(B, n, sizes, E, Es, use_is, weights, seed, spread=1.0):
    """float32 CPU tensors of one case (`to(..., strided=True)` turns them into strided views).  Row 0 (B > 1) is wholly
    padded, row 1 has `done` at t = 0, row 2's stored action at t = 0 is all zeros.  `spread`: logits are
    `spread * standard normal` (1: ordinary; the saturated case places them on a +-30 grid itself)."""
    gen = torch.Generator().manual_seed(seed)
    K, D = len(sizes), sum(sizes)
    c = dict(B=B, n=n, sizes=tuple(sizes), K=K, D=D, E=E, Es=Es, use_is=use_is)

    def view(*shape):
        return torch.randn(*shape, generator=gen)
    c['logits'] = view(B, n + 1, D) * spread
    c['q_target'] = [view(B, n + 1, D) for _ in range(E)]
    c['q_online'] = [view(B, D) for _ in range(E)]
    c['logits0'] = view(B, D) * spread                    # the step's state (policy / temperature step)
    act = torch.cat([torch.eye(s)[torch.randint(0, s, (B, n + 1), generator=gen)] for s in sizes], dim=-1)
    c['action'] = act
    c['mu'] = view(B, n, D).abs().clamp(min=0.05, max=1.)     # behaviour probabilities [B, n, D]
    c['mu0'] = torch.softmax(view(B, D), dim=-1)
    c['reward'] = view(B, n)
    c['done'], c['last'], c['pad'] = (m for m in torch.rand(3, B, n, generator=gen) < 0.25)
    if B > 1:
        c['pad'][0] = True
        c['done'][1, 0] = True
    if B > 2:
        c['action'][2, 0] = 0.
    c['sub_n'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    c['sub_next'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    c['sub_pi'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    c['log_alpha'] = torch.tensor(-0.7)
    c['w'] = (torch.rand(B, 1, generator=gen) + 0.5) if weights else None
    c['y'] = view(B, 1)
    c['gamma'], c['v_rho'], c['v_c'], c['penalty'] = 0.97, 1.0, 0.9, 0.5
    c['gamma_ratio'] = torch.logspace(0, n - 1, n, c['gamma'])
    c['lambda_ratio'] = torch.logspace(0, n - 1, n, 0.95)
    s = torch.tensor(sizes)
    c['target'] = 0.98 * (-torch.log(1 / torch.repeat_interleave(s.float(), s)))
    return c


def saturate(c, seed):
    """logits spread by +-30 so that both sides of the 1e-8 clamp occur, chosen so that every probability is above 1e-6
    or below 1e-12 (asserted in float64 by the caller: float32 and float64 then agree on the side of every entry).  Per
    branch: each logit is 0 or -30 (+ a small perturbation); exp(-30) = 9.4e-14, and with at most 64 entries at level 0 the
    large probabilities stay above 1/64 / e."""
    gen = torch.Generator().manual_seed(seed)
    for key in ('logits', 'logits0'):
        z = c[key]
        level = torch.where(torch.rand(z.shape, generator=gen) < 0.5, 0., -30.)
        j0 = 0
        for s in c['sizes']:         # one entry per branch at level 0 for certain
            level[..., j0] = 0.
            j0 += s
        z.copy_(level + 0.5 * torch.rand(z.shape, generator=gen))
    c['mu0'][:, 0] = 1e-13           # ... and the behaviour probabilities cross the clamp too
    return c


def _strided(t):
    """the same values as a view with room in front of and behind every row (rows 5 / 2 elements further apart)"""
    if t.dim() == 0 or t.dtype == torch.int32:
        return t
    lead, last = (3, 5) if t.is_floating_point() else (1, 2)
    big = torch.zeros(*t.shape[:-1], t.shape[-1] + last, dtype=t.dtype, device=t.device)
    out = big[..., lead:lead + t.shape[-1]]
    out.copy_(t)
    return out


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
        for k in ('gamma_ratio', 'lambda_ratio', 'target'):
            out[k] = out[k].contiguous()
    return out


def v_trace(c, v_n, v_next, pi, mu):
    """oracle/sac_ref.py:106-121 on the case's tensors -> y [B]"""
    td = c['reward'] + c['gamma'] * ~c['done'] * v_next - v_n
    td = c['gamma_ratio'] * td
    if c['use_is']:
        td = c['lambda_ratio'] * td
        ratio = pi / mu.clamp(min=1e-8)
        rho = ratio.clamp(max=c['v_rho'])
        cc = ratio.clamp(max=c['v_c'])
        cc = torch.cat([torch.ones_like(cc[:, :1]), cc[..., :-1]], dim=-1)
        td = torch.cumprod(cc, dim=1) * rho * td
    td = td * ~(c['last'] | c['pad'])
    return v_n[:, 0] + torch.sum(td, dim=1)


def values(c):
    """the return's V(s_t), V(s_t+1) [B, n] and (pi, mu) [B, n] | (None, None), as `_get_y` forms them"""
    K, D = c['K'], c['D']
    alpha = torch.exp(c['log_alpha'])
    stacked = torch.stack(c['q_target'])
    mean_next = stacked[:, :, 1:].index_select(0, c['sub_next'].long()).mean(0)
    mean_n = stacked[:, :, :-1].index_select(0, c['sub_n'].long()).mean(0)
    d_policy = joint_policy(c['logits'], c['sizes'])
    probs = d_policy.probs
    n_p, next_p = probs[:, :-1], probs[:, 1:]
    v_n = torch.sum(n_p * (mean_n - alpha * torch.log(n_p.clamp(min=1e-8))), -1) / K
    v_next = torch.sum(next_p * (mean_next - alpha * torch.log(next_p.clamp(min=1e-8))), -1) / K
    pi = mu = None
    if c['use_is']:
        mu = c['mu'][..., :D] * c['action'][:, :-1, :D]
        mu = torch.where(mu == 0., torch.ones_like(mu), mu).prod(-1)
        pi = torch.exp(d_policy.log_prob(c['action'][..., :D]).sum(-1))[:, :-1]
    return v_n, v_next, pi, mu


def td_error(c, y):
    a0 = c['action'][:, 0]
    qs = torch.stack([torch.sum(a0 * q, dim=-1) / c['K'] for q in c['q_online']])       # [E, B]
    return torch.abs(qs - y.unsqueeze(0)).mean(0)


def ret(c):
    """-> {'y' [B], 'td' [B]}"""
    v_n, v_next, pi, mu = values(c)
    y = v_trace(c, v_n, v_next, pi, mu)
    return {'y': y, 'td': td_error(c, y)}


def q_loss(c):
    """-> {'loss_q' [E], 'grad_q' [E, B, D]} (d sum_e loss_e / d q)"""
    heads = [q.detach().clone().requires_grad_(True) for q in c['q_online']]
    a0 = c['action'][:, 0]
    qs = torch.stack([torch.sum(a0 * q, dim=-1, keepdim=True) / c['K'] for q in heads])
    losses = torch.nn.functional.mse_loss(qs, c['y'].expand_as(qs), reduction='none')
    if c['w'] is not None:
        losses = losses * c['w'].unsqueeze(0)
    per_member = losses.mean(dim=(1, 2))
    per_member.sum().backward()
    return {'loss_q': per_member.detach(), 'grad_q': torch.stack([h.grad for h in heads])}


def policy_loss(c):
    """-> {'loss_policy' [], 'grad_logits' [B, D], 'd_entropy' [], 'p' [B, D], 'h_pi' [B]}"""
    K = c['K']
    z = c['logits0'].detach().clone().requires_grad_(True)
    alpha = torch.exp(c['log_alpha'])
    d_policy = joint_policy(z, c['sizes'])
    probs = d_policy.probs
    mean_q = torch.stack(c['q_online']).index_select(0, c['sub_pi'].long()).mean(0)
    inner = alpha * torch.log(probs.clamp(min=1e-8)) - mean_q
    loss_d = torch.sum(probs * inner, dim=1, keepdim=True) / K
    mu = c['mu0']
    mu_ent = -torch.sum(mu * torch.log(mu.clamp(min=1e-8)), dim=-1) / K
    pi_ent = d_policy.entropy().sum(-1) / K
    loss_d = loss_d + c['penalty'] * (torch.pow(mu_ent - pi_ent, 2.) / 2.).unsqueeze(-1)
    loss = torch.mean(loss_d)
    loss.backward()
    return {'loss_policy': loss.detach(), 'grad_logits': z.grad, 'd_entropy': torch.mean(pi_ent).detach(),
            'p': probs.detach(), 'h_pi': pi_ent.detach()}


def alpha_grad(c):
    """-> {'grad_alpha' []}"""
    log_alpha = c['log_alpha'].detach().clone().requires_grad_(True)
    probs = joint_policy(c['logits0'], c['sizes']).probs
    inner = log_alpha * (-torch.log(probs.clamp(min=1e-8)) - c['target'])
    loss = torch.mean(torch.sum(probs * inner, dim=1, keepdim=True) / c['K'])
    loss.backward()
    return {'grad_alpha': log_alpha.grad}


def all_formulas(c):
    out = {}
    for f in (ret, q_loss, policy_loss, alpha_grad):
        out.update(f(c))
    return out


def clamp_sides(c64):
    """float64: every probability the formulas clamp (policy over the window, at the step's state, behaviour
    probabilities at the step's state) -> one flat tensor"""
    return torch.cat([joint_policy(c64['logits'], c64['sizes']).probs.reshape(-1),
                      joint_policy(c64['logits0'], c64['sizes']).probs.reshape(-1), c64['mu0'].reshape(-1)])


def as_numpy(d):
    return {k: np.asarray(v.detach().cpu().double().numpy()) for k, v in d.items()}


ULP = 2.0 ** -23


def over_the_bound(tag, want, kernel, eager):
    """The rule the kernels over a categorical head are held to (tests/test_discrete_gpu.py, test_hybrid_gpu.py,
    test_dqn_gpu.py, test_categorical_limits_gpu.py), on {name: float64 array} of the float64 restatement, the kernel and
    the float32 eager composition: every element of the kernel's tensors is finite (written) and of the restatement's
    shape; per tensor the kernel's largest absolute error may be at most twice the eager composition's, floor 4 units in
    the last place at the tensor's largest magnitude -> ([(tensor, kernel error, eager error, floor)] of the tensors over
    the bound, the largest share of the bound); prints every figure"""
    assert set(kernel) == set(eager) == set(want)
    bad, share = [], 0.
    for name, ref in want.items():
        assert np.isfinite(kernel[name]).all(), f'{name}: an element was not written'
        assert kernel[name].shape == ref.shape, name
        e_k, e_m = float(np.abs(kernel[name] - ref).max()), float(np.abs(eager[name] - ref).max())
        floor = 4 * ULP * float(np.abs(ref).max())
        bound = max(2 * e_m, floor)
        share = max(share, e_k / bound if bound > 0 else 0.)
        print(f'{tag} {name}: kernel {e_k:.3e}  eager {e_m:.3e}  floor {floor:.3e}  share {e_k / bound if bound else 0.:.2f}')
        if e_k > bound:
            bad.append((name, e_k, e_m, floor))
    return bad, share


GUARD = 64                      # floats in front of and behind every guarded output
SENTINEL = -1.2345679e30        # finite, and no result of these kernels


class Guarded:
    """An allocator of the kernels' output tensors (the `alloc` of the test modules' `_kernels`): each one a NaN-filled,
    contiguous view inside a larger buffer with GUARD floats of SENTINEL in front of it and behind it; `check()` after the
    launches: every sentinel still has its bits"""

    def __init__(self):
        self.buffers = []

    def __call__(self, *shape):
        numel = int(np.prod(shape, dtype=np.int64))
        buf = torch.full((GUARD + numel + GUARD,), SENTINEL, device='cuda')
        view = buf[GUARD:GUARD + numel].view(shape)
        view.fill_(float('nan'))
        self.buffers.append((buf, numel))
        return view

    def check(self):
        assert self.buffers
        bits = torch.tensor(SENTINEL).view(torch.int32).item()
        for i, (buf, numel) in enumerate(self.buffers):
            words = buf.view(torch.int32)
            assert bool((words[:GUARD] == bits).all()), f'output {i} ({numel} floats): written in front of the tensor'
            assert bool((words[GUARD + numel:] == bits).all()), f'output {i} ({numel} floats): written behind the tensor'
