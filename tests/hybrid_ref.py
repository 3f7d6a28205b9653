"""Restatements of the policy-based learner's arithmetic on a HYBRID action space (discrete branches and continuous
actions) on explicit tensors, shared by tests/test_hybrid_host.py (CPU: against `oracle.sac_ref.SacRef`) and
tests/test_hybrid_gpu.py (GPU: the float64 reference of the `asac_hybrid_*` kernels, and — the same torch code in float32
on the device — the eager composition the learner runs without them).  The discrete pieces are tests/discrete_ref.py's.
Formulas: oracle/sac_ref.py:334-365 (`get_y`), 379-393 (`train_rep_q`), 459-476 (`train_policy`), 491-502
(`train_alpha`), 545-551 (`td_error`), 75-92 (the squash corrections), 106-121 (`v_trace`)."""
import math

import torch

from tests import discrete_ref as dr

SQUASH_FLOOR = 1e-2
CLIP_EPS = 0.2


def make_case(B, n, sizes, A, E, Es, use_is, weights, seed):
    """`discrete_ref.make_case` (row 0 wholly padded, row 1 `done` at t = 0, row 2's stored discrete action at t = 0 all
    zeros) plus the continuous head's tensors.  Planted on top: row 3's stored continuous action is +1 at t = 0 and -1 at
    the last stored position (the 0.999 clamp); row 4 has a behaviour probability of 0 at its stored discrete action at
    t = 0 and a continuous one of 0 at the last step; `cq - tq` of member 0 is +0.3 / -0.3 / +0.05 in rows 0 / 1 / 2
    (outside, outside, inside +-CLIP_EPS); the last row's first two critics tie for the minimum in the policy step."""
    c = dr.make_case(B, n, sizes, E, Es, use_is, weights, seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    D = c['D']
    c['A'] = A

    def view(*shape):
        return torch.randn(*shape, generator=gen)
    c_action = torch.rand(B, n + 1, A, generator=gen) * 1.9 - 0.95
    c_mu = torch.rand(B, n, A, generator=gen) * 1.5 + 0.05
    if B > 3:
        c_action[3, 0], c_action[3, n - 1] = 1., -1.
    c['mu_full'] = torch.cat([c['mu'], c_mu], dim=-1)                  # [B, n, D + A]
    if B > 4:
        c['mu_full'][4, 0, :D] *= 1. - c['action'][4, 0]
        c['mu_full'][4, n - 1, D] = 0.
    c['action_full'] = torch.cat([c['action'], c_action], dim=-1)       # [B, n+1, D + A]
    c['loc_w'], c['scale_w'], c['eps_w'] = view(B, n + 1, A), torch.exp(-2. * torch.rand(B, n + 1, A, generator=gen)), view(B, n + 1, A)
    c['cq_target'] = view(E, B, n + 1)
    c['c_q_online'] = view(E, B)
    delta = torch.rand(E, B, generator=gen) - 0.5
    for r, dv in enumerate((0.3, -0.3, 0.05)[:B]):
        delta[0, r] = dv
    c['c_t_q'] = c['c_q_online'] - delta
    c['c_y'] = view(B, 1)
    c['c_q_pi'] = view(E, B)
    if E > 1:
        c['c_q_pi'][0, B - 1] = c['c_q_pi'][1, B - 1] = c['c_q_pi'][:, B - 1].min() - 1.
    c['loc0'], c['scale0'], c['eps0'] = view(B, A), torch.exp(-2. * torch.rand(B, A, generator=gen)), view(B, A)
    c['sub_cn'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    c['sub_cnext'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    c['sub_pi_c'] = torch.randperm(E, generator=gen)[:Es].to(torch.int32)
    if E > 1:       # the tied members are both in the policy step's subset, the larger index first where there is room
        c['sub_pi_c'] = torch.tensor(([1, 0] + list(range(2, E)))[:Es] if Es > 1 else [0], dtype=torch.int32)
    c['log_c_alpha'] = torch.tensor(-1.1)
    c['clip_eps'], c['target_c'] = CLIP_EPS, 1.0 * -float(A)
    return c


def to(c, dtype, device, strided=False):
    """`discrete_ref.to`, with the discrete parts of the stored actions and behaviour probabilities as views of the full
    tensors (what the learner hands the launches)"""
    out = dr.to(c, dtype, device, strided)
    D = c['D']
    out['action'], out['mu'] = out['action_full'][..., :D], out['mu_full'][..., :D]
    if strided:
        for k in ('cq_target', 'c_q_online', 'c_t_q', 'c_q_pi', 'loc_w', 'scale_w', 'eps_w', 'loc0', 'scale0', 'eps0'):
            out[k] = out[k].contiguous()        # (dense in the learner: stacked values, the policy's outputs, noise buffers)
    return out


def _jac(x):
    return torch.clamp(1 - torch.tanh(x) ** 2, min=SQUASH_FLOOR)


def _log_prob(loc, scale, x):
    return -((x - loc) ** 2) / (2 * scale ** 2) - torch.log(scale) - math.log(math.sqrt(2 * math.pi))


def sample_logp(loc, scale, eps):
    """log pi of x = loc + eps scale under the tanh squash: the correction is summed over the action dimensions and then
    subtracted from EVERY dimension's log-probability (oracle 75-76, 83-85)"""
    x = loc + eps * scale
    lp = _log_prob(loc, scale, x) - torch.sum(torch.log(_jac(x)), dim=-1, keepdim=True)
    return lp.sum(-1)


def stored_prob(loc, scale, action):
    """per-dimension probability of the stored continuous actions (oracle 79-80, 362-363)"""
    x = torch.atanh(torch.clamp(action, -0.999, 0.999))
    return torch.exp(_log_prob(loc, scale, x)) / torch.prod(_jac(x), dim=-1, keepdim=True)


def masked_prod(p):
    p = torch.where(torch.isinf(p), torch.ones_like(p), p)
    out = p.prod(-1)
    return torch.where(torch.isfinite(out), out, torch.ones_like(out))


def window(c):
    """(logp [B, n+1], c_pi [B, n+1, A]) of the window: the case's own (`logp_w` / `c_pi`: the sampling launch's, on the
    device) or the formulas'"""
    if 'logp_w' in c:
        return c['logp_w'], c['c_pi']
    D = c['D']
    return sample_logp(c['loc_w'], c['scale_w'], c['eps_w']), stored_prob(c['loc_w'], c['scale_w'], c['action_full'][..., D:])


def logp0(c):
    return c['logp0'] if 'logp0' in c else sample_logp(c['loc0'], c['scale0'], c['eps0'])


def c_values(c):
    """the continuous return's V(s_t), V(s_t+1) [B, n] and (pi, mu) [B, n] | (None, None)"""
    D = c['D']
    alpha = torch.exp(c['log_c_alpha'])
    logp, c_pi = window(c)
    tab = c['cq_target']
    min_n = tab[:, :, :-1].index_select(0, c['sub_cn'].long()).min(dim=0)[0]
    min_next = tab[:, :, 1:].index_select(0, c['sub_cnext'].long()).min(dim=0)[0]
    v_n, v_next = min_n - alpha * logp[:, :-1], min_next - alpha * logp[:, 1:]
    pi = mu = None
    if c['use_is']:
        pi, mu = masked_prod(c_pi[:, :-1]), masked_prod(c['mu_full'][..., D:])
    return v_n, v_next, pi, mu


def td_error(c, d_y, c_y):
    a0 = c['action'][:, 0]
    err = torch.zeros(c['E'], c['B'], dtype=d_y.dtype, device=d_y.device)
    err = err + torch.abs(torch.stack([torch.sum(a0 * q, dim=-1) / c['K'] for q in c['q_online']]) - d_y.unsqueeze(0))
    err = err + torch.abs(c['c_q_online'] - c_y.unsqueeze(0))
    return err.mean(0)


def ret(c):
    """-> {'d_y' [B], 'c_y' [B], 'td' [B]}"""
    d_y = dr.v_trace(c, *dr.values(c))
    c_y = dr.v_trace(c, *c_values(c))
    return {'d_y': d_y, 'c_y': c_y, 'td': td_error(c, d_y, c_y)}


def q_loss(c):
    """-> {'loss_q' [E], 'grad_qd' [E, B, D], 'grad_cq' [E, B]} (d sum_e loss_e / d (head outputs, continuous values))"""
    heads = [q.detach().clone().requires_grad_(True) for q in c['q_online']]
    c_q = c['c_q_online'].detach().clone().requires_grad_(True)
    a0, eps = c['action'][:, 0], c['clip_eps']
    qs = torch.stack([torch.sum(a0 * q, dim=-1, keepdim=True) / c['K'] for q in heads])          # [E, B, 1]
    losses = torch.nn.functional.mse_loss(qs, c['y'].expand_as(qs), reduction='none')
    t_q, yv = c['c_t_q'], c['c_y'].reshape(1, -1)
    clipped = t_q + torch.clamp(c_q - t_q, -eps, eps)
    losses = losses + torch.maximum((clipped - yv) ** 2, (c_q - yv) ** 2).unsqueeze(-1)
    if c['w'] is not None:
        losses = losses * c['w'].unsqueeze(0)
    per_member = losses.mean(dim=(1, 2))
    per_member.sum().backward()
    return {'loss_q': per_member.detach(), 'grad_qd': torch.stack([h.grad for h in heads]), 'grad_cq': c_q.grad}


def policy_loss(c):
    """-> {'loss_policy' [], 'grad_logits' [B, D], 'grad_logp' [B], 'grad_cq_pi' [E, B], 'd_entropy' [], 'c_entropy' []};
    the gradient of the minimum goes to the FIRST arg-min member in subset order"""
    K, B, E = c['K'], c['B'], c['E']
    z = c['logits0'].detach().clone().requires_grad_(True)
    lp = logp0(c).detach().clone().requires_grad_(True)
    alpha, c_alpha = torch.exp(c['log_alpha']), torch.exp(c['log_c_alpha'])
    d_policy = dr.joint_policy(z, c['sizes'])
    probs = d_policy.probs
    mean_q = torch.stack(c['q_online']).index_select(0, c['sub_pi'].long()).mean(0)
    loss_d = torch.sum(probs * (alpha * torch.log(probs.clamp(min=1e-8)) - mean_q), dim=1, keepdim=True) / K
    mu = c['mu0']
    mu_ent = -torch.sum(mu * torch.log(mu.clamp(min=1e-8)), dim=-1) / K
    pi_ent = d_policy.entropy().sum(-1) / K
    loss_d = loss_d + c['penalty'] * (torch.pow(mu_ent - pi_ent, 2.) / 2.).unsqueeze(-1)
    sub = [int(e) for e in c['sub_pi_c']]
    best = torch.full((B,), sub[0], dtype=torch.long, device=lp.device)
    m = c['c_q_pi'][sub[0]].clone()
    for e in sub[1:]:
        lower = c['c_q_pi'][e] < m
        m, best = torch.where(lower, c['c_q_pi'][e], m), torch.where(lower, torch.full_like(best, e), best)
    loss = torch.mean(loss_d + (c_alpha * lp - m).unsqueeze(-1))
    loss.backward()
    grad_cq = torch.zeros(E, B, dtype=lp.dtype, device=lp.device)
    grad_cq[best, torch.arange(B, device=lp.device)] = -1. / B
    c_ent = torch.mean((torch.log(c['scale0']) + 0.5 + 0.5 * math.log(2 * math.pi)).sum(-1))
    return {'loss_policy': loss.detach(), 'grad_logits': z.grad, 'grad_logp': lp.grad, 'grad_cq_pi': grad_cq,
            'd_entropy': torch.mean(pi_ent).detach(), 'c_entropy': c_ent}


def alpha_grad(c):
    """-> {'grad_alpha' [2]}: d loss / d (log_d_alpha, log_c_alpha)"""
    log_d = c['log_alpha'].detach().clone().requires_grad_(True)
    log_c = c['log_c_alpha'].detach().clone().requires_grad_(True)
    probs = dr.joint_policy(c['logits0'], c['sizes']).probs
    loss_d = torch.sum(probs * (log_d * (-torch.log(probs.clamp(min=1e-8)) - c['target'])), dim=1, keepdim=True) / c['K']
    loss_c = log_c * (-logp0(c).unsqueeze(-1) - c['target_c'])
    torch.mean(loss_d + loss_c).backward()
    return {'grad_alpha': torch.stack([log_d.grad, log_c.grad])}


def all_formulas(c):
    out = {}
    for f in (ret, q_loss, policy_loss, alpha_grad):
        out.update(f(c))
    return out
