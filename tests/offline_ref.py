"""Float64 restatement of the continuous policy objective with the offline loss (reference sac_base.py:1882-1903,
operators.py:12-24), as torch autograd on float64 copies of the learner's own modules:

    u      = loc + eps * scale                                   the pre-tanh rsample()
    logp   = sum_d [ Normal(loc, scale).log_prob(u)_d - sum_e log(max(1 - tanh(u_e)^2, 1e-2)) ]   (+inf entries masked)
    L      = mean_b( alpha * logp - min_{e in subset} q_e(s, tanh(u)) + sum_d (u - a)^2 )

`a` is the stored continuous action of the row; the last term is the offline loss (1899-1900), on u itself — no atanh
of the squashed action.  Used by tests/test_offline_loss_gpu.py for the kernels (stock networks) and for the learner's
autograd path (plugin critics): the modules are only called through the plugin interface.
"""
import copy

import torch

SQUASH_FLOOR = 1e-2


def double_copy(module):
    """a float64 CPU copy of a module (the original is not touched)"""
    return copy.deepcopy(module).cpu().double()


def policy_objective(pi, qs, state, eps, stored_action, log_alpha, subset=None, offline=True, obs_list=None):
    """-> (objective, [gradient per parameter tensor of `pi`, `parameters()` order]) in float64.

    pi, qs: float64 CPU modules (`double_copy`); state [N, S], eps [N, A], stored_action [N, A] (any dtype / device);
    log_alpha: scalar; subset: the ensemble members the objective samples, in order (None: all);
    offline=False: the objective without the offline term."""
    f64 = lambda t: torch.as_tensor(t).detach().cpu().double()  # noqa: E731
    state, eps, stored_action = f64(state), f64(eps), f64(stored_action)
    alpha = f64(log_alpha).exp()
    obs_list = [None] if obs_list is None else obs_list
    _, c = pi(state, obs_list)
    u = c.loc + eps * c.scale
    t = torch.tanh(u)
    corr = torch.log(torch.clamp(1. - t * t, min=SQUASH_FLOOR)).sum(-1, keepdim=True)
    lp = c.log_prob(u) - corr                                   # the correction is broadcast to every component
    lp = torch.where(lp == torch.inf, torch.zeros_like(lp), lp)
    logp = lp.sum(-1, keepdim=True)
    members = list(range(len(qs))) if subset is None else [int(e) for e in subset]
    q = torch.stack([qs[e](state, t, obs_list)[1] for e in members])          # [Es, N, 1]
    loss = alpha * logp - q.min(0)[0]
    if offline:
        loss = loss + ((u - stored_action) ** 2).sum(-1, keepdim=True)
    objective = loss.mean()
    grads = torch.autograd.grad(objective, list(pi.parameters()))
    return objective.detach(), [g.detach() for g in grads]


def offline_grad_u(loc, scale, eps, stored_action):
    """-> (mean_b sum_d (u - a)^2, its gradient at u: 2 (u - a) / N) in float64"""
    f64 = lambda t: torch.as_tensor(t).detach().cpu().double()  # noqa: E731
    u = f64(loc) + f64(eps) * f64(scale)
    diff = u - f64(stored_action)
    return (diff ** 2).sum(-1).mean(), 2. * diff / diff.shape[0]
