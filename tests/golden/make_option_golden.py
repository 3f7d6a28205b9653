"""Mint the golden vectors of the option-critic's per-option learner (`algorithm/oc/option_base.OptionBase`) from the
*reference* implementation, run on the CPU.  Run where the reference tree is available (see make_golden.py):

    python tests/golden/make_option_golden.py [case names... | get_y]      (default: all)

  f15_option_<case>.npz   one full call sequence of one option from recorded weights (`w0/`) on seeded tensors (`in/`):
        compute_rep_q_grads (`d_y`, `c_y`), train_rep_q (first moments `g0/`, weights `w_rq/`), train_policy_alpha (`w_pi/`),
        compute_termination_grads + train_termination (`loss_termination`, `g0/optimizer_termination/`, `w_term/`),
        _get_td_error (`td_error`), _update_target_variables(tau) (`w_tgt/`), choose_action with sampling disabled (`act/`).
        The reference's random draws are recorded in consumption order (`eps/<i>`, `perm/<i>`).
  f15_option_get_y.npz    OptionBase._get_y with the policy and the target critics replaced by tables (as f4_get_y): exactly
        the arithmetic of `asac_option_return`.
Stored actions stay inside (-0.99, 0.99): the reference takes atanh of them without a clamp (option_base.py:415).
Fixtures are data only (inputs, recorded draws, expected outputs).
"""
import copy
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg  # noqa: E402  (installs the reference shims)
import ref_shims  # noqa: E402

from algorithm.oc.option_base import OptionBase  # noqa: E402
from algorithm.utils.enums import SEQ_ENCODER  # noqa: E402

O = 3
TAU = 0.1
TERMINAL_ENTROPY = 0.05


def _betas(rng, shape):
    """spread over (0, 1) with exact zeros and ones"""
    b = rng.random(shape).astype(np.float32)
    flat = b.reshape(-1)
    flat[::5] = 0.
    flat[2::7] = 1.
    return b


def _option(nn_rel, fix_policy=False, **kw):
    base = dict(obs_names=['vector'], obs_shapes=[(6,)], d_action_sizes=[], c_action_size=2, model_abs_dir=None,
                nn=mg.load_ref_nn(nn_rel), device='cpu', batch_size=16)
    base.update(kw)
    return OptionBase(0, 'option_0', fix_policy, False, **base)


def _save(path, out):
    for k, v in out.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == 'f':
            assert np.isfinite(v).all(), (path.name, k)
    np.savez_compressed(path, **out)
    assert path.stat().st_size < 1_000_000, (path.name, path.stat().st_size)
    print(path.name, path.stat().st_size, 'bytes')


def f15_get_y():
    out = {}
    rng = np.random.default_rng(15)
    for tag, n, E, Es, A, use_is in [('n4_e2', 4, 2, 2, 2, True), ('n3_e4s2', 3, 4, 2, 4, True),
                                     ('n40_e2', 40, 2, 2, 2, True), ('n1_e2_nois', 1, 2, 2, 2, False)]:
        opt = _option('envs/test/nn_oc.py', n_step=n, c_action_size=A, ensemble_q_num=E, ensemble_q_sample=Es,
                      use_n_step_is=use_is, gamma=0.99, v_lambda=0.95, v_rho=1.0, v_c=0.9)
        B = 21
        loc = torch.from_numpy(rng.standard_normal((B, n + 1, A)).astype(np.float32))
        scale = torch.from_numpy(np.exp(rng.uniform(-3, 0.5, (B, n + 1, A))).astype(np.float32))
        qtab = [torch.from_numpy(rng.standard_normal((B, n + 1, 1)).astype(np.float32)) for _ in range(E)]
        opt.model_policy = lambda states, obs: (None, torch.distributions.Normal(loc, scale, validate_args=False))
        opt.model_target_q_list = [(lambda s, a, o, t=t: (None, t)) for t in qtab]
        with torch.no_grad():
            opt.log_c_alpha.fill_(float(rng.uniform(-3, 0)))
        args = dict(
            next_n_vs_over_options=rng.standard_normal((B, n, O)).astype(np.float32),
            n_terminations=_betas(rng, (B, n)),
            n_last_masks=rng.random((B, n)) < 0.15, n_padding_masks=rng.random((B, n)) < 0.2,
            n_actions=rng.uniform(-0.99, 0.99, (B, n, A)).astype(np.float32),
            n_rewards=rng.standard_normal((B, n)).astype(np.float32),
            n_dones=rng.random((B, n)) < 0.3,
            n_mu_probs=(rng.random((B, n, A)) * 2).astype(np.float32))
        nx_states = torch.zeros((B, n + 1, 6))
        mg.seed_all(150 + n)
        with ref_shims.DrawRecorder() as rec:
            _, c_y = opt._get_y(nx_obses_list=[nx_states], nx_states=nx_states,
                                **{k: torch.from_numpy(v.copy()) for k, v in args.items()})
        for k, v in args.items():
            out[f'{tag}_{k}'] = v
        out[f'{tag}_loc'], out[f'{tag}_scale'] = loc.numpy(), scale.numpy()
        out[f'{tag}_q'] = torch.stack(qtab).numpy()
        out[f'{tag}_eps'] = rec.eps[0].numpy()
        out[f'{tag}_perm'] = torch.stack(rec.perm).numpy()
        out[f'{tag}_log_alpha'] = opt.log_c_alpha.detach().numpy()
        out[f'{tag}_y'] = c_y.numpy()
        out[f'{tag}_cfg'] = np.array([n, E, Es, A, int(use_is)])
        out[f'{tag}_params'] = np.array([0.99, 0.95, 1.0, 0.9])
    _save(HERE / 'f15_option_get_y.npz', out)


def policy_step_in_float64(out, opt, before, state, rec):
    """The continuous policy step (sac_base.py:1882-1908) again in float64, from the weights it started from and the draw
    it consumed.  With a policy scale of 1e-4 the float32 gradient of the reference is itself 1e-3 (of the largest entry)
    off its float64 value — (x - loc) / scale^2 terms of size 1e4 cancel — so the fixture records the float64 first
    moments (`g0_f64/`), the weights one Adam step from them gives (`w_pi_f64/`: from zero moments the step is
    lr * g / (|g| + eps)) and how far the reference's own float32 first moments are from them (`ref32_error/`)."""
    from algorithm.utils.operators import squash_correction_log_prob, sum_log_prob
    policy, critics, alpha, at = before
    policy, critics = policy.double(), [q.double() for q in critics]
    st = state.double()
    _, c_policy = policy(st, [st])
    x = c_policy.loc + rec.eps[at].double() * c_policy.scale
    # (the two critics are both sampled in these cases: the recorded permutation does not change the minimum)
    assert opt.ensemble_q_num == opt.ensemble_q_sample
    c_q = torch.stack([q(st, torch.tanh(x), [st])[1] for q in critics])
    log_prob = sum_log_prob(squash_correction_log_prob(c_policy, x), keepdim=True)
    loss = torch.mean(alpha * log_prob - c_q.min(0)[0])
    loss.backward(inputs=list(policy.parameters()))
    lr, eps = opt.learning_rate, 1e-8
    for j, ((k, p64), p_now) in enumerate(zip(policy.named_parameters(), opt.model_policy.parameters())):
        g = p64.grad
        out[f'g0_f64/optimizer_policy/{j}'] = (0.1 * g).numpy().copy()
        out[f'w_pi_f64/model_policy/{k}'] = (p64.detach() - lr * g / (g.abs() + eps)).float().numpy().copy()
        ref = out[f'g0/optimizer_policy/{j}'].astype(np.float64)
        out[f'ref32_error/optimizer_policy/{j}'] = np.float64(
            np.abs(ref - 0.1 * g.numpy()).max() / max(float(0.1 * g.abs().max()), 1e-300))
    print('policy first moments, reference float32 against float64:',
          ' '.join(f"{float(out[f'ref32_error/optimizer_policy/{j}']):.1e}" for j in range(len(list(policy.parameters())))))


def f15(case, nn_rel, kw, d_action_sizes=(), c_action_size=2, fix_policy=False, with_is_weights=False, seed=15):
    mg.seed_all(seed)
    rng = np.random.default_rng(seed)
    opt = _option(nn_rel, fix_policy=fix_policy, d_action_sizes=list(d_action_sizes), c_action_size=c_action_size, **kw)
    B, n = 16, opt.n_step
    A_all = sum(d_action_sizes) + c_action_size
    out = {}
    mods = {k: v for k, v in opt.ckpt_dict.items() if isinstance(v, torch.nn.Module)}
    # the target networks start as copies of the online ones: move them apart so that the targets, the clipped loss and
    # the Polyak step see two different sets of weights
    with torch.no_grad():
        for name, m in mods.items():
            if 'target' in name:
                for p in m.parameters():
                    p.add_(torch.randn_like(p) * 0.05)
        # ... and the target termination head's last layer is scaled up, so that the terminations it returns spread over
        # its whole range (sigmoid of a value clamped to +-3: 0.047 .. 0.953) instead of sitting near 0.5
        last_w, last_b = list(opt.model_target_termination.parameters())[-2:]
        last_w.mul_(40.)

    def snapshot(prefix, only=None):
        for name, m in mods.items():
            if only is None or any(name.startswith(o) for o in only):
                for k, v in m.state_dict().items():
                    out[f'{prefix}/{name}/{k}'] = v.numpy().copy()
        out[f'{prefix}/log_d_alpha'] = opt.log_d_alpha.detach().numpy().copy()
        out[f'{prefix}/log_c_alpha'] = opt.log_c_alpha.detach().numpy().copy()

    snapshot('w0')
    parts = [np.eye(s, dtype=np.float32)[rng.integers(0, s, (B, n))] for s in d_action_sizes]
    if c_action_size:
        parts.append(rng.uniform(-0.99, 0.99, (B, n, c_action_size)).astype(np.float32))
    last = rng.random((B, n)) < 0.15
    pad = rng.random((B, n)) < 0.2
    last[:, 0] = pad[:, 0] = False
    hidden_shape = tuple(opt.seq_hidden_state_shape)
    inp = dict(
        nx_obs=rng.standard_normal((B, n + 1, 6)).astype(np.float32),
        n_actions=np.concatenate(parts, -1),
        n_rewards=rng.standard_normal((B, n)).astype(np.float32),
        n_dones=rng.random((B, n)) < 0.3,
        n_last_masks=last, n_padding_masks=pad,
        n_mu_probs=(rng.random((B, n, A_all)) * 0.9 + 0.1).astype(np.float32),
        nx_pre_seq_hidden_states=rng.standard_normal((B, n + 1, *hidden_shape)).astype(np.float32),
        next_n_vs_over_options=rng.standard_normal((B, n, O)).astype(np.float32),
        v_over_options=rng.standard_normal((B, O)).astype(np.float32),
        done=rng.random(B) < 0.3,
        priority_is=(rng.random((B, 1)) + 0.5).astype(np.float32),
        act_obs=rng.standard_normal((B, 6)).astype(np.float32),
        act_pre_action=np.concatenate(
            [np.eye(s, dtype=np.float32)[rng.integers(0, s, B)] for s in d_action_sizes]
            + [rng.uniform(-0.9, 0.9, (B, c_action_size)).astype(np.float32)], -1),
        act_pre_hidden=rng.standard_normal((B, *hidden_shape)).astype(np.float32))
    for k, v in inp.items():
        out[f'in/{k}'] = v
    out['in/with_priority_is'] = np.bool_(with_is_weights)
    out['in/tau'], out['in/terminal_entropy'] = np.float64(TAU), np.float64(TERMINAL_ENTROPY)
    t = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
    priority_is = t['priority_is'] if with_is_weights else None

    nx_obses_list = [t['nx_obs']]
    nx_actions = torch.cat([t['n_actions'], torch.zeros_like(t['n_actions'][:, :1])], dim=1)
    nx_pre_actions = torch.cat([torch.zeros_like(nx_actions[:, :1]), nx_actions[:, :-1]], dim=1)
    nx_indexes = torch.arange(n + 1, dtype=torch.int32).repeat(B, 1)
    nx_pad = torch.cat([t['n_padding_masks'], t['n_padding_masks'][:, -1:]], dim=1)

    def states(is_target):
        return opt.get_l_states(nx_indexes, nx_pad, nx_obses_list, nx_pre_actions, t['nx_pre_seq_hidden_states'],
                                is_target=is_target)[0]

    with torch.no_grad():
        nx_target_states = states(True)
    nx_states = states(False)

    seen = {}
    orig_backward = torch.Tensor.backward

    def spy(tensor, *a, **k):
        seen['loss'] = float(tensor.detach())
        return orig_backward(tensor, *a, **k)

    def first_moments(names):
        for oname in names:
            opt_ = getattr(opt, oname, None) if not oname.startswith('optimizer_q_') else opt.optimizer_q_list[int(oname[12:])]
            if opt_ is None:
                continue
            for j, p in enumerate(opt_.param_groups[0]['params']):
                st = opt_.state.get(p)
                out[f'g0/{oname}/{j}'] = (st['exp_avg'] if st else torch.zeros_like(p)).detach().numpy().copy()

    with ref_shims.DrawRecorder() as rec:
        d_y, c_y = opt.compute_rep_q_grads(
            next_n_vs_over_options=t['next_n_vs_over_options'], n_indexes=nx_indexes[:, :-1],
            n_last_masks=t['n_last_masks'], n_padding_masks=t['n_padding_masks'], nx_obses_list=nx_obses_list,
            nx_target_obses_list=nx_obses_list, nx_states=nx_states, nx_target_states=nx_target_states,
            n_actions=t['n_actions'], n_pre_actions=nx_pre_actions[:, :-1], n_rewards=t['n_rewards'].clone(),
            n_dones=t['n_dones'], n_mu_probs=t['n_mu_probs'].clone(),
            n_pre_seq_hidden_states=t['nx_pre_seq_hidden_states'][:, :-1], priority_is=priority_is)
        opt.train_rep_q()
        if d_y is not None:
            out['d_y'] = d_y.detach().numpy().copy()
        if c_y is not None:
            out['c_y'] = c_y.detach().numpy().copy()
        first_moments(['optimizer_rep'] + [f'optimizer_q_{i}' for i in range(opt.ensemble_q_num)])
        snapshot('w_rq', only=('model_rep', 'model_q_'))

        nx_states_d = nx_states.detach()
        before = None
        if not d_action_sizes and not fix_policy:
            before = (copy.deepcopy(opt.model_policy), [copy.deepcopy(q) for q in opt.model_q_list],
                      float(torch.exp(opt.log_c_alpha.detach())), len(rec.eps))
        opt.train_policy_alpha(n_padding_masks=t['n_padding_masks'], n_obses_list=[t['nx_obs'][:, :-1]],
                               nx_states=nx_states_d, n_actions=t['n_actions'], n_mu_probs=t['n_mu_probs'].clone())
        first_moments(['optimizer_policy'])
        snapshot('w_pi', only=('model_policy',))
        if before is not None:
            policy_step_in_float64(out, opt, before, nx_states_d[:, 0], rec)

        y = c_y if c_y is not None else d_y
        torch.Tensor.backward = spy
        try:
            opt.compute_termination_grads(TERMINAL_ENTROPY, [t['nx_obs'][:, 0]], nx_states_d[:, 0], y.detach(),
                                          t['v_over_options'], t['done'], priority_is)
        finally:
            torch.Tensor.backward = orig_backward
        opt.train_termination()
        out['loss_termination'] = np.float64(seen['loss'])
        first_moments(['optimizer_termination'])
        snapshot('w_term', only=('model_termination',))

        td = opt._get_td_error(
            next_n_vs_over_options=t['next_n_vs_over_options'], n_last_masks=t['n_last_masks'],
            n_padding_masks=t['n_padding_masks'], nx_obses_list=nx_obses_list, nx_target_obses_list=nx_obses_list,
            state=nx_states_d[:, 0], nx_target_states=nx_target_states, n_actions=t['n_actions'],
            n_rewards=t['n_rewards'].clone(), n_dones=t['n_dones'], n_mu_probs=t['n_mu_probs'].clone())
        out['td_error'] = td.detach().numpy().copy()
    opt._update_target_variables(TAU)
    snapshot('w_tgt', only=('model_target_',))
    opt.set_train_mode(False)       # (acting as evaluation does: no exploration noise of the dqn-like branch)
    action, prob, hidden, termination = opt.choose_action([t['act_obs']], t['act_pre_action'], t['act_pre_hidden'],
                                                          disable_sample=True)
    out['act/action'], out['act/prob'] = action.numpy().copy(), prob.numpy().copy()
    out['act/hidden'], out['act/termination'] = hidden.numpy().copy(), termination.numpy().copy()
    for i, e in enumerate(rec.eps):
        out[f'eps/{i}'] = e.numpy().copy()
    for i, p in enumerate(rec.perm):
        out[f'perm/{i}'] = p.numpy().copy()
    out['n_eps'], out['n_perm'] = np.int64(len(rec.eps)), np.int64(len(rec.perm))
    if fix_policy:      # the representation and the policy keep their `w0/` values
        for name in ('model_rep', 'model_policy'):
            for k, v in (mods[name].state_dict().items() if name in mods else ()):
                assert np.array_equal(out[f'w0/{name}/{k}'], v.numpy()), (name, k)
    _save(HERE / f'f15_option_{case}.npz', out)


SMALL = str(HERE.parent / 'plugins' / 'nn_oc_small.py')
IS = dict(gamma=0.99, v_lambda=0.95, v_rho=1.0, v_c=0.9)
CASES = {
    'get_y': f15_get_y,
    'mlp': lambda: f15('mlp', 'envs/test/nn_oc.py', dict(n_step=4, use_n_step_is=True, **IS)),
    'mlp_n1': lambda: f15('mlp_n1', 'envs/test/nn_oc.py', dict(n_step=1, use_n_step_is=False, clip_epsilon=0.2),
                          with_is_weights=True),
    'rnn': lambda: f15('rnn', 'envs/test/nn_rnn.py', dict(n_step=3, seq_encoder=SEQ_ENCODER.RNN, **IS)),
    # (narrow critics, plugin API only: with the reference's 64-wide three-layer heads these two files exceed 1 MB)
    'hybrid': lambda: f15('hybrid', SMALL, dict(n_step=3, ensemble_q_num=3, ensemble_q_sample=2, **IS),
                          d_action_sizes=(3, 2)),
    'dqn': lambda: f15('dqn', SMALL, dict(n_step=3, discrete_dqn_like=True, ensemble_q_num=3, ensemble_q_sample=2), d_action_sizes=(3, 2),
                       c_action_size=0),
    'fix_policy': lambda: f15('fix_policy', 'envs/test/nn_oc.py', dict(n_step=4, use_n_step_is=True, **IS),
                              fix_policy=True),
}


def main():
    torch.set_num_threads(1)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()


if __name__ == '__main__':
    main()
