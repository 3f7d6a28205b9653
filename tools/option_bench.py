"""Sequences/s and launches per sequence of one option's training calls (`algorithm/oc/option_base.OptionBase`):
`compute_rep_q_grads + train_rep_q + train_policy_alpha + compute_termination_grads + train_termination + _get_td_error`
on a continuous action space with the stock networks, two ways in one process, same box, same inputs:

  (a) torch    the PyTorch-ROCm composition of the reference's lines (option_base.py:249-801 for this configuration) on the
               learner's own modules, with `torch.optim.Adam`
  (b) native   this class (eager: an option's calls are not captured into a hipGraph, the selector owns the step)

    python tools/option_bench.py [--sequences 300] [--batch 256] [--n-step 4] [--options 3]

With `--discrete 3,2` (branch sizes) the option is pure-discrete with a policy, on tests/plugins/nn_oc_small.py — the shape
of the reference's option-critic configurations (`--batch 1024 --n-step 5 --options 3`) — and the two ways are this class
with `hip_config['fused_option_discrete']` on and off: sequences/s and launches per sequence of the whole sequence, and
the HIP-event time of `compute_rep_q_grads + _get_td_error` alone, three runs each in alternating order.
`on_faster_in_every_run` says whether every on-run of that pair was faster than every off-run (the rule the switch's
default follows).

Every timed window ends in a device synchronise.  Launches per sequence are counted with torch's profiler over three
sequences outside the timing.  No ratio is promised: the numbers are what this run measures."""
import argparse
import json
import sys
import time
from itertools import chain
from pathlib import Path

import numpy as np
import torch
from torch.nn import functional

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make(batch, n_step):
    import asac_amd  # noqa: F401
    from algorithm.oc import OptionBase
    from tests import parity_utils as pu
    torch.manual_seed(0)
    return OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], [], 2, None, pu.plugin('nn_oc'), device='cuda:0',
                      batch_size=batch, n_step=n_step, summary_path=None, write_summary_per_step=1e9)


def inputs(B, n, O, A=2):
    rng = np.random.default_rng(B + n)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    f = lambda *s: dev(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    nx_obs = f(B, n + 1, 6)
    return dict(nx_obs=nx_obs, n_actions=dev(rng.uniform(-0.99, 0.99, (B, n, A)).astype(np.float32)), n_rewards=f(B, n),
                n_dones=dev(rng.random((B, n)) < 0.1), n_last=dev(np.zeros((B, n), bool)), n_pad=dev(np.zeros((B, n), bool)),
                n_mu=dev((rng.random((B, n, A)) * 0.9 + 0.1).astype(np.float32)), v_next=f(B, n, O), v=f(B, O),
                done=dev(rng.random(B) < 0.1), nx_states=nx_obs, hidden=torch.zeros((B, n, 1), device='cuda'))


def native_sequence(opt, d):
    def run():
        obs = [d['nx_obs']]
        _, c_y = opt.compute_rep_q_grads(d['v_next'], None, d['n_last'], d['n_pad'], obs, obs, d['nx_states'], d['nx_states'],
                                         d['n_actions'], None, d['n_rewards'], d['n_dones'], d['n_mu'], d['hidden'])
        opt.train_rep_q()
        opt.train_policy_alpha(d['n_pad'], [d['nx_obs'][:, :-1]], d['nx_states'], d['n_actions'], d['n_mu'])
        opt.compute_termination_grads(0.05, [d['nx_obs'][:, 0]], d['nx_states'][:, 0], c_y, d['v'], d['done'], None)
        opt.train_termination()
        return opt._get_td_error(d['v_next'], d['n_last'], d['n_pad'], obs, obs, d['nx_states'][:, 0], d['nx_states'],
                                 d['n_actions'], d['n_rewards'], d['n_dones'], d['n_mu'])
    return run


def torch_sequence(opt, d):
    """the reference's lines for a continuous action space, V-trace with importance sampling, clipped double-Q loss"""
    from algorithm.utils.operators import squash_correction_log_prob, squash_correction_prob, sum_log_prob
    mk = lambda ps: torch.optim.Adam(ps, lr=opt.learning_rate)  # noqa: E731
    o_q = [mk(q.parameters()) for q in opt.model_q_list]
    o_pi, o_alpha = mk(opt.model_policy.parameters()), mk([opt.log_c_alpha])
    o_term = mk(opt.model_termination.parameters())
    E = opt.ensemble_q_num

    def get_y(beta, obs, states):
        with torch.no_grad():
            alpha = torch.exp(opt.log_c_alpha)
            vbar = d['v_next'].mean(-1)
            nx_actions = torch.cat([d['n_actions'], torch.zeros_like(d['n_actions'][:, :1])], dim=1)
            _, pol = opt.model_policy(states, obs)
            sampled = pol.rsample()
            qs = [q(states, torch.tanh(sampled), obs)[1] for q in opt.model_target_q_list]
            logp = sum_log_prob(squash_correction_log_prob(pol, sampled))
            pick = lambda sl: torch.stack([q[:, sl] for q in qs])[torch.randperm(E)[:opt.ensemble_q_sample]].min(0)[0].squeeze(-1)  # noqa: E731
            n_vs = pick(slice(None, -1)) - alpha * logp[:, :-1]
            next_n_vs = (1 - beta) * (pick(slice(1, None)) - alpha * logp[:, 1:]) + beta * vbar
            pi = squash_correction_prob(pol, torch.atanh(nx_actions))[:, :-1].prod(-1)
            return v_trace(d, d['n_mu'].prod(-1), pi, n_vs, next_n_vs)

    def v_trace(dd, mu, pi, n_vs, next_n_vs):
        td = dd['n_rewards'] + opt.gamma * ~dd['n_dones'] * next_n_vs - n_vs
        td = opt._lambda_ratio * (opt._gamma_ratio * td)
        ratio = pi / mu.clamp(min=1e-8)
        c = torch.minimum(ratio, opt.v_c)
        c = torch.cumprod(torch.cat([torch.ones_like(c[:, :1]), c[:, :-1]], dim=-1), dim=1)
        td = c * torch.minimum(ratio, opt.v_rho) * td * ~(dd['n_last'] | dd['n_pad'])
        return n_vs[:, 0:1] + td.sum(1, keepdim=True)

    def run():
        obs = [d['nx_obs']]
        obs0, state, action = [d['nx_obs'][:, 0]], d['nx_states'][:, 0], d['n_actions'][:, 0]
        with torch.no_grad():
            beta = opt.model_target_termination(d['nx_states'][:, :-1], [d['nx_obs'][:, :-1]]).squeeze(-1)
        c_q = [q(state, action, obs0)[1] for q in opt.model_q_list]
        c_y = get_y(beta, obs, d['nx_states'])
        t_q = [q(state, action, obs0)[1] for q in opt.model_target_q_list]
        loss = 0.
        for q, tq in zip(c_q, t_q):
            clipped = tq + torch.clamp(q - tq, -opt.clip_epsilon, opt.clip_epsilon)
            loss = loss + torch.mean(torch.maximum(functional.mse_loss(clipped, c_y, reduction='none'),
                                                   functional.mse_loss(q, c_y, reduction='none')))
        for o in o_q:
            o.zero_grad()
        loss.backward()
        for o in o_q:
            o.step()
        # policy, temperature
        _, pol = opt.model_policy(state, obs0)
        sampled = pol.rsample()
        logp = sum_log_prob(squash_correction_log_prob(pol, sampled), keepdim=True)
        qs = torch.stack([q(state, torch.tanh(sampled), obs0)[1] for q in opt.model_q_list])
        loss_pi = torch.mean(torch.exp(opt.log_c_alpha.detach()) * logp - qs[torch.randperm(E)[:opt.ensemble_q_sample]].min(0)[0])
        o_pi.zero_grad()
        loss_pi.backward(inputs=list(opt.model_policy.parameters()))
        o_pi.step()
        with torch.no_grad():
            _, pol = opt.model_policy(state, obs0)
            logp = sum_log_prob(squash_correction_log_prob(pol, pol.sample()), keepdim=True)
        loss_alpha = torch.mean(opt.log_c_alpha * (-logp + opt.target_c_alpha * opt.c_action_size))
        o_alpha.zero_grad()
        loss_alpha.backward(inputs=[opt.log_c_alpha])
        o_alpha.step()
        # termination
        term = opt.model_termination(state, obs0)
        loss_t = torch.mean(term * (c_y - d['v'].mean(-1, keepdim=True) + 0.05) * ~d['done'].unsqueeze(-1))
        o_term.zero_grad()
        loss_t.backward()
        o_term.step()
        # TD error
        with torch.no_grad():
            y = get_y(beta, obs, d['nx_states'])
            return torch.mean(torch.cat([torch.abs(q(state, action, obs0)[1] - y) for q in opt.model_q_list], -1), -1, keepdim=True)
    return run


def make_discrete(batch, n_step, sizes, fused):
    import asac_amd  # noqa: F401
    from algorithm.oc import OptionBase
    from tests import parity_utils as pu
    torch.manual_seed(0)
    return OptionBase(0, 'option_0', False, False, ['vector'], [(6,)], list(sizes), 0, None, pu.plugin('nn_oc_small'),
                      device='cuda:0', batch_size=batch, n_step=n_step, summary_path=None, write_summary_per_step=1e9,
                      hip_config={'fused_option_discrete': fused})


def discrete_inputs(B, n, O, sizes):
    d = inputs(B, n, O, A=sum(sizes))
    rng = np.random.default_rng(B + n + 1)
    onehot = np.concatenate([np.eye(s, dtype=np.float32)[rng.integers(0, s, (B, n))] for s in sizes], -1)
    d['n_actions'] = torch.from_numpy(onehot).cuda()
    return d


def discrete_sequence(opt, d):
    def run():
        obs = [d['nx_obs']]
        d_y, _ = opt.compute_rep_q_grads(d['v_next'], None, d['n_last'], d['n_pad'], obs, obs, d['nx_states'], d['nx_states'],
                                         d['n_actions'], None, d['n_rewards'], d['n_dones'], d['n_mu'], d['hidden'])
        opt.train_rep_q()
        opt.train_policy_alpha(d['n_pad'], [d['nx_obs'][:, :-1]], d['nx_states'], d['n_actions'], d['n_mu'])
        opt.compute_termination_grads(0.05, [d['nx_obs'][:, 0]], d['nx_states'][:, 0], d_y, d['v'], d['done'], None)
        opt.train_termination()
        return opt._get_td_error(d['v_next'], d['n_last'], d['n_pad'], obs, obs, d['nx_states'][:, 0], d['nx_states'],
                                 d['n_actions'], d['n_rewards'], d['n_dones'], d['n_mu'])
    return run


def discrete_pair(opt, d):
    """`compute_rep_q_grads` and `_get_td_error` alone: the two calls the switch changes"""
    def run():
        obs = [d['nx_obs']]
        opt.compute_rep_q_grads(d['v_next'], None, d['n_last'], d['n_pad'], obs, obs, d['nx_states'], d['nx_states'],
                                d['n_actions'], None, d['n_rewards'], d['n_dones'], d['n_mu'], d['hidden'])
        return opt._get_td_error(d['v_next'], d['n_last'], d['n_pad'], obs, obs, d['nx_states'][:, 0], d['nx_states'],
                                 d['n_actions'], d['n_rewards'], d['n_dones'], d['n_mu'])
    return run


def event_us(fn, reps):
    """HIP-event time of one call of `fn`, microseconds, over `reps` back-to-back calls"""
    for _ in range(10):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def discrete_main(args):
    sizes = tuple(int(x) for x in args.discrete.split(','))
    d = discrete_inputs(args.batch, args.n_step, args.options, sizes)
    row = {'discrete': list(sizes), 'batch': args.batch, 'n_step': args.n_step, 'options': args.options}
    rates, pair = {'on': [], 'off': []}, {'on': [], 'off': []}
    for rep in range(3):        # alternating order: on/off, off/on, on/off
        for name in (('on', 'off') if rep % 2 == 0 else ('off', 'on')):
            opt = make_discrete(args.batch, args.n_step, sizes, name == 'on')
            fn = discrete_sequence(opt, d)
            rates[name].append(round(timed(fn, args.sequences), 1))
            pair[name].append(round(event_us(discrete_pair(opt, d), args.sequences), 1))
            if rep == 0:
                row[f'{name}_launches'] = round(count_launches(fn), 1)
                row[f'{name}_pair_launches'] = round(count_launches(discrete_pair(opt, d)), 1)
            opt.close()
    for name in ('on', 'off'):
        row[f'{name}_sequences_per_s'] = sorted(rates[name])[1]
        row[f'{name}_runs'] = rates[name]
        row[f'{name}_rep_q_plus_td_us'] = sorted(pair[name])[1]
        row[f'{name}_rep_q_plus_td_us_runs'] = pair[name]
    row['on_faster_in_every_run'] = max(pair['on']) < min(pair['off'])
    print(json.dumps(row), flush=True)


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA) / 3.


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return reps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', type=int, default=300)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--n-step', type=int, default=4)
    ap.add_argument('--options', type=int, default=3)
    ap.add_argument('--discrete', default=None, help='branch sizes, e.g. 3,2: a pure-discrete option, switch on against off')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    if args.discrete:
        return discrete_main(args)
    d = inputs(args.batch, args.n_step, args.options)
    row = {'batch': args.batch, 'n_step': args.n_step, 'options': args.options}
    # each way is timed three times, the two ways interleaved (a drift of the box's clocks hits both); the median is reported
    rates = {'torch': [], 'native': []}
    for rep in range(3):
        for name, build in (('torch', torch_sequence), ('native', native_sequence)):
            opt = make(args.batch, args.n_step)
            fn = build(opt, d)
            rates[name].append(round(timed(fn, args.sequences), 1))
            if rep == 0:
                row[f'{name}_launches'] = round(count_launches(fn), 1)
            opt.close()
    for name, r in rates.items():
        row[f'{name}_sequences_per_s'] = sorted(r)[1]
        row[f'{name}_runs'] = r
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
