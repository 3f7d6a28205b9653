"""What the pure-discrete, policy-based learner's arithmetic around the networks costs as one launch per item
(csrc/discrete.hip, `hip_config['fused_discrete']`) and as the eager chain of small ATen launches, in one process on one box:

  step    train steps/s of `SAC_Base` at the sizes of bench.py's headline configuration (cfg2: batch 256, n_step 4, two
          critics, PER capacity 524288) with `d_action_sizes=[3, 2]` and no continuous action (captured step), and the
          launches of one eager step: the library's entry points from `LaunchProfiler`, every device kernel from torch's
          profiler.  With the flag off the step runs exactly the code of the commit before the discrete kernels, so this is
          the A/B against it without a second checkout; bench.py has no discrete configuration.

    python tools/discrete_bench.py [--steps 600] [--fill 16384] [--dqn-like | --hybrid] [--nets]

`--dqn-like`: the same A/B with `discrete_dqn_like=True` (critics only, double-DQN target; csrc/dqn.hip,
`hip_config['fused_dqn']`), and — acting is not part of the step's figure — the device kernels of ONE `choose_action` call in
train mode with the flag off and on, from torch's profiler.

`--nets`: the A/B of `hip_config['fused_discrete_nets']` (default off: the `eager` column is what a default learner runs) —
the branch stacks of the critics and the policy as head banks (csrc/head_bank.hip), everything around them as by default;
with `--dqn-like` on the DQN-like learner.
`--hybrid`: the same A/B on a hybrid action space, `d_action_sizes=[3, 2]` and `c_action_size=2` (csrc/hybrid.hip,
`hip_config['fused_hybrid']`, default off: the `eager` column is what a default learner runs).

The two ways alternate (off, on, off, on, ...: a drift of the box's clocks hits both) and every timed window ends in a device
synchronise; the median of the rounds is reported, all rounds are listed.  BOTH captured learners stay alive while the tool
alternates between them (two replay buffers, two graphs on one device); each runs alone while it is timed.  One JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROUNDS = 5
D_ACTION_SIZES = [3, 2]


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


C_ACTION_SIZE_HYBRID = 2


def step_row(steps, fill, dqn_like=False, hybrid=False, nets=False):
    import bench
    from asac_amd import native
    from algorithm.sac_base import SAC_Base
    from tests import parity_utils as pu
    cfg = bench.CONFIGS['cfg2']
    plugin = pu.plugin(cfg['plugin'])
    rng = np.random.default_rng(1)
    c_size = C_ACTION_SIZE_HYBRID if hybrid else 0
    episodes = [pu.synthetic_episode(rng, cfg['obs_shapes'], D_ACTION_SIZES, c_size, cfg['hidden'], cfg['episode_len'])
                for _ in range(max(4, fill // cfg['episode_len']))]

    flag, prefix = ('fused_dqn', 'asac_dqn_') if dqn_like else ('fused_discrete', 'asac_discrete_')
    if hybrid:
        flag, prefix = 'fused_hybrid', 'asac_hybrid_'
    if nets:       # the networks themselves: everything else as the default learner runs it
        flag, prefix = 'fused_discrete_nets', 'asac_head_bank_'

    def learner(fused, use_graph):
        torch.manual_seed(0)
        agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], D_ACTION_SIZES, c_size, None, plugin, device='cuda:0',
                         n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'], batch_size=cfg['batch_size'],
                         ensemble_q_num=cfg['ensemble_q_num'], ensemble_q_sample=cfg['ensemble_q_sample'],
                         replay_config={'capacity': cfg['capacity']}, discrete_dqn_like=dqn_like,
                         hip_config={'use_graph': use_graph, flag: fused})
        for ep in episodes:
            agent.put_episode(**ep)
        return agent

    agents = {}
    row = {'mode': 'step', 'nets': nets, 'dqn_like': dqn_like, 'd_action_sizes': D_ACTION_SIZES, 'c_action_size': c_size,
           'batch': cfg['batch_size'],
           'n_step': cfg['n_step'], 'steps': steps, 'rounds': ROUNDS}
    for fused in (False, True):
        tag = 'fused' if fused else 'eager'
        agent = learner(fused, False)
        agent.train()                # the eager step, counted
        with native.LaunchProfiler(repeat=1) as prof:
            agent.train()
        seen = prof.summary()
        row['native_launches_' + tag] = sum(v['calls'] for v in seen.values())
        row['discrete_launches_' + tag] = {k: v['calls'] for k, v in seen.items()
                                           if k.startswith(prefix) or k in ('asac_vtrace_return_direct',
                                                                            'asac_vtrace_return_min')}
        row['device_kernels_' + tag] = count_kernels(agent.train)
        if dqn_like:                 # one `choose_action` call in train mode, 8 agents
            obs = [torch.randn(8, *shape, device='cuda') for shape in cfg['obs_shapes']]
            act_args = (obs, torch.zeros(8, sum(D_ACTION_SIZES) + c_size, device='cuda'),
                        torch.zeros(8, *agent.seq_hidden_state_shape, device='cuda'))
            agent.choose_action_device(*act_args)
            row['acting_device_kernels_' + tag] = count_kernels(lambda: agent.choose_action_device(*act_args))
        agent.close()
        agent = learner(fused, True)
        for _ in range(20):          # eager warm-up, capture, first replays
            agent.train()
        torch.cuda.synchronize()
        assert agent._graph is not None, 'the step must capture'
        agents[fused] = agent
    runs = {False: [], True: []}
    for _ in range(ROUNDS):
        for fused in (False, True):
            agent = agents[fused]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                agent.train()
            torch.cuda.synchronize()
            runs[fused].append(round(steps / (time.perf_counter() - t0), 1))
    for agent in agents.values():
        agent.close()
    row.update(steps_per_s_eager=sorted(runs[False])[ROUNDS // 2], steps_per_s_fused=sorted(runs[True])[ROUNDS // 2],
               runs_eager=runs[False], runs_fused=runs[True])
    row['fused_over_eager'] = round(row['steps_per_s_fused'] / row['steps_per_s_eager'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--fill', type=int, default=16384, help='rows put into the replay before the first step')
    ap.add_argument('--dqn-like', action='store_true', help='discrete_dqn_like=True: the A/B of hip_config[\'fused_dqn\']')
    ap.add_argument('--hybrid', action='store_true', help='c_action_size=2 beside the branches: the A/B of hip_config[\'fused_hybrid\']')
    ap.add_argument('--nets', action='store_true', help='the A/B of hip_config[\'fused_discrete_nets\'] (the branch stacks as head banks); '
                                                         'with --dqn-like on the DQN-like learner')
    args = ap.parse_args()
    assert not (args.dqn_like and args.hybrid) and not (args.nets and args.hybrid), 'one A/B at a time'
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    print(json.dumps(step_row(args.steps, args.fill, args.dqn_like, args.hybrid, args.nets)), flush=True)


if __name__ == '__main__':
    main()
