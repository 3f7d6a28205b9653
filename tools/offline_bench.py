"""What the offline loss (`offline_enabled=True, offline_loss=True`: reference sac_base.py:1899-1900) costs the headline
learner with its term inside the policy-step launches (`hip_config['fused_offline']`, csrc/mlp.hip) and on the eager
branch, in one process on one box:

  offline_fused   `SAC_Base` at the sizes of bench.py's headline configuration (cfg2: vector observation 6, A = 2, batch
                  256, n_step 4, two critics, PER 2^19) with the offline loss, switch on
  offline_eager   the same learner, switch off: the code path of the commit before the kernels
  plain           the cfg2 learner without the loss, beside them

Per row: train steps/s of the captured step, and the launches of one eager step — the library's entry points from
`LaunchProfiler`, every device kernel from torch's profiler.  bench.py has no offline configuration.

    python tools/offline_bench.py [--steps 2000] [--fill 16384]

The three learners stay alive and are timed in turn (plain, eager, fused, plain, ...: a drift of the box's clocks hits all
three); every timed window ends in a device synchronise; the median of the rounds is reported, all rounds are listed.  One
JSON line."""
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
ROWS = {'plain': dict(kw={}, hip={}),
        'offline_eager': dict(kw=dict(offline_enabled=True, offline_loss=True), hip={'fused_offline': False}),
        'offline_fused': dict(kw=dict(offline_enabled=True, offline_loss=True), hip={'fused_offline': True})}


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def learner(cfg, plugin, row, use_graph, episodes):
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(0)
    agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], [], cfg['c_action_size'], None, plugin, device='cuda:0',
                     n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'], batch_size=cfg['batch_size'],
                     ensemble_q_num=cfg['ensemble_q_num'], ensemble_q_sample=cfg['ensemble_q_sample'],
                     replay_config={'capacity': cfg['capacity']}, hip_config={'use_graph': use_graph, **row['hip']},
                     **row['kw'])
    for ep in episodes:
        agent.put_episode(**ep)
    return agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--fill', type=int, default=16384, help='rows put into the replay before the first step')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    import bench
    from asac_amd import native
    from tests import parity_utils as pu
    cfg = bench.CONFIGS['cfg2']
    plugin = pu.plugin(cfg['plugin'])
    rng = np.random.default_rng(1)
    episodes = [pu.synthetic_episode(rng, cfg['obs_shapes'], [], cfg['c_action_size'], cfg['hidden'], cfg['episode_len'])
                for _ in range(max(4, args.fill // cfg['episode_len']))]
    out = {'config': 'cfg2', 'batch': cfg['batch_size'], 'n_step': cfg['n_step'], 'steps': args.steps, 'rounds': ROUNDS}
    agents = {}
    for name, row in ROWS.items():
        agent = learner(cfg, plugin, row, False, episodes)
        agent.train()
        with native.LaunchProfiler(repeat=1) as prof:
            agent.train()
        seen = prof.summary()
        out[name] = {'stock_path': bool(agent._stock_c_only()),
                     'native_launches': sum(v['calls'] for v in seen.values()),
                     'policy_step_launches': {k: v['calls'] for k, v in seen.items()
                                              if k.startswith(('asac_policy_step_fused', 'asac_mlp_backward_policy'))},
                     'device_kernels': count_kernels(agent.train)}
        agent.close()
        agent = learner(cfg, plugin, row, True, episodes)
        for _ in range(20):          # eager warm-up, capture, first replays
            agent.train()
        torch.cuda.synchronize()
        out[name]['captured'] = agent._graph is not None      # (a step that does not capture is timed as it runs: eagerly)
        agents[name] = agent
    runs = {name: [] for name in ROWS}
    for _ in range(ROUNDS):
        for name, agent in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                agent.train()
            torch.cuda.synchronize()
            runs[name].append(round(args.steps / (time.perf_counter() - t0), 1))
    for name, agent in agents.items():
        agent.close()
        out[name].update(steps_per_s=sorted(runs[name])[ROUNDS // 2], runs=runs[name])
    out['fused_over_eager'] = round(out['offline_fused']['steps_per_s'] / out['offline_eager']['steps_per_s'], 4)
    out['fused_over_plain'] = round(out['offline_fused']['steps_per_s'] / out['plain']['steps_per_s'], 4)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
