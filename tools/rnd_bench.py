"""What random network distillation costs the headline learner (`use_rnd=True`, continuous actions, stock networks) on its
two launches (csrc/rnd.hip, `hip_config['fused_rnd']`) and as today's eager chain, in one process on one box:

  step    train steps/s of `SAC_Base` at the sizes of bench.py's headline configuration (cfg2: vector observation 6, A = 2,
          batch 256, n_step 4, two critics) with `use_rnd=True` (captured step), and the launches of one eager step: the
          library's entry points from `LaunchProfiler`, every device kernel from torch's profiler.
  acting  `choose_action_device` calls/s in train mode at batch 10 and 100 with `rnd_n_sample` 10 and 50, and the device
          kernels of one call.

With the flag off both run exactly the code of the commit before the kernels, so this is the A/B against it without a second
checkout; bench.py has no `use_rnd` configuration.

    python tools/rnd_bench.py [--steps 600] [--calls 300] [--fill 16384] [--discrete 3[,2,..]]

`--discrete SIZES` measures the pure-discrete, policy-based learner instead (csrc/drnd.hip, `hip_config['fused_rnd_discrete']`:
branches of these sizes, no continuous action, the plugin `nn_vec_full` — the mountain-car shape is `--discrete 3`), acting at
(batch, rnd_n_sample) = (10, 10) and (100, 50); flag off is again the code of the commit before.

The two ways alternate (off, on, off, on, ...: a drift of the box's clocks hits both) and every timed window ends in a device
synchronise; the median of the rounds is reported, all rounds are listed.  BOTH learners stay alive while the tool alternates
between them; each runs alone while it is timed.  One JSON line per row."""
import argparse
import json
import sys
import time
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROUNDS = 5
ACTING = [(10, 10), (10, 50), (100, 10), (100, 50)]      # (batch, rnd_n_sample)


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def plugin_with_rnd(base):
    """the configuration's plugin plus the stock `ModelRND` (`use_rnd=True` asks the plugin for it)"""
    import algorithm.nn_models as m
    ns = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if k.startswith('Model')})
    if not hasattr(ns, 'ModelRND'):
        ns.ModelRND = m.ModelRND
    return ns


def mode_of(sizes):
    """what a run measures: the branch sizes (--discrete; then no continuous action), the switch and its launches' prefix"""
    if sizes:
        return types.SimpleNamespace(sizes=list(sizes), flag='fused_rnd_discrete', prefix='asac_drnd_')
    return types.SimpleNamespace(sizes=[], flag='fused_rnd', prefix='asac_rnd_')


def action_sizes(cfg, mode):
    return (list(mode.sizes), 0) if mode.sizes else ([], cfg['c_action_size'])


def learner(cfg, plugin, mode, fused, use_graph, episodes=(), **kw):
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(0)
    d_sizes, c_size = action_sizes(cfg, mode)
    agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], d_sizes, c_size, None, plugin, device='cuda:0',
                     n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'], batch_size=cfg['batch_size'],
                     ensemble_q_num=cfg['ensemble_q_num'], ensemble_q_sample=cfg['ensemble_q_sample'],
                     replay_config={'capacity': cfg['capacity']}, use_rnd=True,
                     hip_config={'use_graph': use_graph, mode.flag: fused}, **kw)
    for ep in episodes:
        agent.put_episode(**ep)
    return agent


def alternate(run, rounds=ROUNDS):
    """run(fused) -> a rate; off / on alternating -> {fused: [rates]}"""
    runs = {False: [], True: []}
    for _ in range(rounds):
        for fused in (False, True):
            runs[fused].append(round(run(fused), 1))
    return runs


def step_row(cfg, plugin, mode, steps, fill):
    from asac_amd import native
    from tests import parity_utils as pu
    rng = np.random.default_rng(1)
    episodes = [pu.synthetic_episode(rng, cfg['obs_shapes'], *action_sizes(cfg, mode), cfg['hidden'], cfg['episode_len'])
                for _ in range(max(4, fill // cfg['episode_len']))]
    agents = {}
    row = {'mode': 'step', 'discrete': list(mode.sizes), 'batch': cfg['batch_size'], 'n_step': cfg['n_step'], 'steps': steps,
           'rounds': ROUNDS}
    for fused in (False, True):
        tag = 'fused' if fused else 'eager'
        agent = learner(cfg, plugin, mode, fused, False, episodes)
        agent.train()                # the eager step, counted
        with native.LaunchProfiler(repeat=1) as prof:
            agent.train()
        seen = prof.summary()
        row['native_launches_' + tag] = sum(v['calls'] for v in seen.values())
        row['rnd_launches_' + tag] = {k: v['calls'] for k, v in seen.items() if k.startswith(mode.prefix)}
        row['device_kernels_' + tag] = count_kernels(agent.train)
        agent.close()
        agent = learner(cfg, plugin, mode, fused, True, episodes)
        for _ in range(20):          # eager warm-up, capture, first replays
            agent.train()
        torch.cuda.synchronize()
        assert agent._graph is not None, 'the step must capture'
        agents[fused] = agent

    def run(fused):
        agent = agents[fused]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            agent.train()
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)

    runs = alternate(run)
    for agent in agents.values():
        agent.close()
    row.update(steps_per_s_eager=sorted(runs[False])[ROUNDS // 2], steps_per_s_fused=sorted(runs[True])[ROUNDS // 2],
               runs_eager=runs[False], runs_fused=runs[True])
    row['fused_over_eager'] = round(row['steps_per_s_fused'] / row['steps_per_s_eager'], 4)
    return row


def acting_row(cfg, plugin, mode, batch, k, calls):
    agents = {fused: learner(cfg, plugin, mode, fused, False, rnd_n_sample=k) for fused in (False, True)}
    obs = [torch.randn(batch, *shape, device='cuda') for shape in cfg['obs_shapes']]
    args = (obs, torch.zeros(batch, sum(mode.sizes) if mode.sizes else cfg['c_action_size'], device='cuda'),
            torch.zeros(batch, *agents[True].seq_hidden_state_shape, device='cuda'))
    row = {'mode': 'acting', 'batch': batch, 'rnd_n_sample': k, 'calls': calls, 'rounds': ROUNDS}
    for fused, agent in agents.items():
        for _ in range(3):
            agent.choose_action_device(*args)
        row['device_kernels_' + ('fused' if fused else 'eager')] = count_kernels(lambda: agent.choose_action_device(*args))

    def run(fused):
        agent = agents[fused]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            agent.choose_action_device(*args)
        torch.cuda.synchronize()
        return calls / (time.perf_counter() - t0)

    runs = alternate(run)
    for agent in agents.values():
        agent.close()
    row.update(calls_per_s_eager=sorted(runs[False])[ROUNDS // 2], calls_per_s_fused=sorted(runs[True])[ROUNDS // 2],
               runs_eager=runs[False], runs_fused=runs[True])
    row['fused_over_eager'] = round(row['calls_per_s_fused'] / row['calls_per_s_eager'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--fill', type=int, default=16384, help='rows put into the replay before the first step')
    ap.add_argument('--discrete', default='', help='branch sizes, e.g. 3 or 3,2: the pure-discrete learner (csrc/drnd.hip)')
    args = ap.parse_args()
    mode = mode_of([int(v) for v in args.discrete.split(',')] if args.discrete else [])
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    import bench
    from tests import parity_utils as pu
    cfg = bench.CONFIGS['cfg2']
    plugin = plugin_with_rnd(pu.plugin('nn_vec_full' if mode.sizes else cfg['plugin']))
    print(json.dumps(step_row(cfg, plugin, mode, args.steps, args.fill)), flush=True)
    for batch, k in ([(10, 10), (100, 50)] if mode.sizes else ACTING):
        print(json.dumps(acting_row(cfg, plugin, mode, batch, k, args.calls)), flush=True)


if __name__ == '__main__':
    main()
