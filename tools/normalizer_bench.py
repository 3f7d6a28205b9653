"""What `use_normalization=True` costs the headline learner with the whitening as one launch a step in front of the plugin's
own representation class (`hip_config['fused_normalizer']`, csrc/normalize.hip) and inside a `NormalizedRep` subclass, in one
process on one box:

  norm_fused   `SAC_Base` at the sizes of bench.py's headline configuration (cfg2: vector observation 6, A = 2, batch 256,
               n_step 4, two critics, PER 2^19) with `use_normalization`, switch on
  norm_eager   the same learner, switch off (the default): the code path of the commit before the kernels
  plain        the cfg2 learner without normalization, beside them: the ceiling

Per row: train steps/s of the captured step, and the launches of one eager step — the library's entry points from
`LaunchProfiler`, every device kernel from torch's profiler.  And, for both normalized rows, microseconds per `put_episode`
of T = 1 000 rows (host time between device synchronisations, the replay's own ingest included) for the 6-wide vector and
for a learner with an 84 x 84 x 3 frame.  bench.py has no normalized configuration.

    python tools/normalizer_bench.py [--steps 2000] [--fill 16384] [--puts 20]

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
        'norm_eager': dict(kw=dict(use_normalization=True), hip={'fused_normalizer': False}),
        'norm_fused': dict(kw=dict(use_normalization=True), hip={'fused_normalizer': True})}


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


def put_episode_us(pu, plugin_name, obs_names, obs_shapes, c_action_size, hip, puts, T=1000):
    """median host microseconds of one `put_episode` of T rows, device tensors in, synchronised on both sides"""
    from algorithm.sac_base import SAC_Base
    torch.manual_seed(0)
    agent = SAC_Base(obs_names, obs_shapes, [], c_action_size, None, pu.plugin(plugin_name), device='cuda:0', n_step=3,
                     batch_size=8, replay_config={'capacity': 4096}, use_normalization=True,
                     hip_config={'use_graph': False, **hip})
    rng = np.random.default_rng(2)
    ep = pu.synthetic_episode(rng, obs_shapes, [], c_action_size, tuple(agent.seq_hidden_state_shape), T)
    dev = {k: ([torch.from_numpy(o).cuda() for o in v] if isinstance(v, list) else torch.from_numpy(v).cuda())
           for k, v in ep.items()}
    times = []
    for i in range(puts + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.put_episode(**dev)
        torch.cuda.synchronize()
        if i >= 3:
            times.append(1e6 * (time.perf_counter() - t0))
    agent.close()
    return round(sorted(times)[len(times) // 2], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--fill', type=int, default=16384, help='rows put into the replay before the first step')
    ap.add_argument('--puts', type=int, default=20, help='timed put_episode calls a row')
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
        out[name] = {'stock_path': bool(agent._stock_c_only()), 'stock_rep_class': type(agent.model_rep) is plugin.ModelRep,
                     'native_launches': sum(v['calls'] for v in seen.values()),
                     'whiten_launches': seen.get('asac_obs_whiten', {}).get('calls', 0),
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
    out['fused_over_eager'] = round(out['norm_fused']['steps_per_s'] / out['norm_eager']['steps_per_s'], 4)
    out['fused_over_plain'] = round(out['norm_fused']['steps_per_s'] / out['plain']['steps_per_s'], 4)
    for name in ('norm_eager', 'norm_fused'):
        hip = ROWS[name]['hip']
        out[name]['put_episode_us_T1000'] = {
            'vector_6': put_episode_us(pu, 'nn_vec', ['vector'], [(6,)], 2, hip, args.puts),
            'vector_10_frame_84x84x3': put_episode_us(pu, 'nn_conv84_small', ['vector', 'image'], [(10,), (3, 84, 84)], 4, hip,
                                                      args.puts)}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
