"""What a rotary position encoding in front of the attention core costs, as the epilogue of the projection launch
(csrc/rows_proj.hip, csrc/rope.hip; `seq_layers.FUSED_ROPE`) and as module code behind library GEMMs, per kind, in one process
on one box:

  step    train steps/s of `SAC_Base` at the sizes of bench.py's cfg_attn_h64 over tests/plugins/nn_attn_rope.py with its
          `PE_KIND` set to the kind (captured step), and the launches of one eager step: the library's entry points from
          `LaunchProfiler`, every device kernel from torch's profiler.  With FUSED_ROPE off the step runs exactly the code of
          the commit before the rope kernels, so this is the A/B against it without a second checkout; `tools/ab_rounds.sh`
          cannot reach a rotary layer, since no bench.py configuration has one.

    python tools/rope_bench.py [--kinds ROPE ROPE2] [--steps 600]

The two ways alternate (off, on, off, on, ...: a drift of the box's clocks hits both) and every timed window ends in a device
synchronise; the median of the runs is reported, all runs are listed.  BOTH captured learners of a kind stay alive while the
tool alternates between them (two replay buffers, two graphs on one device); each runs alone while it is timed.  One JSON line
per kind."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROUNDS = 3


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def step_rows(kind, steps):
    import bench
    import algorithm.nn_models as m
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    from tests import parity_utils as pu
    cfg = bench.CONFIGS['cfg_attn_h64']
    plugin = pu.plugin('nn_attn_rope')
    plugin.PE_KIND = m.POSITIONAL_ENCODING[kind]
    before = seq_layers.FUSED_ROPE
    agents, row = {}, {'mode': 'step', 'kind': kind, 'batch': cfg['batch_size'], 'steps': steps}
    for fused in (False, True):      # (FUSED_ROPE is read at every forward: each learner captures its step under its own setting)
        seq_layers.FUSED_ROPE = fused
        tag = 'fused' if fused else 'module'
        torch.manual_seed(0)
        agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], [], cfg['c_action_size'], None, plugin, device='cuda:0',
                         seq_encoder=SEQ_ENCODER.ATTN, n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'],
                         batch_size=cfg['batch_size'], replay_config={'capacity': cfg['capacity']}, hip_config={'use_graph': False})
        rng = np.random.default_rng(1)
        episodes = [pu.synthetic_episode(rng, cfg['obs_shapes'], [], cfg['c_action_size'], cfg['hidden'], cfg['episode_len'])
                    for _ in range(40)]
        for ep in episodes:
            agent.put_episode(**ep)
        agent.train()                # the eager step, counted
        with native.LaunchProfiler(repeat=1) as prof:
            agent.train()
        seen = prof.summary()
        row['native_launches_' + tag] = sum(v['calls'] for v in seen.values())
        row['rope_launches_' + tag] = {k: v['calls'] for k, v in seen.items() if k.startswith('asac_rope') or '_rope_' in k}
        row['device_kernels_' + tag] = count_kernels(agent.train)
        agent.close()
        torch.manual_seed(0)
        agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], [], cfg['c_action_size'], None, plugin, device='cuda:0',
                         seq_encoder=SEQ_ENCODER.ATTN, n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'],
                         batch_size=cfg['batch_size'], replay_config={'capacity': cfg['capacity']}, hip_config={'use_graph': True})
        for ep in episodes:
            agent.put_episode(**ep)
        for _ in range(20):          # eager warm-up, capture, first replays
            agent.train()
        torch.cuda.synchronize()
        assert agent._graph is not None, 'the step must capture'
        agents[fused] = agent
    seq_layers.FUSED_ROPE = before
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
    row.update(steps_per_s_module=sorted(runs[False])[ROUNDS // 2], steps_per_s_fused=sorted(runs[True])[ROUNDS // 2],
               runs_module=runs[False], runs_fused=runs[True])
    row['fused_over_module'] = round(row['steps_per_s_fused'] / row['steps_per_s_module'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kinds', nargs='+', default=['ROPE', 'ROPE2'])
    ap.add_argument('--steps', type=int, default=600)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    for kind in args.kinds:
        print(json.dumps(step_rows(kind, args.steps)), flush=True)


if __name__ == '__main__':
    main()
