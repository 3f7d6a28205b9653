"""What the gate behind an episode attention block costs, as one launch per pass (csrc/rows_gate.hip, `seq_layers.FUSED_GATE`)
and as the gate layer's module code, per gate kind, in one process on one box:

  block   forward + backward of `EpisodeMultiheadAttention(64, 2 layers, 8 heads, gate=kind)` over 1 024 windows of 9 (the
          learner's batch of cfg_attn_h64), eager: ms per pass and launches per pass
  step    train steps/s of `SAC_Base` at the sizes of bench.py's cfg_attn_h64 over tests/plugins/nn_attn_gate.py with its gate
          set to the kind (captured step).  With FUSED_GATE off the step runs exactly the code of the commit before the gate
          kernel, so this is the A/B against it without a second checkout; `tools/ab_rounds.sh` cannot reach a gate, since
          no bench.py configuration has one.

    python tools/gate_bench.py [--kinds RESIDUAL OUTPUT RECURRENT] [--reps 200] [--steps 600] [--no-step]

The two ways alternate (off, on, off, on, ...: a drift of the box's clocks hits both) and every timed window ends in a device
synchronise; the median of the runs is reported, all runs are listed.  Launches and the device's busy time per pass (the sum
of the kernels' durations: the eager pass is bound by the host, ~1 ms for ~45 launches, so its wall time hardly moves with
the launches it loses) are taken with torch's profiler outside the timing.  The step mode keeps BOTH captured learners of a
kind alive while it alternates between them (two replay buffers, two graphs on one device); each runs alone while it is
timed.  One JSON line per kind and mode."""
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


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    events = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    busy = sum(getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.) for e in events)
    return sum(e.count for e in events) / 3., busy / 3.


def timed_ms(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def block_rows(kind, reps):
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import seq_layers
    torch.manual_seed(0)
    attn = m.EpisodeMultiheadAttention(64, num_layers=2, num_heads=8, gate=m.GATE[kind]).cuda()
    B, L = 1024, 9
    key = torch.randn(B, L, 64, device='cuda')
    index = torch.arange(L, device='cuda').repeat(B, 1)
    pad = torch.arange(L, device='cuda').unsqueeze(0) < torch.randint(0, 3, (B, 1), device='cuda')
    h0 = torch.zeros(B, 1, attn.output_hidden_state_dim, device='cuda')

    def fn():
        for p in attn.parameters():
            p.grad = None
        kk = key.clone().requires_grad_(True)
        o, hn, _ = attn(kk, seq_q_len=L, hidden_state=h0, is_prev_hidden_state=True, key_index=index, key_padding_mask=pad)
        (o.sum() + hn.sum()).backward()

    row = {'mode': 'block', 'kind': kind, 'shape': [B, L, 64]}
    runs = {False: [], True: []}
    for rnd in range(ROUNDS):
        for fused in (False, True):
            seq_layers.FUSED_GATE = fused
            runs[fused].append(round(timed_ms(fn, reps), 4))
            if rnd == 0:
                tag = 'fused' if fused else 'module'
                launches, busy = count_launches(fn)
                row['launches_' + tag], row['device_us_' + tag] = round(launches, 1), round(busy, 1)
    seq_layers.FUSED_GATE = True
    row.update(ms_module=sorted(runs[False])[ROUNDS // 2], ms_fused=sorted(runs[True])[ROUNDS // 2],
               runs_module=runs[False], runs_fused=runs[True])
    row['fused_over_module'] = round(row['ms_fused'] / row['ms_module'], 4)
    return row


def step_rows(kind, steps):
    import bench
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import seq_layers
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    from tests import parity_utils as pu
    cfg = bench.CONFIGS['cfg_attn_h64']
    plugin = pu.plugin('nn_attn_gate')
    plugin.GATE_KIND = m.GATE[kind]
    agents = {}
    for fused in (False, True):      # (FUSED_GATE is read at every forward: each learner captures its step under its own setting)
        seq_layers.FUSED_GATE = fused
        torch.manual_seed(0)
        agent = SAC_Base(cfg['obs_names'], cfg['obs_shapes'], [], cfg['c_action_size'], None, plugin, device='cuda:0',
                         seq_encoder=SEQ_ENCODER.ATTN, n_step=cfg['n_step'], burn_in_step=cfg['burn_in_step'],
                         batch_size=cfg['batch_size'], replay_config={'capacity': cfg['capacity']}, hip_config={'use_graph': True})
        rng = np.random.default_rng(1)
        for _ in range(40):
            agent.put_episode(**pu.synthetic_episode(rng, cfg['obs_shapes'], [], cfg['c_action_size'], cfg['hidden'],
                                                     cfg['episode_len']))
        for _ in range(20):          # eager warm-up, capture, first replays
            agent.train()
        torch.cuda.synchronize()
        assert agent._graph is not None
        agents[fused] = agent
    seq_layers.FUSED_GATE = True
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
    row = {'mode': 'step', 'kind': kind, 'batch': cfg['batch_size'], 'steps': steps,
           'steps_per_s_module': sorted(runs[False])[ROUNDS // 2], 'steps_per_s_fused': sorted(runs[True])[ROUNDS // 2],
           'runs_module': runs[False], 'runs_fused': runs[True]}
    row['fused_over_module'] = round(row['steps_per_s_fused'] / row['steps_per_s_module'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kinds', nargs='+', default=['RESIDUAL', 'OUTPUT', 'RECURRENT'])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    for kind in args.kinds:
        print(json.dumps(block_rows(kind, args.reps)), flush=True)
        if not args.no_step:
            print(json.dumps(step_rows(kind, args.steps)), flush=True)


if __name__ == '__main__':
    main()
