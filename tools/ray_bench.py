"""What the ray-sensor encoder's convolution stack costs as one launch per pass (csrc/conv1d.hip, `image_layers.FUSED_CONV1D`)
and as module code (permute, two library convolutions, two activations and their backward), in one process on one box, at
the reference's two ray counts (L = 400: envs/ugv/ugv_parking, L = 61: envs/usv/usv_escort; C = 2):

  layer   forward + backward of `Conv1dLayers(L, 2, 'default', out_dense_n=64, out_dense_depth=2)` over N = 256 x window
          rays, captured as a hipGraph and replayed, so that the figure is the device's time and not the host's cost of
          issuing a dozen launches: us per pass between HIP events
  step    train steps/s of `SAC_Base` (batch 256, n_step = window - 1) over tests/plugins/nn_ray.py with its rays set to L
          (captured step)

    python tools/ray_bench.py [--lengths 400 61] [--window 4] [--reps 300] [--steps 600] [--no-step]

The two ways alternate (off, on, off, on, ...: a drift of the box's clocks hits both) and every timed window ends in a device
synchronise; the median of the runs is reported, all runs are listed.  One JSON line."""
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


def _median(v):
    return sorted(v)[len(v) // 2]


def layer_row(L, window, reps):
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import image_layers
    torch.manual_seed(0)
    layer = m.Conv1dLayers(L, 2, 'default', out_dense_n=64, out_dense_depth=2).cuda()
    N = 256 * window
    x = torch.randn(256, window, L, 2, device='cuda')
    gy = torch.randn(256, window, 64, device='cuda')
    for p in layer.parameters():
        p.grad = torch.zeros_like(p)

    def fn():
        (layer(x) * gy).sum().backward()

    graphs = {}
    for fused in (False, True):     # (FUSED_CONV1D is read at every forward: each graph holds the launches of its setting)
        image_layers.FUSED_CONV1D = fused
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[fused] = g
    image_layers.FUSED_CONV1D = True
    runs = {False: [], True: []}
    for _ in range(ROUNDS):
        for fused in (False, True):
            g = graphs[fused]
            for _ in range(10):
                g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            runs[fused].append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
    row = {'L': L, 'N': N, 'us_module': _median(runs[False]), 'us_fused': _median(runs[True]),
           'runs_module': runs[False], 'runs_fused': runs[True]}
    row['fused_over_module'] = round(row['us_fused'] / row['us_module'], 4)
    return row


def step_row(L, window, steps):
    from algorithm.nn_models.layers import image_layers
    from algorithm.sac_base import SAC_Base
    from tests import parity_utils as pu
    plugin = pu.plugin('nn_ray')
    plugin.RAY_SIZE = L
    shapes = [(L, 2), (6,)]
    agents = {}
    for fused in (False, True):      # (each learner captures its step under its own setting)
        image_layers.FUSED_CONV1D = fused
        torch.manual_seed(0)
        agent = SAC_Base(['ray', 'vector'], shapes, [], 3, None, plugin, device='cuda:0', n_step=window - 1, batch_size=256,
                         replay_config={'capacity': 1 << 14}, hip_config={'use_graph': True})
        rng = np.random.default_rng(1)
        for _ in range(20):
            agent.put_episode(**pu.synthetic_episode(rng, shapes, [], 3, (0,), 100))
        for _ in range(20):          # eager warm-up, capture, first replays
            agent.train()
        torch.cuda.synchronize()
        assert agent._graph is not None
        agents[fused] = agent
    image_layers.FUSED_CONV1D = True
    plugin.RAY_SIZE = 61
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
    row = {'L': L, 'batch': 256, 'window': window, 'steps': steps, 'steps_per_s_module': _median(runs[False]),
           'steps_per_s_fused': _median(runs[True]), 'runs_module': runs[False], 'runs_fused': runs[True]}
    row['fused_over_module'] = round(row['steps_per_s_fused'] / row['steps_per_s_module'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lengths', nargs='+', type=int, default=[400, 61])
    ap.add_argument('--window', type=int, default=4)
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    out = {'tool': 'ray_bench', 'channels': 2, 'window': args.window, 'layer': [], 'step': []}
    for L in args.lengths:
        out['layer'].append(layer_row(L, args.window, args.reps))
        if not args.no_step:
            out['step'].append(step_row(L, args.window, args.steps))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
