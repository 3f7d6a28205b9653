"""What the siamese representation losses cost as one launch an encoder (csrc/siamese.hip, `hip_config['fused_siamese']`)
and as today's eager chain, in one process on one box:

  call    `SAC_Base._train_siamese_representation_learning` alone on a synthetic window (no Q-consistency term, no adaptive
          gating: the loss, both backward passes, the head's Adam step): microseconds a call, the library's launches
          (`LaunchProfiler`) and every device kernel (torch's profiler) of one call, and the peak of
          `torch.cuda.max_memory_allocated` over one call above what was allocated before it.
  step    train steps/s of the whole captured step with the head.

Shapes: usv_search's (batch 256, n-step 3, encoder width 16) with ATC and with BYOL, and a large one (batch 1 024, n-step 4,
width 64) with ATC.  The learner is the vector plugin of the tests with the encoder at the asked width.

    python tools/siamese_bench.py [--calls 300] [--steps 300] [--fill 8192] [--no-step]

With the switch off the learner runs exactly the code of the commit before the kernels, so this is the A/B against it without
a second checkout.  The two ways alternate (off, on, off, on, ...) and every timed window ends in a device synchronise; the
median of the rounds is reported, all rounds are listed.  One JSON line per row."""
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
SHAPES = [('ATC', 256, 3, 16), ('BYOL', 256, 3, 16), ('ATC', 1024, 4, 64)]      # (siamese, batch, n_step, encoder width)
OBS = 6


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def plugin_of_width(width):
    """tests/plugins/nn_vec_full.py's models with the encoder `width` wide"""
    import algorithm.nn_models as m
    from torch import nn
    from tests import parity_utils as pu
    base = pu.plugin('nn_vec_full')

    class ModelRep(base.ModelRep):
        def _build_model(self):
            self.enc = m.LinearLayers(self.obs_shapes[0][0], dense_n=width, dense_depth=1)
            self.dense = nn.Sequential(nn.Linear(width, 8), nn.Tanh())

    ns = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if k.startswith('Model')})
    ns.ModelRep = ModelRep
    return ns


def learner(siamese, batch, n_step, width, fused, use_graph, episodes=()):
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SIAMESE
    torch.manual_seed(0)
    agent = SAC_Base(['vector'], [(OBS,)], [], 2, None, plugin_of_width(width), device='cuda:0', batch_size=batch,
                     n_step=n_step, burn_in_step=2, replay_config={'capacity': 32768}, siamese=SIAMESE[siamese],
                     hip_config={'use_graph': use_graph, 'fused_siamese': fused})
    for ep in episodes:
        agent.put_episode(**ep)
    return agent


def alternate(run):
    runs = {False: [], True: []}
    for _ in range(ROUNDS):
        for fused in (False, True):
            runs[fused].append(round(run(fused), 2))
    return runs


def median(xs):
    return sorted(xs)[len(xs) // 2]


def call_row(siamese, batch, n_step, width, calls):
    from asac_amd import native
    gen = torch.Generator().manual_seed(0)
    obs = [torch.randn(batch, n_step, OBS, generator=gen).cuda()]
    pad = (torch.rand(batch, n_step, generator=gen) < 0.2).cuda()
    agents = {fused: learner(siamese, batch, n_step, width, fused, False) for fused in (False, True)}
    row = {'mode': 'call', 'siamese': siamese, 'batch': batch, 'n_step': n_step, 'width': width, 'rows': batch * n_step,
           'calls': calls, 'rounds': ROUNDS}

    def one(agent):
        return agent._train_siamese_representation_learning(None, None, None, pad, obs, None, None)

    losses = {}
    for fused, agent in agents.items():
        tag = 'fused' if fused else 'eager'
        for _ in range(3):
            one(agent)
        with native.LaunchProfiler(repeat=1) as prof:
            losses[fused] = float(one(agent)[0])
        seen = prof.summary()
        row['native_launches_' + tag] = sum(v['calls'] for v in seen.values())
        row['siamese_launches_' + tag] = {k: v['calls'] for k, v in seen.items() if k.startswith('asac_siamese_')}
        row['device_kernels_' + tag] = count_kernels(lambda: one(agent))
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        one(agent)
        torch.cuda.synchronize()
        row['peak_bytes_' + tag] = torch.cuda.max_memory_allocated() - held

    def run(fused):
        agent = agents[fused]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            one(agent)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / calls

    runs = alternate(run)
    for agent in agents.values():
        agent.close()
    row.update(us_eager=median(runs[False]), us_fused=median(runs[True]), runs_eager=runs[False], runs_fused=runs[True],
               loss_after_4_calls_eager=losses[False], loss_after_4_calls_fused=losses[True])
    row['eager_over_fused'] = round(row['us_eager'] / row['us_fused'], 4)
    return row


def step_row(siamese, batch, n_step, width, steps, fill):
    from tests import parity_utils as pu
    rng = np.random.default_rng(1)
    episodes = [pu.synthetic_episode(rng, [(OBS,)], [], 2, (0,), 200) for _ in range(max(4, fill // 200))]
    agents = {}
    for fused in (False, True):
        agent = learner(siamese, batch, n_step, width, fused, True, episodes)
        for _ in range(20):          # eager warm-up, capture, first replays
            agent.train()
        torch.cuda.synchronize()
        agents[fused] = agent
    row = {'mode': 'step', 'siamese': siamese, 'batch': batch, 'n_step': n_step, 'width': width, 'steps': steps, 'rounds': ROUNDS,
           'captured_eager': agents[False]._graph is not None, 'captured_fused': agents[True]._graph is not None}

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
    row.update(steps_per_s_eager=median(runs[False]), steps_per_s_fused=median(runs[True]), runs_eager=runs[False],
               runs_fused=runs[True])
    row['fused_over_eager'] = round(row['steps_per_s_fused'] / row['steps_per_s_eager'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--fill', type=int, default=8192, help='rows put into the replay before the first step')
    ap.add_argument('--no-step', action='store_true', help='the head alone, not the whole train step')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    for shape in SHAPES:
        print(json.dumps(call_row(*shape, args.calls)), flush=True)
        if not args.no_step:
            print(json.dumps(step_row(*shape, args.steps, args.fill)), flush=True)


if __name__ == '__main__':
    main()
