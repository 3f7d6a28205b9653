"""What one `choose_action_device` call costs with policy-based acting as one launch (csrc/act.hip,
`hip_config['fused_act']`) and as the eager tail of `_choose_action`, in one process on one box.  With the switch off the
call runs exactly the code of the commit before the launch, so this is the A/B against it without a second checkout.

    python tools/act_bench.py [--calls 300] [--warmup 50]

Configurations (stock `nn_vec` plugin, vector observation of 6, inputs resident on the device), each at 16 and 256 rows:
    discrete          d_action_sizes (3, 2)
    hybrid            d_action_sizes (3, 2), c_action_size 2
    continuous_noise  c_action_size 2, action_noise [0., 1.]
    discrete_deter    d_action_sizes (3, 2), disable_sample=True

Both learners of a configuration stay alive; the two ways alternate in rounds (off, on, off, on, ...: a drift of the box's
clocks hits both), every call ends in a device synchronise, and the median over all timed calls of a way is reported in
microseconds, with the library's entry points one call issues (`LaunchProfiler`).  One JSON line per row, then the table."""
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
ROWS = (16, 256)
CONFIGS = {
    'discrete': dict(d=(3, 2), c=0),
    'hybrid': dict(d=(3, 2), c=2),
    'continuous_noise': dict(d=(), c=2, kw=dict(action_noise=[0., 1.])),
    'discrete_deter': dict(d=(3, 2), c=0, acting=dict(disable_sample=True)),
}


def learner(cfg, fused):
    from algorithm.sac_base import SAC_Base
    from tests import parity_utils as pu
    torch.manual_seed(0)
    return SAC_Base(['vector'], [(6,)], list(cfg['d']), cfg['c'], None, pu.plugin('nn_vec'), device='cuda:0', n_step=3,
                    batch_size=16, replay_config={'capacity': 256}, hip_config={'use_graph': False, 'fused_act': fused},
                    **cfg.get('kw', {}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=300, help='timed calls per way and row (at least 200)')
    ap.add_argument('--warmup', type=int, default=50)
    args = ap.parse_args()
    calls = max(200, args.calls)
    import asac_amd  # noqa: F401
    from asac_amd import native
    rows_out = []
    for name, cfg in CONFIGS.items():
        agents = {fused: learner(cfg, fused) for fused in (False, True)}
        for rows in ROWS:
            rng = np.random.default_rng(rows)
            dev = agents[True].device
            obs = [torch.from_numpy(rng.standard_normal((rows, 6)).astype(np.float32)).to(dev)]
            pre = torch.zeros(rows, sum(cfg['d']) + cfg['c'], device=dev)
            hidden = torch.zeros(rows, *agents[True].seq_hidden_state_shape, device=dev)
            act = lambda a: a.choose_action_device(obs, pre, hidden, **cfg.get('acting', {}))      # noqa: E731
            times, native_calls = {False: [], True: []}, {}
            for fused, agent in agents.items():
                for _ in range(args.warmup):
                    act(agent)
                with native.LaunchProfiler(repeat=1) as prof:
                    act(agent)
                native_calls[fused] = {k: v['calls'] for k, v in prof.summary().items()}
            per_round = -(-calls // ROUNDS)
            for _ in range(ROUNDS):
                for fused, agent in agents.items():
                    torch.cuda.synchronize()
                    for _ in range(per_round):
                        t0 = time.perf_counter()
                        act(agent)
                        torch.cuda.synchronize()
                        times[fused].append(time.perf_counter() - t0)
            row = {'config': name, 'rows': rows, 'calls_per_way': len(times[True]),
                   'us_off': 1e6 * float(np.median(times[False])), 'us_on': 1e6 * float(np.median(times[True])),
                   'native_calls_off': sum(native_calls[False].values()), 'native_calls_on': sum(native_calls[True].values()),
                   'entry_points_on': native_calls[True]}
            row['off_over_on'] = row['us_off'] / row['us_on']
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        for agent in agents.values():
            agent.close()
    print('| configuration | rows | off, us / call | on, us / call | off / on | native calls off | native calls on |')
    print('|---|---|---|---|---|---|---|')
    for r in rows_out:
        print(f"| {r['config']} | {r['rows']} | {r['us_off']:.0f} | {r['us_on']:.0f} | {r['off_over_on']:.2f} | "
              f"{r['native_calls_off']} | {r['native_calls_on']} |")


if __name__ == '__main__':
    main()
