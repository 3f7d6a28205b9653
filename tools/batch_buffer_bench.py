"""Steps/s of the training mode without a replay buffer (`use_replay_buffer=False`: the HBM episode batch queue) against
the replay mode, at the cfg2 shape (batch 256, n_step 4, vector observations) and at an image shape (the conv plugin,
3 x 30 x 30 frames, batch 64).  Both modes run the captured step, plain `train()` calls; the batch mode is refilled by
`put_episode` between timed runs (outside the timing) so that every timed step has a batch.

    python tools/batch_buffer_bench.py [--steps 200] [--shape cfg2|image|all]

The two kernels' own times and bytes: run it under `rocprofv3 --kernel-trace --stats -- python tools/batch_buffer_bench.py`
and read `k_batch_put` / `k_batch_pop_gather` from the stats file; the batch-mode lines carry the bytes each launch moves."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {
    'cfg2': dict(plugin='nn_vec', obs_names=['vector'], obs_shapes=[(6,)], c_action_size=2, batch_size=256,
                 kw=dict(n_step=4), ep_len=200),
    'image': dict(plugin='nn_conv', obs_names=['vector', 'image'], obs_shapes=[(10,), (3, 30, 30)], c_action_size=4,
                  batch_size=64, kw=dict(n_step=3, burn_in_step=5, ensemble_q_num=4, ensemble_q_sample=2), ep_len=100),
}


def _episode(rng, shape, T):
    from tests import parity_utils as pu
    return pu.synthetic_episode(rng, shape['obs_shapes'], [], shape['c_action_size'], (0,), T)


def run(shape_name, replay: bool, steps: int):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    from tests import parity_utils as pu
    sh = SHAPES[shape_name]
    kw = dict(sh['kw'])
    convert_config_to_enum(kw)
    agent = SAC_Base(sh['obs_names'], sh['obs_shapes'], [], sh['c_action_size'], None, pu.plugin(sh['plugin']),
                     device='cuda:0', batch_size=sh['batch_size'], use_replay_buffer=replay,
                     replay_config={'capacity': 1 << 16} if replay else None, write_summary_per_step=1e9,
                     save_model_per_step=1e9, **kw)
    rng = np.random.default_rng(0)
    T, B = sh['ep_len'], sh['batch_size']
    eps = [_episode(rng, sh, T) for _ in range(4)]
    per_put = (T - 1) // B

    def fill():
        if replay:
            return
        while len(agent.batch_buffer) < agent.batch_buffer.max_size - per_put:
            agent.put_episode(**eps[int(rng.integers(0, len(eps)))])

    for ep in eps:
        agent.put_episode(**ep)
    for _ in range(10):       # eager warm-up, capture, first replays
        fill()
        agent.train()
    torch.cuda.synchronize()
    elapsed, done = 0.0, 0
    while done < steps:
        fill()
        k = steps - done if replay else min(steps - done, len(agent.batch_buffer))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            agent.train()
        torch.cuda.synchronize()
        elapsed += time.perf_counter() - t0
        done += k
    out = dict(shape=shape_name, mode='replay' if replay else 'batch', steps=done, steps_per_s=round(done / elapsed, 1),
               captured=agent._graph is not None)
    if not replay:
        bb = agent.batch_buffer
        row = sum(t.element_size() * int(np.prod(t.shape[2:], dtype=np.int64)) for t in bb._pool.values())
        row_out = sum(t.element_size() * int(np.prod(t.shape[2:], dtype=np.int64)) for t in bb._batch.values())
        out['pop_gather_bytes'] = B * bb.L * (row + row_out)
        out['put_bytes_per_window'] = bb.L * row
    agent.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--shape', default='all', choices=['all', *SHAPES])
    a = ap.parse_args()
    for name in (SHAPES if a.shape == 'all' else [a.shape]):
        for replay in (True, False):
            print(json.dumps(run(name, replay, a.steps)), flush=True)


if __name__ == '__main__':
    main()
