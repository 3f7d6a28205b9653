"""Episodes/s and launches per step of behaviour cloning (`algorithm/imitation_base.ImitationBase`), three ways in one
process and in this order, per configuration (`mlp`: stock networks on vector observations, `rnn`: GRU representation)
and episode length T in {64, 512}:

  (a) torch    the PyTorch-ROCm composition of the reference's lines: `get_l_states`, `model_policy`, `Normal.log_prob`
               and `entropy`, `torch.optim.Adam` over the same modules (plain ATen backward, no bucket padding)
  (b) eager    the native path with `hip_config={'use_graph': False}`
  (c) graph    the native path, one hipGraph per bucket

    python tools/imitation_bench.py [--episodes 300] [--kernel-only]

Episodes are device tensors; every timed window ends in a device synchronise.  Launches per step are counted with
torch's profiler over three steps outside the timing (for (c): the kernels the replayed graph runs).
`--kernel-only` launches `asac_bc_loss_grad` alone at T x A = 512 x 4 and 4096 x 8 (200 launches each): run it under
`rocprofv3 --kernel-trace --stats -- python tools/imitation_bench.py --kernel-only` and read `k_bc_loss_grad`."""
import argparse
import json
import sys
import time
from itertools import chain
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CONFIGS = {'mlp': ('nn_vec', {}), 'rnn': ('nn_rnn', dict(seq_encoder='RNN'))}


def make(config, use_graph):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import convert_config_to_enum
    from tests import parity_utils as pu
    plugin, kw = CONFIGS[config]
    kw = dict(kw)
    convert_config_to_enum(kw)
    torch.manual_seed(0)
    return SAC_Base(['vector'], [(6,)], [], 2, None, pu.plugin(plugin), device='cuda:0', batch_size=32,
                    replay_config={'capacity': 512}, write_summary_per_step=1e9, save_model_per_step=1e9,
                    hip_config={'use_graph': use_graph}, **kw)


def episode(T):
    rng = np.random.default_rng(T)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return ([dev(rng.standard_normal((1, T, 6)).astype(np.float32))], dev(rng.random((1, T, 2)).astype(np.float32)),
            dev(rng.standard_normal((1, T)).astype(np.float32)), dev(rng.random((1, T)) < 0.5))


def torch_step_fn(sac):
    """the reference's lines on the learner's own modules (its fused layers run their plain autograd forms)"""
    from algorithm.utils.operators import gen_n_pre_actions
    opt = torch.optim.Adam(chain(sac.model_rep.parameters(), sac.model_policy.parameters()), lr=sac.learning_rate)

    def step(obses, actions, rewards, dones):
        T = actions.shape[1]
        idx = torch.arange(0, T, dtype=torch.int32, device=sac.device).unsqueeze(0)
        pad = torch.zeros_like(idx, dtype=torch.bool)
        pad[:, -1] = True
        pre = gen_n_pre_actions(actions, keep_last_action=False)
        hidden = sac.get_initial_seq_hidden_state(1, get_numpy=False).unsqueeze(1).repeat_interleave(T, dim=1)
        states, _ = sac.get_l_states(idx, pad, obses, pre, hidden, is_target=False)
        _, c_policy = sac.model_policy(states, obses)
        loss = torch.mean(-c_policy.log_prob(actions[:, :, sac.d_action_summed_size:]) - 0.1 * c_policy.entropy())
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def count_launches(fn, ep):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            fn(*ep)
        torch.cuda.synchronize()
    n = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    return n / 3.


def timed(fn, ep, episodes):
    for _ in range(10):
        fn(*ep)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(episodes):
        fn(*ep)
    torch.cuda.synchronize()
    return episodes / (time.perf_counter() - t0)


def kernel_only():
    import asac_amd  # noqa: F401
    from asac_amd import native
    native.load()
    for T, A in ((512, 4), (4096, 8)):
        loc, scale = torch.randn(T, A, device='cuda'), torch.rand(T, A, device='cuda') + 0.1
        action = torch.rand(T, A, device='cuda')
        tv = torch.tensor([T], dtype=torch.int32, device='cuda')
        loss, dl, ds = torch.empty(1, device='cuda'), torch.empty_like(loc), torch.empty_like(loc)
        for _ in range(200):
            native.bc_loss_grad(loc, scale, action, 0, tv, 0.1, loss, dl, ds)
        torch.cuda.synchronize()
        print(json.dumps({'kernel': 'k_bc_loss_grad', 'T': T, 'A': A, 'launches': 200,
                          'bytes_per_launch': 5 * T * A * 4}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=300)
    ap.add_argument('--kernel-only', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    if args.kernel_only:
        return kernel_only()
    import asac_amd  # noqa: F401  (puts the package's `algorithm` on the path)
    from algorithm.imitation_base import ImitationBase
    for config in CONFIGS:
        for T in (64, 512):
            ep = episode(T)
            row = {'config': config, 'T': T}
            sac = make(config, False)
            fn = torch_step_fn(sac)
            row['torch_eps_per_s'] = round(timed(fn, ep, args.episodes), 1)
            row['torch_launches'] = round(count_launches(fn, ep), 1)
            sac.close()
            for name, use_graph in (('eager', False), ('graph', True)):
                sac = make(config, use_graph)
                imit = ImitationBase(sac)
                fn = lambda *e: imit._train_one(e[0], e[1])  # noqa: E731  (the device work of `train`)
                row[f'{name}_eps_per_s'] = round(timed(fn, ep, args.episodes), 1)
                row[f'{name}_launches'] = round(count_launches(fn, ep), 1)
                assert imit.captures == int(use_graph)
                sac.close()
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
