"""What attention-weight dropout inside the multi-head attention launches costs and saves (csrc/attn_mh.hip with DROP,
csrc/asac_dropout.h, `seq_layers.FUSED_ATTN_DROPOUT`), in one process on one box:

  core    the core launch with dropout (`asac_attention_mh_dropout_forward / _backward`) against the same launch at p = 0
          (`asac_attention_mh_forward / _backward`): HIP events around launches issued back to back by the library's repeat
          knob, us per launch.  The difference is what the draws and the counter's arrival cost.
  block   forward + backward of one `EpisodeMultiheadAttentionBlock(E, H, dropout=p, gate=RESIDUAL)` in training mode with
          the switch on against the switch off (the baddbmm / softmax / F.dropout / bmm / mean module code: the path of the
          commit before the dropout launch), eager: HIP events around `reps` passes, ms per pass, and the launches of a pass
  step    train steps/s of `SAC_Base` at the sizes of bench.py's cfg_attn_h64 over tests/plugins/nn_attn_dropout.py
          (captured step) with the switch on and off

    python tools/attn_dropout_bench.py [--p 0.005] [--reps 100] [--steps 400] [--modes core block step] [--dense]

--dense measures the OTHER switch, `seq_layers.FUSED_DENSE_DROPOUT` (the live nn.Dropout modules of the dense q / k / v stacks
and of the output block inside the row launches, csrc/rows_proj.hip), with the weights' switch left on: `block` builds the
block with `qkv_dense_depth=1, out_dense_depth=1` (off: the stacks module by module with ATen's dropout — the path of the commit
before those launches; at E = 12 the row kernels do not apply and both ways run the same code), `step` also records which
replay path each learner took (`direct`: the captured step drew no torch random numbers and left torch's replay).

The two ways alternate (off, on, off, on, ...: a drift of the box's clocks hits both); the median of the rounds is reported,
all rounds are listed.  Launches per pass are taken with torch's profiler outside the timing.  One JSON line per shape and
mode."""
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
SHAPES = [(B, Lq, Lk, E, H) for B in (256, 1024) for (Lq, Lk) in ((9, 9), (9, 18)) for (E, H) in ((12, 2), (64, 8))]


def median(xs):
    return sorted(xs)[len(xs) // 2]


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


def events_ms(fn, reps):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def core_row(shape, p, repeat=100):
    from asac_amd import native
    B, Lq, Lk, E, H = shape
    gen = torch.Generator(device='cuda').manual_seed(0)
    q, k, v = (torch.randn(B, L, E, device='cuda', generator=gen) for L in (Lq, Lk, Lk))
    mask = torch.rand(B, Lq, Lk, device='cuda', generator=gen) < 0.3
    g_out, g_w = torch.randn(B, Lq, E, device='cuda', generator=gen), torch.randn(B, Lq, Lk, device='cuda', generator=gen)
    out, w, keep = torch.empty_like(q), torch.empty(B, Lq, Lk, device='cuda'), torch.empty(B, Lq, device='cuda')
    p_heads = torch.empty(B, H, Lq, Lk, device='cuda')
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    state = torch.zeros(native.ATTN_DROPOUT_STATE_WORDS, dtype=torch.int64, device='cuda')
    used = torch.zeros(1, dtype=torch.int64, device='cuda')

    def plain():
        native.attention_mh_forward(q, k, v, mask, H, out, w, keep, p_heads)
        native.attention_mh_backward(q, k, v, mask, H, p_heads, g_out, g_w, gq, gk, gv)

    def drop():
        native.attention_mh_dropout_forward(q, k, v, mask, H, out, w, keep, p_heads, None, None, p, 1234, 1, state, used)
        native.attention_mh_dropout_backward(q, k, v, mask, H, p_heads, g_out, g_w, gq, gk, gv, p, 1234, 1, used)

    runs = {n: [] for n in ('fwd_plain', 'bwd_plain', 'fwd_drop', 'bwd_drop')}
    for _ in range(ROUNDS):
        for fn, tag in ((plain, 'plain'), (drop, 'drop')):
            with native.LaunchProfiler(repeat=repeat) as prof:      # (every launch issued `repeat` times back to back)
                for _ in range(3):
                    fn()
            seen = prof.summary()
            for name, rec in seen.items():
                runs[('fwd_' if name.endswith('forward') else 'bwd_') + tag].append(round(rec['min_us'], 3))
    row = {'mode': 'core', 'shape': list(shape), 'p': p}
    for n, xs in runs.items():
        row['us_' + n] = median(xs)
    row['fwd_extra_us'] = round(row['us_fwd_drop'] - row['us_fwd_plain'], 3)
    row['bwd_extra_us'] = round(row['us_bwd_drop'] - row['us_bwd_plain'], 3)
    row['single_word_arrival_us'] = round(B * 0.030, 2)      # what B arrivals at ONE word would take (csrc/image.hip: 30 ns each)
    row['runs'] = runs
    assert int(torch.count_nonzero(state[1:]).item()) == 0, 'arrival words end every launch zero'
    return row


def block_row(shape, p, reps, dense=False):
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import seq_layers
    from asac_amd import native
    B, Lq, Lk, E, H = shape
    switch = 'FUSED_DENSE_DROPOUT' if dense else 'FUSED_ATTN_DROPOUT'
    torch.manual_seed(0)
    block = seq_layers.EpisodeMultiheadAttentionBlock(E, H, dropout=p, gate=m.GATE.RESIDUAL,
                                                      **(dict(qkv_dense_depth=1, out_dense_depth=1) if dense else {})).cuda()
    assert block.training
    key = torch.randn(B, Lk, E, device='cuda')
    pad = torch.arange(Lk, device='cuda').unsqueeze(0) < torch.randint(0, 3, (B, 1), device='cuda')

    def fn():
        for p_ in block.parameters():
            p_.grad = None
        kk = key.clone().requires_grad_(True)
        o, w = block(kk, seq_q_len=Lq, key_padding_mask=pad)
        (o.sum() + w.sum()).backward()

    row = {'mode': 'block', 'switch': switch, 'shape': list(shape), 'p': p}
    if dense:
        row['same_path'] = not native.rows_proj_supported(E)
    runs = {False: [], True: []}
    for rnd in range(ROUNDS):
        for fused in (False, True):
            setattr(seq_layers, switch, fused)
            runs[fused].append(round(events_ms(fn, reps), 4))
            if rnd == 0:
                tag = 'fused' if fused else 'module'
                launches, busy = count_launches(fn)
                row['launches_' + tag], row['device_us_' + tag] = round(launches, 1), round(busy, 1)
    setattr(seq_layers, switch, True)
    row.update(ms_module=median(runs[False]), ms_fused=median(runs[True]), runs_module=runs[False], runs_fused=runs[True])
    row['fused_over_module'] = round(row['ms_fused'] / row['ms_module'], 4)
    return row


def step_row(steps, dense=False):
    import bench
    from algorithm.nn_models.layers import seq_layers
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    from tests import parity_utils as pu
    cfg = bench.CONFIGS['cfg_attn_h64']
    plugin = pu.plugin('nn_attn_dropout')
    switch = 'FUSED_DENSE_DROPOUT' if dense else 'FUSED_ATTN_DROPOUT'
    agents = {}
    for fused in (False, True):      # (the switch is read at every forward: each learner captures its step under its own setting)
        setattr(seq_layers, switch, fused)
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
    setattr(seq_layers, switch, True)
    runs = {False: [], True: []}
    for _ in range(3):
        for fused in (False, True):
            agent = agents[fused]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                agent.train()
            torch.cuda.synchronize()
            runs[fused].append(round(steps / (time.perf_counter() - t0), 1))
    replay = {fused: 'direct' if agents[fused]._graph.exec_handle is not None else 'torch' for fused in (False, True)}
    for agent in agents.values():
        agent.close()
    row = {'mode': 'step', 'switch': switch, 'replay_module': replay[False], 'replay_fused': replay[True], 'plugin': 'nn_attn_dropout', 'batch': cfg['batch_size'], 'steps': steps,
           'steps_per_s_module': median(runs[False]), 'steps_per_s_fused': median(runs[True]),
           'runs_module': runs[False], 'runs_fused': runs[True]}
    row['fused_over_module'] = round(row['steps_per_s_fused'] / row['steps_per_s_module'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--p', type=float, default=0.005)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--modes', nargs='+', default=['core', 'block', 'step'])
    ap.add_argument('--dense', action='store_true', help='measure FUSED_DENSE_DROPOUT (block, step) instead')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: nothing is measured without one'
    import asac_amd  # noqa: F401
    for mode in args.modes:
        if mode == 'step':
            print(json.dumps(step_row(args.steps, args.dense)), flush=True)
            continue
        for shape in SHAPES:
            row = core_row(shape, args.p) if mode == 'core' else block_row(shape, args.p, args.reps, args.dense)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
