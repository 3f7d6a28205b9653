"""Mint the DQN-like fixtures from the *reference* implementation (`d_action_sizes` set, `c_action_size == 0`,
`discrete_dqn_like=True`: critics only, double-DQN target, epsilon-greedy acting).

Run where the reference tree is importable (see `make_golden.py`):   python tests/golden/make_dqn_golden.py
It calls `make_golden.f6_step` as it stands and writes, next to this file,
  f6_step_dqn.npz       branches (3, 2), ensemble 3 of 2 sampled, n_step 3
  f6_step_dqn_one.npz   branch (4,), n_step 4
  f6_step_dqn_rnn.npz   branches (3, 2), GRU representation, burn_in_step 3, n_step 3
  f16_dqn_y.npz         the reference's `get_dqn_like_d_y` on random tables (inputs, the two subsets, y)
Sizes and plugins as in `make_discrete_golden.py`.

A greedy index that flips between the reference's CPU values and the device's is no kernel error, so every step case must
keep a margin: at the positions the target picks, the gap between the two largest eval values of any branch is at least
`MIN_GAP` of the heads' largest magnitude (the largest |value| of the whole eval table handed to the call, not only of the
picked positions: the stricter reading).  The reference's `get_dqn_like_d_y` is wrapped to measure that; the wrapper sees
both calls of a step, the Q step's target and the TD error's (the latter on the updated critics), and keeps the smallest
margin of all of them, stored as `meta/min_gap`.  The same wrapper asserts the cases' coverage: every L in [0, n) occurs, a
`done` at L occurs, and no row is wholly masked.  A case that misses either gets another seed, not another condition.

`CASES` is what the tests read (tests/test_dqn_host.py, tests/test_dqn_gpu.py): case -> (plugin under tests/plugins,
learner keywords, discrete action sizes).
"""
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent

SMALL = dict(batch_size=16, capacity=256)
CASES = {
    'dqn': ('nn_vec_d32', dict(n_step=3, ensemble_q_num=3, ensemble_q_sample=2, discrete_dqn_like=True), (3, 2)),
    'dqn_one': ('nn_vec', dict(n_step=4, discrete_dqn_like=True), (4,)),
    'dqn_rnn': ('nn_rnn_d32', dict(n_step=3, burn_in_step=3, seq_encoder='RNN', discrete_dqn_like=True), (3, 2)),
}
SEEDS = {'dqn': 6, 'dqn_one': 7, 'dqn_rnn': 6}       # (dqn_one: seed 6 never picks L = 2)
PLUGINS = HERE.parent / 'plugins'
EPISODES = [40, 30, 50, 12]
N_STEPS = 3
MIN_GAP = 1e-5
# (B, n, sizes, E, E_sample) of the function fixture
Y_SHAPES = [(5, 3, (3, 2), 3, 2), (4, 1, (4,), 1, 1), (6, 4, (2, 3, 2), 2, 2)]


def _last_false(gone):
    """[B, n] bool -> L [B]: the last False of each row, n - 1 where there is none"""
    n = gone.shape[1]
    idx = np.where(~gone, np.arange(n)[None, :], -1).max(axis=1)
    return np.where(idx < 0, n - 1, idx)


def _measure(seen, sizes, last, pad, done, eval_next):
    """what one call of the reference's `get_dqn_like_d_y` picked: relative argmax margin, the L values, done at L"""
    gone = (last | pad).numpy()
    L = _last_false(gone)
    rows = np.arange(len(L))
    picked = eval_next.numpy()[:, rows, L]                  # [Es, B, D]
    scale = float(np.abs(eval_next.numpy()).max())
    j0 = 0
    for s in sizes:
        if s > 1:
            top = np.sort(picked[..., j0:j0 + s], axis=-1)
            seen['gap'] = min(seen['gap'], float((top[..., -1] - top[..., -2]).min()) / scale)
        j0 += s
    seen['L'].update(int(v) for v in L)
    seen['done_at_L'] += int(done.numpy()[rows, L].sum())
    seen['masked_rows'] += int(gone.all(axis=1).sum())


def mint_steps(mg):
    from algorithm.utils.enums import convert_config_to_enum
    ref_y = mg.SAC_Base.get_dqn_like_d_y
    for case, (plugin, kw, d_sizes) in CASES.items():
        kw = dict(kw)
        convert_config_to_enum(kw)
        seen = dict(gap=float('inf'), L=set(), done_at_L=0, masked_rows=0)

        def wrapped(self, n_last_masks, n_padding_masks, n_rewards, n_dones, stacked_next_n_d_qs,
                    stacked_next_target_n_d_qs, _seen=seen, _sizes=d_sizes):
            _measure(_seen, _sizes, n_last_masks, n_padding_masks, n_dones, stacked_next_n_d_qs)
            return ref_y(self, n_last_masks, n_padding_masks, n_rewards, n_dones, stacked_next_n_d_qs,
                         stacked_next_target_n_d_qs)

        mg.SAC_Base.get_dqn_like_d_y = wrapped
        try:
            mg.f6_step(case, str(PLUGINS / f'{plugin}.py'),
                       dict(batch_size=SMALL['batch_size'], replay_config={'capacity': SMALL['capacity']}, **kw),
                       EPISODES, N_STEPS, d_action_sizes=d_sizes, c_action_size=0, seed=SEEDS[case])
        finally:
            mg.SAC_Base.get_dqn_like_d_y = ref_y
        assert seen['gap'] >= MIN_GAP, (case, seen['gap'], 'change this case\'s seed')
        assert seen['L'] == set(range(kw['n_step'])) and seen['done_at_L'] > 0 and seen['masked_rows'] == 0, \
            (case, seen, 'change this case\'s seed')
        path = HERE / f'f6_step_{case}.npz'
        out = dict(np.load(path))
        out['meta/min_gap'] = np.float64(seen['gap'])
        np.savez_compressed(path, **out)
        print(case, path.stat().st_size, 'bytes, min gap', seen['gap'], 'L', sorted(seen['L']), 'done at L',
              seen['done_at_L'], 'wholly masked rows', seen['masked_rows'])


def mint_function(mg):
    """`get_dqn_like_d_y` on random tables: full member tables and the two subsets in the file, the subsets applied
    before the call.  Row 0 wholly masked, row 1 `done` at L, row 2 L = 0, row 3 an exact tie in its first branch."""
    import torch
    out = {'n_cases': np.int64(len(Y_SHAPES))}
    gamma = 0.97
    for c, (B, n, sizes, E, Es) in enumerate(Y_SHAPES):
        gen = torch.Generator().manual_seed(160 + c)
        D = sum(sizes)
        ev = torch.randn(E, B, n, D, generator=gen)
        tg = torch.randn(E, B, n + 1, D, generator=gen)
        reward = torch.randn(B, n, generator=gen)
        done, last, pad = (m.clone() for m in torch.rand(3, B, n, generator=gen) < 0.25)
        pad[0] = True
        last[1], pad[1] = False, False
        done[1, n - 1] = True                                 # row 1: L = n - 1, done there
        last[2], pad[2] = False, False
        pad[2, 1:] = True                                     # row 2: L = 0
        done[2] = False
        last[3], pad[3] = False, False                        # row 3: L = n - 1, tie at L in the first branch
        sub_n = torch.randperm(E, generator=gen)[:Es]
        sub_next = torch.randperm(E, generator=gen)[:Es]
        ev[sub_n[0], 3, n - 1, :sizes[0]] = 0.75              # all of the branch equal: the lowest index wins
        stub = types.SimpleNamespace(device='cpu', d_action_sizes=list(sizes), d_action_branch_size=len(sizes),
                                     gamma=gamma, _gamma_ratio=torch.logspace(0, n - 1, n, gamma))
        y = mg.SAC_Base.get_dqn_like_d_y(stub, last, pad, reward, done, ev.index_select(0, sub_n),
                                         tg[:, :, 1:].index_select(0, sub_next))
        for k, v in dict(eval=ev, target=tg, reward=reward, done=done, last=last, pad=pad, sub_n=sub_n.to(torch.int32),
                         sub_next=sub_next.to(torch.int32), y=y).items():
            out[f'c{c}/{k}'] = v.numpy()
        out[f'c{c}/sizes'] = np.asarray(sizes, dtype=np.int64)
        out[f'c{c}/gamma'] = np.float64(gamma)
    out['torch_version'] = np.array(torch.__version__)
    np.savez_compressed(HERE / 'f16_dqn_y.npz', **out)
    print('f16_dqn_y', (HERE / 'f16_dqn_y.npz').stat().st_size, 'bytes')


def main():
    sys.path.insert(0, str(HERE))
    import torch
    import make_golden as mg
    torch.set_num_threads(1)
    mint_function(mg)
    mint_steps(mg)


if __name__ == '__main__':
    main()
