"""Mint the pure-discrete step fixtures from the *reference* implementation (policy-based discrete branch of
`SAC_Base`: `d_action_sizes` set, `c_action_size == 0`, `discrete_dqn_like=False`).

Run where the reference tree is importable (see `make_golden.py`):   python tests/golden/make_discrete_golden.py
It calls `make_golden.f6_step` as it stands and writes, next to this file,
  f6_step_discrete.npz      branches (3, 2), ensemble 3 of 2 sampled, n_step 3
  f6_step_discrete_is.npz   branch (4,), use_n_step_is, n_step 4
  f6_step_discrete_rnn.npz  branches (3, 2), GRU representation, burn_in_step 3, n_step 3
Batch 16 over a ring of 256 rows and, for the two-branch cases, the 32-wide discrete heads of tests/plugins/nn_vec_d32.py
/ nn_rnn_d32.py (plugin API only, so they load under the reference) keep every file under the repository's 1 MiB limit:
weights before / after, the first step's gradients and the per-step snapshots of the ring are what such a fixture holds.

`CASES` is what the tests read (tests/test_discrete_host.py, tests/test_discrete_gpu.py): case -> (plugin under
tests/plugins, learner keywords, discrete action sizes).
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent

SMALL = dict(batch_size=16, capacity=256)
CASES = {
    'discrete': ('nn_vec_d32', dict(n_step=3, ensemble_q_num=3, ensemble_q_sample=2), (3, 2)),
    'discrete_is': ('nn_vec', dict(n_step=4, use_n_step_is=True), (4,)),
    'discrete_rnn': ('nn_rnn_d32', dict(n_step=3, burn_in_step=3, seq_encoder='RNN'), (3, 2)),
}
PLUGINS = HERE.parent / 'plugins'
EPISODES = [40, 30, 50, 12]
N_STEPS = 3


def main():
    sys.path.insert(0, str(HERE))
    import torch
    import make_golden as mg
    from algorithm.utils.enums import convert_config_to_enum
    torch.set_num_threads(1)
    for case, (plugin, kw, d_sizes) in CASES.items():
        kw = dict(kw)
        convert_config_to_enum(kw)
        mg.f6_step(case, str(PLUGINS / f'{plugin}.py'),
                   dict(batch_size=SMALL['batch_size'], replay_config={'capacity': SMALL['capacity']}, **kw),
                   EPISODES, N_STEPS, d_action_sizes=d_sizes, c_action_size=0)
        print(case, (HERE / f'f6_step_{case}.npz').stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
