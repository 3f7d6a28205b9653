"""Mint the random-network-distillation fixtures from the *reference* implementation (`use_rnd=True`, continuous actions
only: `_train_rnd` distils `ModelRND.c_dense`, `rnd_sample_c_action` picks the most novel of `rnd_n_sample` candidates).

Run where the reference tree is importable (see `make_golden.py`):   python tests/golden/make_rnd_golden.py
It calls `make_golden.f6_step` as it stands and writes, next to this file,
  f6_step_rnd_c.npz       nn_vec_full, n_step 3
  f6_step_rnd_c_rnn.npz   nn_rnn_rnd (nn_rnn + the stock ModelRND), GRU representation, burn_in_step 3, n_step 3
  f17_rnd_pick.npz        the reference's own `rnd_sample_c_action` on a stub learner (two reference `ModelRND`s) and a stub
                          policy whose `.sample((k,))` is `loc + scale * eps` for recorded eps: both state dicts, state, loc,
                          scale, eps, the per-candidate errors, the chosen index and the action
Both step cases: batch 16, capacity 256, three steps, `d_action_sizes=()`, `c_action_size=2`.

An argmax that flips between the reference's CPU values and the device's is no kernel error, so every pick case must keep
a margin: for every row, the gap between the two largest errors is at least `MIN_GAP` of the row's largest error.  A case
that misses it gets another seed, not another condition.  The margin found is stored as `meta/min_gap`.

`CASES` / `PICK_SHAPES` are what the tests read (tests/test_rnd_host.py, tests/test_rnd_gpu.py).
"""
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent

SMALL = dict(batch_size=16, capacity=256)
CASES = {
    'rnd_c': ('nn_vec_full', dict(n_step=3, use_rnd=True)),
    'rnd_c_rnn': ('nn_rnn_rnd', dict(n_step=3, burn_in_step=3, seq_encoder='RNN', use_rnd=True)),
}
PLUGINS = HERE.parent / 'plugins'
EPISODES = [40, 30, 50, 12]
N_STEPS = 3
MIN_GAP = 1e-5
# (batch, k, S, A) of the function fixture, and the seed each case keeps its margin with
PICK_SHAPES = [(5, 10, 6, 2), (4, 1, 6, 2), (7, 50, 61, 3)]
PICK_SEEDS = [170, 171, 172]


def mint_steps(mg):
    from algorithm.utils.enums import convert_config_to_enum
    for case, (plugin, kw) in CASES.items():
        kw = dict(kw)
        convert_config_to_enum(kw)
        mg.f6_step(case, str(PLUGINS / f'{plugin}.py'),
                   dict(batch_size=SMALL['batch_size'], replay_config={'capacity': SMALL['capacity']}, **kw),
                   EPISODES, N_STEPS, d_action_sizes=(), c_action_size=2)
        path = HERE / f'f6_step_{case}.npz'
        keys = np.load(path).files
        assert any(k.startswith('g0/optimizer_rnd/') for k in keys) and any(k.startswith('w1/model_rnd/') for k in keys), case
        print(case, path.stat().st_size, 'bytes')


def mint_pick(mg):
    import torch
    from algorithm.nn_models.exploration import ModelRND
    out = {'n_cases': np.int64(len(PICK_SHAPES))}
    worst = float('inf')
    for c, ((batch, k, S, A), seed) in enumerate(zip(PICK_SHAPES, PICK_SEEDS)):
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        rnd, target = ModelRND(S, 0, A), ModelRND(S, 0, A)
        for m in (rnd, target):          # the stock initialisation leaves the biases zero: give them values
            for name, p in m.named_parameters():
                if name.endswith('bias'):
                    p.data.copy_(0.1 * torch.randn(p.shape, generator=gen))
        state = torch.randn(batch, S, generator=gen)
        loc = 0.5 * torch.randn(batch, A, generator=gen)
        scale = 0.2 + torch.rand(batch, A, generator=gen)
        eps = torch.randn(batch, k, A, generator=gen)
        seen = {}

        def spy(model, key):
            orig = model.cal_c_rnd

            def cal(states, actions):
                r = orig(states, actions)
                seen[key] = r.detach().clone()
                return r
            model.cal_c_rnd = cal

        spy(rnd, 'p')
        spy(target, 't')

        def sample(shape, _loc=loc, _scale=scale, _eps=eps, _k=k):
            assert tuple(shape) == (_k,)
            return (_loc.unsqueeze(1) + _scale.unsqueeze(1) * _eps).transpose(0, 1)       # [k, batch, A]

        stub = types.SimpleNamespace(rnd_n_sample=k, model_rnd=rnd, model_target_rnd=target)
        action = mg.SAC_Base.rnd_sample_c_action(stub, state, types.SimpleNamespace(sample=sample))
        err = torch.sum(torch.pow(seen['p'] - seen['t'], 2), dim=-1)                       # [batch, k]
        index = torch.argmax(err, dim=1)
        cand = torch.tanh(loc.unsqueeze(1) + scale.unsqueeze(1) * eps)
        assert torch.equal(action, cand[torch.arange(batch), index])
        if k > 1:
            top = torch.sort(err, dim=1).values
            gap = float(((top[:, -1] - top[:, -2]) / top[:, -1]).min())
            assert gap >= MIN_GAP, (c, gap, 'change this case\'s seed')
            worst = min(worst, gap)
        for name, m in (('rnd', rnd), ('target', target)):
            for kk, v in m.state_dict().items():
                out[f'c{c}/{name}/{kk}'] = v.numpy().copy()
        for kk, v in dict(state=state, loc=loc, scale=scale, eps=eps, err=err, index=index.to(torch.int64),
                          action=action).items():
            out[f'c{c}/{kk}'] = v.numpy()
        out[f'c{c}/shape'] = np.asarray((batch, k, S, A), dtype=np.int64)
    out['meta/min_gap'] = np.float64(worst)
    out['torch_version'] = np.array(torch.__version__)
    np.savez_compressed(HERE / 'f17_rnd_pick.npz', **out)
    print('f17_rnd_pick', (HERE / 'f17_rnd_pick.npz').stat().st_size, 'bytes, min gap', worst)


def main():
    sys.path.insert(0, str(HERE))
    import torch
    import make_golden as mg
    torch.set_num_threads(1)
    mint_pick(mg)
    mint_steps(mg)


if __name__ == '__main__':
    main()
