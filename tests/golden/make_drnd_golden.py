"""Mint the fixtures of random network distillation for a pure-discrete, policy-based learner from the *reference*
implementation (`use_rnd=True`, `d_action_sizes` set, `c_action_size=0`, `discrete_dqn_like=False`: `_train_rnd` distils the
members of `ModelRND.d_dense_list` the stored one-hot actions select, `rnd_sample_d_action` picks the most novel of
`rnd_n_sample` sampled actions).

Run where the reference tree is importable (see `make_golden.py`):   python tests/golden/make_drnd_golden.py
It calls `make_golden.f6_step` as it stands and writes, next to this file,
  f6_step_rnd_d.npz       nn_vec_full, d_action_sizes (3,), n_step 3
  f6_step_rnd_d2.npz      nn_vec_full, d_action_sizes (3, 2), n_step 3
  f6_step_rnd_d_rnn.npz   nn_rnn_rnd (nn_rnn + the stock ModelRND), (4,), GRU representation, burn_in_step 3, n_step 3
  f18_drnd_pick.npz       the reference's own `rnd_sample_d_action` on a stub learner (two reference `ModelRND`s) and a stub
                          policy whose `.sample((k,))` returns recorded one-hot candidates: both state dicts, state, logits,
                          the candidates' indices, the per-candidate errors, the chosen index and the action
The step cases: batch 16, capacity 256, three steps.

An argmax that flips between the reference's CPU values and the device's is no kernel error, so every pick case must keep
a margin: for every row, the gap between the largest error and the largest error of a candidate with ANOTHER action is at
least `MIN_GAP` of the row's largest error (identical candidates tie exactly, and the first wins on both sides).  A case that
misses it gets another seed, not another condition.  The test rebuilds the uniforms from the recorded candidates as the
midpoints of their CDF intervals (float64, from the recorded logits): every such interval must be wider than `MIN_WIDTH`,
so float32 rounding of the running sum cannot move a candidate.  Both margins found are stored under `meta/`.

`CASES` / `PICK_SHAPES` are what the tests read (tests/test_drnd_host.py, tests/test_drnd_gpu.py).
"""
import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent

SMALL = dict(batch_size=16, capacity=256)
# case -> (plugin, d_action_sizes, learner keywords)
CASES = {
    'rnd_d': ('nn_vec_full', (3,), dict(n_step=3, use_rnd=True)),
    # (two branches double every head: one critic and one-block policy heads keep the file under the size limit; the RND
    # models, which this fixture is about, are the stock ones)
    'rnd_d2': ('nn_vec_full', (3, 2), dict(n_step=3, use_rnd=True, ensemble_q_num=1, ensemble_q_sample=1,
                                           nn_config={'policy': {'d_dense_depth': 1}})),
    'rnd_d_rnn': ('nn_rnn_rnd', (4,), dict(n_step=3, burn_in_step=3, seq_encoder='RNN', use_rnd=True,
                                           nn_config={'policy': {'d_dense_depth': 1}})),       # (the size limit again)
}
PLUGINS = HERE.parent / 'plugins'
EPISODES = [40, 30, 50, 12]
N_STEPS = 3
MIN_GAP = 1e-5
MIN_WIDTH = 1e-3
# (batch, k, S, sizes) of the function fixture, and the seed each case keeps its margins with
PICK_SHAPES = [(5, 10, 6, (3,)), (4, 1, 6, (3,)), (7, 50, 64, (3, 2))]
PICK_SEEDS = [180, 181, 182]


class Fixture:
    """an npz whose arrays that repeat another array bit for bit are stored once (`aliases`: a JSON map key -> the key that
    holds the bits): `files` and `[key]` as `numpy.load` gives them for the file `make_golden.f6_step` wrote"""

    def __init__(self, path):
        self._g = np.load(path)
        self._alias = json.loads(str(self._g['aliases'])) if 'aliases' in self._g.files else {}
        self.files = [k for k in self._g.files if k != 'aliases'] + list(self._alias)

    def __getitem__(self, key):
        return self._g[self._alias.get(key, key)]

    def __contains__(self, key):
        return key in self.files


def store_repeats_once(path):
    """rewrite the npz at `path` without the arrays that repeat an earlier one of at least 1 KiB bit for bit (the target
    critics at w0 = the critics, the frozen RND target and `s_dense` at w1 = at w0): lossless, see `Fixture`"""
    with np.load(path) as lazy:
        g = {k: lazy[k] for k in lazy.files}
    seen, keep, alias = {}, {}, {}
    for k, a in g.items():
        sig = (a.dtype.str, a.shape, a.tobytes()) if a.nbytes >= 1024 else None
        if sig is not None and sig in seen:
            alias[k] = seen[sig]
            continue
        if sig is not None:
            seen[sig] = k
        keep[k] = a
    keep['aliases'] = np.array(json.dumps(alias))
    np.savez_compressed(path, **keep)
    back = Fixture(path)
    assert sorted(back.files) == sorted(g) and all(np.array_equal(back[k], a) for k, a in g.items())
    return alias


def mint_steps(mg):
    from algorithm.utils.enums import convert_config_to_enum
    for case, (plugin, sizes, kw) in CASES.items():
        kw = dict(kw)
        convert_config_to_enum(kw)
        mg.f6_step(case, str(PLUGINS / f'{plugin}.py'),
                   dict(batch_size=SMALL['batch_size'], replay_config={'capacity': SMALL['capacity']}, **kw),
                   EPISODES, N_STEPS, d_action_sizes=sizes, c_action_size=0)
        path = HERE / f'f6_step_{case}.npz'
        alias = store_repeats_once(path)
        assert any(k.startswith('w1/model_target_rnd/') for k in alias), 'the target stays frozen'
        keys = Fixture(path).files
        assert any(k.startswith('g0/optimizer_rnd/') for k in keys) and any(k.startswith('w1/model_rnd/d_dense_list.') for k in keys), case
        assert path.stat().st_size < 1_000_000, (case, path.stat().st_size)
        print(case, path.stat().st_size, 'bytes')


def mint_pick(mg):
    import torch
    from algorithm.nn_models.exploration import ModelRND
    out = {'n_cases': np.int64(len(PICK_SHAPES))}
    worst_gap, worst_width = float('inf'), float('inf')
    for c, ((batch, k, S, sizes), seed) in enumerate(zip(PICK_SHAPES, PICK_SEEDS)):
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        D, K = sum(sizes), len(sizes)
        rnd, target = ModelRND(S, D, 0), ModelRND(S, D, 0)
        for m in (rnd, target):          # the stock initialisation leaves the biases zero: give them values
            for name, p in m.named_parameters():
                if name.endswith('bias'):
                    p.data.copy_(0.1 * torch.randn(p.shape, generator=gen))
        state = torch.randn(batch, S, generator=gen)
        logits = torch.randn(batch, D, generator=gen)
        parts = logits.split(list(sizes), dim=-1)
        cand = torch.stack([torch.multinomial(torch.softmax(p.double(), -1), k, replacement=True, generator=gen) for p in parts], -1)
        acts = torch.cat([torch.nn.functional.one_hot(cand[..., j], s) for j, s in enumerate(sizes)], -1).float()   # [batch, k, D]
        seen = {}

        def spy(model, key):
            orig = model.cal_d_rnd

            def cal(states):
                r = orig(states)
                seen[key] = r.detach().clone()
                return r
            model.cal_d_rnd = cal

        spy(rnd, 'p')
        spy(target, 't')

        def sample(shape, _acts=acts, _k=k):
            assert tuple(shape) == (_k,)
            return _acts.transpose(0, 1)       # [k, batch, D]

        stub = types.SimpleNamespace(rnd_n_sample=k, model_rnd=rnd, model_target_rnd=target)
        action = mg.SAC_Base.rnd_sample_d_action(stub, state, types.SimpleNamespace(sample=sample))
        sel = acts.unsqueeze(-1)
        diff = (sel * seen['p'].unsqueeze(1)).sum(-2) - (sel * seen['t'].unsqueeze(1)).sum(-2)
        err = torch.sum(torch.pow(diff, 2), dim=-1)                                       # [batch, k]
        index = torch.argmax(err, dim=1)
        assert torch.equal(action, acts[torch.arange(batch), index])
        for b in range(batch):            # the margin over candidates with another action
            other = [float(err[b, j]) for j in range(k) if not torch.equal(cand[b, j], cand[b, index[b]])]
            if other:
                gap = (float(err[b, index[b]]) - max(other)) / float(err[b, index[b]])
                assert gap >= MIN_GAP, (c, b, gap, 'change this case\'s seed')
                worst_gap = min(worst_gap, gap)
        for j, p in enumerate(parts):     # the CDF interval of every recorded candidate
            edges = torch.cat([torch.zeros(batch, 1, dtype=torch.float64), torch.cumsum(torch.softmax(p.double(), -1), -1)], -1)
            width = (edges.gather(1, cand[..., j] + 1) - edges.gather(1, cand[..., j])).min().item()
            assert width > MIN_WIDTH, (c, j, width, 'change this case\'s seed')
            worst_width = min(worst_width, width)
        for name, m in (('rnd', rnd), ('target', target)):
            for kk, v in m.state_dict().items():
                out[f'c{c}/{name}/{kk}'] = v.numpy().copy()
        for kk, v in dict(state=state, logits=logits, cand=cand.to(torch.int64), err=err, index=index.to(torch.int64),
                          action=action).items():
            out[f'c{c}/{kk}'] = v.numpy()
        out[f'c{c}/shape'] = np.asarray((batch, k, S), dtype=np.int64)
        out[f'c{c}/sizes'] = np.asarray(sizes, dtype=np.int64)
    out['meta/min_gap'] = np.float64(worst_gap)
    out['meta/min_width'] = np.float64(worst_width)
    out['torch_version'] = np.array(torch.__version__)
    np.savez_compressed(HERE / 'f18_drnd_pick.npz', **out)
    size = (HERE / 'f18_drnd_pick.npz').stat().st_size
    assert size < 1_000_000, size
    print('f18_drnd_pick', size, 'bytes, min gap', worst_gap, 'min width', worst_width)


def main():
    sys.path.insert(0, str(HERE))
    import torch
    import make_golden as mg
    torch.set_num_threads(1)
    mint_pick(mg)
    mint_steps(mg)


if __name__ == '__main__':
    main()
