"""Mint `f16_gates.npz` from the *reference* implementation: its `EpisodeMultiheadAttentionBlock(32, 2 heads, gate=g)` for
g in RESIDUAL / OUTPUT / RECURRENT on a [3, 5, 32] window batch, query lengths 2 and 5, with a padding mask that pads query
rows and a `key_index` — inputs, `state_dict`, output, attention weights and the gradients of a fixed cotangent with respect
to the input and every parameter.

Run in the BUILD CONTAINER ONLY, like make_golden.py (it imports the reference checkout behind `ref_shims`):
    python tests/golden/make_gate_golden.py
The fixture is data only; no reference source is copied.
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import ref_shims  # noqa: E402

ref_shims.install()

GATES = ('RESIDUAL', 'OUTPUT', 'RECURRENT')
B, K, E, HEADS = 3, 5, 32, 2
Q_LENS = (2, 5)


def main():
    from algorithm.nn_models.layers.seq_layers import GATE, EpisodeMultiheadAttentionBlock
    rng = np.random.default_rng(16)
    out = {}
    key = rng.standard_normal((B, K, E)).astype(np.float32)
    index = np.stack([np.arange(s, s + K) for s in rng.integers(0, 20, B)]).astype(np.int32)
    pad = np.zeros((B, K), dtype=bool)
    pad[0, :2] = True           # the oldest positions (a query row when the query is the whole window)
    pad[1, -2:] = True          # the newest positions: both rows of the cut query
    out['key'], out['index'], out['pad'] = key, index, pad
    for name in GATES:
        torch.manual_seed(160)
        block = EpisodeMultiheadAttentionBlock(E, HEADS, gate=GATE[name])
        for k_, v in block.state_dict().items():
            out[f'{name}/w/{k_}'] = v.detach().numpy().copy()
        for q in Q_LENS:
            x = torch.from_numpy(key).requires_grad_(True)
            y, w = block(x, q, key_index=torch.from_numpy(index), key_padding_mask=torch.from_numpy(pad))
            cy = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
            cw = torch.from_numpy(rng.standard_normal(tuple(w.shape)).astype(np.float32))
            names, params = zip(*block.named_parameters())
            grads = torch.autograd.grad((y * cy).sum() + (w * cw).sum(), (x, *params))
            pre = f'{name}/q{q}/'
            out[pre + 'y'], out[pre + 'w'] = y.detach().numpy(), w.detach().numpy()
            out[pre + 'cy'], out[pre + 'cw'] = cy.numpy(), cw.numpy()
            out[pre + 'g/key'] = grads[0].numpy()
            for n_, g in zip(names, grads[1:]):
                out[pre + 'g/' + n_] = g.numpy()
    path = HERE / 'f16_gates.npz'
    np.savez_compressed(path, **out)
    # (float32 parameters and their gradients do not compress: 3 gates x 2 query lengths come to ~0.3 MB)
    assert path.stat().st_size < 1_000_000, (path.name, path.stat().st_size)
    print(path.name, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
