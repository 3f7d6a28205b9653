"""CPU: a gated `EpisodeMultiheadAttentionBlock` reproduces the reference's recorded values (golden `f16_gates.npz`:
reference `state_dict` + inputs -> output, attention weights and the gradients of a fixed cotangent, for the RESIDUAL /
OUTPUT / RECURRENT gates with a cut and an uncut query and padded query rows).  This pins the gate layers' module path —
what the one-launch gate (csrc/rows_gate.hip, tests/test_fused_gate_gpu.py) is measured against."""
import numpy as np
import pytest
import torch

from algorithm.nn_models.layers.seq_layers import GATE, EpisodeMultiheadAttentionBlock

GATES = ('RESIDUAL', 'OUTPUT', 'RECURRENT')
Q_LENS = (2, 5)
TOL = dict(rtol=1e-5, atol=5e-6)      # (host BLAS differs by a few 1e-6 between CPUs: the bound of test_attention_golden.py)


def load_block(g, name, width=32, heads=2):
    block = EpisodeMultiheadAttentionBlock(width, heads, gate=GATE[name])
    prefix = f'{name}/w/'
    state = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
    block.load_state_dict(state, strict=True)
    return block


def run_case(block, g, name, q, device='cpu'):
    """-> {tensor name: value} of the recorded case on `device`, keyed like the fixture"""
    pre = f'{name}/q{q}/'
    dev = lambda k: torch.from_numpy(g[k]).to(device)      # noqa: E731
    x = dev('key').requires_grad_(True)
    y, w = block(x, q, key_index=dev('index'), key_padding_mask=dev('pad'))
    names, params = zip(*block.named_parameters())
    grads = torch.autograd.grad((y * dev(pre + 'cy')).sum() + (w * dev(pre + 'cw')).sum(), (x, *params))
    got = {'y': y, 'w': w, 'g/key': grads[0]}
    got.update({'g/' + n: v for n, v in zip(names, grads[1:])})
    return {k: v.detach().cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize('q', Q_LENS)
@pytest.mark.parametrize('name', GATES)
def test_gated_block_matches_reference(golden_dir, name, q):
    g = np.load(golden_dir / 'f16_gates.npz')
    got = run_case(load_block(g, name), g, name, q)
    pre = f'{name}/q{q}/'
    want = {k[len(pre):] for k in g.files if k.startswith(pre)} - {'cy', 'cw'}
    assert set(got) == want, 'every recorded tensor is compared'
    for k, v in got.items():
        np.testing.assert_allclose(v, g[pre + k], err_msg=k, **TOL)
    pad = g['pad'][:, -q:]
    assert pad.any() and np.all(got['y'][pad] == 0), 'padded query rows are exactly zero'
