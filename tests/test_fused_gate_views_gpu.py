"""GPU: inputs of the one-launch gate (`asac_rows_gate_*`, csrc/rows_gate.hip) that its host checks would refuse as they come —
a padding mask or a residual source expanded along the batch or the positions (a stride of 0) — are made dense in front of
the launch instead of raising; and a gated block with `use_layer_norm=True` takes the one-launch gate too (the LayerNorm in
front of the attention stays a module; the gate reads the un-normalised residual)."""
import copy

import numpy as np
import pytest
import torch

from tests.test_fused_gate_gpu import KINDS, _assert_block_close, _block_inputs, _calls, _run_block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('kind', KINDS)
def test_gated_block_with_layer_norm_is_the_cpu_module_with_one_gate_launch_per_pass(kind):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    ref = sl.EpisodeMultiheadAttentionBlock(64, 8, gate=sl.GATE[kind], use_layer_norm=True)
    with torch.no_grad():           # (away from the identity the LayerNorm starts as)
        ref.layer_norm.weight.uniform_(0.5, 1.5)
        ref.layer_norm.bias.uniform_(-0.5, 0.5)
    dev = copy.deepcopy(ref).cuda()
    B, L, q = 40, 9, 4
    inputs = _block_inputs(B, L, q, 64)
    want = _run_block(ref, 'cpu', q, *inputs)
    with native.LaunchProfiler(repeat=1) as prof:
        got = _run_block(dev, 'cuda', q, *inputs)
    assert _calls(prof.summary(), 'asac_rows_gate') == {'asac_rows_gate_forward': 1, 'asac_rows_gate_backward': 1}
    _assert_block_close(got, want, B * L)


@pytest.mark.parametrize('kind', KINDS)
def test_a_padding_mask_expanded_along_the_batch_goes_through_the_gate_launch(kind):
    """`mask_row.expand(B, -1)`: batch stride 0"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    ref = sl.EpisodeMultiheadAttentionBlock(64, 8, gate=sl.GATE[kind])
    dev = copy.deepcopy(ref).cuda()
    B, L, q = 40, 9, 4
    x, _, index, g_out, g_w = _block_inputs(B, L, q, 64)
    row = torch.zeros(1, L, dtype=torch.bool)
    row[0, :2] = row[0, -1] = True       # two padded keys in front, the newest query row padded
    pad = row.expand(B, -1)
    assert pad.stride(0) == 0
    want = _run_block(ref, 'cpu', q, x, pad, index, g_out, g_w)
    with native.LaunchProfiler(repeat=1) as prof:
        got = _run_block(dev, 'cuda', q, x, pad, index, g_out, g_w)
    assert _calls(prof.summary(), 'asac_rows_gate') == {'asac_rows_gate_forward': 1, 'asac_rows_gate_backward': 1}
    _assert_block_close(got, want, B * L)
    assert not got[0][:, -1].any()


@pytest.mark.parametrize('expand', ['batch', 'positions'])
def test_a_residual_source_expanded_along_batch_or_positions_goes_through_the_gate_launch(expand):
    """`_GateRowsFn` on x = one window for the whole batch / one position for the whole window (stride 0), RECURRENT: the values
    of the gate layer's module code on the same tensors"""
    import asac_amd  # noqa: F401
    from algorithm.fused_attention import _GateRowsFn
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    B, L, E = 5, 7, 32
    layer = sl.GatedRecurrentLayer(E).cuda()
    base = torch.randn((1, L, E) if expand == 'batch' else (B, 1, E), device='cuda')
    y0, g_out = torch.randn(B, L, E, device='cuda'), torch.randn(B, L, E, device='cuda')
    pad = torch.rand(B, L, device='cuda') < 0.3
    lins = (layer.dense_x_r, layer.dense_y_r, layer.dense_x_z, layer.dense_y_z, layer.dense_x_g, layer.dense_y_g)
    results = []
    for fused in (False, True):
        for p in layer.parameters():
            p.grad = None
        src, y = base.clone().requires_grad_(True), y0.clone().requires_grad_(True)
        x = src.expand(B, L, E)
        assert 0 in x.stride()
        if fused:
            out = _GateRowsFn.apply(sl.GATE.RECURRENT.value, x, y, pad, *(ll.weight for ll in lins), layer.dense_x_z.bias)
        else:
            out = layer(x, y) * (~pad).to(y.dtype).unsqueeze(-1)
        out.backward(g_out)
        results.append([t.detach().cpu().numpy() for t in (out, src.grad, y.grad, *(p.grad for p in layer.parameters()))])
    for n_, (a, b) in enumerate(zip(results[1], results[0])):
        assert np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=3e-4, atol=3e-5, err_msg=f'tensor {n_}')
