"""GPU: which native launches one forward + backward of an attention module issues, per route of
`MultiheadAttention.forward` — the names in order of first appearance and the calls of each, written out literally.

The table pins the dispatch (seq_layers.py) and the launch pairs behind it (algorithm/fused_attention.py): a change that
sends a configuration down another route, doubles a launch or reorders the parameter-gradient products shows here.  The
expected values were recorded from this same test body on the tree before the launch path was unified.  No numbers are
compared: the per-route tests (test_fused_attn*_gpu.py, test_fused_rope_gpu.py, test_fused_gate*_gpu.py,
test_*_dropout_gpu.py) carry them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3


def _case(E=32, heads=2, L=5, tail=2, value_other=False, index=None, switches=(), train=True, gate=False, dtype=torch.float32,
          **module):
    return dict(E=E, heads=heads, L=L, tail=tail, value_other=value_other, index=index, switches=dict(switches), train=train,
                gate=gate, dtype=dtype, module=module)


# name -> (configuration, [(launch, calls), ...] in order of first appearance)
CASES = {
    # two heads, window <= 16: the projections inside the core's forward launch; one ResBlock behind it: the block's launch pair
    'plain_out0': (_case(out_dense_depth=0),
        [('asac_attention_mh_proj_forward', 1), ('asac_attention_mh_backward', 1), ('asac_rows_proj_backward', 1), ('asac_xty', 3)]),
    'plain_out1': (_case(out_dense_depth=1),
        [('asac_attention_mh_proj_forward', 1), ('asac_attention_mh_block_backward', 1), ('asac_xty', 4)]),
    'plain_out1_all_queries': (_case(out_dense_depth=1, tail=5),
        [('asac_attention_mh_proj_forward', 1), ('asac_attention_mh_block_backward', 1), ('asac_xty', 4)]),
    'plain_out2': (_case(out_dense_depth=2),
        [('asac_attention_mh_proj_forward', 1), ('asac_attention_mh_backward', 1), ('asac_rows_proj_backward', 1), ('asac_xty', 3)]),
    'value_is_not_key': (_case(out_dense_depth=1, value_other=True),
        [('asac_attention_mh_forward', 1), ('asac_rows_resblock_forward', 1), ('asac_rows_resblock_backward', 1), ('asac_xty', 1),
         ('asac_attention_mh_backward', 1)]),
    # window 18: past the in-core projections
    'window18_out1': (_case(out_dense_depth=1, L=18),
        [('asac_rows_proj_forward', 1), ('asac_attention_mh_forward', 1), ('asac_rows_resblock_forward', 1),
         ('asac_rows_resblock_backward', 1), ('asac_xty', 4), ('asac_attention_mh_backward', 1), ('asac_rows_proj_backward', 1)]),
    # rotary encodings
    'rope_tail_index': (_case(pe='ROPE', out_dense_depth=1, index='tail'),
        [('asac_rows_proj_rope_forward', 1), ('asac_attention_mh_forward', 1), ('asac_rows_resblock_forward', 1),
         ('asac_rows_resblock_backward', 1), ('asac_xty', 4), ('asac_attention_mh_backward', 1), ('asac_rows_proj_rope_backward', 1)]),
    'rope2_tail_index': (_case(pe='ROPE2', out_dense_depth=1, index='tail'),
        [('asac_rows_proj_rope_forward', 1), ('asac_attention_mh_forward', 1), ('asac_rows_resblock_forward', 1),
         ('asac_rows_resblock_backward', 1), ('asac_xty', 4), ('asac_attention_mh_backward', 1), ('asac_rows_proj_rope_backward', 1)]),
    'rope_unrelated_indexes': (_case(pe='ROPE', out_dense_depth=1, index='unrelated'),
        [('asac_rows_proj_forward', 1), ('asac_rope_forward', 1), ('asac_attention_mh_forward', 1), ('asac_rows_resblock_forward', 1),
         ('asac_rows_resblock_backward', 1), ('asac_xty', 4), ('asac_attention_mh_backward', 1), ('asac_rope_backward', 1),
         ('asac_rows_proj_backward', 1)]),
    'rope_no_indexes_q_ne_k': (_case(pe='ROPE', out_dense_depth=1),
        [('asac_rows_proj_forward', 1), ('asac_rope_forward', 1), ('asac_attention_mh_forward', 1), ('asac_rows_resblock_forward', 1),
         ('asac_rows_resblock_backward', 1), ('asac_xty', 4), ('asac_attention_mh_backward', 1), ('asac_rope_backward', 1),
         ('asac_rows_proj_backward', 1)]),
    # dropout: of the weights, of the dense stacks
    'weights_dropout_train': (_case(dropout=0.5),
        [('asac_rows_proj_forward', 1), ('asac_attention_mh_dropout_forward', 1), ('asac_attention_mh_dropout_backward', 1),
         ('asac_rows_proj_backward', 1), ('asac_xty', 3)]),
    'weights_dropout_eval': (_case(dropout=0.5, train=False),
        [('asac_attention_mh_proj_forward', 1), ('asac_attention_mh_backward', 1), ('asac_rows_proj_backward', 1), ('asac_xty', 3)]),
    'qkv_dense_dropout': (_case(qkv_dense_depth=1, dropout=0.5),
        [('asac_rows_dense_proj_dropout_forward', 1), ('asac_attention_mh_dropout_forward', 1),
         ('asac_attention_mh_dropout_backward', 1), ('asac_rows_dense_proj_dropout_backward', 1), ('asac_xty_multi', 2)]),
    'out_dense_dropout': (_case(out_dense_depth=1, dropout=0.5),
        [('asac_rows_proj_forward', 1), ('asac_attention_mh_dropout_forward', 1), ('asac_rows_resblock_dropout_forward', 1),
         ('asac_rows_resblock_dropout_backward', 1), ('asac_xty', 4), ('asac_attention_mh_dropout_backward', 1),
         ('asac_rows_proj_backward', 1)]),
    # switches
    'no_block_backward': (_case(out_dense_depth=1, switches={'FUSED_BLOCK_BACKWARD': False}),
        [('asac_attention_mh_proj_forward', 1), ('asac_rows_resblock_backward', 1), ('asac_xty', 4), ('asac_attention_mh_backward', 1),
         ('asac_rows_proj_backward', 1)]),
    'no_qkv_in_core': (_case(out_dense_depth=1, switches={'FUSED_QKV_IN_CORE': False}),
        [('asac_rows_proj_forward', 1), ('asac_attention_mh_forward', 1), ('asac_rows_resblock_forward', 1),
         ('asac_rows_resblock_backward', 1), ('asac_xty', 4), ('asac_attention_mh_backward', 1), ('asac_rows_proj_backward', 1)]),
    'no_multihead': (_case(out_dense_depth=1, switches={'FUSED_MULTIHEAD': False}),
        [('asac_rows_proj_forward', 1), ('asac_rows_proj_backward', 1), ('asac_xty', 3)]),
    # one head
    'one_head_out1': (_case(E=8, heads=1, out_dense_depth=1),
        [('asac_attention_proj_forward', 1), ('asac_attention_proj_backward', 1)]),
    'one_head_out0': (_case(E=8, heads=1, out_dense_depth=0),
        [('asac_attention_proj_forward', 1), ('asac_attention_proj_backward', 1)]),
    'one_head_value_is_not_key': (_case(E=8, heads=1, out_dense_depth=1, value_other=True),
        [('asac_attention_forward', 1), ('asac_attention_backward', 1)]),
    # episode blocks, one per gate kind, with a padding mask
    'block_residual': (_case(gate='RESIDUAL'),
        [('asac_attention_mh_proj_forward', 1), ('asac_rows_gate_forward', 1), ('asac_rows_gate_backward', 1),
         ('asac_attention_mh_block_backward', 1), ('asac_xty', 4)]),
    'block_output': (_case(gate='OUTPUT'),
        [('asac_attention_mh_proj_forward', 1), ('asac_rows_gate_forward', 1), ('asac_rows_gate_backward', 1), ('asac_xty', 5),
         ('asac_attention_mh_block_backward', 1)]),
    'block_recurrent': (_case(gate='RECURRENT'),
        [('asac_attention_mh_proj_forward', 1), ('asac_rows_gate_forward', 1), ('asac_rows_gate_backward', 1), ('asac_xty_multi', 2),
         ('asac_attention_mh_block_backward', 1), ('asac_xty', 4)]),
    'block_cat': (_case(gate='CAT'),
        [('asac_attention_mh_proj_forward', 1), ('asac_attention_mh_block_backward', 1), ('asac_xty', 4)]),
    # float64: nothing native
    'float64': (_case(out_dense_depth=1, dtype=torch.float64), []),
}


def build_case(cfg, seed=0):
    """the module on the device and `run() -> (out, weights, x)`: one forward from a fresh leaf `x`"""
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    torch.manual_seed(seed)
    E, L, tail, kw = cfg['E'], cfg['L'], cfg['tail'], dict(cfg['module'])
    if 'pe' in kw:
        kw['pe'] = m.POSITIONAL_ENCODING[kw['pe']]
    if cfg['gate']:
        layer = m.EpisodeMultiheadAttentionBlock(E, cfg['heads'], gate=m.GATE[cfg['gate']], **kw)
    else:
        layer = m.MultiheadAttention(E, cfg['heads'], **kw)
    layer = (layer.double() if cfg['dtype'] == torch.float64 else layer).cuda().train(cfg['train'])      # (no `.to(dtype)`: it casts the rotary table)
    gen = torch.Generator().manual_seed(seed + 1)
    x0 = torch.randn(B, L, E, generator=gen).to(device='cuda', dtype=cfg['dtype'])
    pad = (torch.arange(L).unsqueeze(0) < torch.tensor([[0], [1], [2]])).cuda()          # padding in front, as the learner's
    key_index = (torch.arange(L).repeat(B, 1) + torch.tensor([[0], [3], [1]])).cuda()
    g_out = torch.randn(B, tail, 2 * E if cfg['gate'] == 'CAT' else E, generator=gen).to(x0)
    g_w = (torch.randn(B, tail, L, generator=gen) * 0.2).to(x0)

    def run():
        x = x0.clone().requires_grad_(True)
        if cfg['gate']:
            out, w = layer(x, tail, key_index=key_index, key_padding_mask=pad)
            return out, w, x
        query = x if tail == L else x[:, -tail:]
        index = {}
        if cfg['index'] == 'tail':
            index = dict(query_index=key_index[:, -tail:], key_index=key_index)
        elif cfg['index'] == 'unrelated':
            index = dict(query_index=key_index[:, -tail:].clone(), key_index=key_index)
        out, w = layer(query, x, x * 1.0 if cfg['value_other'] else x, key_padding_mask=pad, **index)
        return out, w, x

    return layer, run, lambda out, w: (out * g_out).sum() + (w * g_w).sum()


def run_case(name, setattr_):
    """one forward and backward of the case under the launch profiler
    -> ([(launch, calls), ...] in order of first appearance, [out, weights, input gradient, parameter gradients ...])"""
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers
    cfg, _ = CASES[name]
    for switch, value in cfg['switches'].items():
        setattr_(seq_layers, switch, value)
    layer, run, loss = build_case(cfg)
    with native.LaunchProfiler(repeat=1) as prof:
        out, w, x = run()
        loss(out, w).backward()
    seen = prof.summary()
    return [(launch, seen[launch]['calls']) for launch in prof.records], [out, w, x.grad, *(p.grad for p in layer.parameters())]


@pytest.mark.parametrize('name', list(CASES))
def test_launches_of_one_forward_and_backward(name, monkeypatch):
    got, tensors = run_case(name, monkeypatch.setattr)
    print(f'{name!r}: {got!r}')
    assert got == CASES[name][1]
    assert all(torch.isfinite(t).all() for t in tensors if t is not None)
