"""GPU: the rotary position encodings (ROPE / ROPE2, reference nn_models/layers/seq_layers.py `RotaryPositionalEncoding`,
`RotaryPositionalEncoding2` behind the projections of `MultiheadAttention.forward`) as one launch per pass: on their own
(`asac_rope_forward/backward`, csrc/rope.hip) against float64 and the float32 module path, as the epilogue of the projection
launch (`asac_rows_proj_rope_forward/backward`, csrc/rows_proj.hip) bit for bit against the composition, the block against the
CPU module and the recorded reference values, launch counts, the fallbacks, the learner's direct mode and a captured step."""
import copy

import numpy as np
import pytest
import torch

from tests.test_fused_gate_gpu import _assert_block_close, _block_inputs, _calls, _run_block

pytestmark = pytest.mark.gpu

KINDS = ('ROPE', 'ROPE2')
# (B, Lk, Lq, E): a single row; one query position of a longer window, the narrow width; rows that do not fill the last tile, a
# cut query; the wide width; more tiles than one round of workgroups (2 700 rows = 169 tiles)
FUSED_SHAPES = [(1, 1, 1, 32), (5, 18, 1, 32), (37, 9, 3, 64), (3, 7, 7, 128), (300, 9, 9, 64)]
# widths the projection launch does not have: head_dim 5; three pairs; the smallest width with two pairs a half
OTHER_SHAPES = [(4, 20, 20, 40), (3, 7, 5, 6), (2, 5, 5, 8)]
ULP = 2.0 ** -23
T = 5000      # the modules' table length


def _rope_module(kind, E):
    from algorithm.nn_models.layers import seq_layers as sl
    return sl.RotaryPositionalEncoding(E) if kind == 'ROPE' else sl.RotaryPositionalEncoding2(E)


def _tables(kind, module):
    return (torch.view_as_real(module.freqs_cis),) if kind == 'ROPE' else (module.cos_cached, module.sin_cached)


def _strided(gen, B, L, E):
    """-> (buffer, view): strides multiples of 4, a 16-byte aligned start that is not the buffer's"""
    W = (E + 8 + 3) // 4 * 4
    return torch.randn(B, L + 1, W, generator=gen), (lambda t: t[:, 1:, 4:E + 4])


def _indexes(gen, B, Lk, Lq, mode):
    """key indexes [B, Lk] and the query's = their newest Lq entries: consecutive positions from a random start, -1 (the episode
    block's filler: table row T - 1) over the first positions of some rows, one row ending at T - 1 itself; 'arange': the
    stride-0 rows `MultiheadAttention` builds when it is given no index"""
    if mode == 'arange':
        return torch.arange(Lq).unsqueeze(0).expand(B, -1), torch.arange(Lk).unsqueeze(0).expand(B, -1)
    index = torch.arange(Lk).repeat(B, 1) + torch.randint(0, 50, (B, 1), generator=gen)
    index[-1] = torch.arange(T - Lk, T)
    for b in range(0, B, 3):
        index[b, :min(Lk - 1, 1 + b % 4)] = -1
    index = index.to(torch.int32 if mode == 'int32' else torch.int64)
    return index[:, -Lq:], index


def _module_pass(module, qi, ki, q, k, gq, gk):
    q, k = q.detach().clone().requires_grad_(True), k.detach().clone().requires_grad_(True)
    yq, yk = module(qi.long(), ki.long(), q, k)      # (the module's own cast for ROPE; ROPE2 indexes with what it is given)
    ((yq * gq).sum() + (yk * gk).sum()).backward()
    return {n: t.detach().double().cpu() for n, t in (('out_q', yq), ('out_k', yk), ('grad_q', q.grad), ('grad_k', k.grad))}


@pytest.mark.parametrize('mode', ['int32', 'int64', 'arange'])
@pytest.mark.parametrize('B,Lk,Lq,E', FUSED_SHAPES + OTHER_SHAPES)
@pytest.mark.parametrize('kind', KINDS)
def test_rope_kernels_against_f64_and_the_module_path(kind, B, Lk, Lq, E, mode):
    """`asac_rope_forward/backward` on strided views, outputs pre-filled with NaN — against the module code in float64 on the
    CPU (`.double()` leaves the tables' values as they are).  The bound is the rule of test_fused_gate_gpu.py: per tensor the
    kernel's largest absolute error may be at most 2x that of the float32 module path on the same device, with a floor of 4
    units in the last place at the tensor's largest magnitude — an element is two products and a sum, three roundings of at
    most half a unit at magnitudes no larger than ~1.5x the result's maximum."""
    import asac_amd  # noqa: F401
    from asac_amd import native
    gen = torch.Generator().manual_seed(B + Lk + E)
    (bq, view), (bk, _) = _strided(gen, B, Lq, E), _strided(gen, B, Lk, E)
    gq, gk = torch.randn(B, Lq, E, generator=gen), torch.randn(B, Lk, E, generator=gen)
    qi, ki = _indexes(gen, B, Lk, Lq, mode)
    module = _rope_module(kind, E)

    want = _module_pass(copy.deepcopy(module).double(), qi, ki, view(bq).double(), view(bk).double(), gq.double(), gk.double())
    dev = copy.deepcopy(module).cuda()
    bqd, bkd, gqd, gkd, qid, kid = (t.cuda() for t in (bq, bk, gq, gk, qi, ki))
    if mode == 'arange':
        qid, kid = (torch.arange(n, device='cuda').unsqueeze(0).expand(B, -1) for n in (Lq, Lk))
        assert B == 1 or kid.stride(0) == 0
    f32 = _module_pass(dev, qid, kid, view(bqd), view(bkd), gqd, gkd)

    kind_id = {'ROPE': native.ROPE, 'ROPE2': native.ROPE2}[kind]
    assert native.rope_supported(kind_id, E)
    nan = lambda L: torch.full((B, L, E), float('nan'), device='cuda')      # noqa: E731
    out_q, out_k, grad_q, grad_k = nan(Lq), nan(Lk), nan(Lq), nan(Lk)
    native.rope_forward(kind_id, _tables(kind, dev), view(bqd), view(bkd), qid, kid, out_q, out_k)
    native.rope_backward(kind_id, _tables(kind, dev), gqd, gkd, qid, kid, grad_q, grad_k)
    kernel = {n: t.double().cpu() for n, t in (('out_q', out_q), ('out_k', out_k), ('grad_q', grad_q), ('grad_k', grad_k))}

    bad = []
    for name, ref in want.items():
        assert torch.isfinite(kernel[name]).all(), f'{name}: an element was not written'
        e_k, e_m = float((kernel[name] - ref).abs().max()), float((f32[name] - ref).abs().max())
        floor = 4 * ULP * float(ref.abs().max())
        print(f'{kind} {(B, Lk, Lq, E)} {mode} {name}: kernel {e_k:.3e}  module {e_m:.3e}  floor {floor:.3e}')
        if e_k > max(2 * e_m, floor):
            bad.append((name, e_k, e_m, floor))
    assert not bad, bad


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('B,L,Lq,E', FUSED_SHAPES)
@pytest.mark.parametrize('kind', KINDS)
def test_projection_launch_with_rotation_is_the_composition_bit_for_bit(kind, B, L, Lq, E, dtype):
    """`asac_rows_proj_rope_forward` = `asac_rows_proj_forward` then `asac_rope_forward` on its q and k, v untouched;
    `asac_rows_proj_rope_backward` = `asac_rope_backward` then `asac_rows_proj_backward` — torch.equal on everything"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    gen = torch.Generator().manual_seed(B + L + E)
    buf, view = _strided(gen, B, L, E)
    x = view(buf.cuda())
    weights = [(torch.randn(E, E, generator=gen) / E ** 0.5).cuda() for _ in range(3)]
    biases = [torch.randn(E, generator=gen).cuda() for _ in range(3)]
    qi, ki = (t.cuda() for t in _indexes(gen, B, L, Lq, 'int32' if dtype == torch.int32 else 'int64'))
    grads = [torch.randn(B, n, E, generator=gen).cuda() for n in (Lq, L, L)]
    kind_id = {'ROPE': native.ROPE, 'ROPE2': native.ROPE2}[kind]
    tables = _tables(kind, _rope_module(kind, E).cuda())
    tails = [Lq, L, L]
    nan = lambda n: torch.full((B, n, E), float('nan'), device='cuda')      # noqa: E731

    plain = [nan(n) for n in tails]
    native.rows_proj_forward(x, weights, biases, tails, plain)
    want_q, want_k = nan(Lq), nan(L)
    native.rope_forward(kind_id, tables, plain[0], plain[1], qi, ki, want_q, want_k)
    got = [nan(n) for n in tails]
    native.rows_proj_rope_forward(kind_id, tables, ki, x, weights, biases, tails, got)
    for name, a, b in zip('qkv', got, (want_q, want_k, plain[2])):
        assert torch.isfinite(a).all() and torch.equal(a, b), f'forward {name}: {float((a - b).abs().max()):.3e}'
    assert not torch.equal(got[0], plain[0]) or (ki == 0).all(), 'the rotation ran'

    un_q, un_k = nan(Lq), nan(L)
    native.rope_backward(kind_id, tables, grads[0], grads[1], qi, ki, un_q, un_k)
    want_x = nan(L)
    native.rows_proj_backward([un_q, un_k, grads[2]], tails, weights, want_x)
    got_x, got_q, got_k = nan(L), nan(Lq), nan(L)
    native.rows_proj_rope_backward(kind_id, tables, ki, grads, tails, weights, got_x, [got_q, got_k])
    for name, a, b in (('grad_q', got_q, un_q), ('grad_k', got_k, un_k), ('grad_x', got_x, want_x)):
        assert torch.isfinite(a).all() and torch.equal(a, b), f'backward {name}: {float((a - b).abs().max()):.3e}'


def _blocks():
    from algorithm.nn_models.layers import seq_layers as sl
    pe, res = sl.POSITIONAL_ENCODING, sl.GATE.RESIDUAL
    core = {'asac_attention_mh_forward': 1, 'asac_attention_mh_backward': 1}
    out_block = {'asac_rows_resblock_forward': 1, 'asac_rows_resblock_backward': 1}
    return {
        # the same blocks with pe=None run projections, core and output ResBlock as `asac_attention_mh_proj_forward` +
        # `asac_attention_mh_block_backward`; the rotation sits between projections and scores, so here each is a launch
        'rope': (lambda: sl.EpisodeMultiheadAttentionBlock(64, 8, pe=pe.ROPE, gate=res), 64, core, out_block),
        'rope2': (lambda: sl.EpisodeMultiheadAttentionBlock(64, 8, pe=pe.ROPE2, gate=res), 64, core, out_block),
        # the block of the reference's envs/roller/nn_hard_attn.py: one head of 32 channels, no output layer
        'hard_attn': (lambda: sl.EpisodeMultiheadAttentionBlock(32, 1, pe=pe.ROPE2, out_dense_depth=0, gate=res), 32, core, {}),
    }


@pytest.mark.parametrize('q', [9, 4])
@pytest.mark.parametrize('case', ['rope', 'rope2', 'hard_attn'])
def test_rotary_block_is_the_cpu_module_with_one_projection_launch_per_pass(case, q):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    build, E, core, out_block = _blocks()[case]
    ref = build()
    dev = copy.deepcopy(ref).cuda()
    B, L = 300, 9
    inputs = _block_inputs(B, L, q, E)
    want = _run_block(ref, 'cpu', q, *inputs)
    assert sl.FUSED_ROPE in (True, False)
    before = sl.FUSED_ROPE
    try:
        sl.FUSED_ROPE = True
        with native.LaunchProfiler(repeat=1) as prof:
            got = _run_block(dev, 'cuda', q, *inputs)
        seen = prof.summary()
        assert _calls(seen, 'asac_rows_proj') == {'asac_rows_proj_rope_forward': 1, 'asac_rows_proj_rope_backward': 1}, sorted(seen)
        assert not _calls(seen, 'asac_rope'), 'no rotation launch of its own'
        assert _calls(seen, 'asac_attention') == core, sorted(seen)
        assert _calls(seen, 'asac_rows_resblock') == out_block, sorted(seen)
        _assert_block_close(got, want, B * L)

        sl.FUSED_ROPE = False
        with native.LaunchProfiler(repeat=1) as prof:
            got = _run_block(dev, 'cuda', q, *inputs)
        seen = prof.summary()
        assert not _calls(seen, 'asac_rope') and not [k for k in seen if '_rope_' in k], sorted(seen)
        _assert_block_close(got, want, B * L)
    finally:
        sl.FUSED_ROPE = before


@pytest.mark.parametrize('case', ['qkv_depth1', 'distinct_qkv'])
def test_what_the_projection_launch_does_not_cover_rotates_in_one_launch_per_pass(case):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    assert sl.FUSED_ROPE in (True, False)
    before = sl.FUSED_ROPE
    sl.FUSED_ROPE = True
    try:
        if case == 'qkv_depth1':      # projections with a hidden layer, as the reference's toy plugins
            ref = sl.EpisodeMultiheadAttentionBlock(64, 8, pe=sl.POSITIONAL_ENCODING.ROPE, qkv_dense_depth=1, gate=sl.GATE.RESIDUAL)
            dev = copy.deepcopy(ref).cuda()
            B, L, q = 40, 9, 4
            inputs = _block_inputs(B, L, q, 64)
            want = _run_block(ref, 'cpu', q, *inputs)
            with native.LaunchProfiler(repeat=1) as prof:
                got = _run_block(dev, 'cuda', q, *inputs)
            lead, rows = 3, B * L
        else:                         # distinct query / key / value tensors, head_dim 5, no indexes, Lq != Lk
            ref = sl.MultiheadAttention(40, 8, pe=sl.POSITIONAL_ENCODING.ROPE2, out_dense_depth=1)
            dev = copy.deepcopy(ref).cuda()
            B, Lq, Lk = 4, 20, 27
            gen = torch.Generator().manual_seed(1)
            tensors = [torch.randn(B, n, 40, generator=gen) for n in (Lq, Lk, Lk)]
            g_out, g_w = torch.randn(B, Lq, 40, generator=gen), torch.randn(B, Lq, Lk, generator=gen) * 0.2

            def run(layer, device):
                for p in layer.parameters():
                    p.grad = None
                qd, kd, vd = (t.clone().to(device).requires_grad_(True) for t in tensors)
                out, w = layer(qd, kd, vd)
                ((out * g_out.to(device)).sum() + (w * g_w.to(device)).sum()).backward()
                return [t.detach().cpu().numpy() for t in (out, w, qd.grad, kd.grad, vd.grad, *(p.grad for p in layer.parameters()))]
            want = run(ref, 'cpu')
            with native.LaunchProfiler(repeat=1) as prof:
                got = run(dev, 'cuda')
            lead, rows = 5, B * Lk
    finally:
        sl.FUSED_ROPE = before
    seen = prof.summary()
    assert _calls(seen, 'asac_rope') == {'asac_rope_forward': 1, 'asac_rope_backward': 1}, sorted(seen)
    assert not [k for k in seen if k.startswith('asac_rows_proj_rope')]
    _assert_block_close(got, want, rows, lead=lead)


@pytest.mark.parametrize('tag', ['rope_res_ln', 'rope2_out', 'single'])
def test_recorded_reference_cases_through_the_device_path(golden_dir, tag):
    """the reference's own outputs (f7_attention.npz; embed 8: the rotation's own launch) for the hidden-state modes of
    test_attention_golden.py, on the device"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import seq_layers as sl
    from tests.test_attention_golden import CASES, _load
    g = np.load(golden_dir / 'f7_attention.npz')
    attn = m.EpisodeMultiheadAttention(**CASES[tag])
    _load(attn, g, f'{tag}/w/')
    attn = attn.cuda()
    key, index, pad = (torch.from_numpy(g[f'{tag}/{k}']).cuda() for k in ('key', 'index', 'pad'))
    K, Q = key.shape[1], 3
    hs = lambda mode: torch.from_numpy(g[f'{tag}/{mode}/hs']).cuda()      # noqa: E731
    calls = {
        'A': lambda: attn(key, seq_q_len=Q, key_index=index, key_padding_mask=pad),
        'A_full': lambda: attn(key, seq_q_len=K, cut_query=True, key_index=index, key_padding_mask=pad),
        'C': lambda: attn(key, seq_q_len=K, hidden_state=hs('C'), is_prev_hidden_state=True, key_index=index, key_padding_mask=pad),
        'B': lambda: attn(key, seq_q_len=1, hidden_state=hs('B'), is_prev_hidden_state=False, key_index=index, key_padding_mask=pad),
        'R': lambda: attn(key, seq_q_len=Q, query_only_attend_to_rest_key=True, key_index=index),
    }
    assert sl.FUSED_ROPE in (True, False)
    before = sl.FUSED_ROPE
    sl.FUSED_ROPE = True
    try:
        with native.LaunchProfiler(repeat=1) as prof, torch.no_grad():
            got = {mode: fn() for mode, fn in calls.items()}
    finally:
        sl.FUSED_ROPE = before
    assert prof.summary().get('asac_rope_forward', {'calls': 0})['calls'] >= len(calls), sorted(prof.summary())
    rows = key.shape[0] * key.shape[1]
    for mode, (y, h, _) in got.items():
        _assert_block_close([y.cpu().numpy(), h.cpu().numpy()], [g[f'{tag}/{mode}/y'], g[f'{tag}/{mode}/h']], rows)
    assert not got['A'][0][2].any(), 'fully padded rows give zeros'


@pytest.mark.parametrize('case', ['float64', 'subclass', 'misaligned'])
def test_what_the_kernels_do_not_cover_runs_the_module_code(case):
    """no fused-projection launch (float64, a subclassed rope module: no rotation launch either), and the values of the CPU
    module"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    ref = sl.EpisodeMultiheadAttentionBlock(64, 8, pe=sl.POSITIONAL_ENCODING.ROPE, gate=sl.GATE.RESIDUAL)
    if case == 'subclass':
        class Shifted(sl.RotaryPositionalEncoding):
            def forward(self, xq_indexes, xk_indexes, xq, xk):
                return super().forward(xq_indexes + 1, xk_indexes + 1, xq, xk)
        ref.attn.rope = Shifted(64)
    if case == 'float64':
        ref = ref.double()
    dev = copy.deepcopy(ref).cuda()
    if case == 'misaligned':      # a parameter that is a view 4 bytes into its buffer: a segment of a flat buffer behind a scalar
        w = sl._plain_linear(dev.attn.k_proj).weight
        buf = torch.empty(w.numel() + 1, device='cuda')
        buf[1:].copy_(w.detach().reshape(-1))
        w.data = buf[1:].view_as(w)
        assert w.data_ptr() % 16 == 4
    B, L, q = 40, 9, 4
    x, pad, index, g_out, g_w = _block_inputs(B, L, q, 64)
    if case == 'float64':
        x, g_out, g_w = x.double(), g_out.double(), g_w.double()
    want = _run_block(ref, 'cpu', q, x, pad, index, g_out, g_w)
    assert sl.FUSED_ROPE in (True, False)
    before = sl.FUSED_ROPE
    sl.FUSED_ROPE = True
    try:
        with native.LaunchProfiler(repeat=1) as prof:
            got = _run_block(dev, 'cuda', q, x, pad, index, g_out, g_w)
    finally:
        sl.FUSED_ROPE = before
    seen = prof.summary()
    assert not _calls(seen, 'asac_rows_proj'), sorted(seen)
    if case == 'misaligned':
        assert _calls(seen, 'asac_rope') == {'asac_rope_forward': 1, 'asac_rope_backward': 1}, 'the rotation alone is one launch'
    else:
        assert not _calls(seen, 'asac_rope'), sorted(seen)
    if case == 'float64':
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-11)
    else:
        _assert_block_close(got, want, B * L)


def test_two_layers_in_the_learners_direct_mode():
    """`EpisodeMultiheadAttention(64, 2 layers, 8 heads, pe=[ROPE, None])` inside `direct_param_grads(), DeferredPartialSums()`:
    the products of the un-rotated gradients are queued onto the flat `.grad` views — the same `.grad` as a plain backward"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    import algorithm.nn_models as m
    from algorithm.nn_models.layers import seq_layers as sl
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_mlp import DeferredPartialSums, direct_param_grads
    torch.manual_seed(0)
    attn = m.EpisodeMultiheadAttention(64, num_layers=2, num_heads=8, pe=[m.POSITIONAL_ENCODING.ROPE, None]).cuda()
    group = FlatParamGroup([('attn', list(attn.parameters()))], 'cuda')
    B, L = 256, 9
    x, pad, index, g_out, _ = _block_inputs(B, L, L, 64, seed=2)
    x, pad, index, g_out = x.cuda(), pad.cuda(), index.cuda(), g_out.cuda()
    h0 = torch.randn(B, 1, attn.output_hidden_state_dim, device='cuda')

    def loss():
        o, hn, _ = attn(x, seq_q_len=L, hidden_state=h0, is_prev_hidden_state=True, key_index=index, key_padding_mask=pad)
        return (o * g_out).sum() + hn.square().sum()

    assert sl.FUSED_ROPE in (True, False)
    before = sl.FUSED_ROPE
    sl.FUSED_ROPE = True
    try:
        group.grad.zero_()
        loss().backward()
        want = group.grad.clone()
        assert want.abs().max() > 0
        group.grad.zero_()
        with native.LaunchProfiler(repeat=1) as prof:
            with direct_param_grads(), DeferredPartialSums() as later:
                loss().backward()
            later.flush()
    finally:
        sl.FUSED_ROPE = before
    seen = prof.summary()
    assert seen['asac_rows_proj_rope_forward']['calls'] == 1 and seen['asac_rows_proj_rope_backward']['calls'] == 1, sorted(seen)
    off = 0
    for p in attn.parameters():
        a, b = group.grad[off:off + p.numel()].cpu().numpy(), want[off:off + p.numel()].cpu().numpy()
        off += p.numel()
        atol = 2e-7 * B * (L + 1) * max(1.0, float(np.abs(b).max()) ** 0.5) + 3e-5
        np.testing.assert_allclose(a, b, rtol=3e-4, atol=atol)


def test_captured_step_with_a_rotary_representation_matches_eager():
    """a small `SAC_Base` over tests/plugins/nn_attn_rope.py (rotary first block, embed 64): three `train()` calls — eager,
    capture + replay, replay, with host work in between — leave the parameters, the tree and the TD errors of three eager
    calls (the rope launches allocate nothing and synchronise nothing, so they are nodes of the step's graph)"""
    import random
    import asac_amd  # noqa: F401
    from asac_amd import native
    from tests import parity_utils as pu
    from algorithm.nn_models.layers import seq_layers as sl
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    rng = np.random.default_rng(1)
    episodes = [pu.synthetic_episode(rng, [(6,)], [], 2, (64,), T_) for T_ in (60, 45, 70)]
    results = []
    assert sl.FUSED_ROPE in (True, False)
    before = sl.FUSED_ROPE
    sl.FUSED_ROPE = True
    try:
        for use_graph in (False, True):
            torch.manual_seed(3), np.random.seed(3), random.seed(3)
            agent = SAC_Base(['vector'], [(6,)], [], 2, None, pu.plugin('nn_attn_rope'), device='cuda:0', seq_encoder=SEQ_ENCODER.ATTN,
                             n_step=3, burn_in_step=4, batch_size=16, replay_config={'capacity': 256},
                             hip_config={'use_graph': use_graph, 'graph_warmup': 1})
            for ep in episodes:
                agent.put_episode(**ep)
            torch.manual_seed(4)
            rope_launches = 0
            for i in range(3):
                if i == 0:
                    with native.LaunchProfiler(repeat=1) as prof:
                        agent.train()
                    rope_launches = sum(v['calls'] for k, v in prof.summary().items() if k.startswith('asac_rope') or '_rope_' in k)
                else:
                    agent.train()
                torch.cuda.synchronize()
                np.sort(np.random.default_rng(i).standard_normal(1 << 14))         # host work between the replays
            assert rope_launches > 0, 'the step runs the one-launch rotation'
            assert (agent._graph is not None) == use_graph, 'the rotary step must capture'
            results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                            agent._td_error.cpu().numpy().copy()))
            agent.close()
    finally:
        sl.FUSED_ROPE = before
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)
