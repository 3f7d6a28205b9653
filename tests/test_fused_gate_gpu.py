"""GPU: the gate behind an episode attention block (RESIDUAL / OUTPUT / RECURRENT, reference
nn_models/layers/seq_layers.py:297-345, 460-547) with its padded-row factor as one launch per pass
(`asac_rows_gate_forward/backward`, csrc/rows_gate.hip): the kernels against float64 and against the float32 module path,
the block against the CPU module and the recorded reference values, launch counts, the fallbacks, the learner's direct mode
and a captured train step."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ('RESIDUAL', 'OUTPUT', 'RECURRENT')
# (B, L, Lq, E): a single row; one position of a longer window, the narrow width; rows that do not fill the last tile, a cut
# query; the wide width; more tiles than one round of workgroups (2 700 rows = 169 tiles)
SHAPES = [(1, 1, 1, 64), (5, 18, 1, 32), (37, 9, 3, 64), (3, 7, 7, 128), (300, 9, 9, 64)]
ULP = 2.0 ** -23


def _gate_layer(kind, E):
    from algorithm.nn_models.layers import seq_layers as sl
    if kind == 'RESIDUAL':
        return sl.GatedResidualLayer()
    return sl.GatedOutputLayer(E) if kind == 'OUTPUT' else sl.GatedRecurrentLayer(E)


def _gate_weights(kind, layer):
    """-> ([weights in the kernel's order], bias_z | None, [(weight name, pre-activation index, operand name, bias?)])"""
    if kind == 'RESIDUAL':
        return [], None, []
    if kind == 'OUTPUT':
        return [layer.dense.weight], None, [('dense.weight', 0, 'x')]
    names = ('dense_x_r', 'dense_y_r', 'dense_x_z', 'dense_y_z', 'dense_x_g', 'dense_y_g')
    jobs = [(f'{n}.weight', i // 2, 'rx' if n == 'dense_x_g' else n[6]) for i, n in enumerate(names)]
    return [getattr(layer, n).weight for n in names], layer.dense_x_z.bias, jobs


def _activations(kind, layer, x, y):
    """the tensors the forward launch saves, through the module's own layers"""
    if kind == 'RESIDUAL':
        return []
    if kind == 'OUTPUT':
        return [layer.dense(x)]
    r = torch.sigmoid(layer.dense_x_r(x) + layer.dense_y_r(y))
    z = torch.sigmoid(layer.dense_x_z(x) + layer.dense_y_z(y))
    return [r, z, torch.tanh(layer.dense_x_g(r * x) + layer.dense_y_g(y))]


def _module_pass(kind, layer, x, y, row_zero, g_out):
    """out = gatedlayer(x, y) * ~row_zero, as `EpisodeMultiheadAttentionBlock.forward` forms it, and its backward
    -> {name: tensor}"""
    x, y = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    out = layer(x, y)
    if row_zero is not None:
        out = out * (~row_zero).to(out.dtype).unsqueeze(-1)
    out.backward(g_out)
    got = {'out': out, 'grad_x': x.grad, 'grad_y': y.grad}
    with torch.no_grad():
        got.update({f'saved{i}': t for i, t in enumerate(_activations(kind, layer, x, y))})
    got.update({'grad ' + n: p.grad for n, p in layer.named_parameters()})
    return {k: v.detach().double().cpu() for k, v in got.items()}


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('B,L,Lq,E', SHAPES)
@pytest.mark.parametrize('kind', KINDS)
def test_gate_kernels_against_f64_and_the_module_path(kind, B, L, Lq, E, masked):
    """`asac_rows_gate_forward/backward` on a strided tail view, with and without `row_zero` (a batch entry wholly zeroed),
    outputs pre-filled with NaN — against float64 autograd of the gate layer on the CPU.  The bound is the float32 module
    path's own error against the same float64 values on the same device: per tensor the kernel's largest absolute error
    may be at most 2x the module path's (both are f32 sums over the same terms in another order), with a floor of 4 units
    in the last place at the tensor's largest magnitude for tensors where the library happens to be exact.  RESIDUAL is an
    add and a multiply per element: bit-identical.
    Observed on MI355X: DESIGN.md section 5."""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers.seq_layers import GATE
    gen = torch.Generator().manual_seed(B + L + E)
    torch.manual_seed(B + E)
    big = torch.randn(B, L + 1, E + 8, generator=gen)

    def view(t):          # strides (L + 1)(E + 8), E + 8, 1: multiples of 4, a 16-byte aligned start
        return t[:, L + 1 - Lq:, 4:E + 4]
    y, g_out = torch.randn(B, Lq, E, generator=gen), torch.randn(B, Lq, E, generator=gen)
    pad = None
    if masked:
        pad = torch.rand(B, L, generator=gen) < 0.3
        pad[0] = True
    row_zero = None if pad is None else pad[:, -Lq:]
    layer = _gate_layer(kind, E)

    want = _module_pass(kind, copy.deepcopy(layer).double(), view(big).double(), y.double(), row_zero, g_out.double())
    dev = copy.deepcopy(layer).cuda()
    bigd, yd, gd = big.cuda(), y.cuda(), g_out.cuda()
    rzd = None if pad is None else pad.cuda()[:, -Lq:]
    module = _module_pass(kind, dev, view(bigd), yd, rzd, gd)

    weights, bz, jobs = _gate_weights(kind, dev)
    weights, bz = [w.detach() for w in weights], None if bz is None else bz.detach()
    nan = lambda *shape: torch.full(shape or (B, Lq, E), float('nan'), device='cuda')      # noqa: E731
    out, saved = nan(), [nan() for k in want if k.startswith('saved')]
    native.rows_gate_forward(GATE[kind].value, view(bigd), yd, rzd, weights, bz, out, saved)
    grad_x, grad_y, g_pre = nan(), nan(), [nan() for _ in saved]
    rx = nan() if kind == 'RECURRENT' else None
    native.rows_gate_backward(GATE[kind].value, gd, view(bigd), yd, rzd, weights, saved, grad_x,
                              grad_x if kind == 'RESIDUAL' else grad_y, g_pre, rx)
    kernel = {'out': out, 'grad_x': grad_x, 'grad_y': grad_x if kind == 'RESIDUAL' else grad_y}
    kernel.update({f'saved{i}': t for i, t in enumerate(saved)})
    operands = {'x': view(bigd).reshape(-1, E), 'y': yd.view(-1, E), 'rx': None if rx is None else rx.view(-1, E)}
    for name, i, operand in jobs:       # the parameter gradients: products over the rows of what the backward launch wrote
        gw = nan(E, E)
        gb = nan(E) if name == 'dense_x_z.weight' else None
        native.xty(g_pre[i].view(-1, E), operands[operand], gw, gb)
        kernel['grad ' + name] = gw
        if gb is not None:
            kernel['grad dense_x_z.bias'] = gb
    kernel = {k: v.double().cpu() for k, v in kernel.items()}
    assert set(kernel) == set(want) == set(module)

    bad = []
    for name, ref in want.items():
        assert torch.isfinite(kernel[name]).all(), f'{name}: an element was not written'
        e_k, e_m = float((kernel[name] - ref).abs().max()), float((module[name] - ref).abs().max())
        floor = 4 * ULP * float(ref.abs().max())
        print(f'{kind} {(B, L, Lq, E)} masked={masked} {name}: kernel {e_k:.3e}  module {e_m:.3e}  floor {floor:.3e}')
        if kind == 'RESIDUAL':
            if not torch.equal(kernel[name], module[name]):
                bad.append((name, 'not bit-identical to the module path'))
        elif e_k > max(2 * e_m, floor):
            bad.append((name, e_k, e_m, floor))
    assert not bad, bad
    if masked:
        assert not kernel['out'][0].any() and not kernel['grad_x'][0].any(), 'a zeroed batch entry'


def _block_inputs(B, L, q, E, seed=1):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, E, generator=gen)
    pad = torch.arange(L).unsqueeze(0) < torch.randint(0, 4, (B, 1), generator=gen)       # padding in front, as the learner's
    pad[1, -2:] = True                                                                    # ... and two padded query rows
    index = torch.arange(L).repeat(B, 1) + torch.randint(0, 5, (B, 1), generator=gen)
    return x, pad, index, torch.randn(B, q, E, generator=gen), torch.randn(B, q, L, generator=gen) * 0.2


def _run_block(layer, device, q, x, pad, index, g_out, g_w):
    for p in layer.parameters():
        p.grad = None
    xd = x.clone().to(device).requires_grad_(True)
    key = xd * 1.0
    out, w = layer(key, q, key_index=index.to(device), key_padding_mask=pad.to(device))
    ((out * g_out.to(device)).sum() + (w * g_w.to(device)).sum()).backward()
    return [t.detach().cpu().numpy() for t in (out, w, xd.grad, *(p.grad for p in layer.parameters()))]


def _assert_block_close(got, want, rows, lead=3):
    """the bounds of test_fused_attn_mh_gpu.test_projections_and_output_block_around_the_core_are_one_launch_each"""
    for n_, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(a).all()
        atol = 3e-5 if n_ < lead else 2e-7 * rows * max(1.0, float(np.abs(b).max()) ** 0.5) + 3e-5
        np.testing.assert_allclose(a, b, rtol=3e-4, atol=atol, err_msg=f'output {n_}')


def _calls(seen, prefix):
    return {k: v['calls'] for k, v in seen.items() if k.startswith(prefix)}


@pytest.mark.parametrize('q', [9, 4])
@pytest.mark.parametrize('kind', KINDS)
def test_gated_block_is_the_cpu_module_with_one_gate_launch_per_pass(kind, q):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    ref = sl.EpisodeMultiheadAttentionBlock(64, 8, gate=sl.GATE[kind])
    dev = copy.deepcopy(ref).cuda()
    plain = sl.EpisodeMultiheadAttentionBlock(64, 8).cuda()
    B, L = 300, 9
    inputs = _block_inputs(B, L, q, 64)
    want = _run_block(ref, 'cpu', q, *inputs)
    with native.LaunchProfiler(repeat=1) as prof:
        got = _run_block(dev, 'cuda', q, *inputs)
    seen = prof.summary()
    with native.LaunchProfiler(repeat=1) as prof:
        _run_block(plain, 'cuda', q, *inputs)
    ungated = prof.summary()
    assert seen['asac_rows_gate_forward']['calls'] == 1 and seen['asac_rows_gate_backward']['calls'] == 1, sorted(seen)
    for prefix in ('asac_attention', 'asac_rows_proj', 'asac_rows_resblock'):
        assert _calls(seen, prefix) == _calls(ungated, prefix), 'the attention entry points as often as without a gate'
    multi = seen.get('asac_xty_multi', {'calls': 0})['calls']
    single = seen.get('asac_xty', {'calls': 0})['calls'] - ungated.get('asac_xty', {'calls': 0})['calls']
    assert (multi, single) == {'RESIDUAL': (0, 0), 'OUTPUT': (0, 1), 'RECURRENT': (2, 0)}[kind]
    _assert_block_close(got, want, B * L)
    rows = inputs[1][:, -q:].numpy()
    assert rows.any() and not got[0][rows].any(), 'padded query rows of the output are exactly zero'

    sl.FUSED_GATE = False
    try:
        with native.LaunchProfiler(repeat=1) as prof:
            got = _run_block(dev, 'cuda', q, *inputs)
    finally:
        sl.FUSED_GATE = True
    assert not _calls(prof.summary(), 'asac_rows_gate')
    _assert_block_close(got, want, B * L)


@pytest.mark.parametrize('q', [2, 5])
@pytest.mark.parametrize('kind', KINDS)
def test_recorded_reference_cases_through_the_device_path(golden_dir, kind, q):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from tests.test_gate_golden import load_block, run_case
    g = np.load(golden_dir / 'f16_gates.npz')
    block = load_block(g, kind).cuda()
    with native.LaunchProfiler(repeat=1) as prof:
        got = run_case(block, g, kind, q, 'cuda')
    assert _calls(prof.summary(), 'asac_rows_gate') == {'asac_rows_gate_forward': 1, 'asac_rows_gate_backward': 1}
    pre = f'{kind}/q{q}/'
    names = ['y', 'w', 'g/key'] + sorted(k for k in got if k not in ('y', 'w', 'g/key'))
    _assert_block_close([got[k] for k in names], [g[pre + k] for k in names], g['key'].shape[0] * g['key'].shape[1])
    pad = g['pad'][:, -q:]
    assert pad.any() and not got['y'][pad].any()


@pytest.mark.parametrize('case', ['width48', 'misaligned', 'cat', 'float64', 'subclass'])
def test_what_the_kernel_does_not_cover_runs_the_module_code(case):
    """no `rows_gate` launch, and the values of the CPU module"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    E = 48 if case == 'width48' else 64
    gate = {'width48': sl.GATE.RECURRENT, 'misaligned': sl.GATE.OUTPUT, 'cat': sl.GATE.CAT, 'float64': sl.GATE.RECURRENT,
            'subclass': sl.GATE.RESIDUAL}[case]
    ref = sl.EpisodeMultiheadAttentionBlock(E, 8, gate=gate)
    if case == 'subclass':
        class Halved(sl.GatedResidualLayer):
            def forward(self, x, y):
                return x + 0.5 * y
        ref.gatedlayer = Halved()
    if case == 'float64':
        ref = ref.double()
    dev = copy.deepcopy(ref).cuda()
    if case == 'misaligned':      # a parameter that is a view 4 bytes into its buffer: a segment of a flat buffer behind a scalar
        w = dev.gatedlayer.dense.weight
        buf = torch.empty(w.numel() + 1, device='cuda')
        buf[1:].copy_(w.detach().reshape(-1))
        w.data = buf[1:].view_as(w)
        assert w.data_ptr() % 16 == 4
    B, L, q = 40, 9, 4
    x, pad, index, g_out, g_w = _block_inputs(B, L, q, E)
    if case == 'cat':
        g_out = torch.cat([g_out, g_out.flip(-1)], dim=-1)
    if case == 'float64':
        x, g_out, g_w = x.double(), g_out.double(), g_w.double()
    want = _run_block(ref, 'cpu', q, x, pad, index, g_out, g_w)
    with native.LaunchProfiler(repeat=1) as prof:
        got = _run_block(dev, 'cuda', q, x, pad, index, g_out, g_w)
    assert not _calls(prof.summary(), 'asac_rows_gate')
    if case == 'float64':
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-11)
    else:
        _assert_block_close(got, want, B * L)


def test_two_gated_layers_in_the_learners_direct_mode():
    """`EpisodeMultiheadAttention(64, 2 layers, 8 heads, gate=RECURRENT)` inside `direct_param_grads(), DeferredPartialSums()`:
    the gates' products are queued onto the flat `.grad` views with the attention's — the same `.grad` as a plain backward"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    import algorithm.nn_models as m
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_mlp import DeferredPartialSums, direct_param_grads
    torch.manual_seed(0)
    attn = m.EpisodeMultiheadAttention(64, num_layers=2, num_heads=8, gate=m.GATE.RECURRENT).cuda()
    group = FlatParamGroup([('attn', list(attn.parameters()))], 'cuda')
    B, L = 256, 9
    x, pad, index, g_out, _ = _block_inputs(B, L, L, 64, seed=2)
    x, pad, index, g_out = x.cuda(), pad.cuda(), index.cuda(), g_out.cuda()
    h0 = torch.randn(B, 1, attn.output_hidden_state_dim, device='cuda')

    def loss():
        o, hn, _ = attn(x, seq_q_len=L, hidden_state=h0, is_prev_hidden_state=True, key_index=index, key_padding_mask=pad)
        return (o * g_out).sum() + hn.square().sum()

    group.grad.zero_()
    loss().backward()
    want = group.grad.clone()
    assert want.abs().max() > 0
    group.grad.zero_()
    with native.LaunchProfiler(repeat=1) as prof:
        with direct_param_grads(), DeferredPartialSums() as later:
            loss().backward()
        later.flush()
    seen = prof.summary()
    assert seen['asac_rows_gate_forward']['calls'] == 2 and seen['asac_rows_gate_backward']['calls'] == 2
    assert 'asac_xty' not in seen or seen['asac_xty']['calls'] <= 1, 'the products go four at a time'
    off = 0
    for p in attn.parameters():
        a, b = group.grad[off:off + p.numel()].cpu().numpy(), want[off:off + p.numel()].cpu().numpy()
        off += p.numel()
        atol = 2e-7 * B * (L + 1) * max(1.0, float(np.abs(b).max()) ** 0.5) + 3e-5
        np.testing.assert_allclose(a, b, rtol=3e-4, atol=atol)


def test_captured_step_with_a_gated_representation_matches_eager():
    """a small `SAC_Base` over tests/plugins/nn_attn_gate.py (two RECURRENT-gated blocks, embed 64): three `train()` calls —
    eager, capture + replay, replay, with host work in between — leave the parameters, the tree and the TD errors of three
    eager calls (the gate launches allocate nothing and synchronise nothing, so they are nodes of the step's graph)"""
    import random
    import asac_amd  # noqa: F401
    from asac_amd import native
    from tests import parity_utils as pu
    from algorithm.sac_base import SAC_Base
    from algorithm.utils.enums import SEQ_ENCODER
    rng = np.random.default_rng(1)
    episodes = [pu.synthetic_episode(rng, [(6,)], [], 2, (64,), T) for T in (60, 45, 70)]
    results = []
    for use_graph in (False, True):
        torch.manual_seed(3), np.random.seed(3), random.seed(3)
        agent = SAC_Base(['vector'], [(6,)], [], 2, None, pu.plugin('nn_attn_gate'), device='cuda:0', seq_encoder=SEQ_ENCODER.ATTN,
                         n_step=3, burn_in_step=4, batch_size=16, replay_config={'capacity': 256},
                         hip_config={'use_graph': use_graph, 'graph_warmup': 1})
        for ep in episodes:
            agent.put_episode(**ep)
        torch.manual_seed(4)
        gate_launches = 0
        for i in range(3):
            if i == 0:
                with native.LaunchProfiler(repeat=1) as prof:
                    agent.train()
                gate_launches = sum(prof.summary().get(k, {'calls': 0})['calls']
                                    for k in ('asac_rows_gate_forward', 'asac_rows_gate_backward'))
            else:
                agent.train()
            torch.cuda.synchronize()
            np.sort(np.random.default_rng(i).standard_normal(1 << 14))         # host work between the replays
        assert gate_launches > 0, 'the step runs the one-launch gate'
        assert (agent._graph is not None) == use_graph, 'the gated step must capture'
        results.append((agent._params.flat.cpu().numpy().copy(), agent.replay_buffer._tree.cpu().numpy().copy(),
                        agent._td_error.cpu().numpy().copy()))
        agent.close()
    for name, a, b in zip(('parameters', 'tree', 'td_error'), *results):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)
