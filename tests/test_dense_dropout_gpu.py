"""GPU: the live `nn.Dropout` modules of the dense stacks inside the row launches (`asac_rows_dense_proj_dropout_*`,
`asac_rows_resblock_dropout_*`, csrc/rows_proj.hip) against the float64 restatement of tests/dense_dropout_ref.py fed the
RESTATED masks of the call counters the launches report.  Nothing here is compared with torch's own dropout draws.

Tolerances: tests/dense_dropout_tolerances.json holds, per p and output, 4 x the largest error observed on the
MI355X as a FRACTION of the cap — 1 / (1 - p) x (rtol 3e-4, atol 3e-5) for outputs and input gradients, the parameter-gradient
formula of tests/test_attn_dropout_gpu.py with the row count in place of B * Lq for the rest; no fraction exceeds 1.  The whole
module (four launch pairs in a row) is held to four times that cap: `_check`."""
import copy
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

from tests import dense_dropout_ref as ref

pytestmark = pytest.mark.gpu

TOL = json.loads((Path(__file__).resolve().parent / 'dense_dropout_tolerances.json').read_text())
SEED, INSTANCE = 20240229, 77
# (B, L, tail, E, x is a slice of a wider buffer)
SHAPES = [
    (3, 7, 7, 32, False),       # 21 rows: a ragged last tile; two waves without a feature tile
    (3, 7, 1, 64, False),       # the q job has 3 rows, k / v have 21
    (5, 9, 4, 128, False),      # two feature tiles per wave
    (1, 9, 9, 64, False),       # one workgroup is first and last arriver
    (70, 9, 3, 64, False),      # 40 workgroups: more than the 32 leaf arrival words
    (3, 7, 2, 64, True),        # x is buf[:, :, :64] of a [3, 7, 68] buffer: a row pitch that is not the width
]
OUT_SHAPES = [(16, 64), (21, 32), (630, 128)]      # (rows, E) of the output block: a full tile, a ragged one, 40 workgroups


def _state(counter):
    from asac_amd import native
    state = torch.tensor([counter] + [0] * (native.ATTN_DROPOUT_STATE_WORDS - 1), dtype=torch.int64, device='cuda')
    return state, torch.full((1,), -1, dtype=torch.int64, device='cuda')


def _state_is(state, counter):
    return int(state[0].item()) == counter and int(torch.count_nonzero(state[1:]).item()) == 0


@functools.lru_cache(maxsize=None)
def _case(B, L, tail, E, p, counter):
    """inputs, restated masks and the float64 restatement of a shape: built once, shared, never modified"""
    import asac_amd  # noqa: F401
    c = ref.case(B, L, tail, E, p, counter=counter, seed=SEED, instance=INSTANCE)
    c['want'] = ref.composition(c['x'].double(), tail, c['params'], c['lin_out'], c['kept'], c['kept_out'], p, c['g_outs'],
                                c['g_y'], c['row_scale'])
    return c


def _x_on_device(c, strided):
    """(leaf, the [B, L, E] tensor handed to the launch): a slice of a wider buffer where the case says so"""
    x = c['x']
    if not strided:
        leaf = x.clone().cuda().requires_grad_(True)
        return leaf, leaf
    B, L, E = x.shape
    buf = torch.zeros(B, L, E + 4)
    buf[:, :, :E] = x
    leaf = buf.cuda().requires_grad_(True)
    return leaf, leaf[:, :, :E]


CHAIN = 4      # launch pairs between a whole module's input and output: dense stacks, rotation, core, output block


def _check(name, got, want, p, rows, label):
    """`module_*`: the whole module is a chain of CHAIN launch pairs, each held to the cap on its own — to first order their
    errors add, so the chain is held to CHAIN x the cap (the deepest gradients, q_proj's, pass through all four)"""
    tol = TOL[f'p={p}'][name]
    assert np.isfinite(got).all(), name
    frac = ref.fraction_of_cap(got, want, p, rows) / (CHAIN if name.startswith('module_') else 1)
    print(f'dense dropout {label} p={p} {name}: {frac:.4f} of the cap (tolerance {tol:.4f})')
    assert tol <= 1.0
    assert frac <= tol, f'{label} {name}: {frac:.4f} of the cap, tolerance {tol:.4f}'


@pytest.mark.parametrize('B,L,tail,E,strided', SHAPES)
def test_zeros_of_the_hidden_rows_are_the_restated_masks(B, L, tail, E, strided):
    from asac_amd import native
    p, counter = 0.5, 5
    c = _case(B, L, tail, E, p, counter)
    _, x = _x_on_device(c, strided)
    x = x.detach()
    params = [t.cuda() for t in c['params']]
    tails = [tail, L, L]
    new = lambda: [torch.full((B, t, E), float('nan'), device='cuda') for t in tails]      # noqa: E731
    outs, pres, hiddens = new(), new(), new()
    state, used = _state(counter)
    native.rows_dense_proj_dropout_forward(x, params[0::4], params[1::4], params[2::4], params[3::4], tails, outs, pres, hiddens,
                                           p, SEED, INSTANCE, state, used)
    torch.cuda.synchronize()
    assert int(used.item()) == counter and _state_is(state, counter + 1)
    for j, name in enumerate('qkv'):
        got_zero = hiddens[j].cpu().numpy() == 0
        assert (got_zero == ~c['kept'][j]).all(), f'h_{name}: {int((got_zero != ~c["kept"][j]).sum())} entries differ'
        assert 0.25 <= got_zero.mean() <= 0.75 or got_zero.size < 256      # the test cannot pass with an empty or a full mask
        assert all(torch.isfinite(t[j]).all() for t in (outs, pres, hiddens)), 'every row of every output is written'


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('rows,E', OUT_SHAPES)
def test_zeros_of_the_output_block_are_the_restated_mask(rows, E, scaled):
    from asac_amd import native
    p, counter = 0.5, 9
    gen = torch.Generator().manual_seed(rows + E)
    x, w, b = torch.randn(rows, E, generator=gen), torch.randn(E, E, generator=gen) * 0.2, torch.randn(E, generator=gen) * 0.1
    sc = (torch.rand(rows, generator=gen) < 0.7).float() * 1.5
    sc[0] = sc[rows - 1] = 0.
    y, pre = (torch.full((rows, E), float('nan'), device='cuda') for _ in range(2))
    state, used = _state(counter)
    native.rows_resblock_dropout_forward(x.cuda(), w.cuda(), b.cuda(), sc.cuda() if scaled else None, y, pre, p, SEED, INSTANCE,
                                         state, used)
    torch.cuda.synchronize()
    assert int(used.item()) == counter and _state_is(state, counter + 1)
    kept = ref.rows_mask(SEED, INSTANCE, counter, ref.TAG_OUT, rows, E, p)
    got_zero = y.cpu().numpy() == 0
    on = (sc != 0).numpy() if scaled else np.ones(rows, bool)
    assert (got_zero[on] == ~kept[on]).all() and got_zero[~on].all()
    assert 0.25 <= got_zero[on].mean() <= 0.75


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('B,L,tail,E,strided', SHAPES)
def test_dense_stacks_match_the_restatement(B, L, tail, E, strided, p):
    from asac_amd import native
    from algorithm.nn_models.layers.seq_layers import _QkvDenseDropFn
    counter = 3
    c = _case(B, L, tail, E, p, counter)
    leaf, x = _x_on_device(c, strided)
    params = [t.clone().cuda().requires_grad_(True) for t in c['params']]
    state, used = _state(counter)
    with native.LaunchProfiler() as prof:      # (every launch issued 20 times: the repetitions draw alike and count once)
        outs = _QkvDenseDropFn.apply(x, tail, (p, SEED, INSTANCE, state, used), *params)
        sum((o * g.cuda()).sum() for o, g in zip(outs, c['g_outs'])).backward()
    seen = prof.summary()
    assert seen['asac_rows_dense_proj_dropout_forward']['calls'] == 1
    assert seen['asac_rows_dense_proj_dropout_backward']['calls'] == 1
    assert int(used.item()) == counter and _state_is(state, counter + 1)
    got = {f'out_{n}': o.detach().cpu().numpy() for n, o in zip('qkv', outs)}
    got['grad_x'] = leaf.grad.cpu().numpy()[:, :, :E]
    for j, n in enumerate('qkv'):
        for i, kind in enumerate(('dW1', 'db1', 'dW2', 'db2')):
            got[f'{kind}_{n}'] = params[4 * j + i].grad.cpu().numpy()
    for name, a in got.items():
        _check(name.split('_')[0] if name.startswith('d') else name, a, c['want'][name], p, ref.param_rows(name, B, L, tail),
               f'{(B, L, tail, E)} {name}')
    if strided:
        assert float(leaf.grad[:, :, E:].abs().max()) == 0.


@functools.lru_cache(maxsize=None)
def _out_case(rows, E, p, counter):
    gen = torch.Generator().manual_seed(7 * rows + E)
    x, w, b = torch.randn(rows, E, generator=gen), torch.randn(E, E, generator=gen) * (2. / E) ** 0.5, torch.randn(E, generator=gen) * 0.1
    g = torch.randn(rows, E, generator=gen)
    sc = (torch.rand(rows, generator=gen) < 0.7).float()
    sc[0] = sc[rows - 1] = 0.
    kept = ref.rows_mask(SEED, INSTANCE, counter, ref.TAG_OUT, rows, E, p)
    want = {}
    for scaled in (False, True):
        xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
        y = ref.resblock(xd, wd, bd, kept, p, sc.double() if scaled else None)
        (y * g.double()).sum().backward()
        want[scaled] = dict(y=y.detach().numpy(), gx=xd.grad.numpy(), dW=wd.grad.numpy(), db=bd.grad.numpy())
    return dict(x=x, w=w, b=b, g=g, sc=sc, want=want)


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('rows,E', OUT_SHAPES)
def test_output_block_matches_the_restatement(rows, E, scaled, p):
    from asac_amd import native
    from algorithm.nn_models.layers.seq_layers import _OutResDropRowsFn
    counter = 4
    c = _out_case(rows, E, p, counter)
    x, w, b = (c[n].clone().cuda().requires_grad_(True) for n in 'xwb')
    state, used = _state(counter)
    with native.LaunchProfiler() as prof:
        y = _OutResDropRowsFn.apply(x, w, b, c['sc'].cuda() if scaled else None, (p, SEED, INSTANCE, state, used))
        (y * c['g'].cuda()).sum().backward()
    seen = prof.summary()
    assert seen['asac_rows_resblock_dropout_forward']['calls'] == 1 and seen['asac_rows_resblock_dropout_backward']['calls'] == 1
    assert int(used.item()) == counter and _state_is(state, counter + 1)
    got = dict(y=y, gx=x.grad, dW=w.grad, db=b.grad)
    for name, t in got.items():
        _check(name, t.detach().cpu().numpy(), c['want'][scaled][name], p, rows if name in ('dW', 'db') else None,
               f'output block {(rows, E)} scaled={scaled}')


# ---- the whole module ----------------------------------------------------------------------------------------------------
B_, L_, Q_, E_, H_ = 5, 9, 4, 64, 2


@functools.lru_cache(maxsize=None)
def _module_case(p):
    import asac_amd  # noqa: F401
    from algorithm.nn_models.layers.seq_layers import POSITIONAL_ENCODING
    layer = ref.make_layer(E_, H_, POSITIONAL_ENCODING.ROPE, p, seed=3)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(B_, L_, E_, generator=gen)
    am = torch.rand(B_, Q_, L_, generator=gen) < 0.4
    am[0, 0] = True                                                       # a dead row
    rz = torch.rand(B_, Q_, generator=gen) < 0.3                          # padded rows
    rz[1, 0] = True
    ki = (torch.arange(L_).unsqueeze(0) + torch.arange(B_).unsqueeze(1)).contiguous()
    g_out, g_w = torch.randn(B_, Q_, E_, generator=gen), torch.randn(B_, Q_, L_, generator=gen) * 0.2
    return layer, dict(x=x, am=am, rz=rz, ki=ki, g_out=g_out, g_w=g_w)


def _device_layer(layer, counter=0):
    return copy.deepcopy(layer).cuda().reseed(SEED, counter=counter, instance_id=INSTANCE)


def _on_device(c):
    return {n: c[n].cuda() for n in ('ki', 'am', 'rz', 'g_out', 'g_w')}


def _module_pass(dev, c, x=None, backward=True, d=None):
    """one pass of the device module over (x[:, -Q:], x, x) -> (out, weights, x); `d`: the other inputs on the device (a
    captured pass copies nothing)"""
    x = c['x'].clone().cuda().requires_grad_(True) if x is None else x
    d = _on_device(c) if d is None else d
    out, w = dev(x[:, -Q_:], x, x, query_index=d['ki'][:, -Q_:], key_index=d['ki'], attn_mask=d['am'], out_row_mask=d['rz'])
    if backward:
        for p_ in dev.parameters():
            p_.grad = None
        ((out * d['g_out']).sum() + (w * d['g_w']).sum()).backward()
    return out, w, x


def _module_restated(layer, c, counters, p):
    l64 = copy.deepcopy(layer).double()
    kept = ref.module_masks(SEED, INSTANCE, counters, B_, L_, Q_, E_, H_, p)
    x = c['x'].double().requires_grad_(True)
    out, w = ref.module_forward(l64, x, Q_, kept, p, c['ki'][:, -Q_:], c['ki'], c['am'], None, c['rz'])
    ((out * c['g_out'].double()).sum() + (w * c['g_w'].double()).sum()).backward()
    return dict(out=out.detach().numpy(), weights=w.detach().numpy(), grad_x=x.grad.numpy(),
                params=[p_.grad.numpy() for p_ in l64.parameters()])


def _counters(dev):
    return dev.dense_dropout_drawn('qkv'), dev.dropout_drawn(), dev.dense_dropout_drawn('out')


def _check_module(dev, got, want, p, label):
    out, w, x = got
    for name, a in (('out', out), ('weights', w), ('grad_x', x.grad)):
        if a is not None:
            _check(f'module_{name}', a.detach().cpu().numpy(), want[name], p, None, label)
    if x.grad is not None:
        for (n, p_), b in zip(dev.named_parameters(), want['params']):
            rows = B_ * Q_ if n.startswith(('q_proj', 'out_proj')) else B_ * L_
            _check('module_parameter_gradients', p_.grad.cpu().numpy(), b, p, rows, f'{label} {n}')


@pytest.mark.parametrize('p', [0.2, 0.5])
def test_whole_module_matches_the_restatement(p):
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers
    assert seq_layers.FUSED_DENSE_DROPOUT and seq_layers.FUSED_ATTN_DROPOUT
    layer, c = _module_case(p)
    dev = _device_layer(layer, counter=3)
    assert dev.dense_dropout_state('qkv') is None and dev.dense_dropout_state('out') is None
    with native.LaunchProfiler() as prof:
        got = _module_pass(dev, c)
    seen = prof.summary()
    for name in ('asac_rows_dense_proj_dropout', 'asac_rows_resblock_dropout', 'asac_attention_mh_dropout'):
        assert seen[name + '_forward']['calls'] == 1 and seen[name + '_backward']['calls'] == 1, name
    for name in ('asac_rows_resblock_forward', 'asac_rows_proj_forward', 'asac_rows_linear_forward'):
        assert name not in seen, name
    assert _counters(dev) == (3, 3, 3)
    assert dev.dense_dropout_state('qkv') == dev.dense_dropout_state('out') == dev.dropout_state() == (4, 0)
    assert set(dev.state_dict()) == set(layer.state_dict())
    _check_module(dev, got, _module_restated(layer, c, (3, 3, 3), p), p, 'whole module')
    # other counters are other masks, far away: the comparison can tell them apart
    other = _module_restated(layer, c, (4, 3, 3), p)
    assert np.abs(other['out'] - got[0].detach().cpu().numpy()).max() > 100 * 3e-5


def test_a_module_applied_twice_keeps_both_records():
    """observations and next observations: two forwards before either backward, counters c and c + 1 at every site, and each
    pass equals its own restatement"""
    p = 0.5
    layer, c = _module_case(p)
    dev = _device_layer(layer, counter=40)
    x1, x2 = (c['x'].clone().cuda().requires_grad_(True) for _ in range(2))
    o1, w1, _ = _module_pass(dev, c, x1, backward=False)
    first = _counters(dev)
    o2, w2, _ = _module_pass(dev, c, x2, backward=False)
    assert first == (40, 40, 40) and _counters(dev) == (41, 41, 41)
    g_out, g_w = c['g_out'].cuda(), c['g_w'].cuda()
    ((o1 * g_out).sum() + (w1 * g_w).sum() + (o2 * g_out).sum() + (w2 * g_w).sum()).backward()
    for n, (o, w, x) in ((40, (o1, w1, x1)), (41, (o2, w2, x2))):
        want = _module_restated(layer, c, (n, n, n), p)
        for name, a in (('out', o), ('weights', w), ('grad_x', x.grad)):
            _check(f'module_{name}', a.detach().cpu().numpy(), want[name], p, None, f'applied twice, counter {n}')


def test_switches(monkeypatch):
    from asac_amd import native
    from algorithm.nn_models.layers import seq_layers
    p = 0.5
    layer, c = _module_case(p)

    def run(dev, grad=True):
        with native.LaunchProfiler(repeat=1) as prof:
            if grad:
                out, w, _ = _module_pass(dev, c)
            else:
                with torch.no_grad():
                    out, w, _ = _module_pass(dev, c, backward=False)
        return out.detach(), w.detach(), prof.summary()

    def new_launches(seen):
        return [k for k in seen if 'rows_dense_proj_dropout' in k or 'rows_resblock_dropout' in k]

    evald = _device_layer(layer).eval()
    only_dropouts = _device_layer(layer)
    for mod in only_dropouts.modules():
        if isinstance(mod, nn.Dropout):
            mod.eval()
    only_dropouts.dropout = 0.      # (the weights' dropout is F.dropout on this attribute: switched off too, for the bit comparison)
    results = [run(evald), run(only_dropouts)]
    monkeypatch.setattr(seq_layers, 'FUSED_DENSE_DROPOUT', False)
    off = _device_layer(layer)
    out_off, _, seen_off = run(off)
    assert not new_launches(seen_off) and off.dense_dropout_state('qkv') is None and off.dense_dropout_state('out') is None
    assert 0.3 < float((out_off == 0).float().mean()) < 0.8, 'module code: ATen dropped about half of the output block'
    for mod in off.modules():
        if isinstance(mod, nn.Dropout):
            mod.eval()
    off.dropout = 0.
    results.append(run(off))
    monkeypatch.setattr(seq_layers, 'FUSED_DENSE_DROPOUT', True)
    for out, w, seen in results:
        assert not new_launches(seen)
        assert torch.equal(out, results[0][0]) and torch.equal(w, results[0][1]), 'the no-drop paths agree bit for bit'
    assert evald.dense_dropout_state('qkv') is None and only_dropouts.dense_dropout_state('out') is None
    # a CPU copy: module code
    cpu = copy.deepcopy(layer)
    with native.LaunchProfiler(repeat=1) as prof:
        out, _ = cpu(c['x'][:, -Q_:], c['x'], c['x'], query_index=c['ki'][:, -Q_:], key_index=c['ki'], attn_mask=c['am'],
                     out_row_mask=c['rz'])
    assert not prof.summary() and torch.isfinite(out).all() and cpu.dense_dropout_state('qkv') is None
    # acting: training mode under no_grad drops and advances
    dev = _device_layer(layer, counter=7)
    for n in range(2):
        out, w, seen = run(dev, grad=False)
        assert sorted(new_launches(seen)) == ['asac_rows_dense_proj_dropout_forward', 'asac_rows_resblock_dropout_forward']
        assert _counters(dev) == (7 + n,) * 3
        want = _module_restated(layer, c, (7 + n,) * 3, p)
        _check('module_out', out.cpu().numpy(), want['out'], p, None, f'no_grad, counter {7 + n}')
    assert dev.dense_dropout_state('qkv') == dev.dense_dropout_state('out') == (9, 0)


def test_captured_block_draws_afresh_on_every_replay():
    p = 0.5
    layer, c = _module_case(p)
    dev = _device_layer(layer, counter=0)
    x = c['x'].clone().cuda().requires_grad_(True)
    side = torch.cuda.Stream()
    kept, d = {}, _on_device(c)

    def step():
        x.grad = None
        out, w, _ = _module_pass(dev, c, x, d=d)
        kept['out'], kept['w'], kept['gx'] = out.detach(), w.detach(), x.grad

    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                  # warm-up: creates the three states (counters 0 -> 2)
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    offset = torch.cuda.get_rng_state().clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    first = dev.dense_dropout_state('qkv')[0]
    assert first == 2 == dev.dense_dropout_state('out')[0] == dev.dropout_state()[0], 'capturing launches nothing'
    outs = []
    for n in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert _counters(dev) == (first + n,) * 3
        want = _module_restated(layer, c, (first + n,) * 3, p)
        for name, key in (('out', 'out'), ('weights', 'w'), ('grad_x', 'gx')):
            _check(f'module_{name}', kept[key].cpu().numpy(), want[name], p, None, f'replay {n}')
        outs.append(kept['out'].cpu().numpy())
    assert dev.dense_dropout_state('qkv') == dev.dense_dropout_state('out') == dev.dropout_state() == (first + 3, 0)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    assert torch.equal(torch.cuda.get_rng_state(), offset), 'the block draws nothing from the device generator'


def test_first_call_under_capture_runs_the_module_code():
    p = 0.5
    layer, c = _module_case(p)
    dev = copy.deepcopy(layer).cuda()
    x, d = c['x'].cuda(), _on_device(c)
    res = {}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # allocating and seeding a state are not part of a capture
        with torch.no_grad():
            res['out'] = _module_pass(dev, c, x, backward=False, d=d)[0]
    graph.replay()
    torch.cuda.synchronize()
    assert dev.dense_dropout_state('qkv') is None and dev.dense_dropout_state('out') is None and dev.dropout_state() is None
    assert torch.isfinite(res['out']).all()


def test_same_seed_counter_and_instance_give_the_same_bits():
    p = 0.5
    layer, c = _module_case(p)
    dev = _device_layer(layer, counter=11)
    a = [t.detach().cpu().numpy() for t in _module_pass(dev, c)[:2]]
    dev.reseed(SEED, counter=11, instance_id=INSTANCE)
    again = _module_pass(dev, c)
    assert _counters(dev) == (11, 11, 11)
    assert all(np.array_equal(u, t.detach().cpu().numpy()) for u, t in zip(a, again[:2]))
    dev.reseed(SEED + 1, counter=11, instance_id=INSTANCE)
    assert not np.array_equal(a[0], _module_pass(dev, c)[0].detach().cpu().numpy())
