"""GPU: the head-bank kernels (`csrc/head_bank.hip`) and their autograd glue (`algorithm/fused_heads.py`): every output
against float64 (`tests/head_bank_ref.py`) and against the float32 composition of torch operators on the same parameters,
on parameter tables that are views of one flat buffer (misaligned behind every narrow head bias); overwrite / accumulate;
equal bits; the refused arguments; `HeadBank` in its two gradient-delivery modes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import head_bank_ref as hr  # noqa: E402
from tests.discrete_ref import GUARD, SENTINEL, over_the_bound  # noqa: E402

# (S, W, depth, sizes, G): the stock default; the reference plugins' width; a residual first block; S at the two-half
# boundary, one block, three groups; an odd S, three branches, the group limit; a single 64-logit head behind one block;
# and the widths served on zero-padded tiles: the fixtures' 32 (with a residual first block), 96 on the 128-wide tile
SHAPES = [(6, 64, 3, (3, 2), 2), (6, 128, 2, (3, 2), 2), (64, 64, 3, (4,), 1), (128, 128, 1, (17,), 3),
          (61, 128, 2, (3, 2, 5), 8), (8, 64, 1, (64,), 1), (32, 32, 2, (3, 2), 3), (6, 96, 2, (3, 2), 2)]
ROWS = [1, 15, 16, 17, 300]      # one row; a tile edge from both sides; several tiles (an ordered sum of 19 addends)
INVALID = 1                      # hipErrorInvalidValue


def _guarded(*shape, fill=float('nan')):
    """a `fill`ed contiguous tensor inside a larger buffer with GUARD sentinels on both sides -> (view, whole buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device='cuda')
    view = whole[GUARD:GUARD + n]
    view.fill_(fill)
    return view.view(*shape), whole


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all() and (whole[-GUARD:] == SENTINEL).all())


class _Case:
    def __init__(self, S, W, depth, sizes, G, N, seed, window=False):
        from asac_amd import native
        self.S, self.W, self.depth, self.sizes, self.G, self.N = S, W, depth, sizes, G, N
        self.D, self.residual = sum(sizes), hr.residual_flags(S, W, depth)
        flat, self.layout = hr.make_params(S, W, depth, sizes, G, seed)
        self.flat = torch.from_numpy(flat).cuda()
        self.stacks = hr.views_of(self.flat, self.layout)
        rng = np.random.default_rng(seed + 1)
        if window:       # [260, 5, S] sliced [:, 1:] out of a larger tensor: rows read in place
            big = torch.from_numpy(rng.standard_normal((N // 5, 6, S + 3)).astype(np.float32)).cuda()
            self.x = big[:, 1:, :S]
            assert not self.x.is_contiguous() and self.x.shape == (N // 5, 5, S)
        else:
            self.x = torch.from_numpy(rng.standard_normal((N, S)).astype(np.float32)).cuda()
        self.grad_out = torch.from_numpy(rng.standard_normal((G, N, self.D)).astype(np.float32)).cuda()
        self.desc = native.head_bank_desc(S, W, self.residual, sizes, G)
        self.table = native.head_bank_table(self.stacks)

    def grad_buffer(self, fill=float('nan')):
        """a gradient buffer with the parameters' layout (views, table, whole guarded buffer)"""
        from asac_amd import native
        g, whole = _guarded(self.flat.numel(), fill=fill)
        views = hr.views_of(g, self.layout)
        return g, views, native.head_bank_table(views), whole

    def covered(self):
        """mask of the floats of the flat layout that belong to a parameter (the rest is segment padding)"""
        m = torch.zeros(self.flat.numel(), dtype=torch.bool)
        for views in self.layout:
            for off, shape in views:
                m[off:off + int(np.prod(shape))] = True
        return m.cuda()


def _run_case(c, tag):
    from asac_amd import native
    x64 = c.x.reshape(c.N, c.S).double().cpu().numpy()
    p64 = [[t.double().cpu().numpy() for t in st] for st in c.stacks]
    want = {'out': hr.bank_forward(x64, p64, c.residual, c.sizes, c.G)}
    g64, gx64 = hr.bank_backward(x64, p64, c.residual, c.sizes, c.G, c.grad_out.double().cpu().numpy())
    want['grad_x'] = gx64
    for m, gs in enumerate(g64):
        for i, g in enumerate(gs):
            want[f'grad_{m}_{i}'] = g

    out, out_whole = _guarded(c.G, c.N, c.D)
    gx, gx_whole = _guarded(c.N, c.S)
    gflat, gviews, gtable, g_whole = c.grad_buffer()
    native.head_bank_forward(c.desc, c.table, c.x, out)
    native.head_bank_backward(c.desc, c.table, gtable, c.x, c.grad_out, grad_x=gx, accumulate=False)
    torch.cuda.synchronize()
    assert _guards_intact(out_whole) and _guards_intact(gx_whole) and _guards_intact(g_whole), 'a store outside its tensor'
    assert bool(torch.isnan(gflat[~c.covered()]).all()), 'segment padding was written'
    kernel = {'out': out, 'grad_x': gx}
    for m, gs in enumerate(gviews):
        for i, g in enumerate(gs):
            kernel[f'grad_{m}_{i}'] = g

    xe = c.x.detach().clone().requires_grad_(True)
    leaves = [[t.detach().clone().requires_grad_(True) for t in st] for st in c.stacks]
    oe = hr.torch_composition(xe.reshape(c.N, c.S), leaves, c.residual, c.sizes, c.G)
    ge = torch.autograd.grad(oe, [xe] + [t for st in leaves for t in st], c.grad_out)
    eager = {'out': oe.detach(), 'grad_x': ge[0].reshape(c.N, c.S)}
    it = iter(ge[1:])
    for m, st in enumerate(leaves):
        for i in range(len(st)):
            eager[f'grad_{m}_{i}'] = next(it)
    as64 = lambda d: {k: v.double().cpu().numpy() for k, v in d.items()}       # noqa: E731
    return over_the_bound(tag, want, as64(kernel), as64(eager))


@pytest.mark.parametrize('N', ROWS)
@pytest.mark.parametrize('S,W,depth,sizes,G', SHAPES)
def test_kernels_against_float64_and_the_module_composition(S, W, depth, sizes, G, N):
    """`out`, every parameter gradient and `grad_x` of the two entry points, outputs pre-filled with NaN inside guarded
    buffers, parameters and gradient views laid out as `FlatParamGroup` lays them out.  Bound (the rule of
    tests/test_dqn_gpu.py): per tensor the kernel's largest absolute error against float64 may be at most twice that of the
    float32 composition of torch operators on the same parameters (autograd), floor 4 units in the last place at the
    tensor's largest magnitude.  Nothing outside a tensor and no segment padding may be written.
    Observed on MI355X: NOTES.md, "Discrete-nets round" (the largest share of the bound over the cases, and the two
    earlier forms of the kernels that missed it: float32 row sums in launch 2, and the Abramowitz-Stegun erf)."""
    import asac_amd  # noqa: F401
    c = _Case(S, W, depth, sizes, G, N, seed=S + W + depth + N)
    if sizes in ((3, 2), (3, 2, 5)):
        assert any(t.data_ptr() % 16 for st in c.stacks for t in st), 'the case is meant to be misaligned'
    bad, share = _run_case(c, f'{(S, W, depth, sizes, G)} N {N}')
    print(f'{(S, W, depth, sizes, G)} N {N}: largest share of the bound {share:.2f}')
    assert not bad, bad


def test_a_window_view_is_read_in_place():
    """N = 1 300 rows, x a [260, 5, S] window sliced [:, 1:] out of a larger tensor (separate sample and step strides)"""
    import asac_amd  # noqa: F401
    c = _Case(6, 128, 2, (3, 2), 2, 1300, seed=5, window=True)
    bad, share = _run_case(c, 'window')
    print(f'window: largest share of the bound {share:.2f}')
    assert not bad, bad


@pytest.mark.parametrize('S,W,depth,sizes,G,N', [(6, 64, 3, (3, 2), 2, 300), (61, 128, 2, (3, 2, 5), 8, 17)])
def test_overwrite_accumulate_and_equal_bits(S, W, depth, sizes, G, N):
    """accumulate adds exactly the overwrite result to what the views hold (the bits of `pre + overwrite` in float32); two
    launches on equal inputs give equal bits, `grad_x` (an ordered sum over the stacks) included"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    c = _Case(S, W, depth, sizes, G, N, seed=11)
    ws = native.head_bank_backward_workspace('cuda', N, c.desc)
    runs = []
    for _ in range(2):
        gflat, _, gtable, _ = c.grad_buffer()
        gx = torch.full((N, S), float('nan'), device='cuda')
        native.head_bank_backward(c.desc, c.table, gtable, c.x, c.grad_out, grad_x=gx, accumulate=False, workspace=ws)
        runs.append((gflat.clone(), gx.clone()))
    cov = c.covered()
    assert torch.equal(runs[0][0][cov], runs[1][0][cov]) and torch.equal(runs[0][1], runs[1][1])
    pre = torch.from_numpy(np.random.default_rng(3).standard_normal(c.flat.numel()).astype(np.float32)).cuda()
    gflat, _, gtable, _ = c.grad_buffer()
    gflat.copy_(pre)
    native.head_bank_backward(c.desc, c.table, gtable, c.x, c.grad_out, grad_x=None, accumulate=True, workspace=ws)
    assert torch.equal(gflat[cov], (pre + runs[0][0])[cov])
    assert torch.equal(gflat[~cov], pre[~cov])
    out = [torch.full((G, N, c.D), float('nan'), device='cuda') for _ in range(2)]
    for o in out:
        native.head_bank_forward(c.desc, c.table, c.x, o)
    assert torch.equal(out[0], out[1])


def test_refused_arguments_launch_nothing():
    """every bad argument returns hipErrorInvalidValue and leaves sentinel-filled outputs alone; N == 0 is accepted and
    writes nothing"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    lib = native.load()
    c = _Case(6, 64, 2, (3, 2), 2, 5, seed=1)
    out = torch.full((c.G, c.N, c.D), SENTINEL, device='cuda')
    gx = torch.full((c.N, c.S), SENTINEL, device='cuda')
    gflat, _, gtable, _ = c.grad_buffer(fill=SENTINEL)
    ws = native.head_bank_backward_workspace('cuda', c.N, c.desc)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731

    def desc(**kw):
        a = dict(S=c.S, W=c.W, residual=c.residual, sizes=c.sizes, G=c.G)
        a.update(kw)
        return native.head_bank_desc(a['S'], a['W'], a['residual'], a['sizes'], a['G'])

    def fwd(d=c.desc, params=c.table, x=c.x, samples=c.N, steps=1, o=out):
        return lib.asac_head_bank_forward(C.byref(d) if d is not None else None, p(params), p(x), c.S, c.S, samples, steps,
                                          p(o), None)

    def bwd(d=c.desc, params=c.table, grads=gtable, x=c.x, samples=c.N, steps=1, go=c.grad_out, g_x=gx, w=ws):
        return lib.asac_head_bank_backward(C.byref(d) if d is not None else None, p(params), p(grads), p(x), c.S, c.S,
                                           samples, steps, p(go), p(g_x), 0, p(w), None)

    off_sum = desc()
    off_sum.branches.D = c.D + 1
    bad_flag = desc()
    bad_flag.residual[1] = 2
    bad_descs = {'W 0': desc(W=0), 'W 129': desc(W=129), 'S 0': desc(S=0), 'S 129': desc(S=129),
                 'depth 0': desc(residual=()), 'depth 4': desc(residual=(False,) * 4),
                 'K 9': desc(sizes=(2,) * 9), 'D 65': desc(sizes=(33, 32)), 'G 0': desc(G=0), 'G 9': desc(G=9),
                 'residual[0] at S != W': desc(residual=(True, True)), 'a branch of 0': desc(sizes=(5, 0)),
                 'a table that does not add up': off_sum, 'a flag of 2': bad_flag}
    bad_descs['depth 4'].depth = 4
    for name, d in bad_descs.items():
        assert fwd(d=d) == INVALID, name
        assert bwd(d=d) == INVALID, name
    for name, kw in {'desc': dict(d=None), 'params': dict(params=None), 'x': dict(x=None), 'out': dict(o=None),
                     'rows': dict(samples=(1 << 20) + 1), 'negative rows': dict(samples=-1), 'steps 0': dict(steps=0)}.items():
        assert fwd(**kw) == INVALID, name
    for name, kw in {'desc': dict(d=None), 'params': dict(params=None), 'x': dict(x=None), 'grad_out': dict(go=None),
                     'workspace': dict(w=None), 'neither grads nor grad_x': dict(grads=None, g_x=None),
                     'rows': dict(samples=(1 << 20) + 1), 'steps 0': dict(steps=0)}.items():
        assert bwd(**kw) == INVALID, name
    assert fwd(samples=0) == 0 and bwd(samples=0) == 0
    assert lib.asac_head_bank_backward_workspace(0, 6, 64, 2, 5, 4) == -1
    assert lib.asac_head_bank_backward_workspace((1 << 20) + 1, 6, 64, 2, 5, 4) == -1
    assert lib.asac_head_bank_backward_workspace(5, 6, 129, 2, 5, 4) == -1
    torch.cuda.synchronize()
    for t in (out, gx, gflat):
        assert bool((t == SENTINEL).all())
    assert bool((ws == 0).all())


def _bank_of_modules(S, W, depth, sizes, seed=0):
    """a stock-shaped list of `LinearLayers` whose parameters are views of one flat buffer with `.grad` views of another
    (a learner's `FlatParamGroup`, by hand) -> (modules, HeadBank, flat gradient buffer)"""
    from algorithm import fused_heads
    from algorithm.fused import FlatParamGroup
    from algorithm.nn_models.layers import LinearLayers
    torch.manual_seed(seed)
    mods = torch.nn.ModuleList([LinearLayers(S, W, depth, s) for s in sizes]).cuda()
    for p in mods.parameters():
        if p.dim() == 1:
            p.data.uniform_(-0.3, 0.3)
    group = FlatParamGroup([('q_0', list(mods.parameters()))], 'cuda', with_grad=True)
    shape = fused_heads.describe_head_bank([mods])
    assert shape is not None
    return mods, fused_heads.HeadBank(shape), group


def _module_out(mods, x):
    return torch.cat([m.dense(x) for m in mods], dim=-1)


def _float64(mods, x, go, scale=1.):
    """float64 gradients of the modules' composition (tests/head_bank_ref.py) -> ({id(parameter): gradient}, grad_x, out)"""
    sizes = [m.dense[-1].out_features for m in mods]
    depth = (len(mods[0].dense) - 1) // 2
    residual = hr.residual_flags(x.shape[-1], mods[0].dense[0].linear.out_features, depth)
    stacks = [[q.detach().double().cpu().numpy() for q in m.parameters()] for m in mods]
    x64 = x.detach().double().cpu().numpy()
    grads, gx = hr.bank_backward(x64, stacks, residual, sizes, 1, go.double().cpu().numpy()[None])
    table = {id(q): scale * g for m, gs in zip(mods, grads) for q, g in zip(m.parameters(), gs)}
    return table, scale * gx, hr.bank_forward(x64, stacks, residual, sizes, 1)[0]


def _hold(tag, want, got, eager):
    """the kernel bound of this file on {name: tensor | array}: against float64, at most twice the module code's error"""
    as64 = lambda d: {k: (v.detach().double().cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}   # noqa: E731
    bad, _ = over_the_bound(tag, as64(want), as64(got), as64(eager))
    assert not bad, bad


def test_head_bank_default_mode_returns_gradients_to_autograd():
    """`autograd.grad` with respect to a subset of the parameters and to x: what the module code returns"""
    import asac_amd  # noqa: F401
    mods, bank, _ = _bank_of_modules(6, 64, 3, (3, 2))
    x = torch.randn(17, 6, device='cuda', requires_grad=True)
    go = torch.randn(17, 5, device='cuda')
    some = [mods[0].dense[0].linear.weight, mods[1].dense[6].bias, mods[1].dense[2].linear.weight]
    got = torch.autograd.grad(bank(x)[0], [x] + some, go)
    eager = torch.autograd.grad(_module_out(mods, x), [x] + some, go)
    table, gx64, out64 = _float64(mods, x, go)
    names = ['x'] + [f'p{i}' for i in range(len(some))]
    want = dict(zip(names, [gx64] + [table[id(q)] for q in some]))
    with torch.no_grad():
        assert bank(x.detach()).shape == (1, 17, 5)
        want['out'] = out64
        _hold('default', want, dict(zip(names, got), out=bank(x.detach())[0]),
              dict(zip(names, eager), out=_module_out(mods, x.detach())))


def test_head_bank_direct_mode_adds_into_the_grad_views():
    """inside `direct_param_grads()` two backward passes leave their sum in the `.grad` views and hand autograd nothing;
    with `only=` the parameters outside the set are left alone"""
    import asac_amd  # noqa: F401
    from algorithm.param_grads import direct_param_grads
    mods, bank, group = _bank_of_modules(6, 128, 2, (3, 2, 5), seed=1)
    params = list(mods.parameters())
    x = torch.randn(33, 6, device='cuda')
    go = torch.randn(33, 10, device='cuda')
    eager = torch.autograd.grad(_module_out(mods, x), params, go)
    names = [f'p{i}' for i in range(len(params))]
    twice, _, _ = _float64(mods, x, go, scale=2.)
    group.grad.zero_()
    with direct_param_grads():
        for _ in range(2):
            bank(x)[0].backward(go)
    lo, hi = group.grad.data_ptr(), group.grad.data_ptr() + 4 * group.grad.numel()
    assert all(lo <= p.grad.data_ptr() < hi for p in params), 'the gradients are the views of the flat buffer'
    _hold('direct, two passes', {n: twice[id(p)] for n, p in zip(names, params)}, {n: p.grad for n, p in zip(names, params)},
          {n: 2 * g for n, g in zip(names, eager)})
    group.grad.zero_()
    only = [params[0], params[-1]]
    once, _, _ = _float64(mods, x, go)
    with direct_param_grads(only=only):
        bank(x)[0].backward(go, inputs=only)
    inside = {n: p for n, p in zip(names, params) if any(p is q for q in only)}
    assert len(inside) == 2
    _hold('direct, only', {n: once[id(p)] for n, p in inside.items()}, {n: p.grad for n, p in inside.items()},
          {n: g for n, g in zip(names, eager) if n in inside})
    for n, p in zip(names, params):
        assert n in inside or bool((p.grad == 0).all()), n
