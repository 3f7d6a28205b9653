"""GPU: ONE fused module reached TWICE in one backward pass, in the learner's mode — `direct_param_grads()` (the backward
launches ADD the parameter gradients into the `.grad` views of the flat buffer) inside `DeferredPartialSums()` (their second
launches, the fixed-order sums of the per-workgroup partials, wait and run sixteen to a launch).  A shared encoder applied to
two cameras, a head applied to two inputs: both uses queue a sum into the SAME span of the gradient buffer, the jobs of one
`asac_sum_partials_multi` launch run side by side, and `out[i] = out[i] + s` from two of them at once loses one.  The two sums
therefore have to leave in two launches, in the order queued.

Per producer of such jobs (dense stack with the sequential and with the sliced reduction, attention projection block, conv2
and conv1d stack, Linear + Tanh head), with  loss = (mod(x1) * c1).sum() + 2 (mod(x2) * c2).sum():

(a) direct mode without deferral — the stream-ordered reductions — gives the wanted BITS;
(b) with deferral nothing is written before `flush()` and afterwards the buffer holds exactly those bits: each job keeps the
    slab and slice order of the launch it stands for, and jobs on one output are applied in the order queued, so both paths form
    (start + s1) + s2;
(c) the float64 arbiter: the gradient that arrived, `grad - start`, against a float64 copy of the UNFUSED module on the CPU with
    plain autograd.  Yardstick (as tests/test_fused_conv1d_gpu.py): err(a) = max|a - ref64| / max|ref64|;
    e_mod the larger err of the f32 unfused module on the device and on the CPU; err <= max(4 e_mod, sqrt(n) 2^-24), n the
    gradient's reduction length over both uses.  A lost contribution is an error of order 1.
    The attention block's key bias is the one exception in scale: softmax does not see a shift common to all keys of a query,
    so its gradient is identically zero and max|ref64| is float64 rounding noise, not a scale.  Its errors are measured
    against max|ref64| of the key WEIGHT gradient instead — the same rows of d loss / d k summed, against x instead of 1;
(d) a module used twice costs exactly 2 `asac_sum_partials_multi` launches, three times 3; modules used once ride in the first.

The second half covers `fused_conv.DeferredConvBackward.flush()` inside an active `DeferredPartialSums` (sac_aux._train_rpm's
order of calls) with one conv stack behind two forward passes: the sum over the passes may not be formed before the slab sums
have written its terms."""
import copy
import functools
import math

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

KINDS = ['dense_sequential', 'dense_sliced', 'attention', 'conv2', 'conv1d', 'linear_tanh']
CONV1D_SEED = 0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sliced_rows():
    """the smallest N whose dense backward leaves >= 64 row tiles: the sliced (16 slices) reduction"""
    from asac_amd import native
    n = 1
    while native.mlp_backward_tiles(n, 1) < 64:
        n += 1
    assert native.mlp_backward_tiles(300, 1) < 64          # (the other use of the stack keeps the sequential reduction)
    return n


def _attn_plain(mod, key):
    """`MultiheadAttention(E, 1, out_dense_depth=1)(key, key, key)[0]` in plain tensor operations (on the device the module
    itself takes fused launches at every size): pinned to the module in float64 on the CPU by `_reference`"""
    q, k, v = mod.q_proj.dense[0](key), mod.k_proj.dense[0](key), mod.v_proj.dense[0](key)
    w = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(mod.embed_dim), dim=-1)
    o = w @ v
    block = mod.out_proj.dense[0]
    return nn.functional.gelu(block.linear(o)) + o


class _Case:
    """ref: the unfused module on the CPU (f32); xs: the inputs, one per use; plain(mod, x): the unfused forward of a copy of
    `ref` in any dtype on any device; n_of(name, rows): reduction length of parameter `name`'s gradient; backward: the entry
    point whose second launch is deferred"""

    def __init__(self, kind, uses=2):
        import algorithm.nn_models as m
        self.kind, g = kind, _gen(7)
        torch.manual_seed(3)
        if kind.startswith('dense'):
            self.ref = m.LinearLayers(40, [64], 1, 8)
            rows = {'dense_sequential': [300, 77, 41], 'dense_sliced': [_sliced_rows(), 300, 41]}[kind][:uses]
            self.xs = [torch.randn(r, 40, generator=g) for r in rows]
            self.plain = lambda mod, x: mod(x)
            self.n_of = lambda name: sum(rows)
            self.backward = 'asac_mlp_backward'
        elif kind == 'attention':
            self.ref = m.MultiheadAttention(8, 1, out_dense_depth=1)
            with torch.no_grad():
                for p in self.ref.parameters():
                    if p.dim() == 1:
                        p.normal_(0, 0.3, generator=g)       # (biases start at zero: give them something to do)
            self.xs = [torch.randn(b, 9, 8, generator=g) for b in (33, 7)]
            self.plain = _attn_plain
            self.n_of = lambda name: (33 + 7) * 9
            self.backward = 'asac_attention_proj_backward'
        elif kind == 'conv2':
            self.ref = nn.Sequential(nn.Conv2d(3, 16, 8, 4), nn.GELU(), nn.Conv2d(16, 32, 4, 2), nn.GELU())
            self.xs = [torch.randn(n, 3, 30, 30, generator=g) for n in (40, 9)]
            self.plain = lambda mod, x: mod(x).reshape(x.shape[0], -1)
            self.n_of = lambda name: (40 + 9) * (36 if name.startswith('0.') else 4)       # frames x map positions
            self.backward = 'asac_conv2_backward'
        elif kind == 'conv1d':
            torch.manual_seed(CONV1D_SEED)
            self.ref = nn.Sequential(nn.Conv1d(2, 16, 8, 4), nn.LeakyReLU(), nn.Conv1d(16, 32, 4, 2), nn.LeakyReLU())
            self.xs = [torch.randn(n, 61, 2, generator=_gen(CONV1D_SEED + 1000 + j)) for j, n in enumerate((37, 5))]
            self.plain = lambda mod, x: mod(x.permute(0, 2, 1)).reshape(x.shape[0], -1)
            self.n_of = lambda name: (37 + 5) * (14 if name.startswith('0.') else 6)       # rays x output positions
            self.backward = 'asac_conv1_backward'
        elif kind == 'linear_tanh':
            self.ref = nn.Sequential(nn.Linear(18, 8), nn.Tanh())
            self.xs = [torch.randn(r, 18, generator=g) for r in (300, 65)]
            self.plain = lambda mod, x: mod(x)
            self.n_of = lambda name: 300 + 65
            self.backward = 'asac_linear_tanh_backward2'
        else:
            raise KeyError(kind)
        with torch.no_grad():
            shapes = [self.plain(self.ref, x).shape for x in self.xs]
        self.cots = [torch.randn(s, generator=g) for s in shapes]
        self.scales = [1.0, 2.0, 3.0][:len(self.xs)]

    def device_module(self):
        """-> (the fused module on the device, its parameters — to be put in a FlatParamGroup BEFORE `arm()` —, arm, apply)"""
        from algorithm.fused_conv import conv1d_stack_desc, conv_stack_desc, fused_conv1d_stack, fused_conv_stack
        from algorithm.fused_linear import fuse_linear_tanh_heads
        dev = copy.deepcopy(self.ref).cuda()
        holder = nn.ModuleList([dev])

        def arm():
            if self.kind.startswith('dense'):
                dev.fuse = True
            elif self.kind == 'linear_tanh':
                assert fuse_linear_tanh_heads(holder) == 1

        apply = dev
        if self.kind == 'attention':
            apply = lambda x: dev(x[:, -x.shape[1]:], x, x)[0]      # noqa: E731
        elif self.kind == 'conv2':
            apply = lambda x: fused_conv_stack(x, conv_stack_desc(dev, x), dev)      # noqa: E731
        elif self.kind == 'conv1d':
            apply = lambda x: fused_conv1d_stack(x, conv1d_stack_desc(dev, x), dev)      # noqa: E731
        return dev, list(dev.parameters()), arm, apply


def _module_grads(case, mod, device, dtype):
    """{name: gradient (float64, CPU)} of the case's loss through the unfused `mod` with plain autograd"""
    mod.zero_grad(set_to_none=True)
    loss = 0.
    for x, c, s in zip(case.xs, case.cots, case.scales):
        loss = loss + s * (case.plain(mod, x.to(device, dtype)) * c.to(device, dtype)).sum()
    loss.backward()
    return {name: p.grad.detach().double().cpu() for name, p in mod.named_parameters()}


def _scale_name(case, name):
    """the parameter whose float64 gradient sets the scale of `name`'s errors: itself, but for the identically-zero one"""
    return 'k_proj.dense.0.weight' if (case.kind == 'attention' and name == 'k_proj.dense.0.bias') else name


def _errs(case, got, want):
    return {name: float((got[name] - want[name]).abs().max() / want[_scale_name(case, name)].abs().max()) for name in want}


@functools.lru_cache(maxsize=None)
def _reference(kind, uses):
    """-> (case, float64 gradients, e_mod per parameter); the float64 arbiter and the unfused f32 runs, once per kind"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    case = _Case(kind, uses)
    ref64 = copy.deepcopy(case.ref).double()
    if kind == 'attention':
        with torch.no_grad():
            for x in case.xs:
                assert torch.allclose(_attn_plain(ref64, x.double()), ref64(x.double(), x.double(), x.double())[0],
                                      rtol=1e-12, atol=1e-13), 'the plain form is not the module'
    if kind == 'conv1d':
        # LeakyReLU has a kink: a pre-activation closer to zero than f32 rounding takes the other slope in f32 and moves a
        # gradient by a whole term — a condition on the inputs (seed), as in tests/test_fused_conv1d_gpu.py
        with torch.no_grad():
            for x in case.xs:
                z1 = ref64[0](x.double().permute(0, 2, 1))
                z2 = ref64[2](ref64[1](z1))
                min_z = min(float(z1.abs().min()), float(z2.abs().min()))
                assert min_z > 1e-6, f'a pre-activation within 1e-6 of the LeakyReLU kink ({min_z:.3g}): pick the next seed'
    want = _module_grads(case, ref64, 'cpu', torch.float64)
    cpu32 = _module_grads(case, copy.deepcopy(case.ref), 'cpu', torch.float32)
    with native.LaunchProfiler(repeat=1) as prof:
        dev32 = _module_grads(case, copy.deepcopy(case.ref).cuda(), 'cuda', torch.float32)
    assert not prof.summary(), 'the unfused module took a fused launch on the device'
    e_cpu, e_dev = _errs(case, cpu32, want), _errs(case, dev32, want)
    return case, want, {name: max(e_cpu[name], e_dev[name]) for name in want}


@functools.lru_cache(maxsize=None)
def _run(kind, uses):
    """steps (a), (b), (d) on the device, once per kind -> what the tests assert on"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_mlp import DeferredPartialSums, direct_param_grads
    case = _reference(kind, uses)[0]
    dev, params, arm, apply = case.device_module()
    group = FlatParamGroup([(kind, params)], 'cuda')
    arm()
    xs, cots = [x.cuda() for x in case.xs], [c.cuda() for c in case.cots]

    def loss():
        total = 0.
        for x, c, s in zip(xs, cots, case.scales):
            total = total + s * (apply(x) * c).sum()
        return total

    torch.manual_seed(11)
    group.grad.normal_()                  # (the launches ADD: something to add to)
    start = group.grad.clone()
    with native.LaunchProfiler(repeat=1) as prof:
        with direct_param_grads():
            loss().backward()
    plain_launches = prof.summary()
    want_bits = group.grad.clone()
    group.grad.copy_(start)
    with native.LaunchProfiler(repeat=1) as prof:
        with direct_param_grads(), DeferredPartialSums() as later:
            loss().backward()
        mid = group.grad.clone()
        late = later.flush()
    seen = prof.summary()
    base = group.grad.storage_offset()
    delta = group.grad.double() - start.double()         # (exact: what the additions left, rounding of the additions included)
    got = {}
    for name, p in dev.named_parameters():
        off = p.grad.storage_offset() - base
        got[name] = delta[off:off + p.numel()].view(p.shape).cpu()
    return dict(case=case, start=start, want_bits=want_bits, mid=mid, after=group.grad.clone(), got=got, late=late,
                plain_launches=plain_launches, seen=seen)


@pytest.mark.parametrize('kind', KINDS)
def test_a_module_used_twice_gets_the_bits_of_the_stream_ordered_sums(kind):
    """(a) against (b)"""
    r = _run(kind, 2)
    uses = len(r['case'].xs)
    assert r['plain_launches'][r['case'].backward]['calls'] == uses and 'asac_sum_partials_multi' not in r['plain_launches']
    assert not torch.equal(r['want_bits'], r['start'])
    assert r['seen'][r['case'].backward]['calls'] == uses
    assert r['late'] == {}          # (direct mode: nothing is handed back)
    assert torch.equal(r['mid'], r['start']), 'a deferred backward wrote parameter gradients before the flush'
    differ = int((r['after'] != r['want_bits']).sum())
    assert torch.equal(r['after'], r['want_bits']), f'{differ} of {r["after"].numel()} gradient floats differ'


@pytest.mark.parametrize('kind', KINDS)
def test_a_module_used_twice_gets_both_contributions_by_the_float64_modules(kind):
    """(c)"""
    case, want, e_mod = _reference(kind, 2)
    r = _run(kind, 2)
    err = _errs(case, r['got'], want)
    figures, failed = {}, []
    for name in want:
        assert r['got'][name].shape == want[name].shape and torch.isfinite(r['got'][name]).all(), name
        bound = max(4.0 * e_mod[name], math.sqrt(case.n_of(name)) * 2.0 ** -24)
        figures[name] = (err[name], e_mod[name], bound)
        if not err[name] <= bound:
            failed.append(name)
    print('shared', kind, {k: '%.3g / e_mod %.3g / bound %.3g' % v for k, v in figures.items()})
    assert not failed, (failed, figures)


@pytest.mark.parametrize('kind', KINDS)
def test_a_module_used_twice_costs_two_sum_launches(kind):
    """(d)"""
    seen = _run(kind, 2)['seen']
    print('shared', kind, 'asac_sum_partials_multi launches:', seen['asac_sum_partials_multi']['calls'])
    assert seen['asac_sum_partials_multi']['calls'] == 2


def test_a_dense_stack_used_three_times_costs_three_sum_launches_and_keeps_the_bits():
    r = _run('dense_sequential', 3)
    print('shared dense x3 asac_sum_partials_multi launches:', r['seen']['asac_sum_partials_multi']['calls'])
    assert r['seen']['asac_mlp_backward']['calls'] == 3 and r['seen']['asac_sum_partials_multi']['calls'] == 3
    assert torch.equal(r['mid'], r['start']) and torch.equal(r['after'], r['want_bits'])


def test_modules_used_once_ride_in_the_first_of_the_two_launches(monkeypatch):
    """the dense stack twice, the attention block and the Linear + Tanh head once each, in one backward: the once-used modules'
    sums leave with the first use of the stack, its second use alone behind them — and the bits are the undeferred ones"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused import FlatParamGroup
    from algorithm.fused_mlp import DeferredPartialSums, direct_param_grads
    cases = [_reference(k, 2)[0] for k in ('dense_sequential', 'attention', 'linear_tanh')]
    built = [c.device_module() for c in cases]
    group = FlatParamGroup([(c.kind, b[1]) for c, b in zip(cases, built)], 'cuda')
    for b in built:
        b[2]()
    data = [([x.cuda() for x in c.xs], [t.cuda() for t in c.cots]) for c in cases]

    def loss():
        # (the stack's two uses first: the backward reaches the nodes in reverse, the once-used modules' sums are queued
        # in front of the stack's)
        total = 0.
        for (xs, cots), b, uses in zip(data, built, (2, 1, 1)):
            for x, c, s in list(zip(xs, cots, (1.0, 2.0)))[:uses]:
                total = total + s * (b[3](x) * c).sum()
        return total

    torch.manual_seed(11)
    group.grad.normal_()
    start = group.grad.clone()
    with direct_param_grads():
        loss().backward()
    want_bits = group.grad.clone()
    assert not torch.equal(want_bits, start)
    group.grad.copy_(start)
    sizes, launch = [], native.sum_partials_multi
    monkeypatch.setattr(native, 'sum_partials_multi', lambda jobs: (sizes.append(len(jobs)), launch(jobs))[1])
    with native.LaunchProfiler(repeat=1) as prof:
        with direct_param_grads(), DeferredPartialSums() as later:
            loss().backward()
        mid = group.grad.clone()
        later.flush()
    seen = prof.summary()
    print('shared mixed: jobs per asac_sum_partials_multi launch', sizes)
    assert seen['asac_mlp_backward']['calls'] == 2 and seen['asac_attention_proj_backward']['calls'] == 1
    assert seen['asac_linear_tanh_backward2']['calls'] == 1
    assert sizes == [3, 1] and seen['asac_sum_partials_multi']['calls'] == 2
    assert torch.equal(mid, start) and torch.equal(group.grad, want_bits)


def test_one_conv_stack_behind_two_forward_passes_with_both_deferrals():
    """`sac_aux._train_rpm`'s order of calls (`autograd.grad` walks, parameter gradients handed back): per walk
    `DeferredConvBackward` records the cotangents inside an active `DeferredPartialSums`; its `flush()` runs inside that block —
    the multi-cotangent launches leave their slab sums to the outer `flush()` — and a parameter's gradient is the sum over the
    two forward passes.  Two terms, a + b == b + a: the bits of the undeferred walks.  The allocator's free blocks hold NaN
    before the deferred run and the reference runs after it, so a sum formed from memory nobody has written yet shows."""
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.fused_conv import DeferredConvBackward, conv_stack_desc, fused_conv_stack
    from algorithm.fused_mlp import DeferredPartialSums
    torch.manual_seed(5)
    conv = nn.Sequential(nn.Conv2d(3, 16, 8, 4), nn.GELU(), nn.Conv2d(16, 32, 4, 2), nn.GELU()).cuda()
    params = list(conv.parameters())
    frames1, frames2 = torch.randn(40, 3, 30, 30, device='cuda'), torch.randn(9, 3, 30, 30, device='cuda')
    A, B = torch.randn(128, 16, device='cuda'), torch.randn(128, 16, device='cuda')
    f1 = fused_conv_stack(frames1, conv_stack_desc(conv, frames1), conv)
    f2 = fused_conv_stack(frames2, conv_stack_desc(conv, frames2), conv)
    y = f1.sum(0) @ A + f2.sum(0) @ B
    cots = [torch.randn_like(y), torch.randn_like(y)]

    torch.cuda.synchronize()
    poison = [torch.full((1 << 20,), float('nan'), device='cuda') for _ in range(8)]      # 32 MB in 4 MB blocks ...
    poison += [torch.full((n,), float('nan'), device='cuda') for n in (1 << 18, 1 << 16, 1 << 14, 1 << 12, 1 << 10) * 4]
    torch.cuda.synchronize()
    del poison          # ... and small ones, back in the caching allocator: a `torch.empty` served from them holds NaN

    conv_later, aux = DeferredConvBackward(), []
    with native.LaunchProfiler(repeat=1) as prof:
        with DeferredPartialSums() as later:
            for k, c in enumerate(cots):
                later.walk = ('r', k)
                conv_later.walk = len(aux)
                with conv_later:
                    aux.append(list(torch.autograd.grad(y, params, grad_outputs=c, allow_unused=True, retain_graph=True)))
            conv_late = conv_later.flush()          # (its slab sums join the others)
        late = later.flush()
    seen = prof.summary()
    assert all(g is None for walk in aux for g in walk)

    def put(grads, late_grads):       # (sac_aux._train_rpm: a deferred launch's gradients where autograd left None, or beside)
        for j, p in enumerate(params):
            g_late = late_grads.get(id(p))
            if g_late is not None:
                grads[j] = g_late if grads[j] is None else grads[j] + g_late

    for k in range(len(cots)):
        put(aux[k], late.get(('r', k), {}))
    for walk, grads in conv_late.items():
        put(aux[walk], grads)
    got = [[None if g is None else g.clone() for g in walk] for walk in aux]
    want = [torch.autograd.grad(y, params, grad_outputs=c, retain_graph=True) for c in cots]
    per_pass = -(-len(cots) // native.conv2_backward_multi_max(conv_stack_desc(conv, frames1)))
    assert seen['asac_conv2_backward_multi']['calls'] == 2 * per_pass and 'asac_conv2_backward' not in seen
    for k in range(len(cots)):
        for j, p in enumerate(params):
            assert got[k][j] is not None, (k, j)
            assert torch.isfinite(got[k][j]).all(), ('a gradient read before it was written', k, tuple(p.shape))
            assert torch.equal(got[k][j], want[k][j]), (k, tuple(p.shape))
    # (the jobs write buffers of their own: nothing shared, one launch of the sums — as in the step without a shared stack)
    assert seen['asac_sum_partials_multi']['calls'] == 1
