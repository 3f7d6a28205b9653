"""GPU: `asac_image_warp` (csrc/image.hip) behind `RandomResizedCrop` / `ElasticTransform` / `RandomChoice` of
`algorithm/utils/image_transforms.py`.  The reference is the module code of the same file given the launch's own draws (the
window from `drawn()`, the field's noise and displacement from the launch's `noise_out` / `disp_out`).

Bounds.  A resized crop and the elastic gather copy input bits: `torch.equal`.  The displacement field is compared with the
float64 module code on the launch's noise; its error may be at most 4x that of the float32 module code on the same noise (the
separable against the 2-D summation order and the kernel's own `exp`, both O(k 2^-24)).  The elastic gather rounds a
coordinate to a pixel, so a coordinate within 1e-3 of a half-integer may fall either way between two float32 evaluations that
differ in contraction: those pixels are excluded, and there must be under 2 % of them.

Measured on an MI355X (the tests print them): field error, launch / float32 module code: 2.65e-7 / 1.06e-6 (s5_22x24),
2.59e-7 / 7.33e-7 (s2_24x28), 2.29e-7 / 5.64e-7 (pair_22x26); excluded pixels 0.38 %, 0.30 %, 0.35 %; pixels that sample
outside the plane 7.6 %, 30.5 %, 10.8 %; pixels moved 98.3 %, 99.7 %, 91.1 %."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import asac_amd  # noqa: E402,F401
from algorithm.utils import image_transforms as T  # noqa: E402
from algorithm.utils.image_transforms import InterpolationMode  # noqa: E402
import algorithm.nn_models as m  # noqa: E402
from asac_amd import native  # noqa: E402

DEV = torch.device('cuda', 0)
NEAREST, BILINEAR = InterpolationMode.NEAREST, InterpolationMode.BILINEAR
# name -> ((H, W), alpha, sigma)
ELASTIC_CASES = {
    's5_22x24': ((22, 24), 100., 5.),                     # ugv_parking's 41 taps on the smallest plane that admits them
    's2_24x28': ((24, 28), 100., 2.),
    'pair_22x26': ((22, 26), (30., 60.), (2., 3.)),       # 17 and 25 taps, x and y roles, the / H and / W divisors
}


def _planes(n, c, H, W):
    """distinct positive values per pixel and plane (exact in float32): pixel + 1 + plane * H * W"""
    assert n * c * H * W < 2 ** 24
    return torch.arange(1, n * c * H * W + 1, dtype=torch.float32, device=DEV).reshape(n, c, H, W)


def _launches(fn):
    with native.LaunchProfiler(repeat=1) as prof:
        out = fn()
    return out, prof.summary()


def _native(module, x):
    """module(x) and proof that it was ONE launch of the warp kernel"""
    out, seen = _launches(lambda: module(x))
    assert list(seen) == ['asac_image_warp'] and seen['asac_image_warp']['calls'] == 1, seen
    return out


def _keep_field(module, H, W):
    """has the module's launches write the field out; NaN until an elastic call does"""
    module._field_out = (torch.full((2, H, W), float('nan'), device=DEV), torch.full((2, H, W), float('nan'), device=DEV))
    return module._field_out


def _window_ok(d, H, W):
    return 0 < d['height'] <= H and 0 < d['width'] <= W and 0 <= d['top'] <= H - d['height'] and 0 <= d['left'] <= W - d['width']


def _area_ok(d, H, W, lo=0.8, hi=0.9):
    """the host test's bound: h and w are each rounded by at most a half"""
    h, w = d['height'], d['width']
    slack = ((h + w + 1) / 2 + 0.25) / (H * W)
    return lo - slack <= h * w / (H * W) <= hi + slack


def _check_crop(out, x, d, size):
    want = T.resized_crop(x, d['top'], d['left'], d['height'], d['width'], size, NEAREST)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def _check_gather(out, x, disp, planes=None):
    """out == elastic(x, disp) wherever the module code's coordinates are not within 1e-3 of a half-integer; -> shares"""
    H, W = x.shape[-2:]
    gx = torch.linspace((-W + 1) / W, (W - 1) / W, W, device=DEV)[None, :] + disp[0]
    gy = torch.linspace((-H + 1) / H, (H - 1) / H, H, device=DEV)[:, None] + disp[1]
    ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    near_half = lambda c: ((c - torch.floor(c)) - 0.5).abs() <= 1e-3        # noqa: E731
    keep = ~(near_half(ix) | near_half(iy))
    excluded = 1. - keep.float().mean().item()
    assert excluded < 0.02, excluded
    if planes is not None:
        x, out = x.flatten(0, 1)[planes][None], out.flatten(0, 1)[planes][None]
    want = T.elastic(x, disp.permute(1, 2, 0), NEAREST)
    assert torch.equal(out[..., keep], want[..., keep])
    outside = (want[0, 0] == 0).float().mean().item()
    moved = (want[0, 0] != x[0, 0]).float().mean().item()
    return excluded, outside, moved


def _one_field_for_all_planes(out, x):
    """with `_planes` inputs: every plane shows the same source pixel (or zero) at every position"""
    H, W = x.shape[-2:]
    o = out.flatten(0, 1)
    offset = (torch.arange(o.shape[0], device=DEV, dtype=torch.float32) * (H * W))[:, None, None]
    source = torch.where(o == 0, torch.full_like(o, -1.), o - offset)
    assert torch.equal(source, source[:1].expand_as(source))


# ---------------------------------------------------------------------------------------------- 1. resized crop
@pytest.mark.parametrize('size', [(16, 16), (28, 30)], ids=['shrinks', 'enlarges'])
def test_resized_crop_is_the_module_code_of_the_drawn_window(size):
    x = _planes(3, 2, 20, 24)
    rrc = T.RandomResizedCrop(size, scale=(0.8, 0.9), interpolation=NEAREST).reseed(5)
    windows = set()
    for call in range(12):
        out = _native(rrc, x)
        d = rrc.drawn()
        assert set(d) == set(native.IMAGE_WARP_DRAWN) and d['counter'] == call and d['choice'] == 0
        assert out.shape == (3, 2, *size) and _window_ok(d, 20, 24)
        _check_crop(out, x, d, size)
        windows.add((d['top'], d['left'], d['height'], d['width']))
    assert len(windows) >= 6, windows


def test_resized_crop_fallback_and_window_rule():
    x = _planes(1, 1, 20, 20)
    forced = T.RandomResizedCrop((16, 16), scale=(0.9, 1.0), ratio=(2., 3.), interpolation=NEAREST).reseed(6)
    for _ in range(4):
        out = _native(forced, x)
        d = forced.drawn()
        assert (d['height'], d['width'], d['top'], d['left']) == (10, 20, 5, 0)
        _check_crop(out, x, d, (16, 16))
    whole = T.RandomResizedCrop((20, 20), scale=(1.5, 2.0), interpolation=NEAREST).reseed(6)
    assert torch.equal(_native(whole, x), x)
    d = whole.drawn()
    assert (d['height'], d['width'], d['top'], d['left']) == (20, 20, 0, 0)
    # the window rule over 200 calls, as the host test states it for the module code
    x = _planes(1, 1, 20, 24)
    rrc = T.RandomResizedCrop((20, 24), scale=(0.8, 0.9), interpolation=NEAREST).reseed(7)
    fallbacks, windows = 0, set()
    for _ in range(200):
        rrc(x)
        d = rrc.drawn()
        assert _window_ok(d, 20, 24)
        if (d['height'], d['width']) == (20, 24):
            fallbacks += 1
            continue
        assert _area_ok(d, 20, 24), d
        windows.add((d['top'], d['left'], d['height'], d['width']))
    assert fallbacks <= 4 and len(windows) > 20
    assert rrc.counter_state() == (200, 0)


# ---------------------------------------------------------------------------------------------- 2., 3. elastic
_elastic_runs = {}


def _elastic_run(name):
    """one launch per case, shared by the tests: (x, out, noise, displacement)"""
    if name not in _elastic_runs:
        (H, W), alpha, sigma = ELASTIC_CASES[name]
        x = _planes(2, 3, H, W)
        mod = T.ElasticTransform(alpha=alpha, sigma=sigma, interpolation=NEAREST).reseed(len(name))
        noise, disp = _keep_field(mod, H, W)
        out = _native(mod, x)
        d = mod.drawn()
        assert (d['counter'], d['choice'], d['top'], d['left'], d['height'], d['width']) == (0, 0, -1, -1, -1, -1)
        _elastic_runs[name] = (x, out, noise, disp)
    return _elastic_runs[name]


@pytest.mark.parametrize('name', list(ELASTIC_CASES))
def test_elastic_field_against_the_float64_module_code(name):
    (H, W), alpha, sigma = ELASTIC_CASES[name]
    _, _, noise, disp = _elastic_run(name)
    noise, disp = noise.cpu(), disp.cpu()
    assert not noise.isnan().any() and (noise >= -1).all() and (noise < 1).all()
    assert not torch.equal(noise[0], noise[1]) and noise.std() > 0.5               # U[-1, 1): std 0.577
    want = T.elastic_displacement(noise.double(), alpha, sigma).permute(2, 0, 1)
    e_ref = (T.elastic_displacement(noise, alpha, sigma).permute(2, 0, 1).double() - want).abs().max().item()
    e_launch = (disp.double() - want).abs().max().item()
    print(f'field/{name}: launch {e_launch:.3g}, float32 module code {e_ref:.3g}')
    assert e_ref > 0 and e_launch <= 4 * e_ref


@pytest.mark.parametrize('name', list(ELASTIC_CASES))
def test_elastic_gather_is_the_module_code_of_the_drawn_field(name):
    x, out, _, disp = _elastic_run(name)
    excluded, outside, moved = _check_gather(out, x, disp)
    print(f'gather/{name}: excluded {excluded:.4f}, outside {outside:.3f}, moved {moved:.3f}')
    assert outside > 0.01 and moved > 0.5, 'the zero fill and the gather are both exercised'
    _one_field_for_all_planes(out, x)


# ---------------------------------------------------------------------------------------------- 4. many planes
def test_more_planes_than_workgroups():
    x = _planes(130, 4, 22, 24)                              # 520 planes: over the grid's 512 (256 with a large field)
    at = [0, 259, 519]
    rrc = T.RandomResizedCrop((16, 30), scale=(0.8, 0.9), interpolation=NEAREST).reseed(8)
    out = _native(rrc, x)
    d = rrc.drawn()
    _check_crop(out.flatten(0, 1)[at], x.flatten(0, 1)[at], d, (16, 30))
    mod = T.ElasticTransform(alpha=100., sigma=5., interpolation=NEAREST).reseed(9)
    _, disp = _keep_field(mod, 22, 24)
    out = _native(mod, x)
    _check_gather(out, x, disp, planes=at)
    _one_field_for_all_planes(out, x)


# ---------------------------------------------------------------------------------------------- 5. choice, stream, capture
def _parking(seed, instance_id=91):
    """the reference's ugv_parking member list at 24 x 24"""
    choice = T.RandomChoice([
        m.Transform(T.RandomResizedCrop(size=(24, 24), scale=(0.8, 0.9), interpolation=InterpolationMode.NEAREST)),
        m.Transform(T.ElasticTransform(alpha=100, sigma=5, interpolation=InterpolationMode.NEAREST)),
    ]).reseed(seed, instance_id=instance_id)
    _keep_field(choice, 24, 24)
    return choice


def _check_member(choice, out, x):
    d = choice.drawn()
    if d['choice'] == 0:
        assert _window_ok(d, 24, 24)
        _check_crop(out, x, d, (24, 24))
    else:
        assert (d['top'], d['left'], d['height'], d['width']) == (-1, -1, -1, -1)
        _check_gather(out, x, choice._field_out[1])
    return d


def test_choice_eager_and_its_stream():
    x = _planes(4, 3, 24, 24)
    choice = _parking(seed=4321)
    assert [o.kind for o in T._native_ops(choice)] == ['RESIZED_CROP', 'ELASTIC']
    outs, picks = [], []
    for call in range(24):
        out = _native(choice, x)
        d = _check_member(choice, out, x)
        assert d['counter'] == call, 'the counter advances by one per call'
        outs.append(out)
        picks.append(d['choice'])
    assert set(picks) == {0, 1}
    assert choice.counter_state() == (24, 0), 'counter, and the arrival word left at zero'
    # the stream is a function of (seed, instance, counter)
    choice.set_counter(3)
    assert torch.equal(_native(choice, x), outs[3]) and torch.equal(_native(choice, x), outs[4])
    again = _parking(seed=4321)
    assert torch.equal(_native(again, x), outs[0])
    other = _parking(seed=4321, instance_id=92)
    assert not all(torch.equal(_native(other, x), outs[call]) for call in range(4)), 'another instance is another stream'


def test_choice_inside_a_captured_step_draws_afresh():
    from algorithm.captured_step import CapturedStep
    x = _planes(4, 3, 24, 24)
    choice = _parking(seed=99)
    choice(x)                                               # eager warm-up: the instance owns its counter before the capture
    out = torch.empty_like(x)
    step = CapturedStep.capture(lambda: out.copy_(choice(x)), DEV)
    choice.set_counter(0)
    replays, records = [], []
    for replay in range(3):
        step.replay()
        d = _check_member(choice, out, x)
        assert d['counter'] == replay
        replays.append(out.clone())
        records.append(d)
    assert not torch.equal(replays[0], replays[1]) and not torch.equal(replays[1], replays[2]) \
        and not torch.equal(replays[0], replays[2]), 'every replay draws afresh'
    assert choice.counter_state() == (3, 0)
    choice.set_counter(0)
    for want, record in zip(replays, records):
        assert torch.equal(_native(choice, x), want) and choice.drawn() == record


# ---------------------------------------------------------------------------------------------- 6. what stays module code
def test_module_code_fallbacks_do_not_launch():
    scale, ratio = (0.8, 0.9), (3 / 4, 4 / 3)
    rrc = lambda mode: T.RandomResizedCrop((12, 12), scale=scale, interpolation=mode)          # noqa: E731
    ela = lambda mode, sigma=1.: T.ElasticTransform(alpha=30., sigma=sigma, interpolation=mode)    # noqa: E731
    small, big, mid = _planes(1, 2, 16, 16) / 512, _planes(1, 1, 97, 96) / 9312, _planes(1, 1, 70, 70) / 4900
    cases = [(rrc(BILINEAR), small), (rrc(NEAREST), small.clone().requires_grad_()), (rrc(NEAREST), big),
             (rrc(NEAREST), small.double()), (ela(BILINEAR), small), (ela(NEAREST), small.clone().requires_grad_()),
             (ela(NEAREST), big), (ela(NEAREST, 8.), mid)]                  # (sigma 8: 65 taps)
    for module, inp in cases:
        torch.manual_seed(3)
        out, seen = _launches(lambda: module(inp))
        assert not [k for k in seen if k.startswith('asac_image_')], seen
        # the module code from the same host draws
        torch.manual_seed(3)
        H, W = inp.shape[-2:]
        if isinstance(module, T.RandomResizedCrop):
            top, left, h, w = T.get_resized_crop_params(H, W, scale, ratio)
            want = T.resized_crop(inp, top, left, h, w, (12, 12), module.interpolation)
        else:
            noise = (torch.rand(2, H, W) * 2 - 1).to(DEV)
            want = T.elastic(inp, T.elastic_displacement(noise, module.alpha, module.sigma), module.interpolation)
        assert out.dtype == inp.dtype and out.requires_grad == inp.requires_grad and torch.equal(out.detach(), want.detach())
    nine, seen = _launches(lambda: T.RandomChoice([rrc(NEAREST)] * 9)(small))
    assert nine.shape == (1, 2, 12, 12) and list(seen) == ['asac_image_warp'], 'a host pick, then the member\'s own launch'
    # a mixed choice is a host pick between two launchers
    torch.manual_seed(0)
    mixed = T.RandomChoice([rrc(NEAREST), T.GaussianBlur(3, sigma=1.)])
    seen = set()
    for _ in range(12):
        seen |= set(_launches(lambda: mixed(small))[1])
    assert seen == {'asac_image_warp', 'asac_image_augment'}


def test_the_entry_point_refuses_what_is_outside_its_limits():
    lib = native.load()
    x = _planes(2, 3, 30, 30)
    y = torch.full_like(x, -7.)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    elastic = dict(kind=native.IMAGE_WARP_ELASTIC, k0=41, k1=41, alpha0=100., alpha1=100., sigma0=5., sigma1=5.)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731

    def call(op, H=30, W=30, Ho=30, Wo=30, n_ops=1, planes=6):
        return lib.asac_image_warp(ptr(x), ptr(y), planes, 3, H, W, Ho, Wo, native.warp_image_ops([op]), n_ops, 0, 1, ptr(state),
                                   None, None, None, None)

    refused = [call(dict(elastic, k0=65)), call(dict(elastic, k1=40)), call(elastic, H=20, W=45, Ho=20, Wo=45),
               call(elastic, H=100, W=100, Ho=100, Wo=100, planes=3), call(elastic, n_ops=9), call(elastic, Ho=31),
               call(dict(elastic, sigma1=0.)), call(dict(kind=native.IMAGE_WARP_RESIZED_CROP, scale_lo=.9, scale_hi=.8,
                                                         ratio_lo=.75, ratio_hi=1.3))]
    assert refused == [1] * len(refused), refused             # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (y == -7.).all() and state.tolist() == [0, 0], 'nothing was launched'
    with pytest.raises(native.AsacNativeError):
        native.warp_image(x, y, native.warp_image_ops([dict(elastic, k0=65)]), state=state)
