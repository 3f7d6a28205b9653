"""CPU: `algorithm/utils/image_transforms.py` — the module code against float64 evaluations of the definitions it states
(tests/image_ref.py), the draw rules, the unsupported arguments, what `_native_ops` reduces to a launch, and the surface of
`asac_image_augment` (header, binding, wrapper, INTEGRATION.md, the host refusals)."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401
from algorithm.utils import image_transforms as T
from algorithm.utils.transform import DepthNoise, GaussianNoise, SaltAndPepperNoise
import algorithm.nn_models as m
from tests import image_ref as ref

ROOT = Path(__file__).resolve().parent.parent


def _img(*shape, seed=0, dtype=torch.float64):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ---------------------------------------------------------------------------------------------- definitions
@pytest.mark.parametrize('shape,k,sigma', [((2, 3, 9, 9), 9, 9.), ((1, 2, 11, 7), (5, 3), 0.7), ((2, 3, 30, 30), 9, 9.),
                                            ((1, 1, 5, 6), 1, 1.), ((4, 2, 1, 8, 8), 3, 2.)],
                         ids=['reach', 'pair', 'plugin', 'one_tap', 'lead_dims'])
def test_blur_module_code_is_the_definition(shape, k, sigma):
    x = _img(*shape)
    kx, ky = (k, k) if isinstance(k, int) else k
    want = ref.blur(x.numpy(), kx, ky, sigma)
    got = T.GaussianBlur(k, sigma=sigma)(x)
    assert got.shape == x.shape and got.dtype == torch.float64
    assert np.abs(got.numpy() - want).max() <= 1e-13
    got32 = T.GaussianBlur(k, sigma=sigma)(x.float())
    assert got32.dtype == torch.float32 and np.abs(got32.double().numpy() - want).max() <= 2e-6


def test_blur_weights():
    w = T.gaussian_kernel1d(5, 1.5, torch.float64)
    x = np.linspace(-2, 2, 5)
    e = np.exp(-0.5 * (x / 1.5) ** 2)
    assert np.abs(w.numpy() - e / e.sum()).max() <= 1e-15 and abs(float(w.sum()) - 1) <= 1e-15


def test_blur_radius_past_the_plane_raises_as_torch_does():
    with pytest.raises(RuntimeError):
        T.GaussianBlur(9, sigma=1.)(_img(1, 1, 4, 4))


@pytest.mark.parametrize('hw,size,out', [((50, 50), (84, 84), (84, 84)), ((7, 5), (7, 9), (7, 9)), ((1, 1), (4, 4), (4, 4)),
                                          ((6, 9), 12, (12, 18)), ((9, 6), 12, (18, 12)), ((6, 6), 6, (6, 6))],
                         ids=['50to84', '7x5to7x9', '1to4', 'short_side_h', 'short_side_w', 'same'])
def test_resize_module_code_is_the_definition(hw, size, out):
    x = _img(2, 3, *hw)
    got = T.Resize(size)(x)
    assert tuple(got.shape) == (2, 3, *out)
    assert np.abs(got.numpy() - ref.resize(x.numpy(), *out)).max() <= 1e-13
    got32 = T.Resize(size)(x.float())
    assert np.abs(got32.double().numpy() - ref.resize(x.numpy(), *out)).max() <= 5e-5


def test_resize_downscale_antialiases():
    x = _img(1, 1, 16, 16)
    got = T.Resize((8, 8))(x)
    want = torch.nn.functional.interpolate(x, size=(8, 8), mode='bilinear', align_corners=False, antialias=True)
    assert torch.equal(got, want) and np.abs(got.numpy() - ref.resize(x.numpy(), 8, 8)).max() > 1e-3


def test_brightness_module_code_is_the_definition():
    x = _img(2, 3, 5, 5) * 1.2
    got = T.ColorJitter(brightness=(1.3, 1.3))(x)
    assert np.abs(got.numpy() - ref.brightness(x.numpy(), 1.3)).max() <= 1e-15
    assert float(got.max()) == 1.0
    assert T.ColorJitter()(x) is x and T.ColorJitter(brightness=0)(x) is x


# ---------------------------------------------------------------------------------------------- draw rules
def test_random_crop_offsets_cover_the_valid_range_and_no_more():
    H, W = 6, 7
    x = (torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)).expand(2, 3, H, W)
    torch.manual_seed(0)
    crop = T.RandomCrop((4, 5))
    seen = set()
    for _ in range(200):
        y = crop(x)
        assert y.shape == (2, 3, 4, 5)
        first = int(y[0, 0, 0, 0])
        top, left = divmod(first, W)
        assert 0 <= top <= H - 4 and 0 <= left <= W - 5
        assert torch.equal(y, x[..., top:top + 4, left:left + 5])     # one offset for the whole call
        seen.add((top, left))
    assert seen == {(t, l) for t in range(3) for l in range(3)}
    assert T.RandomCrop(6)(torch.zeros(1, 6, 6)).shape == (1, 6, 6)
    with pytest.raises(ValueError):
        T.RandomCrop(8)(x)


def test_random_choice_calls_exactly_one_member():
    calls = [0, 0, 0]

    def member(i):
        def f(x):
            calls[i] += 1
            return x + i
        return f

    choice = T.RandomChoice([member(0), member(1), member(2)])
    torch.manual_seed(1)
    x = torch.zeros(1, 1, 2, 2)
    for n in range(1, 91):
        y = choice(x)
        assert sum(calls) == n and float(y[0, 0, 0, 0]) in (0., 1., 2.)
    assert all(c >= 12 for c in calls), calls       # 30 +- 4.5 sigma


def test_sigma_and_brightness_ranges_are_honoured():
    torch.manual_seed(2)
    x = torch.zeros(1, 1, 7, 7, dtype=torch.float64)
    x[0, 0, 3, 3] = 1.
    blur = T.GaussianBlur(3, sigma=(0.5, 1.5))
    lo, hi = (float(ref.blur(x.numpy(), 3, 3, s)[0, 0, 3, 3]) for s in (0.5, 1.5))      # the peak falls with sigma
    peaks = {float(blur(x)[0, 0, 3, 3]) for _ in range(40)}
    assert len(peaks) == 40 and all(hi <= p <= lo for p in peaks)
    half = torch.full((1, 1, 2, 2), 0.5, dtype=torch.float64)
    jitter = T.ColorJitter(brightness=0.4)
    assert jitter.brightness == (0.6, 1.4) and T.ColorJitter(brightness=1.5).brightness == (0., 2.5)
    factors = {float(jitter(half)[0, 0, 0, 0]) / 0.5 for _ in range(40)}
    assert len(factors) == 40 and all(0.6 <= f <= 1.4 for f in factors)
    assert T.ColorJitter(brightness=(0.2, 0.3)).brightness == (0.2, 0.3)
    assert T.GaussianBlur(5).sigma == (0.1, 2.0) and T.GaussianBlur((5, 3), 2).kernel_size == (5, 3)


# ---------------------------------------------------------------------------------------------- unsupported arguments
@pytest.mark.parametrize('build,name', [
    (lambda: T.ColorJitter(contrast=0.5), 'contrast'), (lambda: T.ColorJitter(saturation=(0.5, 1.)), 'saturation'),
    (lambda: T.ColorJitter(brightness=0.1, hue=0.1), 'hue'),
    (lambda: T.RandomCrop(4, padding=2), 'padding'), (lambda: T.RandomCrop(4, pad_if_needed=True), 'pad_if_needed'),
    (lambda: T.RandomCrop(4, fill=1), 'fill'), (lambda: T.RandomCrop(4, padding_mode='reflect'), 'padding_mode'),
    (lambda: T.Resize(4, interpolation=T.InterpolationMode.NEAREST), 'interpolation'),
    (lambda: T.Resize(4, interpolation='bicubic'), 'interpolation'), (lambda: T.Resize(4, max_size=8), 'max_size'),
    (lambda: T.RandomChoice([lambda x: x], p=[1.]), 'p')])
def test_unsupported_arguments_raise_by_name(build, name):
    with pytest.raises(NotImplementedError, match=name):
        build()


def test_argument_errors():
    for bad in (4, 0, (3, 4), 33):
        with pytest.raises(ValueError):
            T.GaussianBlur(bad)
    for bad in (0., (2., 1.), -1.):
        with pytest.raises(ValueError):
            T.GaussianBlur(3, sigma=bad)
    with pytest.raises(TypeError):
        T.GaussianBlur(3, sigma=1.)(np.zeros((1, 3, 3)))


# ---------------------------------------------------------------------------------------------- _native_ops
def _crop_resize():
    return T.Compose([T.RandomCrop(18), T.Resize((30, 30))])


OP = T._Op
REDUCTIONS = [
    (lambda: T.GaussianBlur(9, sigma=9), [OP('BLUR', kernel_size=(9, 9), sigma=(9., 9.))]),
    (lambda: T.GaussianBlur((5, 3)), [OP('BLUR', kernel_size=(5, 3), sigma=(0.1, 2.0))]),
    (lambda: T.ColorJitter(brightness=0.5), [OP('BRIGHTNESS', factor=(0.5, 1.5))]),
    (lambda: T.ColorJitter(), [OP('COPY')]),
    (lambda: T.RandomCrop(18), [OP('CROP_RESIZE', crop=(18, 18), size=None)]),
    (lambda: T.Resize(30), [OP('CROP_RESIZE', crop=None, size=30)]),
    (lambda: m.Transform(T.GaussianBlur(3, sigma=1)), [OP('BLUR', kernel_size=(3, 3), sigma=(1., 1.))]),
    (lambda: m.Transform(m.Transform(SaltAndPepperNoise(0.2, 0.5))), [OP('SALT_PEPPER', snr=0.2, p=0.5)]),
    (lambda: GaussianNoise(0.1, 0.3), [OP('UNIFORM_NOISE', mean=0.1, std=0.3)]),
    (_crop_resize, [OP('CROP_RESIZE', crop=(18, 18), size=(30, 30))]),
    (lambda: torch.nn.Sequential(T.RandomCrop((4, 5)), T.Resize(9)), [OP('CROP_RESIZE', crop=(4, 5), size=9)]),
    (lambda: m.Transform(_crop_resize()), [OP('CROP_RESIZE', crop=(18, 18), size=(30, 30))]),
    (lambda: T.Compose([T.GaussianBlur(3, sigma=1)]), [OP('BLUR', kernel_size=(3, 3), sigma=(1., 1.))]),
    (lambda: T.RandomChoice([m.Transform(SaltAndPepperNoise(0.2, 0.5)), m.Transform(GaussianNoise()),
                             m.Transform(T.GaussianBlur(9, sigma=9)), _crop_resize()]),
     [OP('SALT_PEPPER', snr=0.2, p=0.5), OP('UNIFORM_NOISE', mean=0., std=0.1),
      OP('BLUR', kernel_size=(9, 9), sigma=(9., 9.)), OP('CROP_RESIZE', crop=(18, 18), size=(30, 30))]),
    # what does not reduce to one launch
    (lambda: T.Compose([T.Resize(30), T.RandomCrop(18)]), None),                 # the other order is two resamplings
    (lambda: T.Compose([T.GaussianBlur(3, sigma=1), T.ColorJitter(brightness=0.1)]), None),
    (lambda: T.Compose([T.RandomCrop(18), T.Resize(30), T.GaussianBlur(3)]), None),
    (lambda: T.RandomChoice([T.GaussianBlur(3), lambda x: x]), None),
    (lambda: T.RandomChoice([T.GaussianBlur(3), T.Compose([T.GaussianBlur(3), T.ColorJitter(brightness=0.1)])]), None),
    (lambda: T.RandomChoice([T.GaussianBlur(3), T.RandomChoice([T.GaussianBlur(3), T.GaussianBlur(5)])]), None),
    (lambda: DepthNoise(0.1), None),
    (lambda: m.Transform(None), None),
    (lambda: (lambda x: x), None),
]


@pytest.mark.parametrize('build,want', REDUCTIONS, ids=[str(i) for i in range(len(REDUCTIONS))])
def test_native_ops_reductions(build, want):
    assert T._native_ops(build()) == want


def test_resolve_against_the_frame():
    """which members the kernel takes at a given frame size, and the output size they give"""
    from asac_amd import native
    f, out = T._resolve(OP('CROP_RESIZE', crop=(18, 18), size=30), 30, 30)
    assert (f['crop_h'], f['crop_w'], out) == (18, 18, (30, 30))
    assert T._resolve(OP('CROP_RESIZE', crop=None, size=(7, 9)), 7, 5)[1] == (7, 9)
    assert T._resolve(OP('CROP_RESIZE', crop=None, size=(8, 8)), 16, 16) is None          # shrinks
    assert T._resolve(OP('CROP_RESIZE', crop=None, size=(20, 8)), 16, 16) is None         # ... along one axis
    assert T._resolve(OP('CROP_RESIZE', crop=(18, 18), size=None), 9, 30) is None         # larger than the frame
    assert T._resolve(OP('BLUR', kernel_size=(9, 9), sigma=(1., 1.)), 4, 30) is None      # k // 2 >= H
    assert T._resolve(OP('BLUR', kernel_size=(9, 9), sigma=(1., 1.)), 5, 5)[1] == (5, 5)
    f, _ = T._resolve(OP('SALT_PEPPER', snr=0.2, p=0.5), 9, 9)
    assert (f['kind'], f['a'], f['b'], f['c']) == (native.IMAGE_SALT_PEPPER, 0.2, 0.25, 0.75)


def test_cpu_tensors_take_the_module_code_and_transform_wraps_unchanged():
    x = _img(2, 4, 3, 20, 20, dtype=torch.float32)
    blur = T.GaussianBlur(3, sigma=1.)
    assert blur._launch(T._native_ops(blur), x) is None
    wrapped = m.Transform(blur)(x)
    assert wrapped.shape == x.shape and torch.equal(wrapped, blur(x))
    assert m.Transform(_crop_resize())(x).shape == (2, 4, 3, 30, 30)
    assert 'frozen' in T.RandomChoice.__doc__.lower() and 'frozen' in T.RandomCrop.__doc__.lower()
    assert not list(blur.state_dict()) and not list(T.RandomChoice([blur]).state_dict())   # a plugin keeps its keys


# ---------------------------------------------------------------------------------------------- surface
def test_entry_point_is_declared_bound_wrapped_and_documented():
    import inspect
    from asac_amd import abi, native
    assert native.ABI_VERSION == 91 and abi.defines['ASAC_ABI_VERSION'] == 91
    assert 'asac_image_augment' in native.EXPORTED_SYMBOLS
    assert len(native._SIGNATURES['asac_image_augment'][1]) == len(abi.functions['asac_image_augment'][1]) == 15
    assert native.image_augment.__name__ == 'image_augment'
    assert [n for n, _ in inspect.getmembers(native) if n.startswith('image_') and callable(getattr(native, n))] == \
        ['image_augment', 'image_ops']
    for macro, value in (('ASAC_IMAGE_MAX_OPS', native.IMAGE_MAX_OPS), ('ASAC_IMAGE_MAX_PLANE', native.IMAGE_MAX_PLANE),
                         ('ASAC_IMAGE_MAX_KERNEL', native.IMAGE_MAX_KERNEL), ('ASAC_IMAGE_COPY', native.IMAGE_COPY),
                         ('ASAC_IMAGE_BLUR', native.IMAGE_BLUR), ('ASAC_IMAGE_BRIGHTNESS', native.IMAGE_BRIGHTNESS),
                         ('ASAC_IMAGE_CROP_RESIZE', native.IMAGE_CROP_RESIZE), ('ASAC_IMAGE_SALT_PEPPER', native.IMAGE_SALT_PEPPER),
                         ('ASAC_IMAGE_UNIFORM_NOISE', native.IMAGE_UNIFORM_NOISE)):
        assert abi.defines[macro] == value, macro
    # 84 x 84 and 30 x 30 fit, and two workgroups (two planes each, plus the taps) fit a CU's 160 KiB
    assert 84 * 84 <= native.IMAGE_MAX_PLANE and 2 * (2 * native.IMAGE_MAX_PLANE + 68) * 4 <= 160 * 1024
    # the descriptor: as many fields, in the header's order
    fields = [field for field, *_ in abi.structs['asac_image_op_t']]
    assert fields == [n for n, _ in native.ImageOp._fields_] and ctypes.sizeof(native.ImageOp) == 4 * len(fields)
    assert 'asac_image_augment' in (ROOT / 'INTEGRATION.md').read_text()
    assert "'image.hip'" in (ROOT / 'advanced-soft-actor-critic_amd' / 'csrc' / 'build.py').read_text()


def test_profiler_key_is_the_entry_point():
    from asac_amd import native
    seen = []

    class Spy:
        def bracket(self, name, fn, *a, **k):
            seen.append(name)

    native.set_profiler(Spy())
    try:
        native.image_augment()
    finally:
        native.set_profiler(None)
    assert seen == ['asac_image_augment']


def test_host_refusals_need_no_device():
    """a refused call returns hipErrorInvalidValue and names itself before anything touches a device: the pointers handed in
    here point nowhere"""
    from asac_amd import native
    lib = native.load()
    bad = 1                                                    # hipErrorInvalidValue
    fake = ctypes.c_void_p(4096)

    def call(op=None, x=fake, y=fake, planes=6, C=3, H=30, W=30, Ho=30, Wo=30, n_ops=1, state=fake, ops='table'):
        table = native.image_ops([op or dict(kind=native.IMAGE_BLUR, kx=9, ky=9, lo=1., hi=1.)])
        rc = lib.asac_image_augment(x, y, planes, C, H, W, Ho, Wo, table if ops == 'table' else None, n_ops, 0, 1, state,
                                    None, None)
        return rc, lib.asac_last_error()

    blur = lambda **k: dict(dict(kind=native.IMAGE_BLUR, kx=9, ky=9, lo=1., hi=1.), **k)    # noqa: E731
    refused = [
        call(x=None), call(y=None), call(ops=None),                                          # null pointers
        call(blur(kx=8)), call(blur(ky=4)), call(blur(kx=33)), call(blur(ky=33)), call(blur(kx=0)),   # even, over 31
        call(H=97, W=96, Ho=97, Wo=96), call(H=1, W=native.IMAGE_MAX_PLANE + 1, Ho=1, Wo=native.IMAGE_MAX_PLANE + 1),
        call(blur(), H=4, W=30, Ho=4, Wo=30),                                                # k // 2 >= H
        call(blur(lo=0., hi=0.)), call(blur(lo=2., hi=1.)),
        call(n_ops=0), call(n_ops=9), call(planes=0), call(planes=7), call(dict(kind=17)),
        call(blur(), Ho=31),                                                                 # only a resize changes the size
        call(dict(kind=native.IMAGE_CROP_RESIZE, crop_h=18, crop_w=18), Ho=17),              # shrinks
        call(dict(kind=native.IMAGE_CROP_RESIZE, crop_h=31, crop_w=18)),
        call(dict(kind=native.IMAGE_CROP_RESIZE, crop_h=18, crop_w=18, top=13, left=0)),
        call(blur(lo=1., hi=2.), state=None),                                                # draws without a counter
        call(dict(kind=native.IMAGE_SALT_PEPPER, a=.2, b=.25, c=.75), state=None),
    ]
    for i, (rc, msg) in enumerate(refused):
        assert rc == bad and b'asac_image_augment' in msg, (i, rc, msg)
    assert b'ASAC_IMAGE_MAX_PLANE' in call(H=97, W=96, Ho=97, Wo=96)[1]
    with pytest.raises(AssertionError):
        native.image_ops([dict(kind=0)] * 9)
