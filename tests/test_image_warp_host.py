"""CPU: `RandomResizedCrop` and `ElasticTransform` of `algorithm/utils/image_transforms.py` — the window rule, the nearest
resize as explicit integer indexing, the displacement field against a float64 evaluation written here, the sampling, the
port of the reference's `ugv_parking` augmentation block, what `_native_ops` reduces to a warp table, the arguments, and the
surface of `asac_image_warp` (header, binding, the host refusals)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import asac_amd  # noqa: F401
from algorithm.utils import image_transforms as T
from algorithm.utils.image_transforms import InterpolationMode
import algorithm.nn_models as m

NEAREST, BILINEAR = InterpolationMode.NEAREST, InterpolationMode.BILINEAR


def ugv_parking_members(size=(84, 84)):
    """the member list of the reference's envs/ugv/ugv_parking/nn_parking.py, `T` being this package's module"""
    return [
        m.Transform(T.RandomResizedCrop(size=size, scale=(0.8, 0.9), interpolation=InterpolationMode.NEAREST)),
        m.Transform(T.ElasticTransform(alpha=100, sigma=5, interpolation=InterpolationMode.NEAREST)),
    ]


# ---------------------------------------------------------------------------------------------- the window
def test_windows_lie_inside_the_frame_and_have_the_drawn_area():
    torch.manual_seed(1)
    H, W, ratio = 20, 24, (3 / 4, 4 / 3)
    whole, seen = 0, set()
    for _ in range(2000):
        top, left, h, w = T.get_resized_crop_params(H, W, (0.8, 0.9), ratio)
        assert 0 < h <= H and 0 < w <= W and 0 <= top <= H - h and 0 <= left <= W - w
        if (top, left, h, w) == (0, 0, H, W):       # the central fallback at this shape (W / H lies inside `ratio`)
            whole += 1
            continue
        # a = sqrt(area * aspect) and b = sqrt(area / aspect) are each rounded by at most a half: w h differs from a b, the
        # drawn area, by at most (a + b) / 2 + 1 / 4 <= (w + h + 1) / 2 + 1 / 4
        slack = ((h + w + 1) / 2 + 0.25) / (H * W)
        assert 0.8 - slack <= h * w / (H * W) <= 0.9 + slack, (h, w)
        seen.add((top, left, h, w))
    # (the whole frame after ten rejections: well under 1 % of the calls at this shape)
    assert whole <= 20 and len(seen) > 20


def test_the_central_fallback():
    for _ in range(20):
        assert T.get_resized_crop_params(20, 20, (0.9, 1.0), (2., 3.)) == (5, 0, 10, 20)       # top, left, h, w
        assert T.get_resized_crop_params(20, 20, (0.9, 1.0), (1 / 3, 1 / 2)) == (0, 5, 20, 10)
        assert T.get_resized_crop_params(20, 24, (1.5, 2.0), (3 / 4, 4 / 3)) == (0, 0, 20, 24)


@pytest.mark.parametrize('size', [(16, 16), (28, 30), (7, 24)], ids=['shrinks', 'enlarges', 'mixed'])
def test_nearest_resized_crop_is_integer_indexing(size):
    x = torch.arange(2 * 3 * 20 * 24, dtype=torch.float32).reshape(2, 3, 20, 24)
    top, left, h, w = 2, 3, 17, 19
    got = T.resized_crop(x, top, left, h, w, size, NEAREST)
    sy = [min(int(math.floor(np.float32(i) * (np.float32(h) / np.float32(size[0])))), h - 1) for i in range(size[0])]
    sx = [min(int(math.floor(np.float32(j) * (np.float32(w) / np.float32(size[1])))), w - 1) for j in range(size[1])]
    want = x[..., top:top + h, left:left + w][..., sy, :][..., sx]
    assert got.shape == (2, 3, *size) and torch.equal(got, want)
    # bilinear is `resize` of the window
    assert torch.equal(T.resized_crop(x, top, left, h, w, size, BILINEAR), T.resize(T.crop(x, top, left, h, w), size))


# ---------------------------------------------------------------------------------------------- the field
def displacement64(noise, alpha, sigma):
    """float64, no loops over pixels: field f is blurred with k_f taps on both axes, the taps along x from sigma[0] and
    along y from sigma[1], over reflect indices; x is divided by H, y by W"""
    noise = np.asarray(noise, dtype=np.float64)
    _, H, W = noise.shape
    out = np.empty((H, W, 2))
    for f in range(2):
        k = int(8 * sigma[f] + 1)
        k += 1 - k % 2
        r = k // 2
        t = np.arange(k) - (k - 1) / 2
        wx, wy = np.exp(-0.5 * (t / sigma[0]) ** 2), np.exp(-0.5 * (t / sigma[1]) ** 2)
        wx, wy = wx / wx.sum(), wy / wy.sum()

        def reflect(n):
            i = np.abs(np.arange(n)[:, None] + np.arange(k)[None, :] - r)
            return np.where(i >= n, 2 * (n - 1) - i, i)                       # [n, k]
        rows = np.einsum('hxk,k->hx', noise[f][:, reflect(W)], wx)            # along x
        both = np.einsum('ykx,k->yx', rows[reflect(H), :], wy)                # along y
        out[..., f] = both * alpha[f] / (H if f == 0 else W)
    return out


def test_displacement_is_the_definition():
    alpha, sigma = (30., 60.), (2., 3.)
    assert T._elastic_taps(sigma) == [17, 25]
    noise = torch.rand(2, 22, 26, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2 - 1
    got = T.elastic_displacement(noise, alpha, sigma)
    want = displacement64(noise.numpy(), alpha, sigma)
    assert got.shape == (22, 26, 2) and got.dtype == torch.float64
    assert np.abs(got.numpy() - want).max() <= 1e-13
    assert np.abs(want[..., 0]).max() > 0.01 and np.abs(want[..., 1]).max() > 0.01
    got32 = T.elastic_displacement(noise.float(), alpha, sigma)
    assert got32.dtype == torch.float32 and np.abs(got32.double().numpy() - want).max() <= 1e-5
    # scalars become pairs; zero noise is no displacement
    assert torch.equal(T.elastic_displacement(noise, 30., 2.), T.elastic_displacement(noise, (30., 30.), (2., 2.)))
    assert not T.elastic_displacement(torch.zeros(2, 22, 26), alpha, sigma).any()
    # a sigma <= 0 skips that field's blur
    raw = T.elastic_displacement(noise, (22., 26.), (0., 0.))
    assert np.abs(raw.numpy() - noise.permute(1, 2, 0).numpy()).max() <= 1e-15


def test_blur_with_a_scalar_sigma_is_unchanged_by_the_pair():
    x = torch.rand(2, 3, 9, 11, generator=torch.Generator().manual_seed(4))
    assert torch.equal(T.gaussian_blur(x, (5, 3), 1.3), T.gaussian_blur(x, (5, 3), (1.3, 1.3)))
    assert not torch.equal(T.gaussian_blur(x, (5, 3), (1.3, 0.4)), T.gaussian_blur(x, (5, 3), (0.4, 1.3)))


def test_zero_displacement_is_the_identity_and_one_pixel_shifts():
    H, W = 6, 8
    x = torch.arange(1, 2 * 3 * H * W + 1, dtype=torch.float32).reshape(2, 3, H, W)
    zero = torch.zeros(H, W, 2)
    assert torch.equal(T.elastic(x, zero, NEAREST), x)
    assert torch.allclose(T.elastic(x, zero, BILINEAR), x, atol=1e-3)
    shift = zero.clone()
    shift[..., 0] = 2 / W                                   # every pixel reads its right neighbour
    out = T.elastic(x, shift, NEAREST)
    assert torch.equal(out[..., :, :-1], x[..., :, 1:]) and not out[..., :, -1].any()
    down = zero.clone()
    down[..., 1] = -2 / H                                   # ... the pixel above it
    out = T.elastic(x, down, NEAREST)
    assert torch.equal(out[..., 1:, :], x[..., :-1, :]) and not out[..., 0, :].any()


def test_module_code_classes():
    torch.manual_seed(0)
    x = torch.rand(2, 3, 20, 24)
    out = T.RandomResizedCrop((16, 16), scale=(0.8, 0.9), interpolation=NEAREST)(x)
    assert out.shape == (2, 3, 16, 16) and set(out.flatten().tolist()) <= set(x.flatten().tolist())
    assert T.RandomResizedCrop(12)(x).shape == (2, 3, 12, 12)
    seg = torch.randint(0, 5, (4, 1, 24, 24)).float()
    out = T.ElasticTransform(alpha=100, sigma=2, interpolation=NEAREST)(seg)
    assert out.shape == seg.shape and set(out.unique().tolist()) <= {0., 1., 2., 3., 4.} and not torch.equal(out, seg)
    assert T.ElasticTransform()(torch.rand(2, 3, 21, 21)).shape == (2, 3, 21, 21)              # 41 taps: 20 < 21 rows
    with pytest.raises(RuntimeError):
        T.ElasticTransform()(x)                                # ... past 20 rows: torch's reflect padding refuses


# ---------------------------------------------------------------------------------------------- the port, the tables
def test_the_ugv_parking_block_builds_and_reduces_to_one_warp_table():
    choice = T.RandomChoice(ugv_parking_members())
    ops = T._native_ops(choice)
    assert [o.kind for o in ops] == ['RESIZED_CROP', 'ELASTIC'] and T._is_warp_table(ops)
    assert ops[0].p == dict(size=(84, 84), scale=(0.8, 0.9), ratio=(3 / 4, 4 / 3))
    assert ops[1].p == dict(alpha=(100., 100.), sigma=(5., 5.))
    from asac_amd import native
    fields, out = T._resolve_warp(ops[1], 84, 84)
    assert (fields['kind'], fields['k0'], fields['k1'], out) == (native.IMAGE_WARP_ELASTIC, 41, 41, (84, 84))
    assert T._resolve_warp(ops[1], 20, 84) is None, '41 taps reach past 20 rows'
    assert T._resolve_warp(T._native_ops(T.ElasticTransform(sigma=8, interpolation=NEAREST))[0], 84, 84) is None, '65 taps'
    assert T._resolve_warp(ops[0], 30, 40)[1] == (84, 84)
    # on the CPU it is module code
    torch.manual_seed(0)
    x = torch.randint(0, 4, (2, 3, 84, 84)).float()
    for _ in range(4):
        assert choice(x).shape == x.shape


def test_what_stays_module_code():
    rrc = lambda mode: T.RandomResizedCrop((24, 24), scale=(0.8, 0.9), interpolation=mode)    # noqa: E731
    ela = lambda mode: T.ElasticTransform(alpha=100, sigma=2, interpolation=mode)             # noqa: E731
    assert T._native_ops(rrc(BILINEAR)) is None and T._native_ops(ela(BILINEAR)) is None
    assert T._native_ops(T.RandomChoice([rrc(BILINEAR), ela(BILINEAR)])) is None
    assert T._native_ops(T.RandomChoice([rrc(NEAREST), ela(BILINEAR)])) is None
    assert T._native_ops(T.RandomChoice([rrc(NEAREST), T.GaussianBlur(3)])) is None, 'two entry points: no one launch'
    assert T._native_ops(T.RandomChoice([T.GaussianBlur(3), T.ColorJitter()])) is not None
    # a copy belongs to either table
    ops = T._native_ops(T.RandomChoice([ela(NEAREST), T.ColorJitter()]))
    assert [o.kind for o in ops] == ['ELASTIC', 'COPY'] and T._is_warp_table(ops)
    assert len(T._native_ops(T.RandomChoice([rrc(NEAREST)] * 9))) == 9      # (`_launch` turns a table over 8 members away)
    assert T.RandomChoice([rrc(NEAREST)] * 9)(torch.zeros(1, 1, 30, 30)).shape == (1, 1, 24, 24)


def test_arguments():
    with pytest.raises(NotImplementedError):
        T.ElasticTransform(fill=1)
    with pytest.raises(NotImplementedError):
        T.ElasticTransform(interpolation=InterpolationMode.BICUBIC)
    with pytest.raises(NotImplementedError):
        T.RandomResizedCrop(8, interpolation=InterpolationMode.BICUBIC)
    with pytest.raises(NotImplementedError):
        T.RandomResizedCrop(8, antialias=False)
    with pytest.raises(TypeError):
        T.RandomResizedCrop(8, scale=0.5)
    with pytest.raises(ValueError):
        T.RandomResizedCrop(8, scale=(0.9, 0.8))
    with pytest.raises(ValueError):
        T.RandomResizedCrop(8, ratio=(0., 1.))
    with pytest.raises(ValueError):
        T.RandomResizedCrop((8, 8, 8))
    with pytest.raises(TypeError):
        T.ElasticTransform(alpha='strong')
    with pytest.raises(ValueError):
        T.ElasticTransform(sigma=(1., 2., 3.))
    e = T.ElasticTransform(alpha=3, sigma=[2])
    assert e.alpha == (3., 3.) and e.sigma == (2., 2.) and e.interpolation == 'bilinear'
    r = T.RandomResizedCrop(8, interpolation='nearest')
    assert r.size == (8, 8) and r.scale == (0.08, 1.0) and r.ratio == (3 / 4, 4 / 3) and r.interpolation == 'nearest'
    assert {'RandomResizedCrop', 'ElasticTransform', 'resized_crop', 'get_resized_crop_params', 'elastic_displacement',
            'elastic'} <= set(T.__all__)
    for cls in (T.RandomResizedCrop, T.ElasticTransform):
        assert 'FROZEN' in cls.__doc__ and issubclass(cls, T._Launcher)


# ---------------------------------------------------------------------------------------------- surface
def test_surface():
    from asac_amd import abi, native
    assert native.ABI_VERSION == 91 and abi.defines['ASAC_ABI_VERSION'] == 91
    assert 'asac_image_warp' in abi.functions, 'asac_image_warp is not declared in include/asac_hip.h'
    assert len(native._SIGNATURES['asac_image_warp'][1]) == len(abi.functions['asac_image_warp'][1]) == 17
    assert 'asac_image_warp' in native.EXPORTED_SYMBOLS
    for name, value in (('ASAC_IMAGE_WARP_MAX_KERNEL', native.IMAGE_WARP_MAX_KERNEL), ('ASAC_IMAGE_WARP_COPY', native.IMAGE_WARP_COPY),
                        ('ASAC_IMAGE_WARP_RESIZED_CROP', native.IMAGE_WARP_RESIZED_CROP),
                        ('ASAC_IMAGE_WARP_ELASTIC', native.IMAGE_WARP_ELASTIC)):
        assert abi.defines[name] == value, name
    assert native.IMAGE_WARP_MAX_KERNEL == 63
    assert native.IMAGE_WARP_DRAWN == ('counter', 'choice', 'top', 'left', 'height', 'width')
    fields = [field for field, *_ in abi.structs['asac_image_warp_op_t']]
    assert fields == [n for n, _ in native.ImageWarpOp._fields_] and ctypes.sizeof(native.ImageWarpOp) == 4 * len(fields)
    # the existing entry point keeps its bits
    assert native.IMAGE_DRAWN == ('counter', 'choice', 'top', 'left', 'sigma', 'factor') and native.IMAGE_MAX_KERNEL == 31


def test_host_refusals_need_no_device():
    """a refused call returns hipErrorInvalidValue and names itself before anything touches a device: the pointers handed in
    here point nowhere"""
    from asac_amd import native
    lib = native.load()
    bad = 1                                                    # hipErrorInvalidValue
    fake = ctypes.c_void_p(4096)
    elastic = lambda **k: dict(dict(kind=native.IMAGE_WARP_ELASTIC, k0=41, k1=41, alpha0=100., alpha1=100., sigma0=5.,   # noqa: E731
                                    sigma1=5.), **k)
    rrc = lambda **k: dict(dict(kind=native.IMAGE_WARP_RESIZED_CROP, scale_lo=.8, scale_hi=.9, ratio_lo=.75,             # noqa: E731
                                ratio_hi=4 / 3), **k)

    def call(op=None, x=fake, y=fake, planes=6, C=3, H=30, W=30, Ho=30, Wo=30, n_ops=1, state=fake, ops='table'):
        table = native.warp_image_ops([op or elastic()])
        rc = lib.asac_image_warp(x, y, planes, C, H, W, Ho, Wo, table if ops == 'table' else None, n_ops, 0, 1, state,
                                 None, None, None, None)
        return rc, lib.asac_last_error()

    refused = [
        call(x=None), call(y=None), call(ops=None),
        call(elastic(k0=40)), call(elastic(k1=65)), call(elastic(k0=0)), call(elastic(k1=-3)),      # even, over 63, none
        call(elastic(), H=20, W=30, Ho=20, Wo=30), call(elastic(), H=30, W=20, Ho=30, Wo=20),       # k // 2 >= an extent
        call(elastic(sigma0=0.)), call(elastic(sigma1=-1.)), call(elastic(sigma0=float('nan'))),
        call(elastic(alpha1=float('inf'))),
        call(H=97, W=96, Ho=97, Wo=96), call(rrc(), H=1, W=native.IMAGE_MAX_PLANE + 1),
        call(elastic(), Ho=31), call(dict(kind=native.IMAGE_WARP_COPY), Wo=29),                     # only the crop resizes
        call(rrc(scale_lo=0.)), call(rrc(scale_lo=.9, scale_hi=.8)), call(rrc(ratio_lo=0.)), call(rrc(ratio_lo=2., ratio_hi=1.)),
        call(rrc(scale_hi=float('inf'))), call(rrc(ratio_hi=float('nan'))),
        call(n_ops=0), call(n_ops=9), call(planes=0), call(planes=7), call(dict(kind=3)), call(dict(kind=-1)),
        call(elastic(), state=None), call(rrc(), state=None),                                       # draws without a counter
    ]
    for i, (rc, msg) in enumerate(refused):
        assert rc == bad and b'asac_image_warp' in msg, (i, rc, msg)
    assert b'ASAC_IMAGE_MAX_PLANE' in call(H=97, W=96, Ho=97, Wo=96)[1]
    assert b'ASAC_IMAGE_WARP_MAX_KERNEL' in call(elastic(k1=65))[1]
    with pytest.raises(AssertionError):
        native.warp_image_ops([dict(kind=0)] * 9)
