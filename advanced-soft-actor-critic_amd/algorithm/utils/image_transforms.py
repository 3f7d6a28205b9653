"""Image augmentations for the siamese / BYOL views of a model plugin: the torchvision transform classes the reference's
plugin files use, as `nn.Module`s on tensors `[..., C, H, W]`.  A plugin file is ported by one line:

    from algorithm.utils import image_transforms as T

Names, argument names, defaults and what is drawn per call follow torchvision's v2 tensor path.  Each class has two paths.

MODULE CODE: plain torch ops with the draws made on the host, as torchvision makes them.  It is the CPU implementation and
what runs for anything the kernel does not take (other dtypes, inputs that require grad, planes over
`native.IMAGE_MAX_PLANE` pixels, a blur whose radius reaches past the plane, a resize that shrinks).

ONE LAUNCH (`asac_image_augment`, csrc/image.hip): float32 CUDA tensors.  The draws are made on the device from a counter in
device memory the instance owns, so a step captured into a graph (`CapturedStep`) draws afresh on every replay; `drawn()`
reports what the last call drew.  `RandomResizedCrop` and `ElasticTransform` with NEAREST interpolation, and a `RandomChoice`
among them, are one launch of a second entry point (`asac_image_warp`) with the same draw protocol and its own `drawn()`
record (counter, choice, top, left, height, width); BILINEAR, a field whose blur has over 63 taps or reaches past the plane,
and a choice that mixes them with the ops above stay module code.

WARNING, captured steps: a module-code draw (`RandomChoice`'s pick, `RandomCrop`'s offsets, a sigma or brightness range, a
resized crop's window, an elastic displacement field) is a host value.  Captured into a graph it is FROZEN: every replay
applies the same member with the same parameters, and nothing reports it.  Inside a captured step keep to what `_native_ops`
reduces to a launch."""
import enum
import itertools
import math
from collections.abc import Sequence

import torch
from torch import nn
from torch.nn import functional as F

from . import transform as _noise

__all__ = ['GaussianBlur', 'ColorJitter', 'RandomCrop', 'Resize', 'RandomResizedCrop', 'ElasticTransform', 'RandomChoice',
           'Compose', 'InterpolationMode', 'gaussian_kernel1d', 'gaussian_blur', 'adjust_brightness', 'crop', 'resize',
           'resized_crop', 'get_resized_crop_params', 'elastic_displacement', 'elastic']


class InterpolationMode(enum.Enum):
    NEAREST = 'nearest'
    NEAREST_EXACT = 'nearest-exact'
    BILINEAR = 'bilinear'
    BICUBIC = 'bicubic'


def _pair(v, what):
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return (v, v)
    if isinstance(v, Sequence) and len(v) == 1:
        return (v[0], v[0])
    if isinstance(v, Sequence) and len(v) == 2:
        return (v[0], v[1])
    raise ValueError(f'{what} should be a number or a pair, got {v!r}')


def _frames(x):
    """[..., C, H, W] -> (leading shape, [N, C, H, W])"""
    if not isinstance(x, torch.Tensor):
        raise TypeError('image transforms take torch tensors (PIL images need torchvision, which the training path does not use)')
    if x.dim() < 3:
        raise ValueError(f'expected [..., C, H, W], got {tuple(x.shape)}')
    return x.shape[:-3], x.reshape(-1, *x.shape[-3:])


# ------------------------------------------------------------------------------------------------
# the definitions, as functions of drawn parameters (module code)
# ------------------------------------------------------------------------------------------------
def gaussian_kernel1d(k: int, sigma: float, dtype=torch.float32, device=None):
    """w = exp(-0.5 (x / sigma)^2) over x = linspace(-(k - 1) / 2, (k - 1) / 2, k), normalised"""
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=dtype, device=device)
    w = torch.exp(-0.5 * (x / sigma).pow(2))
    return w / w.sum()


def gaussian_blur(x, kernel_size, sigma):
    """reflect padding k // 2, then the depthwise product with the outer product of the two 1-D kernels; `sigma`: a float,
    or the pair (along x, along y)"""
    kx, ky = kernel_size
    sx, sy = _pair(sigma, 'sigma')
    lead, f = _frames(x)
    dtype = f.dtype if f.is_floating_point() else torch.float32
    w2 = torch.outer(gaussian_kernel1d(ky, sy, dtype, f.device), gaussian_kernel1d(kx, sx, dtype, f.device))
    C = f.shape[1]
    padded = F.pad(f.to(dtype), [kx // 2, kx // 2, ky // 2, ky // 2], mode='reflect')
    out = F.conv2d(padded, w2.expand(C, 1, ky, kx), groups=C)
    if not f.is_floating_point():
        out = out.round().to(f.dtype)
    return out.reshape(*lead, *out.shape[1:])


def adjust_brightness(x, factor: float):
    return (x * factor).clamp(0, 1)


def crop(x, top: int, left: int, height: int, width: int):
    return x[..., top:top + height, left:left + width]


def _resize_shape(size, H, W):
    if isinstance(size, int):
        short, long_ = (H, W) if H <= W else (W, H)
        new_long = int(size * long_ / short)
        return (size, new_long) if H <= W else (new_long, size)
    return tuple(size)


def resize(x, size):
    """bilinear, align_corners=False, antialias=True; `size`: an int (the shorter side) or (h, w)"""
    lead, f = _frames(x)
    out_hw = _resize_shape(size, f.shape[-2], f.shape[-1])
    if out_hw == tuple(f.shape[-2:]):
        return x
    out = F.interpolate(f, size=out_hw, mode='bilinear', align_corners=False, antialias=True)
    return out.reshape(*lead, *out.shape[1:])


def _interpolation(value, who):
    """-> 'nearest' | 'bilinear' (the two the warps take)"""
    if value in (InterpolationMode.NEAREST, 'nearest', 0):
        return 'nearest'
    if value in (InterpolationMode.BILINEAR, 'bilinear', 2):
        return 'bilinear'
    raise NotImplementedError(f'{who}: interpolation {value!r} is not supported')


def resized_crop(x, top: int, left: int, height: int, width: int, size, interpolation=InterpolationMode.BILINEAR):
    """the window, resampled to `size` (h, w).  NEAREST: torch's legacy rule src = min(floor(dst * in / out), in - 1), no
    antialiasing; BILINEAR: as `resize`"""
    mode = _interpolation(interpolation, 'resized_crop')
    lead, f = _frames(crop(x, top, left, height, width))
    size = tuple(int(s) for s in _pair(size, 'size'))
    if mode == 'nearest':
        dtype = f.dtype
        out = F.interpolate(f if f.is_floating_point() else f.to(torch.float32), size=size, mode='nearest').to(dtype)
    else:
        out = F.interpolate(f, size=size, mode='bilinear', align_corners=False, antialias=True)
    return out.reshape(*lead, *out.shape[1:])


def get_resized_crop_params(H: int, W: int, scale, ratio):
    """torchvision's RandomResizedCrop.get_params, host draws -> (top, left, height, width)"""
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    area = H * W
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect = math.exp(torch.empty(1).uniform_(log_lo, log_hi).item())
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            top = int(torch.randint(0, H - h + 1, size=()))
            left = int(torch.randint(0, W - w + 1, size=()))
            return top, left, h, w
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def elastic_displacement(noise, alpha, sigma):
    """noise [2, H, W] in [-1, 1) -> the displacement [H, W, 2] in grid units (torchvision's ElasticTransform._get_params):
    field 0 moves along x, field 1 along y; each is blurred with k = int(8 * its sigma + 1) taps (made odd) on BOTH axes and
    the sigma PAIR, then scaled by alpha[0] / H resp. alpha[1] / W — torchvision divides x by the height, y by the width"""
    alpha, sigma = _pair(alpha, 'alpha'), _pair(sigma, 'sigma')
    H, W = noise.shape[-2:]
    fields = []
    for i, n in enumerate((H, W)):
        d = noise[i][None, None]
        if sigma[i] > 0.:
            k = _elastic_taps(sigma)[i]
            d = gaussian_blur(d, [k, k], sigma)
        fields.append(d[0, 0] * alpha[i] / n)
    return torch.stack(fields, dim=-1)


def elastic(x, displacement, interpolation=InterpolationMode.BILINEAR):
    """`grid_sample` at the identity grid plus `displacement` [H, W, 2] (zeros outside, align_corners=False): ONE field for
    every frame and channel of the call"""
    mode = _interpolation(interpolation, 'elastic')
    lead, f = _frames(x)
    H, W = f.shape[-2:]
    dtype = f.dtype
    if not f.is_floating_point():
        f = f.to(torch.float32)
    gx = torch.linspace((-W + 1) / W, (W - 1) / W, W, dtype=f.dtype, device=f.device)
    gy = torch.linspace((-H + 1) / H, (H - 1) / H, H, dtype=f.dtype, device=f.device)
    identity = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W)], dim=-1)
    grid = (identity + displacement.to(f)).expand(f.shape[0], H, W, 2)
    out = F.grid_sample(f, grid, mode=mode, padding_mode='zeros', align_corners=False)
    if out.dtype != dtype:
        out = out.round().to(dtype)
    return out.reshape(*lead, *out.shape[1:])


# ------------------------------------------------------------------------------------------------
# the launch
# ------------------------------------------------------------------------------------------------
class _Op:
    """one member of a launch's table before the frame's size is known"""
    __slots__ = ('kind', 'p')

    def __init__(self, kind, **p):
        self.kind, self.p = kind, p

    def __repr__(self):
        return f'_Op({self.kind}, {self.p})'

    def __eq__(self, other):
        return isinstance(other, _Op) and (self.kind, self.p) == (other.kind, other.p)


def _draws(fields, H, W) -> bool:
    """whether a resolved member asks the device for a draw (the entry point's own rule)"""
    from asac_amd import native
    kind = fields['kind']
    if kind in (native.IMAGE_BLUR, native.IMAGE_BRIGHTNESS):
        return fields['hi'] > fields['lo']
    if kind == native.IMAGE_CROP_RESIZE:
        return fields['crop_h'] < H or fields['crop_w'] < W
    return kind in (native.IMAGE_SALT_PEPPER, native.IMAGE_UNIFORM_NOISE)


def _resolve(op, H, W):
    """-> (fields of native.ImageOp, (Ho, Wo)) for an [H, W] frame, or None where the kernel does not take it"""
    from asac_amd import native
    k, p = op.kind, op.p
    if k == 'BLUR':
        kx, ky = p['kernel_size']
        if kx // 2 >= W or ky // 2 >= H:           # (the module code raises, as torch's reflect padding does)
            return None
        return dict(kind=native.IMAGE_BLUR, kx=kx, ky=ky, lo=p['sigma'][0], hi=p['sigma'][1]), (H, W)
    if k == 'BRIGHTNESS':
        return dict(kind=native.IMAGE_BRIGHTNESS, lo=p['factor'][0], hi=p['factor'][1]), (H, W)
    if k == 'CROP_RESIZE':
        ch, cw = p['crop'] if p['crop'] is not None else (H, W)
        if ch > H or cw > W:
            return None
        out = _resize_shape(p['size'], ch, cw) if p['size'] is not None else (ch, cw)
        if out[0] < ch or out[1] < cw:             # a shrinking resize needs the antialiasing filter: module code
            return None
        return dict(kind=native.IMAGE_CROP_RESIZE, crop_h=ch, crop_w=cw), out
    if k == 'SALT_PEPPER':
        half = (1 - p['p']) / 2.
        return dict(kind=native.IMAGE_SALT_PEPPER, a=p['snr'], b=half, c=half + p['p']), (H, W)
    if k == 'UNIFORM_NOISE':
        return dict(kind=native.IMAGE_UNIFORM_NOISE, a=p['mean'], b=p['std']), (H, W)
    if k == 'COPY':
        return dict(kind=native.IMAGE_COPY), (H, W)
    raise AssertionError(k)


_WARP_KINDS = ('RESIZED_CROP', 'ELASTIC')


def _is_warp_table(ops) -> bool:
    """a table for `asac_image_warp`: every member a warp or a copy, at least one a warp"""
    return any(op.kind in _WARP_KINDS for op in ops) and all(op.kind in _WARP_KINDS or op.kind == 'COPY' for op in ops)


def _elastic_taps(sigma):
    """torchvision's kernel sizes of the two fields: int(8 sigma + 1), made odd"""
    taps = []
    for s in sigma:
        k = int(8 * s + 1)
        taps.append(k + 1 - k % 2)
    return taps


def _resolve_warp(op, H, W):
    """-> (fields of native.ImageWarpOp, (Ho, Wo)) for an [H, W] frame, or None where the kernel does not take it"""
    from asac_amd import native
    k, p = op.kind, op.p
    if k == 'RESIZED_CROP':
        (s0, s1), (r0, r1) = p['scale'], p['ratio']
        return dict(kind=native.IMAGE_WARP_RESIZED_CROP, scale_lo=s0, scale_hi=s1, ratio_lo=r0, ratio_hi=r1), tuple(p['size'])
    if k == 'ELASTIC':
        sigma = p['sigma']
        if min(sigma) <= 0.:                                # (a field without a blur: module code)
            return None
        k0, k1 = _elastic_taps(sigma)
        if max(k0, k1) > native.IMAGE_WARP_MAX_KERNEL or max(k0, k1) // 2 >= min(H, W):
            return None
        return dict(kind=native.IMAGE_WARP_ELASTIC, k0=k0, k1=k1, alpha0=p['alpha'][0], alpha1=p['alpha'][1], sigma0=sigma[0],
                    sigma1=sigma[1]), (H, W)
    if k == 'COPY':
        return dict(kind=native.IMAGE_WARP_COPY), (H, W)
    raise AssertionError(k)


_instance_ids = itertools.count(1)


class _Launcher(nn.Module):
    """What a class needs to run as one launch: its instance id in the Philox stream, the seed, and per device the 16-byte
    draw state and the record of the last call's draws.  The tensors are plain attributes created at the first launch on a
    device (no buffers: a plugin's state_dict keeps the reference's keys)."""

    def __init__(self):
        super().__init__()
        self.instance_id = next(_instance_ids)
        self.seed = None                   # None: torch.initial_seed() at the first launch
        self._device_state = {}            # device -> (state int64 [2], drawn float64 [6])
        self._tables = {}                  # (H, W) -> (ctypes table, (Ho, Wo), whether it draws) | None
        self._last_device = None
        self._last_warp = False            # whether the last launch was `asac_image_warp` (its own `drawn` record)
        # (noise, displacement): two float32 [2, H, W] tensors on the device that an elastic call's field is copied to, for
        # tests and inspection; None, None: not kept
        self._field_out = (None, None)
        self._counter0 = 0

    def reseed(self, seed: int, counter: int = 0, instance_id: int | None = None):
        """the stream of draws is a function of (seed, instance id, counter): re-seat all three"""
        self.seed = int(seed)
        if instance_id is not None:
            self.instance_id = int(instance_id)
        self.set_counter(counter)
        return self

    def set_counter(self, counter: int):
        for state, _ in self._device_state.values():
            state.copy_(torch.tensor([int(counter), 0], dtype=torch.int64))
        self._counter0 = int(counter)     # (for a device first launched on later)

    def _state(self, device):
        got = self._device_state.get(device)
        if got is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'{type(self).__name__}: the first launch on a device creates the draw counter and cannot '
                                   'be part of a capture (a captured fill would reset it on every replay): call once before')
            state = torch.tensor([self._counter0, 0], dtype=torch.int64, device=device)
            drawn = torch.full((6,), float('nan'), dtype=torch.float64, device=device)
            got = self._device_state[device] = (state, drawn)
        return got

    def drawn(self) -> dict:
        """what the last launch drew: counter, choice, top, left (-1: none), sigma, factor (NaN: none); after a warp launch
        counter, choice, top, left, height, width (-1: none).  Synchronises."""
        from asac_amd import native
        if self._last_device is None:
            raise RuntimeError('no launch yet')
        rec = self._device_state[self._last_device][1].tolist()
        if self._last_warp:                # a warp table's record: counter, choice, top, left, height, width (-1: none)
            return {k: int(v) for k, v in zip(native.IMAGE_WARP_DRAWN, rec)}
        out = dict(zip(native.IMAGE_DRAWN, rec))
        for k in ('counter', 'choice', 'top', 'left'):
            out[k] = int(out[k])
        return out

    def counter_state(self):
        """(draw counter, arrival word) of the device last launched on.  Synchronises."""
        state = self._device_state[self._last_device][0]
        c, a = state.tolist()
        return c, a & 0xFFFFFFFF

    def _launch(self, ops, x):
        """x through the table `ops` as one launch, or None where the module code has to run"""
        if (ops is None or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() < 3
                or x.requires_grad and torch.is_grad_enabled()):
            return None
        from asac_amd import native
        H, W = x.shape[-2:]
        if H * W > native.IMAGE_MAX_PLANE or x.numel() == 0 or len(ops) > native.IMAGE_MAX_OPS:
            return None
        warp = _is_warp_table(ops)
        if (H, W) not in self._tables:
            resolved = [(_resolve_warp if warp else _resolve)(op, H, W) for op in ops]
            if any(r is None for r in resolved) or len({r[1] for r in resolved}) != 1:
                self._tables[(H, W)] = None        # a member outside the kernel's limits, or members of different sizes
            elif warp:                             # (every warp table draws)
                self._tables[(H, W)] = (native.warp_image_ops([r[0] for r in resolved]), resolved[0][1], True)
            else:
                # (a table that draws nothing launches without the counter: no workgroup arrives anywhere)
                draws = len(resolved) > 1 or any(_draws(r[0], H, W) for r in resolved)
                self._tables[(H, W)] = (native.image_ops([r[0] for r in resolved]), resolved[0][1], draws)
        if self._tables[(H, W)] is None:
            return None
        table, (Ho, Wo), draws = self._tables[(H, W)]
        lead, f = _frames(x)
        f = f.contiguous()
        state, drawn = self._state(x.device)
        if self.seed is None:
            self.seed = torch.initial_seed()
        y = torch.empty(*f.shape[:2], Ho, Wo, dtype=torch.float32, device=x.device)
        if warp:
            native.warp_image(f, y, table, self.seed, self.instance_id, state, drawn, *self._field_out)
        else:
            native.image_augment(f, y, table, self.seed, self.instance_id, state if draws else None, drawn)
        self._last_device, self._last_warp = x.device, warp
        return y.reshape(*lead, *y.shape[1:])


def _native_ops(transform):
    """The table a transform runs as ONE launch with: a list of `_Op` (one entry: that op; several: a device-drawn choice),
    or None where it does not reduce to one."""
    from ..nn_models.layers.image_layers import Transform
    if isinstance(transform, Transform):
        return _native_ops(transform.transform) if transform.transform is not None else None
    if isinstance(transform, GaussianBlur):
        return [_Op('BLUR', kernel_size=transform.kernel_size, sigma=transform.sigma)]
    if isinstance(transform, ColorJitter):
        return [_Op('BRIGHTNESS', factor=transform.brightness)] if transform.brightness is not None else [_Op('COPY')]
    if isinstance(transform, RandomCrop):
        return [_Op('CROP_RESIZE', crop=transform.size, size=None)]
    if isinstance(transform, Resize):
        return [_Op('CROP_RESIZE', crop=None, size=transform.size)]
    if isinstance(transform, RandomResizedCrop):
        if transform.interpolation != 'nearest':            # (the antialiased bilinear resize: module code)
            return None
        return [_Op('RESIZED_CROP', size=transform.size, scale=transform.scale, ratio=transform.ratio)]
    if isinstance(transform, ElasticTransform):
        if transform.interpolation != 'nearest':
            return None
        return [_Op('ELASTIC', alpha=transform.alpha, sigma=transform.sigma)]
    if type(transform) is _noise.SaltAndPepperNoise:
        return [_Op('SALT_PEPPER', snr=float(transform.snr), p=float(transform.p))]
    if type(transform) is _noise.GaussianNoise:
        return [_Op('UNIFORM_NOISE', mean=float(transform.mean), std=float(transform.std))]
    if isinstance(transform, (Compose, nn.Sequential)):
        members = list(transform.transforms) if isinstance(transform, Compose) else list(transform)
        if len(members) == 1:
            return _native_ops(members[0])
        if len(members) == 2:
            first, second = (_native_ops(t) for t in members)
            if (first is not None and second is not None and len(first) == len(second) == 1
                    and first[0].kind == second[0].kind == 'CROP_RESIZE'
                    and first[0].p['size'] is None and second[0].p['crop'] is None):
                return [_Op('CROP_RESIZE', crop=first[0].p['crop'], size=second[0].p['size'])]
        return None
    if isinstance(transform, RandomChoice):
        table = []
        for t in transform.transforms:
            ops = _native_ops(t)
            if ops is None or len(ops) != 1:
                return None
            table.append(ops[0])
        # the warps are another entry point: a choice between them and the ops of `asac_image_augment` is no one launch
        if any(op.kind in _WARP_KINDS for op in table) and not _is_warp_table(table):
            return None
        return table if table else None
    return None


# ------------------------------------------------------------------------------------------------
# the classes
# ------------------------------------------------------------------------------------------------
class GaussianBlur(_Launcher):
    """Blurs with a Gaussian kernel: `kernel_size` an odd int or (kx, ky), at most 31; `sigma` a float or a range (lo, hi)
    one sigma is drawn from uniformly per call.  Module-code draws are frozen inside a captured step (see the module)."""

    def __init__(self, kernel_size, sigma=(0.1, 2.0)):
        super().__init__()
        self.kernel_size = tuple(int(k) for k in _pair(kernel_size, 'kernel_size'))
        for k in self.kernel_size:
            if k <= 0 or k % 2 == 0:
                raise ValueError('Kernel size value should be an odd and positive number.')
            if k > 31:
                raise ValueError('kernel_size is limited to 31')
        lo, hi = (float(s) for s in _pair(sigma, 'sigma'))
        if not 0. < lo <= hi:
            raise ValueError('sigma values should be positive and of the form (min, max).')
        self.sigma = (lo, hi)

    def forward(self, x):
        y = self._launch(_native_ops(self), x)
        if y is not None:
            return y
        lo, hi = self.sigma
        sigma = lo if lo == hi else torch.empty(1).uniform_(lo, hi).item()
        return gaussian_blur(x, self.kernel_size, sigma)

    def extra_repr(self):
        return f'kernel_size={self.kernel_size}, sigma={self.sigma}'


class ColorJitter(_Launcher):
    """Brightness only: clamp(x * f, 0, 1) with one f per call from [max(0, 1 - b), 1 + b] (a float b) or from the pair
    given.  Module-code draws are frozen inside a captured step (see the module)."""

    def __init__(self, brightness=None, contrast=None, saturation=None, hue=None):
        super().__init__()
        for name, value in (('contrast', contrast), ('saturation', saturation), ('hue', hue)):
            if value is not None and value != 0 and value != (0, 0):
                raise NotImplementedError(f'ColorJitter: {name} is not supported')
        self.brightness = self._range(brightness)

    @staticmethod
    def _range(value):
        if value is None:
            return None
        if isinstance(value, (int, float)):
            if value < 0:
                raise ValueError('If brightness is a single number, it must be non negative.')
            value = (max(0., 1. - float(value)), 1. + float(value))
        else:
            value = tuple(float(v) for v in _pair(value, 'brightness'))
        if not 0. <= value[0] <= value[1]:
            raise ValueError(f'brightness values should be between (0, inf), got {value}')
        return None if value == (1., 1.) else value

    def forward(self, x):
        if self.brightness is None:
            return x
        y = self._launch(_native_ops(self), x)
        if y is not None:
            return y
        lo, hi = self.brightness
        return adjust_brightness(x, lo if lo == hi else torch.empty(1).uniform_(lo, hi).item())

    def extra_repr(self):
        return f'brightness={self.brightness}'


class RandomCrop(_Launcher):
    """A `size` window at one (top, left) per call, uniform over the valid offsets.  Module-code draws are frozen inside a
    captured step (see the module)."""

    def __init__(self, size, padding=None, pad_if_needed=False, fill=0, padding_mode='constant'):
        super().__init__()
        for name, value, default in (('padding', padding, None), ('pad_if_needed', pad_if_needed, False), ('fill', fill, 0),
                                     ('padding_mode', padding_mode, 'constant')):
            if value != default:
                raise NotImplementedError(f'RandomCrop: {name} is not supported')
        self.size = tuple(int(s) for s in _pair(size, 'size'))

    def forward(self, x):
        y = self._launch(_native_ops(self), x)
        if y is not None:
            return y
        H, W = x.shape[-2:]
        h, w = self.size
        if h > H or w > W:
            raise ValueError(f'Required crop size {(h, w)} is larger than input image size {(H, W)}')
        top = int(torch.randint(0, H - h + 1, size=()))
        left = int(torch.randint(0, W - w + 1, size=()))
        return crop(x, top, left, h, w)

    def extra_repr(self):
        return f'size={self.size}'


class Resize(_Launcher):
    """Bilinear (align_corners=False, antialias=True) to `size`: an int (the shorter side) or (h, w).  A launch where
    nothing shrinks (antialiasing is a no-op there), module code otherwise."""

    def __init__(self, size, interpolation=InterpolationMode.BILINEAR, max_size=None, antialias=True):
        super().__init__()
        if interpolation not in (InterpolationMode.BILINEAR, 'bilinear', 2):
            raise NotImplementedError(f'Resize: interpolation {interpolation!r} is not supported')
        if max_size is not None:
            raise NotImplementedError('Resize: max_size is not supported')
        if antialias is not True:
            raise NotImplementedError('Resize: antialias=False is not supported')
        self.size = int(size) if isinstance(size, int) else tuple(int(s) for s in _pair(size, 'size'))

    def forward(self, x):
        y = self._launch(_native_ops(self), x)
        return y if y is not None else resize(x, self.size)

    def extra_repr(self):
        return f'size={self.size}'


class RandomResizedCrop(_Launcher):
    """A window of a random share `scale` of the frame's area and a random aspect `ratio` (log-uniform), one per call
    (`get_resized_crop_params`), resampled to `size`.  NEAREST is one launch with the window drawn on the device; BILINEAR
    (antialiased) is module code, whose host draws are FROZEN inside a captured step (see the module)."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), interpolation=InterpolationMode.BILINEAR, antialias=True):
        super().__init__()
        self.size = tuple(int(s) for s in _pair(size, 'size'))
        if min(self.size) < 1:
            raise ValueError(f'size should be positive, got {self.size}')
        if not (isinstance(scale, Sequence) and isinstance(ratio, Sequence)):
            raise TypeError('Scale and ratio should be sequences')
        self.scale = tuple(float(s) for s in _pair(scale, 'scale'))
        self.ratio = tuple(float(r) for r in _pair(ratio, 'ratio'))
        if not (0. < self.scale[0] <= self.scale[1] and 0. < self.ratio[0] <= self.ratio[1]):
            raise ValueError('scale and ratio should be positive and of the form (min, max)')
        self.interpolation = _interpolation(interpolation, 'RandomResizedCrop')
        if antialias is not True and self.interpolation == 'bilinear':
            raise NotImplementedError('RandomResizedCrop: antialias=False is not supported')

    def forward(self, x):
        y = self._launch(_native_ops(self), x)
        if y is not None:
            return y
        top, left, h, w = get_resized_crop_params(x.shape[-2], x.shape[-1], self.scale, self.ratio)
        return resized_crop(x, top, left, h, w, self.size, self.interpolation)

    def extra_repr(self):
        return f'size={self.size}, scale={self.scale}, ratio={self.ratio}, interpolation={self.interpolation}'


class ElasticTransform(_Launcher):
    """Moves every pixel by one smooth random displacement field per call (`elastic_displacement` of uniform noise, strength
    `alpha`, smoothness `sigma`: floats or (x, y) pairs), shared by all frames and channels of the call, zeros outside.
    NEAREST is one launch with the field drawn on the device; BILINEAR is module code, whose host-drawn field is FROZEN inside
    a captured step (see the module)."""

    def __init__(self, alpha=50.0, sigma=5.0, interpolation=InterpolationMode.BILINEAR, fill=0):
        super().__init__()
        if fill not in (0, 0., None):
            raise NotImplementedError('ElasticTransform: fill is not supported')
        for name, value in (('alpha', alpha), ('sigma', sigma)):
            if isinstance(value, bool) or not isinstance(value, (int, float, Sequence)) or isinstance(value, str):
                raise TypeError(f'{name} should be a number or a sequence of numbers')
        self.alpha = tuple(float(a) for a in _pair(alpha, 'alpha'))
        self.sigma = tuple(float(s) for s in _pair(sigma, 'sigma'))
        self.interpolation = _interpolation(interpolation, 'ElasticTransform')

    def forward(self, x):
        y = self._launch(_native_ops(self), x)
        if y is not None:
            return y
        H, W = x.shape[-2:]
        noise = (torch.rand(2, H, W) * 2 - 1).to(x.device)
        return elastic(x, elastic_displacement(noise, self.alpha, self.sigma), self.interpolation)

    def extra_repr(self):
        return f'alpha={self.alpha}, sigma={self.sigma}, interpolation={self.interpolation}'


class Compose(_Launcher):
    """The transforms in turn.  An adjacent `RandomCrop, Resize` pair runs as one launch."""

    def __init__(self, transforms):
        super().__init__()
        if not isinstance(transforms, Sequence) or not transforms:
            raise TypeError('Argument transforms should be a non-empty sequence of callables')
        self.transforms = list(transforms)
        for i, t in enumerate(self.transforms):
            if isinstance(t, nn.Module):
                self.add_module(str(i), t)

    def forward(self, x):
        y = self._launch(_native_ops(self), x)
        if y is not None:
            return y
        for t in self.transforms:
            x = t(x)
        return x


class RandomChoice(_Launcher):
    """One member per call, uniformly.  Where every member reduces to one op (`_native_ops`) the call is one launch and the
    member is drawn on the device; otherwise the pick is a host draw, FROZEN inside a captured step (see the module)."""

    def __init__(self, transforms, p=None):
        super().__init__()
        if not isinstance(transforms, Sequence) or not transforms:
            raise TypeError('Argument transforms should be a non-empty sequence of callables')
        if p is not None:
            raise NotImplementedError('RandomChoice: p is not supported')
        self.transforms = list(transforms)
        for i, t in enumerate(self.transforms):
            if isinstance(t, nn.Module):
                self.add_module(str(i), t)

    def forward(self, x):
        y = self._launch(_native_ops(self), x)
        if y is not None:
            return y
        return self.transforms[int(torch.randint(0, len(self.transforms), size=()))](x)
