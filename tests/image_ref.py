"""float64 evaluations of the definitions `algorithm/utils/image_transforms.py` states, written out in NumPy: what the
module code and the launches of csrc/image.hip are compared with (tests/test_image_transforms_host.py, ..._gpu.py)."""
import numpy as np


def kernel1d(k, sigma):
    x = np.linspace(-(k - 1) / 2, (k - 1) / 2, k, dtype=np.float64)
    w = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return w / w.sum()


def reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur(x, kx, ky, sigma):
    """x [..., H, W] -> separable float64 sums with reflect indexing (no padded copy)"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    wx, wy = kernel1d(kx, sigma), kernel1d(ky, sigma)
    cols = np.arange(W)
    h = np.zeros_like(x)
    for j in range(kx):
        h += wx[j] * x[..., :, reflect(cols + j - kx // 2, W)]
    rows = np.arange(H)
    out = np.zeros_like(x)
    for j in range(ky):
        out += wy[j] * h[..., reflect(rows + j - ky // 2, H), :]
    return out


def _axis(n_out, n_in):
    src = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(src).astype(np.int64)
    lam = src - i0
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), lam


def resize(x, Ho, Wo):
    """bilinear, align_corners=False: src = (dst + 0.5) in / out - 0.5, neighbours clamped to the frame"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    y0, y1, ly = _axis(Ho, H)
    x0, x1, lx = _axis(Wo, W)
    ly = ly[:, None]
    top = x[..., y0, :][..., :, x0] * (1 - lx) + x[..., y0, :][..., :, x1] * lx
    bot = x[..., y1, :][..., :, x0] * (1 - lx) + x[..., y1, :][..., :, x1] * lx
    return top * (1 - ly) + bot * ly


def brightness(x, f):
    return np.clip(np.asarray(x, dtype=np.float64) * float(f), 0., 1.)
