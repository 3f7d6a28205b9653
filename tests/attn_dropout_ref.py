"""Restatements the attention-dropout tests compare against (no test compares anything with torch's own dropout draws):

* Philox4x32-10 in NumPy and the draw layout of csrc/asac_dropout.h as `k_attn_mh` uses it — `mask(...)`;
* the multi-head attention core with the mask as an INPUT, in float64 torch, gradients by autograd — `core(...)`;
* a `MultiheadAttention` around that core (`module_forward`), for the parameter gradients.
"""
import math

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
DROP_TAG = 5
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two uint32 -> four uint32 arrays"""
    c = [np.asarray(w, dtype=np.uint64) & U32 for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & U32, p1 & U32,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & U32, p0 & U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def threshold(p: float) -> int:
    """an element is DROPPED iff its 32-bit word is below floor(p * 2^32) (float64)"""
    return int(math.floor(float(p) * 4294967296.0))


def scale(p: float) -> float:
    """float32(1 / (1 - p)), the quotient formed in double precision"""
    return float(np.float32(1.0 / (1.0 - float(p))))


def words(seed, instance, counter, B, H, Lq, Lk):
    """uint32 [B, H, Lq, Lk]: entry (b, h, i, j) is word j & 3 of block ((b H + h) 32 + i) 8 + (j >> 2)"""
    assert B * H <= 1 << 24 and Lq <= 32 and Lk <= 32
    b, h, i, j4 = np.meshgrid(np.arange(B), np.arange(H), np.arange(Lq), np.arange((Lk + 3) // 4), indexing='ij')
    index = ((b * H + h) * 32 + i) * 8 + j4
    second = (DROP_TAG << 28) | (int(instance) & 0x0FFFFFFF)
    counter, seed = int(counter) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    out = philox4x32_10((index, second, counter & 0xFFFFFFFF, counter >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1).reshape(B, H, Lq, -1)[..., :Lk]      # [B, H, Lq, 4 * blocks] -> the window's keys


def mask(seed, instance, counter, B, H, Lq, Lk, p):
    """bool [B, H, Lq, Lk], True = KEPT: the entry's word is >= floor(p * 2^32)"""
    assert 0. < p < 1.
    return words(seed, instance, counter, B, H, Lq, Lk) >= np.uint32(threshold(p))


def blocked_mask(B, Lq, Lk, attn_mask=None, key_padding_mask=None):
    """bool [B, Lq, Lk] (True = blocked) of the module's two masks, or None"""
    m = None
    if attn_mask is not None:
        m = attn_mask if attn_mask.dim() == 3 else attn_mask.unsqueeze(0).expand(B, -1, -1)
    if key_padding_mask is not None:
        kpm = key_padding_mask.unsqueeze(1).expand(-1, Lq, -1)
        m = kpm if m is None else m | kpm
    return m


def core(q, k, v, heads, blocked, kept, p):
    """float64 q [B, Lq, E], k / v [B, Lk, E]; blocked bool [B, Lq, Lk] or None; kept bool [B, H, Lq, Lk]
    -> (out [B, Lq, E], weights [B, Lq, Lk] = mean over the heads of the DROPPED softmax * keep, keep [B, Lq])"""
    B, Lq, E = q.shape
    Lk, d = k.shape[1], E // heads
    split = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)      # noqa: E731  [B, H, L, d]
    s = split(q) @ split(k).transpose(-1, -2) / math.sqrt(d)
    keep = torch.ones(B, Lq, dtype=q.dtype)
    if blocked is not None:
        dead = blocked.all(-1)                                             # nothing to attend to: the row attends unmasked
        s = s.masked_fill((blocked & ~dead.unsqueeze(-1)).unsqueeze(1), float('-inf'))
        keep = (~dead).to(q.dtype)
    P = torch.softmax(s, dim=-1)
    Pd = P * torch.as_tensor(kept, dtype=q.dtype) * scale(p)
    out = (Pd @ split(v)).permute(0, 2, 1, 3).reshape(B, Lq, E)
    return out, Pd.mean(1) * keep.unsqueeze(-1), keep


def module_forward(layer64, q, k, v, kept, p, attn_mask=None, key_padding_mask=None, out_row_mask=None):
    """a float64 CPU `MultiheadAttention` without positional encoding around `core`: its own projections in front, its
    output stack (whose nn.Dropout the caller has switched off) and the dead-row / padded-row factors behind"""
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    blocked = blocked_mask(B, Lq, Lk, attn_mask, key_padding_mask)
    out, w, keep = core(layer64.q_proj(q), layer64.k_proj(k), layer64.v_proj(v), layer64.num_heads, blocked, kept, p)
    out = layer64.out_proj(out) * keep.unsqueeze(-1)
    if out_row_mask is not None:
        out = out * (~out_row_mask).to(out.dtype).unsqueeze(-1)
    return out, w
