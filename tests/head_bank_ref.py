"""NumPy float64 restatement of a head bank (`csrc/head_bank.hip`, `algorithm/fused_heads.py`), written from
`algorithm/nn_models/layers/linear_layers.py`: G groups of K stacks `LinearLayers(S, W, depth, size_k)` on the same rows —
`depth` ResBlocks `h = gelu(W_l h + b_l) (+ h)` with the erf-form GELU, then the output Linear — the forward, and for a
given `grad_out` the gradient with respect to every parameter and to x.  Row by row matrix algebra, no tiles.

Also the helpers the GPU tests share: parameters laid out as `FlatParamGroup` lays a critic ensemble out (one segment per
group, every segment on a 16-byte boundary, the tensors of a segment back to back — so that behind a head bias of 3 or 2
floats nothing is 16-byte aligned), and the float32 composition of torch operators on the same parameters."""
import math

import numpy as np


def _erf(z):
    """erf of a float64 array (NumPy has none; torch's float64 CPU erf is libm's)"""
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64))).numpy()


def gelu(z):
    return 0.5 * z * (1. + _erf(z / math.sqrt(2.)))


def gelu_grad(z):
    return 0.5 * (1. + _erf(z / math.sqrt(2.))) + z * np.exp(-0.5 * z * z) / math.sqrt(2. * math.pi)


def stack_forward(x, params, residual):
    """x [N, S] float64; params [w_0, b_0, .., head w, head b] (nn.Linear layout) -> (out [N, size], [(h_l, z_l)] per block)"""
    h, kept = x, []
    for l, res in enumerate(residual):
        w, b = params[2 * l], params[2 * l + 1]
        z = h @ w.T + b
        kept.append((h, z))
        h = gelu(z) + h if res else gelu(z)
    return h @ params[-2].T + params[-1], kept, h


def stack_backward(x, params, residual, g_out):
    """-> ([d w_0, d b_0, .., d head w, d head b], d x) for the cotangent g_out [N, size]"""
    _, kept, h_last = stack_forward(x, params, residual)
    grads = [None] * len(params)
    grads[-2], grads[-1] = g_out.T @ h_last, g_out.sum(0)
    gh = g_out @ params[-2]
    for l in range(len(residual) - 1, -1, -1):
        h, z = kept[l]
        gz = gh * gelu_grad(z)
        grads[2 * l], grads[2 * l + 1] = gz.T @ h, gz.sum(0)
        gh = gz @ params[2 * l] + (gh if residual[l] else 0.)
    return grads, gh


def bank_forward(x, stacks, residual, sizes, G):
    """x [N, S]; stacks: M = G K parameter lists, group-major -> out [G, N, D], each group's branches side by side"""
    K = len(sizes)
    return np.stack([np.concatenate([stack_forward(x, stacks[g * K + k], residual)[0] for k in range(K)], axis=1)
                     for g in range(G)])


def bank_backward(x, stacks, residual, sizes, G, grad_out):
    """grad_out [G, N, D] -> (per stack the list of parameter gradients, d x summed over the stacks in ascending order)"""
    K, offs = len(sizes), np.concatenate([[0], np.cumsum(sizes)])
    grads, gx = [], np.zeros_like(x)
    for g in range(G):
        for k in range(K):
            gp, g_in = stack_backward(x, stacks[g * K + k], residual, grad_out[g][:, offs[k]:offs[k + 1]])
            grads.append(gp)
            gx = gx + g_in
    return grads, gx


# ---------------------------------------------------------------------------------------------------------------------
def residual_flags(S, W, depth):
    """what `LinearLayers(S, W, depth, size)` builds: a block adds its input where the widths agree"""
    return tuple((S if l == 0 else W) == W for l in range(depth))


def flat_layout(S, W, depth, sizes, G):
    """-> (floats, [per stack: [(offset, shape), ..]]) of G segments `q_g` as `FlatParamGroup` lays them out"""
    total, stacks = 0, []
    for _ in range(G):
        for size in sizes:
            views = []
            for l in range(depth):
                for shape in ((W, S if l == 0 else W), (W,)):
                    views.append((total, shape))
                    total += int(np.prod(shape))
            for shape in ((size, W), (size,)):
                views.append((total, shape))
                total += int(np.prod(shape))
            stacks.append(views)
        total = (total + 3) // 4 * 4
    return total, stacks


def make_params(S, W, depth, sizes, G, seed):
    """-> (flat float32 array, layout): Kaiming-uniform weights as `LinearLayers` draws them, biases of the same scale (a
    trained network's are not zero)"""
    rng = np.random.default_rng(seed)
    total, layout = flat_layout(S, W, depth, sizes, G)
    flat = np.zeros(total, dtype=np.float32)
    for views in layout:
        for off, shape in views:
            fan_in = shape[1] if len(shape) == 2 else W
            bound = math.sqrt(6. / fan_in) if len(shape) == 2 else 0.3
            flat[off:off + int(np.prod(shape))] = rng.uniform(-bound, bound, int(np.prod(shape))).astype(np.float32)
    return flat, layout


def views_of(flat, layout):
    """views of a flat tensor / array for the layout: per stack [w_0, b_0, .., head w, head b]"""
    return [[flat[off:off + int(np.prod(shape))].reshape(shape) for off, shape in views] for views in layout]


def torch_composition(x, stacks, residual, sizes, G):
    """the float32 composition of torch operators on the same parameter tensors: Linear, erf GELU, residual add, per stack,
    then `torch.cat` per group — what the module code computes -> [G, N, D] (autograd-ready)"""
    import torch
    import torch.nn.functional as F
    K, groups = len(sizes), []
    for g in range(G):
        outs = []
        for k in range(K):
            p, h = stacks[g * K + k], x
            for l, res in enumerate(residual):
                y = F.gelu(F.linear(h, p[2 * l], p[2 * l + 1]))
                h = y + h if res else y
            outs.append(F.linear(h, p[-2], p[-1]))
        groups.append(torch.cat(outs, dim=-1))
    return torch.stack(groups)
