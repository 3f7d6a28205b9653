"""Discrete heads of the stock networks as a bank: the K branch stacks `LinearLayers(S, W, depth, size_k)` of a `ModelQ` or
`ModelPolicy` (`d_dense_list`) — or those of all E critics at once — run as ONE `asac_head_bank_forward` launch, and their
backward as the two launches of `asac_head_bank_backward` (`csrc/head_bank.hip`, MFMA f32), on the parameters where they
lie in the flat buffer.  The launch writes each group's branches side by side: no `torch.cat` follows.
Anything else (a live dropout, another activation, stacks of unequal depth or width, a width the kernel refuses) keeps the
module path: `describe_head_bank` returns None and the caller runs the lines it ran before.
"""
from typing import NamedTuple

import torch

from asac_amd import native

from .fused_mlp import _blocks_of
from .nn_models.layers.linear_layers import LinearLayers
from .param_grads import direct_enabled, direct_skips

__all__ = ['BankShape', 'HeadBank', 'describe_head_bank', 'attach', 'd_heads']


class BankShape(NamedTuple):
    S: int
    W: int
    residual: tuple      # one flag per ResBlock
    sizes: tuple         # the branches' head widths
    G: int
    stacks: list         # M = G K lists of parameters (w_0, b_0, .., head w, head b), group-major


def _stack_of(ll):
    """-> (in width, width, residual flags, head width, parameters) of one `LinearLayers(S, W, depth, size)`, or None"""
    if not isinstance(ll, LinearLayers):
        return None
    found = _blocks_of(ll)
    if found is None:
        return None
    blocks, final = found
    if not blocks or final is None or final.bias is None:
        return None
    W, prev, params = blocks[0].linear.out_features, blocks[0].linear.in_features, []
    S = prev
    for b in blocks:
        if b.linear.in_features != prev or b.linear.out_features != W or b.linear.bias is None:
            return None
        if b.residual and b.linear.in_features != W:
            return None
        params += [b.linear.weight, b.linear.bias]
        prev = W
    if final.in_features != W:
        return None
    params += [final.weight, final.bias]
    return S, W, tuple(bool(b.residual) for b in blocks), final.out_features, params


def describe_head_bank(groups, require_device=True) -> 'BankShape | None':
    """`groups`: a list of G `d_dense_list`s (one per ensemble member; [policy.d_dense_list] for a policy).  -> the bank they
    form, or None: every stack must be GELU ResBlocks of one width behind dropouts of p = 0 and a final Linear with bias;
    depth, width and residual flags equal across all stacks, head widths equal across the groups, float32 parameters (on
    the device unless `require_device` is False), the sizes inside `asac_head_bank_supported`"""
    groups = [list(g) for g in groups]
    if not groups or not groups[0] or any(len(g) != len(groups[0]) for g in groups):
        return None
    first, sizes, stacks = None, None, []
    for g in groups:
        mine = []
        for ll in g:
            st = _stack_of(ll)
            if st is None:
                return None
            S, W, residual, size, params = st
            if first is None:
                first = (S, W, residual)
            if (S, W, residual) != first:
                return None
            if any(p.dtype != torch.float32 or (require_device and not p.is_cuda) for p in params):
                return None
            mine.append(size)
            stacks.append(params)
        if sizes is None:
            sizes = tuple(mine)
        if tuple(mine) != sizes:
            return None
    S, W, residual = first
    if not native.head_bank_supported(S, W, len(residual), sizes, len(groups)):
        return None
    return BankShape(S, W, residual, sizes, len(groups), stacks)


class _HeadBankFn(torch.autograd.Function):
    """inputs: (anchor, x, bank, *the stacks' parameters) — the parameters are inputs so that the node is part of every
    backward / `autograd.grad` that asks for them (fused_mlp._MlpFn)"""

    @staticmethod
    def forward(ctx, anchor, x, bank, *params):
        ctx.bank = bank
        ctx.save_for_backward(x)
        return bank._forward(x)

    @staticmethod
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        gx, pg = ctx.bank._backward(x, grad_out.contiguous(), ctx.needs_input_grad[1], ctx.needs_input_grad[3:])
        return (None, gx, None, *pg)


class HeadBank:
    """The launches of one bank.  The device tables of parameter and gradient pointers are built once: the views keep their
    addresses (`FlatParamGroup.rebind` keeps the layout)."""

    def __init__(self, shape: BankShape):
        self.shape = shape
        self.desc = native.head_bank_desc(shape.S, shape.W, shape.residual, shape.sizes, shape.G)
        self.params = [p for st in shape.stacks for p in st]
        self.device = self.params[0].device
        self.D = sum(shape.sizes)
        self.table = native.head_bank_table([[p.data for p in st] for st in shape.stacks])
        self._grad_table = None
        # a scratch block with the parameters' order: the byte offsets of the views, to which a block's address is added
        offs, total = [], 0
        for st in shape.stacks:
            row = []
            for p in st:
                row.append(4 * total)
                total += p.numel()
            offs.append(row)
        self._scratch_floats = total
        self._scratch_offsets = torch.tensor(offs, dtype=torch.int64).to(self.device)
        self._anchor = torch.zeros(1, device=self.device, requires_grad=True)      # keeps the node in the graph
        self._workspaces = {}

    # -- launches ----------------------------------------------------------------------------------------------------
    def _rows(self, x):
        if x.dim() == 3 and x.stride(2) == 1 and not x.is_contiguous():
            return x                    # a [samples, T, S] window: read in place
        return x.contiguous()

    def _forward(self, x):
        x = self._rows(x)
        out = torch.empty((self.shape.G, *x.shape[:-1], self.D), dtype=torch.float32, device=x.device)
        native.head_bank_forward(self.desc, self.table, x, out)
        return out

    def _workspace(self, N):
        if N not in self._workspaces:
            self._workspaces[N] = native.head_bank_backward_workspace(self.device, N, self.desc)
        return self._workspaces[N]

    def grad_table(self):
        """the table of the `.grad` views (the learner's flat gradient buffer), or None while a parameter has none"""
        if any(p.grad is None for p in self.params):
            return None
        ptrs = [p.grad.data_ptr() for p in self.params]
        if self._grad_table is None or ptrs != self._grad_ptrs:      # (built once: the views keep their addresses)
            self._grad_table = native.head_bank_table([[p.grad for p in st] for st in self.shape.stacks])
            self._grad_ptrs = ptrs
        return self._grad_table

    def _backward(self, x, grad_out, need_x, needs):
        x = self._rows(x)
        N = x.numel() // self.shape.S
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_x else None
        ws = self._workspace(N) if N else None
        pg = [None] * len(needs)
        kw = dict(grad_x=gx, workspace=ws)
        if direct_enabled():
            gt = self.grad_table()
            skipped = [direct_skips(p) for p in self.params]
            if all(skipped):
                if need_x:
                    native.head_bank_backward(self.desc, self.table, None, x, grad_out, **kw)
                return gx, pg
            if gt is not None and not any(skipped):
                # (every `.grad` view of the bank is added to, whatever `needs` says: `_MlpFn`'s contract — a backward
                # restricted to some parameters says so through `direct_param_grads(only=...)`)
                native.head_bank_backward(self.desc, self.table, gt, x, grad_out, accumulate=True, **kw)
                return gx, pg
            # a backward restricted to some of the bank's parameters (or a parameter without a `.grad` view): the products
            # go to a scratch block and the parameters inside the set take their share from there
            views = self._to_scratch(x, grad_out, kw)
            for p, v, skip in zip(self.params, views, skipped):
                if not skip and p.requires_grad:
                    if p.grad is None:
                        p.grad = v.clone()
                    else:
                        p.grad.add_(v)
            return gx, pg
        if any(needs):
            views = self._to_scratch(x, grad_out, kw)
            pg = [v if need else None for v, need in zip(views, needs)]
        elif need_x:
            native.head_bank_backward(self.desc, self.table, None, x, grad_out, **kw)
        return gx, pg

    def _to_scratch(self, x, grad_out, kw):
        scratch = torch.empty(self._scratch_floats, dtype=torch.float32, device=self.device)
        table = self._scratch_offsets + scratch.data_ptr()
        native.head_bank_backward(self.desc, self.table, table, x, grad_out, accumulate=False, **kw)
        views, off = [], 0
        for p in self.params:
            views.append(scratch[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return views

    def __call__(self, x):
        """x [.., S] -> [G, .., D]: the forward launch under `no_grad`, else a node whose backward is the bank's"""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.params)):
            return _HeadBankFn.apply(self._anchor, x, self, *self.params)
        return self._forward(x)


def attach(module) -> bool:
    """give a stock `ModelQ` / `ModelPolicy` the bank of its own `d_dense_list` (G = 1); False if they form none"""
    shape = describe_head_bank([module.d_dense_list]) if getattr(module, 'd_dense_list', None) is not None else None
    module._head_bank = HeadBank(shape) if shape is not None else None
    return shape is not None


def d_heads(module, h):
    """the discrete branches' head outputs on h, concatenated [.., D], from one launch per pass — or None where the module
    carries no bank (the caller then runs its stacks one by one)"""
    bank = getattr(module, '_head_bank', None)
    if bank is None:
        return None
    return bank(h)[0]
