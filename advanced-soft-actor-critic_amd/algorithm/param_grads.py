"""Where the fused backwards put their PARAMETER gradients: the one answer every producer and the learners share.  A leaf
module: it imports torch and the native wrappers only, so every module of the package imports it at top level.

Default: parameter gradients are returned to autograd like any op's, so `autograd.grad`, `backward(inputs=...)` and
gradient gating (`sac_aux.calculate_adaptive_weights`) see exactly what PyTorch semantics promise.
Inside `direct_param_grads()` the backward kernels instead ADD them straight into the parameters' `.grad` views of
the learner's flat gradient buffer (no per-parameter AccumulateGrad launches) and hand autograd nothing: only valid
around a backward pass that is meant to accumulate into every parameter it reaches — the learner wraps exactly
those (the Q loss, the policy objective, the curiosity loss).  A plain global: the autograd engine runs backward
nodes on its own device thread while the caller blocks inside the `with`.
`only`: the backward is restricted to these tensors (`backward(inputs=...)`): `ctx.needs_input_grad` is fixed at
forward time and does not know about that restriction, so a direct-mode backward consults `direct_skips` and leaves
the parameters outside the set alone (no launch, no accumulation) — what autograd does with their gradients anyway.
"""
import contextlib
import os

import torch

from asac_amd import native

_direct_depth = 0
_direct_only = []


@contextlib.contextmanager
def direct_param_grads(only=None):
    global _direct_depth
    if _direct_depth == 0:
        # (a backward pass that raised may have left queued products and an armed end-of-backward callback behind)
        reset_queue()
    _direct_depth += 1
    _direct_only.append(None if only is None else {id(t) for t in only})
    try:
        yield
    finally:
        _direct_only.pop()
        _direct_depth -= 1


def direct_enabled() -> bool:
    return _direct_depth > 0


def direct_skips(*params) -> bool:
    """inside a restricted direct-mode backward: none of `params` is among the tensors the backward may reach"""
    only = _direct_only[-1] if _direct_only else None
    return only is not None and not any(id(p) in only for p in params)


def flat_alias(tensors):
    """-> a 1-D tensor aliasing `tensors` if they sit back to back, in order, in one storage (the learner's flat
    parameter / gradient buffers), else None"""
    t0 = tensors[0]
    base, pos = t0.untyped_storage().data_ptr(), t0.storage_offset()
    first = pos
    for t in tensors:
        if (t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                or t.untyped_storage().data_ptr() != base or t.storage_offset() != pos):
            return None
        pos += t.numel()
    return torch.empty(0, dtype=torch.float32, device=t0.device).set_(t0.untyped_storage(), first, (pos - first,))


def flat_grad_alias(params):
    """-> `flat_alias` of the parameters' `.grad`s when every one of them trains and has one, else None: the part of the
    direct-mode eligibility test the packed producers share (each adds its own conditions in front)"""
    if all(p.requires_grad and p.grad is not None for p in params):
        return flat_alias([p.grad for p in params])
    return None


def spans_meet(spans, held) -> bool:
    """does one of the byte ranges `spans` ([lo, hi) pairs: the floats a job writes or adds to) overlap one of `held`?
    The jobs of one multi-job launch run side by side in no order, so two jobs on one output would race: both queues
    below close a launch in front of a job whose output meets one the launch already holds."""
    return any(lo < b and a < hi for lo, hi in spans for a, b in held)


def _span(t, n=None):
    lo = t.data_ptr()
    return lo, lo + 4 * (t.numel() if n is None else n)


class DeferredPartialSums:
    """While active, the backward launches of the fused modules (dense stacks, convolution stacks, Linear + Tanh heads,
    attention blocks) that would hand parameter gradients BACK to autograd — `autograd.grad` walks, not the learner's
    direct mode — return None for them and leave the second launch of each (the per-workgroup partials summed in workgroup
    order) to `flush()`, which runs up to sixteen of them as ONE launch (`native.sum_partials_multi`; per job the order,
    hence the bits, of the launch it stands for) and returns {walk: {id(parameter): gradient}} for the caller to put where
    autograd left None — like fused_conv.DeferredConvBackward, and for the same walks: those of
    `calculate_adaptive_weights` / `_train_rpm` (reference sac_base.py:1607-1631, 1798-1839), which only collect their
    parameter gradients.  `walk`: set by the caller in front of each `autograd.grad`.  A parameter other nodes of the graph
    use as well still gets those nodes' contributions from autograd; the caller adds."""
    _active = None

    def __init__(self):
        self.jobs, self.grads, self.walk, self._outer = [], {}, 0, None
        self.sums_after = []

    @classmethod
    def active(cls):
        return cls._active if SUM_PARTIALS_LATER else None

    def __enter__(self):
        self._outer, DeferredPartialSums._active = DeferredPartialSums._active, self
        return self

    def __exit__(self, exc_type, exc, tb):
        DeferredPartialSums._active = self._outer
        return False

    def add(self, partial, slabs, slices, slab_stride, n, out, accumulate=False):
        self.jobs.append((partial, slabs, slices, slab_stride, n, out, bool(accumulate)))

    def add_after(self, into, piece):
        """`into += piece` once the sums have run (both views of buffers `add`ed above, `into` the caller's own): what a
        caller that hands its gradients out itself owes a parameter it reached twice (fused_conv.DeferredConvBackward,
        whose `flush()` returns its own {walk: gradients} — keyed by ITS walks, several per call — before the sums have
        run; `record` delivers through this object's `flush()` and under this object's one current `walk`)"""
        self.sums_after.append((into, piece))

    def record(self, params, grads):
        """the gradients (views of buffers `add`ed above) this walk owes `params`"""
        mine = self.grads.setdefault(self.walk, {})
        for p, g in zip(params, grads):
            if g is not None:
                mine.setdefault(id(p), []).append(g)

    @staticmethod
    def _launches(jobs):
        """`jobs` in the order queued, cut into launches: a launch ends where it holds sixteen jobs or where the next job's
        output floats [out, out + n) overlap those of a job it already holds (`spans_meet`: a module reached twice in a
        direct-mode backward — both ADD into its span of the flat gradient buffer); launch after launch they are
        stream-ordered, as the reductions they stand for were.  (`n` floats, not `out.numel()`: an ensemble member's `out`
        is a view that runs on over the next's.)"""
        launches, spans = [], []
        for job in jobs:
            span = _span(job[5], job[4])
            if (not launches or len(launches[-1]) == native.SUM_PARTIALS_MAX_JOBS or spans_meet([span], spans)):
                launches.append([])
                spans = []
            launches[-1].append(job)
            spans.append(span)
        return launches

    def flush(self):
        """-> {walk: {id(parameter): gradient}}; the sums run here (one launch per sixteen recorded backwards, see `_launches`)"""
        jobs, self.jobs = self.jobs, []
        for launch in self._launches(jobs):
            native.sum_partials_multi(launch)
        after, self.sums_after = self.sums_after, []
        for into, piece in after:
            into.add_(piece)
        taken, self.grads = self.grads, {}
        # (a parameter two recorded nodes of one walk share: their gradients added, as autograd would have)
        return {walk: {pid: gl[0] if len(gl) == 1 else sum(gl[1:], gl[0]) for pid, gl in mine.items()}
                for walk, mine in taken.items()}


SUM_PARTIALS_LATER = os.environ.get('ASAC_SUM_PARTIALS_LATER', '1') != '0'    # (A/B switch)


def deliver_packed(params, flat, n, launch, partials):
    """The tail the packed producers' backwards share (convolution stacks, Linear + Tanh head, attention block): their
    parameter gradients are ONE block of `n` floats in the order of `params`.  `flat`: the direct-mode target the caller
    decided on — a `flat_alias` of the `.grad`s, added into — or None: a scratch block, written, one view per parameter.
    `launch(out, mode)` runs the backward kernel whose sum over its partials goes to `out`: mode False (0) written, True (1)
    added, `native.SUM_DEFER` left to the walk's `DeferredPartialSums`, to which `partials()` -> (workspace, slabs, slices,
    slab_stride, n) then describes what the launch left.  -> the gradients autograd receives, one per parameter: None where
    the kernel added them in place, where `DeferredPartialSums.flush()` delivers them, and for a parameter that does not train"""
    later = DeferredPartialSums.active()          # (the sums as one launch with the walk's other second launches)
    out = flat if flat is not None else torch.empty(n, dtype=torch.float32, device=params[0].device)
    launch(out, native.SUM_DEFER if later is not None else flat is not None)
    if later is not None:
        later.add(*partials(), out, accumulate=flat is not None)
    if flat is not None:
        return [None] * len(params)
    grads, off = [], 0
    for p in params:
        k = p.numel()
        grads.append(out[off:off + k].view(p.shape) if p.requires_grad else None)
        off += k
    if later is not None:           # (the gradients reach the caller through `later.flush()`)
        later.record(params, grads)
        grads = [None] * len(params)
    return grads


@contextlib.contextmanager
def learner_backward(only=None):
    """A backward pass of the learner: direct mode with the launches' second launches — the per-workgroup partials summed
    into the flat gradient — run as one launch when the block ends (`flush()`; a block that raises flushes nothing)"""
    with direct_param_grads(only), DeferredPartialSums() as sums_later:
        yield sums_later
    sums_later.flush()


# The `x^T y` queue (fused_rows_linear, fused_gru_wide, layers.seq_layers).
# Direct mode (the learner's `loss.backward()`: gradients are ADDED into the `.grad` views of the flat buffer, nobody reads them
# before the optimizer): the products are not launched one by one but queued and issued four at a time as one launch pair
# (`asac_xty_multi` — the four Linears of an attention block make exactly one), the rest when the backward pass ends.
QUEUE = os.environ.get('ASAC_XTY_QUEUE', '1') != '0'      # (0: one launch pair per product — A/B runs)
_pending = []
_armed = False


def flush_param_grads():
    jobs = list(_pending)
    del _pending[:]
    if len(jobs) == 1:
        native.xty(*jobs[0], accumulate=True)
    elif jobs:
        native.xty_multi(jobs, accumulate=True)


def reset_queue():
    """drop what a failed backward pass left behind (called when the learner opens a direct-mode backward)"""
    global _armed
    del _pending[:]
    _armed = False


def _end_of_backward():
    global _armed
    _armed = False
    flush_param_grads()


def _xty_spans(job):
    return [_span(t) for t in job[2:4] if t is not None]


def queue_param_grads(g2, x2, w_grad, b_grad):
    """w_grad += g2^T x2, b_grad += column sums of g2 — some time before this backward pass returns"""
    global _armed
    if not QUEUE:
        native.xty(g2, x2, w_grad, b_grad, accumulate=True)
        return
    job = (g2, x2, w_grad, b_grad)
    if spans_meet(_xty_spans(job), [s for j in _pending for s in _xty_spans(j)]):
        flush_param_grads()      # (a layer applied twice: its two products add to one gradient, one after the other)
    _pending.append(job)
    if len(_pending) == 4:
        flush_param_grads()
    elif not _armed:
        _armed = True
        torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)
