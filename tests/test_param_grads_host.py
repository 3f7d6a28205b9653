"""Host logic of `algorithm/param_grads.py`: the delivery helper the packed producers share (`deliver_packed`) in its two
modes that need no device — returned to autograd, and left to `DeferredPartialSums` —, the learner's backward context
(`learner_backward`), and the one overlap predicate behind both queues (`spans_meet`).  CPU: launches are recorders."""
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture
def pg(monkeypatch):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm import param_grads
    sums = []
    monkeypatch.setattr(native, 'sum_partials_multi', lambda jobs: sums.append(list(jobs)))
    return param_grads, sums


def _params():
    w1, b1, w2 = torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(4, 3))
    b2 = torch.nn.Parameter(torch.zeros(4), requires_grad=False)
    return [w1, b1, w2, b2]


class _Fakes:
    """the two callables of a producer: `launch` writes 1, 2, ... n into its output unless told to defer"""

    def __init__(self, n, defer_mode):
        self.n, self.defer_mode, self.launches, self.asked = n, defer_mode, [], 0
        self.ws = torch.zeros(5 * n)

    def launch(self, out, mode):
        self.launches.append((out, mode))
        if mode != self.defer_mode:
            out.copy_(torch.arange(1., self.n + 1))

    def partials(self):
        assert self.launches, 'the partials are described after the launch'
        self.asked += 1
        return self.ws, 5, 16, self.n, self.n


def test_deliver_packed_returns_one_view_per_trainable_parameter(pg):
    param_grads, sums = pg
    from asac_amd import native
    params, n = _params(), 6 + 3 + 12 + 4
    fakes = _Fakes(n, native.SUM_DEFER)
    grads = param_grads.deliver_packed(params, None, n, fakes.launch, fakes.partials)
    assert len(fakes.launches) == 1 and fakes.asked == 0 and not sums
    out, mode = fakes.launches[0]
    assert mode == 0 and mode != native.SUM_DEFER and out.shape == (n,) and out.dtype == torch.float32
    assert [None if g is None else tuple(g.shape) for g in grads] == [(3, 2), (3,), (4, 3), None]
    offs = [0, 6, 9]
    for g, off, p in zip(grads, offs, params):           # views of the launch's block, in packed order
        assert g.data_ptr() == out.data_ptr() + 4 * off
        assert torch.equal(g.reshape(-1), torch.arange(1., n + 1)[off:off + p.numel()])


def test_deliver_packed_leaves_the_sum_and_the_gradients_to_the_deferred_sums(pg):
    param_grads, sums = pg
    from asac_amd import native
    params, n = _params(), 6 + 3 + 12 + 4
    fakes = _Fakes(n, native.SUM_DEFER)
    with param_grads.DeferredPartialSums() as later:
        later.walk = 'w'
        grads = param_grads.deliver_packed(params, None, n, fakes.launch, fakes.partials)
        assert grads == [None] * 4
        assert len(fakes.launches) == 1 and fakes.launches[0][1] == native.SUM_DEFER and fakes.asked == 1
        out = fakes.launches[0][0]
        assert len(later.jobs) == 1          # exactly one job, with the partials the producer described, written not added
        partial, slabs, slices, stride, count, target, accumulate = later.jobs[0]
        assert partial is fakes.ws and (slabs, slices, stride, count) == (5, 16, n, n) and target is out and accumulate is False
        recorded = later.grads['w']
        assert set(recorded) == {id(p) for p in params[:3]}          # one view per trainable parameter, none for the frozen one
        assert all(len(v) == 1 for v in recorded.values())
        assert not sums
    late = later.flush()
    assert len(sums) == 1 and len(sums[0]) == 1 and sums[0][0][0] is fakes.ws
    assert set(late) == {'w'} and [tuple(late['w'][id(p)].shape) for p in params[:3]] == [(3, 2), (3,), (4, 3)]
    assert late['w'][id(params[2])].data_ptr() == out.data_ptr() + 4 * 9


def test_deliver_packed_with_the_switch_off_does_not_defer(pg, monkeypatch):
    param_grads, sums = pg
    monkeypatch.setattr(param_grads, 'SUM_PARTIALS_LATER', False)
    fakes = _Fakes(25, 2)
    with param_grads.DeferredPartialSums() as later:
        grads = param_grads.deliver_packed(_params(), None, 25, fakes.launch, fakes.partials)
    assert fakes.launches[0][1] == 0 and not later.jobs and later.flush() == {} and grads[0] is not None and not sums


def test_learner_backward_flushes_once_on_a_clean_exit(pg):
    param_grads, sums = pg
    out = torch.zeros(8)
    assert not param_grads.direct_enabled()
    with param_grads.learner_backward() as later:
        assert param_grads.direct_enabled() and param_grads.DeferredPartialSums.active() is later
        later.add(torch.zeros(16), 2, 1, 8, 8, out, accumulate=True)
        assert not sums
    assert len(sums) == 1 and len(sums[0]) == 1 and not later.jobs
    assert not param_grads.direct_enabled() and param_grads.DeferredPartialSums.active() is None


def test_learner_backward_flushes_nothing_when_the_block_raises(pg):
    param_grads, sums = pg
    with pytest.raises(KeyError):
        with param_grads.learner_backward() as later:
            later.add(torch.zeros(16), 2, 1, 8, 8, torch.zeros(8), accumulate=True)
            raise KeyError('the backward failed')
    assert not sums and len(later.jobs) == 1
    assert not param_grads.direct_enabled() and param_grads.DeferredPartialSums.active() is None


def test_learner_backward_hands_only_to_the_direct_mode(pg):
    param_grads, _ = pg
    a, b = torch.zeros(1), torch.zeros(1)
    with param_grads.learner_backward(only=[a]):
        assert not param_grads.direct_skips(a, b) and param_grads.direct_skips(b)
    assert not param_grads.direct_skips(b)


def _span(buf, start, n):
    return buf[start:].data_ptr(), buf[start:].data_ptr() + 4 * n


@pytest.mark.parametrize('first, second, meet', [
    ((0, 40), (39, 10), True),        # the range cases of tests/test_partial_sums_host.py: the last float of the first ...
    ((10, 30), (0, 11), True),
    ((0, 40), (8, 4), True),          # a view at an offset, inside
    ((8, 4), (0, 40), True),          # ... and around
    ((0, 40), (0, 40), True),         # a module reached twice
    ((0, 40), (40, 24), False),       # outputs that only touch
    ((0, 97), (100, 97), False)])     # ensemble members: the views run on, the floats written do not
def test_spans_meet_on_ranges(pg, first, second, meet):
    param_grads, _ = pg
    buf = torch.zeros(256)
    assert param_grads.spans_meet([_span(buf, *second)], [_span(buf, *first)]) is meet
    assert param_grads.spans_meet([_span(buf, *first)], [_span(buf, *second)]) is meet


def test_spans_meet_on_the_pointer_cases_of_the_xty_queue(pg):
    """tests/test_xty_queue.py's trigger — equal weight pointers or equal bias pointers — as spans [ptr, ptr + 4 numel)"""
    param_grads, _ = pg
    spans = param_grads._xty_spans
    w, b = torch.zeros(3, 2), torch.zeros(3)
    w2, b2 = torch.zeros(3, 2), torch.zeros(3)
    g, x = torch.zeros(4, 3), torch.zeros(4, 2)
    held = spans((g, x, w, b))
    assert param_grads.spans_meet(spans((g, x, w, b)), held)             # the same layer again
    assert param_grads.spans_meet(spans((g, x, w, b2)), held)            # equal weight pointers
    assert param_grads.spans_meet(spans((g, x, w2, b)), held)            # equal bias pointers
    assert param_grads.spans_meet(spans((g, x, w, None)), held)          # ... a job without a bias
    assert not param_grads.spans_meet(spans((g, x, w2, b2)), held)       # another layer
    assert not param_grads.spans_meet(spans((g, x, w2, None)), spans((g, x, w, None)))
    assert not param_grads.spans_meet(spans((g, x, w2, b2)), [])


def test_param_grads_is_a_leaf_module():
    """importing it pulls in neither the dense stack nor the model package (what the function-level imports used to dodge)"""
    code = ('import sys; sys.path.insert(0, %r); import asac_amd; import algorithm.param_grads; '
            'bad = [m for m in sys.modules if m.startswith("algorithm.") and m != "algorithm.param_grads"]; '
            'assert not bad, bad; assert "algorithm.fused_mlp" not in sys.modules' % str(ROOT))
    done = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
