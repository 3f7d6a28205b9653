"""GPU: `algorithm/captured_step.CapturedStep` on its own — what the learners' captured steps rely on, on tensors of a few
elements: a capture replays correctly time after time (its memset nodes rewritten), the raw handle is taken exactly when
the captured work draws no torch random numbers, and never where it does."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def _captured_step():
    import asac_amd  # noqa: F401
    from algorithm.captured_step import CapturedStep
    assert CapturedStep.api_ok()
    return CapturedStep


def _counter_fn(counter):
    def fn():
        counter.add_(1)
        return counter
    return fn


def test_replays_across_host_activity():
    CapturedStep = _captured_step()
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    counter = torch.full((16,), 5.0, device=DEV)
    scratch = torch.ones(16, device=DEV)                         # 64 bytes, zero-filled by ATen
    raw = torch.ones(64, dtype=torch.uint8, device=DEV)          # 64 bytes, zero-filled by a plain hipMemsetAsync

    def fn():
        counter.add_(1)
        torch.zeros(16, out=scratch)
        scratch.zero_()
        assert hip.hipMemsetAsync(raw.data_ptr(), 0, raw.numel(), torch.cuda.current_stream().cuda_stream) == 0

    step = CapturedStep.capture(fn, DEV)
    torch.cuda.synchronize()
    replaced, kept = step.memsets
    assert kept == 0 and replaced >= 1, 'the hipMemsetAsync is a memset node the pass must have rewritten'
    base = counter.cpu()
    for i in range(1, 5):
        scratch.fill_(1)        # what a replay does not rewrite would show
        raw.fill_(1)
        step.replay()
        torch.cuda.synchronize()
        assert torch.equal(counter.cpu(), base + i), f'replay {i}'
        assert not scratch.cpu().any() and not raw.cpu().any(), f'replay {i}: a zero-fill did not take effect'


def test_handle_is_taken_when_no_torch_random_numbers_are_drawn():
    CapturedStep = _captured_step()
    counter = torch.zeros(16, device=DEV)
    step = CapturedStep.capture(_counter_fn(counter), DEV)
    assert step.payload is counter, "fn's return value is the payload"
    assert step.exec_handle is None
    step.replay()
    assert step.exec_handle is not None, 'the first replay saw no torch draw: later ones launch the handle'
    for _ in range(3):
        step.replay()
    torch.cuda.synchronize()
    assert torch.equal(counter.cpu(), torch.full((16,), 4.0))

    through_torch = CapturedStep.capture(_counter_fn(counter), DEV)
    for _ in range(3):
        through_torch.replay(direct=False)
        assert through_torch.exec_handle is None
    torch.cuda.synchronize()
    assert torch.equal(counter.cpu(), torch.full((16,), 7.0))

    at_once = CapturedStep.capture(_counter_fn(counter), DEV, take_exec=True)
    assert at_once.exec_handle is not None
    at_once.replay()
    torch.cuda.synchronize()
    assert torch.equal(counter.cpu(), torch.full((16,), 8.0))


def test_handle_is_not_taken_when_torch_random_numbers_are_drawn():
    CapturedStep = _captured_step()
    out = torch.zeros(8, device=DEV)
    step = CapturedStep.capture(lambda: out.copy_(torch.rand(8, device=DEV)), DEV)
    draws = []
    for _ in range(2):
        step.replay()
        assert step.exec_handle is None, "torch's generator must be advanced before every launch of this graph"
        torch.cuda.synchronize()
        draws.append(out.cpu())
    assert not torch.equal(draws[0], draws[1]), 'a replay past torch would repeat the draw'
