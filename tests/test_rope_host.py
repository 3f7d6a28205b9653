"""CPU: the rotary position encodings' native path answers what it supports without a device, and leaves CPU tensors to the
module code (`seq_layers.FUSED_ROPE` changes nothing there)."""
import pytest
import torch


@pytest.mark.parametrize('kind,width,want', [
    (3, 32, True), (4, 64, True), (3, 128, True), (4, 40, True), (3, 6, True), (4, 8, True), (3, 2, True),
    (3, 7, False), (4, 33, False), (3, 0, False), (4, -2, False),          # odd or empty widths
    (1, 64, False), (2, 64, False), (0, 64, False), (5, 64, False),        # ABSOLUTE, ABSOLUTE_CAT, no encoding, no such kind
])
def test_rope_supported_answers_without_a_device(kind, width, want):
    from asac_amd import native
    assert native.rope_supported(kind, width) is want


def test_native_kinds_are_the_enum_values():
    from asac_amd import native
    from algorithm.nn_models.layers.seq_layers import POSITIONAL_ENCODING
    assert (native.ROPE, native.ROPE2) == (POSITIONAL_ENCODING.ROPE.value, POSITIONAL_ENCODING.ROPE2.value)


@pytest.mark.parametrize('q', [5, 2])
@pytest.mark.parametrize('kind', ['ROPE', 'ROPE2'])
def test_cpu_tensors_take_the_module_path(kind, q):
    from algorithm.nn_models.layers import seq_layers as sl
    torch.manual_seed(0)
    block = sl.EpisodeMultiheadAttentionBlock(64, 8, pe=sl.POSITIONAL_ENCODING[kind], gate=sl.GATE.RESIDUAL)
    gen = torch.Generator().manual_seed(1)
    B, L = 6, 5
    x = torch.randn(B, L, 64, generator=gen)
    index = torch.arange(L).repeat(B, 1) + torch.randint(0, 5, (B, 1), generator=gen)
    index[0, :2] = -1
    pad = torch.arange(L).unsqueeze(0) < torch.randint(0, 3, (B, 1), generator=gen)

    def run():
        for p in block.parameters():
            p.grad = None
        xd = x.clone().requires_grad_(True)
        out, w = block(xd * 1.0, q, key_index=index, key_padding_mask=pad)
        (out.square().sum() + w.square().sum()).backward()
        return [out.detach(), w.detach(), xd.grad, *(p.grad for p in block.parameters())]

    assert sl.FUSED_ROPE in (True, False)
    before = sl.FUSED_ROPE
    results = {}
    try:
        for flag in (True, False):
            sl.FUSED_ROPE = flag
            results[flag] = run()
    finally:
        sl.FUSED_ROPE = before
    for a, b in zip(results[True], results[False]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_index_tail_view_check():
    from algorithm.nn_models.layers.seq_layers import _is_index_tail
    index = torch.arange(24).view(4, 6)
    assert _is_index_tail(index[:, -2:], index) and _is_index_tail(index[:, -6:], index)
    assert not _is_index_tail(index[:, :2], index), 'the oldest entries are not the tail'
    assert not _is_index_tail(index[:, -2:].clone(), index), 'a copy is other memory'
    assert not _is_index_tail(index[:, -2:].int(), index)
    shared = torch.arange(6).unsqueeze(0).expand(4, -1)
    assert _is_index_tail(shared[:, -3:], shared)
    assert not _is_index_tail(torch.arange(3).unsqueeze(0).expand(4, -1), shared), 'positions 0..2 are not the tail of 0..5'
