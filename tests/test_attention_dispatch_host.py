"""Host: what the attention modules keep on the CPU — no native launch for any positional encoding, the reference's
`state_dict` keys (the dropout draw sites are plain attributes), and copies / pickles of a re-seeded module."""
import copy
import pickle

import pytest
import torch


def _modules():
    import asac_amd  # noqa: F401
    import algorithm.nn_models as m
    return m


@pytest.mark.parametrize('pe', [None, 'ROPE', 'ROPE2', 'ABSOLUTE', 'ABSOLUTE_CAT'])
def test_a_cpu_module_issues_no_native_launch(pe, monkeypatch):
    m = _modules()
    from asac_amd import native

    def no_library(*_a, **_k):
        raise AssertionError('a CPU module reached the native library')
    monkeypatch.setattr(native, 'load', no_library)
    torch.manual_seed(0)
    layer = m.MultiheadAttention(32, 2, pe=None if pe is None else m.POSITIONAL_ENCODING[pe], qkv_dense_depth=1,
                                 out_dense_depth=1, dropout=0.5)
    x = torch.randn(3, 5, 32, requires_grad=True)
    pad = torch.arange(5).unsqueeze(0) < torch.tensor([[0], [1], [2]])
    with _recorder(native) as prof:
        for query in (x, x[:, -2:]):
            out, w = layer(query, x, x, key_padding_mask=pad, out_row_mask=pad[:, -query.shape[1]:])
            (out.sum() + w.sum()).backward()
            assert out.shape == (3, query.shape[1], 32) and w.shape == (3, query.shape[1], 5)
            assert torch.isfinite(out).all() and torch.isfinite(w).all()
    assert list(prof.records) == []
    assert layer.dropout_state() is None and layer.dense_dropout_state('qkv') is None and layer.dense_dropout_state('out') is None


class _recorder:
    """`native.LaunchProfiler` without the library calls of its enter / exit: only the record of bracketed launches"""

    def __init__(self, native):
        self.native, self.prof = native, native.LaunchProfiler(repeat=1)

    def __enter__(self):
        self.native.set_profiler(self.prof)
        return self.prof

    def __exit__(self, *exc):
        self.native.set_profiler(None)
        return False


def test_state_dict_keys_are_the_references():
    m = _modules()
    layer = m.MultiheadAttention(32, 2, qkv_dense_depth=1, out_dense_depth=1, dropout=0.5)
    assert list(layer.state_dict().keys()) == [
        'q_proj.dense.0.linear.weight', 'q_proj.dense.0.linear.bias', 'q_proj.dense.2.weight', 'q_proj.dense.2.bias',
        'k_proj.dense.0.linear.weight', 'k_proj.dense.0.linear.bias', 'k_proj.dense.2.weight', 'k_proj.dense.2.bias',
        'v_proj.dense.0.linear.weight', 'v_proj.dense.0.linear.bias', 'v_proj.dense.2.weight', 'v_proj.dense.2.bias',
        'out_proj.dense.0.linear.weight', 'out_proj.dense.0.linear.bias']
    assert [n for n, _ in layer.named_children()] == ['q_proj', 'k_proj', 'v_proj', 'out_proj'] and not list(layer.buffers())


@pytest.mark.parametrize('how', ['deepcopy', 'pickle'])
def test_a_reseeded_module_survives_copy_and_pickle(how):
    m = _modules()
    torch.manual_seed(0)
    layer = m.MultiheadAttention(32, 2, qkv_dense_depth=1, out_dense_depth=1, dropout=0.5)
    assert layer.reseed(9, 7, 3) is layer
    twin = copy.deepcopy(layer) if how == 'deepcopy' else pickle.loads(pickle.dumps(layer))
    assert (twin._drop_seed, twin._drop_counter0, twin._drop_instance) == (9, 7, 3)
    assert twin.dropout_state() is None and twin.dense_dropout_state('qkv') is None and twin.dense_dropout_state('out') is None
    with pytest.raises(RuntimeError, match='no dropout launch yet'):
        twin.dropout_drawn()
    with pytest.raises(RuntimeError, match='no qkv dropout launch yet'):
        twin.dense_dropout_drawn('qkv')
    for (name, a), (_, b) in zip(layer.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), name
    x = torch.randn(3, 5, 32)
    for a, b in zip(layer.eval()(x, x, x), twin.eval()(x, x, x)):
        assert torch.equal(a, b)
