"""CPU: the host side of observation normalization on the native path (`hip_config['fused_normalizer']`): the library's
entry points and their binding, the dispatch predicate, and the owner on CPU tensors, where it keeps the module expression
and the eager update.  (The learner has no CPU path: its checkpoint layout with the switch on and off is compared in
tests/test_normalized_step_gpu.py.)"""
import ctypes

import pytest
import torch

SYMBOLS = ['asac_obs_whiten', 'asac_normalizer_update', 'asac_normalizer_row_lanes']

TAKEN = dict(enabled=True, use_normalization=True, plain_learner=True, data_parallel=False, float32_on_device=True)


def test_library_exports_the_entry_points():
    from asac_amd import native
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    lib = native.load()
    assert lib.asac_struct_size(b'asac_whiten_job_t') == ctypes.sizeof(native.WhitenJob) == 64
    assert lib.asac_struct_size(b'asac_normalizer_job_t') == ctypes.sizeof(native.NormalizerJob) == 48
    assert lib.asac_normalizer_row_lanes() == native.NORM_ROW_LANES == 64


def test_binding_lists_the_header_argument_counts():
    from asac_amd import abi, native
    for name in SYMBOLS:
        assert name in abi.functions, f'{name} is not declared'
        params = abi.functions[name][1]
        assert name in native._SIGNATURES and len(native._SIGNATURES[name][1]) == len(params), name
    for wrapper in ('whiten_jobs', 'obs_whiten', 'normalizer_update'):
        assert callable(getattr(native, wrapper)), wrapper
    assert abi.defines['ASAC_NORM_MAX_OBS'] == native.NORM_MAX_OBS == 8
    assert abi.defines['ASAC_NORM_ROW_LANES'] == native.NORM_ROW_LANES
    assert native.ABI_VERSION == 91, 'pure additions: the ABI version stays'


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(enabled=False), False),                   # hip_config['fused_normalizer'] is off (the default)
    (dict(use_normalization=False), False),
    (dict(plain_learner=False), False),             # an OptionBase
    (dict(data_parallel=True), False),
    (dict(float32_on_device=False), False),
])
def test_dispatch_predicate(change, taken):
    """each clause alone flips the answer"""
    from algorithm.normalizer import fused_normalizer_applies
    assert fused_normalizer_applies(**{**TAKEN, **change}) is taken


def test_the_switch_is_off_by_default_and_decides_the_representation_class():
    import inspect
    from algorithm.sac_base import SAC_Base
    assert "hip_config.get('fused_normalizer', False)" in inspect.getsource(SAC_Base.__init__)
    src = inspect.getsource(SAC_Base._build_model)
    assert 'fused_normalizer_applies(' in src and '_wrap_normalized_rep(nn.ModelRep)' in src


def test_row_pitch_of_views():
    from asac_amd import native
    t = torch.zeros(5, 3, 8)
    assert native._row_pitch(t, 1, 8) == 8 and native._row_pitch(t[..., :6], 1, 6) == 8
    assert native._row_pitch(t[:, 1:], 1, 8) is None                      # [5, 2, 8]: rows 8 apart inside, 24 across
    assert native._row_pitch(t[:1, 1:], 1, 8) == 8 and native._row_pitch(t[:, :1, :6], 1, 6) == 24
    assert native._row_pitch(t[:, 1], 1, 8) == 24
    assert native._row_pitch(t[..., ::2], 1, 4) is None                   # non-unit innermost stride
    img = torch.zeros(4, 6, 3, 5, 7)
    assert native._row_pitch(img, 3, 105) == 105 and native._row_pitch(img[:, 2:], 3, 105) is None
    assert native._row_pitch(img[:, 2], 3, 105) == 630 and native._row_pitch(img[0, 0], 3, 105) == 105
    assert native._row_pitch(img.transpose(-1, -2), 3, 105) is None


def test_owner_layout_and_the_module_path_on_cpu_tensors():
    from algorithm.normalizer import Normalizer, update_expression, whiten_expression
    shapes = [(6,), (3, 5, 7)]
    nz = Normalizer(shapes, torch.device('cpu'))
    assert nz.normalizer_step.dtype == torch.int32 and nz.normalizer_step.shape == () and int(nz.normalizer_step) == 0
    for m, v, s in zip(nz.running_means, nz.running_variances, shapes):
        assert m.shape == v.shape == s and m.dtype == v.dtype == torch.float32
        assert (m == 0).all() and (v == 1).all()
        assert m.untyped_storage().data_ptr() == v.untyped_storage().data_ptr() == nz.flat.untyped_storage().data_ptr()
        assert m.data_ptr() % 16 == v.data_ptr() % 16 == nz.flat.data_ptr() % 16
    gen = torch.Generator().manual_seed(0)
    means = [torch.zeros(s) for s in shapes]
    variances = [torch.ones(s) for s in shapes]
    step = torch.tensor(0, dtype=torch.int32)
    for T in (40, 30):
        ep = [torch.randn((T, *s), generator=gen) * 3 + 1 for s in shapes]
        nz.update(ep)
        update_expression(ep, means, variances, step)
    assert int(nz.normalizer_step) == 70 and nz.normalizer_step.dtype == torch.int32
    for a, b in zip(nz.running_means + nz.running_variances, means + variances):
        assert torch.equal(a, b)
    obs = [torch.randn((4, 3, *s), generator=gen) * 10 for s in shapes]
    got = nz.whiten(obs)
    want = whiten_expression(obs, means, variances, step)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and nz.whitened is None
    out = [torch.empty_like(o) for o in obs]
    assert all(a is b for a, b in zip(nz.whiten(obs, out=out), out)) and all(torch.equal(g, w) for g, w in zip(out, want))
    # uint8 episodes promote as the reference's expression does
    ep8 = [torch.randint(0, 256, (20, *s), dtype=torch.uint8, generator=gen) for s in shapes]
    nz.update(ep8)
    update_expression(ep8, means, variances, step)
    assert all(torch.equal(a, b) for a, b in zip(nz.running_means + nz.running_variances, means + variances))
