"""CPU: the host side of the one-launch siamese losses (`asac_siamese_atc_loss_grad` / `asac_siamese_byol_loss_grad`,
csrc/siamese.hip): the predicate that decides when the learner takes them, and the three entry points named alike by the
header, the binding, the wrappers and INTEGRATION.md."""
import inspect
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ('asac_siamese_atc_workspace_floats', 'asac_siamese_atc_loss_grad', 'asac_siamese_byol_loss_grad')


def _applies(**over):
    import asac_amd  # noqa: F401
    from algorithm.sac_base import fused_siamese_applies
    from algorithm.utils.enums import SIAMESE
    kw = dict(enabled=True, siamese=SIAMESE.ATC, float32_on_device=True, N=768, n=3, widths=[16], target_requires_grad=False)
    kw.update(over)
    if isinstance(kw['siamese'], str):
        kw['siamese'] = SIAMESE[kw['siamese']]
    return fused_siamese_applies(**kw)


TABLE = [
    (dict(), True),                                            # usv_search: batch 256, n-step 3, E 16
    (dict(widths=[16, 16]), True),
    (dict(widths=[1], N=33, n=3), True),                       # E at its lower limit
    (dict(widths=[128]), True),                                # ... and at its upper
    (dict(widths=[129]), False),
    (dict(widths=[0]), False),
    (dict(widths=[16, 129]), False),                           # one encoder outside is enough
    (dict(widths=[]), False),
    (dict(n=1, N=5), True),
    (dict(n=0, N=5), False),
    (dict(n=64, N=192), True),
    (dict(n=65, N=195), False),
    (dict(N=16384, n=4), True),
    (dict(N=16388, n=4), False),
    (dict(N=0, n=3), False),
    (dict(N=770, n=3), False),                                 # n does not divide N
    (dict(enabled=False), False),
    (dict(siamese=None), False),
    (dict(float32_on_device=False), False),                    # CPU tensors, another dtype, a non-contiguous operand
    (dict(target_requires_grad=True), False),
    (dict(siamese='BYOL', widths=[14]), True),
    (dict(siamese='BYOL', widths=[256], N=1, n=1), True),
    (dict(siamese='BYOL', widths=[257]), False),
    (dict(siamese='BYOL', widths=[14], N=1 << 20, n=4), True),
    (dict(siamese='BYOL', widths=[14], N=(1 << 20) + 4, n=4), False),
    (dict(siamese='BYOL', widths=[14], N=770, n=3), True),     # the block length plays no part in the cosine
    (dict(siamese='BYOL', enabled=False), False),
    (dict(siamese='BYOL', target_requires_grad=True), False),
]


@pytest.mark.parametrize('over,want', TABLE, ids=[str(i) for i in range(len(TABLE))])
def test_fused_siamese_applies(over, want):
    assert _applies(**over) is want


def test_entry_points_are_declared_bound_and_wrapped_alike():
    import asac_amd  # noqa: F401
    from asac_amd import abi, native
    assert native.ABI_VERSION == 91          # pure additions
    assert abi.defines['ASAC_ABI_VERSION'] == 91
    for name in ENTRY_POINTS:
        assert name in native.EXPORTED_SYMBOLS
        assert len(native._SIGNATURES[name][1]) == len(abi.functions[name][1]), name
    assert len(abi.functions['asac_siamese_atc_loss_grad'][1]) == 12 and len(abi.functions['asac_siamese_byol_loss_grad'][1]) == 9
    # the wrappers carry the entry points' names (the launch profiler's keys are derived from them)
    assert native.siamese_atc_loss_grad.__name__ == 'siamese_atc_loss_grad'
    assert native.siamese_byol_loss_grad.__name__ == 'siamese_byol_loss_grad'
    assert list(inspect.signature(native.siamese_atc_workspace_floats).parameters) == ['N', 'E']
    # the limits the predicate uses are the header's
    for macro, value in (('ASAC_SIAMESE_MAX_WIDTH', native.SIAMESE_MAX_WIDTH), ('ASAC_SIAMESE_MAX_BLOCK', native.SIAMESE_MAX_BLOCK),
                         ('ASAC_SIAMESE_MAX_ROWS', native.SIAMESE_MAX_ROWS),
                         ('ASAC_SIAMESE_BYOL_MAX_WIDTH', native.SIAMESE_BYOL_MAX_WIDTH),
                         ('ASAC_SIAMESE_BYOL_WORKSPACE_FLOATS', native.SIAMESE_BYOL_WORKSPACE_FLOATS)):
        assert abi.defines[macro] == value, macro
    assert abi.defines['ASAC_SIAMESE_BYOL_MAX_ROWS'] == native.SIAMESE_BYOL_MAX_ROWS == 1 << 20


def test_profiler_names_and_documents():
    import asac_amd  # noqa: F401
    from asac_amd import native
    seen = []

    class Spy:
        def bracket(self, name, fn, *a, **k):
            seen.append(name)

    native.set_profiler(Spy())
    try:
        native.siamese_atc_loss_grad()
        native.siamese_byol_loss_grad()
    finally:
        native.set_profiler(None)
    assert seen == ['asac_siamese_atc_loss_grad', 'asac_siamese_byol_loss_grad']
    notes = (ROOT / 'INTEGRATION.md').read_text()
    for name in ENTRY_POINTS:
        assert name in notes, f'{name} has no row in INTEGRATION.md'
    assert 'siamese.hip' in (ROOT / 'advanced-soft-actor-critic_amd' / 'csrc' / 'build.py').read_text()


def test_workspace_query_and_host_refusals_need_no_device():
    """the size query is host arithmetic; a refused call returns before anything touches the device"""
    import asac_amd  # noqa: F401
    from asac_amd import native
    lib = native.load()
    assert native.siamese_atc_workspace_floats(768, 16) > 768 * 16
    small, large = native.siamese_atc_workspace_floats(48, 16), native.siamese_atc_workspace_floats(16384, 128)
    assert 0 < small < large < (1 << 26)
    for N, E in ((0, 16), (16385, 16), (48, 0), (48, 129)):
        assert native.siamese_atc_workspace_floats(N, E) == -1
    bad = 1                                    # hipErrorInvalidValue
    assert lib.asac_siamese_atc_loss_grad(None, None, None, None, 48, 16, 3, None, None, None, None, None) == bad
    assert lib.asac_siamese_byol_loss_grad(None, None, None, 48, 14, None, None, None, None) == bad
    assert b'asac_siamese_byol_loss_grad' in lib.asac_last_error()


def test_the_switch_is_off_by_default():
    text = (ROOT / 'advanced-soft-actor-critic_amd' / 'algorithm' / 'sac_base.py').read_text()
    assert "hip_config.get('fused_siamese', False)" in text
