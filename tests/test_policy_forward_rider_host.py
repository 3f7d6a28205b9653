"""CPU: the host side of `hip_config['policy_forward_rider']` — the exports of the policy-forward rider and of the loaded
policy step in header, binding and notes, the ABI version, and what the `_ok` predicates refuse.  Only `_ok` questions and
refusals are asked of the library: each is answered before the first HIP call, so no GPU is needed."""
import ctypes as C
from pathlib import Path

from asac_amd import native
from tests.test_mlp_job_abi import GAUSS, INVALID_VALUE, NARROW, PTR, _gauss_desc, _job, _ret

ROOT = Path(__file__).resolve().parent.parent
EXPORTS = ('asac_policy_forward_save_floats', 'asac_mlp_backward_qloss_return_rider_ok',
           'asac_mlp_backward_qloss_return_rider', 'asac_policy_step_fused_loaded_ok', 'asac_policy_step_fused_loaded',
           'asac_policy_step_fused_loaded_offline')
SAVE = C.c_void_p(0x60000)          # a 16-byte aligned address that is inspected, never read


def _pi_job(desc=GAUSS, N=256, **kw):
    return _job(desc, E=1, N=N, x1=None, **kw)


def test_abi_version_is_unchanged_and_header_binding_and_notes_agree_on_the_exports():
    from asac_amd import abi
    assert native.ABI_VERSION == 91 and abi.defines['ASAC_ABI_VERSION'] == 91
    assert native.load().asac_version() == 91
    notes = (ROOT / 'INTEGRATION.md').read_text()
    lib = native.load()
    for name in EXPORTS:
        assert abi.functions[name][0] in ('int', 'int64_t'), name
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert len(native._SIGNATURES[name][1]) == len(abi.functions[name][1]), name
        assert f'`{name}`' in notes, name
    # pure additions: the entry points they stand beside keep their signatures
    assert len(native._SIGNATURES['asac_mlp_backward_qloss_return'][1]) == 11
    assert len(native._SIGNATURES['asac_mlp_backward_qloss_return_rider'][1]) == 11 + 2
    assert len(native._SIGNATURES['asac_policy_step_fused'][1]) == 21
    assert len(native._SIGNATURES['asac_policy_step_fused_offline'][1]) == 23
    # the loaded form has the action given: no sampling outputs, one saved forward
    assert len(native._SIGNATURES['asac_policy_step_fused_loaded'][1]) == 21 - 3 + 1
    assert len(native._SIGNATURES['asac_policy_step_fused_loaded_offline'][1]) == 23 - 3 + 1


def test_save_buffer_size_is_25600_bytes_a_tile():
    lib = native.load()
    assert [lib.asac_policy_forward_save_floats(n) for n in (0, 1, 16, 17, 256)] == [0, 6400, 6400, 12800, 16 * 6400]
    assert native.policy_forward_save_floats(256) * 4 == 400 * 1024


def test_rider_ok_refuses_what_the_launch_could_not_run():
    ok = native.load().asac_mlp_backward_qloss_return_rider_ok
    q, ret = _job(N=256), _ret(256, 4)

    def ask(job=q, r=ret, pi=_pi_job(), save=SAVE):
        return ok(C.byref(job) if job is not None else None, C.byref(r) if r is not None else None,
                  C.byref(pi) if pi is not None else None, save)
    assert ask() == 1
    assert ask(pi=None) == 0                                  # a NULL job
    assert ask(job=None) == 0 and ask(r=None) == 0
    assert ask(pi=_pi_job(N=0)) == 0                          # N = 0
    assert ask(pi=_pi_job(NARROW)) == 0                       # a non-stock policy (and no Gaussian head)
    assert ask(pi=_job(_gauss_desc(), E=2, N=256)) == 0       # more than one policy
    assert ask(pi=_pi_job(_gauss_desc(A=9))) == 0             # (loc | scale) beyond one MFMA tile
    assert ask(save=None) == 0                                # a missing save buffer
    assert ask(save=C.c_void_p(0x60004)) == 0                 # ... or one the 16-byte loads cannot read
    assert ask(pi=_pi_job(x0=None)) == 0                      # no rows
    assert ask(pi=_pi_job(window_T=3)) == 0                   # window addressing
    # where the hosting launch itself does not apply, nothing rides
    assert ask(job=_job(NARROW, N=256)) == 0
    assert ask(r=_ret(256, 65)) == 0
    # 32-row tiles (more than 256 workgroups of 16 rows): the rider's workgroups have the policy step's shape, not theirs
    assert ask(job=_job(N=2049, E=2), r=_ret(2049, 4), pi=_pi_job(N=2049)) == 0
    # more policy tiles than the Q job has workgroups
    assert ask(job=_job(N=16, E=1), r=_ret(16, 4), pi=_pi_job(N=17)) == 0
    assert ask(job=_job(N=16, E=2), r=_ret(16, 4), pi=_pi_job(N=17)) == 1


def test_rider_entry_point_refuses_before_any_launch():
    lib = native.load()
    q, ret, over = _job(N=256), _ret(256, 4), native.MLP_REDUCE_OVERWRITE
    for pi, save in ((None, SAVE), (_pi_job(N=0), SAVE), (_pi_job(NARROW), SAVE), (_pi_job(), None)):
        rc = lib.asac_mlp_backward_qloss_return_rider(C.byref(q), PTR, C.byref(ret), None, 0.2, PTR, None, PTR, PTR, over,
                                                      C.byref(pi) if pi is not None else None, save, None)
        assert rc == INVALID_VALUE
        assert 'asac_mlp_backward_qloss_return_rider' in lib.asac_last_error().decode()


def test_loaded_ok_refuses_a_missing_or_misaligned_saved_forward_and_what_the_plain_form_refuses():
    ok = native.load().asac_policy_step_fused_loaded_ok
    from tests.test_mlp_job_abi import STOCK
    args = (C.byref(STOCK), 0x10000, 9216, C.byref(GAUSS), 0x80000, 9216)
    assert ok(*args, 256, SAVE) == 1
    assert ok(*args, 256, None) == 0
    assert ok(*args, 256, C.c_void_p(0x60008)) == 0
    assert ok(*args, 0, SAVE) == 0
    assert ok(C.byref(STOCK), 0x10000, 9216, C.byref(NARROW), 0x80000, 9216, 256, SAVE) == 0
    assert ok(None, 0x10000, 9216, C.byref(GAUSS), 0x80000, 9216, 256, SAVE) == 0
