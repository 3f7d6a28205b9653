"""CPU: the host side of `hip_config['critic_forward_rider']` — the exports of the critic-forward rider and of the loaded
Q-loss backward in header, binding and notes, the ABI version, the save buffer's size, the plan key, and what the `_ok`
predicates refuse.  Only `_ok` questions and refusals are asked of the library: each is answered before the first kernel
launch, so no GPU is needed.  (Without a device the forward's `_ok` reads a CU count of 0 and refuses every launch; what
it accepts is asked on the GPU, `tests/test_critic_forward_rider_gpu.py`.)"""
import ctypes as C
from pathlib import Path

import torch

from asac_amd import native
from tests.test_mlp_job_abi import GAUSS, INVALID_VALUE, NARROW, PTR, _job, _ret

ROOT = Path(__file__).resolve().parent.parent
EXPORTS = ('asac_critic_forward_save_floats', 'asac_policy_sample_q_forward_saving_ok', 'asac_policy_sample_q_forward_saving',
           'asac_mlp_backward_qloss_return_loaded_ok', 'asac_mlp_backward_qloss_return_loaded',
           'asac_mlp_backward_qloss_return_rider_loaded_ok', 'asac_mlp_backward_qloss_return_rider_loaded')
SAVED = C.c_void_p(0x70000)         # 16-byte aligned addresses that are inspected, never read
SAVE = C.c_void_p(0x60000)


def test_abi_version_is_unchanged_and_header_binding_and_notes_agree_on_the_exports():
    from asac_amd import abi
    assert native.ABI_VERSION == 91 and abi.defines['ASAC_ABI_VERSION'] == 91
    notes = (ROOT / 'INTEGRATION.md').read_text()
    lib = native.load()
    for name in EXPORTS:
        assert abi.functions[name][0] in ('int', 'int64_t'), name
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert len(native._SIGNATURES[name][1]) == len(abi.functions[name][1]), name
        assert f'`{name}`' in notes, name
    # pure additions: the entry points they stand beside keep their signatures
    assert len(native._SIGNATURES['asac_policy_sample_q_forward'][1]) == 6
    assert len(native._SIGNATURES['asac_mlp_backward_qloss_return'][1]) == 11
    assert len(native._SIGNATURES['asac_mlp_backward_qloss_return_rider'][1]) == 13
    # the saving form: the online job and its buffer; the loaded forms: no input gradient, one saved forward
    assert len(native._SIGNATURES['asac_policy_sample_q_forward_saving'][1]) == 6 + 2
    assert len(native._SIGNATURES['asac_mlp_backward_qloss_return_loaded'][1]) == 11 - 1 + 1
    assert len(native._SIGNATURES['asac_mlp_backward_qloss_return_rider_loaded'][1]) == 13 - 1 + 1


def test_save_buffer_size_is_24640_bytes_a_tile_and_member():
    lib = native.load()
    assert [lib.asac_critic_forward_save_floats(n, 2) for n in (0, 1, 16, 17, 256)] == [0, 2 * 6160, 2 * 6160, 4 * 6160, 32 * 6160]
    assert lib.asac_critic_forward_save_floats(256, 0) == 0
    assert native.critic_forward_save_floats(256, 2) * 4 == 788480
    assert native.critic_forward_save_floats(40, 3) == 3 * 3 * 6160


def test_loaded_ok_refuses_what_the_launch_could_not_run():
    ok = native.load().asac_mlp_backward_qloss_return_loaded_ok

    def ask(job=_job(N=256), r=_ret(256, 4), saved=SAVED):
        return ok(C.byref(job) if job is not None else None, C.byref(r) if r is not None else None, saved)
    assert ask() == 1
    assert ask(job=_job(N=1), r=_ret(1, 1)) == 1 and ask(job=_job(N=40, E=3), r=_ret(40, 4)) == 1
    assert ask(job=None) == 0 and ask(r=None) == 0
    assert ask(saved=None) == 0                               # a missing saved forward
    assert ask(saved=C.c_void_p(0x70004)) == 0                # ... or one the 16-byte loads cannot read
    assert ask(job=_job(NARROW, N=256)) == 0                  # where the plain form does not apply, nothing is loaded
    assert ask(r=_ret(256, 65)) == 0
    assert ask(r=_ret(255, 4)) == 0                           # a return over other rows
    # 32-row tiles (more than 256 workgroups of 16 rows): the saved tiles are the sixteen-wave kernel's
    assert ask(job=_job(N=2049, E=2), r=_ret(2049, 4)) == 0


def test_rider_loaded_ok_needs_both_the_policy_rider_and_the_saved_forward():
    ok = native.load().asac_mlp_backward_qloss_return_rider_loaded_ok
    q, ret, pi = _job(N=256), _ret(256, 4), _job(GAUSS, E=1, N=256, x1=None)

    def ask(pi_job=pi, save=SAVE, saved=SAVED):
        return ok(C.byref(q), C.byref(ret), C.byref(pi_job) if pi_job is not None else None, save, saved)
    assert ask() == 1
    assert ask(pi_job=None) == 0 and ask(save=None) == 0 and ask(saved=None) == 0
    assert ask(pi_job=_job(NARROW, E=1, N=256, x1=None)) == 0
    assert ask(saved=C.c_void_p(0x70008)) == 0


def test_loaded_entry_points_refuse_before_any_launch():
    lib = native.load()
    q, ret, over, pi = _job(N=256), _ret(256, 4), native.MLP_REDUCE_OVERWRITE, _job(GAUSS, E=1, N=256, x1=None)
    for saved in (None, C.c_void_p(0x70004)):
        rc = lib.asac_mlp_backward_qloss_return_loaded(C.byref(q), PTR, C.byref(ret), None, 0.2, PTR, PTR, PTR, over, saved, None)
        assert rc == INVALID_VALUE and 'asac_mlp_backward_qloss_return_loaded' in lib.asac_last_error().decode()
        rc = lib.asac_mlp_backward_qloss_return_rider_loaded(C.byref(q), PTR, C.byref(ret), None, 0.2, PTR, PTR, PTR, over,
                                                             C.byref(pi), SAVE, saved, None)
        assert rc == INVALID_VALUE and 'asac_mlp_backward_qloss_return_rider_loaded' in lib.asac_last_error().decode()


def test_saving_forward_refuses_missing_jobs_and_buffers():
    lib = native.load()
    ok = lib.asac_policy_sample_q_forward_saving_ok
    job, online = native.PiQJob(), _job(N=256)
    assert ok(None, None, 0, None, 0, C.byref(online), SAVE) == 0
    assert ok(C.byref(job), None, 0, None, 0, None, SAVE) == 0
    assert ok(C.byref(job), None, 0, None, 0, C.byref(online), None) == 0
    assert ok(C.byref(job), None, 0, None, 0, C.byref(online), C.c_void_p(0x60004)) == 0
    assert ok(C.byref(job), None, 0, None, 0, C.byref(online), SAVE) == 0          # an empty fused job, no extra job
    rc = lib.asac_policy_sample_q_forward_saving(C.byref(job), None, 0, None, 0, C.byref(online), SAVE, None)
    assert rc == INVALID_VALUE and 'asac_policy_sample_q_forward_saving' in lib.asac_last_error().decode()


def test_plan_key_names_the_stored_pair_and_the_window():
    import asac_amd  # noqa: F401
    from algorithm.sac_base import SAC_Base
    base = torch.zeros(8, 3, 6)
    x0, a0 = base[:, 1], torch.zeros(8, 2)
    key = SAC_Base._critic_plan_key(x0, a0, 3)
    assert key == (x0.data_ptr(), 18, a0.data_ptr(), 2, 8, 3)
    assert key != SAC_Base._critic_plan_key(base[:, 0], a0, 3) and key != SAC_Base._critic_plan_key(x0, a0, 5)
    assert key != SAC_Base._critic_plan_key(x0[:4], a0[:4], 3)
