"""CPU: the host-side checks of the fused-MLP entry points that take a pass (`asac_mlp_job_t`) first.  The library loads
and only refusals / `_ok` questions are asked — every one of them is answered before the first HIP call (csrc/mlp.hip:
`job_ok` / `bwd_job_ok` open each entry point), so no GPU is needed."""
import ctypes as C

import pytest

from asac_amd import native

PARAMS, STRIDE = 0x10000, 9216        # a 16-byte aligned address that is inspected, never read; floats per member
PTR = C.c_void_p(0x20000)             # stands for an operation's own operand: never reached behind a refused job


def _desc(widths, residual, in1=2):
    d = native.MlpDesc()
    d.in0, d.in1, d.n_blocks = 6, in1, len(widths)
    off, k = 0, 6 + in1
    for l, w in enumerate(widths):
        d.width[l], d.residual[l] = w, residual[l]
        d.w_off[l], d.b_off[l] = off, off + w * k
        off, k = off + w * k + w, w
    d.head_cols[0], d.head_w_off[0], d.head_b_off[0] = 1, off, off + k
    return d


STOCK = _desc((64, 64, 64), (0, 1, 1))        # the stock critic: three 64-wide blocks on (6 | 2) inputs
NARROW = _desc((32, 32), (0, 1))              # not stock: two blocks of width 32


def _job(desc=STOCK, E=2, N=256, x0=0x30000, x1=0x40000, out=0x50000, window_T=0):
    j = native.MlpJob()
    j.desc, j.params, j.member_stride, j.E, j.N = C.pointer(desc), PARAMS, STRIDE, E, N
    j.x0, j.x0_row_stride, j.x1, j.x1_row_stride, j.out = x0, desc.in0, x1, desc.in1, out
    j.x0_window_T, j.x0_sample_stride = window_T, 3 * desc.in0 if window_T else 0
    return j


# asac_mlp_backward_qloss_return_ok(stock | narrow network, N, E, n) for n in _STEPS, as the library answered before the
# entry points took a job (ABI 84: desc, params, member_stride, E, N, ret) — 16-row tiles carry n <= 64 steps, 32-row tiles
# (more than 256 workgroups of 16 rows) n <= 16
_STEPS = (1, 16, 32, 33, 64, 65)
_RETURN_OK = {(16, 1): '111110', (16, 2): '111110', (16, 4): '111110',
              (256, 1): '111110', (256, 2): '111110', (256, 4): '111110',
              (2049, 1): '111110', (2049, 2): '110000', (2049, 4): '110000',
              (4100, 1): '110000', (4100, 2): '110000', (4100, 4): '110000'}


def _ret(N, n):
    r = native.VtraceArgs()
    r.q, r.y_out, r.E_sample, r.B, r.n = 0x1000, 0x2000, 2, N, n
    return r


def test_return_ok_table_holds_both_answers():
    answers = set(''.join(_RETURN_OK.values()))
    assert answers == {'0', '1'}


@pytest.mark.parametrize('N,E', sorted(_RETURN_OK))
def test_qloss_return_ok_answers_as_before(N, E):
    lib = native.load()
    for desc, want in ((STOCK, _RETURN_OK[(N, E)]), (NARROW, '0' * len(_STEPS))):
        # the question is about the network and the launch shape: the job's inputs stay unset
        job = _job(desc, E=E, N=N, x0=None, x1=None, out=None)
        got = ''.join(str(lib.asac_mlp_backward_qloss_return_ok(C.byref(job), C.byref(_ret(N, n)))) for n in _STEPS)
        assert got == want, (N, E, desc.n_blocks)


def test_qloss_return_ok_says_no_to_a_job_it_cannot_read():
    lib = native.load()
    ret = _ret(256, 4)
    assert lib.asac_mlp_backward_qloss_return_ok(C.byref(_job(N=256)), C.byref(ret)) == 1
    assert lib.asac_mlp_backward_qloss_return_ok(None, C.byref(ret)) == 0
    assert lib.asac_mlp_backward_qloss_return_ok(C.byref(_job(E=0)), C.byref(ret)) == 0
    assert lib.asac_mlp_backward_qloss_return_ok(C.byref(_job(N=0)), C.byref(ret)) == 0
    assert lib.asac_mlp_backward_qloss_return_ok(C.byref(_job()), None) == 0


def _gauss_desc(A=2):
    """the stock policy on its state rows: in1 = 0, heads (loc | scale) of A columns each"""
    d = _desc((64, 64, 64), (0, 1, 1), in1=0)
    d.head_cols[1], d.head_w_off[1], d.head_b_off[1] = A, d.head_b_off[0] + A, d.head_b_off[0] + A + A * 64
    d.head_cols[0], d.head_transform = A, 1
    return d


GAUSS = _gauss_desc()
INVALID_VALUE = 1       # hipErrorInvalidValue: what `bad_arg` returns


def _entry_points(lib):
    """name -> (call(job | None) with the operation's own operands in place, what a job of its own needs beside the
    defaults of `_job`): behind a job that is in order every call would reach the device"""
    def ret_for(j):      # a return target that fits the job, so that the job is the only thing to refuse
        return C.byref(_ret(j.N if j is not None else 256, 4))

    def ref(j):
        return None if j is None else C.byref(j)
    over = native.MLP_REDUCE_OVERWRITE
    return {
        'asac_mlp_forward': (lambda j: lib.asac_mlp_forward(ref(j), None), {}),
        'asac_mlp_backward': (lambda j: lib.asac_mlp_backward(ref(j), PTR, PTR, PTR, PTR, PTR, over, None), {}),
        'asac_mlp_backward_qloss': (lambda j: lib.asac_mlp_backward_qloss(ref(j), PTR, PTR, None, 0.2, PTR, None, PTR, PTR,
                                                                          over, None), {}),
        'asac_mlp_backward_qloss_return': (lambda j: lib.asac_mlp_backward_qloss_return(
            ref(j), PTR, ret_for(j), None, 0.2, PTR, None, PTR, PTR, over, None), {}),
        'asac_mlp_backward_policy_q': (lambda j: lib.asac_mlp_backward_policy_q(ref(j), PTR, None, 1, PTR, None), {}),
        'asac_mlp_backward_policy_sample': (lambda j: lib.asac_mlp_backward_policy_sample(
            ref(j), PTR, PTR, 2, PTR, PTR, PTR, over, None), dict(desc=GAUSS, E=1, x1=None)),
    }


# one defect each, in a job that is otherwise what the entry point takes (asac_mlp_backward_policy_sample has no network
# with in1 > 0 to offer: there the critic's descriptor is refused for its second input either way)
_DEFECTS = {
    'null job': None,
    'E = 0': dict(E=0),
    'N = 0': dict(N=0),
    'x0 = NULL': dict(x0=None),
    'in1 > 0 and x1 = NULL': dict(desc=STOCK, x1=None),
    'x0_window_T = 3': dict(N=255, window_T=3),      # (no window addressing behind these entry points)
}


def _refused_by_name(lib, name, rc):
    """the entry point's plain `bad_arg`: nothing else writes exactly this (a HIP call's failure reads '<name>: <its
    error>', the other refusals '<name>: <what>: invalid argument')"""
    assert rc == INVALID_VALUE, (name, rc)
    assert lib.asac_last_error().decode() == name + ': invalid argument', name


@pytest.mark.parametrize('case', sorted(_DEFECTS))
def test_every_entry_point_refuses_a_bad_job_by_name(case):
    lib = native.load()
    for name, (call, own) in _entry_points(lib).items():
        job = None if _DEFECTS[case] is None else _job(**{**own, **_DEFECTS[case]})
        _refused_by_name(lib, name, call(job))


def test_policy_sample_wants_one_policy_on_its_state_rows():
    """E and x1 used to be implied by parameters the entry point did not have: now they are refused.  The network is a
    Gaussian-head policy on its state alone, so E or x1 is all that is wrong with the job"""
    lib = native.load()
    call, own = _entry_points(lib)['asac_mlp_backward_policy_sample']
    for defect in (dict(E=2), dict(x1=0x40000)):
        lib.asac_mlp_forward(None, None)          # (another entry point's name into the error slot)
        _refused_by_name(lib, 'asac_mlp_backward_policy_sample', call(_job(**{**own, **defect})))
