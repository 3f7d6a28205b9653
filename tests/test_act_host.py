"""CPU: the host side of policy-based acting on the native path (`hip_config['fused_act']`, csrc/act.hip): the dispatch
predicate, the entry points' bookkeeping, and the float64 restatement the GPU tests compare the kernel with
(tests/act_ref.py) against the reference's own `_choose_action` (`tests/golden/f20_act.npz`) and against
`torch.linspace`."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import act_ref as ar
from tests import parity_utils as pu
from tests.golden.make_act_golden import CASES, NARROW

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ('asac_act_sizes_ok', 'asac_act_policy')

PLAIN = dict(enabled=True, plain_learner=True, d_action_sizes=[3, 2], c_action_size=0, discrete_dqn_like=False,
             rnd_in_effect=False, offline_action=False, float32_on_device=True, state_dim=2)


@pytest.mark.parametrize('change,taken', [
    ({}, True),
    (dict(c_action_size=2), True),                                   # hybrid
    (dict(d_action_sizes=[], c_action_size=2), True),                # continuous only: see the docstring
    (dict(d_action_sizes=[64]), True), (dict(d_action_sizes=[2] * 8), True), (dict(c_action_size=8), True),
    (dict(enabled=False), False),                                    # hip_config['fused_act'] = False
    (dict(plain_learner=False), False),                              # an OptionBase
    (dict(discrete_dqn_like=True), False), (dict(rnd_in_effect=True), False), (dict(offline_action=True), False),
    (dict(float32_on_device=False), False), (dict(state_dim=3), False),
    (dict(d_action_sizes=[65]), False), (dict(d_action_sizes=[2] * 9), False), (dict(c_action_size=9), False),
    (dict(d_action_sizes=[], c_action_size=0), False),
])
def test_dispatch_predicate(change, taken):
    """each excluded condition alone turns the path off.  Continuous actions alone satisfy the predicate with or without
    `action_noise`: `_choose_action` asks it fifth, so a stock continuous policy without noise never reaches it (the first
    branch serves it: `test_the_branch_is_asked_behind_the_four_earlier_ones`)"""
    from algorithm.sac_base import fused_act_applies
    assert fused_act_applies(**{**PLAIN, **change}) is taken


def test_the_branch_is_asked_behind_the_four_earlier_ones():
    """in `_choose_action` the predicate's call stands behind the stock continuous launches, `rnd_pick`, `drnd_pick` and
    `dqn_act`, and in front of the eager tail"""
    import inspect
    from algorithm.sac_base import SAC_Base
    src = inspect.getsource(SAC_Base._choose_action)
    order = [src.index(s) for s in ('native.squash_sample_fwd(', 'native.rnd_pick(', 'native.drnd_pick(', 'native.dqn_act(',
                                    'fused_act_applies(', 'native.act_policy(', 'self.model_policy(state, obs_list)\n        if offline_action is None')]
    assert order == sorted(order)
    assert src.count('fused_act_applies(') == 1 and src.count('native.act_policy(') == 1
    assert 'self._random_action(' not in src[order[4]:order[6]], 'the launch did the noise'


def test_header_binding_and_notes_name_both_entry_points():
    from asac_amd import abi, native
    declared = {name for name in abi.functions if name.startswith('asac_act_')}
    bound = {name for name in native.EXPORTED_SYMBOLS if name.startswith('asac_act_')}
    assert declared == bound == set(ENTRY_POINTS)
    notes = (ROOT / 'INTEGRATION.md').read_text()
    for name in ENTRY_POINTS:
        assert callable(getattr(native, name[len('asac_'):])) and f'| `{name}` |' in notes
    assert abi.defines['ASAC_ABI_VERSION'] == native.ABI_VERSION == 91
    assert abi.defines['ASAC_ACT_MAX_CONT'] == native.ACT_MAX_CONT == 8
    assert 'act.hip' in __import__('importlib').import_module('csrc.build').SOURCES


C_TYPES = {'asac_branches_t': 'asac_branches_t', 'const float*': 'c_void_p', 'float*': 'c_void_p', 'int64_t': 'c_long',
           'int32_t': 'c_int', 'float': 'c_float'}


def test_the_ctypes_mirror_has_the_headers_fields_in_order():
    from asac_amd import native
    text = (ROOT / 'include' / 'asac_hip.h').read_text()
    body = re.search(r'typedef struct \{([^}]*)\} asac_act_job_t;', text).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r'((?:const )?\w+\*?)\s+(.*)', decl).groups()
        fields += [(n.strip(), C_TYPES[ctype]) for n in names.split(',')]
    mirror = [(n, t.__name__) for n, t in native.ActJob._fields_]
    assert mirror == fields
    assert fields[0] == ('branches', 'asac_branches_t') and native.ActJob._fields_[0][1] is native.Branches and fields[-2][0] == 'B'


def test_sizes_ok_on_the_host_is_the_librarys_answer():
    import ctypes as C
    from asac_amd import native
    lib = native.load()
    for sizes, A in [((3, 2), 0), ((3, 2), 2), ((), 2), ((), 0), ((64,), 8), ((65,), 0), ((2,) * 8, 1), ((2,) * 9, 0), ((3,), 9),
                     ((3, 0), 0), ((), 8), ((), -1), ((32, 33), 0)]:
        br = native.branches(sizes)
        assert bool(lib.asac_act_sizes_ok(C.byref(br), A)) == native.act_sizes_ok(sizes, A), (sizes, A)
    assert lib.asac_act_sizes_ok(None, 2) == 1 and lib.asac_act_sizes_ok(None, 0) == 0


def test_draw_columns_of_the_binding_and_of_the_restatement_agree():
    from asac_amd import native
    for K in (0, 1, 2, 8):
        for A in (0, 1, 8):
            for det in (False, True):
                for noise in (False, True):
                    assert native.act_draw_columns(K, A, det, noise) == ar.draw_columns(K, A, det, noise)
    assert ar.draw_columns(2, 2, False, True) == (5, 4) and ar.draw_columns(2, 2, True, True) == (3, 2)
    assert ar.draw_columns(2, 2, True, False) == (0, 0) and ar.draw_columns(0, 2, False, True) == (0, 4)


@pytest.mark.parametrize('B', [1, 2, 7, 65, 256, 4096])
@pytest.mark.parametrize('lo,hi', [(0., 1.), (0.1, 0.9), (0.5, 0.5), (0.05, 0.95), (1., 1.)])
def test_noise_levels_are_torch_linspace(lo, hi, B):
    np.testing.assert_array_equal(ar.noise_levels(lo, hi, B), torch.linspace(lo, hi, B).numpy())


def _heads(g, case):
    """the fixture's weights in this repository's modules on the CPU -> (logits, mean, logstd, hidden) float32"""
    import algorithm.nn_models as m
    plugin, sizes, A, _ = CASES[case]
    nn = pu.plugin(plugin)
    t = lambda k: torch.from_numpy(g[f'{case}/{k}'])      # noqa: E731
    sub = lambda name: {k[len(f'{case}/w0/{name}/'):]: torch.from_numpy(g[k]) for k in g.files       # noqa: E731
                        if k.startswith(f'{case}/w0/{name}/')}
    rep = nn.ModelRep(['vector'], [(6,)], list(sizes), A, False)
    rep.load_state_dict(sub('model_rep'))
    with torch.no_grad():
        state, hidden = rep([t('in/obs_list').unsqueeze(1)], t('in/pre_action').unsqueeze(1),
                            t('in/pre_seq_hidden_state').unsqueeze(1))
        policy = m.ModelPolicy(state.shape[-1], list(sizes), A, **NARROW['policy'])
        policy.load_state_dict(sub('model_policy'))
        logits, mean, logstd = policy.heads_raw(state.squeeze(1))
    return logits, mean, logstd, hidden.squeeze(1)


@pytest.mark.parametrize('case', list(CASES))
def test_the_restatement_against_the_reference_fixture(golden_dir, case):
    """`act_ref.act` (deterministic, no noise) on the head outputs of the fixture's weights: the one-hots equal the
    reference's exactly, the continuous action and the probabilities agree to 1e-6 (float64 against the reference's
    float32); the density is evaluated at the reference's own float32 action"""
    g = np.load(golden_dir / 'f20_act.npz')
    _, sizes, A, _ = CASES[case]
    D = sum(sizes)
    logits, mean, logstd, hidden = _heads(g, case)
    np.testing.assert_allclose(hidden.numpy(), g[f'{case}/hidden'], rtol=1e-6, atol=1e-7)
    ref = ar.act(sizes=sizes, logits=logits.numpy(), loc=None if mean is None else mean.numpy(),
                 scale=None if logstd is None else logstd.numpy(), head_raw=True, deterministic=True)
    want_a, want_p = g[f'{case}/action'], g[f'{case}/prob']
    j0 = 0
    for s in sizes:         # the fixture keeps a margin at every argmax, so that float32 rounding cannot move one
        part = np.sort(ar.softmax_branches(logits.numpy(), sizes)[:, j0:j0 + s], axis=-1)
        assert (part[:, -1] - part[:, -2]).min() > 1e-4, 'change the seed of this case'
        j0 += s
    np.testing.assert_array_equal(ref['onehot'], want_a[:, :D])
    np.testing.assert_allclose(ref['p'], want_p[:, :D], rtol=0, atol=1e-6)
    if A:
        np.testing.assert_allclose(ref['a'], want_a[:, D:], rtol=0, atol=1e-6)
        dens = ar.density(want_a[:, D:], ref['loc'], ref['scale'])
        np.testing.assert_allclose(dens, want_p[:, D:], rtol=1e-6, atol=1e-6)


def test_the_restatements_sampling_rules():
    """ties take the lowest index, u == 0 the first entry of positive probability, a masked tail is never returned and
    has probability exactly 0, the noise gate and the uniform index follow the header"""
    z = np.array([[1., 1., 0.5, 2., 2.]], dtype=np.float32)
    assert ar.act(sizes=(3, 2), logits=z, deterministic=True)['index'].tolist() == [[0, 0]]
    masked = np.array([[-np.inf, 0., 0., -np.inf, -np.inf]], dtype=np.float32)
    r = ar.act(sizes=(5,), logits=masked, u=np.array([[0.]], dtype=np.float32))
    assert r['index'].tolist() == [[1]] and r['p'][0].tolist() == [0., 0.5, 0.5, 0., 0.]
    r = ar.act(sizes=(5,), logits=masked, u=np.array([[np.nextafter(np.float32(1), np.float32(0))]], dtype=np.float32))
    assert r['index'].tolist() == [[2]]
    u = np.array([[0.9, 0.9, 0.2, 0.7, 0.4], [0.9, 0.9, 0.6, 0.7, 0.4]], dtype=np.float32)     # (sampling | gate | index)
    r = ar.act(sizes=(3, 2), logits=np.zeros((2, 5), dtype=np.float32), u=u, noise=(0.5, 0.5))
    assert r['index'].tolist() == [[2, 0], [2, 1]]          # row 0: the gate opens (0.2 < 0.5): floor(0.7 * 3), floor(0.4 * 2)
    r = ar.act(loc=np.zeros((1, 1), dtype=np.float32), scale=np.ones((1, 1), dtype=np.float32),
               eps=np.array([[0.5, 2.]], dtype=np.float32), noise=(0.25, 0.25))
    np.testing.assert_allclose(r['a'], np.tanh(np.arctanh(np.float64(np.float32(np.tanh(0.5)))) + 2. * 0.25), rtol=1e-15)
