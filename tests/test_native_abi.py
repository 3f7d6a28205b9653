"""CPU: the C-ABI library loads and exports exactly what include/asac_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'asac_hip.h'


def declared_symbols():
    text = HEADER.read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(asac_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert 'asac_sumtree_sample' in syms and 'asac_window_gather_pad' in syms and len(syms) >= 18


def test_library_exports_every_declared_symbol():
    from asac_amd import native
    if not native.LIB_PATH.exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location('asac_build', ROOT / 'advanced-soft-actor-critic_amd/csrc/build.py')
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    lib = ctypes.CDLL(str(native.LIB_PATH))
    for name in declared_symbols():
        assert hasattr(lib, name), f'{name} declared in asac_hip.h but not exported'


def test_integration_notes_name_every_entry_point():
    """INTEGRATION.md maps every export to the reference lines it replaces: a new entry point without a row there is
    a boundary change nobody wrote down."""
    notes = (ROOT / 'INTEGRATION.md').read_text()
    missing = [name for name in declared_symbols() if name not in notes]
    assert not missing, missing


def test_binding_covers_header_and_abi_version():
    from asac_amd import native
    assert sorted(native.EXPORTED_SYMBOLS) == declared_symbols()
    lib = native.load()
    m = re.search(r'#define ASAC_ABI_VERSION (\d+)', HEADER.read_text())
    assert lib.asac_version() == int(m.group(1)) == native.ABI_VERSION


def test_struct_layouts_match_header_sizes():
    """every struct of the header: where the library knows the name (`asac_struct_size`), sizeof as the library's
    compiler laid it out is the ctypes class's (the host compiler's layouts, field by field: tests/test_abi_host.py)"""
    from asac_amd import abi, native
    lib = native.load()
    known = {name: lib.asac_struct_size(name.encode()) for name in abi.structs}
    known = {name: size for name, size in known.items() if size != -1}
    for name, size in known.items():
        assert size == ctypes.sizeof(abi.ctypes_struct(name)), name
    # a condition, not a measurement: the 21 names csrc/sumtree.hip answers for stay answered (the other 10 of the header's
    # 31 structs have the host compiler's check alone)
    assert {'asac_gather_key_t', 'asac_partial_sum_t', 'asac_row_move_t', 'asac_batch_put_key_t', 'asac_batch_gather_key_t',
            'asac_sidecar_t', 'asac_squash_job_t', 'asac_vtrace_args_t', 'asac_mlp_desc_t', 'asac_mlp_job_t',
            'asac_pi_q_job_t', 'asac_mlp_sample_epilogue_t', 'asac_gru_desc_t', 'asac_conv2_desc_t', 'asac_conv1_desc_t',
            'asac_obs_decoder_params_t', 'asac_branches_t', 'asac_members_t', 'asac_discrete_return_t',
            'asac_whiten_job_t', 'asac_normalizer_job_t'} <= set(known)
    assert native.PiQJob is abi.ctypes_struct('asac_pi_q_job_t')
    assert lib.asac_struct_size(b'no_such_struct') == -1


def test_product_path_refuses_cpu_devices():
    import torch
    from asac_amd import native
    from algorithm.replay_buffer import PrioritizedReplayBuffer
    with pytest.raises(native.AsacNativeError):
        PrioritizedReplayBuffer(batch_size=4, device=torch.device('cpu'), capacity=16)
    from algorithm.agent import EpisodeSlab
    import numpy as np
    with pytest.raises(native.AsacNativeError):     # the agent side's episode slabs live in HBM as well
        EpisodeSlab([(6,)], [np.float32], 2, (0,), 16, torch.device('cpu'), np.zeros(2, np.float32))


def test_binding_argument_counts_match_the_header():
    """every ctypes signature lists as many arguments as the header declares (ctypes accepts EXTRA arguments silently and
    converts them by its default rules — a Python int would travel as a 32-bit int where the C side expects int64)"""
    import re
    from asac_amd import native
    hdr = re.sub(r'/\*.*?\*/', '', (ROOT / 'include' / 'asac_hip.h').read_text(), flags=re.S)
    bad = []
    for name, (_res, args) in native._SIGNATURES.items():
        m = re.search(r'\b' + name + r'\s*\(([^;{]*?)\)\s*;', hdr, re.S)
        assert m, f'{name}: bound but not declared'
        params = [p_ for p_ in m.group(1).split(',') if p_.strip() and p_.strip() != 'void']
        if len(params) != len(args):
            bad.append((name, len(params), len(args)))
    assert not bad, bad
