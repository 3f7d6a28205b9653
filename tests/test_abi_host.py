"""CPU: the binding is the header.  `abi.parse` on each declarator form of include/asac_hip.h; every struct's size and every
field's offset and size as the host C compiler lays them out, against ctypes; every entry point's argument count and
scalar widths against the header text, read a second, dumb way; the values the wrappers pass where an argtype changed."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import asac_amd  # noqa: F401
from asac_amd import abi

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / 'include'


# ------------------------------------------------------------------------------------------------ 1. the parser
def test_comments_defines_and_enumerators():
    got = abi.parse('/* a block\n comment; int x(void); */\n#ifndef G\n#define G\n#include <stdint.h>\n'
                    '#define ASAC_A 7 /* seven */\n#define ASAC_B (1 << 20)\n// int y(void);\n'
                    'enum { ASAC_P = 0, ASAC_Q = 3 /* q */ };\nenum {\n  ASAC_R = 1\n};\n#endif\n')
    assert got.defines == {'ASAC_A': 7, 'ASAC_B': 1 << 20, 'ASAC_P': 0, 'ASAC_Q': 3, 'ASAC_R': 1}
    assert got.structs == {} and got.functions == {}


def test_const_anywhere_and_pointer_to_const_pointer():
    got = abi.parse('int f(const float* const* w, float* const* g, const void* p, int const n, const char* s);')
    assert got.functions == {'f': ('int', [('w', 'float', 2), ('g', 'float', 2), ('p', 'void', 1), ('n', 'int', 0),
                                           ('s', 'char', 1)])}


def test_multi_declarator_fields_and_array_lengths():
    got = abi.parse('#define ASAC_N 4\ntypedef struct {\n  float *param, *grad, *exp_avg;\n'
                    '  int64_t head_w_off[2], head_b_off[2];\n  int32_t width[ASAC_N];\n  const float* base[ASAC_N];\n'
                    '  float lr, beta1;\n} asac_s_t;')
    assert got.structs == {'asac_s_t': [
        ('param', 'float', 1, None), ('grad', 'float', 1, None), ('exp_avg', 'float', 1, None),
        ('head_w_off', 'int64_t', 0, 2), ('head_b_off', 'int64_t', 0, 2), ('width', 'int32_t', 0, 4),
        ('base', 'float', 1, 4), ('lr', 'float', 0, None), ('beta1', 'float', 0, None)]}


def test_nested_struct_by_value_and_struct_pointers():
    got = abi.parse('typedef struct { int32_t a; } asac_in_t;\n'
                    'typedef struct { asac_in_t pi; const asac_in_t* desc; asac_in_t x0, action; } asac_out_t;\n'
                    'int64_t g(const asac_out_t* job_host, void* stream);')
    assert got.structs['asac_out_t'] == [('pi', 'asac_in_t', 0, None), ('desc', 'asac_in_t', 1, None),
                                         ('x0', 'asac_in_t', 0, None), ('action', 'asac_in_t', 0, None)]
    assert got.functions['g'] == ('int64_t', [('job_host', 'asac_out_t', 1), ('stream', 'void', 1)])


def test_void_parameter_list_return_types_and_declarations_over_lines():
    got = abi.parse('#ifdef __cplusplus\nextern "C" {\n#endif\nint v(void);\nconst char* e(void);\n'
                    'int64_t\nw(int64_t rows,\n      unsigned int* counter,\n\n      double\n      beta);\n'
                    '#ifdef __cplusplus\n}\n#endif\n')
    assert got.functions == {'v': ('int', []), 'e': ('char*', []),
                             'w': ('int64_t', [('rows', 'int64_t', 0), ('counter', 'unsigned int', 1), ('beta', 'double', 0)])}
    assert list(got.functions) == ['v', 'e', 'w']     # the header's order


@pytest.mark.parametrize('text', [
    'int f(size_t n);',                         # a type the header does not use
    'int f(int);',                              # a parameter without a name
    'int f(int n[4]);',                         # an array parameter
    'int f(int (*callback)(int));',             # a function pointer
    'typedef struct { int32_t a : 3; } asac_s_t;',
    'typedef struct { asac_later_t x; } asac_s_t;',
    'typedef struct { int32_t a; int32_t a; } asac_s_t;',
    'typedef struct { int32_t w[ASAC_UNKNOWN]; } asac_s_t;',
    'struct tagged { int32_t a; };',
    'static inline int f(int a) { return a; }',
    'int f(int a);\nint f(int a);',
    'int a, f(int b);',
    'int f(void x, int y)[2];',
    '#define ASAC_X (2 * 3)',
    '#pragma once',
    'int f(int a)',                             # no semicolon
    '/* never closed\nint f(int a);',
])
def test_unknown_text_raises(text):
    with pytest.raises(abi.AbiParseError):
        abi.parse(text)


def test_the_header_itself():
    assert len(abi.functions) >= 216 and len(abi.structs) >= 31
    assert abi.defines['ASAC_ABI_VERSION'] >= 91 and abi.defines['ASAC_PAD_EMIT_MASK'] == 4 and abi.defines['ASAC_GATE_MAX_N'] == 1 << 20
    assert abi.HEADER_PATH == INCLUDE / 'asac_hip.h'
    from asac_amd import native
    assert tuple(abi.functions) == native.EXPORTED_SYMBOLS
    held = {cls.c_name: cls for cls in vars(native).values() if isinstance(cls, type) and issubclass(cls, C.Structure)}
    assert set(held) == set(abi.structs) and all(abi.ctypes_struct(name) is cls for name, cls in held.items())
    with pytest.raises(abi.AsacNativeError):     # a struct of the header the binding does not name
        abi.signatures([cls for cls in held.values() if cls is not native.RndGrads])


def test_a_missing_header_is_named(monkeypatch, tmp_path):
    monkeypatch.setattr(abi, 'HEADER_PATH', tmp_path / 'include' / 'asac_hip.h')
    with pytest.raises(abi.AsacNativeError, match=re.escape(str(tmp_path / 'include' / 'asac_hip.h'))):
        abi._read_header()


# ------------------------------------------------------------------------------------------------ 2. layouts
def _host_cc():
    cc = shutil.which('cc')
    if cc:
        return cc
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    for clang in (Path(hipcc).resolve().parent / 'clang', Path(hipcc).resolve().parent.parent / 'llvm' / 'bin' / 'clang',
                  Path(hipcc).resolve().parent.parent / 'lib' / 'llvm' / 'bin' / 'clang'):
        if clang.exists():
            return str(clang)
    raise AssertionError('no host C compiler: neither `cc` nor the clang beside hipcc')


def test_every_struct_layout_is_the_host_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "asac_hip.h"', 'int main(void) {']
    for name, fields in abi.structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, *_ in fields:
            lines.append(f'  printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
    (tmp_path / 'layout.c').write_text('\n'.join(lines + ['  return 0;', '}', '']))
    subprocess.run([_host_cc(), '-std=c99', '-Wall', '-Werror', '-I', str(INCLUDE), str(tmp_path / 'layout.c'),
                    '-o', str(tmp_path / 'layout')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout
    compiled = {words[0]: tuple(int(w) for w in words[1:]) for words in (line.split() for line in out.splitlines())}
    n_fields = 0
    for name, fields in abi.structs.items():
        cls = abi.ctypes_struct(name)
        assert [f for f, _ in cls._fields_] == [f for f, *_ in fields], name
        assert compiled.pop(name) == (C.sizeof(cls),), name
        for field, *_ in fields:
            member = getattr(cls, field)
            assert compiled.pop(f'{name}.{field}') == (member.offset, member.size), f'{name}.{field}'
            n_fields += 1
    assert not compiled     # nothing the C program printed was left unchecked
    assert len(abi.structs) >= 31 and n_fields == sum(len(f) for f in abi.structs.values()) >= 318
    print(f'{len(abi.structs)} structs, {n_fields} fields, 0 skipped')


# ------------------------------------------------------------------------------------------------ 3. signatures, the dumb way
_WIDTH = {'int': (4, 'i'), 'int32_t': (4, 'i'), 'int64_t': (8, 'i'), 'uint32_t': (4, 'i'), 'uint64_t': (8, 'i'),
          'uint8_t': (1, 'i'), 'float': (4, 'f'), 'double': (8, 'f')}


def _kind(ctype):
    return 'f' if ctype in (C.c_float, C.c_double) else 'i'


def test_argument_counts_and_scalar_widths_against_the_header_text():
    from asac_amd import native
    text = re.sub(r'/\*.*?\*/', '', (INCLUDE / 'asac_hip.h').read_text(), flags=re.S)
    checked = 0
    for name, (res, args) in native._SIGNATURES.items():
        m = re.search(r'([\w*]+)\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert m, name
        params = [p.strip() for p in m.group(2).split(',') if p.strip() != 'void']
        assert len(args) == len(params), name
        for p, ctype in zip(params, args):
            if '*' in p:
                assert C.sizeof(ctype) == C.sizeof(C.c_void_p), (name, p)
            else:
                before_name = p.split()[-2]
                assert (C.sizeof(ctype), _kind(ctype)) == _WIDTH[before_name], (name, p)
            checked += 1
        if '*' in m.group(1):
            assert res is C.c_char_p, name
        else:
            assert (C.sizeof(res), _kind(res)) == _WIDTH[m.group(1)], name
    assert len(native._SIGNATURES) >= 216 and checked > 2000


# ------------------------------------------------------------------------------------------------ 4. what the wrappers pass
def _accepts(name, param, value):
    from asac_amd import native
    index = [p for p, _, _ in abi.functions[name][1]].index(param)
    native._SIGNATURES[name][1][index].from_param(value)


def test_changed_argtypes_take_what_the_wrappers_pass():
    from asac_amd import native
    gru = ('asac_gru_forward', 'asac_gru_forward_twin', 'asac_gru_backward', 'asac_gru_backward_at')
    for name in gru:                                            # `_gru_arrays`: one pointer a layer
        for param in ('w_ih', 'w_hh', 'b_ih', 'b_hh') + (('twin_w_ih', 'twin_w_hh', 'twin_b_ih', 'twin_b_hh')
                                                         if name.endswith('_twin') else ()):
            _accepts(name, param, native._PtrArray())
    for name in gru[2:]:
        _accepts(name, 'grad_param_tensors', (C.c_void_p * (4 * native.GRU_MAX_LAYERS))())
    for name in ('asac_attention_proj_forward', 'asac_attention_proj_backward'):
        _accepts(name, 'params_host', (C.c_void_p * 8)())
    for name in ('asac_window_gather_plan', 'asac_window_gather_plan_w'):
        _accepts(name, 'blocks_out', C.byref(C.c_int(0)))
    for param in ('n_replaced', 'n_kept'):
        _accepts('asac_graph_replace_memset_nodes', param, C.byref(C.c_int(0)))
    _accepts('asac_graph_replace_memset_nodes', 'graph', C.c_void_p(0x1000))
    _accepts('asac_conv2_backward_multi', 'grad_ys', (C.c_void_p * 3)(0x1000, 0x2000, 0x3000))
    _accepts('asac_cosine_gate_add', 'aux_host', (C.c_void_p * 2)(0x1000, 0x2000))
    for name in ('asac_drnd_distill', 'asac_drnd_pick'):
        _accepts(name, 'residual', native._residual2((True, False)))
        for param in ('predictors', 'targets'):                # a `drnd_table`'s device address, or None
            _accepts(name, param, native._table_p(None, native.RndStack))
            _accepts(name, param, C.cast(C.c_void_p(0x1000), C.POINTER(native.RndStack)))
    _accepts('asac_drnd_param_grads', 'grads', native._table_p(None, native.RndGrads))
    _accepts('asac_drnd_param_grads', 'grads', C.cast(C.c_void_p(0x1000), C.POINTER(native.RndGrads)))
    for name in ('asac_rnd_distill', 'asac_rnd_pick'):          # host structs by reference, as before
        for param in ('predictor', 'target'):
            _accepts(name, param, C.byref(native.RndStack()))
    _accepts('asac_gru_backward_at', 'adam', C.byref(native.AdamEpilogue()))
    _accepts('asac_gru_backward_at', 'adam', None)
    with pytest.raises(TypeError):                              # what the typed pointers are for
        _accepts('asac_gru_backward_at', 'adam', C.byref(native.RndStack()))
