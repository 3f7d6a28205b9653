"""The C ABI of `libasac_hip.so`, read from `include/asac_hip.h`: the header is the one description of the entry points
and structs, and the ctypes binding (`native.py`) is built from it.  Standard library only (no torch).

`parse(text)` understands the plain C the header is written in: comments, `#define NAME <integer>` (also `(a << b)`),
anonymous `enum { NAME = <integer>, ... };` (its constants join `defines`), `typedef struct { ... } name_t;` and function
declarations.  Anything else raises `AbiParseError` with the offending text; nothing is guessed.

Typing rule (the only one; struct fields and parameters alike):

    int, int32_t, int64_t, uint32_t, uint64_t, uint8_t, float, double by value    the matching ctypes scalar
    const char* (parameter or return)                                            c_char_p
    asac_*_t*                                     POINTER(<that struct's class>): takes byref(x), an array of it, None
    every other pointer (T*, T**, T* const*, void*)                              c_void_p
    struct field  T name[N]  /  T* name[N]                                       scalar * N  /  c_void_p * N
    struct field  asac_*_t name                                                  that struct's class, by value
"""
import ctypes as C
import re
from pathlib import Path
from typing import NamedTuple

PKG_DIR = Path(__file__).resolve().parent
HEADER_PATH = PKG_DIR.parent / 'include' / 'asac_hip.h'     # the file csrc/build.py compiles against


class AsacNativeError(RuntimeError):
    pass


class AbiParseError(ValueError):
    pass


SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64,
           'uint8_t': C.c_uint8, 'float': C.c_float, 'double': C.c_double}
_POINTEE_ONLY = {'void', 'char', 'unsigned int'}     # base types that occur behind a pointer only


class Abi(NamedTuple):
    defines: dict     # {name: int}
    structs: dict     # {c_name: [(field, base_type, pointer_depth, array_len | None), ...]} in header order
    functions: dict   # {name: (return_type, [(param_name, base_type, pointer_depth), ...])} in header order


def _integer(text, defines, where):
    text = text.strip()
    m = re.fullmatch(r'\(\s*(\d+)\s*<<\s*(\d+)\s*\)', text)
    if m:
        return int(m.group(1)) << int(m.group(2))
    if re.fullmatch(r'\d+', text):
        return int(text)
    if text in defines:
        return defines[text]
    raise AbiParseError(f'{where}: not an integer: {text!r}')


def _declarators(text, bases, defines):
    """`const float *a, *b[4]` -> [('a', 'float', 1, None), ('b', 'float', 1, 4)]: one base type (a name of `bases`),
    then comma-separated declarators of stars, a name and at most one array length"""
    tokens = re.findall(r'\w+|[*,\[\]]', text)
    if ''.join(tokens) != re.sub(r'\s+', '', text):
        raise AbiParseError(f'unrecognised declaration: {text.strip()!r}')
    tokens = [t for t in tokens if t != 'const']
    n = 2 if ' '.join(tokens[:2]) in bases else 1      # the base type is one word, or two (`unsigned int`)
    base, out = ' '.join(tokens[:n]), []
    if base not in bases:
        raise AbiParseError(f'unknown type in declaration: {text!r}')
    rest = ' '.join(tokens[n:])
    for decl in rest.split(','):
        m = re.fullmatch(r'\s*((?:\*\s*)*)([A-Za-z_]\w*)\s*(?:\[\s*(\w+)\s*\])?\s*', decl)
        if not m or m.group(2) in bases:
            raise AbiParseError(f'unrecognised declarator {decl.strip()!r} in: {text!r}')
        length = None if m.group(3) is None else _integer(m.group(3), defines, text)
        out.append((m.group(2), base, m.group(1).count('*'), length))
    return out


def parse(text: str) -> Abi:
    defines, structs, functions = {}, {}, {}
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    if '/*' in text or '*/' in text:
        raise AbiParseError('unterminated comment')
    code = []
    for line in text.splitlines():
        if not line.lstrip().startswith('#'):
            code.append(line)
            continue
        words = line.split(None, 2)
        if words[0] == '#define' and len(words) == 3:
            defines[words[1]] = _integer(words[2], defines, line.strip())
        elif not (words[0] in ('#ifndef', '#ifdef', '#endif', '#include') or (words[0] == '#define' and len(words) == 2)):
            raise AbiParseError(f'unrecognised preprocessor line: {line.strip()!r}')
    text = '\n'.join(code)
    text, n_open = re.subn(r'extern\s+"C"\s*\{', ' ', text)
    if n_open:       # its closing brace: the only one outside a struct or enum body
        head, brace, tail = text.rpartition('}')
        if tail.strip():
            raise AbiParseError(f'unrecognised text after extern "C": {tail.strip()!r}')
        text = head
    pos = 0
    statement = re.compile(r'\s*(?:typedef\s+struct\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)|enum\s*\{(?P<enum>[^{}]*)\}'
                           r'|(?P<head>[^;{}()]*)\((?P<params>[^;{}()]*)\))\s*;', re.S)
    while text[pos:].strip():
        m = statement.match(text, pos)
        if not m:
            raise AbiParseError(f'unrecognised declaration: {text[pos:].strip()[:120]!r}')
        pos = m.end()
        bases = set(SCALARS) | _POINTEE_ONLY | set(structs)
        if m.group('struct'):
            fields = []
            for decl in m.group('fields').split(';'):
                if decl.strip():
                    fields += _declarators(decl, bases, defines)
            names = [f[0] for f in fields]
            if not fields or len(set(names)) != len(names) or m.group('struct') in structs:
                raise AbiParseError(f'empty struct, or a name declared twice: {m.group("struct")}')
            structs[m.group('struct')] = fields
        elif m.group('enum') is not None:
            for item in m.group('enum').split(','):
                name, eq, value = item.partition('=')
                if not eq or not re.fullmatch(r'\s*\w+\s*', name):
                    raise AbiParseError(f'unrecognised enumerator: {item.strip()!r}')
                defines[name.strip()] = _integer(value, defines, item.strip())
        else:
            heads = _declarators(m.group('head'), bases, defines)
            if len(heads) != 1:
                raise AbiParseError(f'unrecognised declaration: {m.group(0).strip()!r}')
            (name, base, depth, length), params = heads[0], []
            if m.group('params').strip() != 'void':
                for p in m.group('params').split(','):
                    (pname, pbase, pdepth, plen), = _declarators(p, bases, defines)
                    if plen is not None:
                        raise AbiParseError(f'array parameter in {name}: {p.strip()!r}')
                    params.append((pname, pbase, pdepth))
            if length is not None or name in functions:
                raise AbiParseError(f'unrecognised or repeated function declaration: {name}')
            functions[name] = (base + '*' * depth, params)
    return Abi(defines, structs, functions)


def _read_header() -> Abi:
    if not HEADER_PATH.is_file():
        raise AsacNativeError(f'{HEADER_PATH} is missing: the ctypes binding of libasac_hip.so is built from it')
    return parse(HEADER_PATH.read_text())


defines, structs, functions = _read_header()      # once per process: at the first import of this module
_classes = {}


def _ctype(base, depth, where):
    if depth == 0:
        if base in SCALARS:
            return SCALARS[base]
        if base in structs:
            return ctypes_struct(base)
        raise AbiParseError(f'{where}: `{base}` by value has no ctypes type')
    if depth == 1 and base == 'char':
        return C.c_char_p
    if depth == 1 and base in structs:
        return C.POINTER(ctypes_struct(base))
    return C.c_void_p


def ctypes_struct(c_name: str):
    """the `ctypes.Structure` of a struct of the header (fields in the header's order), built once"""
    if c_name not in _classes:
        fields = []
        for field, base, depth, length in structs[c_name]:
            t = _ctype(base, depth, f'{c_name}.{field}')
            fields.append((field, t if length is None else t * length))
        _classes[c_name] = type(c_name, (C.Structure,), {'_fields_': fields, 'c_name': c_name})
    return _classes[c_name]


def signatures(struct_classes) -> dict:
    """{entry point: (restype, [argtypes])} for every function of the header.  `struct_classes`: the classes the caller
    holds (from `ctypes_struct`); every struct of the header must be among them, so that the binding names each one."""
    struct_classes = tuple(struct_classes)
    held = {name for name, cls in _classes.items() if cls in struct_classes}
    if held != set(structs):
        raise AsacNativeError(f'structs of {HEADER_PATH.name} without a class in the binding: {sorted(set(structs) - held)}')
    return {name: (_ctype(ret.rstrip('*'), ret.count('*'), name),
                   [_ctype(base, depth, f'{name}({pname})') for pname, base, depth in params])
            for name, (ret, params) in functions.items()}
