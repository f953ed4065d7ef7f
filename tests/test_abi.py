"""The C-ABI library loads without a GPU and exports every symbol include/nexoclom_hip.h
declares; the ctypes structures match the header's layout and the ctypes signatures its
prototypes; GPU-less calls fail loudly."""
import ctypes as C
import os
import re

import pytest

from nexoclom_amd import hip_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nexoclom_hip.h')


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(nxc_[a-z0-9_]+)\s*\(', text)))


SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint8_t': C.c_uint8,
           'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64, 'float': C.c_float,
           'double': C.c_double, 'char': C.c_char}
OPAQUE = ('nxc_handle', 'nxc_rows', 'nxc_pairs', 'void')
RETURNS = {'int': C.c_int, 'const char *': C.c_char_p}


def ctype_of(parameter):
    """The ctypes type of one C parameter as hip_api spells it: const and the name dropped,
    ``name[N]`` a pointer, opaque types void; ValueError for anything else."""
    m = re.fullmatch(r'(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?\s*(\[\w*\])?',
                     parameter)
    if not m:
        raise ValueError(f'no translation for the parameter {parameter!r}')
    base, stars, _, array = m.groups()
    depth = stars.count('*') + bool(array)
    struct = getattr(hip_api, base, None) if base.startswith('nxc_') else None
    if base in OPAQUE and depth in (1, 2):
        return C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)
    if isinstance(struct, type) and issubclass(struct, C.Structure) and depth == 1:
        return C.POINTER(struct)
    if base in SCALARS and depth <= 2:
        ct = SCALARS[base]
        for _ in range(depth):
            ct = C.POINTER(ct)
        return ct
    raise ValueError(f'no translation for the parameter {parameter!r}')


def header_signatures(text):
    """{name: (restype, argtypes)} of every ``ret nxc_name(args);`` of the header text."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = {}
    prototype = r'^([\w \t*]+?)\s*\b(nxc_\w+)\s*\(([^()]*)\)\s*;'
    for ret, name, args in re.findall(prototype, text, flags=re.M):
        if ret.strip() not in RETURNS:
            raise ValueError(f'no translation for the return type {ret!r} of {name}')
        args = [' '.join(a.split()) for a in args.split(',')]
        found[name] = (RETURNS[ret.strip()],
                       () if args == ['void'] else tuple(ctype_of(a) for a in args))
    # no prototype escapes the pattern: every nxc_ name followed by '(' is one of them
    assert sorted(found) == sorted(set(re.findall(r'\b(nxc_[a-z0-9_]+)\s*\(', text)))
    return found


def signature_drift(text):
    """The functions whose header prototype and hip_api.SIGNATURES entry differ (either way)."""
    header = header_signatures(text)
    table = {name: (hip_api.RESTYPES.get(name, C.c_int), argtypes)
             for name, argtypes in hip_api.SIGNATURES.items()}
    return sorted(name for name in set(header) | set(table) if header.get(name) != table.get(name))


def test_signatures_match_header():
    assert len(hip_api.SIGNATURES) >= 126 and hip_api.EXPORTS == tuple(hip_api.SIGNATURES)
    assert signature_drift(open(HEADER).read()) == []
    lib = hip_api.load_library()
    for name, argtypes in hip_api.SIGNATURES.items():
        entry = getattr(lib, name)
        assert tuple(entry.argtypes) == argtypes, name
        assert entry.restype is hip_api.RESTYPES.get(name, C.c_int), name
    with pytest.raises(ValueError, match='long double'):
        header_signatures('int nxc_new(nxc_handle *h, long double x);')
    with pytest.raises(ValueError, match='return type'):
        header_signatures('float nxc_new(nxc_handle *h);')


def test_signature_check_sees_a_drift():
    text = open(HEADER).read()
    narrowed = text.replace('int nxc_set_first_index(nxc_handle *h, int64_t first_index);',
                            'int nxc_set_first_index(nxc_handle *h, int32_t first_index);')
    assert narrowed != text and signature_drift(narrowed) == ['nxc_set_first_index']
    shorter = text.replace('int64_t first, int64_t count,\n                      void *cols_out,',
                           'int64_t first,\n                      void *cols_out,')
    assert shorter != text and signature_drift(shorter) == ['nxc_rows_download']


def test_calls_are_checked():
    """ctypes refuses a call that does not fit its declared signature, before it is made; a call
    that fits goes through (and fails in the library: no handle)."""
    lib = hip_api.load_library()
    with pytest.raises(C.ArgumentError):
        lib.nxc_set_first_index(None, 1.5)
    with pytest.raises(TypeError):
        lib.nxc_set_first_index(None)
    assert lib.nxc_set_forces(None, None) != 0
    assert b'null' in lib.nxc_last_error_string()


def test_library_exports_every_declared_symbol():
    lib = hip_api.load_library()
    names = declared_functions()
    assert len(names) >= 25
    for name in names:
        assert hasattr(lib, name), f'{name} declared in nexoclom_hip.h but not exported'
    assert set(names) == set(hip_api.EXPORTS)
    assert lib.nxc_abi_version() == hip_api.ABI_VERSION == 3


def test_struct_layouts_match_header():
    # nxc_forces: 4 doubles, 4 int32, int64, 2 pointers
    assert C.sizeof(hip_api.nxc_forces) == 4*8 + 4*4 + 8 + 2*8
    # nxc_image_desc: 9+2 doubles, 4 int32, 2 int64, 2 ptr, 4 int64, 4+4 ptr
    assert C.sizeof(hip_api.nxc_image_desc) == 11*8 + 4*4 + 2*8 + 2*8 + 4*8 + 8*8
    assert C.sizeof(hip_api.nxc_counters) == 8*8
    assert hip_api.nxc_forces.n_tab.offset == 48
    assert hip_api.nxc_image_desc.nx.offset == 104


def test_no_gpu_means_loud_failure_not_fallback():
    if hip_api.device_count() > 0:
        pytest.skip('a GPU is visible here')
    with pytest.raises(hip_api.HipError):
        hip_api.Context(0)
    lib = hip_api.load_library()
    assert lib.nxc_set_forces(None, None) != 0
    assert b'null' in lib.nxc_last_error_string()


def test_package_does_not_import_the_oracle():
    """Product code must never route through oracle/ (or any CPU integrator)."""
    pkg = os.path.join(ROOT, 'nexoclom_amd')
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(('.py', '.hip', '.hpp', '.h')):
                src = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), fn
                assert 'oracle_math.h' not in src and 'liboracle' not in src, fn
    # tools/ are measurement helpers of the product: no oracle there either, directly or through
    # the test helpers (scripts that need them live in tests/tools/)
    for fn in os.listdir(os.path.join(ROOT, 'tools')):
        if fn.endswith('.py'):
            src = open(os.path.join(ROOT, 'tools', fn)).read()
            assert not re.search(r'^\s*(from|import)\s+(oracle|tests)\b', src, flags=re.M), fn
    # bench.py touches the oracle only inside its cpu_baseline leg; __graft_entry__ only in smoke()
    import ast
    for fn, allowed in (('bench.py', {'cpu_baseline'}), ('__graft_entry__.py', {'smoke'})):
        tree = ast.parse(open(os.path.join(ROOT, fn)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.FunctionDef):
                uses = any(isinstance(n, (ast.Import, ast.ImportFrom)) and
                           ('oracle' in (getattr(n, 'module', '') or '') or
                            any('oracle' in a.name for a in n.names))
                           for n in ast.walk(node))
                assert not uses or node.name in allowed, (fn, node.name)
        for node in tree.body:          # and never at module level
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                mod = getattr(node, 'module', '') or ''
                assert 'oracle' not in mod and all('oracle' not in a.name for a in node.names), fn


def test_ctypes_structs_match_the_compiled_header(tmp_path):
    """Every struct of include/nexoclom_hip.h as gcc lays it out (sizeof and the offset of each
    field) against the ctypes mirror in hip_api.py: a field added on one side only shows up here."""
    import subprocess
    import sys
    structs = [name for name, ct in vars(hip_api).items() if name.startswith('nxc_')
               and isinstance(ct, type) and issubclass(ct, C.Structure)]
    assert len(structs) >= 14
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for name in structs:
        ct = getattr(hip_api, name)
        lines.append(f'printf("{name} %zu", sizeof({name}));')
        for field, *_ in ct._fields_:
            lines.append(f'printf(" %zu", offsetof({name}, {field}));')
        lines.append('printf("\\n");')
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', str(src), '-o', str(exe)])
    out = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    assert len(out) == len(structs)
    for row in out:
        name, size, *offsets = row.split()
        ct = getattr(hip_api, name)
        assert int(size) == C.sizeof(ct), name
        assert [int(o) for o in offsets] == [getattr(ct, f).offset for f, *_ in ct._fields_], name
