"""The ctypes binding is derived from the C headers: the parser's rules on small header texts, the derived struct layouts against
what a C compiler lays out, and the coverage of the two real headers (host only, no compute calls)."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from conftest import REPO
from test_cabi_symbols import _declared_symbols

PARAMS = 'typedef struct ss_hll_params { int32_t p; const float *bias; } ss_hll_params;\n'


def _native():
    import subgraph_sketching_amd as ssa
    return ssa._native


def _parse(text):
    return _native().parse([('small.h', text)])


def _argtypes(params, before=''):
    return _parse(before + f'int ss_f({params});')[2]['ss_f'][1]


@pytest.mark.parametrize('param, expected', [
    ('const uint32_t *const *mh', POINTER(c_void_p)), ('void *stream', c_void_p), ('size_t n', c_size_t), ('double alpha', c_double),
    ('uint64_t seed', c_uint64), ('uint32_t flags', c_uint32), ('int64_t N', c_int64), ('int32_t P', c_int32), ('int code', c_int32),
    ('const uint8_t *regs', c_void_p), ('const float *e', c_void_p), ('const char *name', c_void_p), ('struct ss_hll_params **all', POINTER(c_void_p)),
])
def test_parameter_types(param, expected):
    assert _argtypes(param, PARAMS) == [expected]
    assert _argtypes(f'int32_t first, {param}', PARAMS) == [c_int32, expected]


def test_pointer_to_an_earlier_struct():
    defines, structs, signatures = _parse(PARAMS + 'int ss_f(const ss_hll_params *prm, const struct ss_hll_params *again);')
    assert signatures['ss_f'] == (c_int32, [POINTER(structs['ss_hll_params'])] * 2)


def test_return_types_void_list_and_broken_lines():
    text = ('/* a comment with int ss_hidden(void); inside */\n#ifndef SMALL_H\n#define SMALL_H\n#include <stdint.h>\n'
            '#ifdef __cplusplus\nextern "C" {\n#endif\n'
            'const char *ss_error_string(int code);\nsize_t ss_bytes(int64_t N,\n      int64_t E);\nint ss_version(void);\n'
            'int64_t ss_calls(int32_t reset); /* trailing */\nint ss_wide(const int64_t *src, /* between */ int32_t *col,\n\n   void *stream);\n'
            '#ifdef __cplusplus\n}\n#endif\n#endif\n')
    defines, structs, signatures = _parse(text)
    assert (defines, structs) == ({}, {})
    assert signatures == {'ss_error_string': (c_char_p, [c_int32]), 'ss_bytes': (c_size_t, [c_int64, c_int64]), 'ss_version': (c_int32, []),
                          'ss_calls': (c_int64, [c_int32]), 'ss_wide': (c_int32, [c_void_p, c_void_p, c_void_p])}


def test_struct_fields_arrays_and_the_offset_after_them():
    structs = _parse(PARAMS + 'typedef struct ss_g {\n  const int64_t *rowptr; /* device */\n  int32_t n;\n  uint32_t *mirror[7];\n  uint8_t *b[3];\n'
                     '  float bias;\n  const ss_hll_params *prm;\n  double z; } ss_g;')[1]
    g = structs['ss_g']
    assert [name for name, _ in g._fields_] == ['rowptr', 'n', 'mirror', 'b', 'bias', 'prm', 'z']
    assert [getattr(g, name).offset for name, _ in g._fields_] == [0, 8, 16, 72, 96, 104, 112] and ctypes.sizeof(g) == 120
    assert g.mirror.size == 56 and g.b.size == 24 and dict(g._fields_)['prm'] == POINTER(structs['ss_hll_params'])
    assert g(n=5, bias=0.5).n == 5


@pytest.mark.parametrize('value, expected', [('123', 123), ('4u', 4), ('(-4)', -4), ('(1 << 20)', 1 << 20), ('0', 0)])
def test_integer_defines(value, expected):
    text = f'#define SMALL_H\n#define SS_NAME {value}   /* what it is for */\n#define OTHER_THING some text\n'
    assert _parse(text)[0] == {'SS_NAME': expected}


@pytest.mark.parametrize('text, quoted', [
    ('int ss_f(long n);', 'long n'),                                                  # an unknown type name
    ('int ss_f(unsigned int n);', 'unsigned int n'),
    ('int ss_f(uint8_t byte);', 'uint8_t byte'),                                      # uint8_t is bound as a pointee only
    ('long ss_f(int32_t n);', 'long ss_f(int32_t n);'),
    ('int ss_f(int32_t n, int (*cb)(int32_t));', 'int ss_f(int32_t n, int (*cb)(int32_t))'),   # a function pointer
    ('typedef struct ss_s { void (*cb)(void); } ss_s;', 'void (*cb)(void)'),
    (PARAMS + 'int ss_f(ss_hll_params prm);', 'ss_hll_params prm'),                    # a struct by value
    (PARAMS + 'typedef struct ss_s { ss_hll_params prm; } ss_s;', 'ss_hll_params prm'),
    ('int ss_f(const ss_later *prm);', 'const ss_later *prm'),                        # a struct not declared earlier
    ('typedef struct ss_s { uint32_t flags : 3; } ss_s;', 'uint32_t flags : 3'),      # a bit-field
    ('int ss_f(const char *fmt, ...);', '...'),                                       # a variadic list
    ('int ss_f(int32_t ***deep);', 'int32_t ***deep'),
    ('int ss_f(uint32_t *rows[7]);', 'uint32_t *rows[7]'),                            # arrays are for fields
    ('typedef struct ss_s { int32_t counts[4]; } ss_s;', 'int32_t counts[4]'),        # ... and of pointers only
    ('int ss_f(int32_t);', 'int ss_f(int32_t);'),                                     # a parameter without a name
    ('int ss_f();', 'int ss_f();'),
    ('#define SS_RATIO 0.5', '#define SS_RATIO 0.5'),                                 # defines that are no integer
    ('#define SS_BOTH (SS_A | SS_B)', '#define SS_BOTH (SS_A | SS_B)'),
    ('#define SS_MIN(a, b) ((a) < (b) ? (a) : (b))', '#define SS_MIN(a, b)'),
    ('#define SS_EMPTY', '#define SS_EMPTY'),
    ('#define SS_LONG 5ul', '#define SS_LONG 5ul'),
    ('int ss_f(void);\nstatic inline int ss_g(void) { return 0; }', 'static inline int ss_g(void) {'),   # text between declarations
    ('int ss_f(void);\nint ss_g(void)', 'int ss_g(void)'),
    ('int ss_f(void); // a C++ comment', '// a C++ comment'),
    ('typedef struct ss_s { int32_t n; } ss_t;', 'typedef struct ss_s { int32_t n; } ss_t;'),
    ('typedef int32_t ss_id;', 'typedef int32_t ss_id;'),
    ('struct ss_s;', 'struct ss_s;'),
    ('typedef struct ss_s { union { int32_t a; float b; } u; } ss_s;', 'typedef struct ss_s { union {'),
])
def test_what_the_parser_cannot_read_is_refused(text, quoted):
    with pytest.raises(ValueError) as err:
        _parse(text)
    assert 'small.h' in str(err.value) and quoted in str(err.value)


def _compiler():
    hipcc = shutil.which('hipcc')   # what build() compiles with: <ROCm>/bin/hipcc, its clang at <ROCm>/llvm/bin/clang
    rocm = os.environ.get('ROCM_PATH') or (os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else '/opt/rocm')
    for cc in ('cc', os.path.join(rocm, 'llvm', 'bin', 'clang')):
        if shutil.which(cc):
            return shutil.which(cc)
    pytest.fail('no C compiler found (cc, or the clang of the ROCm installation): build() needs one on the same machine')


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof of every derived struct, offsetof and size of every field, against a C99 program compiled from the same headers"""
    native = _native()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "subgraph_sketch.h"', '#include "subgraph_sketch_debug.h"', 'int main(void) {']
    expected = []
    for tag, struct in native.STRUCTS.items():
        lines.append(f'  printf("{tag} %zu\\n", sizeof({tag}));')
        expected.append(f'{tag} {ctypes.sizeof(struct)}')
        for name, _ in struct._fields_:
            lines.append(f'  printf("{tag}.{name} %zu %zu\\n", offsetof({tag}, {name}), sizeof((({tag} *)0)->{name}));')
            expected.append(f'{tag}.{name} {getattr(struct, name).offset} {getattr(struct, name).size}')
    (tmp_path / 'layout.c').write_text('\n'.join(lines + ['  return 0;', '}', '']))
    exe = str(tmp_path / 'layout')
    subprocess.run([_compiler(), '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), str(tmp_path / 'layout.c'), '-o', exe],
                   check=True)
    printed = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(expected) == sum(1 + len(s._fields_) for s in native.STRUCTS.values()) >= 53
    assert printed == expected


def test_every_declared_entry_point_is_bound_and_nothing_else():
    native = _native()
    assert sorted(native.SIGNATURES) == _declared_symbols()
    assert list(native.STRUCTS) == ['ss_hll_params', 'ss_csr_graph', 'ss_structure_head', 'ss_ppr_graph']
    assert (native.HllParams, native.CsrGraphStruct, native.StructureHeadStruct, native.PprGraphStruct) == tuple(native.STRUCTS.values())


def test_restypes_are_what_the_headers_declare():
    native = _native()
    declared = {}   # a scan of its own: what stands between the start of a line and an entry point's name
    for header in ('subgraph_sketch.h', 'subgraph_sketch_debug.h'):
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', header)).read(), flags=re.S)
        declared.update({name: res.strip() for res, name in re.findall(r'^(\w[\w \t]*?[ \t*]+)(ss_\w+)[ \t]*\(', text, flags=re.M)})
    assert sorted(declared) == _declared_symbols()
    by_text = {'int': c_int32, 'size_t': c_size_t, 'int64_t': c_int64, 'const char *': c_char_p}
    assert {name: res for name, (res, _) in native.SIGNATURES.items()} == {name: by_text[res] for name, res in declared.items()}
    other = {name: res for name, (res, _) in native.SIGNATURES.items() if res is not c_int32}
    byte_counts = {name: c_size_t for name in native.SIGNATURES if name.endswith('_bytes')}
    assert other == {**byte_counts, 'ss_error_string': c_char_p, 'ss_debug_hub_calls': c_int64}


def test_constants_are_the_headers_defines():
    native = _native()
    defines = native.DEFINES
    assert len(defines) == 41 and defines['SS_ERR_UNSUPPORTED'] == -4 and defines['SS_FLAG_MASK_TARGET'] == 4
    assert defines['SS_SUBGRAPH_MAX_DIST'] == 1 << 20
    aliases = ('SS_MAX_HOPS SS_MAX_TABLE SS_FLAG_USE_ZERO_ONE SS_FLAG_FLOOR_SF SS_FLAG_MASK_TARGET SS_CSR_ERR_BOUNDS SS_CSR_ERR_PROTOCOL '
               'GRAPH_HOP_TABLES MAX_MIRRORS PPR_SEGMENT PPR_MAX_COLUMNS PROF_MINHASH_HOP PROF_HLL_HOP PROF_FIRST_HOP_MH PROF_FIRST_HOP_HLL '
               'PROF_PAIRS PROF_CSR PROF_HUB PROF_FUSED PROF_MINHASH_ROWS MEGA_SLICE MEGA_SLOT_BYTES MEGA_DESC_WORDS CSR_FINGERPRINT_BYTES '
               'NEG_MAX_TRIES SUBGRAPH_MAX_DIST COMPONENTS_CHUNK WEDGE_MAX_SLOTS').split()
    for alias in aliases:
        assert getattr(native, alias) == defines[alias if alias.startswith('SS_') else 'SS_' + alias], alias
    assert native.NEG_MODES == {'uniform': defines['SS_NEG_UNIFORM'], 'same_source': defines['SS_NEG_SAME_SOURCE'], 'wedge': defines['SS_NEG_WEDGE']}
    assert native.SUBGRAPH_LABELS == {'drnl': defines['SS_SUBGRAPH_LABEL_DRNL'], 'de': defines['SS_SUBGRAPH_LABEL_DE'],
                                      'de+': defines['SS_SUBGRAPH_LABEL_DE_PLUS']}
    assert defines['SS_PROF_TAGS'] == 1 + max(getattr(native, a) for a in aliases if a.startswith('PROF_'))
    assert (native.ABI_VERSION, native.WEDGE_MAX_SLICES) == (129, 64)   # the two values no header defines
