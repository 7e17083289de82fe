"""ctypes binding of the C-ABI library, derived at import from include/subgraph_sketch.h and include/subgraph_sketch_debug.h.

The headers are the only description of the boundary: `parse` reads them into DEFINES (every `#define SS_NAME <integer>`),
STRUCTS (one ctypes.Structure per `typedef struct`) and SIGNATURES (name -> (restype, argtypes)), and `lib()` applies SIGNATURES
to the loaded handle.  The parser knows the subset of C the two headers keep to, and nothing else:
  - comments are `/* */`; preprocessor lines other than the integer defines, and `extern "C" {` with its closing brace, are skipped;
  - a declaration is `typedef struct NAME { fields } NAME;` or a prototype `T name(T a, T b);` / `T name(void);`
  - after dropping `const` and `struct`, a type is a scalar (int, int32_t, uint32_t, int64_t, uint64_t, size_t, float, double), a
    pointer to a struct declared earlier (POINTER(that struct)), any other single pointer -- to void, a scalar, uint8_t or char --
    (c_void_p; a returned `char *` is c_char_p), or a double pointer to any of these (POINTER(c_void_p)); a field may be an array
    of single pointers `T *name[K]` (c_void_p * K);
  - an integer is `123`, `123u`, `(-1)` or `(1 << 20)`.
Anything else -- another type name, a function pointer, a struct by value, a bit-field, `...`, an `SS_` define that is no integer,
text between declarations -- raises ValueError at import, naming the header and quoting the declaration: a header edit the binding
cannot read fails the host tests instead of reaching a launch with a guessed type.

The HIP library is the product: there is no CPU fallback.  `lib()` raises loudly when the shared
object has not been built (run `python __graft_entry__.py` or `subgraph-sketching_amd/csrc/build.sh`).
"""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(_HERE, '..', 'include')
_HEADERS = ('subgraph_sketch.h', 'subgraph_sketch_debug.h')  # in this order: the second uses the structs of the first
# (SS_LIB: measurement hook -- tools/ab_variant.sh loads a scratch build of the library beside the product's)
LIB_PATH = os.environ.get('SS_LIB') or os.path.join(_HERE, 'libsubgraph_sketch.so')

_SCALARS = {'int': c_int32, 'int32_t': c_int32, 'uint32_t': c_uint32, 'int64_t': c_int64, 'uint64_t': c_uint64,
            'size_t': c_size_t, 'float': c_float, 'double': c_double}
_POINTEES = (*_SCALARS, 'void', 'uint8_t', 'char')  # what a pointer may point to besides a struct
_INTEGER = re.compile(r'(\d+)u?|\((-\d+)\)|\((\d+)\s*<<\s*(\d+)\)')
_DECLARATOR = re.compile(r'(.+?[\s*])(\w+)(?:\[(\d+)\])?', re.S)  # `type name` or `type name[K]`
_PROTOTYPE = re.compile(r'(.+?[\s*])(\w+)\s*\(([^()]*)\)', re.S)
_STATEMENT = re.compile(r'\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;{}]+);)')


def _fail(header, why, text):
    raise ValueError(f'{header}: {why}: `{" ".join(text.split())}`')


def _ctype(spec, structs, returned=False):
    """the ctypes type of the type part of a declaration, such as `const uint32_t *const *`; None when it is outside the subset"""
    words = [w for w in re.findall(r'\w+|\S', spec) if w not in ('const', 'struct')]
    base, stars = (words or [''])[0], words[1:]
    if stars.count('*') != len(stars) or len(stars) > 2:
        return None
    if not stars:
        return _SCALARS.get(base)
    if base not in structs and base not in _POINTEES:
        return None
    if len(stars) == 2:
        return POINTER(c_void_p)
    if base in structs:
        return POINTER(structs[base])
    return c_char_p if returned and base == 'char' else c_void_p


def _declare(text, structs, header, whole, field=False):
    """(name, ctypes type) of one parameter or struct field"""
    m = _DECLARATOR.fullmatch(text.strip())
    ctype = _ctype(m[1], structs) if m else None
    if m and m[3]:
        ctype = c_void_p * int(m[3]) if field and ctype is c_void_p else None
    if ctype is None:
        _fail(header, f'cannot bind `{" ".join(text.split())}` of', whole)
    return m[2], ctype


def parse(headers):
    """(DEFINES, STRUCTS, SIGNATURES) of [(header name, header text), ...], read in that order"""
    defines, structs, signatures = {}, {}, {}
    for header, text in headers:
        text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
        for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SS_\w+)(.*)$', text, flags=re.M):
            m = _INTEGER.fullmatch(value.strip())
            if not m:
                _fail(header, 'not an integer define', f'#define {name}{value}')
            plain, negative, left, shift = m.groups()
            defines[name] = int(plain) if plain else int(negative) if negative else int(left) << int(shift)
        text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
        text, opened = re.subn(r'extern\s+"C"\s*\{', '', text)
        if opened:
            text = ''.join(text.rpartition('}')[::2])
        pos = 0
        while (m := _STATEMENT.match(text, pos)):
            pos, whole = m.end(), m[0]
            tag, body, alias, prototype = m.groups()
            if prototype is None:
                if tag != alias or tag in structs:
                    _fail(header, 'struct tag and typedef name must be one new name', whole)
                fields = [_declare(f, structs, header, whole, field=True) for f in body.split(';') if f.strip()]
                structs[tag] = type(tag, (ctypes.Structure,), {'_fields_': fields})
            else:
                p = _PROTOTYPE.fullmatch(prototype.strip())
                restype = _ctype(p[1], structs, returned=True) if p else None
                if restype is None:
                    _fail(header, 'cannot bind', whole)
                params = [] if p[3].strip() == 'void' else p[3].split(',')
                signatures[p[2]] = (restype, [_declare(a, structs, header, whole)[1] for a in params])
        if text[pos:].strip():
            _fail(header, 'text between declarations', text[pos:][:200])
    return defines, structs, signatures


def _read(header):
    with open(os.path.join(_INCLUDE, header)) as f:
        return f.read()


DEFINES, STRUCTS, SIGNATURES = parse([(h, _read(h)) for h in _HEADERS])

HllParams, CsrGraphStruct = STRUCTS['ss_hll_params'], STRUCTS['ss_csr_graph']  # (ss_csr_graph.reserved is the flags word: GRAPH_HOP_TABLES)
PprGraphStruct, StructureHeadStruct = STRUCTS['ss_ppr_graph'], STRUCTS['ss_structure_head']

SS_MAX_HOPS, SS_MAX_TABLE = DEFINES['SS_MAX_HOPS'], DEFINES['SS_MAX_TABLE']
SS_FLAG_USE_ZERO_ONE, SS_FLAG_FLOOR_SF = DEFINES['SS_FLAG_USE_ZERO_ONE'], DEFINES['SS_FLAG_FLOOR_SF']
SS_FLAG_MASK_TARGET = DEFINES['SS_FLAG_MASK_TARGET']  # ss_exact_pairs / ss_exact_large: balls of the graph without the link's own edge
SS_CSR_ERR_BOUNDS, SS_CSR_ERR_PROTOCOL = DEFINES['SS_CSR_ERR_BOUNDS'], DEFINES['SS_CSR_ERR_PROTOCOL']  # bits of a CSR build's err_flag
GRAPH_HOP_TABLES, MAX_MIRRORS = DEFINES['SS_GRAPH_HOP_TABLES'], DEFINES['SS_MAX_MIRRORS']
PPR_SEGMENT, PPR_MAX_COLUMNS = DEFINES['SS_PPR_SEGMENT'], DEFINES['SS_PPR_MAX_COLUMNS']
ABI_VERSION = 129  # ss_version() of the library the headers beside this package describe
(PROF_MINHASH_HOP, PROF_HLL_HOP, PROF_FIRST_HOP_MH, PROF_FIRST_HOP_HLL, PROF_PAIRS, PROF_CSR, PROF_HUB, PROF_FUSED,
 PROF_MINHASH_ROWS) = (DEFINES['SS_PROF_' + tag] for tag in ('MINHASH_HOP', 'HLL_HOP', 'FIRST_HOP_MH', 'FIRST_HOP_HLL', 'PAIRS', 'CSR',
                                                             'HUB', 'FUSED', 'MINHASH_ROWS'))
MEGA_SLICE, MEGA_SLOT_BYTES, MEGA_DESC_WORDS = DEFINES['SS_MEGA_SLICE'], DEFINES['SS_MEGA_SLOT_BYTES'], DEFINES['SS_MEGA_DESC_WORDS']
CSR_FINGERPRINT_BYTES = DEFINES['SS_CSR_FINGERPRINT_BYTES']
NEG_MODES = {'uniform': DEFINES['SS_NEG_UNIFORM'], 'same_source': DEFINES['SS_NEG_SAME_SOURCE'], 'wedge': DEFINES['SS_NEG_WEDGE']}
NEG_MAX_TRIES = DEFINES['SS_NEG_MAX_TRIES']
SUBGRAPH_LABELS = {'drnl': DEFINES['SS_SUBGRAPH_LABEL_DRNL'], 'de': DEFINES['SS_SUBGRAPH_LABEL_DE'],
                   'de+': DEFINES['SS_SUBGRAPH_LABEL_DE_PLUS']}  # the labels ss_subgraph_labels computes
SUBGRAPH_MAX_DIST = DEFINES['SS_SUBGRAPH_MAX_DIST']
COMPONENTS_CHUNK = DEFINES['SS_COMPONENTS_CHUNK']  # items per workgroup of the count / fill passes of ss_components_* / ss_induced_*
WEDGE_MAX_SLOTS, WEDGE_MAX_SLICES = DEFINES['SS_WEDGE_MAX_SLOTS'], 64  # (no define: the slices ss_wedge_emit takes at most)

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def lib():
    """load (once) and return the ctypes handle; raises NativeLibraryMissing if it was never built"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f'{LIB_PATH} not found: the HIP engine is not built. Run `python __graft_entry__.py` '
                f'(or subgraph-sketching_amd/csrc/build.sh). There is no CPU fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.ss_version() != ABI_VERSION:  # a stale in-tree build with another struct layout would corrupt launches
            raise NativeLibraryMissing(f'{LIB_PATH} is version {handle.ss_version()}, this package needs {ABI_VERSION}: '
                                       f'rebuild with `python __graft_entry__.py`')
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().ss_error_string(code).decode()
        raise RuntimeError(f'{what} failed: {msg} ({code})')
