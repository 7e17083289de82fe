"""CSRs and id arrays planted on the branches of ss_csr_sort_rows (csrc/ss_csr_sort_rows.hip) and of sign.group_ids_stable built on
it, for tests/test_sort_rows_planted_host.py and tests/test_sort_rows_planted_gpu.py.  No test, no torch and no GPU code lives here,
and nothing is imported from the kernel: the helpers below RESTATE its contract.

The contract.  Rows are taken four at a time, rows 4 w .. 4 w + 3 by wavefront w of the short kernel.  Where all four hold at most 16
entries, each is sorted by 16 lanes ('lanes16').  Otherwise the whole wavefront sorts, one after the other, each row of 2 .. 64
entries ('wave'), passes by rows of 0 or 1 entries ('wave_skip') and lists rows above 64 for the long kernel.  That kernel (512
workgroups striding over the list) sorts a row of at most 16 384 entries in one LDS image ('lds'); a longer row ('merge') is sorted in
chunks of 16 384 and the runs merged pairwise, width doubling, ping-ponging between col and a scratch array -- 1 024 threads per merge,
each finding its stretch of the output by a merge-path search -- and copied back when the number of passes is odd.  A trailing run
without a partner is copied by the same code with an empty second run.

The base plan is a list of BLOCKS of four row lengths, every block starting at a row index that is a multiple of four, so a block IS
one wavefront.  VARIANTS drop or append rows so that the last wavefront holds 1, 2 or 3 rows, its last row once long and once short.
PATTERNS are the values of a row as a function of its length; every row of a plan uses the same one."""
import functools

import numpy as np

LANES16 = 16        # longest row of the four-rows-per-wavefront path
WAVE = 64           # longest row the short kernel sorts itself
LDS = 16384         # kSortRowLds: longest row (and every chunk) sorted in one LDS image
LONG_GRID = 512     # workgroups of the long launch
MERGE_THREADS = 1024
PAD = 0x7FFFFFFF    # what the kernels pad a row's image with: larger than or equal to any id

COMPOSITION = [[0, 0, 0, 0], [16, 16, 16, 16], [0, 1, 2, 16],          # the 16-lane path
               [15, 16, 17, 3], [64, 63, 1, 0], [31, 32, 33, 2],       # the whole-wave path
               [65, 2, 64, 0], [65, 66, 127, 1025]]                    # one listed row beside rows still to sort; all four listed
N_LISTED_BLOCKS = 150                                                  # x 4 rows of 65 .. 70 entries: more than LONG_GRID listed rows
LONG_LENGTHS = [128, 129, 1023, 1024, 1500, 16383, 16384, 16385, 20000, 32767, 32768, 32769, 49152, 49153, 65536, 65537, 131073]


def chunks(length):
    """LDS chunks of a row for the long kernel"""
    return -(-length // LDS)


def passes(length):
    """merge passes of a row: the run width doubles from LDS until it covers the row"""
    n, width = 0, LDS
    while width < length:
        n, width = n + 1, width * 2
    return n


def copies_back(length):
    """the sorted row ends in the scratch array (an odd number of passes) and is copied back"""
    return passes(length) % 2 == 1


def last_chunk(length):
    return length - (chunks(length) - 1) * LDS if length else 0


def merges(length):
    """[(pass, start, na, nb)] of every pairwise merge of a row, the partnerless trailing runs (nb == 0) included"""
    out, width, p = [], LDS, 0
    while width < length:
        for s0 in range(0, length, 2 * width):
            na = min(length - s0, width)
            out.append((p, s0, na, min(length - s0 - na, width)))
        width, p = width * 2, p + 1
    return out


def has_lone_run(length):
    return any(nb == 0 for _, _, _, nb in merges(length))


def wave_path(lengths):
    """the path of one wavefront's (up to four) rows"""
    return 'lanes16' if max(lengths, default=0) <= LANES16 else 'wave'


def row_path(length, wave_lengths):
    """the path of one row, given the lengths of the rows that share its wavefront (itself included)"""
    if wave_path(wave_lengths) == 'lanes16':
        return 'lanes16'
    if length > LDS:
        return 'merge'
    if length > WAVE:
        return 'lds'
    return 'wave' if length >= 2 else 'wave_skip'


def row_paths(lengths):
    """row_path of every row of a plan"""
    return [row_path(n, lengths[r - r % 4:r - r % 4 + 4]) for r, n in enumerate(lengths)]


def listed_rows(lengths):
    return sum(n > WAVE for n in lengths)


def workspace_bytes(E):
    """ss_csr_sort_workspace_bytes: a 256-byte counter line, the list of long rows (E / 64 + 2 words), E words of scratch"""
    return 0 if E < 0 else (E // WAVE + 2) * 4 + 256 + max(E, 1) * 4


@functools.lru_cache(maxsize=None)
def base_blocks():
    """[(kind, [four lengths])] of the base plan, kind in 'composition' / 'listed' / 'long'"""
    rng = np.random.RandomState(4)
    blocks = [('composition', list(b)) for b in COMPOSITION]
    blocks += [('listed', [int(x) for x in rng.randint(65, 71, size=4)]) for _ in range(N_LISTED_BLOCKS)]
    for k, n in enumerate(LONG_LENGTHS):  # the long row moves through the four places of its wavefront; the last block leads with it
        row = [int(x) for x in rng.randint(2, 17, size=3)]
        row.insert(0 if n == LONG_LENGTHS[-1] else k % 4, n)
        blocks.append(('long', row))
    return blocks


def base_lengths():
    return [n for _, b in base_blocks() for n in b]


# name: (rows dropped from the end, rows appended) -- the last block of the base plan is [131 073, short, short, short]
VARIANTS = {'n4': (0, []),
            'last1_long': (3, []), 'last1_short': (0, [7]),
            'last2_long': (0, [3, 129]), 'last2_short': (2, []),
            'last3_long': (0, [2, 16, 16385]), 'last3_short': (1, [])}


def lengths_of(variant):
    drop, extra = VARIANTS[variant]
    base = base_lengths()
    return base[:len(base) - drop] + list(extra)


# ---- values ------------------------------------------------------------------------------------------------------------------------
EIGHT = np.array([3, 5, 5 << 8, 77777, 1 << 20, (1 << 20) + 1, 1 << 30, 0x7FFFFFF0], dtype=np.int64)


def _values(pattern, n, rng):
    i = np.arange(n, dtype=np.int64)
    if pattern == 'distinct':
        stride = int(rng.randint(1, max((PAD - 1) // max(n, 1), 1) + 1))
        return rng.permutation(n).astype(np.int64) * stride + int(rng.randint(0, stride))
    if pattern == 'descending':
        return (n - 1 - i) * 7 + 5
    if pattern == 'ascending':
        return i * 3 + 1
    if pattern == 'equal':
        return np.full(n, 123456789, dtype=np.int64)
    if pattern == 'eight':
        return EIGHT[rng.randint(0, 8, size=n)]
    if pattern == 'sawtooth':  # period LDS: every full chunk holds the same multiset (each value three times), in the same order
        return (i % LDS) // 3
    if pattern == 'extremes':  # 0 and 0x7FFFFFFE (one below the pad), and random values between, all repeated
        pool = np.concatenate([[0, 0, PAD - 1, PAD - 1, 1, PAD - 2], rng.randint(0, PAD, size=10)])
        return pool[(i * 7 + rng.randint(0, 16)) % 16] if n < 4 else rng.permutation(np.resize(pool, n))
    raise ValueError(pattern)


PATTERNS = ('distinct', 'descending', 'ascending', 'equal', 'eight', 'sawtooth', 'extremes')
TIE_PATTERNS = ('equal', 'eight', 'sawtooth')


def csr_of(lengths, pattern, seed=0):
    """(rowptr int64 [N + 1], col int32 [E]) with the pattern in every row"""
    rng = np.random.RandomState(seed)
    rowptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lengths)
    col = np.concatenate([_values(pattern, n, rng) for n in lengths] + [np.zeros(0, dtype=np.int64)])
    assert col.min(initial=0) >= 0 and col.max(initial=0) < PAD
    return rowptr, col.astype(np.int32)


def sort_rows(rowptr, col):
    """THE REFERENCE: np.sort of every row"""
    out = col.copy()
    for lo, hi in zip(rowptr[:-1].tolist(), rowptr[1:].tolist()):
        out[lo:hi] = np.sort(col[lo:hi], kind='stable')
    return out


@functools.lru_cache(maxsize=None)
def planted(variant, pattern):
    """(rowptr, col, sorted col) of one plan; shared by the tests and never written to"""
    rowptr, col = csr_of(lengths_of(variant), pattern, seed=PATTERNS.index(pattern))
    want = sort_rows(rowptr, col)
    for a in (rowptr, col, want):
        a.setflags(write=False)
    return rowptr, col, want


# ---- the merge path, restated ------------------------------------------------------------------------------------------------------
def merge_path_split(A, B, d0, strict=False):
    """the number of A's entries among the first d0 outputs of merging A and B with A first on ties (strict: B first) -- the binary
    search along diagonal d0"""
    na, nb = len(A), len(B)
    lo, hi = max(d0 - nb, 0), min(d0, na)
    while lo < hi:
        i = (lo + hi) >> 1
        if (A[i] < B[d0 - i - 1]) if strict else (A[i] <= B[d0 - i - 1]):
            lo = i + 1
        else:
            hi = i
    return lo


def thread_boundaries(na, nb):
    """the diagonals at which the 1 024 threads of one merge begin (0 and the total left out)"""
    m = na + nb
    per = (m + MERGE_THREADS - 1) // MERGE_THREADS
    return [d for d in range(per, m, per)]


def merge_rows_restated(row, strict_search=False):
    """a row of more than LDS entries sorted as the long kernel sorts it: chunks, then merges in which every thread starts from its
    merge-path split and merges sequentially with A first on ties.  Returns (sorted row, [per merge with nb > 0: (nb, the number of
    thread boundaries that fall inside a run of equal values, the number of those whose value is present in both runs)])."""
    n = len(row)
    src = row.copy()
    for c0 in range(0, n, LDS):
        src[c0:c0 + LDS] = np.sort(src[c0:c0 + LDS])
    inside = []
    width = LDS
    while width < n:
        dst = np.empty_like(src)
        for s0 in range(0, n, 2 * width):
            A, B = src[s0:s0 + width], src[s0 + width:s0 + 2 * width]
            na, nb = len(A), len(B)
            bounds = [0] + thread_boundaries(na, nb) + [na + nb]
            hits = 0
            for d0, d1 in zip(bounds[:-1], bounds[1:]):
                i = merge_path_split(A, B, d0, strict=strict_search)
                j = d0 - i
                # the sequential merge from (i, j), A first on ties: of the next d1 - d0 outputs, those from A are the A[i + k] with
                # (number of B's entries from j on below A[i + k]) + k < d1 - d0
                a_tail, b_tail = A[i:i + d1 - d0], B[j:j + d1 - d0]
                pos_a = np.searchsorted(b_tail, a_tail, side='left') + np.arange(len(a_tail))
                pos_b = np.searchsorted(a_tail, b_tail, side='right') + np.arange(len(b_tail))
                out = np.empty(d1 - d0, dtype=src.dtype)
                out[pos_a[pos_a < d1 - d0]] = a_tail[pos_a < d1 - d0]
                out[pos_b[pos_b < d1 - d0]] = b_tail[pos_b < d1 - d0]
                dst[s0 + d0:s0 + d1] = out
            if nb:
                merged = dst[s0:s0 + na + nb]
                d = np.asarray(bounds[1:-1], dtype=np.int64)
                v = merged[d]
                in_a = A[np.minimum(np.searchsorted(A, v), na - 1)] == v
                in_b = B[np.minimum(np.searchsorted(B, v), nb - 1)] == v
                run = merged[d - 1] == v
                inside.append((nb, int(run.sum()), int((run & in_a & in_b).sum())))
        src, width = dst, width * 2
    return src, inside


# ---- id arrays for the grouping -----------------------------------------------------------------------------------------------------
def _ids_of_sizes(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)


@functools.lru_cache(maxsize=None)
def group_sizes(id_layout):
    """group size of every id: the base plan's blocks in ascending, reversed or shuffled order, a block of four empty ids after every
    third block"""
    blocks = [b for _, b in base_blocks()]
    if id_layout == 'reversed':
        blocks = blocks[::-1]
    elif id_layout == 'shuffled':
        blocks = [blocks[k] for k in np.random.RandomState(8).permutation(len(blocks))]
    elif id_layout != 'ascending':
        raise ValueError(id_layout)
    out = []
    for k, b in enumerate(blocks):
        out += b
        if k % 3 == 2:
            out += [0, 0, 0, 0]
    return tuple(out)


ID_LAYOUTS = ('ascending', 'reversed', 'shuffled')
ENTRY_LAYOUTS = ('shuffled', 'ascending', 'descending')
SINGLE_ID = (1, 65, 16385)
GROUPINGS = [f'{a}-{b}' for a in ID_LAYOUTS for b in ENTRY_LAYOUTS] + ['wrapped'] + [f'single-{e}' for e in SINGLE_ID]


@functools.lru_cache(maxsize=None)
def grouping(name):
    """(ids int64 [E], N): ids as given to group_ids_stable (negative ones wrap); shared and never written to"""
    if name.startswith('single-'):
        ids, n = np.zeros(int(name[7:]), dtype=np.int64), 1
        if len(ids) > 1:
            ids[1::2] = -1  # (-1 wraps to the one id there is)
    else:
        id_layout, entry_layout = ('shuffled', 'shuffled') if name == 'wrapped' else name.split('-')
        sizes = group_sizes(id_layout)
        ids, n = _ids_of_sizes(sizes), len(sizes)
        if entry_layout == 'shuffled':
            ids = ids[np.random.RandomState(9).permutation(len(ids))]
        elif entry_layout == 'descending':
            ids = ids[::-1].copy()
        if name == 'wrapped':
            ids = np.where(np.random.RandomState(10).randint(0, 2, size=len(ids)) == 1, ids - n, ids)
    ids.setflags(write=False)
    return ids, n


def grouping_reference(ids, n):
    """(rowptr, order) of the stable grouping: cumulative bincount and numpy's stable argsort of the wrapped ids"""
    wrapped = np.where(ids < 0, ids + n, ids)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(wrapped, minlength=n))
    return rowptr, np.argsort(wrapped, kind='stable')
