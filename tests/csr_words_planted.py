"""Edge lists and edits planted on the three small device words the CSR build leaves behind (csrc/ss_csr.hip), for
tests/test_csr_words_planted_host.py and tests/test_csr_words_planted_gpu.py.  No test, no torch and no GPU code lives here.

The words.  FingerprintWords.skip: fingerprint_kernel (kFpBlocks x FP_THREADS threads) adds up two sums of a mix of every (src, dst)
and fingerprint_decide_kernel compares them with the stored ones; 1 lets every kernel of the build exit.  csr.symmetric: every
kTile-edge tile of tile_sort_kernel (kSortThreads threads, thread i takes the offsets i + k kSortThreads of its tile, or -- full tiles
of 16-byte aligned rows -- the 16-byte pairs i + k kSortThreads, two edges each) sums S_0 / S_1 and a bad-id flag; the last bucket's
workgroup of finish_runs_kernel (kRunThreads threads striding over the tiles) adds the tiles up.  csr.n_self_dev: max(id) + 1, per
tile and then by the same workgroup.

All three are reductions over the whole edge list, so what is planted here is WHERE an edit sits: in which tile, at which offset of
the tile, in which loop of the fingerprint kernel and in which of the three ways the two rows of the list can lie in memory.  The
constants the positions follow from are read out of the sources (constants()); the positions move when a constant moves.

A list is a numpy int64 [2, E].  An edit is described by the columns it overwrites, `name_columns(ei, k, ...) -> [(position, src,
dst)]`, so that a test can make it on the device on one or two columns of a list that is already there; `apply(ei, columns)` and
EDITS[name] give the edited list in numpy."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'subgraph-sketching_amd', 'csrc')

Constants = namedtuple('Constants', 'tile max_keys sort_threads run_threads fp_blocks fp_threads wave')


@functools.lru_cache(maxsize=None)
def constants():
    csr = open(os.path.join(CSRC, 'ss_csr.hip')).read()
    common = open(os.path.join(CSRC, 'ss_common.hpp')).read()

    def const(text, name):
        return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))

    # the fingerprint kernel's workgroup size has no name: it is the second dimension of its one launch
    fp_threads = int(re.search(r'hipLaunchKernelGGL\(fingerprint_kernel, dim3\(kFpBlocks\), dim3\((\d+)\)', csr).group(1))
    return Constants(tile=const(csr, 'kTile'), max_keys=const(csr, 'kMaxKeys'), sort_threads=const(csr, 'kSortThreads'),
                     run_threads=const(csr, 'kRunThreads'), fp_blocks=const(csr, 'kFpBlocks'), fp_threads=fp_threads,
                     wave=const(common, 'kWave'))


# ---- base graphs ------------------------------------------------------------------------------------------------------------------
Base = namedtuple('Base', 'name ei n')


def _symmetric(n, num_edges, seed):
    """undirected random edges over the ids below n - 1 stored in both directions, e | reversed e: no self edge anywhere, the largest
    id is n - 2 (so that `max_id` has room), position j and j + E / 2 hold the two directions of one edge"""
    assert num_edges % 2 == 0
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n - 1, size=(2, num_edges // 2)).astype(np.int64)
    loops = e[0] == e[1]
    e[1, loops] = (e[0, loops] + 1 + rng.randint(0, n - 2, size=int(loops.sum()))) % (n - 1)
    e[0, 7] = n - 2          # (position 7 is no planted offset)
    e[1, 7] = 3
    return np.ascontiguousarray(np.concatenate([e, e[::-1]], axis=1))


@functools.lru_cache(maxsize=None)
def base(name):
    C = constants()
    if name == 'small':        # one-level plan, packed records: three full tiles and a partial one
        return Base(name, _symmetric(5000, 3 * C.tile + 1000, 101), 5000)
    if name == 'reducer':      # one tile more than the reducer workgroup has threads, plus a partial tile of two edges
        return Base(name, _symmetric(5000, (C.run_threads + 1) * C.tile + 2, 102), 5000)
    if name == 'two_level':    # more than kMaxKeys buckets of 1024 nodes
        return Base(name, _symmetric(300000, 40 * C.tile + 6, 103), 300000)
    if name.endswith('_odd'):  # the same edges and one self edge at position 5 (no planted offset): E is odd, the multiset symmetric
        b = base(name[:-4])
        return Base(name, np.ascontiguousarray(np.insert(b.ei, 5, (11, 11), axis=1)), b.n)
    raise KeyError(name)


BASES = ('small', 'reducer', 'two_level')


def levels(n):
    """restatement of make_plan's first decision: one level while the buckets of 1024 nodes are at most kMaxKeys"""
    return 1 if (n + 1023) // 1024 <= constants().max_keys else 2


# ---- how the two rows lie in memory -------------------------------------------------------------------------------------------------
# build_csr keeps ei[0] / ei[1] as views, so the rows' addresses are those of the tensor handed over.  A form is (row pitch in
# elements, first column) of a [2, pitch] int64 buffer whose own address is 16-byte aligned; the list is buffer[:, first:first + E].
FORMS = ('aligned', 'dst_off', 'src_off')


def form_layout(form, E):
    """-> (pitch, first): aligned -- both rows on 16 bytes (even pitch; E itself where it is even); dst_off -- src on 16 bytes, dst 8
    off (odd pitch; an odd E gives the contiguous [2, E]); src_off -- column 1 onwards of an odd-pitch buffer: src 8 off, dst on 16"""
    if form == 'aligned':
        return E + E % 2, 0
    if form == 'dst_off':
        return E + 1 - E % 2, 0
    if form == 'src_off':
        return E + 1 + E % 2, 1
    raise KeyError(form)


def form_view(buffer, form, E):
    """the [2, E] list inside a [2, pitch] buffer (a numpy array or a tensor) of form_layout(form, E)"""
    pitch, first = form_layout(form, E)
    assert tuple(buffer.shape) == (2, pitch)
    return buffer[:, first:first + E]


def form_offsets(form):
    """(address of src, address of dst) modulo 16 the form claims"""
    return {'aligned': (0, 0), 'dst_off': (0, 8), 'src_off': (8, 0)}[form]


def rows_aligned(form):
    return form == 'aligned'


# ---- positions: tile classes and offsets -----------------------------------------------------------------------------------------
# both halves of a 16-byte pair, the wavefront boundary in both load forms (64 edges / 64 pairs), the seams between a thread's loads.
# 3071 / 3072 are there for the slots: without them no offset falls into slot 5 of either form or slot 6 of the scalar one
# (test_csr_words_planted_host asserts that all 8 slots are reached in both forms)
OFFSETS = (0, 1, 63, 64, 127, 128, 511, 512, 1023, 1024, 2047, 2048, 3071, 3072, 4094, 4095)


def tile_classes(E):
    """{name: tile}: 0, 1, one in the middle, run_threads - 1 and run_threads (lists that long: the second iteration of the reducer's
    strided loop), the last full tile and the partial tile"""
    C = constants()
    full, part = divmod(E, C.tile)
    out = {}
    if full > 0:
        out['first'] = 0
    if full > 1:
        out['second'] = 1
    if full > 3:             # (with three full tiles the middle one is the second)
        out['middle'] = full // 2
    if full > C.run_threads:
        out['reducer_last_thread'] = C.run_threads - 1
        out['reducer_second_pass'] = C.run_threads
    if full > 0 and full - 1 not in out.values():   # (`reducer`: its last full tile IS the reducer's second pass)
        out['last_full'] = full - 1
    if part:
        out['partial'] = full
    return out


def offsets_of(E, tile):
    """planted offsets inside a tile: OFFSETS in a full one (its last two are kTile - 2 and kTile - 1), first / second / last edge of the partial one"""
    C = constants()
    count = min(C.tile, E - tile * C.tile)
    if count == C.tile:
        return tuple(o for o in OFFSETS if o < C.tile - 2) + (C.tile - 2, C.tile - 1)
    return tuple(sorted({0, min(1, count - 1), count - 1}))


def positions(E, offsets=None):
    """[(tile class, tile, offset, edge index)] of every planted position of a list of E edges (offsets: only these, where a tile has them)"""
    C = constants()
    out = []
    for cls, tile in tile_classes(E).items():
        for off in offsets_of(E, tile):
            full = min(C.tile, E - tile * C.tile) == C.tile
            if offsets is None or not full or off in offsets:
                out.append((cls, tile, off, tile * C.tile + off))
    return out


def sort_slot(E, aligned, e):
    """(tile, thread, slot 0 .. 7, vectorised) of edge e in tile_sort_kernel: full tiles of aligned rows are read as 16-byte pairs, pair
    p of the tile by thread p % kSortThreads in its load p // kSortThreads (slots 2 k and 2 k + 1); everything else edge by edge"""
    C = constants()
    tile, off = divmod(e, C.tile)
    vec = aligned and min(C.tile, E - tile * C.tile) == C.tile
    if vec:
        pair, half = divmod(off, 2)
        return tile, pair % C.sort_threads, 2 * (pair // C.sort_threads) + half, True
    return tile, off % C.sort_threads, off // C.sort_threads, False


# ---- positions: the loops of fingerprint_kernel -----------------------------------------------------------------------------------
LOAD0, LOAD1, ONE_LOAD, TAIL, SCALAR = 'two_load_first', 'two_load_second', 'one_load', 'scalar_tail', 'all_scalar'


def fp_loop_of(E, aligned, e):
    """the loop of fingerprint_kernel that reads edge e, by walking the loops of the one thread that can reach it as they are written:
        pairs = aligned ? E / 2 : 0;  stride = gridDim.x * blockDim.x;  q = global thread id
        for (; q + stride < pairs; q += 2 * stride)  loads pairs q (LOAD0) and q + stride (LOAD1)
        for (; q < pairs; q += stride)               loads pair q (ONE_LOAD)
        for (e = 2 * pairs + id; e < E; e += stride) loads edge e (TAIL; SCALAR where pairs == 0)
    -> (loop, 'x' / 'y' half of the pair or None)"""
    C = constants()
    stride = C.fp_blocks * C.fp_threads
    pairs = E // 2 if aligned else 0
    assert 0 <= e < E
    if e >= 2 * pairs:
        return (TAIL if pairs else SCALAR), None
    p, half = e // 2, 'xy'[e % 2]
    q = p % stride
    while q + stride < pairs:
        if p == q:
            return LOAD0, half
        if p == q + stride:
            return LOAD1, half
        q += 2 * stride
    while q < pairs:
        if p == q:
            return ONE_LOAD, half
        q += stride
    raise AssertionError('no loop reads this pair')


def fp_positions(E, aligned):
    """{(loop, which, half): edge index}: both halves of the first and the last pair each loop of fingerprint_kernel reads, from its
    bounds: thread g owns the pairs g, g + stride, ... below `pairs`, m_g of them; the two-load loop runs while two are left, so it
    takes the first 2 (m_g / 2) of them alternately as first and second load, and the one-load loop the odd one out.  Where the rows
    are not aligned every edge is read by the scalar loop: its first two edges, the two around the grid's stride and the last."""
    C = constants()
    stride = C.fp_blocks * C.fp_threads
    pairs = E // 2 if aligned else 0
    out = {}
    if pairs:
        p = np.arange(pairs, dtype=np.int64)
        row, g = p // stride, p % stride
        m = (pairs - g + stride - 1) // stride
        two = row < 2 * (m // 2)
        for loop, mask in ((LOAD0, two & (row % 2 == 0)), (LOAD1, two & (row % 2 == 1)), (ONE_LOAD, ~two)):
            idx = np.flatnonzero(mask)
            if len(idx):
                for which, q in (('first', int(idx[0])), ('last', int(idx[-1]))):
                    out[(loop, which, 'x')], out[(loop, which, 'y')] = 2 * q, 2 * q + 1
        if E > 2 * pairs:
            out[(TAIL, 'only', None)] = E - 1
    else:
        for which, e in (('first', 0), ('second', 1), ('stride_end', stride - 1), ('stride_again', stride), ('last', E - 1)):
            if 0 <= e < E:
                out[(SCALAR, which, None)] = e
    return out


# ---- edits ------------------------------------------------------------------------------------------------------------------------
def apply(ei, columns):
    out = np.array(ei, dtype=np.int64, copy=True)
    for pos, s, d in columns:
        out[0, pos], out[1, pos] = s, d
    return out


def neighbours(ei, u):
    return set(ei[1][ei[0] == u].tolist()) | set(ei[0][ei[1] == u].tolist())


def to_self_columns(ei, k):
    """(u, v) becomes (u, u): its reverse stands alone"""
    u, v = int(ei[0, k]), int(ei[1, k])
    assert u != v
    return [(k, u, u)]


def retarget_columns(ei, k):
    """(u, v) becomes (u, w), w the smallest id that is neither u nor a neighbour of u"""
    u, v = int(ei[0, k]), int(ei[1, k])
    taken = neighbours(ei, u) | {u}
    w = next(i for i in range(int(ei.max()) + 1) if i not in taken)
    return [(k, u, w)]


def reverse_position(ei, k):
    """position of one copy of the reverse of edge k"""
    u, v = int(ei[0, k]), int(ei[1, k])
    return int(np.flatnonzero((ei[0] == v) & (ei[1] == u))[0])


def swap_with_reverse_columns(ei, k):
    """the columns at k and at one copy of the reverse exchange places: the same multiset in another order"""
    j = reverse_position(ei, k)
    assert j != k
    return [(k, int(ei[0, j]), int(ei[1, j])), (j, int(ei[0, k]), int(ei[1, k]))]


def swap_partner(ei, k, candidates):
    """the first of `candidates` in another tile than k whose edge (s', d') can trade destinations with (s, d) at k so that the list
    changes and stops being symmetric: four distinct ids, d' no neighbour of s"""
    C = constants()
    s, d = int(ei[0, k]), int(ei[1, k])
    near = neighbours(ei, s)
    for j in candidates:
        s2, d2 = int(ei[0, j]), int(ei[1, j])
        if j // C.tile != k // C.tile and len({s, d, s2, d2}) == 4 and d2 not in near:
            return j
    raise AssertionError('no partner for the destination swap')


def swap_dsts_columns(ei, k, j):
    """(s, d), (s', d') become (s, d'), (s', d): every per-row and per-column statistic is kept"""
    return [(k, int(ei[0, k]), int(ei[1, j])), (j, int(ei[0, j]), int(ei[1, k]))]


def reverse_one_columns(ei, k):
    u, v = int(ei[0, k]), int(ei[1, k])
    assert u != v
    return [(k, v, u)]


def with_duplicate_columns(ei, k, i):
    """column k becomes a second copy of edge X = column i: the list duplicate_shift starts from"""
    return [(k, int(ei[0, i]), int(ei[1, i]))]


def duplicate_shift_columns(ei, k, j):
    """column k, one of two copies of X, becomes a second copy of Y = column j"""
    return [(k, int(ei[0, j]), int(ei[1, j]))]


def max_id_columns(ei, k, n, row):
    """one endpoint (row 0: the source, row 1: the destination) of edge k becomes n - 1, the one occurrence of that id"""
    assert int(ei.max()) == n - 2
    u, v = int(ei[0, k]), int(ei[1, k])
    return [(k, n - 1, v)] if row == 0 else [(k, u, n - 1)]


def bad_id_columns(ei, k, n, row):
    """one endpoint of edge k becomes n, the first id out of range"""
    u, v = int(ei[0, k]), int(ei[1, k])
    return [(k, n, v)] if row == 0 else [(k, u, n)]


def kept_edges(ei, n):
    """what the build documents for ids out of range (tile_sort_kernel): an edge whose destination is out of range is dropped, a
    source out of range is stored as source 0"""
    ei = np.asarray(ei, dtype=np.int64)
    keep = (ei[1] >= 0) & (ei[1] < n)
    src = np.where((ei[0] < 0) | (ei[0] >= n), 0, ei[0])
    return np.stack([src[keep], ei[1][keep]])


def n_self(ei):
    return int(np.asarray(ei).max()) + 1


EDITS = {
    'to_self': lambda ei, k: apply(ei, to_self_columns(ei, k)),
    'retarget': lambda ei, k: apply(ei, retarget_columns(ei, k)),
    'swap_with_reverse': lambda ei, k: apply(ei, swap_with_reverse_columns(ei, k)),
    'reverse_one': lambda ei, k: apply(ei, reverse_one_columns(ei, k)),
}


@functools.lru_cache(maxsize=None)
def directed_cycle():
    """`small` and the arcs a -> b -> c -> a between three nodes no edge joins, one arc in each of the first three tiles: in- and
    out-degree agree at every node, the multiset is not symmetric.  -> (Base, positions of the arcs)"""
    C = constants()
    b = base('small')
    a = 100
    bb = next(i for i in range(a + 1, b.n - 1) if i not in neighbours(b.ei, a))
    c = next(i for i in range(bb + 1, b.n - 1) if i not in neighbours(b.ei, a) and i not in neighbours(b.ei, bb))
    arcs = np.array([[a, bb, c], [bb, c, a]], dtype=np.int64)
    at = np.array([100, C.tile + 100, 2 * C.tile + 100])
    ei = np.ascontiguousarray(np.insert(b.ei, at, arcs, axis=1))
    return Base('directed_cycle', ei, b.n), tuple(int(x) for x in at + np.arange(3))


def hub_base(in_degree):
    """`small` and a star: node 9 receives `in_degree` more edges from the ids 1000 .., each stored in both directions"""
    b = base('small')
    leaves = np.arange(1000, 1000 + in_degree, dtype=np.int64)
    und = np.stack([leaves, np.full(in_degree, 9, dtype=np.int64)])
    return Base('hub', np.ascontiguousarray(np.concatenate([b.ei, und, und[::-1]], axis=1)), b.n)


def degenerate(E, where):
    """E edges over 64 ids: one edge 40 -> 41 whose reverse is missing, first or last in the list, beside E - 1 edges that form a
    symmetric multiset (random pairs in both directions, and the self edge 5 -> 5 where E - 1 is odd).  -> (ei, n, position)"""
    n = 64
    rng = np.random.RandomState(200 + E)
    rest = E - 1
    e = rng.randint(0, 32, size=(2, rest // 2)).astype(np.int64)
    parts = [e, e[::-1]] + ([np.array([[5], [5]], dtype=np.int64)] if rest % 2 else [])
    lone = np.array([[40], [41]], dtype=np.int64)
    parts = [lone] + parts if where == 'first' else parts + [lone]
    ei = np.ascontiguousarray(np.concatenate(parts, axis=1))
    assert ei.shape[1] == E
    return ei, n, 0 if where == 'first' else E - 1


def degenerate_sizes():
    """1, 2, 3 edges and one tile less one, exactly, and plus one"""
    tile = constants().tile
    return (1, 2, 3, tile - 1, tile, tile + 1)
