"""Planted inputs for the kernels of csrc/ss_masked.hip (target-link masking), in numpy only: graph families in which the
masked edge is the ONLY path between its endpoints (K2, bridges, cycles), rows of planted length around every stride of the walks (comb),
the partner at every position of a scanned row (every_position), the sketch shapes at which the kernels take another path, and three
batch patterns (every edge / non-edge pattern of a classify wavefront, more than 2 x 4096 edge links so that a workgroup of
masked_pairs_kernel serves several links in turn, more than 131072 links so that the 16-lane scans take a second trip).

The geometry is restated from the kernel's comments: a sketch row is CM = P / 4 MinHash chunks and CH = M / 16 HLL chunks of 16 bytes,
W4 = CM + CH <= 256; S = 256 / W4 neighbours of a walk are in flight; the first hop runs S1 = 256 / P neighbour slots while P <= 256 and
one slot over permutations t, t + 256, ... beyond; dynamic LDS = (2 h W4 + 256) * 16 + 4 M bytes.  The launch constants are read from
the unit's text.  No test, no torch and no engine code lives here: tests/test_masked_planted_host.py checks the plans and the rule on
them, tests/test_masked_planted_gpu.py runs them."""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(REPO, 'subgraph-sketching_amd', 'csrc', 'ss_masked.hip')


def _constants():
    unit = open(UNIT).read()
    threads = int(re.search(r'constexpr int kMaskedThreads = (\d+);', unit).group(1))
    grid = int(re.search(r'constexpr int kMaskedGrid = (\d+);', unit).group(1))
    lo, hi = re.search(r'grid16 = \(unsigned\)\(\(B \+ groups - 1\) / groups < (\d+) \? \(B \+ groups - 1\) / groups : (\d+)\);', unit).groups()
    assert lo == hi, 'the 16-lane scans cap their grid at one number'
    assert re.search(r'const int groups = kMaskedThreads / kRow;', unit)
    return threads, grid, int(lo)


THREADS, PAIRS_GRID, SCAN_GRID = _constants()
ROW = 16                                  # kRow: the lanes of one link in the classify and row_zeros scans
WAVE = 64
SCAN_LINKS = SCAN_GRID * (THREADS // ROW)  # the links one trip of masked_classify_kernel / masked_row_zeros_kernel covers

SHAPES = [(4, 4), (8, 4), (192, 6), (128, 8), (512, 8), (960, 8), (128, 11), (512, 11)]
HOPS = (1, 2, 3)


def geometry(P, p):
    M = 1 << p
    CM, CH = P >> 2, M >> 4
    W4 = CM + CH
    return SimpleNamespace(P=P, p=p, M=M, CM=CM, CH=CH, W4=W4, S=THREADS // W4 if W4 <= THREADS else 0,
                           S1=THREADS // P if P <= THREADS else 1, supported=W4 <= THREADS)


def lds_bytes(P, p, h):
    g = geometry(P, p)
    return (2 * h * g.W4 + THREADS) * 16 + 4 * g.M


def shape_classes(P, p):
    """the names of the never-run paths (the issue's list) a sketch shape reaches"""
    g = geometry(P, p)
    out = set()
    if P > THREADS:
        out.add('first hop: one slot, permutations t, t + 256, ...')
        if P % THREADS:
            out.add('first hop: partial last trip')
    if P < THREADS and g.S1 == 1:
        out.add('first hop: S1 = 1 with threads whose slot >= S1')
    if g.S1 == THREADS // 4 and P == 4:
        out.add('first hop: S1 = 64')
    if g.W4 == THREADS:
        out.add('a row of exactly 256 chunks')
    if g.M > THREADS:
        out.add('more HLL registers than threads')
    if g.S == 1 and g.W4 < THREADS:
        out.add('S = 1 with idle threads')
    if g.W4 == 2:
        out.add('W4 = 2')
    if g.W4 == 3:
        out.add('W4 = 3: thread 255 inactive')
    return out


ALL_CLASSES = ('first hop: one slot, permutations t, t + 256, ...', 'first hop: partial last trip',
               'first hop: S1 = 1 with threads whose slot >= S1', 'first hop: S1 = 64', 'a row of exactly 256 chunks',
               'more HLL registers than threads', 'S = 1 with idle threads', 'W4 = 2', 'W4 = 3: thread 255 inactive')


# ---- graph families: each returns (n, edge_index [2, E] int64, links [L, 2] int64) --------------------------------------------------
def _und(pairs):
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([a, a[:, ::-1]])


def _graph(n, arcs, links):
    ei = np.ascontiguousarray(np.asarray(arcs, dtype=np.int64).reshape(-1, 2).T)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    assert ei.min() >= 0 and int(ei.max()) == n - 1, 'every family names its last node in an edge: n_self == n'
    assert links.min() >= 0 and links.max() < n
    return n, ei, links


def k2():
    return _graph(2, _und([(0, 1)]), [(0, 1), (1, 0)])


BRIDGE_SIZES = ((0, 0), (3, 3), (40, 300), (300, 300))
BRIDGE_VARIANTS = ('loop_u', 'loop_uv', 'copies', 'u_to_v', 'v_to_u')  # on (3, 3)


def bridge(nl, nr, variant='plain'):
    """u = 0 with nl leaves, v = 1 with nr leaves, five leaves a side with a private second-level leaf; u - v is the only connection"""
    u, v = 0, 1
    arcs, nxt = [], 2
    for x, k in ((u, nl), (v, nr)):
        leaves = np.arange(nxt, nxt + k)
        nxt += k
        arcs.append(_und([(x, y) for y in leaves]))
        second = np.arange(nxt, nxt + min(k, 5))
        nxt += len(second)
        arcs.append(_und(list(zip(leaves[:len(second)], second))))
    middle = {'plain': [(u, v), (v, u)], 'loop_u': [(u, v), (v, u), (u, u)], 'loop_uv': [(u, v), (v, u), (u, u), (v, v)],
              'copies': [(u, v)] * 3 + [(v, u)] * 2, 'u_to_v': [(u, v)], 'v_to_u': [(v, u)]}[variant]
    arcs.insert(1, np.asarray(middle, dtype=np.int64))  # the copies sit in the middle of the edge list, not at its end
    return _graph(nxt, np.concatenate(arcs), [(u, v), (v, u)])


CYCLES = (3, 4, 5, 6, 7)


def cycle(k):
    """the ring on k nodes; without the link the partner is k - 1 hops away: inside three hops for k <= 4, outside for k >= 5"""
    x = np.arange(k)
    return _graph(k, _und(np.stack([x, (x + 1) % k], axis=1)), [(0, 1), (1, 0), (k - 1, 0)])


COMB_DEGREES = (1, 2, 3, 4, 5, 6, 15, 16, 17, 84, 85, 86, 127, 128, 129, 255, 256, 257)  # around S = 4, 5, 85, 128, the 16 lanes, the 256 threads
COMB_TRIANGLES = (4, 16, 85)   # row lengths of the w that are neighbours of v too
COMB_LOOPS = (5, 128)          # row lengths of the w that carry an explicit self loop


def comb():
    """u = 0 - v = 1; u has one neighbour w per planted row length d: row w = {u} + d - 1 private leaves (triangles: {u, v} + d - 2
    leaves; loops: {u, w} + d - 2 leaves).  -> (n, edge_index, links) with comb.rows = {w: its row length}"""
    u, v = 0, 1
    arcs, nxt, rows, tri, loops = [_und([(u, v)])], 2, {}, [], []
    for kind, degrees in (('plain', COMB_DEGREES), ('triangle', COMB_TRIANGLES), ('loop', COMB_LOOPS)):
        for d in degrees:
            w = nxt
            own = 1 if kind == 'plain' else 2
            leaves = np.arange(w + 1, w + 1 + d - own)
            nxt = w + 1 + len(leaves)
            arcs.append(_und([(u, w)] + [(w, y) for y in leaves]))
            if kind == 'triangle':
                arcs.append(_und([(v, w)]))
                tri.append(w)
            if kind == 'loop':
                arcs.append(np.array([[w, w]], dtype=np.int64))
                loops.append(w)
            rows[w] = d
    by_len = {d: w for w, d in rows.items() if w not in tri and w not in loops}
    links = [(u, v), (v, u)] + [(u, by_len[d]) for d in (1, 5, 85, 257)] + [(by_len[256], u), (by_len[17], by_len[17] + 1)]
    links += [(v, tri[0]), (tri[2], u), (u, loops[0]), (loops[1], u)]
    n, ei, links = _graph(nxt, np.concatenate(arcs), links)
    counts = np.bincount(ei[1], minlength=n)
    assert all(int(counts[w]) == d for w, d in rows.items()), 'row w holds the planted number of in-neighbours'
    comb.rows, comb.triangles, comb.loops = rows, tuple(tri), tuple(loops)
    return n, ei, links


POSITION_L = (1, 15, 16, 17, 33, 300)
POSITION_VARIANTS = ('both', 'in', 'out')


def every_position(L, variant='both'):
    """a centre x = 0 with neighbours 1 .. L and the links (x, y), (y, x) for EVERY y: whatever order the builder leaves row x in, the
    partner sits at each of its positions once.  `in`: only y -> x exists (the hit is in row x alone); `out`: only x -> y (row x is
    empty, the hit sits in the one-entry row y)"""
    y = np.arange(1, L + 1)
    xy = np.stack([np.zeros(L, dtype=np.int64), y], axis=1)
    arcs = {'both': np.concatenate([xy, xy[:, ::-1]]), 'in': xy[:, ::-1], 'out': xy}[variant]
    return _graph(L + 1, arcs, np.concatenate([xy, xy[:, ::-1]]))


def forest(members):
    """the disjoint union of families [(name, (n, ei, links))] -> (n, edge_index, links, {name: slice of links}, {name: first node})"""
    arcs, links, where, first, base, count = [], [], {}, {}, 0, 0
    for name, (n, ei, lk) in members:
        arcs.append(ei + base)
        links.append(lk + base)
        where[name] = slice(count, count + len(lk))
        first[name] = base
        count += len(lk)
        base += n
    return base, np.ascontiguousarray(np.concatenate(arcs, axis=1)), np.concatenate(links), where, first


def rule_families():
    """every family of the plan by name (the rule is checked on each of them alone)"""
    out = [('K2', k2())]
    out += [(f'bridge({nl},{nr})', bridge(nl, nr)) for nl, nr in BRIDGE_SIZES]
    out += [(f'bridge(3,3,{variant})', bridge(3, 3, variant)) for variant in BRIDGE_VARIANTS]
    out += [(f'cycle({k})', cycle(k)) for k in CYCLES]
    out += [('comb', comb())]
    out += [(f'every_position({L},{variant})', every_position(L, variant)) for L in POSITION_L for variant in POSITION_VARIANTS]
    return out


def is_bridge(name):
    return name == 'K2' or name.startswith('bridge(')


@functools.lru_cache(maxsize=None)
def small_forest():
    """K2, the bridges and the cycles side by side: what test 1 of the GPU module runs at every shape and hop count"""
    return forest([m for m in rule_families() if is_bridge(m[0]) or m[0].startswith('cycle(')])


# ---- batch patterns ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_forest():
    """the graph of the three batch patterns -> (n, edge_index, distinct edge links [~40, 2], non-edges [.., 2]).  The distinct links
    differ in cost by three orders of magnitude: K2 (two one-entry rows) up to bridge (300, 300) and the comb's u (a 2-hop walk of some
    1 800 rows at h = 3).  The non-edges: pairs in two components, pairs two hops apart in one (both rows scanned to their end), u == v"""
    members = [m for m in rule_families() if m[0] in ('K2', 'bridge(3,3)', 'bridge(300,300)', 'bridge(3,3,copies)', 'bridge(3,3,loop_uv)',
                                                       'comb') or m[0].startswith('cycle(')]
    n, ei, links, where, off = forest(members)
    b, c = off['bridge(300,300)'], off['comb']
    non = [(b + 2, b + 3), (b, b + 400), (b + 2, c), (c, off['K2']), (c + 1, c + 1), (c + 1, c + 2), (off['cycle(7)'], off['cycle(7)'] + 3),
           (off['cycle(3)'], off['cycle(4)']), (c + 2, b + 1), (off['K2'] + 1, off['cycle(5)'] + 2)]
    have = set(map(tuple, ei.T.tolist()))
    assert all((u, v) not in have and (v, u) not in have for u, v in non)
    assert all((u, v) in have or (v, u) in have for u, v in links.tolist())
    assert 35 <= len(links) <= 45
    return n, ei, links, np.asarray(non, dtype=np.int64)


def _pick(distinct, non, is_edge, which):
    links = np.empty((len(which), 2), dtype=np.int64)
    links[is_edge] = distinct[which[is_edge]]
    links[~is_edge] = non[which[~is_edge]]
    return links


def _pattern_orders():
    """classify wavefronts (four links each) by their 4-bit edge pattern: all 16 patterns, then all-edge and no-edge wavefronts side by
    side in both orders, then the 16 patterns backwards"""
    return list(range(16)) + [15, 0, 15, 15, 0, 0] + list(range(15, -1, -1))


@functools.lru_cache(maxsize=None)
def wave_patterns(length):
    """-> (links [length, 2], is_edge bool [length], which distinct link / non-edge each is): link 4 g + i is an edge when bit i of the
    pattern of wavefront g is set; the edges and the non-edges are taken from batch_forest() in turn"""
    n, ei, distinct, non = batch_forest()
    orders = _pattern_orders()
    is_edge = np.array([(orders[(q // 4) % len(orders)] >> (q % 4)) & 1 for q in range(length)], dtype=bool)
    which = np.where(is_edge, np.cumsum(is_edge) % len(distinct), np.cumsum(~is_edge) % len(non))
    return _pick(distinct, non, is_edge, which), is_edge, which


WAVE_LENGTHS = (16 * 10 + 1, 16 * 10 + 15)
MANY_EDGES = 3 * PAIRS_GRID + 7
LONG_BATCH = SCAN_LINKS + 83


@functools.lru_cache(maxsize=None)
def many_edges():
    """-> (links [3 * 4096 + 7, 2], index into the distinct links): edge links only, drawn with a fixed seed"""
    n, ei, distinct, non = batch_forest()
    which = np.random.default_rng(41).integers(0, len(distinct), size=MANY_EDGES)
    return distinct[which], which


@functools.lru_cache(maxsize=None)
def long_batch():
    """-> (links [131072 + 83, 2], is_edge, which): one link in four an edge, edges planted at positions 131071, 131072, 131073 + 16 and
    the last, non-edges at 131073 and the last but one"""
    n, ei, distinct, non = batch_forest()
    rng = np.random.default_rng(43)
    is_edge = rng.random(LONG_BATCH) < 0.25
    for q, e in ((SCAN_LINKS - 1, True), (SCAN_LINKS, True), (SCAN_LINKS + 1, False), (SCAN_LINKS + 17, True), (LONG_BATCH - 2, False),
                 (LONG_BATCH - 1, True)):
        is_edge[q] = e
    which = np.where(is_edge, rng.integers(0, len(distinct), size=LONG_BATCH), rng.integers(0, len(non), size=LONG_BATCH))
    return _pick(distinct, non, is_edge, which), is_edge, which
