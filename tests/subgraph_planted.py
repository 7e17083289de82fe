"""Planted inputs for the two kernels of csrc/ss_subgraph.hip, as the plain arrays ss_subgraph_adj and ss_subgraph_labels take -- hand-made
node rows over hand-made graphs and hand-made local adjacencies, not BFS balls, so that runs, steps, depths and widths sit exactly where
the kernels branch.  No engine code: numpy only.  Every case carries the properties it claims as data (`claims`);
tests/test_subgraph_planted_host.py asserts them and pins the restatements, tests/test_subgraph_planted_gpu.py runs the kernels.

The contracts kept: id rows ascending, distinct, with u and v; CSR rows (in-arcs by target) sorted with duplicates adjacent; nbr entries
local indices < n.  The one exception is adj_switch_probe(), whose boundary rows DESCEND: inside the contract both walks of
ss_subgraph_adj give the same row by design, so which side of `deg > switch * n` a node took cannot be seen; on a strictly descending
row of distinct sources the arcs walk still finds every listed source and the id-row walk finds none (see there).

GROUP = 16 lanes walk one listed node; ADJ_SWEEP = kSubAdjGrid * 16 listed nodes per sweep of the adjacency grid; LABEL_GRID workgroups
label the links, each its rows q, q + LABEL_GRID, ...; LDS_NODES is the hardware limit of the on-chip label tier."""
import numpy as np

GROUP = 16
ADJ_SWEEP = 256 * 32 * 16
LABEL_GRID = 256 * 6
LDS_NODES = 2048
DEFAULT_SWITCH = 4
MAX_DIST_TOP = 1 << 20
KINDS = ('chip', 'workspace', 'empty', 'one_root')


def _ro(a):
    a.setflags(write=False)
    return a


def in_arc_csr(num_nodes, edge_index):
    """(csr_rowptr int64 [N + 1], csr_col int32 [E]): the sources of the arcs into x at col[rowptr[x] : rowptr[x + 1]], ascending"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    order = np.lexsort((ei[0], ei[1]))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=num_nodes))]).astype(np.int64)
    return rowptr, ei[0][order].astype(np.int32)


class AdjCase(object):
    """name, N, ei int64 [2, E], links int64 [B, 2], rowptr int64 [B + 1], ids int64 [T], claims {}; csr() -> the sorted in-arc CSR"""

    def __init__(self, name, N, ei, links, rowptr, ids, **claims):
        self.name, self.N = name, int(N)
        self.ei = _ro(np.asarray(ei, dtype=np.int64).reshape(2, -1))
        self.links = _ro(np.asarray(links, dtype=np.int64).reshape(-1, 2))
        self.rowptr, self.ids = _ro(np.asarray(rowptr, dtype=np.int64)), _ro(np.asarray(ids, dtype=np.int64))
        self.claims = claims
        self._csr = None

    @property
    def T(self):
        return int(self.ids.size)

    def csr(self):
        if self._csr is None:
            self._csr = in_arc_csr(self.N, self.ei)
        return self._csr

    def in_row(self, x):
        """the sorted sources of the arcs into x"""
        rowptr, col = self.csr()
        return col[rowptr[x]:rowptr[x + 1]]


def _arcs(into):
    """{target: [sources, copies included]} -> edge_index, in an order that is not the CSR's"""
    src = np.concatenate([np.asarray(s, dtype=np.int64) for s in into.values()] + [np.zeros((0,), dtype=np.int64)])
    dst = np.concatenate([np.full((len(s),), x, dtype=np.int64) for x, s in into.items()] + [np.zeros((0,), dtype=np.int64)])
    order = np.random.default_rng(len(src)).permutation(len(src))
    return np.stack([src[order], dst[order]])


def _rows(rows):
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])


# ---- adjacency: runs -----------------------------------------------------------------------------------------------------------------------
def adj_runs():
    """listed node x = 50 with 95 in-arcs laid out position by position (claims['layout']: source, first position, copies, listed?):
    a run on positions 15 .. 18 (lane 15, then lanes 0 .. 2 of the next step: lane 0 must not start it again), self loops on 31 .. 33,
    the partner 60 three times, a run of 40 from position 48 (positions 64 .. 79 are one whole step inside it), a listed run that ends
    at deg, unlisted sources between the others and below the smallest id; the partner's own row ends with a source above the largest
    id.  Links (50, 60), (60, 50) and (50, 50) over the same id row"""
    x, v = 50, 60
    row = [20, 30, 40, 50, 60, 70, 80, 90, 100]
    layout = [(5, 3, False), (20, 12, True), (30, 4, True), (35, 6, False), (40, 6, True), (50, 3, False), (55, 3, False), (60, 3, True),
              (70, 8, True), (80, 40, True), (90, 3, True), (100, 4, True)]
    into = {x: [s for s, copies, _ in layout for _ in range(copies)],
            v: [5, 50, 50, 50, 70, 150, 150],
            20: [30, 30, 20, 100, 101], 30: [20], 100: [19, 20, 90, 100, 100, 150], 70: [60, 60, 50, 80], 90: []}
    first, at = {}, 0
    for s, copies, listed in layout:
        first[s] = (at, copies, listed)
        at += copies
    rowptr, ids = _rows([row, row, row])
    return AdjCase('runs', 200, _arcs(into), [[x, v], [v, x], [x, x]], rowptr, ids, x=x, v=v, deg=at, layout=first)


# ---- adjacency: steps ----------------------------------------------------------------------------------------------------------------------
# target -> (deg, listed sources found in each step of 16 positions, the row as segments: k sources Below every id, Listed, unlisted
# beTween the listed ones, Above every id)
STEP_TARGETS = {200: (0, [], ''), 201: (1, [1], 'L1'), 202: (15, [15], 'L15'), 203: (16, [16], 'L16'), 204: (17, [16, 1], 'L17'),
                205: (31, [0, 15], 'B16 L15'), 206: (32, [1, 16], 'B15 L17'), 207: (33, [16, 16, 1], 'L33'), 208: (48, [16, 0, 16], 'L16 T16 L16'),
                209: (48, [1, 16, 0], 'B15 L17 A16')}


def adj_steps():
    """one link whose row lists the 48 even ids 100 .. 194 and the targets 200 .. 209 of STEP_TARGETS; every source once, ascending.
    deg 17 and 32: step 2 is placed after step 1's total of 16 / 1; deg 33: the third step after 32; deg 48: a step without a find
    between two full ones, and after them"""
    pools = {'B': list(range(0, 100)), 'L': list(range(100, 196, 2)), 'T': list(range(101, 196, 2)), 'A': list(range(300, 400))}
    into = {}
    for x, (deg, _, segments) in STEP_TARGETS.items():
        sources = []
        for seg in segments.split():
            sources += [j for j in pools[seg[0]] if not sources or j > sources[-1]][:int(seg[1:])]
        assert len(sources) == deg
        into[x] = sources
    row = pools['L'] + sorted(STEP_TARGETS)
    rowptr, ids = _rows([row])
    return AdjCase('steps', 1000, _arcs(into), [[204, 207]], rowptr, ids, targets=STEP_TARGETS)


# ---- adjacency: the switch -----------------------------------------------------------------------------------------------------------------
SWITCH_RATIOS = (1, DEFAULT_SWITCH)
SWITCH_ROWS = (1, 2, 15, 16, 17, 33)


def _switch_sources(row, x, deg, lo, hi, distinct):
    """deg sources of arcs into x: listed ones of row[lo:hi] (x left out) in 2 and 5 copies (distinct: one), then unlisted ones inside
    the same span of ids; ascending"""
    out = []
    for k, j in enumerate(j for j in row[lo:hi] if j != x):
        copies = 1 if distinct else (2, 5)[k % 2]
        if len(out) + copies <= deg:
            out += [j] * copies
    base = row[lo] if hi > lo else row[0]
    filler = [j for j in range(base + 1, base + 10 * len(row) + 400) if j % 10 != 0]
    out += filler[:deg - len(out)]
    assert len(out) == deg
    return sorted(out)


def _switch(name, distinct):
    blocks, rows, links, into, N = [], [], [], {}, 0
    for s in SWITCH_RATIOS:
        for n in SWITCH_ROWS:
            base = N + 1000
            N = base + 1000
            row = [base + 10 * k for k in range(n)]
            # the node of deg == s * n (the arcs walk at ratio s) and the one of deg == s * n + 1 (the id-row walk), each with its row:
            # the two middle ids of one row, the link between them; n == 1: a row (x, x) each
            nodes = [(row[0], row), (row[0] + 500, [row[0] + 500])] if n == 1 else [(row[n // 2 - 1], row), (row[n // 2], row)]
            lo, hi = (2, n - 2) if n >= 15 else (0, n)  # n >= 15: two ids below every source and two above every source
            for r, (x, own) in enumerate(nodes):
                deg = s * n + r
                into[x] = _switch_sources(own, x, deg, lo, hi, distinct)
                if n == 1 or r == 0:
                    rows.append(own)
                    links.append([x, x] if n == 1 else [nodes[0][0], nodes[1][0]])
                blocks.append(dict(ratio=s, n=n, x=x, deg=deg, by_ids=r == 1, link=len(links) - 1, outer=n >= 15))
    rowptr, ids = _rows(rows)
    return AdjCase(name, N, _arcs(into), links, rowptr, ids, blocks=blocks)


def adj_switch():
    """for switch_ratio s in (1, 4) and rows of n in (1, 2, 15, 16, 17, 33) ids: a listed node of deg == s * n and one of deg == s * n + 1
    (n == 1: a row each), listed sources in 2 and 5 copies, for n >= 15 two ids below and two above every source.  claims['blocks']"""
    return _switch('switch', False)


def adj_switch_probe():
    """the rows of adj_switch with DISTINCT sources (n >= 2); descending_csr() reverses the CSR rows of the boundary nodes.  On a strictly
    descending row of deg >= 2 distinct sources the arcs walk (which only asks that equal sources be adjacent) still finds every listed
    source; the id-row walk's lower bound ends at 0 (the key's position p >= deg / 2: every probe lands at or before p) or at deg
    (p < deg / 2: the first probe is beyond p, and so is every later one), and col[0] == key needs p == 0 >= deg / 2: it finds none.
    So the count pass tells the side a node took.  Outside the kernel's contract, in bounds all the same; count pass only"""
    case = _switch('switch_probe', True)
    case.claims['blocks'] = [b for b in case.claims['blocks'] if b['n'] >= 2]
    return case


def descending_csr(case):
    rowptr, col = case.csr()
    col = col.copy()
    for b in case.claims['blocks']:
        a, e = rowptr[b['x']], rowptr[b['x'] + 1]
        col[a:e] = col[a:e][::-1]
    return rowptr, col


# ---- adjacency: empty rows and the sweep ---------------------------------------------------------------------------------------------------
def _random_graph(rng, n, arcs, copies=0, loops=0):
    """a symmetric random multigraph: `arcs` undirected pairs, `copies` of them repeated, `loops` self loops"""
    a, b = rng.integers(0, n, size=arcs), rng.integers(0, n, size=arcs)
    again = rng.integers(0, arcs, size=copies)
    a, b = np.concatenate([a, a[again]]), np.concatenate([b, b[again]])
    loop = rng.integers(0, n, size=loops)
    return np.stack([np.concatenate([a, b, loop]), np.concatenate([b, a, loop])]).astype(np.int64)


def _random_rows(rng, n, links, sizes):
    rows = []
    for (u, v), size in zip(links, sizes):
        if size == 0:
            rows.append([])
            continue
        rest = rng.permutation(n)
        rest = rest[(rest != u) & (rest != v)][:size - len({int(u), int(v)})]
        rows.append(np.sort(np.concatenate([rest, np.unique([u, v])])))
    return rows


def adj_empty_rows():
    """B = 9 links over a 60-node multigraph: rows 0, 3, 4 and 8 are empty; row 2 lists one isolated node (u == v), row 6 one node with
    a self loop and arcs from unlisted nodes; T = 22"""
    rng = np.random.default_rng(9)
    n = 60
    ei = _random_graph(rng, n - 1, 150, copies=30, loops=6)  # node 59 stays isolated
    ei = np.concatenate([ei, [[7], [7]]], axis=1)
    links = np.array([[1, 2], [3, 4], [59, 59], [5, 6], [7, 8], [9, 10], [7, 7], [11, 12], [13, 13]])
    sizes = [0, 5, 1, 0, 0, 7, 1, 8, 0]
    rowptr, ids = _rows(_random_rows(rng, n - 1, links, sizes))
    return AdjCase('empty_rows', n, ei, links, rowptr, ids, empty=[0, 3, 4, 8], single=[2, 6], T=22)


def adj_sweep():
    """T = ADJ_SWEEP + 21 listed nodes: 66 rows of about 2 000 ids over a 4 000-node multigraph (the grid takes a full sweep of 131 072
    nodes and a partial second one), then two empty rows"""
    rng = np.random.default_rng(66)
    n, T = 4000, ADJ_SWEEP + 21
    ei = _random_graph(rng, n, 14000, copies=3000, loops=200)
    sizes = rng.integers(1960, 2040, size=65).tolist()
    sizes += [T - sum(sizes), 0, 0]
    links = rng.integers(0, n, size=(68, 2))
    links[5, 1] = links[5, 0]
    rowptr, ids = _rows(_random_rows(rng, n, links, sizes))
    return AdjCase('sweep', n, ei, links, rowptr, ids, T=T, rows=66, empty=[66, 67])


ADJ_CASES = {'runs': adj_runs, 'steps': adj_steps, 'switch': adj_switch, 'empty_rows': adj_empty_rows, 'sweep': adj_sweep}


# ---- labels ----------------------------------------------------------------------------------------------------------------------------------
class LabelCase(object):
    """name, rowptr int64 [B + 1], roots int32 [B, 2] (PRESET for an empty row), adj_ptr int64 [T + 1], nbr int32 [A], claims {};
    max_dists / lds: what the case is run at; row(q) -> (local ptr, nbr, ru, rv)"""

    def __init__(self, name, rows, max_dists=(1, 3, 1000, MAX_DIST_TOP), lds=(LDS_NODES,), **claims):
        self.name, self.max_dists, self.lds, self.claims = name, tuple(max_dists), tuple(lds), claims
        self.rowptr = _ro(np.concatenate([[0], np.cumsum([r[0] for r in rows])]).astype(np.int64))
        self.roots = _ro(np.array([[r[1], r[2]] for r in rows], dtype=np.int32).reshape(-1, 2))
        counts = np.concatenate([np.diff(r[3]) for r in rows] + [np.zeros((0,), dtype=np.int64)])
        self.adj_ptr = _ro(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
        self.nbr = _ro(np.concatenate([r[4] for r in rows] + [np.zeros((0,), dtype=np.int32)]).astype(np.int32))

    @property
    def B(self):
        return self.rowptr.size - 1

    @property
    def T(self):
        return int(self.rowptr[-1])

    def row(self, q):
        a, b = self.rowptr[q], self.rowptr[q + 1]
        e0 = self.adj_ptr[a]
        return self.adj_ptr[a:b + 1] - e0, self.nbr[e0:self.adj_ptr[b]], int(self.roots[q, 0]), int(self.roots[q, 1])


PRESET_ROOT = -7  # what an empty row's roots hold: the label kernel never reads them


def ws_ptr(rowptr, lds_max_nodes):
    """as subgraphs._adjacency_and_labels lays the label workspace out: the nodes of the rows longer than the on-chip limit before row q"""
    sizes = np.diff(rowptr)
    return np.concatenate([[0], np.cumsum(np.where(sizes > min(lds_max_nodes, LDS_NODES), sizes, 0))]).astype(np.int64)


def kinds(case, lds_max_nodes):
    """the kind of every row at one limit, as indices into KINDS (a one-root row is 'one_root' in either tier)"""
    sizes = np.diff(case.rowptr)
    k = np.where(sizes > min(lds_max_nodes, LDS_NODES), 1, 0)
    k = np.where(case.roots[:, 0] == case.roots[:, 1], 3, k)
    return np.where(sizes == 0, 2, k)


def _row(n, ru, rv, tgt, src):
    """one row from arcs src -> tgt (local indices): the adjacency row of t lists the distinct sources, ascending"""
    tgt, src = np.asarray(tgt, dtype=np.int64).reshape(-1), np.asarray(src, dtype=np.int64).reshape(-1)
    pair = np.unique(tgt * max(n, 1) + src)
    tgt, src = pair // max(n, 1), pair % max(n, 1)
    assert 0 <= ru < n and 0 <= rv < n and (pair.size == 0 or 0 <= pair.min() <= pair.max() < n * n)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))]).astype(np.int64)
    return n, ru, rv, ptr, src.astype(np.int32)


def _sym(n, ru, rv, a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return _row(n, ru, rv, np.concatenate([a, b]), np.concatenate([b, a]))


def _path_row(n, ru, rv):
    return _sym(n, ru, rv, np.arange(n - 1), np.arange(1, n))


def label_path():
    """paths of 2 048 (on chip: the queue's entry 2 047, 2 047 levels), 2 049 and 5 000 nodes (workspace), the roots at the two ends
    and adjacent in the middle: max_dist 1 000 clips strictly inside the row, 2^20 clips nothing"""
    sizes = (2048, 2049, 5000)
    rows = [_path_row(n, *r) for n in sizes for r in ((0, n - 1), (n // 2 - 1, n // 2))]
    return LabelCase('path', rows, sizes=sizes, depth=[n - 1 for n in sizes])


def _star(k, ru, rv):
    return _sym(k + 1, ru, rv, np.zeros(k, dtype=np.int64), np.arange(1, k + 1))


WIDE_STARS = (15, 16, 17, 255, 256, 257)


def label_wide():
    """rows 0 .. 5: a star of k children from its centre alone (ru == rv: the frontier is f0 = k, f1 = 0); rows 6 .. 11: the same with
    v the last child (f0 = k, f1 = 1); row 12: two trees, u with 5 children and 16 grandchildren, v with 30 children and one grandchild
    (f0 + f1 = 5 + 30: the sides change inside the first pass of 16; then 16 + 1: exactly at the pass); row 13: a root, 64 children and
    a K_{64,64} layer below them, v the last node of it"""
    rows = [_star(k, 0, 0) for k in WIDE_STARS] + [_star(k, 0, k) for k in WIDE_STARS]
    # u = 0, its children 1 .. 5, grandchildren 6 .. 21; v = 22, its children 23 .. 52, one grandchild 53
    a = [0] * 5 + [1 + k % 5 for k in range(16)] + [22] * 30 + [23]
    b = list(range(1, 6)) + list(range(6, 22)) + list(range(23, 53)) + [53]
    rows.append(_sym(54, 0, 22, a, b))
    top, low = np.arange(1, 65), np.arange(65, 129)
    rows.append(_sym(129, 0, 128, np.concatenate([np.zeros(64, dtype=np.int64), np.repeat(top, 64)]), np.concatenate([top, np.tile(low, 64)])))
    return LabelCase('wide', rows, stars=WIDE_STARS, two_trees=(12, [1, 5, 16], [1, 30, 1]), bipartite=(13, [1, 64, 64]))


def label_cut():
    """part {0, 1, 2} -- 3 -- part {4, 5, 6}: with roots (0, 3) the far part is reached from 0 only through 3 ('de': depths 3, 4, 5;
    'de+' and 'drnl': max_dist); row 1 has the roots swapped"""
    a, b = [0, 1, 0, 2, 3, 4, 5], [1, 2, 2, 3, 4, 5, 6]
    return LabelCase('cut', [_sym(7, 0, 3, a, b), _sym(7, 3, 0, a, b)], far=[4, 5, 6], de=[3, 4, 5])


def label_directed():
    """asymmetric rows: a one-way ring of 7 (the walk from y follows nbr[y]: depths from 0 and from 3 differ and never meet the other
    way round), and a random directed graph of 40 nodes"""
    ring = _row(7, 0, 3, np.arange(7), (np.arange(7) + 1) % 7)
    rng = np.random.default_rng(40)
    rand = _row(40, 4, 31, rng.integers(0, 40, size=90), rng.integers(0, 40, size=90))
    return LabelCase('directed', [ring, rand])


def label_one_root():
    """ru == rv: a path from its middle, a star from a leaf, a random graph, a single node"""
    rng = np.random.default_rng(1)
    return LabelCase('one_root', [_path_row(33, 16, 16), _star(20, 7, 7), _sym(50, 9, 9, rng.integers(0, 50, size=70), rng.integers(0, 50, size=70)),
                                  _row(1, 0, 0, [], [])])


def label_far():
    """three isolated nodes, roots 0 and 1: node 2 is unreachable from both; DRNL at max_dist 2^20 is 2^40 + 1"""
    return LabelCase('far', [_row(3, 0, 1, [], [])], max_dists=(1, MAX_DIST_TOP), drnl_top=(1 << 40) + 1)


def _chorded_path(rng, n, ru, rv):
    a, b = rng.integers(0, n, size=n // 8), rng.integers(0, n, size=n // 8)
    return _sym(n, ru, rv, np.concatenate([np.arange(n - 1), a]), np.concatenate([np.arange(1, n), b]))


LIMITS_LDS = (17, 2048, 4096)


def label_limits():
    """rows of 17, 18, 2 048 and 2 049 nodes (paths with a few chords), run at lds_max_nodes 17, 2 048 and 4 096: a row of exactly the
    limit stays on chip, one more takes the workspace, and 4 096 is 2 048"""
    rng = np.random.default_rng(17)
    sizes = (17, 18, 2048, 2049)
    rows = [_chorded_path(rng, n, 0, n - 1) for n in sizes]
    return LabelCase('limits', rows, lds=LIMITS_LDS, sizes=sizes,
                     workspace={17: [18, 2048, 2049], 2048: [2049], 4096: [2049]})


MANY_LDS = 24


def many_kinds():
    """the kind of every row of label_many: workgroup w labels rows w, w + LABEL_GRID, w + 2 * LABEL_GRID"""
    B = 2 * LABEL_GRID + 7
    k = np.zeros(B, dtype=np.int64)
    w = np.arange(LABEL_GRID)
    k[:LABEL_GRID] = w % 4
    k[LABEL_GRID:2 * LABEL_GRID] = (w % 4 + 1 + (w // 4) % 3) % 4
    for q in range(7):
        k[2 * LABEL_GRID + q] = [c for c in range(4) if c not in (k[q], k[LABEL_GRID + q])][q % 2]
    return k


def label_many():
    """B = 2 * 1536 + 7 rows of at most 60 nodes at lds_max_nodes = 24: a workgroup labels two or three rows from the same LDS arrays,
    on-chip rows (2 .. 24 nodes), workspace rows (25 .. 60), empty rows and one-root rows (1 .. 24) in turn"""
    rng = np.random.default_rng(1536)
    rows = []
    for kind in many_kinds():
        n = int({0: rng.integers(2, MANY_LDS + 1), 1: rng.integers(MANY_LDS + 1, 61), 2: 0, 3: rng.integers(1, MANY_LDS + 1)}[kind])
        if n == 0:
            rows.append((0, PRESET_ROOT, PRESET_ROOT, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)))
            continue
        ru = int(rng.integers(0, n))
        rv = ru if kind == 3 else int((ru + 1 + rng.integers(0, n - 1)) % n)
        m = n + n // 2
        rows.append(_sym(n, ru, rv, rng.integers(0, n, size=m), rng.integers(0, n, size=m)))
    return LabelCase('many', rows, lds=(MANY_LDS,), B=2 * LABEL_GRID + 7)


LABEL_CASES = {'path': label_path, 'wide': label_wide, 'cut': label_cut, 'directed': label_directed, 'one_root': label_one_root,
               'far': label_far, 'limits': label_limits, 'many': label_many}


# ---- through exact_subgraphs -----------------------------------------------------------------------------------------------------------------
def api_graph():
    """300 nodes, about 900 arcs, symmetric; 3 100 links (more than two rows for every label workgroup)"""
    rng = np.random.default_rng(300)
    a, b = rng.integers(0, 300, size=450), rng.integers(0, 300, size=450)
    ei = np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int64)
    links = rng.integers(0, 300, size=(3100, 2)).astype(np.int64)
    return 300, _ro(ei), _ro(links)
