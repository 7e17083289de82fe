"""Planted graphs, witness tables and the plain reference for the TABLE HOPS (csrc/ss_walks.hpp minhash_walk128 / minhash_walk / hll_walk /
hll_hop_row16, csrc/ss_hub.hpp table_hub_units, the HLL side of csrc/ss_fused_hop.hip): shared by test_table_hop_planted_host.py and
test_table_hop_planted_gpu.py.  numpy and Python only; nothing here touches the engine's kernels.

A table hop folds the rows of a node's in-neighbours -- word-wise min (MinHash) or byte-wise max (HLL) -- into one output row.  With
hashed sketches a walk that drops one of T entries shows with probability 1 - (1 - 1/T)^P, next to never on a hub row.  Here the input
tables are planted so that EVERY entry of every row under test decides a word of the output:

  witness rounds   round k makes the entries at positions t, t // W == k, witnesses (W words per row: P or M).  Entry t holds at word
                   t % W a value no other entry of its row can beat -- MinHash t + 1 against noise >= 0x4000 0000, HLL
                   30 + t % (max_register - 29) against noise bytes 1 .. 20.  Whoever drops entry t, reads it at the wrong chunk or
                   folds it into the wrong word changes word t % W, and the wrong value names a position.  ceil(T / W) rounds cover a row.
  poison           the row of a node under test is its own witness at position `deg` where it counts; where it does not (no self
                   loop, or skipped) it holds poison in every word of every witness round: MinHash 0, HLL the largest legal register.
                   (A row without ANY entry is the all-zero row by definition, which a folded MinHash 0 would not change: its poison is 1.)
  colour rounds    every pool of sources has a colour >= 1, and a node under test takes its pool's colour where its own row counts;
                   every other node has colour 0.  Round (b, s) fills every word of node j with 1 + (bit b of colour(j) XOR s): what
                   a row legitimately folds is of ONE colour, and a node of any other colour -- the next row's first source, a source
                   of the neighbouring pool, its own row where it must not count -- shows in the round of a bit where the colours
                   differ, s being the foreign node's bit (MinHash: the foreigner holds 1 against 2) or its complement (HLL: 2 against 1).

Positions are those of the CSR handed in (the engine's, read back, on the GPU; `csr_of` here on the host).  `want_rows` is the plain
reference; `walk_entries` is a model of DEFECTIVE walks that only proves the cases bite and is never an expected output."""
from types import SimpleNamespace

import numpy as np

HUB_THRESHOLD = 40
MEGA_SLICE = 1024  # SS_MEGA_SLICE (the tests assert that the library agrees)
NOISE_FLOOR = 0x40000000

# totals (entries folded, the self row included where the row has it) to plant
MH_TOTALS = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 67, 71, 72, 73, 79, 80, 81, 127, 128, 129, 200)
HLL_TOTALS = (0, 1, 3, 4, 5, 15, 16, 17, 19, 20, 21, 31, 32, 33, 34, 35, 36, 37, 47, 48, 49, 63, 64, 65, 100)
FUSED_TOTALS = (0, 1, 6, 7, 8, 13, 14, 15, 16, 31, 32, 33, 34, 47, 48, 49, 100)
HUB_TOTALS = (41, 42, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 511, 512, 513, 1023, 1024, 1025)
ROW16_LONG_COUNTS = (0, 1, 2, 3, 5, 6, 7, 16)  # rows longer than 32 in an aligned block of 16
GENERIC_TOTALS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
GENERIC_TOTALS_WIDE = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 17)  # SG = 64: one neighbour per step, batches of 4; rows of 64 KB, so N stays small
SYMMETRIC_DEGREES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 39, 40, 64, 2 * MEGA_SLICE)  # regular .., one hub row, one mega row
KSOLO = 32  # neighbours a 16-lane group walks alone (hll_row16_finish_by)


def mega_degrees(S=MEGA_SLICE):
    return (S + 1, 2 * S - 2, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 62, 3 * S + 63, 3 * S + 64)


def slices_of(deg, S=MEGA_SLICE):
    """slices the build counts for a mega row: the self row is entry `deg` whether the launch has self loops or not"""
    return (deg + 1 + S - 1) // S


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
def _assemble(degrees, symmetric=False, pad=3):
    """rows under test 0 .. len(degrees) - 1, then one private pool of sources per row (consecutive ids), then `pad` nodes that occur in
    no edge (beyond the inferred self loops: all-zero rows in every setting).  The edges of a row are listed in DESCENDING source id
    and the rows interleaved, so that neither the order inside a row nor the grouping is the edge list's"""
    degrees = np.asarray(degrees, dtype=np.int64)
    n_test = len(degrees)
    start = n_test + np.concatenate([[0], np.cumsum(degrees)])
    src = np.concatenate([np.arange(start[i + 1] - 1, start[i] - 1, -1) for i in range(n_test)] + [np.zeros(0, np.int64)]).astype(np.int64)
    dst = np.repeat(np.arange(n_test, dtype=np.int64), degrees)
    order = np.argsort((np.arange(src.size) * 7919) % 104729, kind='stable')
    ei = np.stack([src[order], dst[order]])
    if symmetric:
        ei = np.concatenate([ei, ei[::-1]], axis=1)
    n = int(start[-1]) + pad
    while n % 16 in (0, 4, 8, 12):  # a partial last group of four and of sixteen
        n += 1
    return SimpleNamespace(n=n, n_test=n_test, degrees=degrees, pool_start=start, edge_index=np.ascontiguousarray(ei), symmetric=symmetric,
                           n_self=int(ei.max()) + 1 if ei.size else 0)


def main_degrees(S=MEGA_SLICE):
    """in-degrees of the rows under test of the main graph, and where its planted blocks sit.
    rows 0 .. 63: sixteen groups of four consecutive rows, group b has its row r longer than 32 iff bit r of b (the fused kernel deals
    four consecutive rows to the lane groups of a wavefront);  rows 64 .. 191: eight aligned blocks of 16 with 0, 1, 2, 3, 5, 6, 7 and 16
    rows longer than 32 (the row16 kernel deals the 16 rows of a workgroup in degree order);  then one row per remaining in-degree: every
    listed total T as in-degree T - 1 (the self row makes it T) and as in-degree T (launches without self loops).  Long rows of the
    blocks have 33 .. 40 entries -- regular under the hub threshold of 40 as well -- and short ones at most 31, so that a row is long
    or short with and without its self row"""
    long_cycle = (33, 34, 35, 36, 37, 40, 39, 38)
    short_cycle = (0, 1, 5, 6, 7, 8, 12, 13, 14, 15, 16, 30, 31, 3, 4, 2, 17, 19, 20, 21)
    degs, nl, ns = [], 0, 0
    for b in range(16):
        for r in range(4):
            if (b >> r) & 1:
                degs.append(long_cycle[nl % len(long_cycle)])
                nl += 1
            else:
                degs.append(short_cycle[ns % len(short_cycle)])
                ns += 1
    for k in ROW16_LONG_COUNTS:
        block = [long_cycle[(nl + q) % len(long_cycle)] if (q * 7) % 16 < k else short_cycle[(ns + q) % len(short_cycle)] for q in range(16)]
        nl, ns = nl + 3, ns + 5
        degs.extend(block)
    assert len(degs) == 64 + 16 * len(ROW16_LONG_COUNTS)
    singles = set()
    for T in MH_TOTALS + HLL_TOTALS + FUSED_TOTALS + HUB_TOTALS:
        singles.update({T, max(T - 1, 0)})
    singles.update(mega_degrees(S))
    singles = sorted(singles)
    return degs + singles, SimpleNamespace(fused=(0, 64), row16=(64, 64 + 16 * len(ROW16_LONG_COUNTS)), singles=(len(degs), len(degs) + len(singles)))


_cache = {}


def main_graph(S=MEGA_SLICE):
    if ('main', S) not in _cache:
        degs, blocks = main_degrees(S)
        g = _assemble(degs)
        g.blocks = blocks
        _cache[('main', S)] = g
    return _cache[('main', S)]


def generic_graph(wide=False):
    """the smaller graph of the run-time-sized kernel: rows of at most 300 entries, totals around the sub-group count 64 / SG and the batch
    of 4 * (64 / SG) entries of every SG; wide: the few totals of SG = 64, on a graph small enough for rows of 64 KB"""
    key = ('generic', wide)
    if key not in _cache:
        degs = set()
        for T in (GENERIC_TOTALS_WIDE if wide else GENERIC_TOTALS):
            degs.update({T, max(T - 1, 0)})
        _cache[key] = _assemble(sorted(degs))
    return _cache[key]


def symmetric_graph(S=MEGA_SLICE):
    if ('symmetric', S) not in _cache:
        degs = [d if d != 2 * MEGA_SLICE else 2 * S for d in SYMMETRIC_DEGREES]
        _cache[('symmetric', S)] = _assemble(degs, symmetric=True)
    return _cache[('symmetric', S)]


def csr_of(edge_index, n):
    """(rowptr int64 [n + 1], col int32 [E]) grouped by destination, sources ascending within a row"""
    src, dst = edge_index
    order = np.lexsort((src, dst))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    return rowptr, src[order].astype(np.int32)


def is_csr_of(rowptr, col, edge_index, n):
    """the CSR (read back from the engine) holds exactly the edges, grouped by destination, in whatever order within a row"""
    want_rp, want_col = csr_of(edge_index, n)
    if not np.array_equal(rowptr, want_rp) or len(col) < want_rp[-1]:
        return False
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    order = np.lexsort((col[:rowptr[-1]], dst))
    return np.array_equal(col[:rowptr[-1]][order], want_col)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def counts_self(rowptr, n_self, skip, hub_rows):
    """bool [N]: row i folds its own row as entry `deg`.  i < n_self; left out for a REGULAR row with deg > 0 when the skip word applies
    (csrc/ss_common.hpp table_hop_total); always kept by a row that a hub or mega unit serves (csrc/ss_hub.hpp table_hub_units:
    total = deg + (i < n_self))"""
    N = len(rowptr) - 1
    deg = np.diff(rowptr)
    own = np.arange(N) < n_self
    if skip:
        regular = np.ones(N, dtype=bool)
        regular[np.asarray(list(hub_rows), dtype=np.int64)] = False
        own &= ~(regular & (deg > 0))
    return own


def want_rows(rowptr, col, n_self, skip, hub_rows, table, reduce):
    """numpy min / max (reduce: 'min' or 'max') over the entries of each row: col[rowptr[i]:rowptr[i + 1]] in CSR order, then row i itself
    where counts_self says so; a row without any entry is all zero"""
    op = {'min': np.minimum, 'max': np.maximum}[reduce]
    N = len(rowptr) - 1
    deg = np.diff(rowptr)
    out = np.zeros_like(table)
    has = np.flatnonzero(deg > 0)
    if has.size:
        out[has] = op.reduceat(table[col[:rowptr[-1]].astype(np.int64)], rowptr[has], axis=0)
    own = counts_self(rowptr, n_self, skip, hub_rows)
    both = own & (deg > 0)
    out[both] = op(out[both], table[both])
    alone = own & (deg == 0)
    out[alone] = table[alone]
    return out


# ---- the planting -------------------------------------------------------------------------------------------------------------------------
def hll_max_register(M):
    p = int(M).bit_length() - 1
    assert 1 << p == M
    return 64 - p + 1  # hll_planted.max_register


class Plan(object):
    """what the tables of one launch setting hold: the graph's CSR, the self loops of the launch (n_self; skip and the rows the hub units
    serve, which keep their own row under it), and per node its position as an entry of the row UNDER TEST it belongs to"""

    def __init__(self, rowptr, col, n_test, n_self, skip=False, hub_rows=(), seed=1):
        self.rowptr, self.col, self.n_test, self.n_self, self.skip = np.asarray(rowptr), np.asarray(col), n_test, int(n_self), bool(skip)
        self.hub_rows = tuple(sorted(int(r) for r in hub_rows))
        self.N = len(rowptr) - 1
        self.deg = np.diff(self.rowptr)
        self.own = counts_self(self.rowptr, self.n_self, self.skip, self.hub_rows)
        self.total = self.deg + self.own
        self.pos = np.full(self.N, -1, dtype=np.int64)     # position of the node in the row under test that lists it (or its own)
        self.colour = np.zeros(self.N, dtype=np.int64)
        for i in range(n_test):
            nodes = self.col[self.rowptr[i]:self.rowptr[i + 1]].astype(np.int64)
            assert (nodes >= n_test).all() and (self.pos[nodes] == -1).all() and len(set(nodes.tolist())) == len(nodes), 'private, distinct pools'
            self.pos[nodes] = np.arange(len(nodes))
            self.colour[nodes] = i + 1
            if self.own[i]:
                self.pos[i] = self.deg[i]
                self.colour[i] = i + 1
        self.poison = np.zeros(self.N, dtype=bool)
        self.poison[:n_test] = ~self.own[:n_test]
        self.colour_bits = max(int(n_test).bit_length(), 1)  # colours 0 .. n_test
        self.seed = seed
        self._base = {}

    def entries(self, i):
        """node ids row i folds, in walk order"""
        nodes = self.col[self.rowptr[i]:self.rowptr[i + 1]].astype(np.int64)
        return np.append(nodes, i) if self.own[i] else nodes

    def rounds(self, W):
        """[(kind, k)]: the witness rounds that cover the longest row under test, then the colour rounds"""
        t_max = int(self.total[:self.n_test].max()) if self.n_test else 0
        return [('witness', k) for k in range(max(-(-t_max // W), 1))] + [('colour', k) for k in range(2 * self.colour_bits)]

    def _noise_base(self, W, sketch):
        if (W, sketch) not in self._base:
            rng = np.random.RandomState(self.seed + W + (0 if sketch == 'minhash' else 1))
            self._base[(W, sketch)] = (rng.randint(0, 1 << 30, size=(self.N, W), dtype=np.int64).astype(np.uint32) if sketch == 'minhash' else
                                       rng.randint(0, 20, size=(self.N, W)).astype(np.uint8))
        return self._base[(W, sketch)]

    def _colour_value(self, k, nodes, reduce):
        b, s = divmod(k, 2)
        return 1 + (((self.colour[nodes] >> b) & 1) ^ s)

    def minhash_table(self, kind, k, P, nodes=None):
        """uint32 [len(nodes), P] (nodes None: all) of round (kind, k)"""
        nodes = np.arange(self.N) if nodes is None else np.asarray(nodes, dtype=np.int64)
        if kind == 'colour':
            return np.repeat(self._colour_value(k, nodes, 'min').astype(np.uint32)[:, None], P, axis=1)
        mix = np.uint32((0x9E3779B1 * (k + 1)) & 0x3FFFFFFF)
        t = (self._noise_base(P, 'minhash')[nodes] ^ mix) | np.uint32(NOISE_FLOOR)   # depends on (node, word, round)
        pos = self.pos[nodes]
        w = np.flatnonzero((pos >= 0) & (pos // P == k))
        t[w, pos[w] % P] = (pos[w] + 1).astype(np.uint32)
        t[self.poison[nodes]] = 0
        t[self.poison[nodes] & (self.deg[nodes] == 0)] = 1
        return t

    def hll_table(self, kind, k, M, nodes=None):
        """uint8 [len(nodes), M] of round (kind, k); every register within hll_planted.max_register(log2 M)"""
        nodes = np.arange(self.N) if nodes is None else np.asarray(nodes, dtype=np.int64)
        if kind == 'colour':
            return np.repeat(self._colour_value(k, nodes, 'max').astype(np.uint8)[:, None], M, axis=1)
        top = hll_max_register(M)
        t = (self._noise_base(M, 'hll')[nodes] + np.uint8((7 * k) % 20)) % np.uint8(20) + np.uint8(1)
        pos = self.pos[nodes]
        w = np.flatnonzero((pos >= 0) & (pos // M == k))
        t[w, pos[w] % M] = (30 + pos[w] % (top - 29)).astype(np.uint8)
        t[self.poison[nodes]] = top
        return t

    def table(self, sketch, kind, k, W, nodes=None):
        return self.minhash_table(kind, k, W, nodes) if sketch == 'minhash' else self.hll_table(kind, k, W, nodes)

    def want(self, sketch, table):
        return want_rows(self.rowptr, self.col, self.n_self, self.skip, self.hub_rows, table, 'min' if sketch == 'minhash' else 'max')


def encoded_position(sketch, kind, k, W, word, value):
    """what a wrong value says about where it came from"""
    value = int(value)
    if kind == 'colour':
        return f'a node whose colour bit {k // 2} is {(value - 1) ^ (k % 2)}' if value in (1, 2) else 'no colour value'
    if sketch == 'minhash':
        if value == 0 or value == 1 and word != 0:
            return 'poison: the own row of a node that must not count'
        return f'entry {value - 1}' if value < NOISE_FLOOR else 'noise: the witness of this word was not folded'
    if value >= 30:
        top = hll_max_register(W)
        return f'entry {k * W + word} if its witness ({30 + (k * W + word) % (top - 29)}), else poison ({top}) or a witness folded into the wrong word'
    return 'noise: the witness of this word was not folded' if value else 'nothing folded'


def first_difference(got, want, sketch, kind, k, what, rows=None):
    """None, or the message of the first differing word: entry point, round, row, word, got, wanted, the position the wrong value encodes"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f'{what}: shape {got.shape} against {want.shape}'
    bad = np.argwhere(got != want)
    if not bad.size:
        return None
    r, w = (int(x) for x in bad[0])
    W = want.shape[1]
    n_rows = len(np.unique(bad[:, 0]))
    return (f'{what}, {sketch} {kind} round {k}: row {int(rows[r]) if rows is not None else r} word {w}: got {int(got[r, w])}, wanted {int(want[r, w])} '
            f'(got encodes {encoded_position(sketch, kind, k, W, w, got[r, w])}; wanted encodes {encoded_position(sketch, kind, k, W, w, want[r, w])}); '
            f'{len(bad)} words in {n_rows} rows differ, first rows {np.unique(bad[:, 0])[:8].tolist()}')


# ---- a model of defective walks: proves that the planted cases bite, never an expected output -------------------------------------------
DEFECTS = ('drops_last_entry', 'drops_lonely_self_row', 'reads_previous_chunk', 'folds_one_past_total', 'skips_a_slice')


def walk_entries(plan, i, defect, S=MEGA_SLICE):
    """the node ids a walk with `defect` folds for row i, or None where the defect cannot occur on that row"""
    good = plan.entries(i)
    T, deg = len(good), int(plan.deg[i])
    if defect == 'drops_last_entry':
        return good[:-1] if T else None
    if defect == 'drops_lonely_self_row':  # the self row is the only entry of its 64-chunk, or of its slice
        return good[:-1] if plan.own[i] and deg > 0 and deg % 64 == 0 else None
    if defect == 'reads_previous_chunk':   # the last chunk's entry t comes from position (t & 63) of the chunk before it
        if T <= 64:
            return None
        lo = (T - 1) // 64 * 64
        bad = good.copy()
        bad[lo:] = good[lo - 64:lo - 64 + (T - lo)]
        return bad
    if defect == 'folds_one_past_total':   # the own row where it does not count (entry `deg` of every walk), else the word after the row's last
        if not plan.own[i]:
            return np.append(good, i)
        nxt = plan.rowptr[i + 1]
        return np.append(good, int(plan.col[nxt])) if nxt < plan.rowptr[-1] else None
    if defect == 'skips_a_slice':
        return np.concatenate([good[:S], good[2 * S:]]) if T > S else None
    raise ValueError(defect)


def fold(plan, sketch, kind, k, W, nodes):
    t = plan.table(sketch, kind, k, W, nodes)
    if not len(nodes):
        return np.zeros(W, dtype=t.dtype)
    return t.min(axis=0) if sketch == 'minhash' else t.max(axis=0)


def defect_shows(plan, sketch, W, i, bad):
    """the (kind, k) of a round in which folding `bad` instead of row i's entries changes the output row, or None"""
    good = plan.entries(i)
    changed = np.setxor1d(good, bad)
    if len(good) == len(bad):
        changed = np.union1d(changed, np.concatenate([good[good != bad], bad[good != bad]]))
    first = [('witness', int(plan.pos[j]) // W) for j in changed if plan.pos[j] >= 0]
    rounds = plan.rounds(W)
    order = [r for r in dict.fromkeys(first) if r in rounds] + [r for r in rounds if r[0] == 'colour'] + [r for r in rounds if r[0] == 'witness']
    for kind, k in dict.fromkeys(order):
        if not np.array_equal(fold(plan, sketch, kind, k, W, good), fold(plan, sketch, kind, k, W, bad)):
            return kind, k
    return None


def sole_holders(plan, sketch, W, i):
    """bool [T]: entry t of row i is, in its witness round t // W, the ONLY entry of the row that attains the folded value of word t % W
    -- which is what `removing the entry changes want_rows` means for a min or a max"""
    nodes = plan.entries(i)
    T = len(nodes)
    out = np.zeros(T, dtype=bool)
    for k in range(-(-T // W)):
        t = plan.table(sketch, 'witness', k, W, nodes).astype(np.int64)
        if sketch == 'hll':
            t = -t
        lo, hi = k * W, min(T, (k + 1) * W)
        cols = np.arange(lo, hi) % W
        sub = t[:, cols]                                   # [T, hi - lo]
        best = sub.min(axis=0)
        out[lo:hi] = (sub[np.arange(lo, hi), np.arange(hi - lo)] == best) & ((sub == best).sum(axis=0) == 1)
    return out


def long_row_patterns(totals, by_degree):
    """the set of 4-bit patterns `which of a wavefront's four rows fold more than KSOLO entries` over aligned blocks: of 4 consecutive
    rows (the fused kernel), or -- by_degree: the in-degrees -- of 16 rows dealt in degree order, ties by row (the row16 kernel)"""
    totals = np.asarray(totals)
    out = set()
    if by_degree is None:
        for q in range(0, len(totals) - 3, 4):
            out.add(sum(1 << r for r in range(4) if totals[q + r] > KSOLO))
        return out
    for q in range(0, len(totals) - 15, 16):
        order = np.lexsort((np.arange(16), np.asarray(by_degree[q:q + 16])))
        dealt = totals[q:q + 16][order]
        for w in range(4):
            out.add(sum(1 << r for r in range(4) if dealt[4 * w + r] > KSOLO))
    return out
