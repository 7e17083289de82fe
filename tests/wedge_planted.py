"""Planted graphs for the two-hop kernels (wedge_walks_kernel, wedge_fold_kernel, wedge_emit_kernel of csrc/ss_wedge.hip), pure
numpy: tests/test_wedge_planted_gpu.py runs them through WedgeGraph.candidates and through the fold and emit launches directly,
tests/test_wedge_planted_host.py pins every plan on scipy's A[sources] @ A, and the small builds on wedge_restatement.py too.

A plan (_Plan) is written source by source: sources are the low ids, a source reaches its endpoints through intermediate nodes of its
own (fresh ids, whose rows nothing else touches), so the multiset of endpoints of every source is known from the plan, not from a
walk over the graph.  Endpoints may be any node: only the rows of a source and of its intermediates are walked.  Every graph function
returns (N, edge_index int64 [2, E], sources int64 [S], expect) with

    expect['walks']  int64 [S]   W(u)
    expect['ends']   S dicts     {v: walks of u that end in v}, v = u included (what the fold and emit kernels store)
    expect['rows']   S dicts     the same without v = u (the candidates of u at min_common = 1 without an exclude list)

A few source ids of every graph are left without an edge (W = 0), the first and the last always, so that sources without work sit
between those with work and at both ends of every list.  Each graph also holds one ordinary small source (`_ordinary`) with a walk
back to itself, an endpoint that is its own neighbour and an endpoint of count 2: min_common, v != u and exclude = the graph's own
edges all change something.

The sizes are written in terms of the kernels' own numbers, which the callers pass in: M = SS_WEDGE_MAX_SLOTS (the largest LDS
table), T = kWedgeThreads = 256 (the neighbours of one slice), R = 16 (the lanes that share a neighbour's row), and the most slices a
source is spread over.  The host tests build some graphs with smaller M and T, where wedge_restatement.py is affordable.

Below: the Python twin of the arithmetic of csrc/ss_wedge.hpp (slot, table_slots, folds, emits), a literal table of known answers of
the slot hash (KNOWN_SLOTS; tools/wedge_host_check.hip checks wedge_slot against the same numbers, so the planted collisions cannot
silently stop being collisions), the probe-chain model that the collision graphs assert their chains with, and a numpy CSR for the
order in which the emit kernel lists a source's endpoints.

Out of scope: the largest W(u) that is still listed, 2^31 - 1.  Its (key, count) arrays alone take 12 bytes per walk, 25.8 GB, and
the sort behind them more; `too_many_walks` covers the rule from the other side (2^31 exactly, and 46 341^2) and the sources next to
such a source."""
import collections

import numpy as np

T = 256   # kWedgeThreads: row u is taken T neighbours at a time
R = 16    # kRow: the lanes of a neighbour's row
N_SOURCES = 96
MAX_WALKS = (1 << 31) - 1


# ---- the twin of csrc/ss_wedge.hpp ----------------------------------------------------------------------------------------------------
def slot(v, k):
    """wedge_slot: the first slot node v is tried at in a table of 2^k slots"""
    return ((int(v) * 2654435761) % (1 << 32)) >> (32 - k)


def slots_of(ids, k):
    """slot() over an int64 array"""
    return ((np.asarray(ids, dtype=np.int64) * 2654435761) % (1 << 32)) >> (32 - k)


def folds(W, slots):
    return W > 0 and 2 * W <= slots


def emits(W, slots):
    return W > 0 and 2 * W > slots


def table_slots(W, slots):
    """wedge_table_slots: the smallest power of two >= 2 W (>= 2), at most `slots`"""
    m = slots
    while m > 2 and (m >> 1) >= 2 * W:
        m >>= 1
    return m


def log2(m):
    return int(m).bit_length() - 1


def tiers(walks, slots, cap=MAX_WALKS):
    """(sources the LDS tier serves, sources the large tier serves) among `walks`"""
    w = [int(x) for x in walks if int(x) <= cap]
    return sum(folds(x, slots) for x in w), sum(emits(x, slots) for x in w)


# (v, k, slot): from the formula in numpy uint32 arithmetic, independently of slot() above
KNOWN_SLOTS = ((0, 1, 0), (1, 1, 1), (2, 1, 0), (3, 1, 1), (69999, 1, 1), (2147483646, 1, 0), (2147483647, 1, 1),
               (1, 6, 39), (2, 6, 15), (3, 6, 54), (255, 6, 38), (65536, 6, 30), (123456789, 6, 31), (2147483647, 6, 56),
               (1, 8, 158), (5, 8, 23), (256, 8, 55), (4095, 8, 217), (69999, 8, 194), (1073741823, 8, 161), (2147483647, 8, 225),
               (1, 12, 2531), (2, 12, 966), (3, 12, 3498), (4096, 12, 1913), (65535, 12, 3511), (1000003, 12, 3444),
               (1073741824, 12, 1024), (2147483646, 12, 1081), (2147483647, 12, 3612))


def probe_places(ids, m):
    """where linear probing from slot(v) leaves each distinct id of `ids` in an empty table of m slots, inserted in the order given
    (the occupied SET does not depend on the order) -> {v: (first slot, final slot)}"""
    k, table, out = log2(m), {}, {}
    for v in ids:
        v = int(v)
        if v in out:
            continue
        h = first = slot(v, k)
        while h in table:
            h = (h + 1) & (m - 1)
        table[h] = v
        out[v] = (first, h)
    return out


def csr(N, ei):
    """(rowptr int64 [N + 1], col int64 [E]) with sorted rows, duplicates kept: numpy only, no list per node"""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    order = np.lexsort((ei[1], ei[0]))
    return np.searchsorted(ei[0][order], np.arange(N + 1)), ei[1][order]


def emit_order(rowptr, col, u):
    """the endpoints of u in the order wedge_emit_kernel documents: w ascending in row u, then v ascending in row w"""
    parts = [col[rowptr[w]:rowptr[w + 1]] for w in col[rowptr[u]:rowptr[u + 1]].tolist()]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
class _Plan(object):
    def __init__(self, n_sources=N_SOURCES):
        self.n_sources, self.next_source, self.next = n_sources, 1, n_sources  # (source 0 stays without an edge)
        self.edges = []                                       # int64 [2, n] pieces
        self.ends = collections.defaultdict(list)             # source -> [(endpoint array, copies of each walk)]

    def source(self):
        """the next source id; every fourth id is passed over and stays without an edge"""
        if self.next_source % 4 == 0:
            self.next_source += 1
        s = self.next_source
        self.next_source += 1
        assert s < self.n_sources - 1, 'more sources than the plan reserved (the last stays without an edge)'
        return s

    def fresh(self, n):
        a = np.arange(self.next, self.next + n, dtype=np.int64)
        self.next += n
        return a

    def arcs(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
        self.edges.append(np.stack([a.reshape(-1), b.reshape(-1)]))

    def through(self, src, w, ends, copies_in=1, copies_out=1):
        """src -> w (copies_in times), w -> v for every v of ends (each copies_out times): w is an intermediate of src alone"""
        ends = np.asarray(ends, dtype=np.int64).reshape(-1)
        self.arcs(np.full(copies_in, src), w)
        if ends.size:
            self.arcs(w, np.repeat(ends, copies_out))
        self.ends[src].append((ends, copies_in * copies_out))

    def hub(self, src, ends):
        """every endpoint through ONE fresh neighbour"""
        self.through(src, int(self.fresh(1)[0]), ends)

    def spokes(self, src, ends):
        """every endpoint through a fresh neighbour of its own (one arc each)"""
        ends = np.asarray(ends, dtype=np.int64).reshape(-1)
        ws = self.fresh(ends.size)
        self.arcs(src, ws)
        self.arcs(ws, ends)
        self.ends[src].append((ends, 1))

    def fans(self, src, degrees, pool, stride):
        """one fresh neighbour per entry of `degrees`, in id order; neighbour i ends in pool[(stride * i + t) % len(pool)], t < d"""
        ws = self.fresh(len(degrees))
        self.arcs(src, ws)
        for i, (w, d) in enumerate(zip(ws.tolist(), degrees)):
            assert d <= len(pool)
            ends = pool[(stride * i + np.arange(d)) % len(pool)]
            if d:
                self.arcs(w, ends)
            self.ends[src].append((ends, 1))
        return ws

    def ordinary(self):
        """src -> a, b; a -> b, src, x; b -> x: the row is {b: 1, x: 2}, one walk returns to src, b is a neighbour of src"""
        src = self.source()
        a, b, x = self.fresh(3).tolist()
        self.through(src, a, [b, src, x])
        self.through(src, b, [x])
        return src

    def finish(self, N=None):
        n = self.next + 1  # (the last node is isolated)
        N = n if N is None else N
        assert n <= N <= 70000
        ei = np.concatenate(self.edges, axis=1)
        ei.setflags(write=False)
        sources = np.arange(self.n_sources, dtype=np.int64)
        walks, ends, rows = np.zeros(self.n_sources, dtype=np.int64), [], []
        for s in range(self.n_sources):
            count = collections.Counter()
            for vs, copies in self.ends.get(s, ()):
                ids, c = np.unique(vs, return_counts=True)
                for v, k in zip(ids.tolist(), c.tolist()):
                    count[v] += k * copies
                walks[s] += vs.size * copies
            ends.append(dict(count))
            rows.append({v: c for v, c in count.items() if v != s})
        assert walks[0] == 0 and walks[-1] == 0 and ei.shape[1] < 400000
        return N, ei, sources, {'walks': walks, 'ends': ends, 'rows': rows}


def want(N, ei, sources, expect, min_common=1, exclude_edges=False, max_walks=None):
    """(rowptr int64, ids int64, common int32, skipped): what .candidates returns for the planted sources, from the plan alone.
    exclude_edges: exclude = the graph's own edge_index"""
    cap = MAX_WALKS if max_walks is None else min(max_walks, MAX_WALKS)
    rowptr, ids, common, skipped = [0], [], [], 0
    for s, u in enumerate(np.asarray(sources).tolist()):
        if expect['walks'][s] > cap:
            skipped += 1
        else:
            gone = set(ei[1][ei[0] == (u + N if u < 0 else u)].tolist()) if exclude_edges else ()
            for v in sorted(expect['rows'][s]):
                if expect['rows'][s][v] >= min_common and v not in gone:
                    ids.append(v)
                    common.append(expect['rows'][s][v])
        rowptr.append(len(ids))
    return np.array(rowptr, dtype=np.int64), np.array(ids, dtype=np.int64), np.array(common, dtype=np.int32), skipped


# ---- the graphs -----------------------------------------------------------------------------------------------------------------------
def _table_sizes(p, M):
    made = {}
    sizes = sorted({w for j in range(log2(M)) for w in (1 << j, (1 << j) + 1)})  # 2^j <= M / 2
    assert sizes[:3] == [1, 2, 3] and sizes[-2:] == [M // 2, M // 2 + 1]
    for W in sizes:
        for shape in (p.hub, p.spokes):  # one neighbour with a W-arc row; W neighbours with one arc each
            s = p.source()
            shape(s, p.fresh(W))  # distinct endpoints: at W = 2^j the table of 2^(j + 1) slots is exactly half full
            made[(W, shape.__name__)] = s
            assert folds(W, M) == (W <= M // 2) and emits(W, M) == (W > M // 2)
            if folds(W, M):
                assert table_slots(W, M) == max(2, 1 << (2 * W - 1).bit_length())
    return made


def table_sizes(M):
    """W = 2^j and 2^j + 1 for every 2^j <= M / 2 (1, 2, 3 among them), distinct endpoints, each W once through one neighbour and once
    through W neighbours: every table size 2 .. M exactly half full and one endpoint over; W = M / 2 folds, M / 2 + 1 emits.
    -> (N, ei, sources, expect, {(W, 'hub' | 'spokes'): source})"""
    p = _Plan()
    made = _table_sizes(p, M)
    made['ordinary'] = p.ordinary()
    return p.finish() + (made,)


def _wide_fold(p, M, T):
    made = {}
    for deg in (T - 1, T, T + 1, 2 * T, 2 * T + 1):  # neighbour out-degrees 0 .. 3 in turn, endpoints shared: counts above 1
        s = p.source()
        p.fans(s, [i % 4 for i in range(deg)], p.fresh(97), 3)
        made[deg] = s
    # a repeated edge u -> w: the copies are adjacent in the sorted row, at places T - 1 and T -- one in each slice
    s = p.source()
    pool = p.fresh(97)
    ws = p.fresh(2 * T - 1)
    for i, w in enumerate(ws.tolist()):
        p.through(s, w, pool[(5 * i + np.arange(1 + i % 3)) % 97], copies_in=2 if i == T - 1 else 1)
    made['repeated'] = s
    # deg(u) = M / 2, one arc per neighbour: into M / 2 distinct nodes (the largest table half full, M / (2 T) slices), and into ONE
    for name, ends in (('distinct', p.fresh(M // 2)), ('one', np.full(M // 2, p.fresh(1)[0]))):
        s = p.source()
        p.spokes(s, ends)
        made[name] = s
    return made


def wide_fold(M, T=T):
    """fold-tier sources whose row u takes more than one slice of T neighbours: deg(u) = T - 1, T, T + 1, 2 T, 2 T + 1 with
    neighbour out-degrees 0 .. 3, a repeated edge across the slice boundary, deg(u) = M / 2 into distinct nodes and into one node.
    -> (N, ei, sources, expect, {name: source})"""
    p = _Plan()
    made = _wide_fold(p, M, T)
    made['ordinary'] = p.ordinary()
    out = p.finish()
    for name, s in made.items():
        assert folds(int(out[3]['walks'][s]), M), (name, int(out[3]['walks'][s]))
    assert out[3]['ends'][made['one']] == {int(max(out[3]['ends'][made['one']])): M // 2}
    return out + (made,)


def _colliding(ids, k, homes, n):
    """the first n of `ids` whose first slot in a table of 2^k slots is one of `homes`"""
    found = ids[np.isin(slots_of(ids, k), list(homes))][:n]
    return found


def collisions(M, N=70000):
    """per table size m of 64, 256, M: a source whose m / 2 endpoints all start probing at slot m - 1 or m - 2 (the chain runs off the
    end of the table to slot 0 and on), and one whose endpoints all start at slot 0; at m = M as many such ids as N offers, the rest
    anywhere; and a source whose 16 endpoints share ONE first slot and are reached by 5 walks each (a key met again inside a chain).
    -> (N, ei, sources, expect, {name: (source, m, colliding ids)})"""
    p = _Plan()
    ids = np.arange(p.n_sources, N, dtype=np.int64)  # (no endpoint is a source)
    made = {}
    for m in sorted({64, 256, M}):
        k = log2(m)
        for name, homes in (('end', (m - 1, m - 2)), ('zero', (0,))):
            hit = _colliding(ids, k, homes, m // 2)
            assert hit.size >= (16 if m == M else m // 2), (m, name, hit.size)
            rest = np.setdiff1d(ids[:4 * m], hit)[:m // 2 - hit.size]  # (anywhere: the table ends up exactly half full)
            ends = np.concatenate([hit, rest])
            assert ends.size == m // 2 == np.unique(ends).size
            s = p.source()
            for a in range(0, ends.size, R + 1):  # through neighbours of R + 1 arcs
                p.hub(s, ends[a:a + R + 1])
            made[(name, m)] = (s, m, hit)
            places = probe_places(ends, m)
            assert table_slots(ends.size, M) == m and len(places) == m // 2
            if name == 'end':  # the chain really passes m - 1 -> 0: some id ends up below the slot it started at
                assert sum(last < first for first, last in places.values()) >= (8 if m == M else m // 2 - 2), (m, places)
            else:
                assert sum(last != first for first, last in places.values()) >= hit.size - 1
    hit = _colliding(ids, 8, (255,), 16)
    assert hit.size == 16
    s = p.source()
    for _ in range(5):
        p.hub(s, hit)
    assert table_slots(80, M) == 256 and sum(last < first for first, last in probe_places(hit, 256).values()) == 15
    made['again'] = (s, 256, hit)
    made['ordinary'] = (p.ordinary(), 0, hit[:0])
    return p.finish(N) + (made,)


def _emit_shapes(p, M, T, R, big):
    made = {}
    pool = p.fresh(big)

    def degrees(deg, bigs):
        """0 first, last and in the middle of the first slice; `big` at each place of bigs, between a 0 and a 1; else 1, R - 1, R, R + 1, 0 in turn"""
        d = [(1, R - 1, R, R + 1, 0, R)[i % 6] for i in range(deg)]
        d[0] = d[deg - 1] = d[T // 2] = 0
        for b in bigs:
            d[b - 1], d[b], d[b + 1] = 0, big, 1
        return d

    for deg, bigs in ((T - 1, (T // 4,)), (T, (T - 3,)), (T + 1, (T - 2,)), (3 * T + 5, (5, 2 * T + 9))):
        s = p.source()
        p.fans(s, degrees(deg, bigs), pool, 5)
        made[deg] = s
    s = p.source()  # every neighbour a sink: W = 0, neither tier, an empty row
    p.fans(s, [0] * 40, pool, 1)
    made['sinks'] = s
    s = p.source()  # 12 slices of one arc per neighbour
    p.spokes(s, pool[(7 * np.arange(12 * T)) % big])
    made['slices'] = s
    return made


def emit_shapes(M, T=T, R=R, big=5000):
    """large-tier sources with deg(u) = T - 1, T, T + 1, 3 T + 5 and neighbour out-degrees from {0, 1, R - 1, R, R + 1, big}: sinks
    first, last and inside a slice, the big row between a sink and a one-arc row; a source whose neighbours are all sinks; a source
    of 12 T neighbours with one arc each.  -> (N, ei, sources, expect, {name: source})"""
    p = _Plan()
    made = _emit_shapes(p, M, T, R, big)
    made['ordinary'] = p.ordinary()
    out = p.finish()
    for name, s in made.items():
        W = int(out[3]['walks'][s])
        assert W == 0 if name == 'sinks' else folds(W, M) if name == 'ordinary' else emits(W, M), (name, W)
    return out + (made,)


def mixed(M, T=T, R=R, big=5000):
    """the sources of table_sizes, wide_fold and emit_shapes in ONE graph, for the launches that are given both tiers' sources at
    once.  -> (N, ei, sources, expect, {'table_sizes' | 'wide_fold' | 'emit_shapes': {name: source}})"""
    p = _Plan(128)
    made = {'table_sizes': _table_sizes(p, M), 'wide_fold': _wide_fold(p, M, T), 'emit_shapes': _emit_shapes(p, M, T, R, big)}
    return p.finish() + (made,)


def too_many_walks(copies_in, copies_out):
    """u -> w copies_in times and w -> v copies_out times: W(u) = copies_in * copies_out >= 2^31 with under 100 000 edges; a second
    source whose only neighbour is the same w (W = copies_out, the large tier, every walk into v), two ordinary sources.
    -> (N, ei, sources, expect, {'giant' | 'beside' | 'ordinary' | 'another': source})"""
    p = _Plan(8)
    giant, beside = p.source(), p.source()
    w, v = p.fresh(2).tolist()
    p.through(giant, w, [v], copies_in=copies_in, copies_out=copies_out)
    p.arcs(beside, w)
    p.ends[beside].append((np.array([v]), copies_out))
    made = {'giant': giant, 'beside': beside, 'ordinary': p.ordinary(), 'another': p.ordinary()}  # (a source without an edge between them)
    out = p.finish(64)
    assert out[3]['walks'][giant] == copies_in * copies_out > MAX_WALKS and out[3]['walks'][beside] == copies_out
    assert out[1].shape[1] < 100000
    return out + (made,)


GIANTS = ((46341, 46341), (65536, 32768))  # W = 2 147 488 281, and 2^31 exactly
