"""What tests/test_exact_tables_planted_host.py and tests/test_exact_tables_planted_gpu.py share: ONE graph whose node ids are chosen
against the node tables of csrc/ss_exact_bfs.hpp, the links that drive the three call families through them (exact_subgraph_features,
exact_subgraph_nodes / exact_subgraphs, sampled_subgraph_nodes), a host model of the on-chip table's probe, and the expected rows by
the restatements.  No test lives here; numpy only at import (scipy and the restatements are imported where a function calls them).

The on-chip tier keys a 4 096-slot open-addressing table in LDS by lds_hash(x) = (x * 2654435761u) >> 20 and probes linearly, wrapping
with & 4095; a slot's value is a 16-bit half of a word shared with its neighbour; the slots are released one by one after every link.
The large tier keeps a level byte per node, four to a word, walks frontier nodes above kBigDegree in-arcs from a 64-entry list and emits
rows by an ordered scan of 4 096 nodes per step.  Random ids spread evenly over the table; the ids here do not:

  one_home      a star whose leaves are every id of home slot 2: one chain of >= 24 displaced keys
  wrap          a star whose leaves are every id with a home in the last 8 slots: the cluster runs over slot 4 095 into slot 0
  window        two stars (hubs A, B) whose leaves are every id of a 64-slot window each (about 1 560): one cluster displaced by hundreds
                of slots that still fits the on-chip limit; the link (A, B) passes it.  Three more stars (C, D, E) with 1 023, 1 023 and
                1 024 leaves of the windows behind: the unions of (C, D) and (C, E) are exactly 2 048 and 2 049
  halves        pairs (x, y) with homes 2k and 2k + 1, alone in their value word, x reached by u only and y by v only at different
                levels; quads 4j .. 4j + 3 of one level word of the large tier, two reached by u only and two by v only
  raced_key     a star of colliding leaves whose every arc is listed 16 times in a row, four leaves with a tail of their own home hung
                on by 16 copies of one arc: the 16 lanes of the group that walks a tail meet one new key at once, behind taken slots
  big_boundary  frontier nodes of exactly 512 and 513 in-arcs (arc multiplicity makes up the degree) and one level of 70 nodes above
                512, six more than the big list holds
  scan_edges    a star over the ids 0, 4 095, 4 096, 4 097, 8 191, 8 192, N - 2 and N - 1, the other ids of their level words isolated;
                graph(99_999) is the same graph without id 99 999: its last level word is partial

Everything expected is a restatement's answer (expected_*), computed once per (case, h, mask) on the part of the graph the links can
reach -- every piece is a component of its own -- and shared; tests/test_exact_tables_planted_host.py pins that restriction, the
planted claims and the constants below on the header's text."""
import collections

import numpy as np

# ---- the constants of csrc/ss_exact_bfs.hpp (tests/test_exact_tables_planted_host.py reads them out of the header) -------------------------
HASH_MULTIPLIER = 2654435761
SLOT_BITS = 12                    # kExactSlotsLog
SLOTS = 1 << SLOT_BITS            # kExactSlots
HASH_SHIFT = 32 - SLOT_BITS
NODE_LIMIT = SLOTS // 2           # kExactMaxNodes: the most nodes a link's union may hold on chip
BIG_DEGREE = 512                  # kBigDegree: a frontier node with MORE in-arcs is walked by the whole workgroup
BIG_LIST = 64                     # kBigList
SCAN_WORDS = 4                    # kScanWords: level words per thread and step of the ordered scan
THREADS = 256                     # kExactThreads
NODES_PER_WORD = 4                # one level byte per node
SCAN_STEP = SCAN_WORDS * THREADS * NODES_PER_WORD  # 4 096 nodes per step
GROUP_LANES = 16                  # kRow: the lanes that walk one frontier node's arcs together
LDS_GRID = 1024                   # kExactGrid: the most workgroups of an on-chip count launch

N = 100_000
ODD_N = 99_999                    # not a multiple of 4: the last level word holds three nodes
SCAN_IDS = (0, SCAN_STEP - 1, SCAN_STEP, SCAN_STEP + 1, 2 * SCAN_STEP - 1, 2 * SCAN_STEP, N - 2, N - 1)
ONE_HOME = 2
WRAP_FROM = SLOTS - 8
WINDOW = (1000, 1064, 1128)       # hub A takes the homes [1000, 1064), hub B [1064, 1128); C, D, E the ids behind
EXACT_LEAVES = (1023, 1023, 1024)  # C, D, E: |B(C) | B(D)| = 2 048, |B(C) | B(E)| = 2 049
HALVES_HOMES = (3600, 3602, 3604, 3606)
RACED_HOMES = (7, 8)
RACED_LEAVES = 30                 # 30 * 16 = 480 in-arcs at the hub: below kBigDegree, the star stays off the big list
RACED_COPIES = GROUP_LANES
RACED_TAILS = 4                   # leaves with a tail: a node whose only in-arcs are 16 copies of one arc
BIG_LEVEL = 70                    # children of hub Q above kBigDegree: six more than kBigList
REUSE_ROWS = 6 * LDS_GRID + 100    # every on-chip workgroup serves six links, some a seventh
REUSE_STEP = 17                   # places between the links a workgroup serves (prime to the number of planted links)
SAMPLED_SEED = 20240911
REUSE_SAMPLING = (24, 0.5)         # (cap, ratio) of the sampled call over the reuse list


def home(x):
    """lds_hash: the slot at which the probe for node x starts (ints or int arrays)"""
    return ((np.asarray(x, dtype=np.int64) * HASH_MULTIPLIER) & 0xFFFFFFFF) >> HASH_SHIFT


def probe(ids, order=None):
    """linear probing of lds_slot on the host: insert `ids` (distinct) in `order` (default: as given) -> (occupied, slot_of, moved):
    the sorted array of the occupied slots, {id: slot} and {id: how many slots past its home the id sits, counted round the table}.
    The OCCUPIED SET DOES NOT DEPEND ON THE INSERTION ORDER (linear probing fills, from every home, the next free slot; which key gets
    it changes, that it is taken does not) -- and the kernels insert in whatever order the lanes arrive.  slot_of and moved DO depend
    on it: assert on the occupied set, or on bounds that hold for every order."""
    ids = [int(x) for x in (ids if order is None else order)]
    assert len(set(ids)) == len(ids) <= SLOTS
    taken, slot_of, moved = {}, {}, {}
    for x in ids:
        i, d = int(home(x)), 0
        while i in taken:
            i, d = (i + 1) & (SLOTS - 1), d + 1
        taken[i] = x
        slot_of[x], moved[x] = i, d
    return np.array(sorted(taken), dtype=np.int64), slot_of, moved


# ---- the graph -------------------------------------------------------------------------------------------------------------------------
class Planted(object):
    """n; ei int64 [2, E]; links int64 [L, 2] and case [L] (the piece each link belongs to); names: the ids each piece is made of
    (dicts of ints and int arrays); degree int64 [n]: the in-arcs of every node, copies counted (the engine's CSR row lengths)"""

    def rows_of(self, *cases):
        return np.array([i for i, c in enumerate(self.case) if c in cases], dtype=np.int64)


class _Ids(object):
    """hands out the ids below n, each once"""

    def __init__(self, n):
        self.n, self.free, self.homes = n, np.ones(n, dtype=bool), home(np.arange(n))
        special = np.zeros(SLOTS, dtype=bool)
        special[[ONE_HOME, *RACED_HOMES]] = True
        special[WRAP_FROM:] = True
        special[WINDOW[0]:WINDOW[2] + 160] = True
        special[HALVES_HOMES[0] - 8:HALVES_HOMES[-1] + 2] = True
        self.ordinary = ~special[self.homes]  # of no planted home
        self.plain_pool = self.ordinary & (self.homes >= 2048) & (self.homes < 3500)

    def take(self, ids):
        ids = np.atleast_1d(np.asarray(ids, dtype=np.int64))
        assert self.free[ids].all() and np.unique(ids).size == ids.size
        self.free[ids] = False
        return ids

    def of_homes(self, lo, hi):
        """every free id with a home in [lo, hi), by (home, id)"""
        ids = np.nonzero(self.free & (self.homes >= lo) & (self.homes < hi))[0]
        return ids[np.argsort(self.homes[ids], kind='stable')]

    def plain(self, count=1):
        """the next free ids of no planted home (hubs, connectors, isolated partners)"""
        return self.take(np.nonzero(self.free & self.plain_pool)[0][:count])


_MADE = {}


def graph(n=N):
    """the planted graph on n nodes (N, or ODD_N: the same ids and arcs without node 99 999), built once per n and read-only"""
    if n in _MADE:
        return _MADE[n]
    assert n in (N, ODD_N)
    ids = _Ids(N)
    und, links, case, names = [], [], [], {}  # und: (a, b, copies of a -> b, copies of b -> a)

    def star(hub, leaves, ab=1, ba=1):
        und.extend((int(hub), int(x), ab, ba) for x in leaves)

    def path(*nodes):
        und.extend((int(a), int(b), 1, 1) for a, b in zip(nodes[:-1], nodes[1:]))

    def link(name, u, v, both=True):
        for a, b in ((u, v), (v, u))[:2 if both else 1]:
            links.append((int(a), int(b)))
            case.append(name)

    # scan_edges first: its ids are fixed, and the rest of their level words stays isolated
    words = sorted({x // NODES_PER_WORD for x in SCAN_IDS})
    ids.take([x for w in words for x in range(NODES_PER_WORD * w, NODES_PER_WORD * w + NODES_PER_WORD)])
    hub, iso = ids.plain(2)
    star(hub, SCAN_IDS)
    names['scan_edges'] = dict(hub=int(hub), iso=int(iso), leaves=np.array(SCAN_IDS))
    link('scan_edges', hub, iso)
    link('scan_edges', 0, N - 2)
    link('scan_edges', SCAN_STEP - 1, 2 * SCAN_STEP)
    link('scan_edges', SCAN_STEP + 1, 2 * SCAN_STEP - 1)
    link('scan_edges', SCAN_STEP, SCAN_STEP)
    link('scan_edges_top', 0, N - 1)          # (the links graph(ODD_N) cannot answer: id 99 999)
    link('scan_edges_top', N - 1, N - 1, both=False)

    # one_home
    leaves = ids.take(ids.of_homes(ONE_HOME, ONE_HOME + 1))
    hub, iso = ids.plain(2)
    star(hub, leaves)
    names['one_home'] = dict(hub=int(hub), iso=int(iso), leaves=leaves)
    link('one_home', hub, iso)
    link('one_home', leaves[0], leaves[-1])
    link('one_home', hub, leaves[len(leaves) // 2])

    # wrap
    leaves = ids.take(ids.of_homes(WRAP_FROM, SLOTS))
    hub, iso = ids.plain(2)
    star(hub, leaves)
    names['wrap'] = dict(hub=int(hub), iso=int(iso), leaves=leaves)
    link('wrap', hub, iso)
    link('wrap', leaves[0], leaves[-1])
    link('wrap', hub, leaves[len(leaves) // 2])

    # window: A and B, then C, D, E with hand-picked leaf counts
    la, lb = ids.take(ids.of_homes(WINDOW[0], WINDOW[1])), ids.take(ids.of_homes(WINDOW[1], WINDOW[2]))
    rest = ids.of_homes(WINDOW[2], WINDOW[2] + 160)
    cuts = np.cumsum((0,) + EXACT_LEAVES)
    lc, ld, le = (ids.take(rest[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
    a, b, c, d, e, iso = ids.plain(6)
    for hub, leaves in ((a, la), (b, lb), (c, lc), (d, ld), (e, le)):
        star(hub, leaves)
    names['window'] = dict(hubs=np.array([a, b, c, d, e]), iso=int(iso), leaves=[la, lb, lc, ld, le])
    link('window', a, iso)
    link('window', la[0], la[-1])
    link('window', a, la[len(la) // 2])
    link('window_two_hubs', a, b)
    link('window_2048', c, d)
    link('window_2049', c, e)

    # halves: u - .. - x and v - .. - y in two components, x at level 1 + i % 3 of u and y at level 1 + (i + 1) % 3 of v
    pairs = []
    for i, k in enumerate(HALVES_HOMES):
        assert k % 2 == 0
        x, y = ids.take(ids.of_homes(k, k + 1)[:1])[0], ids.take(ids.of_homes(k + 1, k + 2)[:1])[0]
        lx, ly = 1 + i % 3, 1 + (i + 1) % 3
        pu, pv = ids.plain(lx), ids.plain(ly)
        path(*pu, x)
        path(*pv, y)
        pairs.append((int(pu[0]), int(pv[0]), int(x), int(y), lx, ly))
        link('halves', pu[0], pv[0], both=False)
    # the level word 4j .. 4j + 3: 4j at level 1 of u, 4j + 1 at level 2 of v, 4j + 2 at level 2 of u, 4j + 3 at level 1 of v
    quads = []
    j = 12500
    while len(quads) < 2:
        q = np.arange(4 * j, 4 * j + 4)
        if ids.free[q].all() and ids.ordinary[q].all():
            ids.take(q)
            u, cu, v, cv = ids.plain(4)
            path(q[0], u, cu, q[2])
            path(q[3], v, cv, q[1])
            quads.append((int(u), int(v), int(q[0])))
            link('halves', u, v, both=False)
        j += 1
    names['halves'] = dict(pairs=pairs, quads=quads)

    # raced_key: every arc 16 times in a row.  The engine's CSR leaves the order inside a row unspecified, so the copies of one arc
    # need not stay side by side in the hub's row; a TAIL hangs on each of the first leaves by 16 copies of one arc, its row is one
    # source 16 times in any order, and the group that walks a tail meets its leaf as one new key in all 16 lanes
    # at once.  Tails and the leaves they hang on all have home RACED_HOMES[0]: a tail is a root, so it holds that slot before its
    # leaf arrives, and the racing insert has to probe past occupied slots -- one for (tail, isolated), one and three for (tail, tail)
    first, second = ids.of_homes(RACED_HOMES[0], RACED_HOMES[0] + 1), ids.of_homes(RACED_HOMES[1], RACED_HOMES[1] + 1)
    tails = ids.take(first[-RACED_TAILS:])
    leaves = ids.take(np.concatenate([first[:-RACED_TAILS], second])[:RACED_LEAVES])
    hub, iso = ids.plain(2)
    star(hub, leaves, RACED_COPIES, RACED_COPIES)
    for x, y in zip(leaves, tails):
        und.append((int(x), int(y), RACED_COPIES, RACED_COPIES))
    names['raced_key'] = dict(hub=int(hub), iso=int(iso), leaves=leaves, tails=tails)
    link('raced_key', hub, iso)
    link('raced_key', leaves[0], leaves[-1])
    link('raced_key', hub, leaves[RACED_TAILS + 1])
    link('raced_key', tails[0], iso)
    link('raced_key', tails[1], tails[2])

    # big_boundary: hub T over a child of exactly 512 in-arcs and one of 513; hub Q over 70 children above 512 and three of 512.  A
    # child has two leaves of its own (one in-arc each way) and the rest of its in-arcs are copies of the hub's arc
    def family(hub, degrees):
        kids = ids.plain(len(degrees))
        for kid, deg in zip(kids, degrees):
            und.append((int(hub), int(kid), deg - 2, 1))
            star(kid, ids.plain(2))
        return kids

    t, q, iso = ids.plain(3)
    t_kids = family(t, (BIG_DEGREE, BIG_DEGREE + 1))
    q_kids = family(q, [BIG_DEGREE + 1 + i % 3 for i in range(BIG_LEVEL)] + [BIG_DEGREE] * 3)
    names['big_boundary'] = dict(t=int(t), q=int(q), iso=int(iso), t_kids=t_kids, q_kids=q_kids)
    link('big_boundary', t, iso)
    link('big_boundary', t_kids[0], t_kids[1])
    link('big_boundary', q, iso)
    link('big_boundary', q_kids[0], q_kids[-1])
    link('big_boundary', q, q_kids[BIG_LEVEL // 2])

    src, dst = [], []
    for a, b, ab, ba in und:
        src += [a] * ab + [b] * ba
        dst += [b] * ab + [a] * ba
    ei = np.array([src, dst], dtype=np.int64)
    lk, case = np.array(links, dtype=np.int64), np.array(case)
    if n == ODD_N:  # the same graph without its last node
        ei = ei[:, (ei < n).all(axis=0)]
        keep = (lk < n).all(axis=1)
        lk, case = lk[keep], case[keep]
        names['scan_edges'] = dict(names['scan_edges'], leaves=np.array([x for x in SCAN_IDS if x < n]))
    g = Planted()
    g.n, g.ei, g.links, g.case, g.names = n, ei, lk, case, names
    g.degree = np.bincount(ei[1], minlength=n)
    g.ei.setflags(write=False)
    g.links.setflags(write=False)
    g._component, g._expected = None, {}
    _MADE[n] = g
    return g


def reuse_links(g, rows=REUSE_ROWS):
    """(links int64 [rows, 2], of int64 [rows], swapped bool [rows]): row r = 1 024 b + w is planted link of[r] = (w + REUSE_STEP *
    (b // 2)) % L, AS IT IS in the even blocks b and with its ends SWAPPED in the odd ones.  An on-chip count launch runs 1 024
    workgroups, each over the rows q, q + 1 024, ...: workgroup w serves (u, v), (v, u) of one link, then (u', v'), (v', u') of the
    link REUSE_STEP places on, then a third pair, all from one table.  A value half that a release leaves behind carries the other
    side's bits into the swapped link's counts, a key left behind is one node too many in the next link's union, and where the three
    links lie on both sides of the on-chip limit the workgroup finishes a link (lds_release), abandons one (lds_clear) and serves the
    next from the table that left.  (The fill launches run 768 workgroups: another mix.)"""
    r = np.arange(rows)
    w, b = r % LDS_GRID, r // LDS_GRID
    of = (w + REUSE_STEP * (b // 2)) % len(g.links)
    swapped = b % 2 == 1
    links = np.where(swapped[:, None], g.links[of][:, ::-1], g.links[of])
    return np.ascontiguousarray(links), of, swapped


def reuse_limit(sizes):
    """the on-chip limit that sends about a third of the reuse rows (the largest unions) to the large tier"""
    return int(np.sort(sizes)[(2 * len(sizes)) // 3])


def workgroups_serving_after_an_overflow(sizes, limit, grid=LDS_GRID):
    """how many of the `grid` workgroups of an on-chip count launch serve a row within `limit` straight after one beyond it: the
    link that is served from the table lds_clear has just rebuilt"""
    count = 0
    for w in range(grid):
        over = np.asarray(sizes[w::grid]) > limit
        count += bool((over[:-1] & ~over[1:]).any())
    return count


# ---- the expected rows, by the restatements ----------------------------------------------------------------------------------------------
class Part(object):
    """the components of g that some links touch: nodes int64 [m] ascending (g's ids), arcs int64 [2, e] (g's ids, copies kept) and the
    same renumbered by rank in `nodes`: small_n, small_arcs, small_links; small_loops: a self loop at every kept node (every node of g
    lies below n_self = max(edge_index) + 1 = n, which tests/test_exact_tables_planted_host.py asserts)"""


def restrict(g, links):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    if g._component is None:
        A = sp.csr_matrix((np.ones(g.ei.shape[1]), (g.ei[0], g.ei[1])), shape=(g.n, g.n))
        g._component = connected_components(A, directed=False)[1]
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    keep = np.isin(g._component, np.unique(g._component[links.reshape(-1)]))
    p = Part()
    p.n, p.links = g.n, links
    p.nodes = np.nonzero(keep)[0]
    p.arcs = g.ei[:, keep[g.ei[0]]]
    p.small_n = p.nodes.size
    p.small_arcs = np.searchsorted(p.nodes, p.arcs)
    p.small_links = np.searchsorted(p.nodes, links)
    loops = np.arange(p.small_n)
    p.small_loops = np.stack([loops, loops])
    return p


def _cached(g, key, make):
    if key not in g._expected:
        out = make()
        for a in (out if isinstance(out, tuple) else ()):
            for b in (a if isinstance(a, tuple) else (a,)):
                if isinstance(b, np.ndarray):
                    b.setflags(write=False)
        g._expected[key] = out
    return g._expected[key]


def _links_key(g, links):
    """(links int64 [L, 2], what names them in a cache key): g's own planted links unless others are given"""
    if links is None:
        return g.links, None
    links = np.ascontiguousarray(links, dtype=np.int64).reshape(-1, 2)
    return links, links.tobytes()


def expected_features(g, h, mask, links=None):
    """(features fp32, I, balls) of every planted link of g (or of `links`) by exact_restatement; mask: a link that is an edge is
    restated on the graph without both arcs of it (masked_restatement.without_link)"""
    links, key = _links_key(g, links)

    def make():
        import exact_restatement as er
        p = restrict(g, links)
        e = np.concatenate([p.small_arcs, p.small_loops], axis=1)
        f, I, balls = er.restate(p.small_n, e, p.small_links, h)
        if mask:
            for q, (u, v) in enumerate(p.small_links.tolist()):
                own = ((e[0] == u) & (e[1] == v)) | ((e[0] == v) & (e[1] == u))
                if u != v and own.any():
                    f[q], I[q], balls[q] = [x[0] for x in er.restate(p.small_n, e[:, ~own], np.array([[u, v]]), h)]
        return f, I, balls
    return _cached(g, ('features', h, mask, key), make)


def expected_nodes(g, h, mask, links=None):
    """(rowptr, ids, dist) of every planted link of g (or of `links`) by exact_nodes_restatement, ids in g's numbering"""
    links, key = _links_key(g, links)

    def make():
        import exact_nodes_restatement as nr
        p = restrict(g, links)
        rowptr, ids, dist = nr.restate(p.small_n, p.small_arcs, p.small_links, h, mask_target=mask, directed=True)
        return rowptr, p.nodes[ids], dist
    return _cached(g, ('nodes', h, mask, key), make)


def union_sizes(g, h, mask, links=None):
    """int64 [L]: |B_h(u) | B_h(v)| per link -- what decides the tier of the features and node-list calls: a union of at most the limit
    stays on chip"""
    return np.diff(expected_nodes(g, h, mask, links)[0])


def in_arc_table(g):
    """{x: set of the sources of the arcs into x}: the sampled restatement's sparse neighbour table (its keys hash g's ids)"""
    def make():
        table = collections.defaultdict(set)
        for j, x in zip(g.ei[0].tolist(), g.ei[1].tolist()):
            table[x].add(j)
        return table
    return _cached(g, 'table', make)


def expected_sampled(g, h, cap, ratio, links=None, seed=SAMPLED_SEED):
    """((rowptr, ids, hop), visited int64 [L], sampled) of every planted link of g (or of `links`) by sampled_subgraph_restatement.
    visited: the roots and every hop's whole fringe -- what the on-chip table of the sampled walk holds, so what decides ITS tier;
    sampled: the links where some hop dropped a node"""
    links, key = _links_key(g, links)

    def make():
        import sampled_subgraph_restatement as ssr
        table = in_arc_table(g)
        out = ssr.restate_nodes(g.n, g.ei, links, h, cap=cap, ratio=ratio, seed=seed, nb=table, return_info=True)
        visited = []
        for u, v in links.tolist():
            fr = []
            ssr.walk(table, u, v, h, cap, ratio, seed, fr)
            visited.append(len({u, v}) + sum(F for F, _ in fr))
        return out[:3], np.array(visited, dtype=np.int64), int(out[3]['sampled_links'])
    return _cached(g, ('sampled', h, cap, ratio, seed, key), make)


def take_rows(rowptr, ids, per_node, of):
    """the rows `of` (a list of row indices, repeats allowed) of a node-row triple, as a triple of their own"""
    lens = np.diff(rowptr)[of]
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    at = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in of] + [np.zeros((0,), dtype=np.int64)]).astype(np.int64)
    return out_ptr, ids[at], per_node[at]
