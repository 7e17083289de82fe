"""The semantics of WedgeGraph.candidates (subgraph-sketching_amd/wedge.py, csrc/ss_wedge.hip) restated in numpy, one
source at a time, plus the graphs the two-hop tests share.  Nothing here imports the package: the GPU tests compare the kernels with
this file, the host tests compare this file with a brute force over every walk and with scipy.

    graph            the directed pairs u -> v of edge_index as given: no self loops added, duplicates kept, negative ids wrapped
    row u            every v with u -> v, duplicates kept
    walk of u        u -> w -> v, w in row u, v in row w; each copy of a repeated edge is its own walk
    W(u)             the number of walks = sum of deg(w) over w in row u
    common[u, v]     the walks of u that end in v
    candidates of u  every v != u with common[u, v] >= min_common and (u -> v) not in `exclude`
    skipped          a source outside [-N, N), or with W(u) > max_walks or W(u) >= 2^31: lists nothing, is counted
"""
import functools

import numpy as np


def rows_of(N, ei):
    """row u = the sorted int64 array of every v with u -> v in ei, duplicates kept, negative ids wrapped"""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    ei = np.where(ei < 0, ei + N, ei)
    order = np.lexsort((ei[1], ei[0]))
    starts = np.searchsorted(ei[0][order], np.arange(N + 1))
    return [ei[1][order][starts[u]:starts[u + 1]] for u in range(N)]


def walks(N, ei, sources):
    """int64 [S]: W(u) per source, 0 for a source outside [-N, N)"""
    rows = rows_of(N, ei)
    deg = np.array([len(r) for r in rows], dtype=np.int64)
    out = []
    for u in np.asarray(sources, dtype=np.int64).reshape(-1).tolist():
        u = u + N if u < 0 else u
        out.append(int(deg[rows[u]].sum()) if 0 <= u < N else 0)
    return np.array(out, dtype=np.int64)


def candidates(N, ei, sources, exclude=None, min_common=1, max_walks=None):
    """(rowptr int64 [S + 1], ids int64 [T], common int32 [T], skipped sources): row s = the candidates of sources[s], ascending"""
    rows = rows_of(N, ei)
    gone = rows_of(N, exclude) if exclude is not None else None
    W = walks(N, ei, sources)
    rowptr, ids, common, skipped = [0], [], [], 0
    for s, u in enumerate(np.asarray(sources, dtype=np.int64).reshape(-1).tolist()):
        u = u + N if u < 0 else u
        if not 0 <= u < N or W[s] >= (1 << 31) or (max_walks is not None and W[s] > max_walks):
            skipped += 1
            rowptr.append(len(ids))
            continue
        ends = np.concatenate([rows[w] for w in rows[u]]) if len(rows[u]) else np.zeros(0, dtype=np.int64)
        count = np.bincount(ends, minlength=N)
        ok = count >= min_common
        ok[u] = False
        if gone is not None:
            ok[gone[u]] = False
        v = np.nonzero(ok)[0]
        ids.extend(v.tolist())
        common.extend(count[v].tolist())
        rowptr.append(len(ids))
    return np.array(rowptr, dtype=np.int64), np.array(ids, dtype=np.int64), np.array(common, dtype=np.int32), skipped


# ---- the graphs ---------------------------------------------------------------------------------------------------------------------
def symmetric(e):
    e = np.asarray(e, dtype=np.int64).reshape(2, -1)
    return np.concatenate([e, e[::-1]], axis=1)


def star(n=64):
    """centre 0, leaves 1 .. n - 2, node n - 1 isolated: every walk of the centre returns to it, a leaf's end in the centre's row"""
    return n, symmetric(np.stack([np.zeros(n - 2, dtype=np.int64), np.arange(1, n - 1)]))


def clique(n=12, N=64):
    """a K_n on nodes 0 .. n - 1 of N nodes"""
    return N, symmetric(np.array([[a, b] for a in range(n) for b in range(a + 1, n)]).T)


def path(n=64):
    a = np.arange(n - 1, dtype=np.int64)
    return n, symmetric(np.stack([a, a + 1]))


def odd_graph():
    """directed, 64 nodes: the edge 0 -> 1 three times and 1 -> 2 twice, a self loop at 3 (with 3 -> 4), the one-way edge 5 -> 6 (6 has
    no out-edge), 7 <-> 8 alone (the only walks of 7 return to 7), negative ids for 9 -> 10 -> 11, and node 63 isolated at the end"""
    N = 64
    e = [(0, 1)] * 3 + [(1, 2)] * 2 + [(1, 0), (3, 3), (3, 4), (4, 3), (5, 6), (7, 8), (8, 7), (9 - N, 10), (10, 11 - N), (2, 0), (2, 5)]
    return N, np.array(e, dtype=np.int64).T


@functools.lru_cache(maxsize=None)
def _boundary():
    # source i -> its own hubs, a hub -> its own leaves: W = the leaves behind the source's hubs
    e, nxt = [], [16]

    def fresh(n):
        a = list(range(nxt[0], nxt[0] + n))
        nxt[0] += n
        return a

    for src, fans in ((0, [31]), (1, [32]), (2, [33]), (3, [10, 22]), (5, [1] * 32)):
        for n in fans:
            hub = fresh(1)[0]
            e.append((src, hub))
            e.extend((hub, v) for v in fresh(n))
    sink = fresh(1)[0]  # source 4: 32 neighbours that all lead to ONE node
    for w in fresh(32):
        e.append((4, w))
        e.append((w, sink))
    N = nxt[0] + 1
    ei = np.array(e, dtype=np.int64).T
    ei.setflags(write=False)
    return N, ei


def boundary_graph():
    """(N, edge_index, directed): W(0) = 31, W(1) = 32 (one hub), W(2) = 33, W(3) = 32 over two hubs, W(4) = 32 walks that all end in
    ONE node (count 32 in one slot), W(5) = 32 walks that end in 32 distinct nodes through 32 neighbours (a 64-slot table half full);
    sources 6 .. 15 have no edge; the last node is isolated"""
    return _boundary()


def uniform_graph(n, e_und, seed):
    rng = np.random.RandomState(seed)
    return symmetric(rng.randint(0, n, size=(2, e_und)))


def induced(ei, n):
    """the edges of ei among the first n nodes"""
    ei = np.asarray(ei)
    return ei[:, (ei[0] < n) & (ei[1] < n)]
