"""The exact enclosing subgraphs restated in numpy, for the subgraph tests (ElphHashes.exact_subgraphs).

The node rows are those of exact_nodes_restatement.restate on the in-arc walk the engine follows (directed=True; on a symmetric
edge_index that is the symmetrised graph).  Per link this file adds
  the local adjacency   row of listed node x: the distinct j != x of the link's row with an arc j -> x in edge_index, as local indices,
                        ascending, with the number of copies (np.unique over the sources of x's in-arcs); mask_target and u != v: without
                        (x = u, j = v) and (x = v, j = u) -- SEAL's subgraph[0, 1] = subgraph[1, 0] = 0
  roots                 the local indices of u and v
  the BFS depths        from a root over those adjacency rows, optionally with one node removed (a plain queue)
  the labels            'de', 'de+', 'drnl' of the reference's labelling_tricks.py from those depths; 'hop' / 'zo' from the ball distances
u == v (outside the reference's domain): one root, nothing removed, both depths equal.
adjacency_of_rows() is the adjacency and the roots of node rows made by anyone (restate() calls it; tests/subgraph_planted.py hands it
hand-made rows); link_labels() takes one link's raw arrays.
"""
from collections import deque

import numpy as np

import exact_nodes_restatement as nr

INF = np.iinfo(np.int64).max


class Restated(object):
    """rowptr, ids, dist, roots, adj_ptr, nbr, weight as ExactSubgraphs holds them (numpy); z per label through labels()"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def row(self, q):
        a, b = self.rowptr[q], self.rowptr[q + 1]
        e0 = self.adj_ptr[a]
        return self.ids[a:b], self.adj_ptr[a:b + 1] - e0, self.nbr[e0:self.adj_ptr[b]], self.weight[e0:self.adj_ptr[b]]


def restate(num_nodes, edge_index, links, h, mask_target=True, max_nodes=None):
    n = int(num_nodes)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    links = np.where(links < 0, links + n, links)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    rowptr, ids, dist = nr.restate(n, ei, links, h, mask_target=mask_target, directed=True)
    if max_nodes is not None:
        keep = np.diff(rowptr) <= max_nodes
        rows = [r if k else (r[0][:0], r[1][:0]) for r, k in zip(nr.rows(rowptr, ids, dist), keep)]
        rowptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
        ids = np.concatenate([r[0] for r in rows] + [np.zeros((0,), dtype=np.int64)])
        dist = np.concatenate([r[1].reshape(-1, 2) for r in rows] + [np.zeros((0, 2), dtype=np.uint8)])
    roots, adj_ptr, nbr, weight = adjacency_of_rows(n, ei, links, rowptr, ids, mask_target)
    return Restated(rowptr=rowptr, ids=ids, dist=dist, roots=roots, adj_ptr=adj_ptr, nbr=nbr, weight=weight, links=links)


def adjacency_of_rows(num_nodes, edge_index, links, rowptr, ids, mask_target):
    """(roots int32 [L, 2], adj_ptr int64 [T + 1], nbr int32 [A], weight int32 [A]) of given node rows: row q = ids[rowptr[q] :
    rowptr[q + 1]], ascending, distinct, with both ends of links[q] (ids in [0, num_nodes)) unless it is empty; whoever made the rows"""
    n = int(num_nodes)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    # in-arcs grouped by target: sources of the arcs j -> x at src[ptr[x] : ptr[x + 1]]
    order = np.argsort(ei[1], kind='stable')
    src = ei[0][order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=n))])
    roots = np.full((len(links), 2), -1, dtype=np.int32)
    counts, nbr, weight = [], [], []
    for q, (u, v) in enumerate(links):
        row = ids[rowptr[q]:rowptr[q + 1]]
        if row.size == 0:
            continue
        roots[q] = [np.searchsorted(row, u), np.searchsorted(row, v)]
        assert row[roots[q, 0]] == u and row[roots[q, 1]] == v
        for x in row:
            j, w = np.unique(src[ptr[x]:ptr[x + 1]], return_counts=True)
            ok = j != x
            if mask_target and u != v:
                ok &= j != (v if x == u else u if x == v else -1)
            at = np.minimum(np.searchsorted(row, j), row.size - 1)
            ok &= row[at] == j
            counts.append(int(ok.sum()))
            nbr.append(at[ok])
            weight.append(w[ok])
    adj_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda parts: np.concatenate(parts + [np.zeros((0,), dtype=np.int64)]).astype(np.int32)
    return roots, adj_ptr, cat(nbr), cat(weight)


def bfs(ptr, nbr, root, removed=-1):
    """int64 [n] depths from local node `root` over the adjacency rows (INF: unreachable; `removed` is never entered and stays INF)"""
    depth = np.full((len(ptr) - 1,), INF, dtype=np.int64)
    depth[root] = 0
    todo = deque([root])
    while todo:
        y = todo.popleft()
        for j in nbr[ptr[y]:ptr[y + 1]]:
            if j != removed and depth[j] == INF:
                depth[j] = depth[y] + 1
                todo.append(j)
    return depth


def drnl(du, dv):
    d = du + dv
    z = 1 + np.minimum(du, dv) + (d // 2) * (d // 2 + d % 2 - 1)
    z[(du == 0) | (dv == 0)] = 1
    return z


def link_labels(ptr, nbr, ru, rv, node_label, max_dist):
    """the labels of one link's subgraph: int64 [n] ('drnl') or [n, 2] ('de', 'de+')"""
    remove = node_label in ('de+', 'drnl') and ru != rv
    du = bfs(ptr, nbr, ru, rv if remove else -1)
    dv = bfs(ptr, nbr, rv, ru if remove else -1) if ru != rv else du.copy()
    if remove:  # the removed partner's own entry, put in before the clip as labelling_tricks.py does
        du[rv] = dv[ru] = 0 if node_label == 'drnl' else 1
    du, dv = np.minimum(du, max_dist), np.minimum(dv, max_dist)
    return drnl(du, dv) if node_label == 'drnl' else np.stack([du, dv], axis=1)


def labels(sub, node_label, max_dist=1000):
    """z of a Restated for one label mode (None for None)"""
    if node_label is None:
        return None
    if node_label in ('hop', 'zo'):
        hop = sub.dist.min(axis=1).astype(np.int64) if len(sub.dist) else np.zeros((0,), dtype=np.int64)
        return hop if node_label == 'hop' else (hop == 0).astype(np.int64)
    out = [np.zeros((0, 2) if node_label != 'drnl' else (0,), dtype=np.int64)]
    for q in range(len(sub.rowptr) - 1):
        if sub.rowptr[q + 1] > sub.rowptr[q]:
            _, ptr, nbr, _ = sub.row(q)
            out.append(link_labels(ptr, nbr, int(sub.roots[q, 0]), int(sub.roots[q, 1]), node_label, max_dist))
    return np.concatenate(out).astype(np.int64)
