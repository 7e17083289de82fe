"""The exact subgraph node lists restated in numpy / scipy, for the node-list tests (ElphHashes.exact_subgraph_nodes).

Per link (u, v): the distances d_u, d_v of every node from scipy.sparse.csgraph.shortest_path on the symmetrised graph without self
loops (mask_target: without the link's own edge), clipped to h + 1 (= "not within h": a sentinel, not a distance); the row lists
every node with d_u <= h or d_v <= h, ascending by id.  A root is at distance 0 from itself whatever the graph.

The engine follows in-edges (flow source -> target), which on a symmetric edge_index -- every graph of the modelled project -- is the
symmetrised graph; `directed=True` restates exactly that walk for an edge_index that is not symmetric.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path


def _arcs(edge_index, directed):
    """(rows, cols): x can step to j.  Symmetrised: both directions of every edge; directed: x -> j for every edge j -> x"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    if directed:
        r, c = ei[1], ei[0]
    else:
        r, c = np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]])
    keep = r != c
    return r[keep], c[keep]


def _distances(n, r, c, sources):
    """float [len(sources), n] hop distances (inf: unreachable)"""
    A = sp.csr_matrix((np.ones(r.size, dtype=np.float64), (r, c)), shape=(n, n))
    A.sum_duplicates()
    return np.atleast_2d(shortest_path(A, method='D', directed=True, unweighted=True, indices=np.asarray(sources, dtype=np.int64)))


def restate(num_nodes, edge_index, links, h, mask_target=False, directed=False):
    """(rowptr int64 [L + 1], ids int64 [T], dist uint8 [T, 2]) of the pairs `links` (int [L, 2], negative ids wrapped)"""
    n = int(num_nodes)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    links = np.where(links < 0, links + n, links)
    r, c = _arcs(edge_index, directed)
    rowptr, ids, dist = [0], [], []
    if len(links):
        nodes, inv = np.unique(links.reshape(-1), return_inverse=True)
        inv = inv.reshape(-1, 2)
        plain = _distances(n, r, c, nodes)
    for q, (u, v) in enumerate(links):
        d = plain[inv[q]]
        if mask_target and u != v:
            own = ((r == u) & (c == v)) | ((r == v) & (c == u))
            if own.any():
                d = _distances(n, r[~own], c[~own], [u, v])
        d = np.where(d <= h, d, h + 1).astype(np.uint8)
        x = np.nonzero((d[0] <= h) | (d[1] <= h))[0]
        ids.append(x.astype(np.int64))
        dist.append(d[:, x].T)
        rowptr.append(rowptr[-1] + x.size)
    ids = np.concatenate(ids) if ids else np.zeros((0,), dtype=np.int64)
    dist = np.concatenate(dist).reshape(-1, 2) if dist else np.zeros((0, 2), dtype=np.uint8)
    return np.asarray(rowptr, dtype=np.int64), ids, np.ascontiguousarray(dist, dtype=np.uint8)


def rows(rowptr, ids, dist):
    """[(ids, dist)] per link"""
    return [(ids[a:b], dist[a:b]) for a, b in zip(rowptr[:-1], rowptr[1:])]
