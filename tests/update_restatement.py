"""The rule of ElphHashes.update_hash_tables restated in numpy / scipy (no code shared with the engine), plus the graph generators and
"rebuild and diff" helpers of tests/test_update_host.py and tests/test_update_gpu.py.

With n_self = max(edge_index) + 1 of the NEW graph (0 when it has no edge) and its in-edges j -> i:
  seed    = targets of `added` + targets of `removed` + { i : (i < n_self) != (cards_old[i, 0] > 0) }  (a row had its implicit self loop
            iff its old hop-1 HLL row was non-zero iff its old hop-1 cardinality is positive)
  dirty_1 = seed
  dirty_k = seed + { i : i has an in-neighbour in dirty_{k-1}, or (i < n_self and i in dirty_{k-1}) }
Hop k of the update recomputes exactly the rows of dirty_k."""
import numpy as np
import scipy.sparse as sp


def n_self_of(edge_index):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    return int(ei.max()) + 1 if ei.size else 0


def dirty_sets(num_nodes, new_edge_index, cards_old, added=None, removed=None, max_hops=3):
    """-> {k: bool [N]} for k = 1 .. max_hops"""
    n = int(num_nodes)
    ei = np.asarray(new_edge_index, dtype=np.int64).reshape(2, -1)
    n_self = n_self_of(ei)
    seed = np.zeros(n, dtype=bool)
    for ch in (added, removed):
        if ch is not None:
            seed[np.asarray(ch, dtype=np.int64).reshape(2, -1)[1]] = True
    had_loop = np.asarray(cards_old)[:, 0] > 0
    seed |= (np.arange(n) < n_self) != had_loop
    # A[i, j] = 1 iff j -> i is an edge of the new graph (pull form)
    A = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.int32), (ei[1], ei[0])), shape=(n, n))
    loops = np.arange(n) < n_self
    dirty = {1: seed.copy()}
    for k in range(2, max_hops + 1):
        prev = dirty[k - 1]
        pulled = np.asarray(A @ prev.astype(np.int32)).reshape(-1) > 0
        dirty[k] = seed | pulled | (loops & prev)
    return dirty


def undirected(e):
    e = np.asarray(e, dtype=np.int64).reshape(2, -1)
    return np.concatenate([e, e[::-1]], axis=1)


def uniform_graph(n, e_und, seed):
    rng = np.random.RandomState(seed)
    return undirected(rng.randint(0, n, size=(2, e_und)))


def power_law_graph(n, e_und, seed, exponent=3.0):
    """targets drawn as n * u^exponent: node 0 is the largest hub"""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, size=e_und)
    dst = np.minimum((n * rng.random_sample(e_und) ** exponent).astype(np.int64), n - 1)
    return undirected(np.stack([src, dst]))


def remove_edges(edge_index, und_positions):
    """drop the undirected edges at `und_positions` of an edge list laid out as undirected() makes it -> (new edge_index, removed [2, 2R])"""
    ei = np.asarray(edge_index, dtype=np.int64)
    half = ei.shape[1] // 2
    pos = np.asarray(und_positions, dtype=np.int64)
    keep = np.ones(ei.shape[1], dtype=bool)
    keep[pos] = False
    keep[pos + half] = False
    return ei[:, keep], np.concatenate([ei[:, pos], ei[:, pos + half]], axis=1)


def add_edges(edge_index, und_edges):
    """append the undirected edges [2, A] -> (new edge_index, added [2, 2A])"""
    add = undirected(und_edges)
    return np.concatenate([np.asarray(edge_index, dtype=np.int64), add], axis=1), add


def directed_graph(n, e, seed):
    """e directed edges with uniform endpoints (copies and self loops as they fall)"""
    return np.random.RandomState(seed).randint(0, n, size=(2, e)).astype(np.int64)


def remove_directed(edge_index, positions):
    """drop the directed edges at `positions` -> (new edge_index, removed [2, R])"""
    ei = np.asarray(edge_index, dtype=np.int64)
    pos = np.asarray(positions, dtype=np.int64)
    keep = np.ones(ei.shape[1], dtype=bool)
    keep[pos] = False
    return ei[:, keep], ei[:, pos]


def add_directed(edge_index, edges):
    """append the directed edges [2, A] -> (new edge_index, added [2, A])"""
    add = np.asarray(edges, dtype=np.int64).reshape(2, -1)
    return np.concatenate([np.asarray(edge_index, dtype=np.int64), add], axis=1), add


def changed_rows(old, new):
    """bool [N]: rows of two [N, W] tables that differ anywhere"""
    return (np.asarray(old) != np.asarray(new)).reshape(len(old), -1).any(axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
