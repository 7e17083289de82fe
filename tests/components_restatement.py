"""numpy / scipy restatement of subgraph_sketching_amd.components (csrc/ss_components.hip): the weak connected components
of an edge_index with every label canonicalised to its component's smallest node id, the sizes, the largest component under the tie rule
(most nodes, then the smallest root), the node mapper and the ordered edge filter.  Everything is exact integer work; the GPU tests compare
whole arrays with it, the host tests compare it with the reference's own component (tests/golden/g19_lcc.npz) and a plain union-find."""
import numpy as np
import scipy.sparse as ssp
from scipy.sparse.csgraph import connected_components as _scipy_components


def wrapped(N, ids):
    """torch-style negative ids wrapped (the ids are taken to lie in [-N, N))"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids < 0, ids + N, ids)


def labels(N, edge_index):
    """int64 [N]: the smallest node id of every node's weak component"""
    ei = wrapped(N, edge_index).reshape(2, -1)
    A = ssp.csr_matrix((np.ones(ei.shape[1], dtype=np.int8), (ei[0], ei[1])), shape=(N, N))
    C, lab = _scipy_components(A, directed=True, connection='weak')
    smallest = np.full(C, N, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(N, dtype=np.int64))
    return smallest[lab]


def roots_and_sizes(lab):
    """(roots ascending, their sizes), both int64 [C]"""
    roots, sizes = np.unique(lab, return_counts=True)
    assert np.array_equal(lab[roots], roots)
    return roots.astype(np.int64), sizes.astype(np.int64)


def largest(lab):
    """the node ids of the largest component, ascending; np.argmax takes the FIRST maximum of the ascending roots: the smallest root"""
    roots, sizes = roots_and_sizes(lab)
    return np.flatnonzero(lab == roots[np.argmax(sizes)]).astype(np.int64)


def tied(lab):
    """how many components share the largest size"""
    _, sizes = roots_and_sizes(lab)
    return int((sizes == sizes.max()).sum())


def induced(N, edge_index, nodes=None, mask=None):
    """(nodes, mapper, edge_index', edge_ids): the subgraph of a mask (new ids ascending) or of a list of distinct ids (new id = position)"""
    assert (nodes is None) != (mask is None)
    if mask is not None:
        nodes = np.flatnonzero(np.asarray(mask, dtype=bool))
    nodes = wrapped(N, nodes)
    assert len(set(nodes.tolist())) == len(nodes)
    mapper = np.full(N, -1, dtype=np.int64)
    mapper[nodes] = np.arange(len(nodes), dtype=np.int64)
    ei = wrapped(N, edge_index).reshape(2, -1)
    edge_ids = np.flatnonzero((mapper[ei[0]] >= 0) & (mapper[ei[1]] >= 0)).astype(np.int64)
    return nodes.astype(np.int64), mapper, mapper[ei[:, edge_ids]], edge_ids


def largest_component_subgraph(N, edge_index):
    keep = np.zeros(N, dtype=bool)
    keep[largest(labels(N, edge_index))] = True
    return induced(N, edge_index, mask=keep)


def symmetric_random_graph(N, undirected, seed):
    """the recipe of tests/golden/make_golden_lcc.py: `undirected` random pairs of numpy's default_rng(seed), each listed in both directions"""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, N, size=(2, undirected), dtype=np.int64)
    return np.concatenate([e, e[::-1]], axis=1)
