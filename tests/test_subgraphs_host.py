"""Exact enclosing subgraphs without a GPU: the numpy restatement (tests/subgraph_restatement.py) against the reference's own labelling
functions (tests/golden/g17_seal_labels.npz), against scipy slicing and against answers known by hand; the Python argument errors of
ElphHashes.exact_subgraphs (raised before the compute device is touched) and the C-ABI argument checks of ss_subgraph_adj /
ss_subgraph_labels (they return before any launch)."""
from argparse import Namespace
from ctypes import c_void_p

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import exact_nodes_restatement as nr
import subgraph_restatement as sr
from conftest import load_golden
from test_exact_nodes_host import _ba40, _uniform300

GOLDEN_LABELS = {'drnl': 'drnl', 'de': 'de', 'de+': 'deplus'}


def _multigraph():
    """24 nodes: a ring with chords whose undirected edges are repeated 1, 2 or 5 times (both directions alike), one arc repeated in one
    direction only, self loops on a root (0), on an inner node (3) and on a far node; links: an edge of every multiplicity, a
    non-edge, u == v, a negative id"""
    n = 24
    und = [(i, (i + 1) % n, (1, 2, 5)[i % 3]) for i in range(n)] + [(0, 7, 2), (3, 12, 5), (5, 18, 1), (1, 3, 1)]
    src = np.concatenate([np.repeat([a, b], m) for a, b, m in und] + [[2, 2, 2], [0, 0, 3, 20]])
    dst = np.concatenate([np.repeat([b, a], m) for a, b, m in und] + [[9, 9, 9], [0, 0, 3, 20]])
    links = np.array([[0, 1], [1, 2], [2, 3], [3, 12], [0, 12], [9, 2], [2, 9], [0, 0], [3, 3], [-1, 4], [6, 15]], dtype=np.int64)
    return n, np.stack([src, dst]).astype(np.int64), links


def _path():
    """the path u - a - v - b (0 - 1 - 2 - 3) of the design's worked example, link (u, v) = (0, 2)"""
    ei = np.array([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]], dtype=np.int64)
    return 4, ei, np.array([[0, 2]], dtype=np.int64)


def _two_components():
    """two triangles 0-1-2 and 3-4-5 and an isolated node 6; roots in different components, in one, and on the isolated node"""
    tri = np.array([[0, 1], [1, 2], [2, 0], [3, 4], [4, 5], [5, 3]]).T
    ei = np.concatenate([tri, tri[::-1]], axis=1).astype(np.int64)
    return 7, ei, np.array([[0, 3], [1, 5], [0, 1], [6, 2], [4, 4]], dtype=np.int64)


# ---- the restatement against the reference's labelling functions -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def g17():
    return load_golden('g17_seal_labels.npz')


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_restatement_equals_the_reference_labels(g17, h, mask):
    n, ei, _ = _ba40()
    links = g17[f'links_m{int(mask)}']
    assert (links[:, 0] != links[:, 1]).all() and len(links) >= (150 if mask else 8)
    sub = sr.restate(n, ei, links, h, mask_target=mask)
    key = f'h{h}_m{int(mask)}'
    np.testing.assert_array_equal(sub.rowptr, g17[key + '_rowptr'])
    np.testing.assert_array_equal(sub.ids, g17[key + '_ids'])
    for md in g17['max_dists']:
        for label, name in GOLDEN_LABELS.items():
            np.testing.assert_array_equal(sr.labels(sub, label, int(md)), g17[f'{key}_d{int(md)}_{name}'], err_msg=f'{label} max_dist {md}')


# ---- the adjacency against scipy slicing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('graph', ['ba40', 'uniform300', 'directed300', 'multigraph'])
def test_adjacency_is_the_sliced_matrix(graph, mask):
    """row x of the local adjacency = row x of M[ids][:, ids], M[x, j] = copies of the arc j -> x, without the diagonal and (masked,
    u != v) without the entries (u, v) and (v, u) -- k_hop_subgraph's A[nodes, :][:, nodes] with subgraph[0, 1] = subgraph[1, 0] = 0"""
    n, ei, links = {'ba40': _ba40, 'uniform300': _uniform300, 'directed300': lambda: _uniform300(True), 'multigraph': _multigraph}[graph]()
    M = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.int64), (ei[1], ei[0])), shape=(n, n))
    M.sum_duplicates()
    for h in (1, 2):
        sub = sr.restate(n, ei, links, h, mask_target=mask)
        assert sub.nbr.dtype == np.int32 and sub.weight.dtype == np.int32 and sub.adj_ptr.dtype == np.int64 and sub.roots.dtype == np.int32
        assert sub.adj_ptr.size == sub.ids.size + 1 and sub.adj_ptr[-1] == sub.nbr.size == sub.weight.size
        for q, (u, v) in enumerate(sub.links):
            ids, ptr, nbr, weight = sub.row(q)
            S = M[ids][:, ids].tolil()
            S.setdiag(0)
            ru, rv = sub.roots[q]
            assert ids[ru] == u and ids[rv] == v
            if mask and u != v:
                S[ru, rv] = S[rv, ru] = 0
            S = S.tocsr()
            S.eliminate_zeros()
            S.sort_indices()
            np.testing.assert_array_equal(ptr, S.indptr)
            np.testing.assert_array_equal(nbr, S.indices)
            np.testing.assert_array_equal(weight, S.data)
    if graph == 'multigraph':
        assert {1, 2, 5} <= set(sub.weight.tolist()) and (mask or 3 in sub.weight)  # (the one-way triple arc 2 -> 9 is a masked link's own)


# ---- answers known by hand -------------------------------------------------------------------------------------------------------------------
def test_path_example():
    n, ei, links = _path()
    sub = sr.restate(n, ei, links, 1, mask_target=True)
    np.testing.assert_array_equal(sub.ids, [0, 1, 2, 3])          # all four nodes are in the union of the 1-hop balls
    np.testing.assert_array_equal(sub.dist, [[0, 2], [1, 1], [2, 0], [2, 1]])
    np.testing.assert_array_equal(sub.roots, [[0, 2]])
    np.testing.assert_array_equal(sub.adj_ptr, [0, 1, 3, 5, 6])
    np.testing.assert_array_equal(sub.nbr, [1, 0, 2, 1, 3, 2])
    assert sr.labels(sub, 'de', 1000)[3].tolist() == [3, 1]       # b is three steps from u inside the subgraph: beyond h + 1
    assert sr.labels(sub, 'de+', 1000)[3].tolist() == [1000, 1]   # and unreachable from u once v is removed
    assert sr.labels(sub, 'drnl', 1000)[3] == 250002
    np.testing.assert_array_equal(sr.labels(sub, 'de+', 1000), [[0, 1], [1, 1], [1, 0], [1000, 1]])
    np.testing.assert_array_equal(sr.labels(sub, 'drnl', 1000), [1, 2, 1, 250002])
    np.testing.assert_array_equal(sr.labels(sub, 'de', 1), [[0, 1], [1, 1], [1, 0], [1, 1]])
    np.testing.assert_array_equal(sr.labels(sub, 'hop'), [0, 1, 0, 1])
    np.testing.assert_array_equal(sr.labels(sub, 'zo'), [1, 0, 1, 0])
    assert sr.labels(sub, None) is None


def test_unreachable_and_equal_roots():
    n, ei, links = _two_components()
    sub = sr.restate(n, ei, links, 2, mask_target=True)
    de, drnl = sr.labels(sub, 'de', 7), sr.labels(sub, 'drnl', 7)
    a, b = sub.rowptr[0], sub.rowptr[1]                           # (0, 3): roots in different components
    np.testing.assert_array_equal(sub.ids[a:b], [0, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(de[a:b], [[0, 7], [1, 7], [1, 7], [7, 0], [7, 1], [7, 1]])
    np.testing.assert_array_equal(drnl[a:b], [1, 14, 14, 1, 14, 14])
    a, b = sub.rowptr[4], sub.rowptr[5]                           # (4, 4): one root, nothing removed
    np.testing.assert_array_equal(sub.ids[a:b], [3, 4, 5])
    np.testing.assert_array_equal(sub.roots[4], [1, 1])
    np.testing.assert_array_equal(de[a:b], [[1, 1], [0, 0], [1, 1]])
    np.testing.assert_array_equal(drnl[a:b], [2, 1, 2])
    np.testing.assert_array_equal(sr.labels(sub, 'de+', 7)[a:b], [[1, 1], [0, 0], [1, 1]])


def test_ids_do_not_depend_on_mask_target():
    """a shortest path from {u, v} never uses the edge u - v: only the distance bytes change"""
    n, ei, _ = _ba40()
    links = ei[:, :60].T
    for h in (1, 2, 3):
        plain, masked = (nr.restate(n, ei, links, h, mask_target=m, directed=True) for m in (False, True))
        np.testing.assert_array_equal(plain[0], masked[0])
        np.testing.assert_array_equal(plain[1], masked[1])
        assert (plain[2] != masked[2]).any()


@pytest.mark.parametrize('mask', [False, True])
def test_de_labels_equal_the_ball_distances_within_h(mask):
    """a ball distance of at most h is the distance inside the induced subgraph (the path lies in the ball)"""
    n, ei, links = _uniform300()
    for h in (1, 2, 3):
        sub = sr.restate(n, ei, links, h, mask_target=mask)
        de = sr.labels(sub, 'de', 1000)
        near = sub.dist <= h
        assert near.any() and (~near).any()
        np.testing.assert_array_equal(de[near], sub.dist[near])
        assert (de[~near] > h).all()


def test_max_nodes_empties_rows():
    n, ei, links = _uniform300()
    full = sr.restate(n, ei, links, 2)
    sizes = np.diff(full.rowptr)
    cap = int(np.median(sizes))
    sub = sr.restate(n, ei, links, 2, max_nodes=cap)
    assert (np.diff(sub.rowptr)[sizes > cap] == 0).all() and (sub.roots[sizes > cap] == -1).all() and (sub.roots[sizes <= cap] >= 0).all()
    q = int(np.nonzero(sizes <= cap)[0][-1])
    for got, want in zip(sub.row(q), full.row(q)):
        np.testing.assert_array_equal(got, want)


# ---- C ABI without a GPU --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    for name in ('ss_subgraph_adj', 'ss_subgraph_labels'):
        assert name in ssa._native.SIGNATURES and hasattr(lib, name)
    assert ssa.ExactSubgraphs is ssa.subgraphs.ExactSubgraphs and hasattr(ssa.ElphHashes, 'exact_subgraphs')
    assert ssa._native.SUBGRAPH_LABELS == {'drnl': 0, 'de': 1, 'de+': 2} and ssa.knobs.SUBGRAPH_ADJ_SWITCH >= 0


def test_cabi_argument_errors():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    p = c_void_p(0x3000)  # never dereferenced: every call below returns from the host-side checks
    adj = lambda rp=p, col=p, N=100, links=p, B=10, rowptr=p, ids=p, T=50, sw=4, counts=p, adj_ptr=None, nbr=None, w=None, roots=None: \
        lib.ss_subgraph_adj(rp, col, N, links, B, rowptr, ids, T, 0, sw, counts, adj_ptr, nbr, w, roots, None)
    assert adj(B=0, links=None) == 0 and adj(T=0, ids=None) == 0          # nothing to do, no launch
    assert adj(B=-1) == -1 and adj(T=-1) == -1 and adj(N=-1) == -1
    assert adj(N=0) == -1 and adj(N=1 << 31) == -1 and adj(sw=-1) == -1
    for gone in ('rp', 'col', 'links', 'rowptr', 'ids', 'counts'):
        assert adj(**{gone: None}) == -1
    assert adj(adj_ptr=p, nbr=None, w=p, roots=p) == -1 and adj(adj_ptr=p, nbr=p, w=None, roots=p) == -1  # fill pass without outputs
    assert adj(adj_ptr=p, nbr=p, w=p, roots=None) == -1
    lab = lambda rowptr=p, B=10, roots=p, adj_ptr=p, nbr=p, mode=0, md=1000, lim=2048, ws_ptr=p, z=p: \
        lib.ss_subgraph_labels(rowptr, B, roots, adj_ptr, nbr, mode, md, lim, ws_ptr, None, z, None)
    assert lab(mode=3) == -4 and lab(mode=-1) == -4 and lab(mode=7, B=0) == -4  # an unknown label mode
    assert lab(B=0, rowptr=None) == 0
    assert lab(B=-1) == -1 and lab(md=0) == -1 and lab(md=(1 << 20) + 1) == -1 and lab(lim=-1) == -1
    for gone in ('rowptr', 'roots', 'adj_ptr', 'nbr', 'ws_ptr', 'z'):
        assert lab(**{gone: None}) == -1


# ---- Python argument errors before any launch ---------------------------------------------------------------------------------------------
def _eh(h=2):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))


def test_python_argument_errors():
    eh = _eh()
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    links = torch.tensor([[0, 1], [2, 3]])
    for bad in ('DRNL', 'degree', 'drnl-', 0, True):
        with pytest.raises(ValueError, match='node_label'):
            eh.exact_subgraphs(links, 5, ei, node_label=bad)
    for bad in (0, -1, (1 << 20) + 1, 2.0, '3', True, None):
        with pytest.raises(ValueError, match='max_dist'):
            eh.exact_subgraphs(links, 5, ei, max_dist=bad)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError):
            eh.exact_subgraphs(links, 5, ei, mask_target=bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            eh.exact_subgraphs(links, 5, ei, max_nodes=bad)
    for bad in (torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.float32)):
        with pytest.raises(ValueError):
            eh.exact_subgraphs(bad, 5, ei)
    with pytest.raises(ValueError):
        eh.exact_subgraphs(links, 5, ei.to(torch.float32))
    with pytest.raises(ValueError):
        eh.exact_subgraphs(links, 5, ei, batch_size=0)
    with pytest.raises(IndexError):
        eh.exact_subgraphs(torch.tensor([[0, 5]]), 5, ei)
    with pytest.raises(IndexError, match='edge_index refers to nodes outside'):
        eh.exact_subgraphs(links, 5, torch.tensor([[0, 1], [1, 5]]))
    eh.max_hops = 4
    with pytest.raises(NotImplementedError):
        eh.exact_subgraphs(links, 5, ei)


@pytest.mark.parametrize('label', ['drnl', 'de', 'de+', 'hop', 'zo', None])
def test_python_empty_link_list_needs_no_device(label):
    sg = _eh(3).exact_subgraphs(torch.zeros((0, 2), dtype=torch.long), 5, torch.tensor([[0], [1]]), node_label=label, return_info=True)
    assert sg.rowptr.tolist() == [0] and sg.adj_ptr.tolist() == [0] and sg.ids.shape == (0,) and sg.dist.shape == (0, 2)
    assert sg.roots.shape == (0, 2) and sg.roots.dtype == torch.int32 and sg.nbr.shape == sg.weight.shape == (0,)
    assert sg.nbr.dtype == sg.weight.dtype == torch.int32 and sg.adj_ptr.dtype == torch.int64
    if label is None:
        assert sg.z is None
    else:
        assert sg.z.dtype == torch.int64 and sg.z.shape == ((0, 2) if label in ('de', 'de+') else (0,))
    assert sg.edge_index().shape == (2, 0) and sg.batch().shape == (0,) and sg.info['truncated'].shape == (0,)
