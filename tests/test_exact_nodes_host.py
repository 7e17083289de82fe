"""Exact subgraph node lists without a GPU: the scipy restatement (tests/exact_nodes_restatement.py) against the restatement of the
exact counts (tests/exact_restatement.py) -- the counts are histograms of the distance pairs --, the C-ABI argument checks of
ss_exact_nodes_pairs / ss_exact_nodes_large (they return before any launch) and the Python argument errors of
ElphHashes.exact_subgraph_nodes (raised before the compute device is touched)."""
from argparse import Namespace
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import exact_nodes_restatement as nr
import exact_restatement as er
from conftest import load_golden


def _ba40():
    """the committed 40-node BA graph with two more, isolated nodes (40, 41: at or above max(edge_index) + 1)"""
    g = load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    keys = set((ei[0] * n + ei[1]).tolist())
    non = next((u, v) for u in range(n) for v in range(u + 1, n) if u * n + v not in keys and v * n + u not in keys)
    links = np.array([ei[:, 0], ei[:, 17], non, [5, 5], [41, 3], [3, 40], [40, 41], [41, 41], [-1 - 2, -42], [int(ei[0, 3]) - 42, ei[1, 3]]],
                     dtype=np.int64)
    return n + 2, ei, links


def _uniform300(directed=False):
    """300 nodes, uniform endpoints, node 7 isolated BELOW max(edge_index) + 1, a few duplicate and self-loop edges"""
    rng = np.random.RandomState(21)
    n = 300
    e = rng.randint(0, n, size=(2, 500)).astype(np.int64)
    e = e[:, (e != 7).all(axis=0)]
    ei = e if directed else np.concatenate([e, e[::-1]], axis=1)
    ei = np.concatenate([ei, ei[:, :40], np.array([[4, 9, 299], [4, 9, 299]])], axis=1)
    links = np.concatenate([ei[:, :30].T, rng.randint(0, n, size=(40, 2)), [[7, 12], [12, 7], [7, 7], [33, 33], [-1, -300], [-293, 5]]])
    return n, ei, links.astype(np.int64)


def _masked_edge_index(ei, u, v):
    """ei without every copy of u -> v and v -> u; a self-loop edge at the largest id keeps max(edge_index) + 1 (it changes nothing else)"""
    own = ((ei[0] == u) & (ei[1] == v)) | ((ei[0] == v) & (ei[1] == u))
    top = int(ei.max())
    return np.concatenate([ei[:, ~own], [[top], [top]]], axis=1)


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('graph', ['ba40', 'uniform300', 'directed300'])
def test_distance_histograms_are_the_exact_counts(graph, h, mask):
    """#{x : d_u <= k1 and d_v <= k2} = I[k1 - 1][k2 - 1], #{x : d_u <= k} and #{x : d_v <= k} = the ball sizes, and the row length =
    the two h-balls minus their intersection.  A root at or above max(edge_index) + 1 has an empty sketch ball but lists itself at
    distance 0: there the histograms hold exactly that one node more"""
    directed = graph == 'directed300'
    n, ei, links = _ba40() if graph == 'ba40' else _uniform300(directed)
    n_self = int(ei.max()) + 1
    rowptr, ids, dist = nr.restate(n, ei, links, h, mask_target=mask, directed=directed)
    assert rowptr.dtype == np.int64 and ids.dtype == np.int64 and dist.dtype == np.uint8 and dist.shape == (ids.size, 2)
    wrapped = np.where(links < 0, links + n, links)
    for q, (x, d) in enumerate(nr.rows(rowptr, ids, dist)):
        u, v = wrapped[q]
        assert (np.diff(x) > 0).all() and d.max() <= h + 1 and (d.min(axis=1) <= h).all()
        assert d[x == u][0][0] == 0 and d[x == v][0][1] == 0
        if u == v:
            assert (d[:, 0] == d[:, 1]).all()
        I, balls = er.counts(n, _masked_edge_index(ei, u, v) if mask else ei, [[u, v]], h)
        extra_u, extra_v = int(u >= n_self), int(v >= n_self)
        for k1 in range(1, h + 1):
            assert (d[:, 0] <= k1).sum() == balls[0, 0, k1 - 1] + extra_u
            assert (d[:, 1] <= k1).sum() == balls[0, 1, k1 - 1] + extra_v
            for k2 in range(1, h + 1):
                assert ((d[:, 0] <= k1) & (d[:, 1] <= k2)).sum() == I[0, k1 - 1, k2 - 1] + (extra_u if u == v else 0)
        union = balls[0, 0, h - 1] + balls[0, 1, h - 1] - I[0, h - 1, h - 1] + extra_u + (extra_v if u != v else 0)
        assert x.size == union


def test_restatement_by_hand():
    # path 0 - 1 - 2 - 3 - 4, node 5 isolated; edges in both directions, one duplicate, one self loop
    ei = np.array([[0, 1, 1, 2, 2, 3, 3, 4, 0, 2], [1, 0, 2, 1, 3, 2, 4, 3, 1, 2]])
    rowptr, ids, dist = nr.restate(6, ei, [[0, 3], [1, 2], [5, 0], [2, 2]], 2)
    np.testing.assert_array_equal(rowptr, [0, 5, 10, 14, 19])
    np.testing.assert_array_equal(ids[:5], [0, 1, 2, 3, 4])
    np.testing.assert_array_equal(dist[:5], [[0, 3], [1, 2], [2, 1], [3, 0], [3, 1]])
    np.testing.assert_array_equal(ids[10:14], [0, 1, 2, 5])
    np.testing.assert_array_equal(dist[10:14], [[3, 0], [3, 1], [3, 2], [0, 3]])
    rowptr, ids, dist = nr.restate(6, ei, [[1, 2]], 2, mask_target=True)  # without 1 - 2: the path falls apart
    np.testing.assert_array_equal(ids, [0, 1, 2, 3, 4])
    np.testing.assert_array_equal(dist, [[1, 3], [0, 3], [3, 0], [3, 1], [3, 2]])
    rowptr, ids, dist = nr.restate(4, np.zeros((2, 0), dtype=np.int64), [[0, 3], [2, 2]], 3)
    np.testing.assert_array_equal(rowptr, [0, 2, 3])
    np.testing.assert_array_equal(ids, [0, 3, 2])
    np.testing.assert_array_equal(dist, [[0, 4], [4, 0], [0, 0]])


# ---- C ABI without a GPU -------------------------------------------------------------------------------------------------------------
def test_cabi_argument_errors():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    N = 100
    g = ssa._native.CsrGraphStruct(rowptr=0x1000, col=0x2000, num_nodes=N, n_self_loops=0, n_self_loops_dev=None)
    p = c_void_p(0x3000)
    ws = lib.ss_exact_workspace_bytes(10)
    pairs = lambda graph, links, B, n, h, counts=p, rowptr=None, ids=None, dist=None, wsb=ws, lim=2048: lib.ss_exact_nodes_pairs(
        graph, links, B, n, h, 0, lim, counts, rowptr, ids, dist, None, p, wsb, None)
    large = lambda graph, links, B, n, h, counts=p, rowptr=None, ids=None, dist=None, slots=4, arena=p, ab=1 << 30: lib.ss_exact_nodes_large(
        graph, links, B, n, h, 0, counts, rowptr, ids, dist, p, ws, slots, arena, ab, None)
    for fn in (pairs, large):
        assert fn(byref(g), p, 10, N, 4) == -4
        assert fn(byref(g), p, 10, N, 0) == -4
        assert fn(byref(g), p, -1, N, 2) == -1
        assert fn(byref(g), p, 10, -1, 2) == -1
        assert fn(byref(g), None, 0, N, 2) == 0   # B == 0: nothing to do, no launch
        assert fn(None, p, 10, N, 2) == -1
        assert fn(byref(g), None, 10, N, 2) == -1
        assert fn(byref(g), p, 10, N + 1, 2) == -1  # graph->num_nodes != N
        assert fn(byref(g), p, 10, N, 2, counts=None) == -1           # count pass without counts
        assert fn(byref(g), p, 10, N, 2, rowptr=p, ids=None, dist=p) == -1  # fill pass without ids
        assert fn(byref(g), p, 10, N, 2, rowptr=p, ids=p, dist=None) == -1
    assert pairs(byref(g), p, 10, N, 2, wsb=ws - 1) == -3
    assert pairs(byref(g), p, 10, N, 2, lim=-1) == -1
    assert large(byref(g), p, 10, N, 2, slots=0) == -1
    assert large(byref(g), p, 10, N, 2, arena=None) == -1
    assert large(byref(g), p, 10, N, 2, ab=lib.ss_exact_slot_bytes(N) * 4 - 1) == -3


# ---- Python argument errors before any launch ---------------------------------------------------------------------------------------
def _eh(h=2):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))


def test_python_argument_errors():
    eh = _eh()
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    links = torch.tensor([[0, 1], [2, 3]])
    eh.max_hops = 4
    with pytest.raises(NotImplementedError):
        eh.exact_subgraph_nodes(links, 5, ei)
    eh.max_hops = 2
    for bad in (torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2, 2), dtype=torch.long), torch.zeros((3,), dtype=torch.long),
                torch.zeros((2, 2), dtype=torch.float32), torch.zeros((2, 2), dtype=torch.bool)):
        with pytest.raises(ValueError):
            eh.exact_subgraph_nodes(bad, 5, ei)                      # a bad links shape / dtype
    for bad in (ei.to(torch.float32), torch.zeros((3, 3), dtype=torch.long), torch.zeros((2,), dtype=torch.long)):
        with pytest.raises(ValueError):
            eh.exact_subgraph_nodes(links, 5, bad)                   # float edge_index, bad shapes
    for bad in ([[0, 5]], [[-6, 0]], [[0, 1], [7, 0]]):
        with pytest.raises(IndexError):
            eh.exact_subgraph_nodes(torch.tensor(bad), 5, ei)        # ids out of range
    with pytest.raises(IndexError, match='edge_index refers to nodes outside'):
        eh.exact_subgraph_nodes(links, 5, torch.tensor([[0, 1], [1, 5]]))
    for bad in (1, 0, None, 'yes', torch.tensor(True)):
        with pytest.raises(ValueError):
            eh.exact_subgraph_nodes(links, 5, ei, mask_target=bad)   # non-bool mask_target
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            eh.exact_subgraph_nodes(links, 5, ei, max_nodes=bad)     # max_nodes < 1 (or no integer)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            eh.exact_subgraph_nodes(links, 5, ei, batch_size=bad)    # batch_size < 1
    with pytest.raises(ValueError):
        eh.exact_subgraph_nodes(links, -1, ei)


def test_python_empty_link_list_needs_no_device():
    eh = _eh(3)
    none = torch.zeros((0, 2), dtype=torch.long)
    rowptr, ids, dist = eh.exact_subgraph_nodes(none, 5, torch.tensor([[0], [1]]))
    assert rowptr.tolist() == [0] and rowptr.dtype == torch.int64
    assert ids.shape == (0,) and ids.dtype == torch.int64 and dist.shape == (0, 2) and dist.dtype == torch.uint8
    rowptr, ids, dist, info = eh.exact_subgraph_nodes(none, 5, torch.tensor([[0], [1]]), max_nodes=3, return_info=True)
    assert info['truncated'].shape == (0,) and info['lds_links'] == 0 and info['large_links'] == 0
