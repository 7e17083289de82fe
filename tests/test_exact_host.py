"""Exact subgraph features without a GPU: the scipy restatement (tests/exact_restatement.py) against BFS distances and set regions,
the C-ABI argument checks of ss_exact_pairs / ss_exact_large (they return before any launch) and the Python argument errors of
ElphHashes.exact_subgraph_features (raised before the compute device is touched)."""
from argparse import Namespace
from ctypes import byref, c_void_p

import networkx as nx
import numpy as np
import pytest
import torch

import exact_restatement as er
from conftest import load_golden


def _random_graph(rng, n, e, directed, dup, loops, trailing):
    """edge_index [2, E] over nodes [0, n - trailing) (the last `trailing` nodes isolated)"""
    m = n - trailing
    ei = rng.randint(0, m, size=(2, e)).astype(np.int64)
    if not directed:
        ei = np.concatenate([ei, ei[::-1]], axis=1)
    if dup:
        ei = np.concatenate([ei, ei[:, : e // 3]], axis=1)
    if loops:
        x = rng.randint(0, m, size=5)
        ei = np.concatenate([ei, np.stack([x, x])], axis=1)
    return ei


def _nx_counts(n, ei, links, h):
    """I and balls from networkx BFS distances over the reversed edges of G' (B_k(x) = nodes within k in-edge hops of x, for x
    below n_self; empty for k >= 1 otherwise)"""
    n_self = int(ei.max()) + 1 if ei.size else 0
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(ei[1].tolist(), ei[0].tolist()))  # x -> j for every edge j -> x: BFS from x walks in-edges
    def ball(x, k):
        if x >= n_self:
            return set()
        return set(nx.single_source_shortest_path_length(g, x, cutoff=k))
    I = np.zeros((len(links), h, h), dtype=np.int64)
    balls = np.zeros((len(links), 2, h), dtype=np.int64)
    for i, (u, v) in enumerate(links):
        u, v = int(u) % n, int(v) % n
        for k1 in range(h):
            bu = ball(u, k1 + 1)
            balls[i, 0, k1] = len(bu)
            balls[i, 1, k1] = len(ball(v, k1 + 1))
            for k2 in range(h):
                I[i, k1, k2] = len(bu & ball(v, k2 + 1))
    return I, balls


@pytest.mark.parametrize('directed,dup,loops,trailing', [(False, False, False, 0), (True, False, False, 0), (False, True, True, 0),
                                                         (True, True, True, 3), (False, False, False, 4)])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_restatement_matches_networkx_bfs(h, directed, dup, loops, trailing):
    rng = np.random.RandomState(11 * h + 3 * directed + 2 * dup + trailing)
    n = 60
    ei = _random_graph(rng, n, 90, directed, dup, loops, trailing)
    links = np.concatenate([rng.randint(0, n, size=(40, 2)), [[0, 0], [n - 1, 0], [-1, -2], [5, 5]]]).astype(np.int64)
    I, balls = er.counts(n, ei, links, h)
    nI, nballs = _nx_counts(n, ei, links, h)
    np.testing.assert_array_equal(I, nI)
    np.testing.assert_array_equal(balls, nballs)
    if trailing:
        n_self = int(ei.max()) + 1
        assert n_self <= n - trailing
        tail = (links % n) >= n_self
        assert not balls[:, 0][tail[:, 0]].any() and not balls[:, 1][tail[:, 1]].any()


def test_restatement_empty_graph():
    I, balls = er.counts(5, np.zeros((2, 0), dtype=np.int64), [[0, 1], [4, 4]], 2)
    assert not I.any() and not balls.any()


def _set_regions_h2(nbrs, u, v):
    """true sizes of the LABEL_LOOKUP[2] regions from neighbour sets (the `ball` walk of test_reference_suite_port.py)"""
    def ball(fringe):
        out = set(fringe)
        for x in fringe:
            out |= nbrs[x]
        return out
    u1, v1 = ball({u}), ball({v})
    u2, v2 = ball(u1), ball(v1)
    r11 = u1 & v1
    r21 = (u2 & v1) - r11
    r12 = (u1 & v2) - r11
    r22 = (u2 & v2) - (r11 | r21 | r12)
    return [len(r11), len(r21), len(r12), len(r22), len(v1 - u2), len(u1 - v2), len((v2 - v1) - u2), len((u2 - u1) - v2)]


def test_restated_features_equal_set_regions_ba40():
    """h = 2, use_zero_one: columns 0-6 are the sizes of the (d_u, d_v) regions; column 7 keeps the reference's quirk (f0 subtracted
    twice, hashing.py:287) and is checked against that formula instead"""
    g = load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), g['edge_index']
    nbrs = [set() for _ in range(n)]
    for s, d in ei.T.tolist():
        nbrs[s].add(d)
    links = np.array([(u, v) for u in range(n) for v in range(n)], dtype=np.int64)
    feats, I, balls = er.restate(n, ei, links, 2, use_zero_one=True)
    want = np.array([_set_regions_h2(nbrs, u, v) for u, v in links], dtype=np.float32)
    np.testing.assert_array_equal(feats[:, :7], want[:, :7])
    np.testing.assert_array_equal(feats[:, 7], want[:, 7] - feats[:, 0])


def test_restated_features_flags():
    rng = np.random.RandomState(2)
    ei = _random_graph(rng, 50, 80, False, False, False, 0)
    links = rng.randint(0, 50, size=(30, 2))
    for h in (1, 2, 3):
        I, balls = er.counts(50, ei, links, h)
        base = er.features(I, balls, True, False)
        no01 = er.features(I, balls, False, False)
        zero = {1: [], 2: [4, 5], 3: [4, 5, 11, 12]}[h]
        keep = [c for c in range(h * (h + 2)) if c not in zero]
        assert not no01[:, zero].any()
        np.testing.assert_array_equal(no01[:, keep], base[:, keep])
        np.testing.assert_array_equal(er.features(I, balls, True, True), np.maximum(base, 0))


# ---- C ABI without a GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import subgraph_sketching_amd as ssa
    return ssa._native.lib()


def _graph(N):
    import subgraph_sketching_amd as ssa
    return ssa._native.CsrGraphStruct(rowptr=0x1000, col=0x2000, num_nodes=N, n_self_loops=0, n_self_loops_dev=None)


def test_cabi_sizes(lib):
    assert lib.ss_exact_workspace_bytes(-1) == 0 and lib.ss_exact_workspace_bytes(1 << 31) == 0
    assert lib.ss_exact_workspace_bytes(0) >= 16 and lib.ss_exact_workspace_bytes(1000) >= 16 + 4 * 1000
    assert lib.ss_exact_slot_bytes(0) == 0 and lib.ss_exact_slot_bytes(-5) == 0 and lib.ss_exact_slot_bytes(1 << 31) == 0
    N = 2_927_963  # ogbl-citation2: N distance bytes + 2N int32 visit lists
    assert 9 * N <= lib.ss_exact_slot_bytes(N) <= 9 * N + 64


def test_cabi_argument_errors(lib):
    g, N = _graph(100), 100
    p = c_void_p(0x3000)
    ws = lib.ss_exact_workspace_bytes(10)
    pairs = lambda graph, links, B, n, h, feats=p, wsb=ws, lim=2048: lib.ss_exact_pairs(
        graph, links, B, n, h, 0, lim, None, None, feats, None, p, wsb, None)
    large = lambda graph, links, B, n, h, slots=4, arena=p, ab=1 << 30: lib.ss_exact_large(
        graph, links, B, n, h, 0, None, None, p, p, ws, slots, arena, ab, None)
    for fn in (pairs, large):
        assert fn(byref(g), p, 10, N, 4) == -4
        assert fn(byref(g), p, 10, N, 0) == -4
        assert fn(byref(g), p, -1, N, 2) == -1
        assert fn(byref(g), p, 10, -1, 2) == -1
        assert fn(byref(g), None, 0, N, 2) == 0   # B == 0: nothing to do, no launch
        assert fn(None, p, 10, N, 2) == -1
        assert fn(byref(g), None, 10, N, 2) == -1
        assert fn(byref(g), p, 10, N + 1, 2) == -1  # graph->num_nodes != N
    assert pairs(byref(g), p, 10, N, 2, feats=None) == -1
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
        eh.exact_subgraph_features(links, 5, ei)
    eh.max_hops = 2
    for bad in (torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2, 2), dtype=torch.long), torch.zeros((3,), dtype=torch.long),
                torch.zeros((2, 2), dtype=torch.float32), torch.zeros((2, 2), dtype=torch.bool)):
        with pytest.raises(ValueError):
            eh.exact_subgraph_features(bad, 5, ei)
    for bad in (torch.zeros((3, 3), dtype=torch.long), torch.zeros((2,), dtype=torch.long), torch.zeros((2, 3)),):
        with pytest.raises(ValueError):
            eh.exact_subgraph_features(links, 5, bad)
    with pytest.raises(ValueError):
        eh.exact_subgraph_features(links, 5, ei, batch_size=0)
    with pytest.raises(ValueError):
        eh.exact_subgraph_features(links, -1, ei)
    for bad in ([[0, 5]], [[-6, 0]], [[0, 1], [7, 0]]):
        with pytest.raises(IndexError):
            eh.exact_subgraph_features(torch.tensor(bad), 5, ei)
    with pytest.raises(IndexError, match='edge_index refers to nodes outside'):
        eh.exact_subgraph_features(links, 5, torch.tensor([[0, 1], [1, 5]]))
    with pytest.raises(IndexError, match='edge_index refers to nodes outside'):
        eh.exact_subgraph_features(links, 5, torch.tensor([[0, -1], [1, 2]]))


def test_python_empty_link_list_needs_no_device():
    eh = _eh(3)
    f = eh.exact_subgraph_features(torch.zeros((0, 2), dtype=torch.long), 5, torch.tensor([[0], [1]]))
    assert f.shape == (0, 15) and f.dtype == torch.float32
    f, I, balls = eh.exact_subgraph_features(torch.zeros((0, 2), dtype=torch.long), 5, torch.tensor([[0], [1]]), return_counts=True)
    assert I.shape == (0, 3, 3) and balls.shape == (0, 2, 3) and I.dtype == balls.dtype == torch.int32
