"""Per-hop sampled enclosing subgraphs without a GPU: the Python-set restatement (tests/sampled_subgraph_restatement.py) against what the
reference's own k_hop_subgraph returned with sampling off (tests/golden/g18_seal_khop.npz) and against the exact node lists'
restatement, the properties of the walk (a rejected node stays visited, floor(ratio * F), m == 0 ends it, u == v, directed graphs,
multigraphs, negative ids), the sampling law on a star, and every argument error of ElphHashes.sampled_subgraph_nodes /
exact_subgraphs(max_nodes_per_hop=, ratio_per_hop=, seed=) and of ss_sampled_nodes_pairs / ss_sampled_nodes_large (before any launch)."""
from argparse import Namespace
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import exact_nodes_restatement as nr
import sampled_subgraph_restatement as ssr
from conftest import load_golden
from test_exact_nodes_host import _ba40, _uniform300


def k8_with_tails():
    """K_8 on 0 .. 7; node i carries the path i - (8 + 3i) - (9 + 3i) - (10 + 3i); symmetric"""
    a, b = np.nonzero(~np.eye(8, dtype=bool))
    tails = [(i, 8 + 3 * i) for i in range(8)] + [(8 + 3 * i + k, 9 + 3 * i + k) for i in range(8) for k in range(2)]
    t = np.array(tails + [(y, x) for x, y in tails]).T
    return 32, np.concatenate([np.stack([a, b]), t], axis=1).astype(np.int64)


def star(leaves=64, links=4000):
    """hub 0, leaves 1 .. 64, then `links` isolated nodes w: the links (hub, w) all see the same fringe under keys of their own"""
    leaf = np.arange(1, leaves + 1)
    ei = np.stack([np.concatenate([np.zeros_like(leaf), leaf]), np.concatenate([leaf, np.zeros_like(leaf)])]).astype(np.int64)
    w = np.arange(leaves + 1, leaves + 1 + links)
    return leaves + 1 + links, ei, np.stack([np.zeros_like(w), w], axis=1).astype(np.int64)


STAR_SEED = 2024


# ---- against the reference and the exact node lists -----------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [1, 2, 3])
def test_unsampled_walk_equals_the_reference(h):
    g18, g = load_golden('g18_seal_khop.npz'), load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    np.testing.assert_array_equal(g18['links'], g['links'])
    rowptr, ids, hop = ssr.restate_nodes(n, ei, g18['links'], h)
    np.testing.assert_array_equal(rowptr, g18[f'h{h}_rowptr'])
    np.testing.assert_array_equal(ids, g18[f'h{h}_ids'])
    np.testing.assert_array_equal(hop, g18[f'h{h}_hop'])


@pytest.mark.parametrize('graph', ['ba40', 'uniform300', 'directed300'])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_a_cap_that_never_bites_gives_the_exact_node_list(graph, h):
    n, ei, links = _ba40() if graph == 'ba40' else _uniform300(directed=graph == 'directed300')
    want = nr.restate(n, ei, links, h, mask_target=False, directed=True)
    for cap in (None, n):
        got = ssr.restate_nodes(n, ei, links, h, cap=cap, seed=5, return_info=True)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2].min(axis=1))
        assert got[3]['sampled_links'] == 0


# ---- properties of the walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [2, 3])
def test_a_rejected_node_stays_visited(h):
    n, ei = k8_with_tails()
    links = np.array([[0, 1], [2, 7], [3, 3], [0, 8]])
    nb = ssr.in_neighbours(n, ei)
    late = 0
    for seed in range(8):
        rowptr, ids, hop = ssr.restate_nodes(n, ei, links, h, cap=2, seed=seed)
        for (u, v), (row, hops) in zip(links.tolist(), ssr.rows(rowptr, ids, hop)):
            assert len(row) <= 2 + 2 * h and set(hops[np.isin(row, [u, v])].tolist()) == {0}
            for x, d in zip(row.tolist(), hops.tolist()):
                if d >= 2:  # a neighbour of a root was in the hop-1 fringe: kept then, or rejected for good
                    assert u not in nb[x] and v not in nb[x]
                    late += 1
    assert late > 0


def test_floor_of_ratio_times_fringe_and_an_empty_hop_ends_the_walk():
    n, ei, _ = star(leaves=7, links=1)  # hub 0, leaves 1 .. 7, node 8 isolated
    chain = np.array([[1, 9, 10], [9, 10, 11]])  # leaf 1 - 9 - 10 - 11
    ei = np.concatenate([ei, chain, chain[::-1]], axis=1)
    nb = ssr.in_neighbours(12, ei)
    for ratio, cap, m in ((1.0, None, 7), (0.5, None, 3), (0.3, None, 2), (0.29, None, 2), (0.28, None, 1), (0.14, None, 0), (0.999, None, 6),
                          (0.5, 2, 2), (0.5, 5, 3), (1.0, 1, 1)):
        fr = []
        hop_of = ssr.walk(nb, 0, 8, 3, cap, ratio, 11, fr)
        want = 7 if ratio == 1.0 else int(ratio * 7)
        assert m == (want if cap is None else min(want, cap)) and fr[0] == (7, m)
        assert sum(d == 1 for d in hop_of.values()) == m
        if m == 0:
            assert len(fr) == 1 and set(hop_of) == {0, 8}  # the walk ended: nothing at hop 2
    # (0.57 * 7 = 3.9899999999999998: the product is taken in double and truncated)
    fr = []
    ssr.walk(nb, 0, 8, 1, None, 0.57, 0, fr)
    assert fr == [(7, int(0.57 * 7))] and int(0.57 * 7) == 3
    # a hop whose fringe is empty ends the walk as well
    fr = []
    assert set(ssr.walk(nb, 8, 8, 3, None, 1.0, 0, fr)) == {8} and fr == [(0, 0)]


def test_equal_roots_directed_multigraph_and_negative_ids():
    n, ei, links = _uniform300(directed=True)  # (holds duplicate arcs and self loops; links with u == v and negative ids)
    clean = np.unique(ei[:, ei[0] != ei[1]], axis=1)
    assert clean.shape[1] < ei.shape[1]
    wrapped = np.where(links < 0, links + n, links)
    assert (links < 0).any() and (wrapped[:, 0] == wrapped[:, 1]).any()
    for h, cap, ratio in ((2, 3, 1.0), (3, None, 0.5), (3, 2, 0.7)):
        got = ssr.restate_nodes(n, ei, links, h, cap=cap, ratio=ratio, seed=9)
        for other in (ssr.restate_nodes(n, clean, links, h, cap=cap, ratio=ratio, seed=9),     # repeated arcs and loops change nothing
                      ssr.restate_nodes(n, ei, wrapped, h, cap=cap, ratio=ratio, seed=9)):     # a negative id is the node it wraps to
            for a, b in zip(got, other):
                np.testing.assert_array_equal(a, b)
        for (u, v), (row, hops) in zip(wrapped.tolist(), ssr.rows(*got)):
            assert (np.diff(row) > 0).all() and (hops[np.isin(row, [u, v])] == 0).all() and (hops == 0).sum() == len({u, v})
    # in-arcs are what is walked: on the arc 0 -> 1 alone, 1 reaches 0 and 0 reaches nothing
    one = np.array([[0], [1]])
    assert ssr.restate_nodes(3, one, [[1, 2]], 1)[1].tolist() == [0, 1, 2] and ssr.restate_nodes(3, one, [[0, 2]], 1)[1].tolist() == [0, 2]


def test_full_restatement_masks_the_target_link_in_the_adjacency_only():
    n, ei, links = _ba40()
    for mask in (False, True):
        sub = ssr.restate(n, ei, links, 2, mask_target=mask, cap=3, seed=1)
        np.testing.assert_array_equal(sub.ids, ssr.restate_nodes(n, ei, links, 2, cap=3, seed=1)[1])  # the walk keeps the target link
        ids, ptr, nbr, weight = sub.row(0)  # (links[0] is an edge)
        ru, rv = sub.roots[0]
        assert (rv in nbr[ptr[ru]:ptr[ru + 1]]) == (not mask)
        assert ssr.labels(sub, 'hop').tolist() == sub.hop.tolist() and ssr.labels(sub, 'drnl').shape == sub.ids.shape


# ---- the sampling law -----------------------------------------------------------------------------------------------------------------
def _within_five_sigma(counts, trials, p):
    sigma = np.sqrt(trials * p * (1 - p))
    return np.abs(counts - trials * p).max() <= 5 * sigma


def test_sampling_law_on_a_star():
    n, ei, links = star()
    rowptr, ids, hop = ssr.restate_nodes(n, ei, links, 1, cap=8, seed=STAR_SEED)
    assert (np.diff(rowptr) == 10).all()
    leaves = ids[hop == 1]
    assert leaves.min() >= 1 and leaves.max() <= 64
    assert _within_five_sigma(np.bincount(leaves, minlength=65)[1:], 4000, 1 / 8)
    rowptr, ids, hop = ssr.restate_nodes(n, ei, links, 1, ratio=0.25, seed=STAR_SEED)
    assert (np.diff(rowptr) == 18).all()  # exactly 16 leaves in every row
    assert _within_five_sigma(np.bincount(ids[hop == 1], minlength=65)[1:], 4000, 1 / 4)


# ---- argument errors before any launch ------------------------------------------------------------------------------------------------
def _eh(h=2):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))


@pytest.mark.parametrize('method', ['sampled_subgraph_nodes', 'exact_subgraphs'])
def test_python_argument_errors(method):
    eh = _eh()
    call = getattr(eh, method)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    links = torch.tensor([[0, 1], [2, 3]])
    for bad in (0, -1, 2.0, 2.5, True, 'many'):
        with pytest.raises(ValueError, match='max_nodes_per_hop'):
            call(links, 5, ei, max_nodes_per_hop=bad)
    for bad in (0, 0.0, -0.5, 1.5, 2, float('nan'), float('inf'), True, '0.5', None):
        with pytest.raises(ValueError, match='ratio_per_hop'):
            call(links, 5, ei, ratio_per_hop=bad)
    for bad in (-1, 1 << 63, 0.5, 1.0, True, None):
        with pytest.raises(ValueError, match='seed'):
            call(links, 5, ei, max_nodes_per_hop=2, seed=bad)
    # everything else goes through exact.check_arguments
    eh.max_hops = 4
    with pytest.raises(NotImplementedError):
        call(links, 5, ei, max_nodes_per_hop=2)
    eh.max_hops = 2
    for bad in (torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 2), dtype=torch.float32)):
        with pytest.raises(ValueError):
            call(bad, 5, ei, max_nodes_per_hop=2)
    with pytest.raises(IndexError):
        call(torch.tensor([[0, 5]]), 5, ei, ratio_per_hop=0.5)
    with pytest.raises(IndexError, match='edge_index refers to nodes outside'):
        call(links, 5, torch.tensor([[0, 1], [1, 5]]), ratio_per_hop=0.5)
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match='max_nodes'):
            call(links, 5, ei, max_nodes_per_hop=2, max_nodes=bad)
    with pytest.raises(ValueError, match='batch_size'):
        call(links, 5, ei, max_nodes_per_hop=2, batch_size=0)


def test_exact_subgraphs_takes_the_sampling_arguments_by_keyword_only():
    eh = _eh()
    with pytest.raises(TypeError):
        eh.exact_subgraphs(torch.zeros((0, 2), dtype=torch.long), 5, torch.tensor([[0], [1]]), 11000000, True, None, 'drnl', 1000, False, 2)


def test_python_empty_link_list_needs_no_device():
    import subgraph_sketching_amd as ssa
    eh = _eh(3)
    none, ei = torch.zeros((0, 2), dtype=torch.long), torch.tensor([[0], [1]])
    rowptr, ids, hop, info = eh.sampled_subgraph_nodes(none, 5, ei, max_nodes_per_hop=3, ratio_per_hop=0.5, seed=7, return_info=True)
    assert rowptr.tolist() == [0] and rowptr.dtype == ids.dtype == torch.int64 and ids.shape == hop.shape == (0,) and hop.dtype == torch.uint8
    assert info['truncated'].shape == (0,) and info['lds_links'] == info['large_links'] == info['sampled_links'] == 0
    assert len(eh.sampled_subgraph_nodes(none, 5, ei)) == 3
    sg = eh.exact_subgraphs(none, 5, ei, max_nodes_per_hop=3, node_label='de', return_info=True)
    assert type(sg) is ssa.subgraphs.SampledSubgraphs and isinstance(sg, ssa.subgraphs.ExactSubgraphs)
    assert sg.dist is None and sg.hop.shape == (0,) and sg.z.shape == (0, 2) and sg.roots.shape == (0, 2) and sg.adj_ptr.tolist() == [0]
    assert sg.info['sampled_links'] == 0 and sg.num_links == 0 and sg.edge_index().shape == (2, 0)
    assert type(sg.to('cpu')) is ssa.subgraphs.SampledSubgraphs
    plain = eh.exact_subgraphs(none, 5, ei)  # the defaults: today's type and fields
    assert type(plain) is ssa.subgraphs.ExactSubgraphs and plain.dist.shape == (0, 2) and not hasattr(plain, 'hop')


def test_cabi_argument_errors():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    N = 100
    g = ssa._native.CsrGraphStruct(rowptr=0x1000, col=0x2000, num_nodes=N, n_self_loops=0, n_self_loops_dev=None)
    p = c_void_p(0x3000)  # never dereferenced: every call below is answered by the host-side checks
    ws = lib.ss_exact_workspace_bytes(10)

    def pairs(graph, links, B, n, h, cap=3, ratio=0.5, seed=1, counts=p, state=p, rowptr=None, ids=None, hop=None, wsb=ws, lim=2048):
        return lib.ss_sampled_nodes_pairs(graph, links, B, n, h, cap, ratio, seed, lim, counts, state, rowptr, ids, hop, None, p, wsb, None)

    def large(graph, links, B, n, h, cap=3, ratio=0.5, seed=1, counts=p, state=p, rowptr=None, ids=None, hop=None, slots=4, arena=p, ab=1 << 30):
        return lib.ss_sampled_nodes_large(graph, links, B, n, h, cap, ratio, seed, counts, state, rowptr, ids, hop, p, ws, slots, arena, ab, None)

    for fn in (pairs, large):
        assert fn(byref(g), p, 10, N, 4) == -4
        assert fn(byref(g), p, 10, N, 0) == -4
        assert fn(byref(g), p, -1, N, 2) == -1
        assert fn(byref(g), p, 10, -1, 2) == -1
        assert fn(byref(g), None, 0, N, 2) == 0   # B == 0: nothing to do, no launch
        assert fn(byref(g), None, 0, N, 2, cap=0, ratio=1.0, seed=(1 << 63) - 1) == 0   # no cap, the whole fringe, the largest seed
        for bad in (dict(cap=-1), dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.0000001), dict(ratio=float('nan')), dict(seed=1 << 63)):
            assert fn(byref(g), p, 10, N, 2, **bad) == -1 and fn(byref(g), None, 0, N, 2, **bad) == -1   # (checked before B == 0)
        assert fn(None, p, 10, N, 2) == -1
        assert fn(byref(g), None, 10, N, 2) == -1
        assert fn(byref(g), p, 10, N + 1, 2) == -1  # graph->num_nodes != N
        assert fn(byref(g), p, 10, N, 2, counts=None) == -1            # count pass without counts
        assert fn(byref(g), p, 10, N, 2, state=None) == -1
        assert fn(byref(g), p, 10, N, 2, rowptr=p, ids=None, hop=p) == -1  # fill pass without ids
        assert fn(byref(g), p, 10, N, 2, rowptr=p, ids=p, hop=None) == -1
        assert fn(byref(g), p, 10, N, 2, rowptr=p, ids=p, hop=p, state=None) == -1
    assert pairs(byref(g), p, 10, N, 2, wsb=ws - 1) == -3
    assert pairs(byref(g), p, 10, N, 2, lim=-1) == -1
    assert large(byref(g), p, 10, N, 2, slots=0) == -1
    assert large(byref(g), p, 10, N, 2, arena=None) == -1
    assert large(byref(g), p, 10, N, 2, ab=lib.ss_exact_slot_bytes(N) * 4 - 1) == -3
