"""CPU tests of what tests/test_large_exact_gpu.py trusts (tests/large_exact_helpers.py): the closed forms of the clique batch against
subgraph_restatement on a scaled-down copy, the boundary arithmetic of both shapes against the built library and the kernel source, and
the host-side restriction of the arena graph to the neighbourhood of the restated links against the restatements on the whole graph.
If a constant of the library moves, the arithmetic tests say which shape to resize."""
import os
import re

import numpy as np
import torch

import exact_nodes_restatement as nr
import exact_restatement as er
import large_exact_helpers as lx
import masked_restatement as mr
import sampled_subgraph_restatement as ssr
import subgraph_restatement as sr
from conftest import REPO

CPU = torch.device('cpu')


# ---- Part B: the closed forms ---------------------------------------------------------------------------------------------------------
def _small_clique():
    """the clique on 32 of 64 nodes with the (a + b) % 7 duplication and six links: a negative id (row 0), a reversed pair (row 1),
    u == v (row 2)"""
    n, lo, hi = 64, 16, 48
    _, ei = lx.clique_graph(CPU, n, lo, hi)
    links = lx.clique_links(CPU, 6, n, lo, hi, self_rows=(2,))
    return n, lo, hi, ei, links


def test_clique_closed_forms_equal_the_restatement():
    n, lo, hi, ei, links = _small_clique()
    lk = links.numpy()
    assert (lk < 0).any() and lk[2, 0] - lk[2, 1] in (0, n, -n)
    w = np.where(lk < 0, lk + n, lk)
    assert (w[:, 0] < w[:, 1]).any() and (w[:, 0] > w[:, 1]).any() and len({tuple(r) for r in w.tolist()}) == len(w)
    pairs = ei.numpy().T.tolist()
    assert max(pairs.count(p) for p in pairs[:200]) == 2 and min(pairs.count(p) for p in pairs[:200]) == 1  # both weights occur
    want = sr.restate(n, ei.numpy(), lk, 1, mask_target=True)
    x = lx.clique_expected(links, n, lo, hi)
    for name in ('rowptr', 'ids', 'dist', 'roots', 'adj_ptr'):
        np.testing.assert_array_equal(getattr(x, name).numpy(), getattr(want, name), err_msg=name)
    np.testing.assert_array_equal(x.z.numpy(), sr.labels(want, 'drnl'))
    assert x.A == want.adj_ptr[-1] == want.nbr.size == int(x.lengths.sum()) and x.row_start[-1] == x.A
    nbr, weight = [], []
    for q0 in range(0, len(lk), 4):  # in chunks, a full one and a short one, as the GPU test walks them
        a, b = lx.clique_expected_arcs(x, q0, min(q0 + 4, len(lk)), lo)
        assert a.dtype == b.dtype == torch.int32
        nbr.append(a.numpy())
        weight.append(b.numpy())
    np.testing.assert_array_equal(np.concatenate(nbr), want.nbr)
    np.testing.assert_array_equal(np.concatenate(weight), want.weight)
    assert set(want.weight.tolist()) == {1, 2}


def test_clique_links_of_the_large_batch():
    """520 links: 518 distinct pairs with u != v inside the clique, both orders, negative ids, and the two u == v rows"""
    n, lo, hi = lx.CLIQUE_N, lx.CLIQUE_LO, lx.CLIQUE_HI
    lk = lx.clique_links(CPU).numpy()
    assert lk.shape == (lx.CLIQUE_LINKS, 2) and (lk < 0).any() and (lk >= 0).any()
    w = np.where(lk < 0, lk + n, lk)
    assert w.min() >= lo and w.max() < hi
    same = np.nonzero(w[:, 0] == w[:, 1])[0]
    assert tuple(same) == lx.CLIQUE_SELF
    rest = np.delete(w, same, axis=0)
    assert len({tuple(r) for r in rest.tolist()}) == len(rest) == 518
    assert (rest[:, 0] < rest[:, 1]).sum() > 100 and (rest[:, 0] > rest[:, 1]).sum() > 100


# ---- the boundary arithmetic -------------------------------------------------------------------------------------------------------------
def test_arena_boundary_arithmetic():
    import subgraph_sketching_amd as ssa
    n, slots = lx.ARENA_N, lx.ARENA_SLOTS
    assert n == 4456448 and lx.slot_words(n) == 10027008
    assert ssa._native.lib().ss_exact_slot_bytes(n) == 4 * lx.slot_words(n) == 40108032
    for m in (1, 2, 3, 4, 5, 4101, 50000, n - 1, n + 1):  # the Python restatement of exact_slot_words, against the library
        assert ssa._native.lib().ss_exact_slot_bytes(m) == 4 * lx.slot_words(m), m
    assert slots * 4 * lx.slot_words(n) == 10267656192
    assert lx.first_slot_at_or_beyond(n, 1 << 31) == 215      # slots 215 .. 255 lie wholly beyond uint32 word 2^31
    assert lx.first_slot_at_or_beyond(n, 1 << 30) == 108      # slots 108 .. 255 beyond byte 2^32
    assert slots * lx.slot_words(n) > (1 << 31) + 16 * lx.slot_words(n)
    assert 215 * lx.slot_words(n) >= 1 << 31 > 214 * lx.slot_words(n)
    assert lx.ARENA_LINKS == 16 * slots and lx.dist_words(n) == 1114112
    # the star: 300 leaves, 600 in-arcs at the hub, above the degree from which the whole workgroup walks a frontier node
    src = open(os.path.join(REPO, 'subgraph-sketching_amd', 'csrc', 'ss_exact_bfs.hpp')).read()
    assert int(re.search(r'constexpr int kBigDegree = (\d+);', src).group(1)) == lx.BIG_DEGREE < 2 * lx.STAR_LEAVES
    assert lx.arena_needs() > 4 * slots * 4 * lx.slot_words(n)


def test_arc_boundary_arithmetic():
    x = lx.clique_expected(lx.clique_links(CPU))
    K, L = 2048, lx.CLIQUE_LINKS
    assert x.K == K and x.A == L * K * (K - 1) - 2 * 518 == 2179972084
    assert x.A > (1 << 31) + (1 << 24)
    assert lx.row_in_which(x, 1 << 31) == 512                 # 2^31 / 4 192 254 = 512.25
    assert x.row_start[512] < 1 << 31 < x.row_start[513]
    assert sum(s >= 1 << 31 for s in x.row_start[:-1]) == 7 >= 5
    assert 512 < lx.CLIQUE_SELF[1] < L and lx.CLIQUE_SELF[0] < 512
    assert int(x.adj_ptr[-1]) == x.A and x.adj_ptr.numel() == L * K + 1
    assert 8 * x.A == 17439776672                             # nbr + weight
    assert L % lx.CHUNK_ROWS != 0                             # the chunk walk ends on a short chunk


# ---- Part A: the graph, the links and the host-side restriction ---------------------------------------------------------------------------
def test_neighbourhood_restatements_equal_the_whole_graph():
    """a 3 000-node copy of the arena graph: restating the first links on their 2-hop neighbourhood (renumbered) gives what restating
    them on the whole graph gives, for the counts (masked or not), the node rows (masked or not) and the sampled rows"""
    n, h = 3000, lx.ARENA_H
    g = lx.arena_graph(CPU, n, seed=5)
    ei = g.ei.numpy()
    assert np.bincount(ei[1], minlength=n)[g.hub] >= 2 * lx.STAR_LEAVES > lx.BIG_DEGREE
    assert np.array_equal(np.sort(ei[0] * n + ei[1]), np.sort(ei[1] * n + ei[0]))  # symmetric, copies included
    links = lx.arena_links(g, 512, seed=6)
    lk = links.numpy()
    w = np.where(lk < 0, lk + n, lk)
    assert lk.min() >= -n and (lk < 0).any() and (w[:, 0] == w[:, 1]).any() and (w == g.hub).any() and (w >= n - n // 4).any()
    first = links[:96]
    nb = lx.neighbourhood(g, first, h)
    assert nb.small_n < n and np.array_equal(nb.nodes[nb.small_links], w[:96])
    for mask in (False, True):
        f, I, balls = lx.restate_features(nb, h, mask)
        if mask:  # tests/test_masked_gpu.py::_scipy_on_g_uv on the whole graph
            loops = np.arange(mr.n_self_of(ei))
            outs = [er.restate(n, np.concatenate([mr.without_link(ei, u, v), np.stack([loops, loops])], axis=1), np.array([[u, v]]), h)
                    for u, v in w[:96].tolist()]
            wf, wI, wb = [np.concatenate([o[i] for o in outs]) for i in range(3)]
        else:
            wf, wI, wb = er.restate(n, ei, w[:96], h)
        assert np.array_equal(I, wI) and np.array_equal(balls, wb) and np.array_equal(f.view(np.int32), wf.view(np.int32))
        for got, want in zip(lx.restate_nodes(nb, h, mask), nr.restate(n, ei, w[:96], h, mask_target=mask, directed=True)):
            np.testing.assert_array_equal(got, want)
    want = ssr.restate_nodes(n, ei, w[:96], h, cap=lx.SAMPLED['max_nodes_per_hop'], ratio=lx.SAMPLED['ratio_per_hop'], seed=lx.SAMPLED['seed'])
    for got, wnt in zip(lx.restate_sampled(nb, h), want):
        np.testing.assert_array_equal(got, wnt)
    assert (np.diff(want[0]) < np.diff(nr.restate(n, ei, w[:96], h)[0])).any()  # the caps drop something
