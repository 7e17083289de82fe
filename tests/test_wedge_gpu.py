"""Exact two-hop candidates (csrc/ss_wedge.hip, wedge.py) on the GPU: WedgeGraph.candidates against the numpy
restatement of its semantics (wedge_restatement.py) -- rowptr, ids and common exactly -- through both kernel tiers and across their
boundary, a hub through the large tier, the invariances of a row, max_walks, ids out of range, and topk_links_wedge against the
brute-force composition (score_links over the restated candidate pairs, sorted), bit for bit.

Left out: the agreement with topk_links under a head that scores 0 outside the common-neighbour set.  The head reads sketch ESTIMATES
of the intersections, which are not zero exactly where the exact count is, so no such head is easy to construct.

Run on an MI355X: profiles/wedge_planted_tests.txt."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from negatives_restatement import negatives_graph
from score_restatement import raw_head
import wedge_restatement as restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _ba40():
    g = load_golden('g3_g4_ba40.npz')
    return int(g['num_nodes']), g['edge_index'].astype(np.int64)


def _uniform3000():
    n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
    return n, restated.uniform_graph(n, e_und, seed)


def _uniform200():
    N, ei = _uniform3000()
    return 200, restated.induced(ei, 200)


GRAPHS = {'ba40': _ba40, 'uniform200': _uniform200, 'uniform3000': _uniform3000, 'star': restated.star, 'clique': restated.clique,
          'path': restated.path, 'odd': restated.odd_graph, 'boundary': restated.boundary_graph, 'hub': negatives_graph,
          'star3000': lambda: restated.star(3000)}
# per graph: a degree-0 node, a negative id and a duplicate source are always among them
SOURCES = {'star': [0, 1, 62, 63, -1, -63, 1],                 # the centre, leaves, the isolated node
           'odd': [0, 7, 5, 3, 9, 63, -1, 1, 2, 7, 9 - 64],    # 7: its only walks return to itself; 63: no edge
           'boundary': list(range(8)) + [-1, 4, 4],
           'hub': [382, 0, 5, 149, 398, 388, 383, 399, 360, 3, -18, 382],
           'star3000': [0, 1, 2998, 2999, -1, 1]}


@pytest.fixture(scope='module')
def graphs(ssa, dev):
    """(N, edge_index, WedgeGraph, sources) per graph, built once; every test reads them only"""
    made = {}

    def get(name):
        if name not in made:
            N, ei = GRAPHS[name]()
            src = SOURCES.get(name)
            if src is None:
                deg0 = np.setdiff1d(np.arange(N), np.where(ei[0] < 0, ei[0] + N, ei[0]))
                src = list(np.random.RandomState(11).choice(N, size=min(N, 35), replace=False)) + [0, N - 1, -1, 0] + deg0[:1].tolist()
            made[name] = (N, ei, ssa.WedgeGraph(N, torch.from_numpy(np.ascontiguousarray(ei)).to(dev)), np.array(src, dtype=np.int64))
        return made[name]

    return get


def _assert_same(got, want, where=None):
    rowptr, ids, common = got[:3]
    assert rowptr.dtype == torch.int64 and ids.dtype == torch.int64 and common.dtype == torch.int32
    if where is not None:
        assert rowptr.device == where and ids.device == where and common.device == where
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(ids.cpu().numpy(), want[1])
    np.testing.assert_array_equal(common.cpu().numpy(), want[2])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def _rows(got):
    rowptr, ids, common = (t.cpu().numpy() for t in got[:3])
    return [(ids[a:b], common[a:b]) for a, b in zip(rowptr[:-1], rowptr[1:])]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ba40', 'uniform200', 'uniform3000', 'star', 'clique', 'path', 'odd', 'boundary', 'hub', 'star3000'])
def test_candidates_equal_the_restatement(ssa, dev, graphs, name):
    N, ei, g, src = graphs(name)
    want = restated.candidates(N, ei, src)
    n_walks = restated.walks(N, ei, src)
    assert want[1].size and (n_walks == 0).any() == (name not in ('ba40', 'path', 'uniform3000')), 'a trivial expectation checks nothing'
    sd = torch.from_numpy(src).to(dev)
    for slots in (None, 64, 1):  # the default tier boundary, a low one, everything through the large tier
        rowptr, ids, common, info = g.candidates(sd, return_info=True, _lds_slots=slots)
        _assert_same((rowptr, ids, common), want, dev)
        assert info['skipped_sources'] == want[3] == 0
        assert info['walks'].dtype == torch.int64 and info['walks'].device == dev
        np.testing.assert_array_equal(info['walks'].cpu().numpy(), n_walks)
        large = int((2 * n_walks > (slots or ssa._native.WEDGE_MAX_SLOTS)).sum())
        assert (info['lds_sources'], info['large_sources']) == (int((n_walks > 0).sum()) - large, large)
    two = g.candidates(sd, min_common=2)
    _assert_same(two, restated.candidates(N, ei, src, min_common=2), dev)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_tier_boundary(ssa, dev, graphs):
    """W(u) = 31, 32, 33 around 2 W <= 64; 32 walks into ONE node (count 32 in one slot); 32 walks into 32 nodes (the table half full)"""
    N, ei, g, _ = graphs('boundary')
    sd = torch.arange(8, device=dev)
    want = restated.candidates(N, ei, np.arange(8))
    low = g.candidates(sd, return_info=True, _lds_slots=64)
    assert low[3]['walks'].tolist() == [31, 32, 33, 32, 32, 32, 0, 0]
    assert (low[3]['lds_sources'], low[3]['large_sources']) == (5, 1)
    rows = _rows(low)
    assert rows[4][0].size == 1 and rows[4][1].tolist() == [32] and rows[5][0].size == 32 and (rows[5][1] == 1).all()
    _assert_same(low, want, dev)
    default = g.candidates(sd, return_info=True)
    assert (default[3]['lds_sources'], default[3]['large_sources']) == (6, 0)
    least = g.candidates(sd, return_info=True, _lds_slots=1)
    assert (least[3]['lds_sources'], least[3]['large_sources']) == (0, 6)
    assert _same(low, default) and _same(low, least)
    for slots in (2, 32, 128):
        assert _same(g.candidates(sd, _lds_slots=slots), low)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_hub_through_the_large_tier(ssa, dev, graphs, monkeypatch):
    """node 382 of the negative-sampling graph has 150 neighbours; its W(u) fits the default LDS table, so the boundary is lowered to
    1 024 slots to send it (and it alone among these sources) through the large tier; the centre of a 3 000-node star does not fit the
    default table and takes the large tier as it is, once as one workgroup and once spread over 12"""
    N, ei, g, src = graphs('hub')
    want = restated.candidates(N, ei, src)
    W = int(restated.walks(N, ei, [382])[0])
    assert 1024 < 2 * W <= ssa._native.WEDGE_MAX_SLOTS and len(restated.rows_of(N, ei)[382]) >= 150
    got = g.candidates(torch.from_numpy(src).to(dev), return_info=True, _lds_slots=1024)
    assert got[3]['large_sources'] == 3  # (382 is listed three times, once as -18)
    _assert_same(got, want, dev)
    N, ei, g, src = graphs('star3000')
    want = restated.candidates(N, ei, src)
    sd = torch.from_numpy(src).to(dev)
    one = g.candidates(sd, return_info=True)
    assert one[3]['large_sources'] == 4 and one[3]['lds_sources'] == 0
    _assert_same(one, want, dev)
    monkeypatch.setattr(ssa.wedge, '_WEDGE_SLICE_WALKS', 256)  # 2 998 walks: 12 workgroups per source
    _assert_same(g.candidates(sd), want, dev)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_row_depends_on_its_source_only(ssa, dev, graphs, monkeypatch):
    N, ei, g, _ = graphs('uniform3000')
    rng = np.random.RandomState(3)
    exclude = np.concatenate([ei, ei[:, ::3], np.stack([np.arange(50), np.arange(50)]), ei[:, :500] - N], axis=1)
    ex = torch.from_numpy(exclude).to(dev)
    S = 70
    src = rng.randint(-N, N, size=S).astype(np.int64)  # (duplicates and negative ids included)
    src[:3] = src[3:6]
    sd = torch.from_numpy(src).to(dev)
    for excl, ex_np in ((None, None), (ex, exclude)):
        want = restated.candidates(N, ei, src, exclude=ex_np)
        first = g.candidates(sd, exclude=excl)
        _assert_same(first, want, dev)
        rows_first = _rows(first)
        perm = rng.permutation(S)
        for (a, b), (c, d) in zip(_rows(g.candidates(sd[torch.from_numpy(perm).to(dev)], exclude=excl)), [rows_first[i] for i in perm]):
            assert np.array_equal(a, c) and np.array_equal(b, d)
        assert _same(g.candidates(torch.where(sd < 0, sd + N, sd), exclude=excl), first)
        on_cpu = g.candidates(torch.from_numpy(src), exclude=None if excl is None else excl.cpu())  # CPU in, CPU out
        assert all(t.device.type == 'cpu' for t in on_cpu) and _same(on_cpu, [t.cpu() for t in first])
        parts = [_rows(g.candidates(sd[a:b], exclude=excl)) for a, b in ((0, 1), (1, 33), (33, S))]
        for (a, b), (c, d) in zip(sum(parts, []), rows_first):
            assert np.array_equal(a, c) and np.array_equal(b, d)
        # a tiny byte budget: blocks of 7 sources for the walks launch, one source per expansion
        for slots in (None, 64, 1):
            monkeypatch.setattr(ssa.wedge, '_WEDGE_BLOCK_BYTES', 24 * 7)
            split = g.candidates(sd, exclude=excl, _lds_slots=slots)
            monkeypatch.setattr(ssa.wedge, '_WEDGE_BLOCK_BYTES', 1 << 30)
            assert _same(split, first)
    if True:  # exclude = edge_index: no listed pair is an edge
        rowptr, ids, _ = g.candidates(sd, exclude=torch.from_numpy(np.ascontiguousarray(ei)).to(dev))
        u = np.repeat(np.where(src < 0, src + N, src), np.diff(rowptr.cpu().numpy()))
        edges = set(zip(*ei.tolist()))
        assert ids.numel() and not any((a, b) in edges for a, b in zip(u.tolist(), ids.cpu().tolist()))
    none = g.candidates(sd[:0], exclude=ex, return_info=True)
    assert none[0].tolist() == [0] and none[1].shape == (0,) and none[2].shape == (0,) and none[3]['walks'].shape == (0,)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_max_walks_just_below_and_at_a_sources_walks(ssa, dev, graphs):
    N, ei, g, src = graphs('hub')
    n_walks = restated.walks(N, ei, src)
    W = int(n_walks[0])  # the hub's
    sd = torch.from_numpy(src).to(dev)
    for cap, skipped in ((W, 0), (W - 1, 3), (0, int((n_walks > 0).sum()))):
        got = g.candidates(sd, max_walks=cap, return_info=True)
        want = restated.candidates(N, ei, src, max_walks=cap)
        _assert_same(got, want, dev)
        assert got[3]['skipped_sources'] == want[3] == skipped
        np.testing.assert_array_equal(got[3]['walks'].cpu().numpy(), n_walks)
        assert (_rows(got)[0][0].size > 0) == (cap == W)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_ids_out_of_range(ssa, dev):
    N, ei = restated.odd_graph()
    g = ssa.WedgeGraph(N, torch.from_numpy(ei).to(dev))
    good = g.candidates(torch.tensor([0, 9], device=dev))
    bad = torch.tensor([0, N, 9, -N - 1], device=dev)
    got = g.candidates(bad, return_info=True)  # 'deferred': reported late; the bad rows are empty, the others untouched
    with pytest.raises(IndexError):
        g.check_errors()
    g.check_errors()  # (reported once)
    rows, want = _rows(got), _rows(good)
    assert rows[1][0].size == 0 and rows[3][0].size == 0 and np.array_equal(rows[0][0], want[0][0]) and np.array_equal(rows[2][0], want[1][0])
    assert got[3]['skipped_sources'] == 2 and got[3]['walks'].tolist() == [restated.walks(N, ei, [0])[0], 0, 1, 0]
    g.candidates(torch.tensor([0], device=dev), exclude=torch.tensor([[0], [N]], device=dev))
    with pytest.raises(IndexError):
        g.check_errors()
    with pytest.raises(IndexError):  # CPU ids: at once
        g.candidates(torch.tensor([0, N]))
    g.strict_bounds = True
    with pytest.raises(IndexError):
        g.candidates(bad)
    assert _same(g.candidates(torch.tensor([0, 9], device=dev)), good)
    g.strict_bounds = False
    assert _same(g.candidates(bad), got)
    with pytest.raises(IndexError):  # a device edge_index is checked when the graph is built
        ssa.WedgeGraph(N, torch.tensor([[0], [N]], device=dev))


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def _eh(ssa, h=2, P=128):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    return eh


@pytest.fixture(scope='module')
def tables(ssa, dev, graphs):
    made = {}

    def get(name):
        if name not in made:
            N, ei = graphs(name)[:2]
            made[name] = _eh(ssa, h=3).build_hash_tables(N, torch.from_numpy(np.ascontiguousarray(ei)).to(dev))
        return made[name]

    return get


def _bits(a):
    a = np.asarray(a, dtype=np.float32)
    return np.where(a == 0, np.float32(0), a).view(np.int32)  # +-0 compare equal, every other value bit for bit


def _head(ssa, h, normalised, seed):
    nf = h * (h + 2)
    return ssa.StructureHead(normalised=normalised, **raw_head(2 * nf if normalised else nf, seed))


def _brute_force(eh, table, cards, head, deg, sources, N, k, want, dev):
    """score_links over the restated candidate pairs, each row sorted by (score desc, id asc) and padded"""
    rowptr, cand = want[:2]
    u = np.where(sources < 0, sources + N, sources)
    links = np.stack([np.repeat(u, np.diff(rowptr)), cand], 1)
    sc = eh.score_links(torch.from_numpy(links).to(dev), table, cards, head, degrees=deg).cpu().numpy()
    assert np.all(np.isfinite(sc))
    ids = np.full((len(sources), k), -1, dtype=np.int64)
    scores = np.full((len(sources), k), -np.inf, dtype=np.float32)
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        order = np.lexsort((cand[a:b], -sc[a:b]))[:k]
        ids[r, :len(order)] = cand[a:b][order]
        scores[r, :len(order)] = sc[a:b][order]
    return ids, scores


@pytest.mark.parametrize('name,h,normalised', [('uniform3000', 1, False), ('uniform3000', 2, False), ('uniform3000', 3, False),
                                               ('uniform3000', 2, True), ('hub', 2, False)])
def test_topk_links_wedge_equals_the_brute_force_composition(ssa, dev, graphs, tables, name, h, normalised, monkeypatch):
    N, ei, g, src = graphs(name)
    table, cards = tables(name)
    sub, c = {k: table[k] for k in range(h + 1)}, cards[:, :h]
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, normalised, 30 + 2 * h + int(normalised))
    deg = torch.from_numpy(np.bincount(ei[0][ei[0] % 7 != 3], minlength=N).astype(np.float32)).to(dev) if normalised else None
    sd = torch.from_numpy(src).to(dev)
    for excl in (None, ei):
        want = restated.candidates(N, ei, src, exclude=excl)
        sizes = np.diff(want[0])
        mid = int(np.median(sizes[sizes > 0])) + 1
        assert (sizes < mid).any() and (sizes >= mid).any()  # k = mid: some rows end in padding, some are cut
        ex = None if excl is None else torch.from_numpy(np.ascontiguousarray(excl)).to(dev)
        for k, slots in ((1, None), (mid, None), (mid, 64), (N, 1)):
            ids, scores = eh.topk_links_wedge(sd, sub, c, k, head, g, degrees=deg, exclude=ex, _lds_slots=slots)
            assert ids.shape == (len(src), k) and ids.dtype == torch.int64 and scores.dtype == torch.float32 and ids.device == dev
            w_ids, w_scores = _brute_force(eh, sub, c, head, deg, src, N, k, want, dev)
            np.testing.assert_array_equal(ids.cpu().numpy(), w_ids)
            np.testing.assert_array_equal(_bits(scores.cpu().numpy()), _bits(w_scores))
            if k == N:
                assert (ids[:, -1] == -1).all() and torch.isinf(scores[:, -1]).all()
    # min_common, max_walks (a skipped source: a row of padding) and a split walk reach the ranking too
    n_walks = restated.walks(N, ei, src)
    cap = int(np.unique(n_walks)[-2])  # the sources with the most walks are skipped
    first = eh.topk_links_wedge(sd, sub, c, 5, head, g, degrees=deg, min_common=2, max_walks=cap)
    w = _brute_force(eh, sub, c, head, deg, src, N, 5, restated.candidates(N, ei, src, min_common=2, max_walks=cap), dev)
    np.testing.assert_array_equal(first[0].cpu().numpy(), w[0])
    np.testing.assert_array_equal(_bits(first[1].cpu().numpy()), _bits(w[1]))
    assert (first[0][torch.from_numpy(n_walks > cap).to(dev)] == -1).all() and (n_walks > cap).any()
    monkeypatch.setattr(ssa.wedge, '_WEDGE_BLOCK_BYTES', 24 * 7)
    split = eh.topk_links_wedge(sd, sub, c, 5, head, g, degrees=deg, min_common=2, max_walks=cap)
    assert torch.equal(split[0], first[0]) and torch.equal(split[1].view(torch.int32), first[1].view(torch.int32))
    on_cpu = eh.topk_links_wedge(sd.cpu(), sub, c, 5, head, g, degrees=deg, min_common=2, max_walks=cap)
    assert on_cpu[0].device.type == 'cpu' and torch.equal(on_cpu[0], first[0].cpu()) and torch.equal(on_cpu[1], first[1].cpu())
    empty = eh.topk_links_wedge(sd[:0], sub, c, 5, head, g, degrees=deg)
    assert empty[0].shape == (0, 5) and empty[1].shape == (0, 5) and empty[0].dtype == torch.int64 and empty[1].dtype == torch.float32


def test_topk_links_wedge_reports_ids_out_of_range(ssa, dev, graphs, tables):
    N, ei, g, _ = graphs('ba40')
    table, cards = tables('ba40')
    sub, c = {k: table[k] for k in range(3)}, cards[:, :2]
    eh = _eh(ssa)
    head = _head(ssa, 2, False, 9)
    good = eh.topk_links_wedge(torch.tensor([0, 5], device=dev), sub, c, 3, head, g)
    ids, scores = eh.topk_links_wedge(torch.tensor([0, -N - 1, 5], device=dev), sub, c, 3, head, g)
    with pytest.raises(IndexError):
        eh.check_errors()
    assert (ids[1] == -1).all() and torch.isinf(scores[1]).all()
    assert torch.equal(ids[[0, 2]], good[0]) and torch.equal(scores[[0, 2]], good[1])
    eh.strict_bounds = True
    with pytest.raises(IndexError):
        eh.topk_links_wedge(torch.tensor([N], device=dev), sub, c, 3, head, g)
