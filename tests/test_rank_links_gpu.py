"""ElphHashes.rank_links (csrc/ss_rank.hip) on the GPU against its definition: the brute-force score_links matrix of every
link's source against all N nodes, counted in numpy (rank_restatement.py).  `greater` and `equal` must match as integers, exactly.
Plus ties, exclusion as a set with an immune target, agreement with topk_links' order, the engine's flags, every sketch shape the scan
dispatches on, a skewed graph, independence from batching and order, input kinds and the error paths.

Graphs, degrees (three nodes of degree 0, a source among them), heads and helpers follow test_topk_links_gpu.py."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from rank_restatement import candidates, rank_counts, tied_below, wrap
from score_restatement import raw_head

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


def _eh(ssa, h=2, p=8, P=128, floor_sf=False, use_zero_one=True):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=floor_sf, use_zero_one=use_zero_one))
    eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    return eh


def _uniform_graph(n, e_und, seed):
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _power_law_graph(n=50000, e_und=250000, seed=7):
    """the generator of test_topk_gpu.py"""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, size=e_und)
    dst = np.minimum((n * rng.random_sample(e_und) ** 3).astype(np.int64), n - 1)
    e = np.stack([src, dst]).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _graph(name):
    if name == 'ba40':
        g = load_golden('g3_g4_ba40.npz')
        return int(g['num_nodes']), g['edge_index'].astype(np.int64)
    if name == 'uniform3000':
        n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
        return n, _uniform_graph(n, e_und, seed)
    return 50000, _power_law_graph()


def _links(name, N, ei):
    if name == 'ba40':  # all N * N ordered pairs, u == t included: several staged blocks, partial groups of 16
        return np.stack([np.repeat(np.arange(N), N), np.tile(np.arange(N), N)], 1).astype(np.int64)
    rng = np.random.RandomState(13)
    edges = ei[:, rng.choice(ei.shape[1], size=40, replace=False)].T            # positives as evaluation lists them
    others = rng.randint(0, N, size=(40, 2))                                    # (almost surely) non-edges
    negative = rng.randint(-N, 0, size=(20, 2))                                 # torch-style ids
    repeated = np.stack([np.full(20, edges[0, 0]), rng.randint(0, N, size=20)], 1)  # one source, twenty targets
    ends = np.array([[0, N - 1], [N - 1, 0], [-1, -N], [5, 5]])
    return np.concatenate([edges, others, negative, repeated, ends]).astype(np.int64)


def _degrees(N, ei, first_source):
    """float32 [N] degrees of the edge list without the edges of nodes 3, N - 2 and the first link's source: those three have degree 0"""
    drop = np.array([3, N - 2, int(first_source) % N])
    keep = ~(np.isin(ei[0], drop) | np.isin(ei[1], drop))
    deg = np.bincount(ei[0][keep], minlength=N).astype(np.float32)
    assert int((deg == 0).sum()) >= 3 and int((deg > 0).sum()) > N // 2
    return deg


def _sub(table, cards, h):
    return {k: table[k] for k in range(h + 1)}, cards[:, :h]


def _head(ssa, h, normalised, seed, **changes):
    nf = h * (h + 2)
    return ssa.StructureHead(normalised=normalised, **dict(raw_head(2 * nf if normalised else nf, seed), **changes))


def _score_rows(eh, table, cards, head, deg, links, N, dev):
    """score_links over the N links (u, v) of every distinct source u of `links`, u first: {u: float32 [N]}"""
    us = np.unique(wrap(links, N)[:, 0])
    pairs = np.stack([np.repeat(us, N), np.tile(np.arange(N, dtype=np.int64), len(us))], 1)
    sc = eh.score_links(torch.from_numpy(pairs).to(dev), table, cards, head, degrees=deg).cpu().numpy().reshape(len(us), N)
    assert np.all(np.isfinite(sc))
    return {int(u): sc[i] for i, u in enumerate(us)}


def _want(rows, links, N, exclude=None):
    return rank_counts(lambda q, u: rows[u], links, N, exclude)


def _assert_same(got, want, where=''):
    greater, equal = got
    assert greater.dtype == torch.int64 and equal.dtype == torch.int64 and greater.shape == equal.shape == (len(want[0]),)
    g, e = greater.cpu().numpy(), equal.cpu().numpy()
    bad = np.nonzero((g != want[0]) | (e != want[1]))[0]
    assert bad.size == 0, f'{where}: {bad.size} links differ, first {int(bad[0])}: got ({g[bad[0]]}, {e[bad[0]]}), want ({want[0][bad[0]]}, {want[1][bad[0]]})'


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope='module')
def world(ssa, dev):
    """3-hop tables (P = 128, p = 8) of the two golden graphs, their links and degrees, built once; every test reads them only"""
    res = {}
    for name in ('ba40', 'uniform3000'):
        N, ei = _graph(name)
        table, cards = _eh(ssa, h=3).build_hash_tables(N, torch.from_numpy(ei).to(dev))
        links = _links(name, N, ei)
        deg = torch.from_numpy(_degrees(N, ei, links[0, 0])).to(dev)
        res[name] = (N, ei, table, cards, links, deg)
    return res


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', ['ba40', 'uniform3000'])
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('normalised', [False, True])
def test_matches_brute_force(ssa, dev, world, graph, h, normalised):
    N, ei, table, cards, links, deg = world[graph]
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, normalised, 40 + 2 * h + int(normalised))
    dg = deg if normalised else None
    rows = _score_rows(eh, sub, c, head, dg, links, N, dev)
    assert len(np.unique(np.stack(list(rows.values())))) > N // 4
    for excl in (None, ei):
        got = eh.rank_links(_t(links, dev), sub, c, head, degrees=dg, exclude=_t(excl, dev))
        assert got[0].device == dev and got[1].device == dev
        want = _want(rows, links, N, excl)
        _assert_same(got, want, f'exclude={excl is not None}')
        assert want[0].max() > 0 and (want[0] + want[1]).max() <= N - 1


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', ['ba40', 'uniform3000'])
def test_ties(ssa, dev, world, graph):
    N, ei, table, cards, links, deg = world[graph]
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    raw = raw_head(8, 3)
    ident = dict(bn_weight=torch.ones(8), bn_bias=torch.zeros(8), bn_mean=torch.zeros(8), bn_var=torch.ones(8), bn_eps=0.0)
    w = wrap(links, N)
    for head in (ssa.StructureHead(**dict(raw, out_weight=torch.zeros(8))),                     # every score is b2
                 ssa.StructureHead(**dict(raw, **ident, bias=torch.full((8,), -1e30)))):     # every ReLU closed
        for excl in (None, ei):
            greater, equal = eh.rank_links(_t(links, dev), sub, c, head, exclude=_t(excl, dev))
            size = np.array([int(candidates(int(u), int(t), N, excl).sum()) for u, t in w])
            assert int(greater.abs().sum()) == 0
            np.testing.assert_array_equal(equal.cpu().numpy(), size)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_exclusion_is_a_set_and_the_target_is_immune(ssa, dev, world):
    N, ei, table, cards, links, deg = world['uniform3000']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, True, 31)
    call = lambda excl: eh.rank_links(_t(links, dev), sub, c, head, degrees=deg, exclude=_t(excl, dev))
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    clean = call(ei)
    loops = np.stack([np.arange(N), np.arange(N)])
    messy = np.concatenate([ei, ei, loops, ei - N], axis=1)              # every column twice, self loops, negative ids
    assert same(call(messy), clean)
    # a link's own column is another link's exclusion when they share a source: the immunity is checked on the links whose source
    # is no other link's
    w = wrap(links, N)
    _, index, count = np.unique(w[:, 0], return_index=True, return_counts=True)
    alone = np.sort(index[count == 1])
    assert 60 <= alone.size < len(links)
    call_alone = lambda excl: eh.rank_links(_t(links[alone], dev), sub, c, head, degrees=deg, exclude=_t(excl, dev))
    clean_alone = (clean[0][alone], clean[1][alone])
    own = w[alone].T                                                     # those links' own (u -> t) columns
    assert same(call_alone(np.concatenate([ei, own], axis=1)), clean_alone)
    is_own = np.isin(ei[0] * N + ei[1], own[0] * N + own[1])
    assert is_own.sum() >= 30
    assert same(call_alone(ei[:, ~is_own]), clean_alone)
    without = call(None)
    assert bool((clean[0] <= without[0]).all()) and bool((clean[1] <= without[1]).all())
    assert not same(clean, without)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_agrees_with_the_order_of_topk_links(ssa, dev, world):
    """for an eligible target: its place in the topk_links(u, k = N) row == greater + #{tied v < t}"""
    N, ei, table, cards, links, deg = world['uniform3000']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    for head, dg in ((_head(ssa, h, False, 32), None), (_head(ssa, h, False, 3, out_weight=torch.zeros(8)), None), (_head(ssa, h, True, 33), deg)):
        rows = _score_rows(eh, sub, c, head, dg, links, N, dev)
        for excl in (None, ei):
            w = wrap(links, N)
            eligible = np.array([bool(candidates(int(u), int(u), N, excl)[t]) for u, t in w])
            assert eligible.sum() >= 40
            lk = w[eligible]
            greater, equal = (a.cpu().numpy() for a in eh.rank_links(_t(lk, dev), sub, c, head, degrees=dg, exclude=_t(excl, dev)))
            ids, _ = eh.topk_links(_t(lk[:, 0], dev), sub, c, N, head, degrees=dg, exclude=_t(excl, dev))
            hit = ids.cpu().numpy() == lk[:, 1:2]
            assert np.all(hit.sum(1) == 1)
            pos = hit.argmax(1)
            below = tied_below(lambda q, u: rows[u], lk, N, excl)
            np.testing.assert_array_equal(pos, greater + below)
            assert np.all(greater <= pos) and np.all(pos <= greater + equal)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [2, 3])
@pytest.mark.parametrize('use_zero_one,floor_sf', [(False, False), (True, True), (False, True)])
def test_engine_flags(ssa, dev, world, h, use_zero_one, floor_sf):
    N, ei, table, cards, links, deg = world['ba40']
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h, floor_sf=floor_sf, use_zero_one=use_zero_one)
    plain = _eh(ssa, h=h)
    for normalised in (False, True):
        head = _head(ssa, h, normalised, 60 + h)
        dg = deg if normalised else None
        rows = _score_rows(eh, sub, c, head, dg, links, N, dev)
        if not use_zero_one:  # (two or four features are zeroed: the scores cannot stay)
            other = _score_rows(plain, sub, c, head, dg, links, N, dev)
            assert any(not np.array_equal(rows[u], other[u]) for u in rows), 'the flag must change the scores'
        _assert_same(eh.rank_links(_t(links, dev), sub, c, head, degrees=dg, exclude=_t(ei, dev)), _want(rows, links, N, ei))


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,p', [(8, 4), (64, 8), (256, 8), (192, 6), (128, 16)])
def test_sketch_shapes(ssa, dev, P, p):
    """the run-time-size path ((8, 4), (192, 6), (128, 16)) and the fast instantiations other than P = 128"""
    N, ei = _graph('uniform3000')
    h = 2
    eh = _eh(ssa, h=h, p=p, P=P)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    links = np.array([[17, 4], [0, N - 1], [N - 1, 0], [-2, 17], [17, -3], [ei[0, 0], ei[1, 0]]], dtype=np.int64)
    deg = torch.from_numpy(_degrees(N, ei, links[0, 0])).to(dev)
    for normalised in (False, True):
        head = _head(ssa, h, normalised, P + p)
        dg = deg if normalised else None
        rows = _score_rows(eh, table, cards, head, dg, links, N, dev)
        for excl in (None, ei):
            _assert_same(eh.rank_links(_t(links, dev), table, cards, head, degrees=dg, exclude=_t(excl, dev)), _want(rows, links, N, excl))


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('P', [64, 192, 256, 36])
def test_fast_shapes_at_the_other_hop_counts(ssa, dev, h, P):
    """every (h, P) instantiation stages another number of links per workgroup: 45 links cross a block boundary in each
    (P = 36: the run-time-size instantiation of every hop count, fewer MinHash chunks than lanes)"""
    N, ei = _graph('ba40')
    eh = _eh(ssa, h=h, P=P)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    links = np.stack([np.arange(45) % N, (7 * np.arange(45) + 3) % N], 1).astype(np.int64)
    deg = torch.from_numpy(_degrees(N, ei, links[0, 0])).to(dev)
    head = _head(ssa, h, True, P + h)
    rows = _score_rows(eh, table, cards, head, deg, links, N, dev)
    for excl in (None, ei):
        _assert_same(eh.rank_links(_t(links, dev), table, cards, head, degrees=deg, exclude=_t(excl, dev)), _want(rows, links, N, excl))


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_skewed_graph(ssa, dev):
    N, ei = _graph('powerlaw50k')
    h = 2
    eh = _eh(ssa, h=h)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    links = np.array([[0, 31337], [31337, 0], [-1, -N + 2]], dtype=np.int64)  # from the largest row, from a leaf, negative ids
    deg = torch.from_numpy(np.bincount(ei[0], minlength=N).astype(np.float32)).to(dev)
    assert int((deg == 0).sum()) > 0
    exclude = torch.from_numpy(ei).to(dev)
    for normalised in (False, True):
        head = _head(ssa, h, normalised, 5)
        dg = deg if normalised else None
        rows = _score_rows(eh, table, cards, head, dg, links, N, dev)
        _assert_same(eh.rank_links(_t(links, dev), table, cards, head, degrees=dg, exclude=exclude), _want(rows, links, N, ei))


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [2, 3])
def test_rows_do_not_depend_on_batching(ssa, dev, world, monkeypatch, h):
    N, ei, table, cards, _, deg = world['uniform3000']
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, True, 70 + h)
    exclude = torch.from_numpy(ei).to(dev)
    L = 70
    lk = np.random.RandomState(L).randint(-N, N, size=(L, 2))
    lk[40:50] = lk[5]                                         # duplicate links
    lk[50:60, 0] = lk[6, 0]                                   # and a repeated source
    lk = torch.from_numpy(lk).to(dev)
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    call = lambda s: eh.rank_links(s, sub, c, head, degrees=deg, exclude=exclude)
    first = call(lk)
    assert int(first[0].max()) > 0 and int(first[0].min()) >= 0
    assert same(call(lk), first)
    perm = torch.from_numpy(np.random.RandomState(L + 1).permutation(L)).to(dev)
    assert same(call(lk[perm]), (first[0][perm], first[1][perm]))
    parts = [call(lk[a:b]) for a, b in ((0, 1), (1, 33), (33, L))]
    assert same((torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])), first)
    assert bool((first[0][40:50] == first[0][5]).all()) and bool((first[1][40:50] == first[1][5]).all())
    for launch, chunk in ((3, 3), (300, 200)):
        monkeypatch.setattr(ssa.engine, '_RANK_LAUNCH_LINKS', launch)   # the links split into launches,
        monkeypatch.setattr(ssa.engine, '_RANK_EXCLUDE_PAIRS', chunk)   # the excluded pairs into chunks
        split = call(lk)
        monkeypatch.undo()
        assert same(split, first)


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_inputs(ssa, dev, world):
    N, ei, table, cards, links, deg = world['ba40']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, True, 8)
    lk = torch.from_numpy(links[::7] - N * (np.arange(len(links[::7]))[:, None] % 2))  # every other link with negative ids
    d = eh.rank_links(lk.to(dev), sub, c, head, degrees=deg, exclude=torch.from_numpy(ei).to(dev))
    cpu = eh.rank_links(lk, sub, c.cpu(), head, degrees=deg.cpu(), exclude=torch.from_numpy(ei))   # CPU in, CPU out
    assert all(a.device.type == 'cpu' and a.dtype == torch.int64 for a in cpu) and all(a.device == dev for a in d)
    assert torch.equal(cpu[0], d[0].cpu()) and torch.equal(cpu[1], d[1].cpu())
    # the reference's dict of int64 / int8 leaves (a torch.load-ed cache) gives the same rows as the SketchTable
    plain = {k: {'minhash': table[k]['minhash'].cpu().clone(), 'hll': table[k]['hll'].cpu().clone()} for k in range(h + 1)}
    p = eh.rank_links(lk, plain, c.cpu(), head, degrees=deg.cpu(), exclude=torch.from_numpy(ei))
    assert torch.equal(p[0], cpu[0]) and torch.equal(p[1], cpu[1])
    one = eh.rank_links(lk[3].to(dev), sub, c, head, degrees=deg, exclude=torch.from_numpy(ei).to(dev))   # a [2]-shaped link
    assert one[0].shape == (1,) and int(one[0][0]) == int(d[0][3]) and int(one[1][0]) == int(d[1][3])
    e = eh.rank_links(lk[:0].to(dev), sub, c, head, degrees=deg)
    assert e[0].shape == (0,) and e[1].shape == (0,) and e[0].dtype == torch.int64 and e[1].dtype == torch.int64


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_errors(ssa, dev, world):
    N, ei, table, cards, _, deg = world['ba40']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, False, 9)
    ok = torch.tensor([[0, 5], [5, 7]], dtype=torch.int64)
    with pytest.raises(IndexError):
        eh.rank_links(torch.tensor([[0, N]]), sub, c, head)
    with pytest.raises(IndexError):
        eh.rank_links(torch.tensor([[-N - 1, 0]]), sub, c, head)
    with pytest.raises(IndexError):
        eh.rank_links(ok, sub, c, head, exclude=torch.tensor([[0], [N]]))
    with pytest.raises(ValueError):
        eh.rank_links(ok, sub, c, _head(ssa, 3, False, 1))                      # a 3-hop head
    with pytest.raises(ValueError):
        eh.rank_links(ok, sub, c, _head(ssa, h, True, 1))                       # normalised without degrees
    with pytest.raises(ValueError):
        eh.rank_links(ok, sub, c, head, degrees=deg)                            # degrees with a plain head
    with pytest.raises(ValueError):
        eh.rank_links(ok, sub, c, raw_head(8, 1))                               # not a StructureHead
    with pytest.raises(ValueError, match='mask_target'):
        eh.rank_links(ok, sub, c, head, mask_target=torch.zeros((2, 0), dtype=torch.int64))
    # device ids: reported late, as get_subgraph_features does; the bad link's row is -1 / -1, the other rows are untouched
    exclude = torch.from_numpy(ei).to(dev)
    good = eh.rank_links(ok.to(dev), sub, c, head, exclude=exclude)
    for bad in ([0, N], [-N - 1, 7]):
        g, e = eh.rank_links(torch.tensor([[0, 5], bad, [5, 7]], device=dev), sub, c, head, exclude=exclude)
        with pytest.raises(IndexError):
            eh.check_errors()
        assert int(g[1]) == -1 and int(e[1]) == -1
        assert torch.equal(g[[0, 2]], good[0]) and torch.equal(e[[0, 2]], good[1])
    g, e = eh.rank_links(ok.to(dev), sub, c, head, exclude=torch.tensor([[0, 0], [-N - 1, 3]], device=dev))
    with pytest.raises(IndexError):
        eh.check_errors()
    eh.check_errors()  # (reported once)
    want = eh.rank_links(ok.to(dev), sub, c, head, exclude=torch.tensor([[0], [3]], device=dev))
    assert torch.equal(g, want[0]) and torch.equal(e, want[1])    # (the out-of-range column is dropped, the other one applies)
    eh.strict_bounds = True
    with pytest.raises(IndexError):
        eh.rank_links(torch.tensor([[0, N]], device=dev), sub, c, head)
    with pytest.raises(IndexError):
        eh.rank_links(ok.to(dev), sub, c, head, exclude=torch.tensor([[0], [N]], device=dev))
