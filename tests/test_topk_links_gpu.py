"""ElphHashes.topk_links (csrc/ss_topk_head.hip) on the GPU against the brute-force composition it replaces: score_links
over all N links (u, v) of a source, the exclusion applied, sorted by (score desc, id asc), padded.  Ids must match exactly and scores
bit for bit (up to the sign of zero).  Plus ties, the engine's flags, every sketch shape the scan dispatches on, a skewed graph,
invariance under batching and order, input kinds, an accuracy anchor that does not rest on score_links, and the error paths.

Degrees are the edge list's, counted after the edges of three nodes (a source among them) are dropped: neither golden graph has a
node without edges, and the NaN / Inf -> 0 rule of the normalised copy must be hit from both sides of a pair."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from score_restatement import e_fp, raw_head

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


def _sources(name, N):
    if name == 'ba40':
        return np.arange(N, dtype=np.int64)  # two full groups of 16 and a partial one; more than one staged block
    s = list(np.random.RandomState(11).choice(N, size=35, replace=False)) + [0, N - 1, -1]
    return np.array(s, dtype=np.int64)


def _degrees(N, ei, sources):
    """float32 [N] degrees of the edge list without the edges of nodes 3, N - 2 and the first source: those three have degree 0"""
    drop = np.array([3, N - 2, int(sources[0]) % N])
    keep = ~(np.isin(ei[0], drop) | np.isin(ei[1], drop))
    deg = np.bincount(ei[0][keep], minlength=N).astype(np.float32)
    assert int((deg == 0).sum()) >= 3 and int((deg > 0).sum()) > N // 2
    return deg


def _sub(table, cards, h):
    return {k: table[k] for k in range(h + 1)}, cards[:, :h]


def _head(ssa, h, normalised, seed, **changes):
    nf = h * (h + 2)
    return ssa.StructureHead(normalised=normalised, **dict(raw_head(2 * nf if normalised else nf, seed), **changes))


def _all_scores(eh, table, cards, head, deg, sources, N, dev):
    """score_links over the S * N links (u, v), u first: float32 [S, N]"""
    u = np.where(sources < 0, sources + N, sources)
    links = np.stack([np.repeat(u, N), np.tile(np.arange(N, dtype=np.int64), len(u))], 1)
    sc = eh.score_links(torch.from_numpy(links).to(dev), table, cards, head, degrees=deg)
    return sc.cpu().numpy().reshape(len(u), N)


def _rank(sc, sources, k, N, exclude=None):
    """expected (ids, scores) from the score matrix of _all_scores"""
    ids = np.full((len(sources), k), -1, dtype=np.int64)
    scores = np.full((len(sources), k), -np.inf, dtype=np.float32)
    ex = None if exclude is None else np.where(exclude < 0, exclude + N, exclude)
    for r, u in enumerate(sources):
        u = int(u) + N if int(u) < 0 else int(u)
        elig = np.ones(N, dtype=bool)
        elig[u] = False
        if ex is not None:
            elig[ex[1][ex[0] == u]] = False
        cand = np.nonzero(elig)[0]
        order = np.lexsort((cand, -sc[r][cand]))[:k]
        ids[r, :len(order)] = cand[order]
        scores[r, :len(order)] = sc[r][cand[order]]
    return ids, scores


def _bits(a):
    a = np.asarray(a, dtype=np.float32)
    return np.where(a == 0, np.float32(0), a).view(np.int32)  # +-0 compare equal, every other value bit for bit


def _assert_same(got, want):
    ids, scores = got
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32
    np.testing.assert_array_equal(ids.cpu().numpy(), want[0])
    np.testing.assert_array_equal(_bits(scores.cpu().numpy()), _bits(want[1]))


def _same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.fixture(scope='module')
def world(ssa, dev):
    """3-hop tables (P = 128, p = 8) of the two golden graphs, their sources and degrees, built once; every test reads them only"""
    res = {}
    for name in ('ba40', 'uniform3000'):
        N, ei = _graph(name)
        table, cards = _eh(ssa, h=3).build_hash_tables(N, torch.from_numpy(ei).to(dev))
        sources = _sources(name, N)
        deg = torch.from_numpy(_degrees(N, ei, sources)).to(dev)
        res[name] = (N, ei, table, cards, sources, deg)
    return res


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', ['ba40', 'uniform3000'])
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('normalised', [False, True])
def test_matches_brute_force(ssa, dev, world, graph, h, normalised):
    N, ei, table, cards, sources, deg = world[graph]
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, normalised, 40 + 2 * h + int(normalised))
    dg = deg if normalised else None
    src = torch.from_numpy(sources).to(dev)
    sc = _all_scores(eh, sub, c, head, dg, sources, N, dev)
    assert np.all(np.isfinite(sc)) and len(np.unique(sc)) > N // 4
    for excl in (None, ei):
        for k in (1, 10, N):
            got = eh.topk_links(src, sub, c, k, head, degrees=dg, exclude=None if excl is None else torch.from_numpy(excl).to(dev))
            assert got[0].shape == (len(sources), k) and got[0].device == dev and got[1].device == dev
            _assert_same(got, _rank(sc, sources, k, N, excl))
            if k == N:  # every row ends in padding: u itself (and its excluded partners) are never candidates
                assert (got[0][:, -1] == -1).all() and torch.isinf(got[1][:, -1]).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', ['ba40', 'uniform3000'])
def test_ties_come_back_by_ascending_id(ssa, dev, world, graph):
    N, ei, table, cards, sources, deg = world[graph]
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    src = torch.from_numpy(sources).to(dev)
    raw = raw_head(8, 3)
    b2 = np.float32(raw['out_bias'][0].item())
    ident = dict(bn_weight=torch.ones(8), bn_bias=torch.zeros(8), bn_mean=torch.zeros(8), bn_var=torch.ones(8), bn_eps=0.0)
    for head in (ssa.StructureHead(**dict(raw, out_weight=torch.zeros(8))),                     # every score is b2
                 ssa.StructureHead(**dict(raw, **ident, bias=torch.full((8,), -1e30)))):     # every ReLU closed
        for excl in (None, ei):
            k = 12
            ids, scores = eh.topk_links(src, sub, c, k, head, exclude=None if excl is None else torch.from_numpy(excl).to(dev))
            want = _rank(np.full((len(sources), N), b2, dtype=np.float32), sources, k, N, excl)
            _assert_same((ids, scores), want)
            valid = want[0] >= 0
            assert np.all(np.diff(want[0], axis=1)[valid[:, 1:]] > 0)
            assert np.all(scores.cpu().numpy()[valid].view(np.int32) == b2.view(np.int32))


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [2, 3])
@pytest.mark.parametrize('use_zero_one,floor_sf', [(False, False), (True, True), (False, True)])
def test_engine_flags(ssa, dev, world, h, use_zero_one, floor_sf):
    N, ei, table, cards, sources, deg = world['ba40']
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h, floor_sf=floor_sf, use_zero_one=use_zero_one)
    plain = _eh(ssa, h=h)
    src = torch.from_numpy(sources).to(dev)
    for normalised in (False, True):
        head = _head(ssa, h, normalised, 60 + h)
        dg = deg if normalised else None
        sc = _all_scores(eh, sub, c, head, dg, sources, N, dev)
        if not use_zero_one:  # (two or four features are zeroed: the scores cannot stay)
            assert not np.array_equal(sc, _all_scores(plain, sub, c, head, dg, sources, N, dev)), 'the flag must change the scores'
        _assert_same(eh.topk_links(src, sub, c, 10, head, degrees=dg, exclude=torch.from_numpy(ei).to(dev)), _rank(sc, sources, 10, N, ei))


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,p', [(8, 4), (64, 8), (256, 8), (192, 6), (128, 16)])
def test_sketch_shapes(ssa, dev, P, p):
    """the run-time-size path ((8, 4), (192, 6), (128, 16)) and the fast instantiations other than P = 128"""
    N, ei = _graph('uniform3000')
    h = 2
    eh = _eh(ssa, h=h, p=p, P=P)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = np.array([17, 0, N - 1, -2], dtype=np.int64)
    deg = torch.from_numpy(_degrees(N, ei, sources)).to(dev)
    src = torch.from_numpy(sources).to(dev)
    for normalised in (False, True):
        head = _head(ssa, h, normalised, P + p)
        dg = deg if normalised else None
        sc = _all_scores(eh, table, cards, head, dg, sources, N, dev)
        for excl in (None, ei):
            got = eh.topk_links(src, table, cards, 10, head, degrees=dg, exclude=None if excl is None else torch.from_numpy(excl).to(dev))
            _assert_same(got, _rank(sc, sources, 10, N, excl))


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('P', [64, 192, 256])
def test_fast_shapes_at_the_other_hop_counts(ssa, dev, h, P):
    """every (h, P) instantiation stages another number of sources per workgroup: 40 sources cross a block boundary in each"""
    N, ei = _graph('ba40')
    eh = _eh(ssa, h=h, P=P)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = _sources('ba40', N)
    deg = torch.from_numpy(_degrees(N, ei, sources)).to(dev)
    head = _head(ssa, h, True, P + h)
    sc = _all_scores(eh, table, cards, head, deg, sources, N, dev)
    got = eh.topk_links(torch.from_numpy(sources).to(dev), table, cards, N, head, degrees=deg)
    _assert_same(got, _rank(sc, sources, N, N))


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_skewed_graph(ssa, dev):
    N, ei = _graph('powerlaw50k')
    h = 2
    eh = _eh(ssa, h=h)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = np.array([0, 31337, -1], dtype=np.int64)  # the largest row, a leaf, a negative id
    deg = torch.from_numpy(np.bincount(ei[0], minlength=N).astype(np.float32)).to(dev)
    assert int((deg == 0).sum()) > 0
    exclude = torch.from_numpy(ei).to(dev)
    for normalised in (False, True):
        head = _head(ssa, h, normalised, 5)
        dg = deg if normalised else None
        sc = _all_scores(eh, table, cards, head, dg, sources, N, dev)
        _assert_same(eh.topk_links(torch.from_numpy(sources).to(dev), table, cards, 25, head, degrees=dg, exclude=exclude),
                     _rank(sc, sources, 25, N, ei))


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [2, 3])
def test_rows_do_not_depend_on_batching(ssa, dev, world, monkeypatch, h):
    N, ei, table, cards, _, deg = world['uniform3000']
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, True, 70 + h)
    exclude = torch.from_numpy(ei).to(dev)
    S = 70
    src = torch.from_numpy(np.random.RandomState(S).randint(-N, N, size=S)).to(dev)  # (duplicates and negative ids included)
    call = lambda s: eh.topk_links(s, sub, c, 25, head, degrees=deg, exclude=exclude)
    first = call(src)
    assert bool(torch.isfinite(first[1]).all())
    assert _same_bits(call(src), first)
    perm = torch.from_numpy(np.random.RandomState(S + 1).permutation(S)).to(dev)
    assert _same_bits(call(src[perm]), (first[0][perm], first[1][perm]))
    parts = [call(src[a:b]) for a, b in ((0, 1), (1, 33), (33, S))]
    assert _same_bits((torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])), first)
    monkeypatch.setattr(ssa.engine, '_TOPK_KEY_BYTES', 3 * 8 * N)  # the key buffer split into blocks of 3 sources
    blocked = call(src)
    monkeypatch.undo()
    assert _same_bits(blocked, first)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_inputs(ssa, dev, world):
    N, ei, table, cards, _, deg = world['ba40']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, True, 8)
    src = torch.arange(-N, N, 3, dtype=torch.int64)
    d_ids, d_sc = eh.topk_links(src.to(dev), sub, c, 7, head, degrees=deg, exclude=torch.from_numpy(ei).to(dev))
    c_ids, c_sc = eh.topk_links(src, sub, c, 7, head, degrees=deg.cpu(), exclude=torch.from_numpy(ei))   # CPU in, CPU out
    assert c_ids.device.type == 'cpu' and c_sc.device.type == 'cpu' and d_ids.device == dev and d_sc.device == dev
    assert torch.equal(c_ids, d_ids.cpu()) and torch.equal(c_sc, d_sc.cpu())
    # the reference's dict of int64 / int8 leaves (a torch.load-ed cache) and CPU cards give the same rows as the SketchTable
    plain = {k: {'minhash': table[k]['minhash'].cpu().clone(), 'hll': table[k]['hll'].cpu().clone()} for k in range(h + 1)}
    p_ids, p_sc = eh.topk_links(src, plain, c.cpu(), 7, head, degrees=deg.cpu(), exclude=torch.from_numpy(ei))
    assert torch.equal(p_ids, c_ids) and torch.equal(p_sc, c_sc)
    e_ids, e_sc = eh.topk_links(src[:0], sub, c, 7, head, degrees=deg)
    assert e_ids.shape == (0, 7) and e_sc.shape == (0, 7) and e_ids.dtype == torch.int64 and e_sc.dtype == torch.float32


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [1, 2, 3])
def test_scores_against_the_float64_head_on_the_engine_rows(ssa, dev, world, h):
    """for the returned (u, id) pairs: |score - head.reference(get_subgraph_features row)| <= e_fp, the bound score_links is held to"""
    N, ei, table, cards, sources, deg = world['uniform3000']
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    src = torch.from_numpy(sources).to(dev)
    for normalised in (False, True):
        head = _head(ssa, h, normalised, 80 + h)
        dg = deg if normalised else None
        ids, scores = eh.topk_links(src, sub, c, 50, head, degrees=dg, exclude=torch.from_numpy(ei).to(dev))
        assert bool((ids >= 0).all())
        u = torch.where(src < 0, src + N, src)
        links = torch.stack([u[:, None].expand_as(ids).reshape(-1), ids.reshape(-1)], 1)
        rows = eh.get_subgraph_features(links, sub, c, degrees=dg).double().cpu().numpy()
        assert np.all(np.isfinite(rows))
        err = np.abs(scores.double().cpu().numpy().reshape(-1) - head.reference(rows))
        bar = e_fp(head, rows)
        worst = int(np.argmax(err - bar))
        assert np.all(err <= bar), f'h={h} normalised={normalised}: pair {links[worst].tolist()}: {err[worst]:.3e} > {bar[worst]:.3e}'


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors(ssa, dev, world):
    N, ei, table, cards, _, deg = world['ba40']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, False, 9)
    ok = torch.tensor([0, 5], dtype=torch.int64)
    with pytest.raises(IndexError):
        eh.topk_links(torch.tensor([0, N]), sub, c, 3, head)
    with pytest.raises(IndexError):
        eh.topk_links(torch.tensor([-N - 1]), sub, c, 3, head)
    with pytest.raises(IndexError):
        eh.topk_links(ok, sub, c, 3, head, exclude=torch.tensor([[0], [N]]))
    for k in (0, N + 1):
        with pytest.raises(ValueError):
            eh.topk_links(ok, sub, c, k, head)
    with pytest.raises(ValueError):
        eh.topk_links(ok, sub, c, 3, _head(ssa, 3, False, 1))                      # a 3-hop head
    with pytest.raises(ValueError):
        eh.topk_links(ok, sub, c, 3, _head(ssa, h, True, 1))                       # normalised without degrees
    with pytest.raises(ValueError):
        eh.topk_links(ok, sub, c, 3, head, degrees=deg)                            # degrees with a plain head
    with pytest.raises(ValueError):
        eh.topk_links(ok, sub, c, 3, raw_head(8, 1))                               # not a StructureHead
    # device ids: reported late, as get_subgraph_features does; the bad source's row is padding, the other rows are untouched
    good = eh.topk_links(torch.tensor([0, 5], device=dev), sub, c, 3, head)
    ids, scores = eh.topk_links(torch.tensor([0, N, 5], device=dev), sub, c, 3, head)
    with pytest.raises(IndexError):
        eh.check_errors()
    assert (ids[1] == -1).all() and torch.isinf(scores[1]).all()
    assert _same_bits((ids[[0, 2]], scores[[0, 2]]), good)
    eh.topk_links(ok.to(dev), sub, c, 3, head, exclude=torch.tensor([[0], [-N - 1]], device=dev))
    with pytest.raises(IndexError):
        eh.check_errors()
    eh.check_errors()  # (reported once)
    eh.strict_bounds = True
    with pytest.raises(IndexError):
        eh.topk_links(torch.tensor([N], device=dev), sub, c, 3, head)
