"""ElphHashes.topk_candidates (csrc/ss_topk.hip) on the GPU against the brute-force composition it replaces: _get_intersections over
all N pairs of a source, the exclusion applied, sorted by (score desc, id asc).  Ids must match exactly and scores bit for bit (up to
the sign of zero); plus the non-default sketch shapes, collab size, invariance under batching and order, input kinds, the error
paths and a pin against the CPU oracle."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import load_golden, oracle_params

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


def _eh(ssa, h=2, p=8, P=128):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    return eh


def _uniform_graph(n, e_und, seed):
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _power_law_graph(n=50000, e_und=250000, seed=7):
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, size=e_und)
    dst = np.minimum((n * rng.random_sample(e_und) ** 3).astype(np.int64), n - 1)
    e = np.stack([src, dst]).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _brute(eh, table, sources, k, hops, N, exclude=None):
    """expected (ids, scores) from _get_intersections over all N pairs of every source"""
    dev = torch.device('cuda:0')
    ids = np.full((len(sources), k), -1, dtype=np.int64)
    scores = np.full((len(sources), k), -np.inf, dtype=np.float32)
    for r, u in enumerate(sources):
        u = int(u) + N if int(u) < 0 else int(u)
        links = torch.stack([torch.full((N,), u, dtype=torch.int64), torch.arange(N, dtype=torch.int64)], 1).to(dev)
        sc = eh._get_intersections(links, table)[hops].cpu().numpy()
        elig = np.ones(N, dtype=bool)
        elig[u] = False
        if exclude is not None:
            ex = np.where(exclude < 0, exclude + N, exclude)
            elig[ex[1][ex[0] == u]] = False
        cand = np.nonzero(elig)[0]
        order = np.lexsort((cand, -sc[cand]))[:k]
        ids[r, :len(order)] = cand[order]
        scores[r, :len(order)] = sc[cand[order]]
    return ids, scores


def _bits(a):
    a = np.asarray(a, dtype=np.float32)
    return np.where(a == 0, np.float32(0), a).view(np.int32)  # +-0 compare equal, every other value bit for bit


def _assert_same(got, want):
    ids, scores = got
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32
    np.testing.assert_array_equal(ids.cpu().numpy(), want[0])
    np.testing.assert_array_equal(_bits(scores.cpu().numpy()), _bits(want[1]))


def _graph(name):
    if name == 'ba40':
        g = load_golden('g3_g4_ba40.npz')
        return int(g['num_nodes']), g['edge_index'].astype(np.int64)
    if name == 'uniform3000':
        n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
        return n, _uniform_graph(n, e_und, seed)
    return 50000, _power_law_graph()


def _sources(N, n_src, seed, hubs=True):
    rng = np.random.RandomState(seed)
    s = list(rng.choice(N, size=min(n_src, N), replace=False))
    if hubs:
        s += [0, N - 1, -1]  # a power-law graph's largest rows, the last node, a negative id
    return np.array(s, dtype=np.int64)


@pytest.mark.parametrize('graph', ['ba40', 'uniform3000', 'powerlaw50k'])
@pytest.mark.parametrize('h', [2, 3])
def test_matches_brute_force(ssa, dev, graph, h):
    N, ei = _graph(graph)
    eh = _eh(ssa, h=h)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = _sources(N, {'ba40': 40, 'uniform3000': 12, 'powerlaw50k': 3}[graph], seed=h)
    src = torch.from_numpy(sources).to(dev)
    combos = [(k1, k2) for k1 in range(1, h + 1) for k2 in range(1, h + 1)]
    if graph == 'powerlaw50k':
        combos = [(1, 1), (1, h), (h, 2)]
    for hops in combos:
        for excl in (None, ei):
            for k in (1, 10, N):
                if graph == 'powerlaw50k' and k == N:
                    continue
                want = _brute(eh, table, sources, k, hops, N, excl)
                got = eh.topk_candidates(src, table, k, hops=hops, exclude=None if excl is None else torch.from_numpy(excl).to(dev))
                _assert_same(got, want)
                if k == N:  # every row ends in padding: u itself (and its excluded partners) are never candidates
                    assert (got[0][:, -1] == -1).all() and torch.isinf(got[1][:, -1]).all()
    # k = N on the power-law graph, one combination (the full ranking of a hub and a leaf)
    if graph == 'powerlaw50k':
        want = _brute(eh, table, sources[-3:], N, (1, 1), N, ei)
        _assert_same(eh.topk_candidates(src[-3:], table, N, exclude=torch.from_numpy(ei).to(dev)), want)


@pytest.mark.parametrize('P,p', [(8, 4), (128, 16), (64, 8), (256, 8), (192, 6)])
def test_other_sketch_shapes(ssa, dev, P, p):
    N, ei = _graph('uniform3000')
    eh = _eh(ssa, h=2, p=p, P=P)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = _sources(N, 40, seed=P + p)
    src = torch.from_numpy(sources).to(dev)
    for hops in ((1, 1), (2, 1)):
        for excl in (None, ei):
            want = _brute(eh, table, sources, 10, hops, N, excl)
            _assert_same(eh.topk_candidates(src, table, 10, hops=hops, exclude=None if excl is None else torch.from_numpy(excl).to(dev)),
                         want)


def test_collab_size(ssa, dev):
    N = 235868
    ei = _uniform_graph(N, 1200000, seed=9)
    eh = _eh(ssa, h=2)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = _sources(N, 64, seed=1, hubs=False)
    got = eh.topk_candidates(torch.from_numpy(sources).to(dev), table, 100, hops=(1, 1), exclude=torch.from_numpy(ei).to(dev))
    _assert_same(got, _brute(eh, table, sources, 100, (1, 1), N, ei))
    got = eh.topk_candidates(torch.from_numpy(sources[:8]).to(dev), table, 100, hops=(2, 2), exclude=torch.from_numpy(ei).to(dev))
    _assert_same(got, _brute(eh, table, sources[:8], 100, (2, 2), N, ei))


def test_rows_do_not_depend_on_batching(ssa, dev, monkeypatch):
    N, ei = _graph('uniform3000')
    eh = _eh(ssa, h=2)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    exclude = torch.from_numpy(ei).to(dev)
    for S in (65, 200):
        src = torch.from_numpy(np.random.RandomState(S).randint(0, N, size=S)).to(dev)  # (duplicates included)
        ids, scores = eh.topk_candidates(src, table, 25, hops=(1, 2), exclude=exclude)
        again = eh.topk_candidates(src, table, 25, hops=(1, 2), exclude=exclude)
        assert torch.equal(again[0], ids) and torch.equal(again[1].view(torch.int32), scores.view(torch.int32))
        perm = torch.from_numpy(np.random.RandomState(S + 1).permutation(S)).to(dev)
        pi, ps = eh.topk_candidates(src[perm], table, 25, hops=(1, 2), exclude=exclude)
        assert torch.equal(pi, ids[perm]) and torch.equal(ps.view(torch.int32), scores[perm].view(torch.int32))
        parts = [eh.topk_candidates(src[a:b], table, 25, hops=(1, 2), exclude=exclude) for a, b in ((0, 1), (1, 33), (33, S))]
        assert torch.equal(torch.cat([p[0] for p in parts]), ids)
        assert torch.equal(torch.cat([p[1] for p in parts]).view(torch.int32), scores.view(torch.int32))
        # the key buffer split into blocks of 7 sources
        monkeypatch.setattr(ssa.engine, '_TOPK_KEY_BYTES', 7 * 8 * N)
        bi, bs = eh.topk_candidates(src, table, 25, hops=(1, 2), exclude=exclude)
        monkeypatch.undo()
        assert torch.equal(bi, ids) and torch.equal(bs.view(torch.int32), scores.view(torch.int32))


def test_inputs(ssa, dev):
    g = load_golden('g3_g4_ba40.npz')
    N, ei = int(g['num_nodes']), g['edge_index'].astype(np.int64)
    eh = _eh(ssa, h=2)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    src = torch.arange(-N, N, 3, dtype=torch.int64)
    d_ids, d_sc = eh.topk_candidates(src.to(dev), table, 7, exclude=torch.from_numpy(ei).to(dev))
    c_ids, c_sc = eh.topk_candidates(src, table, 7, exclude=torch.from_numpy(ei))   # CPU in, CPU out
    assert c_ids.device.type == 'cpu' and c_sc.device.type == 'cpu' and d_ids.device == dev
    assert torch.equal(c_ids, d_ids.cpu()) and torch.equal(c_sc, d_sc.cpu())
    # the reference's dict of int64 / int8 leaves (a torch.load-ed cache) gives the same rows as the SketchTable
    plain = {k: {'minhash': table[k]['minhash'].cpu().clone(), 'hll': table[k]['hll'].cpu().clone()} for k in range(3)}
    p_ids, p_sc = eh.topk_candidates(src, plain, 7, exclude=torch.from_numpy(ei))
    assert torch.equal(p_ids, c_ids) and torch.equal(p_sc, c_sc)
    e_ids, e_sc = eh.topk_candidates(src[:0], table, 7)
    assert e_ids.shape == (0, 7) and e_sc.shape == (0, 7)


def test_errors(ssa, dev):
    g = load_golden('g3_g4_ba40.npz')
    N, ei = int(g['num_nodes']), g['edge_index'].astype(np.int64)
    eh = _eh(ssa, h=2)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    ok = torch.tensor([0, 5], dtype=torch.int64)
    with pytest.raises(IndexError):
        eh.topk_candidates(torch.tensor([0, N]), table, 3)
    with pytest.raises(IndexError):
        eh.topk_candidates(torch.tensor([-N - 1]), table, 3)
    with pytest.raises(IndexError):
        eh.topk_candidates(ok, table, 3, exclude=torch.tensor([[0], [N]]))
    for k in (0, N + 1):
        with pytest.raises(ValueError):
            eh.topk_candidates(ok, table, k)
    for hops in ((0, 1), (1, 3), (3, 1)):
        with pytest.raises(ValueError):
            eh.topk_candidates(ok, table, 3, hops=hops)
    # device ids: reported late, as get_subgraph_features does
    eh.topk_candidates(torch.tensor([0, N], device=dev), table, 3)
    with pytest.raises(IndexError):
        eh.check_errors()
    eh.topk_candidates(ok.to(dev), table, 3, exclude=torch.tensor([[0], [-N - 1]], device=dev))
    with pytest.raises(IndexError):
        eh.check_errors()
    eh.check_errors()  # (reported once)
    eh.strict_bounds = True
    with pytest.raises(IndexError):
        eh.topk_candidates(torch.tensor([N], device=dev), table, 3)


def test_scores_pin_the_oracle(ssa, dev, regenerated_tables):
    from oracle import oracle
    g = load_golden('g3_g4_ba40.npz')
    N, ei = int(g['num_nodes']), g['edge_index'].astype(np.int64)
    eh = _eh(ssa, h=2)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    tabs = {k: {'minhash': table[k].mh_u32.cpu().numpy().view(np.uint32), 'hll': table[k].hll_u8.cpu().numpy()} for k in range(3)}
    prm = oracle_params(regenerated_tables[8])
    for hops in ((1, 1), (1, 2), (2, 2)):
        ids, scores = eh.topk_candidates(torch.arange(N), table, N, hops=hops)
        for u in range(N):
            valid = ids[u] >= 0
            links = np.stack([np.full(int(valid.sum()), u), ids[u][valid].numpy()], 1)
            _, dbg = oracle.pair_features(links, tabs, cards.cpu().numpy(), 2, prm, debug=True)
            np.testing.assert_allclose(scores[u][valid].numpy(), dbg['inter'][:, hops[0] - 1, hops[1] - 1], rtol=1e-5, atol=0)
            assert int(valid.sum()) == N - 1


# ---------------------------------------------------------------------------------------------------------------------------
# one-hop tables, awkward exclude lists, source counts around the 32-source staging block, an oracle pin at a generic shape
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_hop_tables(ssa, dev):
    N, ei = _graph('uniform3000')
    eh = _eh(ssa, h=1)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = _sources(N, 40, seed=21)
    src = torch.from_numpy(sources).to(dev)
    for excl in (None, ei):
        for k in (1, 17):
            want = _brute(eh, table, sources, k, (1, 1), N, excl)
            _assert_same(eh.topk_candidates(src, table, k, exclude=None if excl is None else torch.from_numpy(excl).to(dev)), want)
    with pytest.raises(ValueError):
        eh.topk_candidates(src, table, 3, hops=(1, 2))


def test_exclude_lists_with_negative_ids_duplicates_and_self_edges(ssa, dev):
    N, ei = _graph('uniform3000')
    eh = _eh(ssa, h=2)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = _sources(N, 30, seed=22)
    rng = np.random.RandomState(23)
    u = np.concatenate([np.repeat(sources, 8), sources])
    v = np.concatenate([rng.randint(0, N, size=8 * len(sources)), sources])       # ... and every source's self edge
    neg = rng.rand(len(u)) < 0.5
    ex = np.stack([np.where(neg, u - N, u), np.where(rng.rand(len(u)) < 0.5, v - N, v)])  # ids as negative as positive
    ex = np.where(ex < -N, ex + N, ex)
    ex = np.concatenate([ex, ex[:, ::3], ei[:, :500]], axis=1)                    # duplicate edges
    want = _brute(eh, table, sources, 25, (1, 2), N, ex)
    got = eh.topk_candidates(torch.from_numpy(sources).to(dev), table, 25, hops=(1, 2), exclude=torch.from_numpy(ex).to(dev))
    _assert_same(got, want)
    # the excluded partners are really gone: every pair of the list with a source in it is absent from that source's row
    ids = got[0].cpu().numpy()
    exw = np.where(ex < 0, ex + N, ex)
    for r, s in enumerate(np.where(sources < 0, sources + N, sources)):
        assert not np.isin(ids[r], exw[1][exw[0] == s]).any()


@pytest.mark.parametrize('S', [31, 32, 33])
def test_source_counts_around_the_staging_block(ssa, dev, S):
    N, ei = _graph('uniform3000')
    eh = _eh(ssa, h=2)
    table, _ = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    sources = np.random.RandomState(S).randint(-N, N, size=S).astype(np.int64)
    for hops in ((1, 1), (2, 1)):
        want = _brute(eh, table, sources, 12, hops, N, ei)
        _assert_same(eh.topk_candidates(torch.from_numpy(sources).to(dev), table, 12, hops=hops, exclude=torch.from_numpy(ei).to(dev)),
                     want)


def test_scores_pin_the_oracle_at_a_generic_shape(ssa, dev, regenerated_tables):
    """p = 6, P = 192, three hops: every score of a full ranking against the oracle's intersection estimate"""
    from oracle import oracle
    g = load_golden('g3_g4_ba40.npz')
    N, ei = int(g['num_nodes']), g['edge_index'].astype(np.int64)
    eh = _eh(ssa, h=3, p=6, P=192)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(ei).to(dev))
    tabs = {k: {'minhash': table[k].mh_u32.cpu().numpy().view(np.uint32), 'hll': table[k].hll_u8.cpu().numpy()} for k in range(4)}
    prm = oracle_params(regenerated_tables[6])
    for hops in ((3, 3), (1, 3), (2, 1)):
        ids, scores = eh.topk_candidates(torch.arange(N), table, N, hops=hops)
        for u in range(N):
            valid = ids[u] >= 0
            assert int(valid.sum()) == N - 1
            links = np.stack([np.full(N - 1, u), ids[u][valid].numpy()], 1)
            _, dbg = oracle.pair_features(links, tabs, cards.cpu().numpy(), 3, prm, debug=True)
            np.testing.assert_allclose(scores[u][valid].numpy(), dbg['inter'][:, hops[0] - 1, hops[1] - 1], rtol=1e-5, atol=0)
