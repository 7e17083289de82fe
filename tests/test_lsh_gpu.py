"""The LSH index over the MinHash tables (csrc/ss_lsh.hip, lsh.py) on the GPU: lsh_candidates against the numpy
restatement of its semantics (lsh_restatement.py: exact slice equality, no keys) -- rowptr, ids and bands exactly --, the verification
path under a 6-bit sort key, the max_bucket boundary, buckets at both ends of a band's sorted order, the invariances of a row, and
topk_links_lsh against the brute-force composition (score_links over the restated candidate pairs, sorted) and against topk_links.

The (graph, P, hop, rows, bands) cases were chosen on the CPU from oracle tables so that the restatement alone is non-trivial (at least
half the sources have a candidate, none has all N - 1); every test asserts that again on the tables it is given.

Written, not yet run on an MI355X (the host walk was rehearsed on the CPU with numpy stand-ins for the three launches); the kernels'
first runs there are those of test_lsh_planted_gpu.py (profiles/lsh_planted_tests.txt)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from score_restatement import raw_head
import lsh_restatement as restated

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


def _eh(ssa, h=2, P=128):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
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


def graph(name):
    if name == 'ba40':
        g = load_golden('g3_g4_ba40.npz')
        return int(g['num_nodes']), g['edge_index'].astype(np.int64)
    if name == 'uniform3000':
        n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
        return n, _uniform_graph(n, e_und, seed)
    return 50000, _power_law_graph()


def sources_of(name, N):
    if name == 'ba40':
        return np.arange(N, dtype=np.int64)
    return np.array(list(np.random.RandomState(11).choice(N, size=35, replace=False)) + [0, N - 1, -1], dtype=np.int64)


# (graph, P, hop, rows, bands): P in {128, 8, 256}, rows in {1, 2, 4}, hop in {1, 2} and bands below P // rows all occur
CASES = [('ba40', 128, 1, 4, None), ('ba40', 128, 1, 2, None), ('ba40', 128, 1, 1, 6), ('ba40', 8, 1, 1, None), ('ba40', 8, 1, 2, None),
         ('ba40', 8, 2, 4, None), ('ba40', 256, 1, 2, None), ('ba40', 256, 1, 4, None), ('ba40', 256, 2, 4, 3),
         ('uniform3000', 128, 1, 1, None), ('uniform3000', 128, 1, 2, None), ('uniform3000', 128, 2, 1, None),
         ('uniform3000', 128, 2, 2, 40), ('uniform3000', 8, 1, 1, None), ('uniform3000', 8, 2, 2, None), ('uniform3000', 8, 2, 1, 5),
         ('uniform3000', 256, 1, 2, None), ('uniform3000', 256, 2, 2, None), ('uniform3000', 256, 2, 1, 100),
         ('powerlaw50k', 128, 1, 2, None), ('powerlaw50k', 128, 2, 4, None), ('powerlaw50k', 8, 2, 2, None), ('powerlaw50k', 128, 1, 1, 16)]


def nontrivial(rowptr, N):
    sizes = np.diff(rowptr)
    return bool(np.mean(sizes > 0) >= 0.5 and sizes.max() < N - 1)


@pytest.fixture(scope='module')
def tables(ssa, dev):
    """(N, edge_index, table, cards, int64 MinHash rows per hop on the host) per (graph, P, h), built once; every test reads them only"""
    made = {}

    def get(name, P=128, h=2):
        if (name, P, h) not in made:
            N, ei = restated.trailing_graph(60, 40)[:2] if name == 'trailing' else graph(name)
            table, cards = _eh(ssa, h=h, P=P).build_hash_tables(N, torch.from_numpy(ei).to(dev))
            rows = {k: table[k]['minhash'].cpu().numpy() for k in range(1, h + 1)}
            made[(name, P, h)] = (N, ei, table, cards, rows)
        return made[(name, P, h)]

    return get


def _assert_same(got, want, where=None):
    rowptr, ids, bands = got
    assert rowptr.dtype == torch.int64 and ids.dtype == torch.int64 and bands.dtype == torch.int32
    if where is not None:
        assert rowptr.device == where and ids.device == where and bands.device == where
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(ids.cpu().numpy(), want[1])
    np.testing.assert_array_equal(bands.cpu().numpy(), want[2])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _rows(got):
    """the rows of a (rowptr, ids, bands) result as a list of (ids, bands) host arrays"""
    rowptr, ids, bands = (t.cpu().numpy() for t in got)
    return [(ids[a:b], bands[a:b]) for a, b in zip(rowptr[:-1], rowptr[1:])]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,P,hop,rows,bands', CASES)
def test_candidates_equal_the_restatement(ssa, dev, tables, name, P, hop, rows, bands):
    N, ei, table, cards, mh = tables(name, P)
    eh = _eh(ssa, P=P)
    src = sources_of(name, N)
    want = restated.lsh_candidates(mh[hop], src, rows, bands)
    assert nontrivial(want[0], N), 'a trivial expectation checks nothing'
    index = eh.build_lsh_index(table, hop=hop, rows=rows, bands=bands)
    b = P // rows if bands is None else bands
    assert (index.hop, index.rows, index.bands, index.num_nodes, index.num_perm, index.max_bucket) == (hop, rows, b, N, P, 1024)
    assert index.nbytes == 12 * b * N + 8 * b and index.keys.device == dev
    assert index.skipped_buckets.dtype == torch.int64 and index.skipped_buckets.device == dev
    np.testing.assert_array_equal(index.skipped_buckets.cpu().numpy(), restated.skipped_buckets(mh[hop], rows, bands))
    _assert_same(eh.lsh_candidates(torch.from_numpy(src).to(dev), index), want, dev)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,P,hop,rows,bands', [CASES[0], CASES[5], CASES[10], CASES[17], CASES[19], CASES[20]])
def test_verification_under_a_six_bit_key(ssa, dev, tables, name, P, hop, rows, bands):
    """64 keys for N nodes: every key bucket is full of false matches, only the comparison of the slices themselves keeps them out"""
    N, ei, table, cards, mh = tables(name, P)
    eh = _eh(ssa, P=P)
    src = sources_of(name, N)
    want = restated.lsh_candidates(mh[hop], src, rows, bands, max_bucket=N)
    assert nontrivial(want[0], N)
    index = eh.build_lsh_index(table, hop=hop, rows=rows, bands=bands, max_bucket=N, _key_bits=6)
    assert int(index.keys.max()) < 64 and int(index.keys.min()) >= 0 and int(index.skipped_buckets.sum()) == 0
    if N >= 3000:  # (a band of BA40 has too few distinct slices for that)
        assert all(len(torch.unique(index.keys[j])) == 64 for j in (0, index.bands - 1))
    _assert_same(eh.lsh_candidates(torch.from_numpy(src).to(dev), index), want, dev)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,rows', [(128, 4), (8, 1)])
def test_max_bucket_boundary(ssa, dev, tables, P, rows):
    """exactly m = 40 trailing nodes share one row (three rounds of a 16-lane walk): max_bucket = m lists them, m - 1 skips them"""
    N, ei, table, cards, mh = tables('trailing', P)
    m, b = 40, P // rows
    assert len(np.unique(mh[1][N - m:], axis=0)) == 1 and len(np.unique(mh[1], axis=0)) == N - m + 1
    eh = _eh(ssa, P=P)
    src = np.array([0, N - m, N - 1, 7, -2, N - 17], dtype=np.int64)
    for cap, listed in ((m, True), (m - 1, False)):
        index = eh.build_lsh_index(table, hop=1, rows=rows, max_bucket=cap)
        got = eh.lsh_candidates(torch.from_numpy(src).to(dev), index)
        _assert_same(got, restated.lsh_candidates(mh[1], src, rows, max_bucket=cap), dev)
        ids, shared = _rows(got)[2]  # node N - 1
        if listed:
            np.testing.assert_array_equal(ids, np.arange(N - m, N - 1))
            assert (shared == b).all()
        else:
            assert ids.size == 0
        skipped = index.skipped_buckets.cpu().numpy()
        np.testing.assert_array_equal(skipped, restated.skipped_buckets(mh[1], rows, max_bucket=cap))
        assert listed or (skipped >= 1).all()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,P,hop,rows', [('uniform3000', 128, 1, 1), ('ba40', 8, 1, 1)])
def test_buckets_at_both_ends_of_a_band(ssa, dev, tables, name, P, hop, rows):
    """the nodes at the first and at the last place of every band's sorted order as sources: equal ranges that touch 0 and N"""
    N, ei, table, cards, mh = tables(name, P)
    eh = _eh(ssa, P=P)
    index = eh.build_lsh_index(table, hop=hop, rows=rows)
    ends = torch.cat([index.perm[:, 0], index.perm[:, -1]]).to(torch.int64)
    groups = restated.band_groups(mh[hop], rows)
    first, last = index.perm[:, 0].cpu().numpy(), index.perm[:, -1].cpu().numpy()
    for at in (first, last):  # some band's end bucket has partners (and is not skipped): the walk there lists something
        assert any(1 < sizes[group[at[j]]] <= 1024 for j, (group, sizes) in enumerate(groups))
    want = restated.lsh_candidates(mh[hop], ends.cpu().numpy(), rows)
    assert nontrivial(want[0], N)
    _assert_same(eh.lsh_candidates(ends, index), want, dev)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_row_depends_on_its_source_only(ssa, dev, tables, monkeypatch):
    N, ei, table, cards, mh = tables('uniform3000')
    eh = _eh(ssa)
    hop, rows = 1, 2
    index = eh.build_lsh_index(table, hop=hop, rows=rows)
    rng = np.random.RandomState(3)
    # duplicates, self loops and negative ids in the exclude list: the edge list, a part of it again, loops, wrapped copies
    exclude = np.concatenate([ei, ei[:, ::3], np.stack([np.arange(50), np.arange(50)]), ei[:, :500] - N], axis=1)
    ex = torch.from_numpy(exclude).to(dev)
    S = 70
    src = rng.randint(-N, N, size=S).astype(np.int64)  # (duplicates and negative ids included)
    src[:3] = src[3:6]
    sd = torch.from_numpy(src).to(dev)
    for excl, ex_np in ((None, None), (ex, exclude)):
        want = restated.lsh_candidates(mh[hop], src, rows, exclude=ex_np)
        assert nontrivial(want[0], N)
        first = eh.lsh_candidates(sd, index, exclude=excl)
        _assert_same(first, want, dev)
        rows_first = _rows(first)
        perm = rng.permutation(S)
        for (a, b), (c, d) in zip(_rows(eh.lsh_candidates(sd[torch.from_numpy(perm).to(dev)], index, exclude=excl)), [rows_first[i] for i in perm]):
            assert np.array_equal(a, c) and np.array_equal(b, d)
        wrapped = torch.where(sd < 0, sd + N, sd)
        assert _same(eh.lsh_candidates(wrapped, index, exclude=excl), first)
        on_cpu = eh.lsh_candidates(torch.from_numpy(src), index, exclude=None if excl is None else excl.cpu())  # CPU in, CPU out
        assert all(t.device.type == 'cpu' for t in on_cpu) and _same(on_cpu, [t.cpu() for t in first])
        parts = [_rows(eh.lsh_candidates(sd[a:b], index, exclude=excl)) for a, b in ((0, 1), (1, 33), (33, S))]
        for (a, b), (c, d) in zip(sum(parts, []), rows_first):
            assert np.array_equal(a, c) and np.array_equal(b, d)
        # a tiny byte budget: blocks of a few sources for the counts, of some hundred entries for the fill
        monkeypatch.setattr(ssa.lsh, '_LSH_BLOCK_BYTES', 12 * index.bands * 7)
        split = eh.lsh_candidates(sd, index, exclude=excl)
        monkeypatch.undo()
        assert _same(split, first)
        # min_bands = 2 is the min_bands = 1 result filtered
        two = eh.lsh_candidates(sd, index, exclude=excl, min_bands=2)
        _assert_same(two, restated.lsh_candidates(mh[hop], src, rows, exclude=ex_np, min_bands=2), dev)
        assert 0 < two[1].numel() < first[1].numel()
        for (a, b), (c, d) in zip(_rows(two), rows_first):
            assert np.array_equal(a, c[d >= 2]) and np.array_equal(b, d[d >= 2])
    none = eh.lsh_candidates(sd[:0], index, exclude=ex)
    assert none[0].tolist() == [0] and none[1].shape == (0,) and none[2].shape == (0,)
    _assert_same(none, restated.lsh_candidates(mh[hop], src[:0], rows), dev)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.asarray(a, dtype=np.float32)
    return np.where(a == 0, np.float32(0), a).view(np.int32)  # +-0 compare equal, every other value bit for bit


def _head(ssa, h, normalised, seed):
    nf = h * (h + 2)
    return ssa.StructureHead(normalised=normalised, **raw_head(2 * nf if normalised else nf, seed))


def _degrees(N, ei, sources):
    """float32 [N] degrees of the edge list without the edges of nodes 3, N - 2 and the first source: those three have degree 0"""
    drop = np.array([3, N - 2, int(sources[0]) % N])
    keep = ~(np.isin(ei[0], drop) | np.isin(ei[1], drop))
    return np.bincount(ei[0][keep], minlength=N).astype(np.float32)


def _brute_force(eh, table, cards, head, deg, sources, N, k, want, dev):
    """score_links over the restated candidate pairs, each row sorted by (score desc, id asc) and padded"""
    rowptr, cand, _ = want
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


@pytest.mark.parametrize('name,rows', [('uniform3000', 2), ('ba40', 4)])
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('normalised', [False, True])
def test_topk_links_lsh_equals_the_brute_force_composition(ssa, dev, tables, name, rows, h, normalised):
    N, ei, table, cards, mh = tables(name, 128, 3)
    sub, c = {k: table[k] for k in range(h + 1)}, cards[:, :h]
    eh = _eh(ssa, h=h)
    src = sources_of(name, N)
    head = _head(ssa, h, normalised, 30 + 2 * h + int(normalised))
    deg = torch.from_numpy(_degrees(N, ei, src)).to(dev) if normalised else None
    index = eh.build_lsh_index(sub, hop=1, rows=rows)
    sd = torch.from_numpy(src).to(dev)
    for excl in (None, ei):
        want = restated.lsh_candidates(mh[1], src, rows, exclude=excl)
        sizes = np.diff(want[0])
        assert nontrivial(want[0], N)
        mid = int(np.median(sizes[sizes > 0])) + 1
        assert (sizes < mid).any() and (sizes >= mid).any()  # k = mid: some rows end in padding, some are cut
        for k in (1, mid, N):
            ids, scores = eh.topk_links_lsh(sd, sub, c, k, head, index, degrees=deg, exclude=None if excl is None else torch.from_numpy(excl).to(dev))
            assert ids.shape == (len(src), k) and ids.dtype == torch.int64 and scores.dtype == torch.float32 and ids.device == dev
            w_ids, w_scores = _brute_force(eh, sub, c, head, deg, src, N, k, want, dev)
            np.testing.assert_array_equal(ids.cpu().numpy(), w_ids)
            np.testing.assert_array_equal(_bits(scores.cpu().numpy()), _bits(w_scores))
            if k == N:
                assert (ids[:, -1] == -1).all() and torch.isinf(scores[:, -1]).all()
    # min_bands and a split walk reach the ranking too
    two = eh.topk_links_lsh(sd, sub, c, 5, head, index, degrees=deg, min_bands=2)
    w = _brute_force(eh, sub, c, head, deg, src, N, 5, restated.lsh_candidates(mh[1], src, rows, min_bands=2), dev)
    np.testing.assert_array_equal(two[0].cpu().numpy(), w[0])
    np.testing.assert_array_equal(_bits(two[1].cpu().numpy()), _bits(w[1]))


def test_topk_links_lsh_rows_do_not_depend_on_the_split(ssa, dev, tables, monkeypatch):
    N, ei, table, cards, mh = tables('uniform3000', 128, 3)
    h = 2
    sub, c = {k: table[k] for k in range(h + 1)}, cards[:, :h]
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, False, 4)
    index = eh.build_lsh_index(sub, hop=2, rows=2)
    src = torch.from_numpy(np.random.RandomState(9).randint(-N, N, size=50)).to(dev)
    ex = torch.from_numpy(ei).to(dev)
    first = eh.topk_links_lsh(src, sub, c, 10, head, index, exclude=ex)
    assert bool((first[0][:, 0] >= 0).float().mean() >= 0.5)
    monkeypatch.setattr(ssa.lsh, '_LSH_BLOCK_BYTES', 12 * index.bands * 7)
    split = eh.topk_links_lsh(src, sub, c, 10, head, index, exclude=ex)
    monkeypatch.undo()
    assert torch.equal(split[0], first[0]) and torch.equal(split[1].view(torch.int32), first[1].view(torch.int32))
    on_cpu = eh.topk_links_lsh(src.cpu(), sub, c, 10, head, index, exclude=ex.cpu())
    assert on_cpu[0].device.type == 'cpu' and torch.equal(on_cpu[0], first[0].cpu()) and torch.equal(on_cpu[1], first[1].cpu())
    empty = eh.topk_links_lsh(src[:0], sub, c, 10, head, index)
    assert empty[0].shape == (0, 10) and empty[1].shape == (0, 10) and empty[0].dtype == torch.int64 and empty[1].dtype == torch.float32


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalised', [False, True])
def test_rows_are_a_subset_of_topk_links(ssa, dev, tables, normalised):
    N, ei, table, cards, mh = tables('uniform3000', 128, 3)
    h = 2
    sub, c = {k: table[k] for k in range(h + 1)}, cards[:, :h]
    eh = _eh(ssa, h=h)
    src = sources_of('uniform3000', N)
    sd = torch.from_numpy(src).to(dev)
    head = _head(ssa, h, normalised, 12)
    deg = torch.from_numpy(_degrees(N, ei, src)).to(dev) if normalised else None
    ex = torch.from_numpy(ei).to(dev)
    index = eh.build_lsh_index(sub, hop=2, rows=2)
    ids, scores = eh.topk_links_lsh(sd, sub, c, 50, head, index, degrees=deg, exclude=ex)
    full_ids, full_scores = eh.topk_links(sd, sub, c, N - 1, head, degrees=deg, exclude=ex)
    ids, scores, full_ids, full_scores = (t.cpu().numpy() for t in (ids, scores, full_ids, full_scores))
    assert (ids[:, 0] >= 0).mean() >= 0.5
    for r in range(len(src)):
        score_of = dict(zip(full_ids[r][full_ids[r] >= 0].tolist(), _bits(full_scores[r][full_ids[r] >= 0]).tolist()))
        mine = ids[r] >= 0
        assert all(score_of.get(v) == b for v, b in zip(ids[r][mine].tolist(), _bits(scores[r][mine]).tolist()))
        assert np.all(np.diff(scores[r][mine]) <= 0)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_ids_out_of_range(ssa, dev, tables):
    N, ei, table, cards, mh = tables('ba40')
    eh = _eh(ssa)
    head = _head(ssa, 2, False, 9)
    index = eh.build_lsh_index(table, hop=1, rows=2)
    good = eh.lsh_candidates(torch.tensor([0, 5], device=dev), index)
    good_top = eh.topk_links_lsh(torch.tensor([0, 5], device=dev), table, cards, 3, head, index)
    # device ids: reported late, as topk_links reports them; the bad source's row is empty / padding, the other rows are untouched
    got = eh.lsh_candidates(torch.tensor([0, N, 5], device=dev), index)
    with pytest.raises(IndexError):
        eh.check_errors()
    rows, want = _rows(got), _rows(good)
    assert rows[1][0].size == 0 and np.array_equal(rows[0][0], want[0][0]) and np.array_equal(rows[2][0], want[1][0])
    ids, scores = eh.topk_links_lsh(torch.tensor([0, -N - 1, 5], device=dev), table, cards, 3, head, index)
    with pytest.raises(IndexError):
        eh.check_errors()
    assert (ids[1] == -1).all() and torch.isinf(scores[1]).all()
    assert torch.equal(ids[[0, 2]], good_top[0]) and torch.equal(scores[[0, 2]], good_top[1])
    eh.lsh_candidates(torch.tensor([0, 5], device=dev), index, exclude=torch.tensor([[0], [-N - 1]], device=dev))
    with pytest.raises(IndexError):
        eh.check_errors()
    eh.check_errors()  # (reported once)
    with pytest.raises(IndexError):  # CPU ids: at once
        eh.lsh_candidates(torch.tensor([0, N]), index)
    eh.strict_bounds = True
    with pytest.raises(IndexError):
        eh.lsh_candidates(torch.tensor([N], device=dev), index)
    with pytest.raises(IndexError):
        eh.topk_links_lsh(torch.tensor([N], device=dev), table, cards, 3, head, index)
    eh.strict_bounds = False
    assert _same(eh.lsh_candidates(torch.tensor([0, N, 5], device=dev), index), got)
