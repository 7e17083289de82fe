"""Every kernel that ends in the HLL++ estimator (csrc/ss_common.hpp hll_estimate / bias_of_6nn, csrc/ss_pair_math.hpp
intersection_estimate) on the planted inputs of tests/hll_planted.py: rows on either side of each of its decisions -- the last
linear-counting row and the first one off it, the two rows nearest to e = 5m, the clamped top window, a row next to a raw entry, the empty
and the saturated union, match == P with V == M and V == 0 -- through ss_hll_count at every precision and table length, the pair query
(ordinary, grouped and run-aware kernels, fast and generic shapes), the masked query, the one-vs-all scans (topk_candidates, topk_links,
rank_links), score_links, and the build kernels (first hop, table hop, fused stage, hub kernels, hll_prop, update_hash_tables).

Bars (all derived, tests/hll_planted.py): integers and tables equal; a planted row's harmonic sum is exact in fp32 in any order, so its
estimate -- linear counting, bias-corrected or raw -- equals the numpy restatement estimate32 BIT FOR BIT, and an intersection equals
fl(fl(match / P) * estimate32); rows whose sum is not exact (unions of two different planted rows, graph rows with large registers) are
held to the oracle at the project's RTOL; features to the oracle at RTOL / ATOL of test_gpu_parity.py."""
import functools
from argparse import Namespace
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import hll_planted as hp
from hll_planted import F32
from rank_restatement import rank_counts

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-4  # tests/test_gpu_parity.py
FAST_SHAPES = ((64, 8), (128, 8), (192, 8), (256, 8))
GENERIC_SHAPES = ((8, 4), (192, 6), (128, 16), (2048, 8))


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _setup(p, n_tbl):
    t = hp.tables(p, n_tbl)
    return t, hp.params(t), hp.cases(p, t)


def _eh(ssa, t, h=2, P=128, **kw):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=t.p, minhash_num_perm=P, floor_sf=False, use_zero_one=True), **kw)
    eh.hll_tables = t  # (installed as test_bias_lookup_with_unsorted_and_short_tables does)
    return eh


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _assert_bits(got, want, what):
    """fp32 arrays equal bit for bit (-0.0 == +0.0 is not needed anywhere here); the message carries the largest ulp distance"""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    if bad.size:
        d = np.abs(_bits(got).ravel()[bad].astype(np.int64) - _bits(want).ravel()[bad].astype(np.int64))
        i = bad[int(np.argmax(d))]
        raise AssertionError(f'{what}: {bad.size} of {got.size} values differ, largest distance {int(d.max())} ulp at {int(i)}: '
                             f'got {got.ravel()[i]!r}, want {want.ravel()[i]!r}')


def _estimates(prm, regs):
    """(estimate32 fp32 [n], branch [n], exact bool [n]) of register rows, memoised on (V, S)"""
    V, S, exact = hp.stats(regs)
    memo, out, br = {}, np.zeros(len(regs), F32), np.zeros(len(regs), np.int32)
    for i in range(len(regs)):
        key = (int(V[i]), float(S[i]))
        if key not in memo:
            memo[key] = hp.estimate32(prm, *key)
        out[i], br[i] = memo[key]
    return out, br, np.asarray(exact)


def _check_counts(got, regs, t, prm, what):
    """cardinalities of register rows: bit for bit where the harmonic sum is exact, the oracle at RTOL elsewhere; estimate_ref and
    estimate64 at RTOL on the exact rows with an estimate >= 1.  -> (branch, exact)"""
    from oracle import oracle
    got = np.asarray(got, dtype=F32)
    want, br, exact = _estimates(prm, regs)
    _assert_bits(got[exact], want[exact], what)
    if (~exact).any():
        np.testing.assert_allclose(got[~exact], oracle.hll_count(regs[~exact], hp.oracle_params(t)), rtol=RTOL, atol=0, err_msg=what)
    V, S, _ = hp.stats(regs)
    seen = set()
    for i in np.flatnonzero(exact & (want >= 1)):
        key = (int(V[i]), float(S[i]))
        if key in seen:
            continue
        seen.add(key)
        for other in (hp.estimate_ref(prm, *key)[0], hp.estimate64(prm, *key)[0]):
            assert abs(float(got[i]) - float(other)) <= RTOL * abs(float(other)), (what, i, float(got[i]), float(other))
    return br, exact


# ---- ss_hll_count -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_tbl', hp.TABLE_LENGTHS)
@pytest.mark.parametrize('p', hp.PRECISIONS)
def test_hll_count_takes_the_right_branch_on_every_planted_row(ssa, dev, p, n_tbl):
    """every case in every zero layout, at row counts 1, rows_per_block - 1, rows_per_block + 1 and all; p = 4 and 5 have fewer lanes
    than rows per lane group, p > 10 reads the linear-counting table from global memory"""
    t, prm, cs = _setup(p, n_tbl)
    eh = _eh(ssa, t)
    assert eh._params(dev).struct.lc_min_zeros == prm.lc_min_zeros and eh._params(dev).struct.n_tbl == prm.n_tbl
    planted = np.stack([hp.row(p, c.V, c.counts, layout, seed=i) for layout in hp.ZERO_LAYOUTS for i, c in enumerate(cs.values())])
    SG = min(64, (1 << p) // 16)
    rows_per_block = 4 * (64 // SG) * 4  # csrc/ss_count.hip: wavefronts * lane groups * kCountRows
    n_all = max(rows_per_block + 1, len(planted))
    regs = planted[np.arange(n_all) % len(planted)]
    dregs = torch.from_numpy(regs).to(dev)
    for n in sorted({1, rows_per_block - 1, rows_per_block + 1, n_all}):
        got = eh.hll_count(dregs[:n]).cpu().numpy()
        br, exact = _check_counts(got, regs[:n], t, prm, f'p={p} n_tbl={n_tbl} n={n}')
        assert exact.all()
    assert set(br.tolist()) == {0, 1, 2}
    got = got[:len(cs)]
    for i, (name, c) in enumerate(cs.items()):
        assert _bits(got[i]) == _bits(c.value), (name, got[i], c.value)


def _tie_points(prm):
    """fp32 estimates exactly midway between raw[w - 1] and raw[w + 5] whose two fp32 squared distances are EQUAL (checked here, in
    numpy): the window may start at w - 1 or at w, and the documented rule -- ties to the lower index -- says w - 1"""
    out = []
    for w in range(1, prm.n_tbl - 5):
        lo, hi = prm.raw[w - 1], prm.raw[w + 5]
        e = F32((lo + hi) * F32(0.5))
        if (e - lo) * (e - lo) == (e - hi) * (e - hi) and lo < e < hi:
            out.append((w, e))
    return out


@pytest.mark.parametrize('n_tbl', hp.TABLE_LENGTHS)
@pytest.mark.parametrize('p', [4, 8, 11, 16])
def test_bias_lookup_on_planted_estimates(ssa, dev, p, n_tbl):
    """_estimate_bias and _refine_hll_count_estimate on estimates below raw[0] and above raw[n - 1], exactly on raw entries, on window
    ties, at 5m and its two fp32 neighbours, and in the clamped top window (reached here on the shipped table too)"""
    t, prm, _ = _setup(p, n_tbl)
    eh = _eh(ssa, t)
    raw, five_m = prm.raw, prm.five_m
    ties = _tie_points(prm)
    es = [F32(0.5) * raw[0], np.nextafter(raw[0], F32(0)), raw[0], raw[prm.n_tbl // 2], raw[-1], np.nextafter(raw[-1], F32(np.inf)),
          F32(2) * raw[-1], np.nextafter(five_m, F32(0)), five_m, np.nextafter(five_m, F32(np.inf)), raw[-4], np.nextafter(raw[-4], F32(np.inf)),
          F32(0.5) * (raw[-4] + raw[-3]), raw[5], raw[min(6, prm.n_tbl - 1)]] + [e for _, e in ties]
    es = np.array(es, dtype=F32)
    for w, e in ties:
        assert hp.window32(prm, e) == w - 1, 'a stable argsort resolves the tie to the lower index'
    want_b = np.array([hp.bias32(prm, e) for e in es], dtype=F32)
    want_r = np.array([F32(e - b) if e <= five_m else e for e, b in zip(es, want_b)], dtype=F32)
    d = torch.from_numpy(es).to(dev)
    _assert_bits(eh._estimate_bias(d).cpu().numpy(), want_b, f'_estimate_bias p={p} n_tbl={n_tbl}')
    refined = eh._refine_hll_count_estimate(d.clone()).cpu().numpy()
    _assert_bits(refined, want_r, f'_refine_hll_count_estimate p={p} n_tbl={n_tbl}')
    ref = np.array([F32(e - hp.bias_ref(prm, e)) if e <= five_m else e for e in es], dtype=F32)
    r64 = np.array([e - hp.bias64(prm, e) if e <= five_m else e for e in es.astype(np.float64)])
    big = np.abs(ref) >= 1
    np.testing.assert_allclose(refined[big], ref[big], rtol=RTOL, atol=0)
    # (on a tie of the fp32 distances fp64 may see the other entry nearer: compared where both pick the same window)
    same = np.array([set(np.argsort((float(e) - prm.raw.astype(np.float64)) ** 2, kind='stable')[:6]) == set(range(hp.window32(prm, e), hp.window32(prm, e) + 6))
                     for e in es])
    assert same[:13].sum() >= 8
    np.testing.assert_allclose(refined[big & same], r64[big & same], rtol=RTOL, atol=0)
    assert hp.window32(prm, es[0]) == 0 and hp.window32(prm, raw[-1]) == hp.window32(prm, es[6]) == prm.n_tbl - 6
    if n_tbl in (256, 512):
        assert ties, 'an evenly spaced table has exact ties'


# ---- the link queries ---------------------------------------------------------------------------------------------------------------
class Planted(object):
    """the planted hop tables of one (P, p, table length, hop count) on the device, and what numpy says of every link"""

    def __init__(self, ssa, dev, P, p, n_tbl=None, h=2):
        from oracle import oracle
        extra_links = 1000 if p <= 11 else 75  # (rows of 64 KB at p = 16)
        self.P, self.p, self.h = P, p, h
        self.t, self.prm, self.cs = _setup(p, n_tbl)
        qt = hp.query_table(p, P, self.cs)
        hops = [qt]
        for _ in range(h - 1):
            nxt = hp.second_hop(hops[-1] if len(hops) == 1 else SimpleNs(hops[-1], qt))
            hops.append(nxt)
        self.qt, self.N = qt, qt.N
        self.mh, self.hll = [x.mh for x in hops], [x.hll for x in hops]
        rng = np.random.RandomState(P + p)
        self.links = np.concatenate([qt.links, rng.randint(0, qt.N, size=(extra_links, 2))]).astype(np.int64)
        assert len(self.links) % 16 != 0, 'a ragged link count'
        self.oprm = hp.oracle_params(self.t)
        self.cards = np.stack([oracle.hll_count(x, self.oprm) for x in self.hll], axis=1).astype(F32)
        self.eh = _eh(ssa, self.t, h=h, P=P)
        self.table = {0: None}
        for k in range(h):
            self.table[k + 1] = {'minhash': torch.from_numpy(self.mh[k].view(np.int32)).to(dev), 'hll': torch.from_numpy(self.hll[k]).to(dev)}
        self.dcards = torch.from_numpy(self.cards).to(dev)
        self.dlinks = torch.from_numpy(self.links).to(dev)
        self.want = hp.expected_pairs(self.prm, P, self.mh, self.hll, self.links)
        otab = {k + 1: {'minhash': self.mh[k], 'hll': self.hll[k]} for k in range(h)}
        self.ofeat, self.odbg = oracle.pair_features(self.links, otab, self.cards, h, self.oprm, debug=True)
        assert np.array_equal(self.odbg['branch'], self.want.branch)

    def check_debug(self, dbg, what):
        want = self.want
        assert np.array_equal(dbg['match'].cpu().numpy(), want.match), (what, 'match')
        assert np.array_equal(dbg['zeros'].cpu().numpy(), want.zeros), (what, 'zeros')
        inter = dbg['inter'].cpu().numpy()
        _assert_bits(inter[want.exact], want.inter[want.exact], f'{what}: intersections of exact unions')
        np.testing.assert_allclose(inter, self.odbg['inter'], rtol=RTOL, atol=0, err_msg=what)
        return inter


class SimpleNs(object):
    """a further hop's rows with the planted table's block structure (second_hop permutes by position)"""

    def __init__(self, hop, qt):
        self.hll, self.mh, self.C, self.N = hop.hll, hop.mh, qt.C, qt.N


@functools.lru_cache(maxsize=None)
def _planted(ssa, dev, P, p, n_tbl=None, h=2):
    return Planted(ssa, dev, P, p, n_tbl, h)


QUERY_CASES = [(P, p, None, 2) for P, p in FAST_SHAPES + GENERIC_SHAPES] + [(128, 8, 257, 2), (128, 8, 6, 2), (128, 8, 512, 3), (8, 4, 512, 2)]


@pytest.mark.parametrize('P,p,n_tbl,h', QUERY_CASES)
def test_pair_query_on_planted_tables(ssa, dev, monkeypatch, P, p, n_tbl, h):
    """ss_pair_features with its debug outputs, then the same links through the grouped entry point (GROUP_LINKS_MIN lowered to the link
    count; (0, v) repeats its source) and, for the fast shapes, through both kernels behind it"""
    pl = _planted(ssa, dev, P, p, n_tbl, h)
    eh, want = pl.eh, pl.want
    feats, dbg = eh._pair_kernel(pl.dlinks, pl.table, pl.dcards, want_debug=True)
    pl.check_debug(dbg, f'P={P} p={p} n_tbl={n_tbl} h={h}')
    assert set(np.unique(want.branch[want.exact]).tolist()) == {0, 1, 2}
    full = want.match == P
    assert (full & (want.zeros == pl.prm.m)).any() and (full & (want.zeros == 0)).any(), 'match == P with V == M and with V == 0'
    f = feats.cpu().numpy()
    np.testing.assert_allclose(f, pl.ofeat, rtol=RTOL, atol=ATOL)
    monkeypatch.setattr(ssa.knobs, 'GROUP_LINKS_MIN', 0)
    assert torch.equal(eh.get_subgraph_features(pl.dlinks, pl.table, pl.dcards), feats)
    monkeypatch.setattr(ssa.knobs, 'GROUP_LINKS_MIN', len(pl.links))
    for mode in (True, 'auto', False):
        eh.group_links = mode
        assert torch.equal(eh.get_subgraph_features(pl.dlinks, pl.table, pl.dcards), feats), mode
    if (P, p) in FAST_SHAPES:
        H = ssa.hashing
        lib, prm = ssa._native.lib(), eh._params(dev)
        mh_ptrs = (c_void_p * h)(*[pl.table[k]['minhash'].data_ptr() for k in range(1, h + 1)])
        hl_ptrs = (c_void_p * h)(*[pl.table[k]['hll'].data_ptr() for k in range(1, h + 1)])
        order = H.group_links_by_source(pl.dlinks, pl.N, dev)
        for which in (0, 1):
            for o in (order, None):
                out = torch.full_like(feats, 7.0)
                rc = lib.ss_pair_features_grouped_kernel(which, H._ptr(pl.dlinks), H._ptr(o), len(pl.links), pl.N, h, mh_ptrs, P, hl_ptrs,
                                                         H._ptr(pl.dcards), pl.dcards.stride(0), byref(prm.struct), eh._flags(), None,
                                                         H._ptr(out), None, H._stream(dev))
                assert rc == 0 and torch.equal(out, feats), (which, o is not None)


@pytest.mark.parametrize('P,p,n_tbl', [(128, 8, None), (128, 8, 257), (64, 8, None), (256, 8, 512), (8, 4, None), (192, 6, None)])
def test_masked_query_keeps_the_planted_estimates(ssa, dev, P, p, n_tbl):
    """the masked kernel's own pair finish: with an edge list that holds none of the links (edges between other rows) the mask
    removes nothing, and match, zeros and every feature must be the plain query's, bit for bit"""
    pl = _planted(ssa, dev, P, p, n_tbl, 2)
    eh = pl.eh
    feats, dbg = eh._pair_kernel(pl.dlinks, pl.table, pl.dcards, want_debug=True)
    pl.check_debug(dbg, 'plain')
    a = pl.qt.pairs[:, 0]
    between = np.stack([a[:-1], a[1:]])  # a rows of neighbouring pairs: no link joins them
    linked = set(map(tuple, pl.links.tolist())) | set(map(tuple, pl.links[:, ::-1].tolist()))
    between = between[:, [tuple(e) not in linked for e in between.T.tolist()]]
    assert between.shape[1] > len(a) // 2
    for ei in (between, between[:, ::2]):
        got, mdbg = eh.get_subgraph_features(pl.dlinks, pl.table, pl.dcards, mask_target=torch.from_numpy(ei).to(dev), return_debug=True)
        assert not bool(mdbg['masked'].any())
        assert np.array_equal(mdbg['match'].cpu().numpy(), pl.want.match) and np.array_equal(mdbg['zeros'].cpu().numpy(), pl.want.zeros)
        assert torch.equal(got, feats), ei.shape


def _first_feature_head(ssa, h):
    """a fixed-weight head whose score IS the first feature, I[1, 1] >= 0, bit for bit: W' has the single entry W'[0, 0] = 1, t' = 0,
    w2 = e_0, no bias -- every product is exact and every other term a zero"""
    nf = h * (h + 2)
    w = torch.zeros(nf, nf)
    w[0, 0] = 1.0
    e0 = torch.zeros(nf)
    e0[0] = 1.0
    head = ssa.StructureHead(weight=w, bias=torch.zeros(nf), bn_weight=torch.ones(nf), bn_bias=torch.zeros(nf), bn_mean=torch.zeros(nf),
                             bn_var=torch.ones(nf), bn_eps=0.0, out_weight=e0, out_bias=None)
    assert head.w1[0, 0] == 1.0 and np.count_nonzero(head.w1) == 1 and not head.shift.any() and head.b2 == 0.0
    return head


@pytest.mark.parametrize('P,p,n_tbl', [(128, 8, None), (128, 8, 257), (192, 6, None), (8, 4, 512)])
def test_one_vs_all_scans_on_planted_tables(ssa, dev, P, p, n_tbl):
    """topk_candidates from source 0 (every case through a union with nothing) and from a split row, for every pair of hops; then the
    structure head fixed so that the score is I[1, 1] itself: score_links, topk_links and rank_links (expected counts from
    rank_restatement on the planted scores), with the tables as built and with the two hops swapped"""
    pl = _planted(ssa, dev, P, p, n_tbl, 2)
    eh, N = pl.eh, pl.N
    sources = np.array([0, int(pl.qt.pairs[3, 0]), int(pl.qt.pairs[-1, 1])], dtype=np.int64)
    all_links = np.stack([np.repeat(sources, N), np.tile(np.arange(N, dtype=np.int64), len(sources))], 1)
    want = hp.expected_pairs(pl.prm, P, pl.mh, pl.hll, all_links)
    _, dbg = eh._pair_kernel(torch.from_numpy(all_links).to(dev), pl.table, pl.dcards, want_debug=True)
    inter = dbg['inter'].cpu().numpy()
    assert np.array_equal(dbg['zeros'].cpu().numpy(), want.zeros) and np.array_equal(dbg['match'].cpu().numpy(), want.match)
    _assert_bits(inter[want.exact], want.inter[want.exact], 'pair kernel, one source against all')
    assert want.exact[:1 + pl.qt.C].all(), 'source 0 against a case row: the union is the planted row'
    truth = inter.reshape(len(sources), N, 2, 2)  # (exact entries: numpy's; the others: the pair kernel's, held to the oracle above)
    dsrc = torch.from_numpy(sources).to(dev)
    for k1 in (1, 2):
        for k2 in (1, 2):
            ids, scores = eh.topk_candidates(dsrc, pl.table, N - 1, hops=(k1, k2))
            ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
            for s, u in enumerate(sources):
                assert sorted(ids[s].tolist()) == [v for v in range(N) if v != u]
                _assert_bits(scores[s], truth[s, ids[s], k1 - 1, k2 - 1], f'topk_candidates hops=({k1}, {k2}) source {u}')
                key = np.lexsort((ids[s], -scores[s].astype(np.float64)))
                assert np.array_equal(key, np.arange(N - 1)), 'score descending, id ascending'
    head = _first_feature_head(ssa, 2)
    for swapped in (False, True):
        table = {0: None, 1: pl.table[2], 2: pl.table[1]} if swapped else pl.table
        cards = pl.dcards.flip(1).contiguous() if swapped else pl.dcards
        row = truth[:, :, 1, 1] if swapped else truth[:, :, 0, 0]  # s(u, v) = I[1, 1] of the tables as given
        sc = eh.score_links(torch.from_numpy(all_links).to(dev), table, cards, head).cpu().numpy().reshape(len(sources), N)
        _assert_bits(sc, row, f'score_links swapped={swapped}')
        ids, scores = eh.topk_links(dsrc, table, cards, N - 1, head)
        ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        for s, u in enumerate(sources):
            assert sorted(ids[s].tolist()) == [v for v in range(N) if v != u]
            _assert_bits(scores[s], row[s, ids[s]], f'topk_links swapped={swapped} source {u}')
        rl = np.concatenate([np.stack([np.full(N, u), np.arange(N)], 1) for u in sources]).astype(np.int64)[::3]
        greater, equal = eh.rank_links(torch.from_numpy(rl).to(dev), table, cards, head)
        index = {int(u): s for s, u in enumerate(sources)}
        wg, we = rank_counts(lambda q, u: row[index[u]], rl, N)
        assert np.array_equal(greater.cpu().numpy(), wg) and np.array_equal(equal.cpu().numpy(), we), f'rank_links swapped={swapped}'


# ---- the build kernels ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hood():
    return hp.neighbourhoods()


@functools.lru_cache(maxsize=None)
def _oracle_build(n_tbl, with_extra):
    from oracle import oracle
    nb = _hood()
    t, prm, _ = _setup(8, n_tbl)
    ei = np.concatenate([nb.edge_index, nb.extra_edge], axis=1) if with_extra else nb.edge_index
    tab, cards = oracle.build_hash_tables(nb.n, ei, 2, 128, hp.oracle_params(t))
    return ei, tab, cards


def _check_build(table, cards, n_tbl, with_extra, what):
    """hop-1 and hop-2 tables equal to the oracle's; cards by _check_counts; the planted targets (and, at hop 2, their out-neighbours)
    sit on the intended side of lc_min_zeros with an exact sum, so they are compared bit for bit"""
    nb = _hood()
    t, prm, _ = _setup(8, n_tbl)
    _, otab, _ = _oracle_build(n_tbl, with_extra)
    c = cards.cpu().numpy()
    for k in (1, 2):
        hll = table[k].hll_u8.cpu().numpy() if hasattr(table[k], 'hll_u8') else table[k]['hll'].cpu().numpy().view(np.uint8)
        mh = table[k].mh_u32.cpu().numpy() if hasattr(table[k], 'mh_u32') else table[k]['minhash'].cpu().numpy()
        assert np.array_equal(hll, otab[k]['hll']), (what, k, 'hll')
        assert np.array_equal(mh.astype(np.uint32) if mh.dtype != np.int32 else mh.view(np.uint32), otab[k]['minhash']), (what, k, 'minhash')
        br, exact = _check_counts(c[:, k - 1], hll, t, prm, f'{what} hop {k} cards')
        last = nb.targets[-1]
        for tg, count in nb.want_registers.items():
            if tg == last and with_extra:
                count += 1
            rows = [tg] if k == 1 else nb.out_nodes[tg]
            for r in rows:
                assert exact[r] and int((hll[r] == 0).sum()) == 256 - count and br[r] == (0 if count == 147 else 1), (what, k, r)
        for r in ([nb.big] if k == 1 else nb.big_out):  # (the clamped top window of the tables of 257 and 512 entries)
            assert exact[r] and br[r] == 1 and np.array_equal(hll[r], otab[1]['hll'][nb.big]), (what, k, r)
        assert {0, 1} <= set(br.tolist())


BUILD_TABLES = (None, 6, 257, 512)  # (None: the 200 entries as shipped; 257 and 512: raw / bias stay in global memory in the fused stage)


@pytest.mark.parametrize('threshold', [None, 1024, 64])
@pytest.mark.parametrize('n_tbl', BUILD_TABLES)
def test_build_on_planted_neighbourhoods(ssa, dev, monkeypatch, n_tbl, threshold):
    """build_hash_tables with the fused stage on and off.  threshold None: the default (128: the targets, in-degree about 160, are hub
    rows); 1024: every row regular -- the first hop's rows that leave the linear-counting range read raw / bias from global memory;
    64: the out-neighbour rows stay regular, the targets go through the hub kernels"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    nb = _hood()
    t, _, _ = _setup(8, n_tbl)
    ei = torch.from_numpy(nb.edge_index).to(dev)
    indeg = np.bincount(nb.edge_index[1], minlength=nb.n)
    assert all(128 < indeg[tg] < 1024 for tg in nb.targets)
    for fuse in (True, False):
        eh = _eh(ssa, t, fuse_hop_stage=fuse)
        for rep in range(2):  # (the second build of a shape runs with the hub hint of the first)
            table, cards = eh.build_hash_tables(nb.n, ei)
            _check_build(table, cards, n_tbl, False, f'n_tbl={n_tbl} threshold={threshold} fuse={fuse} build {rep}')


@pytest.mark.parametrize('threshold', [1024, 64])
@pytest.mark.parametrize('n_tbl', BUILD_TABLES)
def test_hll_prop_hands_out_the_planted_cardinalities(ssa, dev, monkeypatch, n_tbl, threshold):
    """the ELPH call sequence: hll_prop carries the cardinalities its kernel computed, hll_count hands them out once and recomputes them
    the second time (ss_hll_count): both must be the planted values"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    nb = _hood()
    t, prm, _ = _setup(8, n_tbl)
    eh = _eh(ssa, t)
    ei = torch.from_numpy(nb.edge_index).to(dev)
    hei = torch.cat([ei, torch.arange(nb.n, device=dev).repeat(2, 1)], dim=1)
    _, otab, _ = _oracle_build(n_tbl, False)
    x = eh.initialise_hll(nb.n)
    for k in (1, 2):
        x = eh.hll_prop(x, hei)
        regs = x.cpu().numpy().view(np.uint8)
        assert np.array_equal(regs, otab[k]['hll']), k
        carried = x._ss_count is not None
        first, second = eh.hll_count(x).cpu().numpy(), eh.hll_count(x).cpu().numpy()
        assert carried and x._ss_count is None
        _check_counts(first, regs, t, prm, f'hll_prop hop {k} carried')
        _assert_bits(second, first, f'hll_prop hop {k}: ss_hll_count against the carried values')


@pytest.mark.parametrize('threshold', [1024, 64])
@pytest.mark.parametrize('n_tbl', BUILD_TABLES)
def test_update_moves_a_target_across_the_linear_counting_limit(ssa, dev, monkeypatch, n_tbl, threshold):
    """update_hash_tables adding the one edge that takes the last target from 147 to 148 registers (linear counting -> bias-corrected,
    at hop 1 for the target and at hop 2 for its out-neighbours), and removing it again"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    nb = _hood()
    t, _, _ = _setup(8, n_tbl)
    eh = _eh(ssa, t)
    base = torch.from_numpy(nb.edge_index).to(dev)
    extra = torch.from_numpy(nb.extra_edge).to(dev)
    more = torch.cat([base, extra], dim=1)
    table, cards = eh.build_hash_tables(nb.n, base)
    _check_build(table, cards, n_tbl, False, 'before')
    table, cards = eh.update_hash_tables(table, cards, nb.n, more, added=extra, copy=True)
    _check_build(table, cards, n_tbl, True, f'n_tbl={n_tbl} threshold={threshold}: edge added')
    table, cards = eh.update_hash_tables(table, cards, nb.n, base, removed=extra, copy=True)
    _check_build(table, cards, n_tbl, False, f'n_tbl={n_tbl} threshold={threshold}: edge removed')


# ---- single-sketch table hops on hub rows, under both hub schedules ------------------------------------------------------------------------
_SINGLE_SKETCH_HOPS = r"""
import sys
from argparse import Namespace
from ctypes import byref
import numpy as np, torch
sys.path[:0] = [%r, %r]
import subgraph_sketching_amd as ssa
import hll_planted as hp
from subgraph_sketching_amd._runtime import _ptr, _stream
dev = torch.device('cuda:0')
d = np.load(sys.argv[1])
n = int(d['n'])
csr = ssa.hashing.build_csr(torch.from_numpy(d['edge_index']).to(dev), n, dev, check=True, hub_threshold=8)
csr.use_inferred_self_loops = True
eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
eh.hll_tables = hp.tables(8, None)
prm = eh._params(dev)
mh1, hll1 = torch.from_numpy(d['mh1'].view(np.int32)).to(dev), torch.from_numpy(d['hll1']).to(dev)
mh2, hll2 = torch.full_like(mh1, 0x5A5A5A5A), torch.full_like(hll1, 255)
cards = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
lib, graph, s = ssa._native.lib(), csr.struct(), _stream(dev)
lib.ss_debug_hub_calls(1)
rc_mh = lib.ss_propagate(byref(graph), _ptr(mh1), _ptr(mh2), 128, None, None, 0, None, 0, None, s)
calls_mh = lib.ss_debug_hub_calls(1)
rc_hll = lib.ss_propagate(byref(graph), None, None, 0, _ptr(hll1), _ptr(hll2), 256, _ptr(cards), 1, byref(prm.struct), s)
calls_hll = lib.ss_debug_hub_calls(1)
torch.cuda.synchronize()
np.savez(sys.argv[2], rc=[rc_mh, rc_hll], calls=[calls_mh, calls_hll], hubs=int(csr.hub_count[0]), mega=int(csr.mega_count[0]),
         mh2=mh2.cpu().numpy().view(np.uint32), hll2=hll2.cpu().numpy(), cards=cards.cpu().numpy())
"""


@pytest.mark.parametrize('launches', ['0', '1'])
def test_single_sketch_table_hops_on_hub_rows_under_both_hub_schedules(tmp_path, launches):
    """ss_propagate with the MinHash table alone and with the HLL table alone on the planted neighbourhoods at a hub threshold of 8 (the
    targets are hub rows, `big` a mega row), from the oracle's hop-1 tables: the hop-2 tables equal the oracle's, the cardinalities pass
    _check_counts.  Once with the hub units hosted by the row launches and once as launches of their own -- SS_HUB_LAUNCHES is read once
    per process, hence a child process per schedule.  The MinHash-alone call is counted twice by ss_debug_hub_calls, the HLL-alone call
    once, as they always were."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    nb = _hood()
    t, prm, _ = _setup(8, None)
    _, otab, _ = _oracle_build(None, False)
    src, out = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(src, n=nb.n, edge_index=nb.edge_index, mh1=otab[1]['minhash'].astype(np.uint32), hll1=otab[1]['hll'].astype(np.uint8))
    env = dict(os.environ, SS_HUB_LAUNCHES=launches)
    done = subprocess.run([sys.executable, '-c', _SINGLE_SKETCH_HOPS % (REPO, os.path.dirname(os.path.abspath(__file__))), src, out], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(out)
    assert got['rc'].tolist() == [0, 0] and int(got['hubs']) >= len(nb.targets) and int(got['mega']) >= 1
    assert got['calls'].tolist() == [2, 1]
    assert np.array_equal(got['mh2'], otab[2]['minhash']), 'MinHash alone'
    assert np.array_equal(got['hll2'], otab[2]['hll']), 'HLL alone'
    _check_counts(got['cards'], got['hll2'], t, prm, f'HLL alone, SS_HUB_LAUNCHES={launches}')
