"""The planted estimator inputs of tests/hll_planted.py checked on the CPU: the generator keeps its promises (zero counts, register
counts, splits, exact harmonic sums in the kernel's order and two others), every boundary case exists for every precision and table
length and tells the branches apart, the numpy restatement agrees with the C oracle (value and branch id), and the planted
neighbourhoods give the intended zero counts.  test_hll_planted_gpu.py feeds the same inputs to the kernels."""
import functools

import numpy as np
import pytest

import hll_planted as hp
from hll_planted import F32

QUERY_SHAPES = ((128, 8), (8, 4), (192, 6), (2048, 8))


@functools.lru_cache(maxsize=None)
def _setup(p, n_tbl):
    t = hp.tables(p, n_tbl)
    return t, hp.params(t), hp.cases(p, t)


ALL = [(p, n) for p in hp.PRECISIONS for n in hp.TABLE_LENGTHS]


def _kernel_order_sum(regs):
    """the harmonic sum as hll_row16_stats adds it, in fp32: lane l of 16 takes the chunks l, l + 16, ..., dword by dword, the even
    bytes of a dword then its odd bytes; the lanes' partial sums then meet in the butterfly of row16_sum_f (xor 1, xor 2, half mirror,
    mirror)"""
    M = regs.size
    CH = M // 16
    terms = np.ldexp(F32(1.0), -regs.astype(np.int32)).astype(F32).reshape(CH, 16)
    lanes = np.zeros(16, dtype=F32)
    byte_order = [4 * d + b for d in range(4) for b in (0, 2, 1, 3)]
    for c0 in range(0, CH, 16):
        n = min(16, CH - c0)
        for b in byte_order:
            lanes[:n] = lanes[:n] + terms[c0:c0 + n, b]
    i = np.arange(16)
    for partner in (i ^ 1, i ^ 2, (i & 8) | (7 - (i & 7)), 15 - i):
        lanes = (lanes + lanes[partner]).astype(F32)
    assert np.all(lanes == lanes[0])
    return lanes[0]


def _sequential_sum(terms):
    s = F32(0.0)
    for x in terms:
        s = F32(s + x)
    return s


@pytest.mark.parametrize('p', hp.PRECISIONS)
def test_rows_hold_the_plan_and_sum_exactly_in_any_order(p):
    _, prm, cs = _setup(p, None)
    M = 1 << p
    for i, (name, c) in enumerate(cs.items()):
        S, k = hp.exact_sum(c.V, c.counts)
        assert S * 2.0 ** k == int(S * 2.0 ** k) < (1 << 24), name
        for layout in hp.ZERO_LAYOUTS:
            r = hp.row(p, c.V, c.counts, layout, seed=i)
            assert r.dtype == np.uint8 and r.shape == (M,)
            assert int((r == 0).sum()) == c.V, (name, layout)
            assert {int(v): int(n) for v, n in zip(*np.unique(r[r > 0], return_counts=True))} == {v: n for v, n in c.counts.items() if n}, (name, layout)
            assert int(r.max()) <= hp.max_register(p)
            V, S64, exact = hp.stats(r)
            assert int(V) == c.V and float(S64) == S and bool(exact), (name, layout)
            if p <= 11 or layout == 'strided':
                assert float(_kernel_order_sum(r)) == S, (name, layout, 'kernel order')
        r = hp.row(p, c.V, c.counts, 'shuffled', seed=i)
        if p <= 10:
            terms = np.ldexp(F32(1.0), -r.astype(np.int32)).astype(F32)
            assert float(_sequential_sum(terms)) == S and float(_sequential_sum(np.sort(terms))) == S, name
        if c.V:  # where the zeros sit
            CH = M // 16
            first, last, strided = (hp.row(p, c.V, c.counts, lay, seed=i) for lay in ('first', 'last', 'strided'))
            assert not first[:c.V].any() and not last[M - c.V:].any()
            per_chunk = (strided.reshape(CH, 16) == 0).sum(axis=1)
            assert per_chunk.max() - per_chunk.min() <= 1, 'round robin: the chunks differ by at most one zero'
    assert hp.max_register(p) == 64 - p + 1
    with pytest.raises(AssertionError):
        hp.row(p, 0, {hp.max_register(p) + 1: M})


@pytest.mark.parametrize('p', [4, 8, 16])
def test_splits_have_the_row_as_their_union(p):
    _, _, cs = _setup(p, None)
    for i, (name, c) in enumerate(cs.items()):
        r = hp.row(p, c.V, c.counts, 'shuffled', seed=i)
        for mode in hp.SPLIT_MODES:
            a, b = hp.split(r, mode, seed=i)
            assert a.dtype == b.dtype == np.uint8 and np.array_equal(np.maximum(a, b), r), (name, mode)
        a, b = hp.split(r, 'dominated', seed=i)
        assert np.all(b <= a) and (not r.any() or not np.array_equal(a, b))
        a, b = hp.split(r, 'even_odd')
        assert not a[1::2].any() and not b[0::2].any()
        a, b = hp.split(r, 'chunks')
        assert not a.reshape(-1, 16)[1::2].any() and not b.reshape(-1, 16)[0::2].any()


@pytest.mark.parametrize('P', [8, 128, 2048])
def test_minhash_rows_have_exactly_k_equal_words(P):
    base = np.random.RandomState(P).randint(1, 1 << 32, size=P, dtype=np.uint64).astype(np.uint32)
    for k in (0, 1, P - 1, P):
        for place in hp.MATCH_PLACES:
            other = hp.minhash_row(base, k, place)
            eq = other == base
            assert int(eq.sum()) == k, (k, place)
            if place == 'first':
                assert eq[:k].all()
            elif place == 'last':
                assert eq[P - k:].all()
            elif 0 < k < P:  # one per lane first: the equal words spread over the 4-word chunks round robin
                per_chunk = eq.reshape(P // 4, 4).sum(axis=1)
                assert per_chunk.max() - per_chunk.min() <= 1


@pytest.mark.parametrize('p,n_tbl', ALL)
def test_tables_are_sorted_and_what_the_engine_derives(p, n_tbl):
    import subgraph_sketching_amd as ssa
    t, prm, _ = _setup(p, n_tbl)
    assert prm.n_tbl == (n_tbl or len(ssa.hll_tables.load(p, prefer='regenerated').raw_estimate))
    assert 6 <= prm.n_tbl <= ssa._native.SS_MAX_TABLE == 512
    assert np.all(np.diff(prm.raw) > 0)
    assert t.raw_estimate.astype(F32).astype(np.float64).tolist() == t.raw_estimate.tolist() or n_tbl is None
    assert prm.five_m == F32(5 * (1 << p))
    # the two things the arithmetic rules out (module docstring of hll_planted)
    assert prm.lc_min_zeros - 1 > float(prm.alpha_mm) / float(prm.five_m), 'a row with lc_min_zeros - 1 zeros cannot reach 5m'
    assert F32(prm.alpha_mm / F32(prm.lc_min_zeros - 1)) < prm.five_m
    if n_tbl is None:
        assert (prm.raw[-4] > prm.five_m) == (p > 4), 'p > 4: the shipped table ends above 5m, no row reaches its clamped top window'
    else:
        assert prm.raw[-1] < prm.five_m
    if p == 8:
        assert prm.lc_min_zeros == 109 and prm.m - prm.lc_min_zeros == 147


@pytest.mark.parametrize('p,n_tbl', ALL)
def test_every_case_kind_survives_and_tells_the_branches_apart(p, n_tbl):
    t, prm, cs = _setup(p, n_tbl)
    assert tuple(cs) == hp.expected_kinds(prm), 'a kind is missing'
    M, L = prm.m, prm.lc_min_zeros
    want_V = {'empty': M, 'one_register': M - 1, 'lc_last': L, 'off_lc_low': L - 1, 'off_lc_high': L - 1}
    want_branch = {'empty': 0, 'one_register': 0, 'lc_last': 0, 'off_lc_low': 1, 'off_lc_high': 1, 'five_m_below': 1, 'five_m_above': 2,
                   'top_window': 1, 'near_raw_below': 1, 'near_raw_above': 1, 'saturated': 2}
    for name, c in cs.items():
        assert c.V == want_V.get(name, 0) and c.branch == want_branch[name], name
        assert sum(c.counts.values()) == M - c.V
        if name in ('empty', 'one_register', 'saturated'):
            continue
        agree, v, gap = hp.judge(prm, c.V, c.S)
        assert agree, (name, 'the three restatements must take the same branch')
        assert hp.tells_apart(v, gap, name in hp.STRICT_KINDS), (name, float(v), gap)
    assert float(cs['empty'].value) == 0.0
    assert cs['off_lc_low'].e < cs['off_lc_high'].e and hp.window32(prm, cs['off_lc_low'].e) != hp.window32(prm, cs['off_lc_high'].e) or prm.n_tbl == 6
    assert cs['five_m_below'].e <= prm.five_m < cs['five_m_above'].e
    assert hp.ulps(cs['five_m_below'].e, cs['five_m_above'].e) <= 64, 'the two rows at 5m are a few ulp apart'
    if 'top_window' in cs:
        e = cs['top_window'].e
        assert prm.raw[-4] < e <= prm.five_m and hp.window32(prm, e) == prm.n_tbl - 6
        # (what the window one further up would have read: past the table's end -- nothing to compare, the clamp is the only answer)
    for name in ('near_raw_below', 'near_raw_above'):
        j = int(cs[name].note[4:-1])
        assert hp.ulps(cs[name].e, prm.raw[j]) <= 64 and (cs[name].e > prm.raw[j]) == (name == 'near_raw_above'), name
    sat = cs['saturated']
    assert sat.counts == {hp.max_register(p): M} and np.isfinite(sat.value) and sat.value > prm.five_m


@pytest.mark.parametrize('p,n_tbl', ALL)
def test_restatement_equals_the_oracle_on_every_case(p, n_tbl):
    from oracle import oracle
    t, prm, cs = _setup(p, n_tbl)
    rows = hp.case_rows(p, cs)
    got, branch = oracle.hll_count(rows, hp.oracle_params(t), return_branch=True)
    for i, (name, c) in enumerate(cs.items()):
        v32, b32 = hp.estimate32(prm, c.V, c.S)
        vref, bref = hp.estimate_ref(prm, c.V, c.S)
        v64, b64 = hp.estimate64(prm, c.V, c.S)
        assert b32 == bref == b64 == int(branch[i]) == c.branch, name
        assert v32 == c.value
        if b32 == hp.BRANCH_BIAS:  # (the oracle adds the six in distance order, like estimate_ref)
            assert got[i] == vref, name
        else:
            assert got[i] == v32 == vref, name
        if v32 >= 1:
            assert abs(float(v32) - float(vref)) <= hp.RTOL * abs(float(vref)), name
            assert abs(float(v32) - v64) <= hp.RTOL * abs(v64), name


@pytest.mark.parametrize('P,p', QUERY_SHAPES)
def test_pair_expectations_equal_the_oracle(P, p):
    from oracle import oracle
    t, prm, cs = _setup(p, 257 if (P, p) == (128, 8) else None)
    qt = hp.query_table(p, P, cs)
    q2 = hp.second_hop(qt)
    assert not qt.hll[0].any() and not q2.hll[0].any(), 'row 0 is the identity of the union at both hops'
    assert np.array_equal(qt.hll[1:1 + qt.C], hp.case_rows(p, cs))
    for a, b in qt.pairs:
        ci = (a - 1 - qt.C) // (2 * len(hp.SPLIT_MODES))
        assert np.array_equal(np.maximum(qt.hll[a], qt.hll[b]), qt.hll[1 + ci])
        assert np.array_equal(np.maximum(q2.hll[a], q2.hll[b]), qt.hll[1 + (ci + 1) % qt.C])
    want = hp.expected_pairs(prm, P, [qt.mh, q2.mh], [qt.hll, q2.hll], qt.links)
    otab = {1: {'minhash': qt.mh, 'hll': qt.hll}, 2: {'minhash': q2.mh, 'hll': q2.hll}}
    cards = np.zeros((qt.N, 2), dtype=F32)
    _, dbg = oracle.pair_features(qt.links, otab, cards, 2, hp.oracle_params(t), debug=True)
    assert np.array_equal(dbg['match'], want.match) and np.array_equal(dbg['zeros'], want.zeros) and np.array_equal(dbg['branch'], want.branch)
    plain = want.exact & (want.branch != hp.BRANCH_BIAS)
    assert np.array_equal(dbg['inter'][plain], want.inter[plain])
    np.testing.assert_allclose(dbg['inter'], want.inter, rtol=hp.RTOL, atol=0)
    # the planted links are the cases: (0, v) at (1, 1) is case v, at (2, 2) case v + 1; every split pair likewise; all exact
    C = qt.C
    kinds = list(cs.values())
    for v in range(1, C + 1):
        assert want.zeros[v - 1, 0, 0] == kinds[v - 1].V and want.zeros[v - 1, 1, 1] == kinds[v % C].V
        assert want.branch[v - 1, 0, 0] == kinds[v - 1].branch
    assert want.exact[:C].all() and want.exact[qt.N - 1:, 0, 0].all() and want.exact[qt.N - 1:, 1, 1].all()
    first_pair = qt.N - 1
    for i in range(len(qt.pairs)):
        ci = i // len(hp.SPLIT_MODES)
        assert want.zeros[first_pair + i, 0, 0] == kinds[ci].V and want.branch[first_pair + i, 0, 0] == kinds[ci].branch
    assert set(np.unique(want.branch)) == {0, 1, 2}
    full = want.match == P
    assert (full & (want.zeros == prm.m)).any() and (full & (want.zeros == 0)).any(), 'match == P with V == M and with V == 0'
    assert {0, 1, P - 1, P} <= set(np.unique(want.match[:, 0, 0]).tolist())


def test_planted_neighbourhoods_give_the_intended_zero_counts():
    from oracle import oracle
    t = hp.tables(8)
    prm = hp.params(t)
    nb = hp.neighbourhoods()
    assert nb.full == 147 and nb.M == 256 and int(nb.edge_index.max()) == nb.n - 1
    hop0 = oracle.hll_init(nb.n, 8)
    assert np.all((hop0 != 0).sum(axis=1) == 1), 'a hop-0 row has one non-zero register'
    oprm = hp.oracle_params(t)

    def zeros_of(ei):
        tab, cards = oracle.build_hash_tables(nb.n, ei, 2, 4, oprm)
        return (tab[1]['hll'] == 0).sum(axis=1), (tab[2]['hll'] == 0).sum(axis=1), tab, cards

    z1, z2, tab, cards = zeros_of(nb.edge_index)
    assert sorted(set(nb.want_registers.values())) == [147, 148]
    groups = {t_ // 4 for t_ in nb.targets}
    assert len(groups) >= 5 and len({t_ // 64 for t_ in nb.targets}) >= 4, 'targets in several 4-row groups and wavefronts'
    for t_, count in nb.want_registers.items():
        assert z1[t_] == 256 - count, t_
        indeg = int((nb.edge_index[1] == t_).sum())
        assert indeg > count - 1, 'some neighbours share a register: a max is taken'
        _, br = oracle.hll_count(tab[1]['hll'][t_], oprm, return_branch=True)
        assert br[0] == (0 if count == 147 else 1)
        for w in nb.out_nodes[t_]:
            assert z2[w] == z1[t_] and np.array_equal(tab[2]['hll'][w] == 0, tab[1]['hll'][t_] == 0), (t_, w)
            assert z1[w] >= 254
    last = nb.targets[-1]
    z1x, z2x, _, _ = zeros_of(np.concatenate([nb.edge_index, nb.extra_edge], axis=1))
    assert z1[last] == 109 and z1x[last] == 108, 'the 148th register arrives through the one extra edge'
    changed = np.flatnonzero(z1 != z1x)
    assert changed.tolist() == [last]
    assert all(z2x[w] == 108 for w in nb.out_nodes[last])
    # the big row: exact, bias-corrected from the clamped top window of the two resampled tables that do not fit the fused stage's LDS
    row1 = tab[1]['hll'][nb.big]
    V, S, exact = hp.stats(row1)
    assert bool(exact) and int(V) < 109
    for w in nb.big_out:
        assert np.array_equal(tab[2]['hll'][w], row1) and int((nb.edge_index[1] == w).sum()) == 1
    for n_tbl in (257, 512):
        pt = hp.params(hp.tables(8, n_tbl))
        e = F32(pt.alpha_mm / F32(S))
        assert pt.raw[-4] < e <= pt.five_m and hp.window32(pt, e) == n_tbl - 6
        assert hp.estimate32(pt, int(V), float(S))[1] == hp.BRANCH_BIAS
    # lc_min_zeros is the last linear-counting row
    assert prm.lc[109] <= prm.threshold < prm.lc[108]
