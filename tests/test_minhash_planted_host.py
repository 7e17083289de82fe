"""The planted permutation parameters of tests/minhash_planted.py checked on the CPU: the solver stays inside the reference's range,
every scenario lands where it is meant to (buckets, offsets, tops, the all-ones middle, the wanted values), the documented rules R0 / R1 /
R2 fire on the planted row for the planted permutation and nowhere else, the discriminating scenarios really make the un-flagged
shortcut wrong (so a kernel with a rule missing fails test_minhash_planted_gpu.py), and the C oracle agrees with the Python-integer
values under planted parameters, at hop 0, hop 1 and hop 2."""
import random
from ctypes import c_int32, c_int64

import numpy as np
import pytest

import minhash_planted as mp
from minhash_planted import M32, M61, MID_ONES, R1

SINGLE_WAVE = ('rows8', 'rows4', 'plain1')


def _oracle_minhash_init(a, b, n, first_node=0):
    from oracle import oracle
    out = np.empty((n, len(a)), dtype=np.uint32)
    oracle.lib().so_minhash_init(c_int64(first_node), c_int64(n), c_int32(len(a)), oracle._p(mp.as_u64(a)), oracle._p(mp.as_u64(b)),
                                 oracle._p(out))
    return out


def test_hash_restatement_and_inverse():
    from oracle import oracle
    got = oracle.hash_nodes(mp.N)
    assert [int(v) for v in got] == mp.hashes()
    rng = random.Random(1)
    for h in [0, 1, M32, (1 << 64) - 1] + [rng.getrandbits(64) for _ in range(200)]:
        assert mp.splitmix64(mp.inverse_splitmix64(h)) == h and mp.inverse_splitmix64(mp.splitmix64(h)) == h
    # x mod (2^61 - 1) on either side of the subtraction, in integers
    M = M61
    assert [mp.value_of_x(x) for x in (M - 1, M, M + 1, (7 << 61) | M, 0, (1 << 64) - 1)] == [0xFFFFFFFE, 0, 1, 7, 0, 7]


def test_solver_stays_in_range():
    """ids 10 .. 521, neighbouring pairs with an odd hash difference, S3 targets with free bucket and middle bits: every solution
    is inside [1, 2^61 - 1) x [0, 2^61 - 1), reproduces both targets, and needs about 64 draws (1 / 8 per parameter)"""
    rng = random.Random(7)
    draws = []
    for i in range(10, 522):
        h0, h1 = mp.node_hash(i), mp.node_hash(i + 1)
        if not (h0 - h1) & 1:
            continue
        pair = {}

        def first(r):
            pair['x'] = mp.short_targets('S3', r, False)
            return pair['x'][0]

        a, b, x0, x1, n = mp.plant(h0, first, h1, lambda r: pair['x'][1], rng=rng)
        assert 1 <= a < M61 and 0 <= b < M61
        assert mp.x_of(a, b, h0) == x0 and mp.x_of(a, b, h1) == x1
        draws.append(n)
    assert len(draws) > 200 and max(draws) < mp.DRAW_CAP // 10 and 30 < sum(draws) / len(draws) < 130
    a, b, x0, _, _ = mp.plant(mp.node_hash(10), 0, rng=rng)  # one target: a drawn, b solved
    assert 1 <= a < M61 and 0 <= b < M61 and mp.x_of(a, b, mp.node_hash(10)) == 0
    with pytest.raises(AssertionError):
        mp.solve(4, 0, 2, 1)  # an even hash difference has no inverse


def test_graph_is_what_the_layouts_assume():
    g = mp.graph()
    assert g.n == mp.N and int(g.edge_index.max()) == g.n - 1
    deg = np.bincount(g.edge_index[1], minlength=g.n)
    assert [int(deg[r]) for r in g.long.values()] == [61, 130, 130, 210, 1100]
    assert all(r % 8 == 0 for r in g.long.values())
    for name, s, t in g.short:
        assert deg[s] == (0 if t is None else 1) and (t is None or t < s)
    tops = [s for name, s, _ in g.short if name == 'S10top']
    assert any(s % 8 == 7 for s in tops) and any(s % 8 != 7 for s in tops)
    for row in g.long.values():  # no duplicate among a row's sources, and only L130S lists itself
        assert len(set(g.col[row])) == len(g.col[row]) and (row in g.col[row]) == (row == g.long['L130S'])
    for case in mp.LONG_CASES:  # A and B of a case are entries of their own long row only
        row, col, pa, pb, ids = mp.case_entries(case)
        for i in ids:
            assert [r for r in g.long.values() if i in g.col[r] or i == r] == [row], case
    # the cases that ask for equal slots in two batches of one wavefront
    assert (7 % 60, 7 // 60) == (127 % 60, 0) and 127 // 60 == 2 and 6 % 56 == 118 % 56 and 8 % 64 == 72 % 64
    assert 9 % 64 == 1033 % 64 and (9 // 64) % 16 == (1033 // 64) % 16 == 0


def test_short_scenarios_land_where_intended():
    g, sp = mp.graph(), mp.short_params()
    assert all(1 <= a < M61 and 0 <= b < M61 for a, b in zip(sp.a, sp.b))
    where = {}
    for inf in sp.info:
        q, name, s, t = inf.q, inf.name, inf.row, inf.neighbour
        where.setdefault(name, set()).add(q // 64)
        own = mp.parts(sp.a[q], sp.b[q], s)
        if t is None:
            assert own.x == inf.targets[0] and own.bucket == mp.TOP_BUCKET - mp.ONE_ENTRY.index(name) and own.mid != MID_ONES
            continue
        e0, e1 = mp.parts(sp.a[q], sp.b[q], t), own
        assert (e0.x, e1.x) == inf.targets
        if name in ('S1', 'S2'):
            assert e0.bucket == e1.bucket and (e0.value < e1.value) == (name == 'S1')
        elif name in ('S3', 'S3m', 'S4', 'S4m'):
            lo, hi = (e0, e1) if name in ('S3', 'S4') else (e1, e0)
            assert hi.bucket - lo.bucket == (1 if name.startswith('S3') else 2)
            assert (lo.xp & 63, lo.top, hi.xp & 63, hi.top) == (63, 7, 0, 0)
            assert (lo.value > hi.value) == name.startswith('S3')
        else:
            e, other = (e1, e0) if inf.planted else (e0, e1)
            assert 1 << 20 <= other.bucket < 1 << 25 and other.mid != MID_ONES
            if name == 'S5':
                assert e.lo32 >= (1 << 32) - 8 and e.top == 0 and e.bucket == 0 and e.value > other.value
            elif name == 'S6':
                assert e.lo32 == M32 and e.top == 7 and e.mid != MID_ONES and e.value == 6
            elif name == 'S7':
                assert e.lo32 < 56 and e.bucket == 0 and e.xp >= 8
            elif name == 'S9':
                assert e.mid == MID_ONES and 1 << 12 <= e.bucket < 1 << 19
            else:
                assert e.value == mp.S8_VALUES[name]
                if name in mp.S8_SUMS:
                    assert e.mid == MID_ONES and e.lo32 + e.top == mp.S8_SUMS[name]
                else:
                    assert e.x == (0 if name == 'S8zero' else (1 << 64) - 1)
    assert set(where) == set(mp.SHORT_VARIANTS) and all(js == {0, 1, 2, 3} for js in where.values()), 'every scenario in every register'
    planted_entry = {}
    for inf in sp.info:
        if inf.planted is not None:
            planted_entry.setdefault(inf.name, set()).add(inf.planted)
    assert all(v == {0, 1} for v in planted_entry.values()), 'the planted entry is the neighbour and the own id in turn'


def test_short_rows_are_flagged_by_their_own_scenario_only():
    g, sp = mp.graph(), mp.short_params()
    H = mp.hashes()
    for inf in sp.info:
        hs = [H[e] for e in mp.walked(inf.row)]
        for q in range(256):
            flags = mp._flags_x([mp.x_of(sp.a[q], sp.b[q], h) for h in hs], inf.row)
            for layout, f in flags.items():
                if q != inf.q:
                    assert not f, (inf.name, inf.row, q, layout, f)
                elif inf.name in mp.EXACT_FLAGS:
                    assert f == mp.REQUIRED[inf.name], (inf.name, layout, f)
                else:
                    assert mp.REQUIRED[inf.name] <= f, (inf.name, layout, f)
    # a one-entry row in the top bucket that is the last row of its chunk: the key is exactly the start value of m1 and m2
    for inf in sp.info:
        if inf.name == 'S10top' and inf.row % 8 == 7:
            for R in (4, 8):
                _, slots = mp.rows_share(0, 0, inf.row % R, R)
                assert slots == [63] and (mp.parts(sp.a[inf.q], sp.b[inf.q], inf.row).xp & ~63) | 63 == M32


def test_discriminating_short_scenarios_fool_the_unflagged_shortcut():
    """S2, S3 (and its mirror image), S5: with the flags ignored the shortcut answers the wrong entry's value in the planted
    permutation, in every layout; S8 at r = M: the un-reduced low word is 0xFFFFFFFF where the value is 0 (and r > M would keep M);
    S4, just outside R1, and S1 are answered right"""
    sp = mp.short_params()
    seen = set()
    for inf in sp.info:
        q = inf.q
        want = mp.want_row(mp.graph().entries[inf.row], sp.a, sp.b)
        for layout in mp.row_layouts(inf.row):
            got = mp.shortcut_row(inf.row, [sp.a[q]], [sp.b[q]], layout)[0][0]
            if inf.name in ('S2', 'S3', 'S3m', 'S5'):
                assert got != want[q], (inf.name, layout)
                seen.add(inf.name)
            elif inf.name in ('S1', 'S4', 'S4m', 'S10third'):
                assert got == want[q], (inf.name, layout)
        if inf.name == 'S8m':
            x = inf.targets[inf.planted]
            assert mp.shortcut_of_x(x) == M32 and mp.value_of_x(x) == 0 == want[q] and (x & M61) + (x >> 61) == M61
            seen.add(inf.name)
        if inf.name == 'S5':  # the smallest key and the largest value of the row
            assert want[q] < max(mp.value_of_x(x) for x in inf.targets)
    assert seen == {'S2', 'S3', 'S3m', 'S5', 'S8m'}


@pytest.mark.parametrize('rule', mp.RULES)
def test_long_sets_raise_their_rule_alone(rule):
    g, lp = mp.graph(), mp.long_params(rule)
    H = mp.hashes()
    assert all(1 <= a < M61 and 0 <= b < M61 for a, b in zip(lp.a, lp.b))
    want = {row: mp.want_row(g.entries[row], lp.a, lp.b) for row in g.long.values()}
    fooled = {case: 0 for case in mp.LONG_CASES}
    winners = {case: set() for case in mp.LONG_CASES}
    for row in g.long.values():
        for layout in mp.row_layouts(row):
            got = mp.shortcut_row(row, lp.a, lp.b, layout)
            for inf in lp.info:
                value, flags = got[inf.q]
                if inf.row != row:
                    assert not flags and value == want[row][inf.q], (rule, row, inf.q, layout)
                    continue
                assert flags <= mp.LONG_REQUIRED[rule], (rule, inf.case, layout, flags)
                if layout in SINGLE_WAVE:
                    assert flags == mp.LONG_REQUIRED[rule], (rule, inf.case, layout, flags)
                if not flags:
                    assert value == want[row][inf.q], 'an unflagged row must be right on the fast path'
                elif value != want[row][inf.q] and layout in SINGLE_WAVE:
                    fooled[inf.case] += 1
    for inf in lp.info:
        va, vb = mp.value_of_x(inf.targets[0]), mp.value_of_x(inf.targets[1])
        assert want[inf.row][inf.q] == min(va, vb), 'A and B hold the two smallest buckets: one of them is the minimum'
        winners[inf.case].add(va < vb)
        pa, pb = (mp.parts_of_x(x) for x in inf.targets)
        assert max(pa.bucket, pb.bucket) <= 256
        if rule == 'clean':
            assert abs(pa.bucket - pb.bucket) == 2
    assert all(w == {True, False} for w in winners.values()), 'the winner alternates between A and B'
    if rule != 'clean':
        assert all(n > 0 for n in fooled.values()), f'every case of the {rule} set has permutations the shortcut alone gets wrong: {fooled}'
    if rule == 'same':  # equal slots in two batches of one wavefront: identical keys, the first one walked stays
        for case, layout in ((('L130', 7, 127), 'rows4'), (('L130', 6, 118), 'rows8'), (('L130', 8, 72), 'plain1'), (('L1100', 9, 1033), 'plain16')):
            row, col, pa, pb, ids = mp.case_entries(case)
            pos, slots = next(s for s in mp.row_layouts(row)[layout] if pa in s[0])
            assert pb in pos and slots[pos.index(pa)] == slots[pos.index(pb)]
            wrong = 0
            for inf in lp.info:
                if inf.case == case:
                    assert mp.parts_of_x(inf.targets[0]).bucket == mp.parts_of_x(inf.targets[1]).bucket
                    value, flags = mp.shortcut_row(row, [lp.a[inf.q]], [lp.b[inf.q]], layout)[0]
                    assert value == mp.value_of_x(inf.targets[0]) and flags == {R1}, 'un-flagged, the answer would be A'
                    wrong += value != want[row][inf.q]
            assert wrong > 0, 'the true minimum is B for half the permutations'


def test_oracle_agrees_on_planted_parameters():
    """hop 0 by the oracle's own kernel under the planted parameters, hops 1 and 2 by its edge propagation: equal to the Python-integer
    tables the GPU tests expect"""
    from oracle import oracle
    g = mp.graph()
    ei = oracle.add_self_loops(g.edge_index)
    for a, b in ((mp.short_params().a, mp.short_params().b), (mp.long_params('adjacent').a, mp.long_params('adjacent').b)):
        hop0 = _oracle_minhash_init(a, b, g.n)
        for node in (0, 1, 407, g.n - 1):
            assert hop0[node].tolist() == [mp.value_of_x(mp.x_of(aq, bq, mp.node_hash(node))) for aq, bq in zip(a, b)]
        want = mp.want_tables(g.n, g.edge_index, a, b)
        hop1, _ = oracle.propagate(g.n, ei, mh=hop0)
        assert np.array_equal(hop1, want[0])
        hop2, _ = oracle.propagate(g.n, ei, mh=hop1)
        assert np.array_equal(hop2, want[1])
        for row in list(g.long.values())[:2] + [s for _, s, _ in g.short[:19]]:
            assert want[0][row].tolist() == mp.want_row(g.entries[row], a, b)


@pytest.mark.parametrize('p', [4, 8, 16])
def test_planted_hll_hashes(p):
    from oracle import oracle
    hvs = mp.hll_hashes(p)
    m = 1 << p
    assert hvs['top_rank'] >> p == 0 and mp.hll_rank(hvs['top_rank'], p) == 64 - p + 1
    assert hvs['second_rank'] >> p == 1 and mp.hll_rank(hvs['second_rank'], p) == 64 - p
    assert hvs['rank_one'] >> 63 == 1 and mp.hll_rank(hvs['rank_one'], p) == 1
    assert hvs['register_0'] & (m - 1) == 0 and hvs['register_last'] & (m - 1) == m - 1
    assert [hvs[f'byte_{k}'] & 15 for k in range(16)] == list(range(16))
    for name, hv in hvs.items():
        pre = mp.inverse_splitmix64(hv)
        assert 1 <= pre <= mp.PRE_MAX and mp.splitmix64(pre) == hv
        rows = oracle.hll_init(3, p, first_node=pre - 1)
        for k in range(3):
            assert rows[k].tolist() == mp.hll_row(mp.splitmix64(pre + k), p), (name, k)


@pytest.mark.parametrize('P', [8, 2048])
def test_planted_minhash_init(P):
    hv, a, b, names = mp.minhash_init_params(P)
    assert all(1 <= x < M61 for x in a) and all(0 <= x < M61 for x in b) and set(names) == set(mp.S8_VALUES)
    pre = mp.inverse_splitmix64(hv)
    got = _oracle_minhash_init(a, b, 2, first_node=pre - 1)
    assert got[0].tolist() == [mp.S8_VALUES[name] for name in names]
    assert got[1].tolist() == [mp.value_of_x(mp.x_of(aq, bq, mp.splitmix64(pre + 1))) for aq, bq in zip(a, b)]
    assert {0xFFFFFFFE, 0, 1, 7} <= set(got[0].tolist())
