"""The conditions that keep test_table_hop_planted_gpu.py honest, asserted on the CPU (tests/table_hop_planted.py):
1. witness coverage is 100 %: for every row under test, both sketches and EVERY entry, removing the entry changes want_rows in some round;
2. for every row under test and every foreign colour some colour round tells them apart in the direction that shows;
3. a Python model of a defective walk changes the table in at least one round, for each defect;
4. the planted totals, the long-row patterns per wavefront and per degree-sorted workgroup, and the slice counts are the listed ones;
5. want_rows equals oracle.propagate on a random small graph."""
import numpy as np
import pytest

import table_hop_planted as tp

S = tp.MEGA_SLICE


def _plans(g):
    """(name, Plan) of a graph on the host CSR: with and without the inferred self loops"""
    rowptr, col = tp.csr_of(g.edge_index, g.n)
    return [('self', tp.Plan(rowptr, col, g.n_test, g.n_self)), ('no_self', tp.Plan(rowptr, col, g.n_test, 0))]


def _symmetric_plans():
    g = tp.symmetric_graph()
    rowptr, col = tp.csr_of(g.edge_index, g.n)
    units = [i for i in range(g.n_test) if g.degrees[i] > tp.HUB_THRESHOLD]
    return [('skip', tp.Plan(rowptr, col, g.n_test, g.n_self, skip=True, hub_rows=units)), ('keep', tp.Plan(rowptr, col, g.n_test, g.n_self))]


GRAPHS = {'main': lambda: _plans(tp.main_graph()), 'generic': lambda: _plans(tp.generic_graph()), 'generic_wide': lambda: _plans(tp.generic_graph(True)),
          'symmetric': _symmetric_plans}
SHAPES = {'main': (('minhash', 128), ('hll', 256)), 'symmetric': (('minhash', 128), ('hll', 256)),
          'generic': (('minhash', 4), ('minhash', 12), ('minhash', 260), ('hll', 16), ('hll', 1024)), 'generic_wide': (('minhash', 256), ('hll', 65536))}


def test_the_library_agrees_on_the_constants():
    import subgraph_sketching_amd as ssa
    import hll_planted as hp
    assert ssa._native.MEGA_SLICE == S
    for M in (16, 256, 1024, 65536):
        assert tp.hll_max_register(M) == hp.max_register(int(M).bit_length() - 1)


# ---- 4: what is planted ---------------------------------------------------------------------------------------------------------------------
def test_the_main_graph_plants_the_listed_totals_patterns_and_slices():
    g = tp.main_graph()
    assert 25000 < g.n < 40000 and g.n % 4 != 0 and g.n % 16 != 0
    deg = np.bincount(g.edge_index[1], minlength=g.n)
    assert np.array_equal(deg[:g.n_test], g.degrees) and not deg[g.n_test:].any() and g.n_self <= g.n - 3
    for name, plan in _plans(g):
        tot = plan.total[:g.n_test]
        regular = set(tot[plan.deg[:g.n_test] <= tp.HUB_THRESHOLD].tolist())
        assert {T for T in tp.MH_TOTALS + tp.HLL_TOTALS + tp.FUSED_TOTALS if T - (name == 'self') <= tp.HUB_THRESHOLD} - ({0} if name == 'self' else set()) <= regular
        assert set(tp.MH_TOTALS + tp.HLL_TOTALS + tp.FUSED_TOTALS) - ({0} if name == 'self' else set()) <= set(tot.tolist()), 'all of them with the hub list withheld'
        hubs = (plan.deg[:g.n_test] > tp.HUB_THRESHOLD) & (plan.deg[:g.n_test] <= S)
        # (a hub row has more than 40 in-edges: with its self row it folds at least 42 entries, and the 41 of in-degree 40 are a regular
        # row's; without self loops 1 025 entries are a mega row's)
        assert set(tp.HUB_TOTALS) - ({1025} if name == 'no_self' else {41}) <= set(tot[hubs].tolist()), name
        assert name == 'no_self' or 41 in regular
        assert name == 'no_self' or 1025 in tot[hubs], 'in-degree S plus the self row: still a hub row'
        mega = plan.deg[:g.n_test] > S
        assert sorted(plan.deg[:g.n_test][mega].tolist()) == sorted(tp.mega_degrees())
        # the fused kernel's wavefronts: every pattern of long rows among four consecutive rows; the row16 kernel's: none, the last one,
        # two, three, all of the four rows a wavefront gets once the workgroup's 16 are dealt in degree order
        lo, hi = g.blocks.fused
        assert tp.long_row_patterns(tot[lo:hi], None) == set(range(16)), name
        lo, hi = g.blocks.row16
        assert lo % 16 == 0 and tp.long_row_patterns(tot[lo:hi], g.degrees[lo:hi]) == {0b0000, 0b1000, 0b1100, 0b1110, 0b1111}, name
        assert [int((tot[q:q + 16] > tp.KSOLO).sum()) for q in range(lo, hi, 16)] == list(tp.ROW16_LONG_COUNTS)
    # mega rows: with the self row, 2S has a last slice that holds the self row and nothing else and 2S - 1 fills its last slice exactly;
    # without it the slice the build counted for it is empty
    assert [tp.slices_of(d) for d in tp.mega_degrees()] == [2, 2, 2, 3, 3, 4, 4, 4]
    assert (2 * S + 1) - 2 * S == 1 and (2 * S - 1 + 1) % S == 0 and tp.slices_of(2 * S) * S - S >= 2 * S
    assert {257 % 64, 1025 % 64} == {1}, 'the self row alone in a 64-chunk'


def test_the_generic_and_symmetric_graphs_plant_the_listed_totals():
    for wide, totals in ((False, tp.GENERIC_TOTALS), (True, tp.GENERIC_TOTALS_WIDE)):
        g = tp.generic_graph(wide)
        assert g.degrees.max() <= 300 and g.n * (65536 if wide else 8192) < 64 << 20, 'the widest table stays under 64 MB'
        for name, plan in _plans(g):
            assert set(totals) - ({0} if name == 'self' else set()) <= set(plan.total[:g.n_test].tolist())
    assert {1, 63, 64, 65, 255, 256, 257, 300} <= set(tp.GENERIC_TOTALS)  # P = 4: 64 sub-groups, batches of 256
    for SG in (1, 4, 16, 32, 64):
        G = 64 // SG
        assert {G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1} - {0} <= set(tp.GENERIC_TOTALS if SG < 64 else tp.GENERIC_TOTALS_WIDE) | set(tp.GENERIC_TOTALS), SG
    g = tp.symmetric_graph()
    src, dst = g.edge_index
    assert sorted(zip(src.tolist(), dst.tolist())) == sorted(zip(dst.tolist(), src.tolist())), 'a symmetric edge multiset'
    d = g.degrees
    assert ((d > tp.HUB_THRESHOLD) & (d <= S)).sum() == 1 and (d > S).sum() == 1 and {0, 39, 40} <= set(d.tolist())
    (_, skip), (_, keep) = _symmetric_plans()
    units = d > tp.HUB_THRESHOLD
    assert skip.own[:g.n_test][units].all() and not skip.own[:g.n_test][~units & (d > 0)].any() and skip.own[:g.n_test][d == 0].all()
    assert keep.own[:g.n_self].all() and skip.poison[:g.n_test].sum() == (~units & (d > 0)).sum()


# ---- 1: witness coverage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', sorted(GRAPHS))
def test_every_entry_of_every_row_under_test_is_the_sole_holder_of_a_word(graph):
    """for a min or a max, removing an entry changes the fold iff the entry alone attains the folded value of some word: checked for
    EVERY entry of every row under test in the entry's own witness round (sole_holders), and literally -- the entry taken out of the CSR,
    want_rows on both -- for the first and the last entry of some rows"""
    for name, plan in GRAPHS[graph]():
        for sketch, W in SHAPES[graph]:
            if W == 65536 and name == 'no_self':
                continue  # (the same entries without the last one)
            n_rounds = len([r for r in plan.rounds(W) if r[0] == 'witness'])
            assert n_rounds == max(-(-int(plan.total[:plan.n_test].max()) // W), 1)
            for i in range(plan.n_test):
                held = tp.sole_holders(plan, sketch, W, i)
                assert held.all(), (graph, name, sketch, W, i, np.flatnonzero(~held)[:5])
    if graph == 'main':
        assert n_rounds == 13 and len([r for r in plan.rounds(128) if r[0] == 'witness']) == 25
        name, plan = GRAPHS[graph]()[0]
        rows = [i for i in range(plan.n_test) if plan.total[i] in (1, 33, 65, 1025, 3 * S + 65)]
        assert {int(plan.total[i]) for i in rows} == {1, 33, 65, 1025, 3 * S + 65}
        for sketch, W in SHAPES[graph]:
            reduce = 'min' if sketch == 'minhash' else 'max'
            for i in rows:
                for t in sorted({0, int(plan.deg[i]) - 1} & set(range(int(plan.deg[i])))):
                    at = int(plan.rowptr[i]) + t
                    rowptr = plan.rowptr.copy()
                    rowptr[i + 1:] -= 1
                    table = plan.table(sketch, 'witness', t // W, W)
                    a = plan.want(sketch, table)
                    b = tp.want_rows(rowptr, np.delete(plan.col, at), plan.n_self, False, (), table, reduce)
                    assert (a[i] != b[i]).any() and np.array_equal(np.delete(a, i, 0), np.delete(b, i, 0)), (sketch, i, t)
                table = plan.table(sketch, 'witness', int(plan.deg[i]) // W, W)  # ... and the self row: the launch without self loops
                a, b = plan.want(sketch, table), tp.want_rows(plan.rowptr, plan.col, 0, False, (), table, reduce)
                assert (a[i] != b[i]).any(), (sketch, i, 'self')


# ---- 2: colours -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', sorted(GRAPHS))
def test_a_foreign_colour_shows_in_some_colour_round(graph):
    for name, plan in GRAPHS[graph]():
        assert plan.colour.max() < 1 << plan.colour_bits and len(plan.rounds(128)) - len([r for r in plan.rounds(128) if r[0] == 'witness']) == 2 * plan.colour_bits
        colours = np.unique(plan.colour)
        vals = np.stack([plan._colour_value(k, np.arange(plan.N), None) for k in range(2 * plan.colour_bits)])  # [rounds, N]
        by_colour = np.stack([1 + (((colours >> (k // 2)) & 1) ^ (k % 2)) for k in range(2 * plan.colour_bits)])  # [rounds, colours]
        for i in range(plan.n_test):
            mine = plan.entries(i)
            if not len(mine):
                continue  # (folds nothing: the all-zero row, which any colour value changes)
            c = np.unique(plan.colour[mine])
            assert c.tolist() == [i + 1], 'what a row legitimately folds is of one colour'
            legit = vals[:, mine[0]]
            foreign = colours != i + 1
            # MinHash: the foreigner holds 1 where the row holds 2; HLL: 2 where the row holds 1 -- for EVERY foreign colour
            assert ((by_colour < legit[:, None]).any(axis=0) | ~foreign).all() and ((by_colour > legit[:, None]).any(axis=0) | ~foreign).all(), (name, i)
            # the foreigners the walks can meet: the next row's first source, a source of the neighbouring pool, the own row that must not count
            near = [int(plan.col[plan.rowptr[i + 1]])] if plan.rowptr[i + 1] < plan.rowptr[-1] else []
            near += [int(mine[-1]) + 1] if mine[-1] + 1 < plan.N and mine[-1] >= plan.n_test else []
            near += [] if plan.own[i] else [i]
            for j in near:
                if plan.colour[j] == i + 1:
                    continue
                assert (vals[:, j] < legit).any() and (vals[:, j] > legit).any(), (name, i, j)


# ---- 3: defective walks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('defect', tp.DEFECTS)
def test_a_defective_walk_changes_the_table(defect):
    """the model is never an expected output: it only proves that the planted rows catch each defect, for both sketches, on every row of
    the main graph where the defect can occur"""
    hit = 0
    for name, plan in GRAPHS['main']():
        for i in range(plan.n_test):
            bad = tp.walk_entries(plan, i, defect)
            if bad is None:
                continue
            hit += 1
            for sketch, W in SHAPES['main']:
                assert tp.defect_shows(plan, sketch, W, i, bad) is not None, (defect, name, sketch, i, int(plan.total[i]))
    assert hit >= (3 if defect == 'drops_lonely_self_row' else 8)


def test_the_lonely_self_row_cases_exist():
    (_, plan), _ = GRAPHS['main']()
    lonely = [int(plan.deg[i]) for i in range(plan.n_test) if tp.walk_entries(plan, i, 'drops_lonely_self_row') is not None]
    assert {64, 128, 256, 512, S, 2 * S} <= set(lonely)  # alone in a 64-chunk; 2S: alone in a slice


# ---- 5: the reference -----------------------------------------------------------------------------------------------------------------------
def test_want_rows_equals_the_oracle_on_a_random_graph():
    from oracle import oracle
    rng = np.random.RandomState(3)
    n = 300
    ei = rng.randint(0, n - 9, size=(2, 1500)).astype(np.int64)
    ei = ei[:, ei[1] % 7 != 0]  # rows without an in-edge
    n_self = int(ei.max()) + 1
    mh = rng.randint(0, 1 << 32, size=(n, 12), dtype=np.int64).astype(np.uint32)
    hll = rng.randint(0, 58, size=(n, 64)).astype(np.uint8)
    rowptr, col = tp.csr_of(ei, n)
    assert tp.is_csr_of(rowptr, col, ei, n) and not tp.is_csr_of(rowptr, np.roll(col, 1), ei, n)
    loops = np.arange(n_self, dtype=np.int64)
    for with_self, edges in ((True, np.concatenate([ei, np.stack([loops, loops])], axis=1)), (False, ei)):
        want_mh, want_hll = oracle.propagate(n, edges, mh, hll)
        ns = n_self if with_self else 0
        assert np.array_equal(tp.want_rows(rowptr, col, ns, False, (), mh, 'min'), want_mh)
        assert np.array_equal(tp.want_rows(rowptr, col, ns, False, (), hll, 'max'), want_hll)
    # the skip word: regular rows with an in-edge leave their own row out, rows the hub units serve keep it
    hub = [int(np.argmax(np.diff(rowptr)))]
    got = tp.want_rows(rowptr, col, n_self, True, hub, mh, 'min')
    plain = tp.want_rows(rowptr, col, 0, False, (), mh, 'min')
    with_self = tp.want_rows(rowptr, col, n_self, False, (), mh, 'min')
    deg = np.diff(rowptr)
    assert np.array_equal(got[hub], with_self[hub]) and np.array_equal(np.delete(got, hub, 0)[np.delete(deg, hub) > 0], np.delete(plain, hub, 0)[np.delete(deg, hub) > 0])
    assert np.array_equal(got[deg == 0], with_self[deg == 0])
