"""The plans of masked_planted.py without a GPU: the restated rule of target-link masking (tests/masked_restatement.py) against one
oracle rebuild per link on every planted family -- rows, match, zeros and row_zeros bit for bit --, the facts that need no reference
(a bridge link shares nothing after masking), four WRONG rules that each change an integer on the family named for them -- the argument
on paper that tests/test_masked_planted_gpu.py would fail on a kernel that took one of them --, the arithmetic of the batch patterns
and the shape that masked.py refuses."""
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import masked_planted as mp
import masked_restatement as mr
from conftest import oracle_params
from oracle import oracle

FAMILIES = dict(mp.rule_families())


def _params(p):
    import subgraph_sketching_amd as ssa
    return oracle_params(ssa.hll_tables.load(p))


def counts_of(rows):
    """(match [h, h], zeros [h, h], row_zeros [2, h]) of {kind: [2, h, W]} rows, as the pair arithmetic counts them"""
    mh, hl = rows['minhash'], rows['hll']
    match = (mh[0][:, None, :] == mh[1][None, :, :]).sum(axis=2).astype(np.int32)
    zeros = (np.maximum(hl[0][:, None, :], hl[1][None, :, :]) == 0).sum(axis=2).astype(np.int32)
    return match, zeros, (hl == 0).sum(axis=2).astype(np.int32)


def check_rule(n, ei, links, h, num_perm=128, p=8):
    """masked_rows on every link against the oracle's rebuild without the link -> [(match, zeros, row_zeros)] per link"""
    prm = _params(p)
    tables, _ = oracle.build_hash_tables(n, ei, h, num_perm, prm)
    nbrs, n_self = mr.in_neighbours(n, ei), mr.n_self_of(ei)
    out = []
    for u, v in links.tolist():
        assert mr.is_edge(nbrs, u, v)
        rows = mr.masked_rows(u, v, nbrs, n_self, tables, h)
        _, want_dbg, want_rows, _ = mr.leave_one_out(u, v, n, ei, h, num_perm, prm)
        for kind in ('minhash', 'hll'):
            assert np.array_equal(rows[kind], want_rows[kind]), f'link ({u}, {v}): {kind} rows differ from the rebuild'
        match, zeros, row_zeros = counts_of(rows)
        assert np.array_equal(match, want_dbg['match']) and np.array_equal(zeros, want_dbg['zeros']), (u, v)
        assert np.array_equal(row_zeros, (want_rows['hll'] == 0).sum(axis=2)), (u, v)
        out.append((match, zeros, row_zeros))
    return out


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def test_the_constants_and_the_geometry_are_the_sources():
    unit = open(mp.UNIT).read()
    assert (mp.THREADS, mp.PAIRS_GRID, mp.SCAN_GRID, mp.SCAN_LINKS) == (256, 4096, 8192, 131072)
    assert 'const size_t dyn = ((size_t)2 * h * W4 + kMaskedThreads) * 16 + (size_t)M * 4;' in unit
    assert 'const int W4 = (P >> 2) + (M >> 4);' in unit and 'L.S = kMaskedThreads / L.W4;' in unit
    assert 'const int S1 = P <= kMaskedThreads ? kMaskedThreads / P : 1;' in unit
    assert re.search(r'grid = \(unsigned\)\(B < kMaskedGrid \? B : kMaskedGrid\);', unit)
    want = {(4, 4): (2, 128, 64), (8, 4): (3, 85, 32), (192, 6): (52, 4, 1), (128, 8): (48, 5, 2), (512, 8): (144, 1, 1),
            (960, 8): (256, 1, 1), (128, 11): (160, 1, 2), (512, 11): (256, 1, 1)}
    for shape in mp.SHAPES:
        g = mp.geometry(*shape)
        assert (g.W4, g.S, g.S1) == want[shape] and g.supported
        assert mp.lds_bytes(*shape, 3) <= 64 * 1024  # no launch of the plan asks for more dynamic LDS than a kernel gets unasked
    assert mp.lds_bytes(512, 11, 3) == 36864 and mp.lds_bytes(960, 8, 3) == 29696


def test_the_shapes_cover_every_path_named():
    seen = set()
    for shape in mp.SHAPES:
        seen |= mp.shape_classes(*shape)
    assert seen == set(mp.ALL_CLASSES)
    assert mp.shape_classes(960, 8) >= {'first hop: partial last trip', 'a row of exactly 256 chunks'} and 960 % 256 == 192
    assert 'more HLL registers than threads' in mp.shape_classes(512, 11) and mp.geometry(512, 11).M == 2048
    old = set()
    for shape in ((128, 8), (64, 6), (256, 10), (8, 4)):  # the shapes of tests/test_masked_gpu.py
        old |= mp.shape_classes(*shape)
    assert old == {'W4 = 3: thread 255 inactive', 'more HLL registers than threads'}
    # the comb's row lengths surround every S of the plan (the hop-3 walk takes s = slot, slot + S, ... <= the row length) and 16, 256
    S = {mp.geometry(*shape).S for shape in mp.SHAPES}
    assert S == {1, 4, 5, 85, 128}
    for s in S | {mp.ROW, mp.THREADS}:
        assert {s - 1, s, s + 1} - {0} <= set(mp.COMB_DEGREES), s
    n, ei, links = mp.comb()
    assert sorted(mp.comb.rows.values()) == sorted(mp.COMB_DEGREES + mp.COMB_TRIANGLES + mp.COMB_LOOPS)


def test_every_position_puts_the_partner_at_every_position():
    for L in mp.POSITION_L:
        n, ei, links = mp.every_position(L)
        row = ei[0][ei[1] == 0]
        assert len(row) == L and sorted(links[:L, 1].tolist()) == sorted(row.tolist())  # one link (x, y) per entry of row x
        assert np.array_equal(links[L:], links[:L, ::-1])
        n, ei, links = mp.every_position(L, 'in')
        assert not (ei[1] != 0).any()  # rows y are empty: the hit is in row x alone
        n, ei, links = mp.every_position(L, 'out')
        assert not (ei[1] == 0).any()  # row x is empty: the hit is in the one-entry row y
    assert {L % 16 for L in mp.POSITION_L} >= {0, 1, 15} and max(mp.POSITION_L) > mp.THREADS


def test_pattern_arithmetic():
    n, ei, distinct, non = mp.batch_forest()
    nbrs = mr.in_neighbours(n, ei)
    assert all(mr.is_edge(nbrs, u, v) for u, v in distinct.tolist()) and not any(mr.is_edge(nbrs, u, v) for u, v in non.tolist())
    assert len(np.unique(distinct, axis=0)) == len(distinct)
    for length in mp.WAVE_LENGTHS:
        links, is_edge, which = mp.wave_patterns(length)
        assert length % 16 in (1, 15) and len(links) == length
        assert [mr.is_edge(nbrs, u, v) for u, v in links.tolist()] == is_edge.tolist()
        whole = is_edge[:length // 4 * 4].reshape(-1, 4)
        pattern = (whole * (1 << np.arange(4))).sum(axis=1)
        assert set(pattern.tolist()) == set(range(16))
        pairs = set(zip(pattern[:-1].tolist(), pattern[1:].tolist()))
        assert {(15, 0), (0, 15), (15, 15), (0, 0)} <= pairs  # all-edge and no-edge wavefronts side by side, in one workgroup and across two
    links, which = mp.many_edges()
    assert len(links) == mp.MANY_EDGES > 2 * mp.PAIRS_GRID and set(which.tolist()) == set(range(len(distinct)))
    assert np.array_equal(links, distinct[which])
    links, is_edge, which = mp.long_batch()
    assert len(links) == mp.LONG_BATCH > mp.SCAN_LINKS
    assert is_edge[mp.SCAN_LINKS - 1] and is_edge[mp.SCAN_LINKS] and not is_edge[mp.SCAN_LINKS + 1] and is_edge[-1] and not is_edge[-2]
    assert is_edge[mp.SCAN_LINKS:].sum() >= 3 and (~is_edge[mp.SCAN_LINKS:]).sum() >= 3
    assert np.array_equal(links[is_edge], distinct[which[is_edge]]) and np.array_equal(links[~is_edge], non[which[~is_edge]])
    assert is_edge.sum() > 2 * mp.PAIRS_GRID


# ---- the rule against the rebuild --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', mp.HOPS)
@pytest.mark.parametrize('name', list(FAMILIES))
def test_rule_against_rebuild_on_every_family(name, h):
    n, ei, links = FAMILIES[name]
    check_rule(n, ei, links, h)


SHAPE_FAMILIES = ('bridge(3,3)', 'bridge(40,300)') + tuple(f'bridge(3,3,{v})' for v in mp.BRIDGE_VARIANTS)


@pytest.mark.parametrize('num_perm,p', mp.SHAPES)
def test_rule_against_rebuild_at_every_shape(num_perm, p):
    """... and the facts that need no reference: the two sides of a bridge share nothing once the bridge is gone, so every match count
    is 0 (this is where it is established that no two of these few ids collide in a 32-bit hash at any shape); with the bridge in
    place the 3-hop balls of u and v are both the whole component, so the stored hop-3 rows agree in all P permutations"""
    prm = _params(p)
    for name in SHAPE_FAMILIES:
        n, ei, links = FAMILIES[name]
        got = check_rule(n, ei, links, 3, num_perm, p)
        for match, zeros, row_zeros in got:
            assert not match.any(), name
        if 'to' not in name:
            tables, cards = oracle.build_hash_tables(n, ei, 3, num_perm, prm)
            _, dbg = oracle.pair_features(links, tables, cards, 3, prm, debug=True)
            assert (dbg['match'][:, 2, 2] == num_perm).all() and (dbg['match'] > 0).any(axis=(1, 2)).all(), name
    n, ei, links = FAMILIES['K2']
    M = 1 << p
    for match, zeros, row_zeros in check_rule(n, ei, links, 3, num_perm, p):
        assert not match.any() and (row_zeros == M - 1).all()  # each endpoint is left with its own self loop, at every hop


@pytest.mark.parametrize('h', mp.HOPS)
def test_bridge_links_share_nothing_after_masking(h):
    for name, (n, ei, links) in FAMILIES.items():
        if mp.is_bridge(name):
            for match, zeros, row_zeros in check_rule(n, ei, links, h):
                assert not match.any(), name


# ---- sensitivity: four wrong rules ---------------------------------------------------------------------------------------------------
MUTANTS = ('stored_h1', 'first_copy', 'one_dir', 'no_wpartner')
# (a fifth candidate -- dropping the "w itself" term of hop 3 -- cannot show on any graph: R2(x) already folds H1(w) for every w in N'(x),
# and R3 folds R2.  It is not asserted.)


def mutant_rows(u, v, nbrs, n_self, tables, h, mutant=None):
    """masked_restatement.masked_rows written again with one switch per wrong rule:
      stored_h1    H1(y) is the stored T1(y) for y in {u, v} too
      first_copy   only the first copy of the partner leaves a row
      one_dir      the partner leaves row u only
      no_wpartner  at hop 3 the partner stays in the row of a w that is an endpoint (w = x through its explicit self loop)"""
    out = {}
    for kind in ('minhash', 'hll'):
        T0, T1 = tables[0][kind], tables[1][kind]
        width, dtype = T0.shape[1], T0.dtype

        def nprime(x):
            nb = nbrs[x]
            partner = v if x == u else (u if x == v else None)
            if partner is None or (mutant == 'one_dir' and x == v):
                return nb
            if mutant == 'first_copy':
                hit = np.flatnonzero(nb == partner)
                return np.delete(nb, hit[:1])
            return nb[nb != partner]

        def fold(rows):
            if not rows:
                return np.zeros(width, dtype=dtype)
            return np.stack(rows).min(axis=0) if kind == 'minhash' else np.stack(rows).max(axis=0)

        R1 = {x: fold([T0[j] for j in nprime(x)] + ([T0[x]] if x < n_self else [])) for x in (u, v)}

        def H1(y):
            return R1[y] if y in R1 and mutant != 'stored_h1' else T1[y]

        rows = np.zeros((2, h, width), dtype=dtype)
        for side, x in enumerate((u, v)):
            rows[side, 0] = R1[x]
            if h >= 2:
                R2 = fold([H1(w) for w in nprime(x)] + ([R1[x]] if x < n_self else []))
                rows[side, 1] = R2
            if h >= 3:
                parts = [R2] if x < n_self else []
                for w in nprime(x):
                    if w < n_self:
                        parts.append(H1(w))
                    parts.extend(H1(y) for y in (nbrs[w] if mutant == 'no_wpartner' else nprime(w)))
                rows[side, 2] = fold(parts)
        out[kind] = rows
    return out


def changed_links(name, mutant, h=3, num_perm=128, p=8):
    """how many links of a family get another match, zeros or row_zeros integer from the wrong rule"""
    n, ei, links = FAMILIES[name]
    tables, _ = oracle.build_hash_tables(n, ei, h, num_perm, _params(p))
    nbrs, n_self = mr.in_neighbours(n, ei), mr.n_self_of(ei)
    changed = 0
    for u, v in links.tolist():
        right = mr.masked_rows(u, v, nbrs, n_self, tables, h)
        same = mutant_rows(u, v, nbrs, n_self, tables, h)
        assert all(np.array_equal(right[k], same[k]) for k in right)  # without a switch it is the rule
        wrong = counts_of(mutant_rows(u, v, nbrs, n_self, tables, h, mutant))
        changed += any(not np.array_equal(a, b) for a, b in zip(counts_of(right), wrong))
    return changed


def test_stored_h1_shows_on_every_bridge_with_a_leaf_and_on_the_long_cycles():
    """H1 of an endpoint is looked up through a leaf at hop 3 (u -> leaf -> u) or through an explicit self loop; bridge (0, 0) and K2
    have neither, nothing looks H1(u) up there.  The leak is ONE id (the partner) more in a row: on bridge (300, 300) that is one id
    among 306, which moves no integer at (128, 8) (0 of 2 links) and does at 960 permutations or 2048 registers"""
    for name in FAMILIES:
        if name.startswith('bridge(') and name not in ('bridge(0,0)', 'bridge(300,300)'):
            assert changed_links(name, 'stored_h1') == 2, name
    assert changed_links('bridge(300,300)', 'stored_h1', 3, 960, 8) == 2 and changed_links('bridge(300,300)', 'stored_h1', 3, 512, 11) == 2
    for k in (5, 6, 7):
        assert changed_links(f'cycle({k})', 'stored_h1') == 3, k
    assert changed_links('bridge(0,0)', 'stored_h1') == 0 and changed_links('K2', 'stored_h1') == 0
    assert changed_links('bridge(3,3,loop_uv)', 'stored_h1', h=2) == 2  # through the self loop one hop earlier


def test_first_copy_shows_on_the_bridge_with_copies():
    for h in mp.HOPS:
        assert changed_links('bridge(3,3,copies)', 'first_copy', h=h) == 2
    assert changed_links('bridge(3,3)', 'first_copy') == 0  # one copy each way: nothing to tell apart


def test_no_wpartner_shows_on_the_bridges_with_self_loops():
    assert changed_links('bridge(3,3,loop_u)', 'no_wpartner') >= 1 and changed_links('bridge(3,3,loop_uv)', 'no_wpartner') == 2
    assert changed_links('bridge(3,3)', 'no_wpartner') == 0
    assert changed_links('bridge(3,3,loop_uv)', 'no_wpartner', h=2) == 0  # the switch sits in the hop-3 walk


@pytest.mark.parametrize('name', list(FAMILIES))
def test_one_dir_shows_on_every_family(name):
    assert changed_links(name, 'one_dir', h=1 if name.startswith('every_position(300') else 3) >= 1


@pytest.mark.parametrize('num_perm,p', mp.SHAPES)
def test_every_mutant_shows_at_every_shape(num_perm, p):
    assert changed_links('bridge(3,3)', 'stored_h1', 3, num_perm, p) == 2 and changed_links('bridge(3,3)', 'one_dir', 3, num_perm, p) >= 1
    assert changed_links('bridge(3,3,copies)', 'first_copy', 3, num_perm, p) == 2
    assert changed_links('bridge(3,3,loop_uv)', 'no_wpartner', 3, num_perm, p) == 2


# ---- the shape masked.py refuses ---------------------------------------------------------------------------------------------------------
def test_a_row_of_257_chunks_is_refused_before_the_device_is_touched():
    import subgraph_sketching_amd as ssa
    assert mp.geometry(964, 8).W4 == 257 and not mp.geometry(964, 8).supported and mp.geometry(960, 8).supported
    links, ei = torch.tensor([[0, 1]]), torch.tensor([[0, 1], [1, 0]])
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=964, floor_sf=False, use_zero_one=True))
    with pytest.raises(NotImplementedError, match='one 16-byte chunk per thread'):  # ({} as tables: nothing is looked up before the refusal)
        eh.get_subgraph_features(links, {}, torch.zeros((2, 2)), mask_target=ei)
    from subgraph_sketching_amd import masked
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=960, floor_sf=False, use_zero_one=True))
    masked.check_arguments(eh, links, ei, 10)  # 256 chunks pass
    # the C entry point draws the same line (every pointer below is a fake one: the call returns before it reads any of them)
    from ctypes import byref, c_void_p
    lib, fake, ptrs = ssa._native.lib(), c_void_p(8), (c_void_p * 3)(8, 8, 8)
    g = ssa._native.CsrGraphStruct(rowptr=8, col=8, num_nodes=4, n_self_loops=4)
    prm = ssa._native.HllParams(p=8, n_tbl=len(ssa.hll_tables.load(8).bias), alpha_mm=1.0, threshold=1.0, lc_min_zeros=1, raw_est=8, bias=8, lc_table=8)
    assert lib.ss_masked_pair_features(byref(g), fake, 3, 4, 2, fake, fake, ptrs, 964, ptrs, fake, 2, byref(prm), 0, fake, None, None, None, None,
                                       None, fake, 1 << 20, None) == -4
