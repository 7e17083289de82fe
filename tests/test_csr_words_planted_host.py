"""csr_words_planted.py keeps its promises (no GPU): the constants are in the sources, every planted index lies in the tile, offset
and loop it claims, every edit changes the multiset exactly as stated, every form has the row addresses it claims."""
from collections import Counter

import numpy as np
import pytest
import torch

import csr_words_planted as P
import symmetric_self_restatement as R


def _pairs(ei):
    return Counter(zip(ei[0].tolist(), ei[1].tolist()))


def _delta(old, new):
    """(pairs the edit added, pairs it took away): the two lists differ in a few columns only"""
    changed = np.flatnonzero((old != new).any(axis=0))
    was, now = _pairs(old[:, changed]), _pairs(new[:, changed])
    return now - was, was - now


def _sorted_columns(ei):
    return np.sort(ei[0] * (1 << 32) + ei[1])


def test_constants_are_found_in_the_sources():
    C = P.constants()
    assert all(isinstance(v, int) and v > 0 for v in C)
    assert C.tile % C.sort_threads == 0 and C.tile // C.sort_threads == 8     # a thread's 8 slots
    assert C.sort_threads % C.wave == 0 and C.fp_threads % C.wave == 0
    # OFFSETS are the boundaries of these constants: both halves of a pair, a wavefront in both load forms, a thread's slots
    assert set(P.offsets_of(4 * C.tile, 0)) >= {0, 1, C.wave - 1, C.wave, 2 * C.wave - 1, 2 * C.wave, C.sort_threads - 1, C.sort_threads,
                                                2 * C.sort_threads - 1, 2 * C.sort_threads, C.tile // 2 - 1, C.tile // 2, C.tile - 2, C.tile - 1}


@pytest.mark.parametrize('name', P.BASES + ('small_odd', 'reducer_odd'))
def test_bases(name):
    C = P.constants()
    b = P.base(name)
    E = b.ei.shape[1]
    assert b.ei.dtype == np.int64 and b.ei.flags['C_CONTIGUOUS']
    assert R.is_symmetric_multiset(b.ei)
    assert int(b.ei.min()) >= 0 and int(b.ei.max()) == b.n - 2
    loops = np.flatnonzero(b.ei[0] == b.ei[1])
    planted = {e for _, _, _, e in P.positions(E)}
    assert not planted & set(loops.tolist())
    assert E % 2 == (1 if name.endswith('_odd') else 0)
    if name.startswith('small'):
        assert E // C.tile == 3 and E % C.tile and P.levels(b.n) == 1
    if name.startswith('reducer'):
        assert -(-E // C.tile) > C.run_threads and E // 2 > 3 * C.fp_blocks * C.fp_threads and P.levels(b.n) == 1
        assert {'reducer_last_thread', 'reducer_second_pass'} <= set(P.tile_classes(E))
    if name == 'two_level':
        assert b.n // 1024 > C.max_keys and P.levels(b.n) == 2


@pytest.mark.parametrize('name', P.BASES)
def test_positions_lie_where_they_claim(name):
    C = P.constants()
    E = P.base(name).ei.shape[1]
    classes = P.tile_classes(E)
    assert classes['first'] == 0 and classes['second'] == 1 and E // C.tile - 1 in classes.values() and classes['partial'] == E // C.tile
    assert len(set(classes.values())) == len(classes)
    assert 1 < classes['middle'] < E // C.tile - 1 if name != 'small' else set(classes.values()) == {0, 1, 2, 3}
    if name == 'reducer':   # thread run_threads - 1 of the reducer's first pass, thread 0 of its second
        assert classes['reducer_last_thread'] == C.run_threads - 1 and classes['reducer_second_pass'] == C.run_threads
        assert classes['reducer_second_pass'] == E // C.tile - 1 and 'last_full' not in classes
    seen = set()
    for cls, tile, off, e in P.positions(E):
        assert classes[cls] == tile and 0 <= e < E and e // C.tile == tile and e % C.tile == off
        for aligned in (True, False):
            t, thread, slot, vec = P.sort_slot(E, aligned, e)
            assert t == tile and 0 <= thread < C.sort_threads and 0 <= slot < 8
            assert vec == (aligned and cls != 'partial')
            seen.add((cls != 'partial', vec, slot, 'first' if thread % C.wave == 0 else 'last' if thread % C.wave == C.wave - 1 else '-'))
    for vec in (True, False):   # every slot of a thread, and both ends of a wavefront, in both load forms
        assert {s for full, v, s, _ in seen if full and v == vec} == set(range(8))
        assert {w for full, v, _, w in seen if full and v == vec} >= {'first', 'last'}


@pytest.mark.parametrize('name', ('small', 'small_odd', 'reducer', 'reducer_odd', 'two_level'))
def test_fingerprint_positions_lie_in_the_loops_they_claim(name):
    C = P.constants()
    E = P.base(name).ei.shape[1]
    stride = C.fp_blocks * C.fp_threads
    for aligned in (True, False):
        got = P.fp_positions(E, aligned)
        for (loop, which, half), e in got.items():
            assert P.fp_loop_of(E, aligned, e) == (loop, half), (loop, which, half, e)
        loops = {loop for loop, _, _ in got}
        if not aligned:
            assert loops == {P.SCALAR}
            assert got[(P.SCALAR, 'first', None)] == 0 and got[(P.SCALAR, 'last', None)] == E - 1
            assert ((P.SCALAR, 'stride_again', None) in got) == (E > stride)
        else:
            want = {P.ONE_LOAD} | ({P.TAIL} if E % 2 else set()) | ({P.LOAD0, P.LOAD1} if E // 2 > stride else set())
            assert loops == want
            if name.startswith('reducer'):
                assert got[(P.LOAD0, 'first', 'x')] == 0 and got[(P.LOAD1, 'first', 'x')] == 2 * stride
                assert got[(P.LOAD1, 'last', 'y')] - got[(P.LOAD0, 'last', 'y')] == 2 * stride
                # all threads run the two-load loop, only some the one-load loop
                assert got[(P.ONE_LOAD, 'last', 'x')] // 2 - got[(P.ONE_LOAD, 'first', 'x')] // 2 + 1 < stride
            if E % 2:
                assert got[(P.TAIL, 'only', None)] == E - 1
    # every edge is read by exactly the loop the closed form says (a sample, and the seams)
    probe = sorted(set(np.random.RandomState(1).randint(0, E, size=200).tolist()) | {0, E - 1} | {e for e in (2 * stride - 1, 2 * stride, 4 * stride) if e < E})
    for e in probe:
        assert P.fp_loop_of(E, True, e)[0] in (P.LOAD0, P.LOAD1, P.ONE_LOAD, P.TAIL)


def _a_position(E, cls='second'):
    return next(e for c, _, off, e in P.positions(E) if c == cls and off == 1)


@pytest.mark.parametrize('name', ('small', 'two_level'))
def test_edits_change_the_multiset_as_stated(name):
    b = P.base(name)
    E = b.ei.shape[1]
    before = _pairs(b.ei)
    for _, _, _, k in P.positions(E)[::5]:
        u, v = int(b.ei[0, k]), int(b.ei[1, k])
        got = P.EDITS['to_self'](b.ei, k)
        assert _delta(b.ei, got) == (Counter({(u, u): 1}), Counter({(u, v): 1}))
        assert not R.is_symmetric_multiset(got)

        got = P.EDITS['retarget'](b.ei, k)
        added, removed = _delta(b.ei, got)
        (new, one), = added.items()
        assert one == 1 and new[0] == u and new[1] not in (u, v) and (new[1], u) not in before and new not in before
        assert removed == Counter({(u, v): 1}) and not R.is_symmetric_multiset(got)

        got = P.EDITS['swap_with_reverse'](b.ei, k)
        assert not np.array_equal(got, b.ei) and np.array_equal(_sorted_columns(got), _sorted_columns(b.ei))
        assert R.is_symmetric_multiset(got)
        assert (int(got[0, k]), int(got[1, k])) == (v, u)

        got = P.EDITS['reverse_one'](b.ei, k)
        assert _delta(b.ei, got) == (Counter({(v, u): 1}), Counter({(u, v): 1}))
        assert not R.is_symmetric_multiset(got)

        j = P.swap_partner(b.ei, k, [e for _, _, _, e in P.positions(E)])
        s2, d2 = int(b.ei[0, j]), int(b.ei[1, j])
        got = P.apply(b.ei, P.swap_dsts_columns(b.ei, k, j))
        assert j // P.constants().tile != k // P.constants().tile
        assert _delta(b.ei, got) == (Counter({(u, d2): 1, (s2, v): 1}), Counter({(u, v): 1, (s2, d2): 1}))
        assert np.array_equal(got[0], b.ei[0]) and np.array_equal(np.sort(got[1]), np.sort(b.ei[1]))   # rows' and columns' statistics
        assert np.array_equal(np.bincount(got[1], minlength=b.n), np.bincount(b.ei[1], minlength=b.n))
        assert not R.is_symmetric_multiset(got)

        for row in (0, 1):
            got = P.apply(b.ei, P.max_id_columns(b.ei, k, b.n, row))
            assert P.n_self(b.ei) == b.n - 1 and P.n_self(got) == b.n and int((got == b.n - 1).sum()) == 1 and got[row, k] == b.n - 1
            got = P.apply(b.ei, P.bad_id_columns(b.ei, k, b.n, row))
            assert int((got >= b.n).sum()) == 1 and got[row, k] == b.n and P.n_self(got) == b.n + 1
            kept = P.kept_edges(got, b.n)
            assert kept.shape[1] == E - row and int(kept.max()) < b.n
            if row == 0:
                assert _delta(b.ei, kept) == (Counter({(0, v): 1}), Counter({(u, v): 1}))    # stored as source 0
            else:
                assert np.array_equal(kept, np.delete(b.ei, k, axis=1))                      # dropped


def test_duplicate_shift():
    b = P.base('small')
    E = b.ei.shape[1]
    k, i, j = _a_position(E, 'second'), _a_position(E, 'first'), _a_position(E, 'last_full')
    X, Y = tuple(b.ei[:, i].tolist()), tuple(b.ei[:, j].tolist())
    start = P.apply(b.ei, P.with_duplicate_columns(b.ei, k, i))
    shifted = P.apply(start, P.duplicate_shift_columns(start, k, j))
    assert X != Y and _pairs(b.ei)[X] == 1 and _pairs(b.ei)[Y] == 1
    assert _pairs(start)[X] == 2 and _pairs(start)[Y] == 1 and _pairs(shifted)[X] == 1 and _pairs(shifted)[Y] == 2
    assert _pairs(shifted) - _pairs(start) == Counter({Y: 1}) and _pairs(start) - _pairs(shifted) == Counter({X: 1})


def test_directed_cycle():
    C = P.constants()
    b, at = P.directed_cycle()
    small = P.base('small')
    assert b.ei.shape[1] == small.ei.shape[1] + 3
    assert sorted(e // C.tile for e in at) == [0, 1, 2]
    arcs = [tuple(b.ei[:, e].tolist()) for e in at]
    (a, b1), (b2, c1), (c2, a2) = arcs
    assert (b1, c1, a2) == (b2, c2, a) and len({a, b1, c1}) == 3
    assert _pairs(b.ei) - _pairs(small.ei) == Counter(arcs)
    assert np.array_equal(np.bincount(b.ei[0], minlength=b.n), np.bincount(b.ei[1], minlength=b.n))   # in- = out-degree everywhere
    assert not R.is_symmetric_multiset(b.ei)


def test_hub_base():
    b = P.hub_base(200)
    deg = np.bincount(b.ei[1], minlength=b.n)
    assert 128 < deg[9] <= 256 and int((deg > 128).sum()) == 1 and R.is_symmetric_multiset(b.ei)


@pytest.mark.parametrize('where', ['first', 'last'])
def test_degenerate_lists(where):
    assert P.degenerate_sizes() == (1, 2, 3, P.constants().tile - 1, P.constants().tile, P.constants().tile + 1)
    for E in P.degenerate_sizes():
        ei, n, k = P.degenerate(E, where)
        assert ei.shape == (2, E) and int(ei.max()) < n and k == (0 if where == 'first' else E - 1)
        assert tuple(ei[:, k].tolist()) == (40, 41) and not R.is_symmetric_multiset(ei)
        assert R.is_symmetric_multiset(np.delete(ei, k, axis=1))


@pytest.mark.parametrize('form', P.FORMS)
@pytest.mark.parametrize('E', [1, 2, 3, 4096, 4097, 13288, 13289])
def test_forms_have_the_row_addresses_they_claim(form, E):
    pitch, first = P.form_layout(form, E)
    buf = torch.zeros((2, pitch), dtype=torch.int64)
    assert buf.data_ptr() % 16 == 0
    ei = P.form_view(buf, form, E)
    assert tuple(ei.shape) == (2, E)
    src, dst = ei[0].contiguous(), ei[1].contiguous()   # (as build_csr takes them: views, no copy)
    assert src.data_ptr() == buf.data_ptr() + 8 * first and dst.data_ptr() == src.data_ptr() + 8 * pitch
    assert (src.data_ptr() % 16, dst.data_ptr() % 16) == P.form_offsets(form)
    if form == 'dst_off' and E % 2:
        assert ei.is_contiguous()      # the contiguous [2, E] of an odd E
    if form == 'aligned' and E % 2 == 0:
        assert ei.is_contiguous()
