"""The planted CSRs of sort_rows_planted.py without a GPU: the plan reaches every path, pass count, copy-back parity and tail of
ss_csr_sort_rows that its docstring names; the tie patterns put thread boundaries of every merge inside runs of equal values (a
numpy restatement of the merge path); the library's workspace formula and the argument checks that run before anything is
launched."""
import ctypes

import numpy as np
import pytest

import sort_rows_planted as P


def test_the_length_helpers_restate_the_contract():
    # (length: chunks, passes, copied back, last chunk, a partnerless run) -- worked out by hand from the kernel's two loops
    want = {16384: (1, 0, False, 16384, False), 16385: (2, 1, True, 1, False), 20000: (2, 1, True, 3616, False),
            32768: (2, 1, True, 16384, False), 32769: (3, 2, False, 1, True), 49152: (3, 2, False, 16384, True),
            49153: (4, 2, False, 1, False), 65536: (4, 2, False, 16384, False), 65537: (5, 3, True, 1, True),
            131073: (9, 4, False, 1, True)}
    for n, w in want.items():
        assert (P.chunks(n), P.passes(n), P.copies_back(n), P.last_chunk(n), P.has_lone_run(n)) == w, n
    assert P.merges(32769) == [(0, 0, 16384, 16384), (0, 32768, 1, 0), (1, 0, 32768, 1)]
    assert [P.row_path(n, [n, 3]) for n in (0, 1, 2, 16)] == ['lanes16'] * 4
    assert [P.row_path(n, [n, 17]) for n in (0, 1, 2, 16, 17, 64, 65, 16384, 16385)] == \
        ['wave_skip', 'wave_skip', 'wave', 'wave', 'wave', 'wave', 'lds', 'lds', 'merge']


def test_the_plan_is_not_trivial():
    blocks = P.base_blocks()
    lengths = P.base_lengths()
    assert len(lengths) % 4 == 0 and all(len(b) == 4 for _, b in blocks)
    paths = P.row_paths(lengths)
    assert set(paths) == {'lanes16', 'wave', 'wave_skip', 'lds', 'merge'}
    merged = [n for n in lengths if n > P.LDS]
    assert {P.passes(n) for n in merged} == {1, 2, 3, 4}
    assert {P.copies_back(n) for n in merged} == {True, False}
    assert any(P.last_chunk(n) == 1 for n in merged) and any(P.has_lone_run(n) for n in merged)
    assert any(P.last_chunk(n) == 1 and P.has_lone_run(n) for n in merged)       # 32 769: the lone run is one entry
    assert any(P.last_chunk(n) == P.LDS for n in merged)
    assert P.listed_rows(lengths) > P.LONG_GRID
    # both sides of every threshold, in a row of its own
    for n in (16, 17, 64, 65, P.LDS, P.LDS + 1):
        assert n in lengths
    # every composition block is one wavefront, as written
    for k, (kind, b) in enumerate(blocks):
        assert lengths[4 * k:4 * k + 4] == b
    comp = [b for kind, b in blocks if kind == 'composition']
    assert comp == P.COMPOSITION
    assert [P.wave_path(b) for b in comp] == ['lanes16'] * 3 + ['wave'] * 5
    where = {tuple(b): 4 * k for k, (_, b) in enumerate(blocks)}
    assert all(where[tuple(b)] % 4 == 0 for b in comp)
    # one row of 17 puts its three short neighbours on the whole-wave path; a listed row sits beside rows the wave still sorts
    r = where[(15, 16, 17, 3)]
    assert paths[r:r + 4] == ['wave'] * 4
    r = where[(65, 2, 64, 0)]
    assert paths[r:r + 4] == ['lds', 'wave', 'wave', 'wave_skip']
    r = where[(65, 66, 127, 1025)]
    assert paths[r:r + 4] == ['lds'] * 4
    r = where[(0, 1, 2, 16)]
    assert paths[r:r + 4] == ['lanes16'] * 4
    # every long length has a block of its own, with three rows of 2 .. 16 entries, and stands in every place of a wavefront
    long_blocks = [b for kind, b in blocks if kind == 'long']
    assert sorted(max(b) for b in long_blocks) == sorted(P.LONG_LENGTHS)
    assert all(sorted(b)[:3] == sorted(x for x in b if 2 <= x <= 16) for b in long_blocks)
    assert {b.index(max(b)) for b in long_blocks} == {0, 1, 2, 3}
    assert 500_000 < sum(lengths) < 700_000


def test_the_variants_end_in_every_partial_wave():
    seen = set()
    for name in P.VARIANTS:
        lengths = P.lengths_of(name)
        tail = len(lengths) % 4
        seen.add((tail, lengths[-1] > P.WAVE))
        assert name == 'n4' or (f'last{tail}' in name and ('long' in name) == (lengths[-1] > P.WAVE))
        rowptr, col, want = P.planted(name, 'eight')
        assert rowptr[-1] == len(col) == sum(lengths) and rowptr.dtype == np.int64 and col.dtype == np.int32
    assert seen >= {(t, long) for t in (1, 2, 3) for long in (True, False)} and (0, False) in seen


@pytest.mark.parametrize('pattern', P.PATTERNS)
def test_the_patterns_are_what_they_say(pattern):
    rowptr, col, want = P.planted('n4', pattern)
    assert col.min() >= 0 and col.max() < P.PAD
    rows = [(col[a:b], want[a:b]) for a, b in zip(rowptr[:-1], rowptr[1:]) if b - a > 1]
    for row, srt in rows:
        assert (np.diff(srt.astype(np.int64)) >= 0).all() and np.array_equal(np.sort(row), srt)
    big = max(rows, key=lambda r: len(r[0]))[0].astype(np.int64)
    if pattern == 'distinct':
        assert all(len(np.unique(r)) == len(r) for r, _ in rows) and not (np.diff(big) > 0).all()
    elif pattern == 'descending':
        assert all((np.diff(r.astype(np.int64)) < 0).all() for r, _ in rows)
    elif pattern == 'ascending':
        assert all((np.diff(r.astype(np.int64)) > 0).all() for r, _ in rows)
    elif pattern == 'equal':
        assert len(np.unique(col)) == 1
    elif pattern == 'eight':
        assert len(np.unique(big)) == 8 and len(np.unique(col)) == 8
    elif pattern == 'sawtooth':
        assert np.array_equal(big[:P.LDS], big[P.LDS:2 * P.LDS]) and np.array_equal(big[:P.LDS], big[7 * P.LDS:8 * P.LDS])
        assert big[P.LDS] == 0 and big[P.LDS - 1] > big[P.LDS]
    else:
        assert 0 in big and P.PAD - 1 in big and any(0 in r and P.PAD - 1 in r for r, _ in rows if len(r) <= 16)


@pytest.mark.parametrize('pattern', P.TIE_PATTERNS + ('distinct',))
def test_thread_boundaries_of_every_merge_fall_inside_tie_runs(pattern):
    """the long kernel's merges restated: for the tie patterns, some thread of EVERY merge begins inside a run of equal values; where
    the second run has more than one entry (or the values are few), inside a run that both runs feed.  A second run of one entry
    [0] of the sawtooth cannot have that: its run of zeros is shorter than a thread's stretch.

    The restatement also shows what the values can NOT show: a search that puts B first on ties (`<`) hands every thread another
    valid split of the same prefix, and the sequential merge emits the same values from it.  For int32 keys without a payload the
    two tie rules are not distinguishable."""
    rowptr, col, want = P.planted('n4', pattern)
    n_merges = 0
    for lo, hi in zip(rowptr[:-1].tolist(), rowptr[1:].tolist()):
        if hi - lo <= P.LDS:
            continue
        got, inside = P.merge_rows_restated(col[lo:hi])
        assert np.array_equal(got, want[lo:hi])
        assert len(inside) == sum(nb > 0 for _, _, _, nb in P.merges(hi - lo))
        n_merges += len(inside)
        for nb, in_run, in_both in inside:
            if pattern == 'distinct':
                assert in_run == 0
            else:
                assert in_run > 0
                assert in_both > 0 or (pattern == 'sawtooth' and nb == 1)
        if hi - lo in (32769, 65537):
            other, _ = P.merge_rows_restated(col[lo:hi], strict_search=True)
            assert np.array_equal(other, got)
    assert n_merges == 1 + 1 + 1 + 1 + 2 + 2 + 3 + 3 + 4 + 8


# ---- the library, without a device ------------------------------------------------------------------------------------------------
def _lib():
    import subgraph_sketching_amd as ssa
    return ssa._native.lib()


def test_workspace_bytes_follow_the_formula():
    fn = _lib().ss_csr_sort_workspace_bytes
    for E in (-5, -1, 0, 1, 63, 64, 65, 127, 128, 16384, 16385, 533271, (1 << 31) - 1):
        assert fn(E) == P.workspace_bytes(E), E
    assert fn(0) == 8 + 256 + 4 and fn(64) == 12 + 256 + 256 and fn(-1) == 0
    assert fn(533271) == 2_166_676
    E = sum(P.base_lengths())
    assert E == 574_461 and fn(E) == P.workspace_bytes(E) == 2_334_008   # the base plan
    for name in P.VARIANTS:
        E = sum(P.lengths_of(name))
        assert fn(E) == 4 * E + 4 * (E // 64 + 2) + 256


def test_argument_errors_of_the_library_are_reported_without_a_gpu():
    from ctypes import c_void_p
    lib = _lib()
    fn = lib.ss_csr_sort_rows
    fake = c_void_p(256)  # never dereferenced
    INVALID, WORKSPACE, OK = -1, -3, 0  # SS_ERR_INVALID_ARG, SS_ERR_WORKSPACE, SS_OK

    def call(rowptr=fake, col=fake, N=8, E=100, only_if=None, ws=fake, ws_bytes=None):
        return fn(rowptr, col, N, E, only_if, ws, lib.ss_csr_sort_workspace_bytes(E) if ws_bytes is None else ws_bytes, None)

    for bad in (-1, 1 << 31, 1 << 40):
        assert call(N=bad) == INVALID and call(E=bad, ws_bytes=1 << 40) == INVALID
    assert call(N=(1 << 31) - 1, E=(1 << 31) - 1, ws=None) == WORKSPACE  # the largest sizes pass the range check
    assert call(rowptr=None) == INVALID and call(col=None) == INVALID
    assert call(ws=None) == WORKSPACE
    assert call(ws_bytes=lib.ss_csr_sort_workspace_bytes(100) - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    # nothing to do: OK before a pointer is looked at or anything is launched
    assert call(N=0) == OK and call(E=0) == OK
    assert call(N=0, rowptr=None, col=None, ws=None, ws_bytes=0) == OK and call(E=0, rowptr=None, col=None, ws=None, ws_bytes=0) == OK
    assert call(N=-1, E=0) == INVALID and call(N=0, E=-1) == INVALID  # (the range check comes first)
