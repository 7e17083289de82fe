"""The three device words of ss_csr_build_symmetric -- FingerprintWords.skip, csr.symmetric, csr.n_self_dev -- on the edge lists, forms
and edits of csr_words_planted.py: one edge changed at every tile class, offset and fingerprint loop, in every way the two rows can
lie in memory.  Every expectation is exact: the words are compared with their numpy values, rowptr with the counts of the list that
is supposed to be in place, every row's sources as a multiset with that list's.

Each base list is uploaded once; the forms are device copies of it and every edit is made on the device on one or two columns of a
clone.  After every build, rebuilt or skipped, the CSR itself is compared on the device with the list it should describe (_expect,
checked once per base against oracle.csr_build).

The symmetry product runs tile class x offset x form in full on `small` and `two_level`; on `reducer` (2.1 M edges per build) the tile
classes are crossed with the offsets {0, 1, kTile - 1} only -- its purpose is the tile, not the slot."""
import functools

import numpy as np
import pytest
import torch

import csr_words_planted as P
import symmetric_self_restatement as R

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


# ---- lists on the device ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _uploaded(name):
    """the one upload of a base list"""
    return torch.from_numpy(P.base(name).ei).to('cuda:0')


def _in_form(ei_dev, form):
    """a fresh [2, pitch] buffer holding the list in `form` -> the [2, E] view build_csr is handed"""
    E = ei_dev.size(1)
    pitch, _ = P.form_layout(form, E)
    buf = torch.zeros((2, pitch), dtype=torch.int64, device=ei_dev.device)
    ei = _view(buf, form, E)
    ei.copy_(ei_dev)
    return ei


def _view(buf, form, E):
    ei = P.form_view(buf, form, E)
    assert buf.data_ptr() % 16 == 0 and ei[0].is_contiguous() and ei[1].is_contiguous()
    assert (ei[0].data_ptr() % 16, ei[1].data_ptr() % 16) == P.form_offsets(form), 'the form degraded to another'
    return ei


def _edited(ei, form, columns):
    """a clone of the list (and of its buffer: the same form) with these columns overwritten"""
    E = ei.size(1)
    pitch, first = P.form_layout(form, E)
    buf = torch.as_strided(ei, (2, pitch), (pitch, 1), ei.storage_offset() - first).clone()
    out = _view(buf, form, E)
    pos = torch.tensor([c[0] for c in columns], dtype=torch.int64, device=ei.device)
    out[:, pos] = torch.tensor([[c[1] for c in columns], [c[2] for c in columns]], dtype=torch.int64, device=ei.device)
    return out


def _clone(ei, form):
    return _edited(ei, form, [])


# ---- what a list should build -----------------------------------------------------------------------------------------------------
def _expect(ei, n):
    """(rowptr, sorted row << 32 | source keys) of the list on the device, with what the build documents for ids out of range: a
    destination out of range is dropped, a source out of range is stored as source 0"""
    src, dst = ei[0], ei[1]
    keep = (dst >= 0) & (dst < n)
    src = torch.where((src < 0) | (src >= n), torch.zeros_like(src), src)[keep]
    dst = dst[keep]
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=ei.device)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return rowptr, torch.sort((dst << 32) | src).values


def _check_csr(csr, want, what):
    rowptr, keys = want
    assert torch.equal(csr.rowptr, rowptr), f'{what}: rowptr'
    m, n = keys.numel(), csr.num_nodes
    rows = torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1], output_size=m)
    got = torch.sort((rows << 32) | csr.col[:m].to(torch.int64)).values
    assert torch.equal(got, keys), f'{what}: the rows do not hold the sources of this list'


def _check_against_oracle(csr, ei_np, n):
    """the full comparison, once per base: oracle.csr_build on the host"""
    from oracle import oracle
    kept = P.kept_edges(ei_np, n)
    rowptr, col = oracle.csr_build(n, kept)
    m = kept.shape[1]
    assert np.array_equal(csr.rowptr.cpu().numpy(), rowptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    got = csr.col.cpu().numpy()[:m].astype(np.int64)
    assert np.array_equal(np.sort((rows << 32) | got), np.sort((rows << 32) | col[:m].astype(np.int64)))


class Built(object):
    """one CsrGraph built with a fingerprint, and rebuilt in place through `reuse`"""

    def __init__(self, ssa, dev, ei, n, **kw):
        self.ssa, self.dev, self.n = ssa, dev, n
        self.csr = ssa.hashing.build_csr(ei, n, dev, check=False, fingerprint=True, **kw)
        assert self.csr.fingerprint is not None

    def again(self, ei, **kw):
        got = self.ssa.hashing.build_csr(ei, self.n, self.dev, check=False, reuse=self.csr, fingerprint=True, **kw)
        assert got is self.csr, 'the build was not handed to the cached CSR'
        return self

    @property
    def skip(self):
        return int(self.csr.fingerprint.view(torch.int32)[5].item())   # FingerprintWords.skip of the last build

    @property
    def symmetric(self):
        return int(self.csr.symmetric.item())

    @property
    def n_self(self):
        return int(self.csr.n_self_dev.item())

    def words(self):
        return self.skip, self.symmetric, self.n_self


def _positions(name, E):
    tile = P.constants().tile
    return P.positions(E, offsets=(0, 1, tile - 1) if name.startswith('reducer') else None)


# ---- the symmetry word ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', P.FORMS)
@pytest.mark.parametrize('name', P.BASES)
def test_symmetry_word_sees_one_edge_anywhere(ssa, dev, name, form):
    """the base says 1; edge k -> a self edge says 0 (its reverse stands alone, in another tile); the columns of k and of a copy of
    its reverse exchanged say 1 again, from a rebuild -- at every planted position"""
    b = P.base(name)
    E = b.ei.shape[1]
    ei = _in_form(_uploaded(name), form)
    want = _expect(ei, b.n)
    built = Built(ssa, dev, ei, b.n)
    assert built.words() == (0, 1, b.n - 1)
    _check_csr(built.csr, want, 'base')
    if form == 'aligned':
        _check_against_oracle(built.csr, b.ei, b.n)
    for cls, tile, off, k in _positions(name, E):
        what = f'{cls} tile {tile} offset {off}'
        alone = _edited(ei, form, P.to_self_columns(b.ei, k))
        assert built.again(alone).words() == (0, 0, b.n - 1), f'to_self, {what}'
        _check_csr(built.csr, _expect(alone, b.n), f'to_self, {what}')
        swapped = _edited(ei, form, P.swap_with_reverse_columns(b.ei, k))
        assert built.again(swapped).words() == (0, 1, b.n - 1), f'swap_with_reverse, {what}'
        _check_csr(built.csr, want, f'swap_with_reverse, {what}')


@pytest.mark.parametrize('name', P.BASES)
def test_symmetry_word_sees_a_retargeted_and_a_reversed_edge(ssa, dev, name):
    """aligned rows (the 16-byte loads), the second edge of every tile class: (u, v) -> (u, w) and (u, v) -> (v, u) say 0, the base 1"""
    b = P.base(name)
    ei = _in_form(_uploaded(name), 'aligned')
    want = _expect(ei, b.n)
    built = Built(ssa, dev, ei, b.n)
    assert built.words() == (0, 1, b.n - 1)
    for cls, tile, off, k in P.positions(b.ei.shape[1], offsets=(1,)):
        if off != 1:
            continue
        for edit in (P.retarget_columns, P.reverse_one_columns):
            what = f'{edit.__name__}, {cls} tile {tile}'
            other = _edited(ei, 'aligned', edit(b.ei, k))
            assert built.again(other).words() == (0, 0, b.n - 1), what
            _check_csr(built.csr, _expect(other, b.n), what)
            assert built.again(_clone(ei, 'aligned')).words() == (0, 1, b.n - 1), f'back from {what}'
            _check_csr(built.csr, want, f'back from {what}')


@pytest.mark.parametrize('form', P.FORMS)
def test_symmetry_word_sees_a_directed_cycle(ssa, dev, form):
    """in- and out-degree agree at every node, one arc in each of three tiles: only the pairs tell"""
    b, at = P.directed_cycle()
    assert not R.is_symmetric_multiset(b.ei)
    ei = _in_form(torch.from_numpy(b.ei).to(dev), form)
    built = Built(ssa, dev, ei, b.n)
    assert built.words() == (0, 0, b.n - 1)
    _check_csr(built.csr, _expect(ei, b.n), 'directed cycle')
    _check_against_oracle(built.csr, b.ei, b.n)
    # ... and with the three arcs turned into self edges the list is `small` again
    plain = _edited(ei, form, [(k, int(b.ei[0, k]), int(b.ei[0, k])) for k in at])
    assert built.again(plain).words() == (0, 1, b.n - 1)
    _check_csr(built.csr, _expect(plain, b.n), 'cycle taken out')


# ---- the skip word ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', P.FORMS)
@pytest.mark.parametrize('name', ('small', 'small_odd', 'reducer', 'reducer_odd', 'two_level'))
def test_fingerprint_sees_one_edge_in_every_loop(ssa, dev, name, form):
    """both halves of the first and the last pair of each load of the two-load loop and of the one-load loop, the scalar tail (odd E,
    aligned rows) and the all-scalar form (a misaligned row): one edge reversed, and one edge retargeted, is another list -- and the
    base is the base again afterwards.  Reorderings are skipped; edits that keep every per-row and per-column count are not."""
    b = P.base(name)
    E = b.ei.shape[1]
    ei = _in_form(_uploaded(name), form)
    want = _expect(ei, b.n)
    built = Built(ssa, dev, ei, b.n)
    assert built.words() == (0, 1, b.n - 1)
    _check_csr(built.csr, want, 'base')
    assert built.again(_clone(ei, form)).words() == (1, 1, b.n - 1), 'the same list in another tensor'
    _check_csr(built.csr, want, 'base, skipped')
    planted = P.fp_positions(E, P.rows_aligned(form))
    assert planted
    for (loop, which, half), k in planted.items():
        for edit in (P.reverse_one_columns, P.retarget_columns):
            what = f'{edit.__name__} in {loop} ({which}' + (f' pair, .{half}' if half else '') + f'), edge {k}'
            other = _edited(ei, form, edit(b.ei, k))
            want_other = _expect(other, b.n)
            assert built.again(other).words() == (0, 0, b.n - 1), what
            _check_csr(built.csr, want_other, what)
            if edit is P.reverse_one_columns and which in ('first', 'only'):   # the word of the kept build survives a skip
                assert built.again(_clone(other, form)).words() == (1, 0, b.n - 1), f'{what}, again'
                _check_csr(built.csr, want_other, f'{what}, skipped')
            assert built.again(_clone(ei, form)).words() == (0, 1, b.n - 1), f'back from {what}'
            _check_csr(built.csr, want, f'back from {what}')
    ks = sorted(set(planted.values()))
    k = ks[len(ks) // 2]
    # the same multiset in another order: skipped, and the CSR stays
    assert built.again(_edited(ei, form, P.swap_with_reverse_columns(b.ei, k))).words() == (1, 1, b.n - 1), 'swap_with_reverse'
    _check_csr(built.csr, want, 'swap_with_reverse')
    # two edges trade destinations: the multisets of sources and of destinations stay, the list does not
    j = P.swap_partner(b.ei, k, [e for _, _, _, e in P.positions(E)])
    traded = _edited(ei, form, P.swap_dsts_columns(b.ei, k, j))
    assert built.again(traded).words() == (0, 0, b.n - 1), 'swap_dsts'
    _check_csr(built.csr, _expect(traded, b.n), 'swap_dsts')
    # X twice and Y once -> X once and Y twice
    i = next(e for e in ks if e not in (k, j))
    cols = P.with_duplicate_columns(b.ei, k, i)
    start = _edited(ei, form, cols)
    assert built.again(start).skip == 0
    shifted = _edited(start, form, P.duplicate_shift_columns(P.apply(b.ei, cols), k, j))
    assert built.again(shifted).skip == 0, 'duplicate_shift'
    _check_csr(built.csr, _expect(shifted, b.n), 'duplicate_shift')
    assert built.again(_clone(ei, form)).words() == (0, 1, b.n - 1)
    _check_csr(built.csr, want, 'base, at the end')


def test_the_shape_is_part_of_the_fingerprint(ssa, dev):
    """the same edges under another hub threshold are rebuilt, and the hub list obeys the new threshold: node 9 has an in-degree
    between the two"""
    b = P.hub_base(200)
    deg = np.bincount(b.ei[1], minlength=b.n)
    lo, hi = 128, 256
    assert lo < deg[9] <= hi and deg.max() == deg[9]
    ei = torch.from_numpy(b.ei).to(dev)
    built = Built(ssa, dev, ei, b.n, hub_threshold=lo)
    csr, want = built.csr, _expect(ei, b.n)

    def hubs():
        return sorted(csr.hub_rows[:int(csr.hub_count.item())].tolist())

    def rebuild():
        got = ssa.csr._rebuild_csr_if_changed(csr, ei[0], ei[1], None)
        assert got is csr
        _check_csr(csr, want, f'threshold {csr.hub_threshold}')
        return built.skip

    assert built.skip == 0 and hubs() == np.flatnonzero(deg > lo).tolist() == [9]
    assert rebuild() == 1 and hubs() == [9]
    csr.hub_threshold = hi
    assert rebuild() == 0 and hubs() == np.flatnonzero(deg > hi).tolist() == []
    assert rebuild() == 1 and hubs() == []
    csr.hub_threshold = lo
    assert rebuild() == 0 and hubs() == [9]
    assert built.symmetric == 1 and built.n_self == b.n - 1


# ---- n_self -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', P.FORMS)
@pytest.mark.parametrize('name', P.BASES)
def test_n_self_sees_the_one_largest_id_anywhere(ssa, dev, name, form):
    """the one occurrence of id n - 1, as a source and as a destination, at every planted position: n_self is n on a fresh build and
    on a rebuild, n - 1 on the base before and after"""
    b = P.base(name)
    ei = _in_form(_uploaded(name), form)
    want = _expect(ei, b.n)
    built = Built(ssa, dev, ei, b.n)
    assert built.words() == (0, 1, P.n_self(b.ei)) and P.n_self(b.ei) == b.n - 1
    for nth, (cls, tile, off, k) in enumerate(_positions(name, b.ei.shape[1])):
        for row in (0, 1):
            what = f'id n - 1 in row {row}, {cls} tile {tile} offset {off}'
            cols = P.max_id_columns(b.ei, k, b.n, row)
            assert P.n_self(P.apply(b.ei, cols)) == b.n
            raised = _edited(ei, form, cols)
            assert built.again(raised).words() == (0, 0, b.n), what
            _check_csr(built.csr, _expect(raised, b.n), what)
            if row == nth % 2:
                fresh = Built(ssa, dev, raised, b.n)
                assert fresh.words() == (0, 0, b.n), f'{what}, fresh build'
            assert built.again(_clone(ei, form)).words() == (0, 1, b.n - 1), f'back from {what}'
        _check_csr(built.csr, want, f'back at {cls} tile {tile} offset {off}')


# ---- ids out of range -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', P.FORMS)
@pytest.mark.parametrize('name', P.BASES)
def test_an_id_out_of_range_is_reported_from_any_tile(ssa, dev, name, form):
    """id n as a source (stored as source 0) and as a destination (dropped) at the second edge of every tile class: the flag is set,
    the list is not symmetric, n_self is that of the ids as given; a skipped rebuild of the same list reports again into a zeroed
    flag; the repaired list clears the report"""
    b = P.base(name)
    ei = _in_form(_uploaded(name), form)
    want = _expect(ei, b.n)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    built = Built(ssa, dev, ei, b.n, err_flag=flag)
    assert built.words() == (0, 1, b.n - 1) and int(flag.item()) == 0
    for cls, tile, off, k in P.positions(b.ei.shape[1], offsets=(1,)):
        if off != 1:
            continue
        for row in (0, 1):
            what = f'id n in row {row}, {cls} tile {tile}'
            cols = P.bad_id_columns(b.ei, k, b.n, row)
            assert P.n_self(P.apply(b.ei, cols)) == b.n + 1
            bad = _edited(ei, form, cols)
            want_bad = _expect(bad, b.n)
            assert int(want_bad[0][-1]) == b.ei.shape[1] - row
            assert built.again(bad, err_flag=flag).words() == (0, 0, b.n + 1), what
            assert int(flag.item()) == 1, what
            _check_csr(built.csr, want_bad, what)
            flag.zero_()
            assert built.again(_clone(bad, form), err_flag=flag).words() == (1, 0, b.n + 1), f'{what}, skipped'
            assert int(flag.item()) == 1, f'{what}: a skipped build reports what the kept build met'
            _check_csr(built.csr, want_bad, f'{what}, skipped')
            flag.zero_()
            assert built.again(_clone(ei, form), err_flag=flag).words() == (0, 1, b.n - 1), f'{what}, repaired'
            assert int(flag.item()) == 0, f'{what}, repaired'
            _check_csr(built.csr, want, f'{what}, repaired')
            assert built.again(_clone(ei, form), err_flag=flag).words() == (1, 1, b.n - 1) and int(flag.item()) == 0


# ---- the smallest lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', P.FORMS)
@pytest.mark.parametrize('where', ['first', 'last'])
@pytest.mark.parametrize('E', P.degenerate_sizes())
def test_degenerate_lists(ssa, dev, E, where, form):
    """one edge without its reverse, first or last of 1 .. kTile + 1 edges"""
    ei_np, n, k = P.degenerate(E, where)
    assert not R.is_symmetric_multiset(ei_np)
    ei = _in_form(torch.from_numpy(ei_np).to(dev), form)
    built = Built(ssa, dev, ei, n)
    assert built.words() == (0, 0, P.n_self(ei_np)) and P.n_self(ei_np) == 42
    _check_csr(built.csr, _expect(ei, n), 'first build')
    _check_against_oracle(built.csr, ei_np, n)
    assert built.again(_clone(ei, form)).words() == (1, 0, 42)
    mended_np = P.apply(ei_np, [(k, 40, 40)])
    assert R.is_symmetric_multiset(mended_np)
    mended = _edited(ei, form, [(k, 40, 40)])
    assert built.again(mended).words() == (0, 1, P.n_self(mended_np))
    _check_csr(built.csr, _expect(mended, n), 'the lone edge made a self edge')
    assert built.again(_clone(ei, form)).words() == (0, 0, 42)
    _check_csr(built.csr, _expect(ei, n), 'and back')
