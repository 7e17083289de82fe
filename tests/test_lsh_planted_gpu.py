"""The three kernels of csrc/ss_lsh.hip (band keys, count, fill) on PLANTED MinHash tables (lsh_planted.py): tables made so that a
tile shape of the keys kernel, a bucket size of the 16-lane walk, a partly filled wavefront or a row offset beyond 4 GiB is reached on
purpose.  test_lsh_gpu.py takes its tables from graphs, which decide the buckets themselves.

  a. tile geometry   every (P, rows, bands) of lsh_planted.TILE_CASES at N in {T, T + 1, 2 T - 1, 3 T + 5}, T = min(64, 8192 // P):
                     T = 64 / 42 / 16 / 8 / 4, P = 4, rows * bands not a multiple of 4, a last workgroup of 1 .. T rows; N = 1, N = 2.
                     index.keys against the numpy restatement of band_key, index.perm as a permutation that sorts them.
  b. rounds          buckets of 2, 15, 16, 17, 31, 32, 33, 48 and 49 members, max_bucket = m and m - 1 for each, key_bits 1 / 6 / 64.
  c. wavefronts      bands in {1, 3, 5}: sources out of range between good ones in one wavefront, S * bands = 1, < 4, not 0 mod 16.
  d. > 4 GiB         an int32 table of 8 650 752 rows of 512 bytes made on the device, groups across rows 2^22 and 2^23.

References: lsh_restatement.lsh_candidates on the table (a - c) and lsh_planted.expected from the plan alone (d; pinned on the
restatement for every small case by test_lsh_host.py).  Everything is an integer and compared exactly.  Every test asserts of its own
expectation that at least half the sources have a candidate and none has all N - 1 (the one- and two-node tables cannot).

Not covered: the key index j * N + v beyond 2^31 ELEMENTS needs bands * N >= 2^31 -- more than 25 GB of index and a sort of it, which
is no test of a few seconds.  The 64-bit form of that product in the kernels is read, not run."""
from argparse import Namespace
import gc

import numpy as np
import pytest
import torch

import lsh_planted as planted
import lsh_restatement as restated
from large_table_helpers import GB, NEEDS_ONE_TABLE, release_all, require_free_memory

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


def _eh(ssa, P=128):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    return eh


def _assert_same(got, want, where):
    rowptr, ids, bands = got
    assert rowptr.dtype == torch.int64 and ids.dtype == torch.int64 and bands.dtype == torch.int32
    assert rowptr.device == where and ids.device == where and bands.device == where
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(ids.cpu().numpy(), want[1])
    np.testing.assert_array_equal(bands.cpu().numpy(), want[2])


def _rows(got):
    rowptr, ids, bands = (t.cpu().numpy() for t in got)
    return [(ids[a:b], bands[a:b]) for a, b in zip(rowptr[:-1], rowptr[1:])]


def _device_table(table, groups, N, P, rows, bands, seed, dev, near=()):
    """the numpy table on the device; the torch twin of the generator makes the same one there"""
    t = torch.from_numpy(table).to(dev)
    assert torch.equal(planted.planted_table_torch(N, P, rows, bands, groups, seed, dev, block=max(1, N // 3), near=near), t)
    return {1: {'minhash': t}}


def _check_keys_and_perm(index, table, rows, b, key_bits=64):
    """per band: the sorted keys are the sorted restated band keys, perm is a permutation, and the restated key of perm[i] is keys[i]
    (which node of a run of equal keys comes first is torch.sort's choice and not looked at)"""
    N = table.shape[0]
    want = planted.band_keys(table, rows, b, key_bits)
    keys, perm = index.keys.cpu().numpy(), index.perm.cpu().numpy()
    assert keys.shape == (b, N) and perm.shape == (b, N) and keys.dtype == np.int64 and perm.dtype == np.int32
    np.testing.assert_array_equal(keys, np.sort(want, axis=1))
    np.testing.assert_array_equal(np.sort(perm, axis=1), np.broadcast_to(np.arange(N, dtype=np.int32), (b, N)))
    np.testing.assert_array_equal(np.take_along_axis(want, perm.astype(np.int64), axis=1), keys)


# a ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1, 2, 3])
@pytest.mark.parametrize('P,rows,bands', planted.TILE_CASES)
def test_tile_geometry(ssa, dev, P, rows, bands, which):
    N = planted.tile_sizes(P)[which]
    b = planted.resolve_bands(P, rows, bands)
    groups, src = planted.tile_plan(P, rows, bands, N)
    table = planted.planted_table(N, P, rows, bands, groups, seed=N + P)
    want = restated.lsh_candidates(table, src, rows, b)
    assert planted.nontrivial(want[0], N), 'a trivial expectation checks nothing'
    eh = _eh(ssa, P)
    index = eh.build_lsh_index(_device_table(table, groups, N, P, rows, bands, N + P, dev), hop=1, rows=rows, bands=bands)
    assert (index.rows, index.bands, index.num_nodes, index.num_perm) == (rows, b, N, P)
    _check_keys_and_perm(index, table, rows, b)
    np.testing.assert_array_equal(index.skipped_buckets.cpu().numpy(), np.zeros(b, dtype=np.int64))
    _assert_same(eh.lsh_candidates(torch.from_numpy(src).to(dev), index), want, dev)
    two = eh.lsh_candidates(torch.from_numpy(src).to(dev), index, min_bands=2)
    _assert_same(two, restated.lsh_candidates(table, src, rows, b, min_bands=2), dev)


def test_one_and_two_node_tables(ssa, dev):
    """N = 1: every row is empty and nothing faults; N = 2: each node lists the other, in both planted bands"""
    for N, P, rows, bands, groups, src in ((1, 12, 1, 5, [], [0, -1, 0]), (2, 128, 4, None, [([1, 0], [0, 31])], [0, 1, -1])):
        src = np.array(src, dtype=np.int64)
        b = planted.resolve_bands(P, rows, bands)
        table = planted.planted_table(N, P, rows, bands, groups, seed=N + P)
        eh = _eh(ssa, P)
        index = eh.build_lsh_index(_device_table(table, groups, N, P, rows, bands, N + P, dev), hop=1, rows=rows, bands=bands)
        _check_keys_and_perm(index, table, rows, b)
        got = eh.lsh_candidates(torch.from_numpy(src).to(dev), index)
        _assert_same(got, restated.lsh_candidates(table, src, rows, b), dev)
        _assert_same(got, planted.expected(N, rows, b, groups, src, 1024)[0], dev)
        assert got[1].numel() == (0 if N == 1 else 3)
        eh.check_errors()


# b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rounds(dev):
    """(groups, by_size, numpy table, the table on the device); read only"""
    N, P, rows = planted.ROUND_N, planted.ROUND_P, planted.ROUND_ROWS
    groups, by_size = planted.round_plan()
    near = planted.round_near(groups)  # rows one word away from every bucket
    table = planted.planted_table(N, P, rows, None, groups, seed=N + P, near=near)
    return groups, by_size, table, _device_table(table, groups, N, P, rows, None, N + P, dev, near=near)


def _by_position(index, groups):
    """the first, a middle and the last member of every group as its first band's sorted order places them"""
    perm = index.perm.cpu().numpy()
    out = []
    for members, band_set in groups:
        at = np.nonzero(np.isin(perm[band_set[0]], members))[0]
        assert len(at) == len(members) and at[-1] - at[0] == len(members) - 1, 'the members of a bucket are neighbours in the order'
        out += [int(perm[band_set[0]][i]) for i in (at[0], at[len(at) // 2], at[-1])]
    return out


def test_round_boundaries_default_max_bucket(ssa, dev, rounds):
    groups, by_size, table, on_dev = rounds
    N, rows, b = planted.ROUND_N, planted.ROUND_ROWS, 32
    eh = _eh(ssa)
    index = eh.build_lsh_index(on_dev, hop=1, rows=rows)
    _check_keys_and_perm(index, table, rows, b)
    src = np.concatenate([planted.round_sources(groups), np.array(_by_position(index, groups), dtype=np.int64)])
    want = restated.lsh_candidates(table, src, rows)
    assert planted.nontrivial(want[0], N) and set(planted.ROUND_SIZES) <= planted.bucket_sizes(N, b, groups, src)
    assert {1, 3, 4, 5, 32} <= set(want[2].tolist())
    _assert_same(eh.lsh_candidates(torch.from_numpy(src).to(dev), index), want, dev)
    np.testing.assert_array_equal(index.skipped_buckets.cpu().numpy(), np.zeros(b, dtype=np.int64))


@pytest.mark.parametrize('m', planted.ROUND_SIZES)
def test_round_boundaries_at_max_bucket(ssa, dev, rounds, m):
    """max_bucket = m lists the bucket of m members, max_bucket = m - 1 skips it (and counts it)"""
    groups, by_size, table, on_dev = rounds
    N, rows = planted.ROUND_N, planted.ROUND_ROWS
    members, band = by_size[m]
    eh = _eh(ssa)
    for cap, listed in ((m, True), (m - 1, False)):
        index = eh.build_lsh_index(on_dev, hop=1, rows=rows, max_bucket=cap)
        # the sources of every group (compared only: at a small max_bucket most of their buckets are skipped) ...
        wide = np.concatenate([planted.round_sources(groups), np.array(_by_position(index, groups), dtype=np.int64)])
        _assert_same(eh.lsh_candidates(torch.from_numpy(wide).to(dev), index), restated.lsh_candidates(table, wide, rows, max_bucket=cap), dev)
        # ... and this group's own: a few background rows, its first / middle / last member by position, then every member
        background = [int(v) for v in planted.round_sources(groups)[-22:-2][:min(10, m)]]
        src = np.array(background + _by_position(index, [(members, [band])]) + members, dtype=np.int64)
        want = restated.lsh_candidates(table, src, rows, max_bucket=cap)
        assert not listed or planted.nontrivial(want[0], N)
        got = eh.lsh_candidates(torch.from_numpy(src).to(dev), index)
        _assert_same(got, want, dev)
        for ids, shared in _rows(got)[-m:]:  # the members themselves
            assert ids.size == (m - 1 if listed else 0) and (shared == 1).all()
        skipped = index.skipped_buckets.cpu().numpy()
        np.testing.assert_array_equal(skipped, restated.skipped_buckets(table, rows, max_bucket=cap))
        assert skipped[band] == (0 if listed else 1) + (3 > cap)  # (the group of three is in every band)


def test_clipped_search_under_a_six_bit_key(ssa, dev, rounds):
    """64 keys for 601 nodes: every key range is full of false matches, and max_bucket = 26 applies to the RANGE (lsh.py's module
    text), so the group of 17 is dropped with its range of 28 while the groups of 15 and 16 are listed out of ranges of 25.  Their
    ranges start inside the band's order with more than max_bucket + 1 entries to go: the second binary search is clipped.
    The expectation is the restatement's, handed the key-range sizes (lsh_planted.candidates_under_keys: slice equality decides
    membership, the restated band_key decides which bands of a source are dropped) -- an exact comparison, not only the two
    documented properties."""
    groups, by_size, table, on_dev = rounds
    N, rows, cap = planted.ROUND_N, planted.ROUND_ROWS, planted.SIX_BIT_MAX_BUCKET
    src = planted.six_bit_sources(groups)
    want, skipped = planted.candidates_under_keys(table, src, rows, None, cap, 6)
    keys = planted.band_keys(table, rows, None, 6)
    runs = planted.key_run_lengths(keys)
    seen = set()
    for m in (15, 16, 17):
        u, band = by_size[m][0][0], by_size[m][1]
        assert (keys[band] < keys[band][u]).sum() > 0 and (keys[band] >= keys[band][u]).sum() > cap + 1
        seen.add(bool(runs[band][u] <= cap))
        assert m <= cap and runs[band][u] > m
    assert seen == {True, False} and planted.nontrivial(want[0], N)
    eh = _eh(ssa)
    index = eh.build_lsh_index(on_dev, hop=1, rows=rows, max_bucket=cap, _key_bits=6)
    _check_keys_and_perm(index, table, rows, 32, 6)
    np.testing.assert_array_equal(index.skipped_buckets.cpu().numpy(), skipped)
    _assert_same(eh.lsh_candidates(torch.from_numpy(src).to(dev), index), want, dev)


@pytest.mark.parametrize('key_bits', [1, 64])
def test_round_boundaries_under_other_key_widths(ssa, dev, rounds, key_bits):
    """_key_bits = 1: two ranges of about 300 nodes per band, every planted bucket found among the false matches (max_bucket = N),
    the rows that miss a bucket by one word among them (test_lsh_host.py: some of every kind share the range);
    _key_bits = 64: the default, said aloud"""
    groups, by_size, table, on_dev = rounds
    N, rows = planted.ROUND_N, planted.ROUND_ROWS
    eh = _eh(ssa)
    index = eh.build_lsh_index(on_dev, hop=1, rows=rows, max_bucket=N, _key_bits=key_bits)
    _check_keys_and_perm(index, table, rows, 32, key_bits)
    assert key_bits == 64 or set(torch.unique(index.keys).tolist()) == {0, 1}
    src = np.concatenate([planted.round_sources(groups), np.array(_by_position(index, groups), dtype=np.int64)]) if key_bits == 64 \
        else planted.round_sources(groups)
    want = restated.lsh_candidates(table, src, rows, max_bucket=N)
    assert planted.nontrivial(want[0], N) and set(planted.ROUND_SIZES) <= planted.bucket_sizes(N, 32, groups, src)
    _assert_same(eh.lsh_candidates(torch.from_numpy(src).to(dev), index), want, dev)
    assert int(index.skipped_buckets.sum()) == 0


# c ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', planted.WAVE_BANDS)
def test_partly_filled_wavefronts(ssa, dev, b):
    """16 items (source, band) per workgroup, 4 per wavefront: with 1, 3 or 5 bands a source out of range shares its wavefront with
    its neighbours, and the last wavefront is partly empty.  Device ids, deferred reporting (the default)."""
    N, P, rows = planted.WAVE_N, planted.WAVE_P, planted.WAVE_ROWS
    groups, good = planted.wave_plan(b)
    table = planted.planted_table(N, P, rows, b, groups, seed=N + P)
    eh = _eh(ssa)
    index = eh.build_lsh_index(_device_table(table, groups, N, P, rows, b, N + P, dev), hop=1, rows=rows, bands=b)
    _check_keys_and_perm(index, table, rows, b)

    def ask(ids):
        return eh.lsh_candidates(torch.tensor(ids, dtype=torch.int64, device=dev), index)

    alone = {}
    for u in good:  # S * b = b: 1, 3 and 5 live rows
        got = ask([u])
        _assert_same(got, restated.lsh_candidates(table, [u], rows, b), dev)
        alone[u] = _rows(got)[0]
    eh.check_errors()
    assert np.mean([alone[u][0].size > 0 for u in good]) >= 0.5 and max(alone[u][0].size for u in good) < N - 1
    assert {2, 3, 4, 5} <= planted.bucket_sizes(N, b, groups, good)  # (every planted size, all of them inside one round)
    for S in (1, 2, 3, 17):  # S * b is 1, below 4, and no multiple of 16
        want = restated.lsh_candidates(table, good[:S], rows, b)
        assert planted.nontrivial(want[0], N)
        _assert_same(ask(good[:S]), want, dev)
    eh.check_errors()
    mixed = [good[0], N, good[1], -N - 1, good[2], good[3]]
    long = list(good[:17])
    for at, bad in ((1, N), (3, -N - 1), (8, N + 5), (16, 1 << 40)):
        long[at] = bad
    for ids in (mixed, long, [N], [-N - 1, good[4]], [good[5], N, good[6]]):
        got = ask(ids)
        with pytest.raises(IndexError):
            eh.check_errors()
        eh.check_errors()  # (reported once)
        for u, (cand, shared) in zip(ids, _rows(got)):
            if -N <= u < N:
                assert np.array_equal(cand, alone[u][0]) and np.array_equal(shared, alone[u][1])
            else:
                assert cand.size == 0


# d ---------------------------------------------------------------------------------------------------------------------------------
def test_table_of_more_than_4_gib(ssa, dev):
    """an int32 [8 650 752, 128] table (4.43 GB; row 2^22 starts at byte 2^31, row 2^23 at byte 2^32) made on the device by the torch
    twin of the generator, rows = 2, bands = 4 (a 0.42 GB index); a dozen groups across both boundaries, N - 1 and 0.  Against
    lsh_planted.expected (the plan alone), and index.keys at every source row against the restated band_key of that row."""
    release_all(dev)
    N, P, rows, b = planted.LARGE_N, planted.LARGE_P, planted.LARGE_ROWS, planted.LARGE_BANDS
    require_free_memory(dev, NEEDS_ONE_TABLE, 'the LSH index over a 4.43 GB table')  # (what the 4.43 GB spmm operand asks for)
    torch.cuda.reset_peak_memory_stats(dev)
    groups, src = planted.large_plan()
    want, skipped = planted.expected(N, rows, b, groups, src, 1024)
    assert planted.nontrivial(want[0], N) and {17, 33} <= planted.bucket_sizes(N, b, groups, src)
    t = planted.planted_table_torch(N, P, rows, b, groups, 7, dev, dtype=torch.int32)
    assert t.numel() * 4 > (1 << 32) and t.dtype == torch.int32
    eh = _eh(ssa)
    index = eh.build_lsh_index({1: {'minhash': t}}, hop=1, rows=rows, bands=b)
    assert index.mh_u32.data_ptr() == t.data_ptr() and index.nbytes == 12 * b * N + 8 * b
    _assert_same(eh.lsh_candidates(torch.from_numpy(src).to(dev), index), want, dev)
    np.testing.assert_array_equal(index.skipped_buckets.cpu().numpy(), skipped)
    # keys sorted, perm a permutation, and the key found at the place of every source row is the restated key of that row
    assert bool((index.keys[:, 1:] >= index.keys[:, :-1]).all())
    at = torch.from_numpy(np.where(src < 0, src + N, src)).to(dev)
    host_rows = t.index_select(0, at).cpu().numpy().view(np.uint32).astype(np.int64)
    restated_keys = planted.band_keys(host_rows, rows, b)
    everyone = torch.arange(N, dtype=torch.int64, device=dev)
    for j in range(b):
        assert int(index.perm[j].min()) >= 0 and int(index.perm[j].max()) < N
        place = torch.zeros((N,), dtype=torch.int64, device=dev)
        place[index.perm[j].to(torch.int64)] = everyone
        assert torch.equal(index.perm[j][place].to(torch.int64), everyone), 'perm is no permutation'
        np.testing.assert_array_equal(index.keys[j][place[at]].cpu().numpy(), restated_keys[j])
    eh.check_errors()
    peak = torch.cuda.max_memory_allocated(dev)
    print(f'\n[lsh planted] 4 GiB case: peak torch.cuda.max_memory_allocated() = {peak} bytes ({peak / GB:.2f} GiB)')
    del index, t, place, everyone
    gc.collect()  # (the packed twin is cached ON the table tensor: a cycle)
    torch.cuda.empty_cache()
