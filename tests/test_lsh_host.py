"""The LSH index (ElphHashes.build_lsh_index / lsh_candidates / topk_links_lsh) without a GPU: the numpy restatement of
its semantics (lsh_restatement.py) against a naive double loop written here, on oracle tables; the argument checks that run before a
device is touched; the ranking key's torch form and the selection by it; the host block walk rehearsed with numpy stand-ins for the two
launches; the new entry points in the header, the bindings and the library."""
from argparse import Namespace
import collections
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, oracle_params
from score_restatement import raw_head
import lsh_planted as planted
import lsh_restatement as restated


def _eh(h=2, P=128, p=8):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))


def _oracle_tables(regenerated_tables, N, ei, P, h=2):
    from oracle import oracle
    table, _ = oracle.build_hash_tables(N, ei, h, P, oracle_params(regenerated_tables[8]))
    return {k: table[k]['minhash'].astype(np.int64) for k in range(h + 1)}


def _naive(mh, sources, rows, bands, max_bucket, exclude=None, min_bands=1):
    """the O(N^2 b) double loop over (u, v) and the bands, bucket sizes counted by a third loop"""
    N, P = mh.shape
    rowptr, ids, shared = [0], [], []
    for u in sources:
        u = int(u) + N if int(u) < 0 else int(u)
        for v in range(N):
            n = 0
            for j in range(bands):
                mine = mh[u, j * rows:(j + 1) * rows]
                if np.array_equal(mine, mh[v, j * rows:(j + 1) * rows]):
                    size = sum(1 for w in range(N) if np.array_equal(mine, mh[w, j * rows:(j + 1) * rows]))
                    n += size <= max_bucket
            gone = v == u or (exclude is not None and any((int(a) % N, int(b) % N) == (u, v) for a, b in exclude.T))
            if n >= min_bands and not gone:
                ids.append(v)
                shared.append(n)
        rowptr.append(len(ids))
    return np.array(rowptr, dtype=np.int64), np.array(ids, dtype=np.int64), np.array(shared, dtype=np.int32)


def _assert_same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize('P,hop,rows,bands', [(128, 1, 4, None), (128, 1, 2, 9), (8, 2, 4, None), (8, 1, 1, 5)])
def test_restatement_against_the_double_loop_on_ba40(regenerated_tables, P, hop, rows, bands):
    g = load_golden('g3_g4_ba40.npz')
    N, ei = int(g['num_nodes']), g['edge_index'].astype(np.int64)
    mh = _oracle_tables(regenerated_tables, N, ei, P)[hop]
    sources = np.array([0, 5, 17, -1, 5, N - 1, -N], dtype=np.int64)
    b = P // rows if bands is None else bands
    want = _naive(mh, sources, rows, b, 1024)
    assert np.mean(np.diff(want[0]) > 0) >= 0.5 and np.diff(want[0]).max() < N - 1, 'a trivial case checks nothing'
    _assert_same(restated.lsh_candidates(mh, sources, rows, bands), want)
    _assert_same(restated.lsh_candidates(mh, sources, rows, bands, min_bands=2), _naive(mh, sources, rows, b, 1024, min_bands=2))
    exclude = np.concatenate([ei[:, ::2], ei[:, :5], np.array([[0, -1, 5], [0, 3, 5 - N]])], axis=1)  # duplicates, self loops, negative ids
    _assert_same(restated.lsh_candidates(mh, sources, rows, bands, exclude=exclude), _naive(mh, sources, rows, b, 1024, exclude=exclude))
    for cap in (1, 3):  # buckets of more than `cap` members are skipped
        _assert_same(restated.lsh_candidates(mh, sources, rows, bands, max_bucket=cap), _naive(mh, sources, rows, b, cap))


def test_restatement_on_trailing_nodes_and_the_max_bucket_boundary(regenerated_tables):
    N, ei, m = restated.trailing_graph()
    mh = _oracle_tables(regenerated_tables, N, ei, 128)[1]
    assert len(np.unique(mh[N - m:], axis=0)) == 1 and len(np.unique(mh, axis=0)) == N - m + 1, 'the trailing nodes share ONE row'
    sources = np.array([0, N - m, N - 1, 7, -2], dtype=np.int64)
    rows, b = 4, 32
    for cap, listed in ((m, True), (m - 1, False), (1024, True)):
        got = restated.lsh_candidates(mh, sources, rows, max_bucket=cap)
        _assert_same(got, _naive(mh, sources, rows, b, cap))
        row = got[1][got[0][2]:got[0][3]]  # the candidates of node N - 1
        if listed:
            np.testing.assert_array_equal(row, np.arange(N - m, N - 1))
            assert (got[2][got[0][2]:got[0][3]] == b).all()
        else:
            assert row.size == 0
        np.testing.assert_array_equal(restated.skipped_buckets(mh, rows, max_bucket=cap), np.full(b, 0 if listed else 1))


def _table(N=30, P=128, p=8, h=2):
    return {k: {'minhash': torch.zeros((N, P), dtype=torch.int64), 'hll': torch.zeros((N, 1 << p), dtype=torch.int8)}
            for k in range(h + 1)}


def _index(N=30, P=128, rows=4, bands=32):
    """an LshIndex over CPU tensors: enough for every check that comes before a device is touched"""
    from subgraph_sketching_amd.lsh import LshIndex
    return LshIndex(1, rows, bands, 1024, torch.zeros((N, P), dtype=torch.int32), torch.zeros((bands, N), dtype=torch.int64),
                    torch.zeros((bands, N), dtype=torch.int32), torch.zeros((bands,), dtype=torch.int64))


def _head(h=2):
    import subgraph_sketching_amd as ssa
    return ssa.StructureHead(**raw_head(h * (h + 2), 1))


CARDS = torch.zeros((30, 2))
OK = torch.tensor([0, 1])


def test_index_properties():
    index = _index()
    assert (index.hop, index.rows, index.bands, index.num_nodes, index.num_perm, index.max_bucket) == (1, 4, 32, 30, 128, 1024)
    assert index.nbytes == 32 * 30 * 12 + 32 * 8 and index.skipped_buckets.dtype == torch.int64


@pytest.mark.parametrize('kw', [dict(rows=4, bands=33), dict(rows=5, bands=26), dict(rows=129), dict(rows=0), dict(bands=0), dict(hop=0),
                                dict(hop=3), dict(max_bucket=0), dict(_key_bits=0), dict(_key_bits=65), dict(rows=2.5)])
def test_build_arguments_are_checked_before_a_device_is_touched(kw):
    with pytest.raises(ValueError):
        _eh().build_lsh_index(_table(), **kw)


def test_query_arguments_are_checked_before_a_device_is_touched():
    eh, index = _eh(), _index()
    for min_bands in (0, -1):
        with pytest.raises(ValueError, match='min_bands'):
            eh.lsh_candidates(OK, index, min_bands=min_bands)
        with pytest.raises(ValueError, match='min_bands'):
            eh.topk_links_lsh(OK, _table(), CARDS, 5, _head(), index, min_bands=min_bands)
    with pytest.raises(ValueError, match='LshIndex'):
        eh.lsh_candidates(OK, _table())
    with pytest.raises(ValueError):
        eh.lsh_candidates(torch.tensor([[0, 1]]), index)
    with pytest.raises(ValueError):
        eh.lsh_candidates(torch.tensor([0.5]), index)
    with pytest.raises(ValueError):
        eh.lsh_candidates(OK, index, exclude=torch.tensor([0, 1, 2]))
    for bad in ([0, 30], [-31]):  # CPU ids are checked at once, as topk_links checks them
        with pytest.raises(IndexError):
            eh.lsh_candidates(torch.tensor(bad), index)
        with pytest.raises(IndexError):
            eh.topk_links_lsh(torch.tensor(bad), _table(), CARDS, 5, _head(), index)
    with pytest.raises(IndexError):
        eh.lsh_candidates(OK, index, exclude=torch.tensor([[0], [30]]))


def test_the_index_must_fit_the_table():
    eh = _eh()
    with pytest.raises(ValueError, match='index was built'):
        eh.topk_links_lsh(OK, _table(), CARDS, 5, _head(), _index(N=31))
    with pytest.raises(ValueError, match='index was built'):
        eh.topk_links_lsh(OK, _table(), CARDS, 5, _head(), _index(P=64, bands=16))
    for k in (0, -1, 31):
        with pytest.raises(ValueError, match='k must lie'):
            eh.topk_links_lsh(OK, _table(), CARDS, k, _head(), _index())
    with pytest.raises(ValueError, match='max_hash_hops'):
        eh.topk_links_lsh(OK, _table(), CARDS, 5, _head(h=3), _index())
    with pytest.raises(ValueError, match='degrees'):
        eh.topk_links_lsh(OK, _table(), CARDS, 5, _head(), _index(), degrees=torch.ones(30))
    with pytest.raises(ValueError, match='cards'):
        eh.topk_links_lsh(OK, _table(), None, 5, _head(), _index())


def test_the_ranking_key_in_torch_is_the_inverse_of_its_decoder():
    from subgraph_sketching_amd.engine import TOPK_SENTINEL, _decode_topk_keys, _encode_topk_keys
    scores = torch.tensor([0.0, -0.0, 1.5, -1.5, 3e38, -3e38, 1e-45, -1e-45, 2.0, 2.0], dtype=torch.float32)
    ids = torch.tensor([7, 7, 0, 1, 2, 3, 4, 5, 9, 8], dtype=torch.int64)
    keys = _encode_topk_keys(scores, ids)
    back_ids, back = _decode_topk_keys(keys)
    assert torch.equal(back_ids, ids)
    assert torch.equal(back.view(torch.int32), torch.where(scores == 0, torch.zeros(()), scores).view(torch.int32))  # -0.0 comes back as +0.0
    assert keys[0] == keys[1] and bool((keys > TOPK_SENTINEL).all())
    order = np.lexsort((ids.numpy(), -scores.numpy()))  # (score desc, id asc); the two zeros are one key
    assert torch.equal(torch.argsort(keys, descending=True, stable=True), torch.from_numpy(order))


def test_the_selection_against_a_lexsort():
    from subgraph_sketching_amd.candidates import _select_rows
    N, n, k = 50, 5, 3
    rows = [([7], [0.5]),                                                  # one candidate
            ([3, 20, 49], [1.0, 2.0, -1.0]),                               # exactly k
            ([1, 4, 9, 16, 25, 36], [2.0, 3.0, 2.0, 3.0, 2.0, 1.0]),       # more than k, tied scores: ids break ties ascending
            ([0, 2, 5, 8, 11], [-0.0, -2.5, 0.0, -1e-30, -0.0]),           # -0.0 and +0.0 are one key (the id decides), negative scores
            ([], [])]                                                      # none, and the last: trailing rows
    keys = torch.tensor([s * N + v for s, (ids, _) in enumerate(rows) for v in ids], dtype=torch.int64)
    sc = torch.tensor([x for _, scores in rows for x in scores], dtype=torch.float32)
    assert bool((keys[1:] > keys[:-1]).all())
    got_ids, got = _select_rows(keys, sc, n, N, k)
    assert got_ids.dtype == torch.int64 and got.dtype == torch.float32 and got_ids.shape == got.shape == (n, k)
    want_ids, want = np.full((n, k), -1, dtype=np.int64), np.full((n, k), -np.inf, dtype=np.float32)
    for s, (ids, scores) in enumerate(rows):
        ids, scores = np.array(ids, dtype=np.int64), np.array(scores, dtype=np.float32)
        order = np.lexsort((ids, -scores))[:k]  # (score desc, id asc); numpy compares the two zeros equal
        want_ids[s, :len(order)], want[s, :len(order)] = ids[order], scores[order]
    np.testing.assert_array_equal(got_ids.numpy(), want_ids)
    np.testing.assert_array_equal(got.numpy(), want)
    assert want_ids[2].tolist() == [4, 16, 1] and want_ids[3].tolist() == [0, 5, 11] and want_ids[4].tolist() == [-1] * k


# ---- the host walk, rehearsed: the two launches replaced by numpy stand-ins that read the restatement's band groups ------------------
def _rehearse(monkeypatch, mh, rows, bands, max_bucket):
    import subgraph_sketching_amd as ssa
    lsh = ssa.lsh
    N, P = mh.shape
    groups = restated.band_groups(mh, rows, bands)
    rng = np.random.RandomState(0)
    launches = collections.Counter()

    def partners(u, j):
        """the other members of u's band-j bucket: none for a skipped bucket and for an id out of range"""
        u = u + N if u < 0 else u
        if not 0 <= u < N:
            return np.zeros(0, dtype=np.int64)
        group, sizes = groups[j]
        if sizes[group[u]] > max_bucket:
            return np.zeros(0, dtype=np.int64)
        members = np.nonzero(group == group[u])[0]
        return members[members != u]

    def count(index, sources, counts, err):
        launches['count'] += 1
        assert counts.shape == (sources.numel() * bands,) and counts.dtype == torch.int32
        counts.copy_(torch.tensor([len(partners(u, j)) for u in sources.tolist() for j in range(bands)], dtype=torch.int32))

    def fill(index, sources, offsets, entries):
        launches['fill'] += 1
        assert offsets.shape == (sources.numel() * bands,)
        for s, u in enumerate(sources.tolist()):
            for j in range(bands):
                v, o = rng.permutation(partners(u, j)), int(offsets[s * bands + j])  # (in no particular order)
                entries[o:o + len(v)] = torch.from_numpy(s * N + v)

    def exclude_csr(ex, n, device, strict, err):
        if ex is None:
            return None, err
        ex = ex.numpy()
        ex = np.where(ex < 0, ex + n, ex)
        gone = [ex[1][ex[0] == u] for u in range(n)]
        return SimpleNamespace(rowptr=torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in gone])]).astype(np.int64)),
                               col=torch.from_numpy(np.concatenate(gone).astype(np.int32))), err

    monkeypatch.setattr(lsh, '_launch_count', count)
    monkeypatch.setattr(lsh, '_launch_fill', fill)
    monkeypatch.setattr(ssa.candidates, '_exclude_csr', exclude_csr)  # (where the shared walk looks it up)
    index = lsh.LshIndex(1, rows, bands, max_bucket, torch.from_numpy(mh.astype(np.uint32).view(np.int32)), torch.zeros((bands, N), dtype=torch.int64),
                         torch.zeros((bands, N), dtype=torch.int32), torch.zeros((bands,), dtype=torch.int64))
    eh = _eh(P=P)
    eh.strict_bounds = False
    return lsh, eh, index, launches


def _walk_sources(N):
    return np.array(list(range(0, N, N // 15)) + [N - 1, -1, -N, 0, 0, 5 - N], dtype=np.int64)  # about twenty: negative ids, duplicates


def _planted_table():
    """[60, 16] with values in {0, 1, 2}: with rows = 2 nine slices per band, so buckets of several nodes and pairs that meet in several bands"""
    return np.random.RandomState(3).randint(0, 3, size=(60, 16)).astype(np.int64)


# (trailing: rows = 1, so that with the trailing nodes' buckets skipped (max_bucket = 9) a ring node alone still lists more than the
# small budget holds: up to 253 entries against 224; rows = 4 leaves them 4 at the most)
@pytest.mark.parametrize('name,rows,bands,max_bucket', [('trailing', 1, 128, 9), ('trailing', 1, 128, 10), ('planted', 2, 8, 1024)])
def test_the_host_walk_rehearsed_with_stand_ins(monkeypatch, regenerated_tables, name, rows, bands, max_bucket):
    if name == 'trailing':
        N, ei, m = restated.trailing_graph()
        mh = _oracle_tables(regenerated_tables, N, ei, 128)[1]
    else:
        mh = _planted_table()
        N = mh.shape[0]
    lsh, eh, index, launches = _rehearse(monkeypatch, mh, rows, bands, max_bucket)
    src = _walk_sources(N)
    S = len(src)
    shared = restated.shared_bands(mh, src, rows, bands, max_bucket).astype(np.int64)
    shared[np.arange(S), np.where(src < 0, src + N, src)] = 0
    entries = shared.sum(axis=1)  # what each source lists before the pairs are made unique
    if name == 'planted':
        assert (np.bincount(shared.reshape(-1)) > 0).sum() >= 4 and entries.min() > 0, 'pairs that meet in 1, 2, 3 ... bands'
    else:
        trailing = entries[np.where(src < 0, src + N, src) >= N - m]
        assert (trailing == ((m - 1) * bands if max_bucket >= m else 0)).all() and len(trailing) >= 3  # ONE bucket per band: kept or skipped
    pair = restated.lsh_candidates(mh, src, rows, bands, max_bucket)
    exclude = np.stack([np.repeat(src, np.diff(pair[0]))[::2], pair[1][::2]])  # every other listed pair ...
    exclude = np.concatenate([exclude, exclude[:, :3], np.array([[0, -1, 5], [0, 3, 5 - N]])], axis=1)  # ... a repeated pair, a self loop, a negative id
    for kw in (dict(), dict(min_bands=2), dict(exclude=exclude)):
        want = restated.lsh_candidates(mh, src, rows, bands, max_bucket, **kw)
        assert want[1].size, 'a trivial case checks nothing'
        tkw = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
        whole = eh.lsh_candidates(torch.from_numpy(src), index, **tkw)
        _assert_same([t.numpy() for t in whole], want)
        # a few hundred bytes: a block boundary falls inside the source list, and one source alone exceeds the entry budget
        small = 12 * bands * 7
        monkeypatch.setattr(lsh, '_LSH_BLOCK_BYTES', small)
        assert S > 7 and entries.max() > small // lsh._LSH_ENTRY_BYTES
        before = launches['count']
        split = eh.lsh_candidates(torch.from_numpy(src), index, **tkw)
        assert all(torch.equal(a, b) for a, b in zip(split, whole))
        assert launches['count'] - before == -(-S // 7)
        monkeypatch.setattr(lsh, '_LSH_BLOCK_BYTES', 1 << 30)
    none = eh.lsh_candidates(torch.from_numpy(src[:0]), index)
    assert none[0].tolist() == [0] and none[1].shape == (0,) and none[1].dtype == torch.int64 and none[2].dtype == torch.int32
    # one source outside [-N, N) (a device caller's: CPU ids are refused by the argument check): its row is empty, the others are as before
    from subgraph_sketching_amd.candidates import _rows
    bad = np.concatenate([src[:4], [N + 3], src[4:]])
    with pytest.raises(IndexError):
        eh.lsh_candidates(torch.from_numpy(bad), index)
    rowptr, ids, n_bands = _rows(torch.device('cpu'), S + 1, N, lsh._walk(eh, 'lsh_candidates', torch.from_numpy(bad), None, index, 1))
    want = restated.lsh_candidates(mh, src, rows, bands, max_bucket)
    np.testing.assert_array_equal(rowptr.numpy(), np.concatenate([want[0][:5], want[0][4:]]))
    _assert_same((ids.numpy(), n_bands.numpy()), want[1:])


def test_the_entry_points_are_declared_bound_and_exported():
    import subgraph_sketching_amd as ssa
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'subgraph_sketch.h')).read(), flags=re.S)
    assert os.path.exists(ssa._native.LIB_PATH), 'run `python __graft_entry__.py` first (build())'
    handle = ctypes.CDLL(ssa._native.LIB_PATH)
    for name, n_args in (('ss_lsh_band_keys', 8), ('ss_lsh_count', 14), ('ss_lsh_fill', 14)):
        assert re.search(r'\bint\s+%s\s*\(' % name, text)
        restype, argtypes = ssa._native.SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == n_args and hasattr(handle, name)
    for name in ('build_lsh_index', 'lsh_candidates', 'topk_links_lsh'):
        assert callable(getattr(ssa.ElphHashes, name))
    assert handle.ss_version() == 129


def test_argument_errors_of_the_library_are_reported_without_a_gpu():
    from ctypes import c_void_p
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(8)  # never dereferenced
    assert lib.ss_lsh_band_keys(fake, 30, 128, 4, 33, 64, fake, None) == -1       # rows * bands > P
    assert lib.ss_lsh_band_keys(fake, 30, 130, 4, 32, 64, fake, None) == -4       # P not a multiple of 4
    assert lib.ss_lsh_band_keys(fake, 1 << 31, 128, 4, 32, 64, fake, None) == -1  # the permutation is int32
    assert lib.ss_lsh_band_keys(fake, 30, 128, 4, 32, 65, fake, None) == -1
    assert lib.ss_lsh_band_keys(None, 30, 128, 4, 32, 64, fake, None) == -1
    assert lib.ss_lsh_band_keys(None, 0, 128, 4, 32, 64, None, None) == 0         # no nodes: nothing to do
    assert lib.ss_lsh_count(fake, 2, 30, fake, 128, 4, 32, 64, fake, fake, 0, fake, None, None) == -1     # max_bucket < 1
    assert lib.ss_lsh_count(fake, 2, 30, fake, 128, 4, 32, 64, fake, fake, 8, None, None, None) == -1     # no counts
    assert lib.ss_lsh_count(None, 0, 30, None, 128, 4, 32, 64, None, None, 8, None, None, None) == 0      # no sources
    assert lib.ss_lsh_fill(fake, 2, 30, fake, 128, 4, 32, 64, fake, fake, 8, None, fake, None) == -1      # no offsets
    assert lib.ss_lsh_fill(fake, -1, 30, fake, 128, 4, 32, 64, fake, fake, 8, fake, fake, None) == -1


# ---- planted tables (lsh_planted.py): the generator and expected() pinned on the restatement for every small case of --------------
# ---- test_lsh_planted_gpu.py, and the non-triviality conditions those tests assert -------------------------------------------------

def _pin(N, P, rows, bands, groups, sources, caps=(1024,), trivial_ok=False, near=()):
    """expected() == the restatement on the generated table for every max_bucket of `caps`, with exclude and min_bands on the first;
    background rows have no partner; the noise words change nothing.  -> the table"""
    b = planted.resolve_bands(P, rows, bands)
    table = planted.planted_table(N, P, rows, bands, groups, seed=N + P, near=near)
    assert table.shape == (N, P) and table.dtype == np.int64 and table.min() >= 0 and table.max() < (1 << 32)
    members = set(v for m, J in groups if J for v in m)
    for j, (group, sizes) in enumerate(restated.band_groups(table, rows, b)):
        in_band = set(v for m, J in groups if j in J for v in m)
        assert all(sizes[group[v]] == 1 for v in range(N) if v not in in_band), 'a background row has a partner'
    everyone = np.arange(N, dtype=np.int64)
    alone = restated.lsh_candidates(table, everyone, rows, b)
    assert all(alone[0][v] == alone[0][v + 1] for v in range(N) if v not in members)
    for i, cap in enumerate(caps):
        want, skipped = planted.expected(N, rows, b, groups, sources, cap)
        _assert_same(want, restated.lsh_candidates(table, sources, rows, b, max_bucket=cap))
        np.testing.assert_array_equal(skipped, restated.skipped_buckets(table, rows, b, max_bucket=cap))
        if i == 0 and not trivial_ok:
            assert planted.nontrivial(want[0], N), 'a trivial expectation checks nothing'
    if P > rows * b:
        other = planted.planted_table(N, P, rows, bands, groups, seed=N + P, noise_seed=977, near=near)
        assert np.array_equal(other[:, :rows * b], table[:, :rows * b]) and (other[:, rows * b:] != table[:, rows * b:]).mean() > 0.9
        _assert_same(restated.lsh_candidates(other, sources, rows, b), restated.lsh_candidates(table, sources, rows, b))
        np.testing.assert_array_equal(planted.band_keys(other, rows, b), planted.band_keys(table, rows, b))
    k = min(6, len(sources), len(alone[1]))  # pairs that exist among them, by positive and by negative id
    exclude = np.stack([np.tile(sources[:k], 2), np.concatenate([alone[1][:k], alone[1][:k] - N])])
    _assert_same(planted.expected(N, rows, b, groups, sources, caps[0], exclude=exclude)[0],
                 restated.lsh_candidates(table, sources, rows, b, max_bucket=caps[0], exclude=exclude))
    _assert_same(planted.expected(N, rows, b, groups, sources, caps[0], min_bands=2)[0],
                 restated.lsh_candidates(table, sources, rows, b, max_bucket=caps[0], min_bands=2))
    twin = planted.planted_table_torch(N, P, rows, bands, groups, seed=N + P, device='cpu', block=7, near=near)
    assert twin.dtype == torch.int64 and np.array_equal(twin.numpy(), table)
    packed = planted.planted_table_torch(N, P, rows, bands, groups, seed=N + P, device='cpu', dtype=torch.int32, near=near)
    assert np.array_equal(packed.numpy().view(np.uint32).astype(np.int64), table)
    return table


@pytest.mark.parametrize('P,rows,bands', planted.TILE_CASES)
def test_planted_tile_cases(P, rows, bands):
    T = planted.tile_rows(P)
    assert T == min(64, 8192 // P) and planted.tile_sizes(P) == [T, T + 1, 2 * T - 1, 3 * T + 5]
    for N in planted.tile_sizes(P):
        groups, sources = planted.tile_plan(P, rows, bands, N)
        members = set(v for m, _ in groups for v in m)
        assert {0, N - 1} <= members and all({k - 1, k} <= members for k in range(T, N, T))
        assert {0, N - 1} <= set(int(u) % N for u in sources)
        _pin(N, P, rows, bands, groups, sources)


def test_planted_one_and_two_node_tables():
    _pin(1, 12, 1, 5, [], np.array([0, -1, 0], dtype=np.int64), trivial_ok=True)
    want, _ = planted.expected(2, 4, 32, [([1, 0], [0, 31])], np.array([0, 1, -1], dtype=np.int64), 1024)
    assert want[1].tolist() == [1, 0, 0] and want[2].tolist() == [2, 2, 2]
    _pin(2, 128, 4, None, [([1, 0], [0, 31])], np.array([0, 1, -1], dtype=np.int64), trivial_ok=True)


def test_planted_round_case():
    N, P, rows = planted.ROUND_N, planted.ROUND_P, planted.ROUND_ROWS
    groups, by_size = planted.round_plan()
    sources = planted.round_sources(groups)
    caps = [1024] + [c for m in planted.ROUND_SIZES for c in (m, m - 1)]
    near = planted.round_near(groups)
    table = _pin(N, P, rows, None, groups, sources, caps=caps, near=near)
    one_bit = planted.band_keys(table, rows, None, 1)
    for w in (rows - 1, 0, 1):  # a near miss of every kind meets its leader in one range of a one-bit key: only the slices tell them apart
        assert any(one_bit[j][v] == one_bit[j][leader] for v, leader, j, miss in near if miss == w)
    for v, leader, j, w in near:
        differ = np.nonzero(table[v, j * rows:(j + 1) * rows] != table[leader, j * rows:(j + 1) * rows])[0]
        assert differ.tolist() == [w]
    assert set(planted.ROUND_SIZES) <= planted.bucket_sizes(N, 32, groups, sources)
    want = planted.expected(N, rows, 32, groups, sources, 1024)[0]
    assert set(want[2].tolist()) >= {1, 3, 4, 5, 32}
    for m, (members, band) in by_size.items():   # max_bucket = m lists the group, m - 1 skips it
        row = lambda cap: np.diff(planted.expected(N, rows, 32, groups, members[:1], cap)[0][0])[0]
        assert row(m) == m - 1 and row(m - 1) == 0
        skipped = lambda cap: planted.expected(N, rows, 32, groups, sources, cap)[1][band] - (3 > cap)  # (the group of three is in every band)
        assert skipped(m - 1) == 1 and skipped(m) == 0
    # the six-bit key: a planted group that fits max_bucket is dropped because its key range does not, another is listed through a
    # range with false matches; both sit inside their band's order with more than max_bucket + 1 entries from their range's start on
    cap = planted.SIX_BIT_MAX_BUCKET
    keys = planted.band_keys(table, rows, None, 6)
    runs = planted.key_run_lengths(keys)
    assert keys.min() >= 0 and keys.max() < 64
    dropped = listed = False
    for m, (members, band) in by_size.items():
        u = members[0]
        inside = (keys[band] < keys[band][u]).sum() > 0 and (keys[band] >= keys[band][u]).sum() > cap + 1
        dropped |= bool(m <= cap < runs[band][u] and inside)
        listed |= bool(m < runs[band][u] <= cap and inside)
    assert dropped and listed
    six = planted.six_bit_sources(groups)
    got, skipped = planted.candidates_under_keys(table, six, rows, None, cap, 6)
    full = restated.lsh_candidates(table, six, rows, None, max_bucket=cap)
    assert planted.nontrivial(got[0], N) and 0 < got[1].size < full[1].size and skipped.sum() > 0
    pairs = lambda r: set(zip(np.repeat(np.arange(len(six)), np.diff(r[0])).tolist(), r[1].tolist(), r[2].tolist()))
    assert set((s, v) for s, v, _ in pairs(got)) <= set((s, v) for s, v, _ in pairs(full))
    # with all 64 bits the key ranges are the buckets, and the short-key restatement is the restatement
    _assert_same(planted.candidates_under_keys(table, sources, rows, None, 1024, 64)[0], restated.lsh_candidates(table, sources, rows))


@pytest.mark.parametrize('b', planted.WAVE_BANDS)
def test_planted_wave_case(b):
    N, P, rows = planted.WAVE_N, planted.WAVE_P, planted.WAVE_ROWS
    groups, good = planted.wave_plan(b)
    assert len(good) >= 17 and len(set(good)) == len(good)
    _pin(N, P, rows, b, groups, np.array(good, dtype=np.int64))
    for S in (1, 2, 3, 17):
        want = planted.expected(N, rows, b, groups, good[:S], 1024)[0]
        assert planted.nontrivial(want[0], N)
    assert [S * b % 16 for S in (1, 2, 3, 17) for b in planted.WAVE_BANDS].count(0) == 0


def test_planted_large_plan_and_the_band_key():
    groups, sources = planted.large_plan()
    N, b = planted.LARGE_N, planted.LARGE_BANDS
    planted.check_plan(N, b, groups)
    assert N * planted.LARGE_P * 4 > (1 << 32) and len(groups) == 12
    for bound in planted.LARGE_BOUNDS:
        assert any(min(m) < bound <= max(m) for m, _ in groups) and {bound - 1, bound} <= set(sources.tolist())
    assert any(N - 1 in m for m, _ in groups)
    want, skipped = planted.expected(N, planted.LARGE_ROWS, b, groups, sources, 1024)
    assert planted.nontrivial(want[0], N) and skipped.sum() == 0 and {17, 33} <= planted.bucket_sizes(N, b, groups, sources)
    # band_key: r = 1 is one round of the splitmix64 finaliser from the state r ^ x, plus the golden ratio; wrapping in 64 bits
    def h(x):
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 & planted.M64
        x ^= x >> 27
        x = x * 0x94D049BB133111EB & planted.M64
        return x ^ (x >> 31)
    t = np.array([[0, 1, (1 << 32) - 1, 12345], [7, 7, 7, 7]], dtype=np.int64)
    for rows, bands in ((1, 4), (2, 2), (4, 1), (3, 1)):
        for bits in (64, 6, 1):
            keys = planted.band_keys(t, rows, bands, bits).view(np.uint64)
            for j in range(bands):
                for v in range(2):
                    k = rows
                    for x in t[v, j * rows:(j + 1) * rows].tolist():
                        k = (h(k ^ x) + planted.GOLDEN) & planted.M64
                    assert int(keys[j, v]) == k & ((1 << bits) - 1)
