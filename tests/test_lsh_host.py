"""The LSH index (ElphHashes.build_lsh_index / lsh_candidates / topk_links_lsh) without a GPU: the numpy restatement of
its semantics (lsh_restatement.py) against a naive double loop written here, on oracle tables; the argument checks that run before a
device is touched; the ranking key's torch form; the new entry points in the header, the bindings and the library."""
from argparse import Namespace
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, oracle_params
from score_restatement import raw_head
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
