"""ElphHashes.topk_candidates without a GPU: the host decode of the scan's ranking keys against a numpy restatement of the kernel's
encoding (csrc/ss_topk.hip topk_key), and the argument checks that run before anything is launched."""
from argparse import Namespace

import numpy as np
import pytest
import torch


def _encode(scores, ids):
    """numpy restatement of topk_key: monotone score bits (-0 folded into +0) as a signed high word, 0xFFFFFFFF - id low"""
    b = np.asarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, 0, b)
    m = np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    hi = m ^ 0x80000000
    return ((hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids, dtype=np.uint64))).view(np.int64)


def _random_scores(rng, n):
    x = np.concatenate([rng.standard_normal(n).astype(np.float32) * 1e3,
                        rng.standard_normal(n).astype(np.float32) * 1e-30,
                        np.array([0.0, -0.0, 1.0, -1.0, 3.4e38, -3.4e38, 1e-45, -1e-45], dtype=np.float32)])
    return np.concatenate([x, x[: n // 2]])  # repeated scores: ties broken by id


def test_decode_round_trip_and_order():
    from subgraph_sketching_amd.engine import TOPK_SENTINEL, _decode_topk_keys
    rng = np.random.RandomState(0)
    scores = _random_scores(rng, 2000)
    ids = rng.permutation(len(scores)).astype(np.int64) * 997 % (1 << 31)
    keys = _encode(scores, ids)
    got_ids, got_scores = _decode_topk_keys(torch.from_numpy(keys))
    assert got_ids.dtype == torch.int64 and got_scores.dtype == torch.float32
    np.testing.assert_array_equal(got_ids.numpy(), ids)
    want = np.where(scores == 0, np.float32(0), scores)  # -0 comes back as +0
    np.testing.assert_array_equal(got_scores.numpy().view(np.int32), want.view(np.int32))
    # signed int64 order of the keys == (score descending, id ascending)
    by_key = np.argsort(keys)[::-1]
    by_contract = np.lexsort((ids, -scores.astype(np.float64)))
    np.testing.assert_array_equal(by_key, by_contract)
    # the sentinel lies below every real key and decodes to padding
    assert keys.min() > TOPK_SENTINEL
    pi, ps = _decode_topk_keys(torch.tensor([TOPK_SENTINEL, int(keys[0])]))
    assert pi.tolist() == [-1, ids[0]] and ps[0].item() == float('-inf')


def test_decode_extremes():
    from subgraph_sketching_amd.engine import _decode_topk_keys
    ids = np.array([0, 1, (1 << 32) - 2, 12345], dtype=np.int64)
    scores = np.array([np.inf, -np.inf, 0.5, -2.5], dtype=np.float32)
    got_ids, got_scores = _decode_topk_keys(torch.from_numpy(_encode(scores, ids)))
    np.testing.assert_array_equal(got_ids.numpy(), ids)
    np.testing.assert_array_equal(got_scores.numpy(), scores)


def _eh(h=2, P=128, p=8):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))


def _table(N=30, P=128, p=8, h=2):
    return {k: {'minhash': torch.zeros((N, P), dtype=torch.int64), 'hll': torch.zeros((N, 1 << p), dtype=torch.int8)}
            for k in range(h + 1)}


@pytest.mark.parametrize('k', [0, -1, 31])
def test_k_out_of_range(k):
    with pytest.raises(ValueError):
        _eh().topk_candidates(torch.tensor([0, 1]), _table(), k)


@pytest.mark.parametrize('hops', [(0, 1), (1, 0), (1, 3), (3, 3), (1,), 'ab'])
def test_hops_out_of_range(hops):
    with pytest.raises(ValueError):
        _eh().topk_candidates(torch.tensor([0, 1]), _table(), 5, hops=hops)


@pytest.mark.parametrize('bad', [[0, 30], [-31], [29, 100]])
def test_cpu_sources_out_of_range(bad):
    with pytest.raises(IndexError):
        _eh().topk_candidates(torch.tensor(bad), _table(), 5)


@pytest.mark.parametrize('bad', [[[0], [30]], [[-31], [1]]])
def test_cpu_exclude_out_of_range(bad):
    with pytest.raises(IndexError):
        _eh().topk_candidates(torch.tensor([0, -30]), _table(), 5, exclude=torch.tensor(bad))


def test_malformed_inputs():
    eh = _eh()
    with pytest.raises(ValueError):
        eh.topk_candidates(torch.tensor([[0, 1]]), _table(), 5)
    with pytest.raises(ValueError):
        eh.topk_candidates(torch.tensor([0.0]), _table(), 5)
    with pytest.raises(ValueError):
        eh.topk_candidates(torch.tensor([0]), _table(), 5, exclude=torch.tensor([0, 1, 2]))


@pytest.mark.parametrize('P', [6, 2052])
def test_unsupported_sketch_shape(P):
    with pytest.raises(NotImplementedError):
        _eh(P=P).topk_candidates(torch.tensor([0]), _table(P=P), 5)
