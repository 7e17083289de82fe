"""PPR without a GPU: the fp64 restatement of pagerank_power (tests/ppr_restatement.py) against a direct solve, and the host-side
plan of heuristics.PPR (the reference's sorted link order, runs of equal sources, source -> (batch, column))."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from ppr_restatement import pagerank_power, ppr_solve


def _multigraph(seed, n=40, e=160):
    """directed, int-weighted, with duplicate entries, dangling rows (no out-edges) and node n-1 isolated"""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n - 1, size=e)
    dst = rng.randint(0, n - 1, size=e)
    dangling = rng.choice(n - 1, size=4, replace=False)
    keep = ~np.isin(src, dangling)
    src, dst = src[keep], dst[keep]
    src = np.concatenate([src, src[:10]])  # duplicates: csr_matrix((w, (src, dst))) keeps them until it sums them
    dst = np.concatenate([dst, dst[:10]])
    w = rng.randint(1, 4, size=len(src))
    return sp.csr_matrix((w, (src, dst)), shape=(n, n)), dangling


@pytest.mark.parametrize('p', [0.5, 0.85])
@pytest.mark.parametrize('seed', [0, 1])
def test_restatement_converges_to_the_direct_solve(p, seed):
    A, dangling = _multigraph(seed)
    n = A.shape[0]
    busy = np.argsort(-np.diff(A.indptr), kind='stable')
    sources = [int(busy[0]), int(busy[1]), int(dangling[0]), n - 1]
    vec, iters, res = pagerank_power(A, sources, p=p, tol=1e-7)
    for j, s in enumerate(sources):
        # stopped at a step of 1e-7 on the unnormalised scale n: at most ~tol / ((1 - p) n) from the fixed point
        np.testing.assert_allclose(vec[j], ppr_solve(A, s, p), rtol=0, atol=5e-7 / ((1 - p) * n))
        assert res[j][-1] <= 1e-7 and all(r > 1e-7 for r in res[j][:-1])  # stopped on tol, not max_iter
        assert len(res[j]) == iters[j] + 1
    assert iters[2] == iters[3] == 1  # dangling / isolated source: the first step reproduces x0
    np.testing.assert_array_equal(vec[3], np.eye(n)[n - 1])
    assert 10 < iters[0] < 100 and 10 < iters[1] < 100


def test_restatement_max_iter_path():
    A, dangling = _multigraph(2)
    n = A.shape[0]
    a = int(np.argmax(np.diff(A.indptr)))
    vec, iters, _ = pagerank_power(A, [a, n - 1], p=0.85, tol=0.0, max_iter=30)
    assert list(iters) == [30, 1]
    vec, iters, res = pagerank_power(A, [a], p=0.85, tol=0.0, max_iter=100)
    assert iters[0] <= 100 and (iters[0] == 100 or res[0][-1] == 0.0)  # tol = 0 ends on max_iter or on an exact fixed point
    np.testing.assert_allclose(vec[0], ppr_solve(A, a, 0.85), rtol=0, atol=1e-12)


def test_dangling_mass_returns_to_the_source():
    """a source whose only out-edge leads to a dangling node: the dangling node's mass goes back to the source"""
    A = sp.csr_matrix((np.ones(2), ([0, 2], [1, 3])), shape=(4, 4))
    vec, _, _ = pagerank_power(A, [0], p=0.85, tol=1e-12)
    # x1 = 0.85 x0 and x0 = 0.15 x0 + x1 (z_0 = 0.15 / n, dangling z_1 = 1 / n): x1 / x0 = 0.85
    np.testing.assert_allclose(vec[0], np.array([1, 0.85, 0, 0]) / 1.85, atol=1e-12)
    np.testing.assert_allclose(vec[0], ppr_solve(A, 0, 0.85), atol=1e-12)


def test_plan_follows_the_reference_sort_with_ties():
    from subgraph_sketching_amd.heuristics import ppr_plan
    ei = torch.tensor([[5, 1], [2, 7], [5, 3], [0, 0], [2, 2], [9, 4], [5, 5], [0, 8], [7, 7], [2, 6]])
    plan = ppr_plan(ei, 2)
    src_index, sort_indices = torch.sort(ei[:, 0])
    assert torch.equal(plan.edge_reindex, torch.stack([src_index, ei[sort_indices, 1]]))
    assert plan.edge_reindex.shape == (2, 10)
    assert plan.sources.tolist() == [0, 2, 5, 7, 9]
    # runs: 0 x2, 2 x3, 5 x3, 7 x1, 9 x1 -> columns 0 1 | 0 1 | 0
    assert plan.link_col.tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 1, 0]
    assert plan.link_col.dtype == torch.int32
    assert plan.batches == [(0, 2, 0, 5), (2, 2, 5, 4), (4, 1, 9, 1)]
    for lo, cnt, first, count in plan.batches:  # every link of a batch has its source in that batch, at its column
        srcs = plan.edge_reindex[0, first:first + count]
        col = plan.link_col[first:first + count].long()
        assert torch.equal(plan.sources[lo + col], srcs) and int(col.max()) < cnt


def test_plan_of_one_batch_and_of_nothing():
    from subgraph_sketching_amd.heuristics import ppr_plan
    ei = torch.tensor([[3, 1], [3, 2], [1, 0]])
    plan = ppr_plan(ei, 64)
    assert plan.batches == [(0, 2, 0, 3)] and plan.link_col.tolist() == [0, 1, 1]
    empty = ppr_plan(torch.zeros((0, 2), dtype=torch.int64), 64)
    assert empty.edge_reindex.shape == (2, 0) and empty.batches == [] and len(empty.link_col) == 0
    with pytest.raises(ValueError):
        ppr_plan(torch.zeros(5, dtype=torch.int64), 64)
    with pytest.raises(ValueError):
        ppr_plan(torch.zeros((5, 3), dtype=torch.int64), 64)


def _fresh_matrix():
    # canonical already, as the reference runner builds it: tocsr() hands back this very object
    return sp.csr_matrix((np.array([1, 2, 1, 3, 1]), (np.array([0, 1, 2, 3, 4]), np.array([1, 2, 3, 4, 0]))), shape=(5, 5))


def test_adjacency_cache_entry_dies_with_the_matrix():
    """the cached adjacency (and any PageRank operator on it) must not keep the caller's matrix alive"""
    import gc
    from subgraph_sketching_amd import heuristics
    A = _fresh_matrix()
    assert A.has_canonical_format
    key = (id(A), 'cpu')
    adj = heuristics._adjacency(A, torch.device('cpu'))
    assert heuristics._ADJ_CACHE[key][1] is adj
    adj.ppr_operator(0.85)
    del A, adj
    gc.collect()
    assert key not in heuristics._ADJ_CACHE


@pytest.mark.parametrize('dtype', [np.int64, np.float32, np.float64])
def test_ppr_operator_is_the_restated_operator_and_leaves_the_adjacency_alone(dtype):
    """the operator built from the device CSR equals W and z of the restatement bit for bit, in the matrix's own dtype, and
    the arrays CN / AA / RA read are unchanged by building it"""
    from subgraph_sketching_amd.heuristics import DeviceAdjacency
    from ppr_restatement import operator
    rng = np.random.RandomState(4)
    n, e = 2000, 20000
    src = rng.randint(0, n, size=e)
    dst = np.minimum((n * rng.random_sample(e) ** 4).astype(np.int64), n - 1)  # the first rows of A^T hold > 256 entries
    A = sp.csr_matrix((rng.randint(1, 4, size=e).astype(dtype), (src, dst)), shape=(n, n))
    adj = DeviceAdjacency(A, torch.device('cpu'))
    before = [t.clone() for t in (adj.rowptr, adj.col, adj.val)], adj.colsum.copy(), adj.multiplier('RA').clone()
    for p in (0.5, 0.85):
        op = adj.ppr_operator(p)
        W, z = operator(A, p)
        M = sp.csr_matrix((op.w.numpy()[:op.nnz], op.col.numpy()[:op.nnz], op.rowptr.numpy()), shape=A.shape)
        assert abs(M - W).max() == 0 and np.array_equal(op.z, z) and np.array_equal(op.zdev.numpy(), z)
        assert op.n_hubs > 0 and op.n_segments > op.n_hubs
        deg = np.diff(op.rowptr.numpy())
        hubs = op.hub_rows.numpy()[:op.n_hubs]
        assert np.array_equal(hubs, np.nonzero(deg > 256)[0])
        assert np.array_equal(np.diff(op.hub_seg.numpy()), (deg[hubs] + 255) // 256)
    assert adj.ppr_operator(0.85) is adj.ppr_operator(0.85)
    for a, b in zip(before[0], (adj.rowptr, adj.col, adj.val)):
        assert torch.equal(a, b)
    assert np.array_equal(before[1], adj.colsum) and torch.equal(before[2], adj.multiplier('RA'))
