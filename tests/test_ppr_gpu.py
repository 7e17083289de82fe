"""heuristics.PPR / personalized_pagerank on the GPU against the fp64 restatement of pagerank_power (tests/ppr_restatement.py):
vectors, iteration counts, float32 scores, the reference's return convention, bit-identity across batch widths and source order,
hub rows, collab size, and the error paths."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from ppr_restatement import pagerank_power

pytestmark = pytest.mark.gpu


def _small_graph(seed, n=60, e=300):
    """directed multigraph, int weights, duplicate entries, dangling rows, node n - 1 isolated"""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n - 1, size=e)
    dst = rng.randint(0, n - 1, size=e)
    keep = ~np.isin(src, rng.choice(n - 1, size=5, replace=False))
    src, dst = src[keep], dst[keep]
    src, dst = np.concatenate([src, src[:20]]), np.concatenate([dst, dst[:20]])
    return sp.csr_matrix((rng.randint(1, 5, size=len(src)), (src, dst)), shape=(n, n))


def _power_law_graph(n=50000, e=600000, seed=3):
    """in-degrees skewed so that the first nodes hold thousands of in-edges (rows of A^T cut into many segments)"""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, size=e)
    dst = np.minimum((n * rng.random_sample(e) ** 4).astype(np.int64), n - 1)
    return sp.csr_matrix((rng.randint(1, 4, size=e), (src, dst)), shape=(n, n))


def _uniform_graph(n=235868, e=2400000, seed=4):
    rng = np.random.RandomState(seed)
    return sp.csr_matrix((np.ones(e, dtype=np.int64), (rng.randint(0, n, size=e), rng.randint(0, n, size=e))), shape=(n, n))


def _check_against_restatement(A, sources, p, tol=1e-7, max_iter=100):
    from subgraph_sketching_amd.heuristics import personalized_pagerank
    vec, iters = personalized_pagerank(A, torch.tensor(sources), p=p, tol=tol, max_iter=max_iter)
    assert vec.dtype == torch.float64 and vec.device.type == 'cpu' and vec.shape == (len(sources), A.shape[0])
    ref, ref_iters, res = pagerank_power(A, sources, p=p, tol=tol, max_iter=max_iter)
    vec, iters = vec.numpy(), iters.numpy()
    for j in range(len(sources)):
        if iters[j] != ref_iters[j]:
            # the stop rule compares a residual whose last bits depend on the summation order: a count may differ by one only
            # where the restatement's residual at the earlier of the two steps lies within 1e-6 relative of tol
            k = min(iters[j], ref_iters[j])
            assert abs(int(iters[j]) - int(ref_iters[j])) == 1 and abs(res[j][k] - tol) <= 1e-6 * tol, (j, iters[j], ref_iters[j])
            ref[j] = pagerank_power(A, [sources[j]], p=p, tol=0.0, max_iter=int(iters[j]))[0][0]
        np.testing.assert_allclose(vec[j], ref[j], rtol=1e-10, atol=1e-300)
    return vec, iters, ref_iters


@pytest.mark.parametrize('p', [0.5, 0.85])
@pytest.mark.parametrize('seed', [0, 1])
def test_vectors_and_iterations_match_the_restatement(p, seed):
    A = _small_graph(seed)
    n = A.shape[0]
    dangling = int(np.nonzero(np.diff(A.indptr) == 0)[0][0])
    sources = list(range(0, n - 1, 3)) + [dangling, n - 1]
    vec, iters, _ = _check_against_restatement(A, sources, p)
    assert iters[-1] == 1 and iters[-2] == 1  # isolated / dangling source: one step, exactly e_src
    np.testing.assert_array_equal(vec[-1], np.eye(n)[n - 1])


def test_max_iter_path():
    A = _small_graph(2)
    _, iters, ref_iters = _check_against_restatement(A, [0, 1, 7, A.shape[0] - 1], 0.85, tol=0.0, max_iter=25)
    assert list(iters) == [25, 25, 25, 1]


def test_scores_and_return_convention():
    from subgraph_sketching_amd.heuristics import PPR
    A = _small_graph(5)
    n = A.shape[0]
    rng = np.random.RandomState(9)
    ei = torch.from_numpy(rng.randint(0, n, size=(400, 2)))  # many ties in the source column
    scores, edge_reindex = PPR(A, ei)
    src_index, sort_indices = torch.sort(ei[:, 0])
    assert torch.equal(edge_reindex, torch.stack([src_index, ei[sort_indices, 1]]))
    assert scores.dtype == torch.float32 and scores.device.type == 'cpu' and scores.shape == (400,)
    sources = torch.unique(ei[:, 0]).tolist()
    ref, _, _ = pagerank_power(A, sources, p=0.85, tol=1e-7)
    row = {s: j for j, s in enumerate(sources)}
    expect = np.array([ref[row[int(s)], int(d)] for s, d in edge_reindex.T], dtype=np.float32)
    np.testing.assert_allclose(scores.numpy(), expect, rtol=1e-6, atol=1e-30)


def test_bit_identical_across_batch_width_and_source_order():
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd.heuristics import PPR, personalized_pagerank
    A = _power_law_graph(n=6000, e=80000)
    sources = torch.arange(0, 6000, 37)
    perm = torch.from_numpy(np.random.RandomState(1).permutation(len(sources)))
    ei = torch.stack([sources.repeat(3), torch.arange(3 * len(sources)) % 6000], 1)
    saved = ssa.knobs.PPR_COLUMNS
    try:
        runs = []
        for S in (1, 7, 64, len(sources), 64):
            ssa.knobs.PPR_COLUMNS = S
            vec, iters = personalized_pagerank(A, sources)
            vperm, iperm = personalized_pagerank(A, sources[perm])
            assert torch.equal(vperm, vec[perm]) and torch.equal(iperm, iters[perm])
            runs.append((vec, iters, PPR(A, ei)[0]))
    finally:
        ssa.knobs.PPR_COLUMNS = saved
    for vec, iters, scores in runs[1:]:
        assert torch.equal(vec, runs[0][0]) and torch.equal(iters, runs[0][1]) and torch.equal(scores, runs[0][2])


def test_power_law_hubs_match_the_restatement():
    A = _power_law_graph()
    indeg = np.bincount(A.indices, minlength=A.shape[0])
    assert indeg.max() > 3000 and (indeg > 256).sum() > 10  # rows of A^T that are cut into segments
    rng = np.random.RandomState(7)
    sources = [int(i) for i in np.argsort(-indeg)[:8]] + [int(i) for i in rng.choice(A.shape[0], 56, replace=False)]
    _check_against_restatement(A, sources, 0.85)


def test_collab_size_uniform_graph_matches_the_restatement():
    A = _uniform_graph()
    sources = [int(i) for i in np.random.RandomState(8).choice(A.shape[0], 32, replace=False)]
    _, iters, _ = _check_against_restatement(A, sources, 0.85)
    assert 20 < iters.min() and iters.max() < 100


def test_errors_empty_and_devices():
    from subgraph_sketching_amd.heuristics import PPR, personalized_pagerank
    A = _small_graph(3)
    n = A.shape[0]
    with pytest.raises(IndexError):
        PPR(A, torch.tensor([[0, 1], [n, 2]]))
    with pytest.raises(IndexError):
        PPR(A, torch.tensor([[0, 1], [2, -1]]))
    with pytest.raises(IndexError):
        personalized_pagerank(A, torch.tensor([0, n]))
    with pytest.raises(ValueError):
        PPR(A, torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError):
        PPR(A, torch.tensor([[0, 1, 2]]))
    scores, er = PPR(A, torch.zeros((0, 2), dtype=torch.int64))
    assert scores.shape == (0,) and er.shape == (2, 0)
    ei = torch.tensor([[3, 1], [0, 2], [3, 3], [1, 0]])
    cpu_scores, cpu_er = PPR(A, ei)
    gpu_scores, gpu_er = PPR(A, ei.cuda())
    assert cpu_scores.device.type == 'cpu' and cpu_er.device.type == 'cpu'
    assert gpu_scores.is_cuda and gpu_er.is_cuda
    # each device sorts with its own (unstable) torch.sort, as the reference would: ties may come in another order
    g_src, g_idx = torch.sort(ei.cuda()[:, 0])
    assert torch.equal(gpu_er, torch.stack([g_src, ei.cuda()[g_idx, 1]]))
    by_link = {tuple(l): float(x) for l, x in zip(cpu_er.T.tolist(), cpu_scores)}
    assert {tuple(l): float(x) for l, x in zip(gpu_er.T.tolist(), gpu_scores.cpu())} == by_link
    # the operator is cached on the adjacency; a DeviceAdjacency is accepted as well
    from subgraph_sketching_amd.heuristics import DeviceAdjacency
    adj = DeviceAdjacency(A.tocoo(), torch.device('cuda:0'))
    assert torch.equal(PPR(adj, ei)[0], cpu_scores)
    # CN / AA / RA on an adjacency that has run PPR give what they give on a fresh one
    from subgraph_sketching_amd.heuristics import AA, CN, RA
    fresh = DeviceAdjacency(A.tocoo(), torch.device('cuda:0'))
    for fn in (CN, AA, RA):
        assert torch.equal(fn(adj, ei)[0], fn(fresh, ei)[0])


# ---------------------------------------------------------------------------------------------------------------------------
# inputs at the edges: matrix dtypes, damping, tolerance, step limits, degenerate graphs, the check interval
# ---------------------------------------------------------------------------------------------------------------------------
def _weighted(dtype, seed=5):
    """_small_graph's pattern with float32 / float64 weights (duplicates summed in that dtype) or as a bool matrix"""
    A = _small_graph(seed).tocoo()
    rng = np.random.RandomState(seed + 100)
    if dtype == 'bool':
        return sp.csr_matrix((np.ones(A.nnz, dtype=bool), (A.row, A.col)), shape=A.shape)
    return sp.csr_matrix((rng.uniform(0.05, 3.0, size=A.nnz).astype(dtype), (A.row, A.col)), shape=A.shape)


def _dangling_and_isolated(A):
    deg = np.diff(A.indptr)
    return [int(np.nonzero(deg == 0)[0][0]), A.shape[0] - 1]


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'bool'])
def test_matrix_dtypes_match_the_restatement(dtype):
    A = _weighted(dtype)
    assert A.dtype == np.dtype(dtype)
    for p in (0.5, 0.85):
        _check_against_restatement(A, [0, 3, 17] + _dangling_and_isolated(A), p)


@pytest.mark.parametrize('p', [0.0, 0.15, 0.99])
@pytest.mark.parametrize('tol', [0.0, 1e-12, 1e-3])
def test_damping_and_tolerance_edges(p, tol):
    """tol = 0 stops only on a residual of exactly 0, i.e. once the iterate reaches its fixed point to the last bit -- a step
    that depends on rounding, not on the method (p = 0 gets there after one step); 12 steps stay well above that floor"""
    A = _weighted('float64', seed=6)
    _, iters, _ = _check_against_restatement(A, [1, 2, 40] + _dangling_and_isolated(A), p, tol=tol, max_iter=12 if tol == 0 else 40)
    if tol == 0 and p > 0:
        assert (iters[:3] == 12).all()


@pytest.mark.parametrize('max_iter', [0, 1, 2])
def test_step_limits(max_iter):
    A = _small_graph(7)
    _, iters, ref_iters = _check_against_restatement(A, [0, 5, 9] + _dangling_and_isolated(A), 0.85, max_iter=max_iter)
    assert np.array_equal(iters, ref_iters)
    assert (iters[:3] == max(max_iter, 1)).all()  # the reference steps once before it checks max_iter
    assert (iters[3:] == 1).all()  # a dangling or isolated source is its own fixed point: the second residual is 0


def test_duplicate_sources_and_self_loops():
    A = _small_graph(8).tolil()
    for u in (3, 5, 11):
        A[u, u] = 2
    A = A.tocsr()
    assert A.diagonal()[[3, 5, 11]].all()
    vec, _, _ = _check_against_restatement(A, [3, 3, 5, 3, 11, 5], 0.85)
    assert np.array_equal(vec[0], vec[1]) and np.array_equal(vec[0], vec[3]) and np.array_equal(vec[2], vec[5])
    from subgraph_sketching_amd.heuristics import PPR
    links = torch.tensor([[3, 3], [3, 5], [5, 5], [3, 11], [3, 3]])
    scores, back = PPR(A, links)
    src = back[0].numpy()
    assert scores.numpy()[src == 3].size == 4 and len(set(scores.numpy()[(src == 3) & (back[1].numpy() == 3)].tolist())) == 1


@pytest.mark.parametrize('n,edges', [(1, []), (1, [(0, 0)]), (2, []), (2, [(0, 1)]), (2, [(0, 1), (1, 0), (1, 1)])])
def test_one_and_two_node_graphs(n, edges):
    e = np.array(edges, dtype=np.int64).reshape(-1, 2)
    A = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    sources = [0] if n == 1 else [0, 1, 0]
    vec, _, _ = _check_against_restatement(A, sources, 0.85)
    assert np.allclose(vec.sum(axis=1), 1.0, rtol=1e-12)
    from subgraph_sketching_amd.heuristics import PPR
    links = torch.tensor([[0, 0]] if n == 1 else [[1, 0], [0, 1], [0, 0]])
    scores, back = PPR(A, links)
    for (u, v), s in zip(back.T.tolist(), scores.tolist()):
        assert s == np.float32(vec[sources.index(u), v])


@pytest.mark.parametrize('every', [1, 3, 1000])
def test_check_interval_does_not_change_results(every, monkeypatch):
    """knobs.PPR_CHECK_EVERY only says how often the host asks whether any column is still running"""
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd.heuristics import personalized_pagerank
    A = _small_graph(9)
    sources = torch.tensor([0, 4, 8, 15, 23] + _dangling_and_isolated(A))
    for p, tol, max_iter in ((0.85, 1e-7, 100), (0.99, 1e-12, 37), (0.5, 0.0, 5)):
        base = personalized_pagerank(A, sources, p=p, tol=tol, max_iter=max_iter)
        monkeypatch.setattr(ssa.knobs, 'PPR_CHECK_EVERY', every)
        got = personalized_pagerank(A, sources, p=p, tol=tol, max_iter=max_iter)
        monkeypatch.undo()
        assert torch.equal(got[1], base[1]), (p, tol, max_iter)
        assert torch.equal(got[0].view(torch.int64), base[0].view(torch.int64)), (p, tol, max_iter)
        _check_against_restatement(A, sources.tolist(), p, tol=tol, max_iter=max_iter)
