"""graph_prep without a device: the numpy restatement (tests/graph_prep_restatement.py) against scipy and np.unique, the chunk rule
against float64 and against the plain loop, to_undirected on a hand-written list, the two-grouping composition of the sorted order, the
planted graph's plan, and the argument errors the host module raises before it touches a device."""
import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import graph_prep_planted as planted
import graph_prep_restatement as R


def _random_list(seed, N=40, E=600):
    rng = np.random.RandomState(seed)
    return rng.randint(0, N, E).astype(np.int64), rng.randint(0, N, E).astype(np.int64), N


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_structure_and_integer_sums_against_scipy_and_unique(seed):
    row, col, N = _random_list(seed)
    w = np.random.RandomState(seed + 10).randint(-9, 10, len(row)).astype(np.int64)
    out = R.coalesce(row, col, w, N, 'add')
    A = ssp.coo_matrix((w, (row, col)), shape=(N, N)).tocsr()
    A.sum_duplicates()
    S = ssp.coo_matrix((np.ones_like(w), (row, col)), shape=(N, N)).tocsr()  # (structure and counts: explicit zeros of A stay stored too)
    S.sum_duplicates()
    assert np.array_equal(out['rowptr'], S.indptr) and np.array_equal(out['col'], S.indices) and np.array_equal(out['count'], S.data)
    assert np.array_equal(out['rowptr'], A.indptr) and np.array_equal(out['col'], A.indices) and np.array_equal(out['value'], A.data)
    keys, inverse, counts = np.unique(row * N + col, return_inverse=True, return_counts=True)
    assert np.array_equal(out['row'] * N + out['col'], keys) and np.array_equal(out['count'], counts)
    assert np.array_equal(out['value'], np.bincount(inverse, weights=w).astype(np.int64))
    assert np.array_equal(out['row'], np.repeat(np.arange(N), np.diff(out['rowptr'])))
    assert out['starts'][-1] == len(row) and np.array_equal(np.sort(out['perm']), np.arange(len(row)))


def test_the_two_groupings_compose_the_sorted_order():
    """what graph_prep.sorted_positions does with ss_csr_group_ids + ss_csr_sort_rows, rehearsed with stable argsorts"""
    for seed in range(4):
        row, col, _ = _random_list(seed, N=12, E=500)
        assert np.array_equal(R.sorted_positions_two_groupings(row, col), R.sorted_positions(row, col))
    row, col, _ = planted.edges(2048, 256, 'shuffled')
    assert np.array_equal(R.sorted_positions_two_groupings(row, col), R.sorted_positions(row, col))


@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.int64])
@pytest.mark.parametrize('op', R.OPS)
def test_the_fast_fold_is_the_loop(dtype, op):
    rng = np.random.RandomState(3)
    for n in (1, 2, 255, 256, 257, 513, 700):
        v = (rng.uniform(-1, 1, n) * 10.0 ** rng.randint(-3, 4, n)).astype(dtype) if dtype != np.int64 else \
            ((1 << 62) - rng.randint(0, 1000, n)).astype(np.int64)
        a, b = R.fold(v, op), R.fold_loop(v, op)
        assert a.dtype == b.dtype == dtype and a.tobytes() == b.tobytes(), (n, a, b)
    if dtype != np.int64:
        for v in ([0.0, -0.0], [-0.0, 0.0], [1.0, np.nan, -1.0], [np.nan], [-0.0, 0.0, 0.0, -0.0]):
            v = np.array(v, dtype=dtype)
            assert R.fold(v, op).tobytes() == R.fold_loop(v, op).tobytes(), (v, op)


def test_min_max_rules():
    for dtype in (np.float32, np.float64):
        z = lambda *v: np.array(v, dtype=dtype)
        assert np.signbit(R.fold_loop(z(-0.0, 0.0), 'min')) and not np.signbit(R.fold_loop(z(0.0, -0.0), 'min'))
        assert np.signbit(R.fold_loop(z(-0.0, 0.0), 'max')) and not np.signbit(R.fold_loop(z(0.0, -0.0), 'max'))
        for op in ('min', 'max'):
            assert np.isnan(R.fold_loop(z(1.0, np.nan, -1.0), op)) and np.isnan(R.fold_loop(z(np.nan, 2.0), op))
            assert R.fold_loop(z(1.0, np.nan), op).tobytes() == np.array(np.nan, dtype=dtype).tobytes()
        assert R.fold_loop(z(3.0, -2.0, 5.0), 'min') == -2.0 and R.fold_loop(z(3.0, -2.0, 5.0), 'max') == 5.0
    assert R.fold_loop(np.array([-7, 2], dtype=np.int64), 'mean') == -3  # floor, not truncation
    assert R.fold_loop(np.array([7, -2], dtype=np.int64), 'mean') == 2


def test_fractional_add_against_float64(capsys):
    """the chunked float32 sum of a run of k entries lies within gamma_{k + 1} * sum |w| of the exact sum (a sequential sum of n terms
    is within gamma_{n - 1}; chunks of at most 256 and at most ceil(k / 256) chunk sums make fewer than k + 1 roundings per term)"""
    u = np.float64(2.0 ** -24)
    worst = 0.0
    rng = np.random.RandomState(5)
    for k in (1, 2, 3, 255, 256, 257, 511, 513, 4000, 16385):
        w = (rng.uniform(-1, 1, k) * 10.0 ** rng.randint(-3, 4, k)).astype(np.float32)
        got = np.float64(R.fold_loop(w, 'add'))
        exact = np.sum(w.astype(np.float64))  # (float64 of float32 terms: its own error is 2^-29 of this bound)
        gamma = (k + 1) * u / (1 - (k + 1) * u)
        bound = gamma * np.sum(np.abs(w.astype(np.float64)))
        assert abs(got - exact) <= bound, (k, got, exact, bound)
        worst = max(worst, abs(got - exact) / bound)
    with capsys.disabled():
        print(f'\ngraph_prep: worst |chunked float32 sum - float64 sum| / (gamma_(k+1) * sum|w|) over the planted run lengths = {worst:.4f}')
    assert worst <= 1.0


def test_the_chunk_rule_is_the_plain_loop_up_to_257_and_differs_from_258():
    """Up to 256 entries there is one chunk.  At 257 the second chunk is ONE entry, so the chunked sum is (the sequential sum of the
    first 256) + the last entry: still the plain loop, for every input.  258 entries is the first length at which the second chunk sums
    on its own, and a planted run shows that the test can see the rule."""
    rng = np.random.RandomState(7)
    for k in (1, 2, 100, 255, 256, 257):
        for _ in range(3):
            w = (rng.uniform(-1, 1, k) * 10.0 ** rng.randint(-3, 4, k)).astype(np.float32)
            assert R.fold_loop(w, 'add').tobytes() == R.fold_sequential(w, 'add').tobytes()
    # 1, 255 zeros | 2^-24, 2^-24.  Plain loop: 1 + 2^-24 is a tie and rounds to even, 1, twice.  Chunk rule: 2^-24 + 2^-24 = 2^-23 =
    # one ulp of 1 survives
    w = np.array([1.0] + [0.0] * 255 + [2.0 ** -24, 2.0 ** -24], dtype=np.float32)
    assert len(w) == 258
    assert R.fold_sequential(w, 'add') == np.float32(1.0)
    assert R.fold_loop(w, 'add') == np.float32(1.0) + np.float32(2.0 ** -23) != np.float32(1.0)
    assert R.fold(w, 'add').tobytes() == R.fold_loop(w, 'add').tobytes()


def test_to_undirected_on_a_hand_written_list():
    # a reciprocal pair (0,1)/(1,0), a duplicate (2,3) twice, a self loop (4,4), a lone arc (5,0)
    row = np.array([0, 1, 2, 2, 4, 5])
    col = np.array([1, 0, 3, 3, 4, 0])
    w = np.array([1.5, 2.0, 0.25, 0.5, 3.0, 7.0], dtype=np.float32)
    out = R.to_undirected(row, col, w, 6, 'add')
    assert out['row'].tolist() == [0, 0, 1, 2, 3, 4, 5]
    assert out['col'].tolist() == [1, 5, 0, 3, 2, 4, 0]
    assert out['value'].tolist() == [3.5, 7.0, 3.5, 0.75, 0.75, 6.0, 7.0]
    assert out['count'].tolist() == [2, 1, 2, 2, 2, 2, 1]
    assert out['rowptr'].tolist() == [0, 2, 3, 4, 5, 6, 7]
    assert R.is_symmetric(out)
    plain = R.coalesce(row, col, w, 6, 'add')
    assert plain['row'].tolist() == [0, 1, 2, 4, 5] and plain['value'].tolist() == [1.5, 2.0, 0.75, 3.0, 7.0]
    assert not R.is_symmetric(plain) and not R.is_symmetric(plain, weights=False)
    assert R.to_undirected(row, col, w, 6, 'mean')['value'].tolist() == [1.75, 7.0, 1.75, 0.375, 0.375, 3.0, 7.0]


def test_the_planted_graph_is_what_its_plan_says():
    block, chunk = 2048, 256
    runs = planted.plan(block, chunk)
    assert runs == sorted(runs) and len({(r, c) for r, c, _ in runs}) == len(runs)
    lengths = [n for _, _, n in runs]
    for n in (1, 2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 64 * chunk + 1):
        assert n in lengths
    starts = np.concatenate([[0], np.cumsum(lengths)])
    assert 2 * block - 1 in starts and 2 * block in starts          # heads at the last / first position of a workgroup
    big = lengths.index(64 * chunk + 1)
    assert starts[big] == 2 * block and starts[big + 1] > 3 * block  # and a run across the boundaries
    rows = sorted({r for r, _, _ in runs})
    assert rows[0] == 3 and {b - a - 1 for a, b in zip(rows, rows[1:])} >= {1, 2, 100} and rows[-1] < planted.N - 1
    for order in ('shuffled', 'ascending', 'descending'):
        row, col, run_of = planted.edges(block, chunk, order)
        out = R.coalesce(row, col, None, planted.N)
        assert list(zip(out['row'], out['col'], out['count'])) == runs
        assert np.array_equal(run_of[out['perm']], np.repeat(np.arange(len(runs)), lengths))


def test_argument_errors_before_any_device():
    import subgraph_sketching_amd as ssa
    gp = ssa.graph_prep
    assert ssa.coalesce is gp.coalesce and ssa.to_undirected is gp.to_undirected and ssa.coalesce_graph is gp.coalesce_graph
    assert ssa._native.lib().ss_coalesce_chunk() == R.CHUNK and ssa._native.lib().ss_coalesce_block() % 256 == 0
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    w = torch.ones(3)
    with pytest.raises(ValueError, match='square'):
        gp.coalesce(ei, w, 3, 4)
    with pytest.raises(ValueError, match='out of scope'):
        gp.coalesce(ei, w, 3, 3, op='mul')
    with pytest.raises(ValueError, match='multi-column'):
        gp.coalesce(ei, torch.ones(3, 2), 3, 3)
    with pytest.raises(ValueError, match='int64, float32 or float64'):
        gp.coalesce(ei, torch.ones(3, dtype=torch.float16), 3, 3)
    with pytest.raises(ValueError, match='int64, float32 or float64'):
        gp.to_undirected(ei, torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        gp.coalesce(ei, torch.ones(4), 3, 3)
    with pytest.raises(ValueError, match='int64'):
        gp.coalesce(ei.to(torch.int32), w, 3, 3)
    with pytest.raises(ValueError):
        gp.coalesce(ei[0], w, 3, 3)
    with pytest.raises(ValueError, match='num_nodes'):
        gp.coalesce_graph(0, ei)
    with pytest.raises(ValueError, match='num_nodes'):
        gp.coalesce_graph(1 << 31, ei)
    with pytest.raises(ValueError, match='long_entries'):
        gp.coalesce_graph(3, ei, w, long_entries=0)
    with pytest.raises(ValueError, match='reduce'):
        gp.coalesce_graph(3, ei, w, reduce='mul')
    with pytest.raises(ValueError, match='differentiable'):
        gp.coalesce_graph(3, ei, torch.ones(3, requires_grad=True))
    huge = torch.zeros(1, dtype=torch.int64).as_strided((2, (1 << 30) + 1), (0, 0))  # (a shape over one word: never read)
    with pytest.raises(ValueError, match='doubled'):
        gp.to_undirected(huge, num_nodes=5)
    lib = ssa._native.lib()
    assert lib.ss_coalesce_mark(None, None, None, 5, 3, None, None, None) == -1       # null pointers
    assert lib.ss_coalesce_mark(None, None, None, 0, 3, None, None, None) == 0        # empty: nothing to do
    assert lib.ss_coalesce_mark(None, None, None, 1 << 31, 3, None, None, None) == -1
    assert lib.ss_coalesce_fill(None, None, None, 0, 3, None, 0, None, None, None, None, None) == 0
    assert lib.ss_coalesce_fill(None, None, None, 4, 3, None, 5, None, None, None, None, None) == -1   # more runs than entries
    assert lib.ss_coalesce_reduce(None, None, 0, None, 0, 0, 0, 256, None, None, None, 0, None, None) == 0
    assert lib.ss_coalesce_reduce(None, None, 3, None, 0, 0, 0, 0, None, None, None, 0, None, None) == -1  # long_entries < 1
    from ctypes import c_void_p
    fake = c_void_p(8)  # never dereferenced: the calls below are rejected by the host-side checks
    assert lib.ss_coalesce_reduce(fake, fake, 3, fake, 3, 7, 0, 256, fake, fake, fake, 1, fake, None) == -4  # no such dtype
    assert lib.ss_coalesce_reduce(fake, fake, 3, fake, 3, 1, 4, 256, fake, fake, fake, 1, fake, None) == -4  # no such op ('mul')
    assert lib.ss_coalesce_reduce_long(fake, fake, 3, fake, 3, 1, 9, fake, fake, fake, 1, None) == -4
    assert lib.ss_coalesce_symmetric(None, None, None, 0, 3, None, 0, None, None) == -1
