"""CN / AA / RA on the host: the restatement's float32 summation order against scipy itself, and the CPU oracle's float32 mode
against the restatement bit for bit (tests/heuristics_restatement.py) -- what the GPU tests then hold the kernel to."""
import numpy as np
import pytest
import scipy.sparse as sp

import heuristics_restatement as hr


@pytest.mark.parametrize('scale', [1.0, 1e-3, 1e4])
def test_pairwise_order_is_scipys_row_sum(scale):
    """one-row float32 matrices of every length up to 300 and across the 128-term leaves and numpy's 8192-element buffer"""
    rng = np.random.RandomState(int(scale * 7) % 1000)
    lengths = list(range(0, 301)) + [1000, 1023, 1024, 1025, 8191, 8192, 8193, 8200, 20000]
    for m in lengths:
        t = (rng.uniform(-1, 1, size=m) * 10.0 ** rng.uniform(-4, 4, size=m) * scale).astype(np.float32)
        t[t == 0] = 1  # stored zeros would be part of the row: keep to non-zero terms, as scipy's products are
        row = sp.csr_matrix((t, (np.zeros(m, dtype=np.int64), np.arange(m))), shape=(1, max(m, 1)))
        want = np.array(np.sum(row, 1)).flatten()[0]
        assert want.dtype == np.float32
        got = hr.row_sum_f32(t)
        assert got.tobytes() == want.tobytes(), m
    # and the order matters on these inputs: plain in-order float32 accumulation differs somewhere
    t = (rng.uniform(0, 1, size=5000) * 10.0 ** rng.uniform(-4, 4, size=5000)).astype(np.float32)
    seq = np.float32(0)
    for x in t:
        seq = np.float32(seq + x)
    assert seq != hr.row_sum_f32(t)


def _cases():
    src, dst, links, n = hr.shared_count_graph()
    for wk in ('unit', 'random', 'small', 'colsum_one', 'zeros'):
        yield f'shared-{wk}', hr.matrix(src, dst, hr.weights(wk, src, dst, n, 1), n, wk), links
    s2, d2 = hr.powerlaw_graph(4000, 30000, 5)
    rng = np.random.RandomState(6)
    l2 = np.concatenate([rng.randint(0, 4000, size=(4000, 2)), rng.randint(0, 40, size=(1000, 2))])
    for wk in ('unit', 'random'):
        yield f'powerlaw-{wk}', hr.matrix(s2, d2, hr.weights(wk, s2, d2, 4000, 2), 4000), l2


@pytest.mark.parametrize('kind', ['CN', 'AA', 'RA'])
def test_oracle_float32_mode_is_the_restatement(kind):
    from oracle import oracle
    seen_counts = set()
    for name, A, links in _cases():
        assert A.dtype == np.float32
        want = hr.scores(A, links, kind)
        got = oracle.common_neighbour_scores(A, links, kind)
        assert got.dtype == np.float32
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert len(bad) == 0, (name, kind, bad[:5], got[bad[:5]], want[bad[:5]])
        if name.startswith('shared'):
            P = A[links[:, 0]].multiply(A[links[:, 1]])
            seen_counts |= set(np.diff(P.tocsr().indptr).tolist())
    assert set(hr.COUNTS) - {0} <= seen_counts | {0}  # every length of interest was really summed


def test_multiplier_edge_cases_are_reached():
    """the weightings of the GPU tests reach negative AA multipliers (column sums in (0, 1)) and zero ones (sums of 1)"""
    src, dst, _, n = hr.shared_count_graph()
    small = hr.multiplier(hr.matrix(src, dst, hr.weights('small', src, dst, n, 1), n), 'AA')
    one = hr.multiplier(hr.matrix(src, dst, hr.weights('colsum_one', src, dst, n, 1), n), 'AA')
    assert small.dtype == np.float32 and (small < 0).sum() > 1000
    assert (one == 0).sum() > 100 and np.isfinite(one).all()


def test_oracle_fp64_mode_for_other_dtypes():
    """int matrices: CN and the fp64 sums exact up to the final rounding; bool: integer counts; float64: within one ulp"""
    from oracle import oracle
    src, dst, links, n = hr.shared_count_graph(counts=(1, 9, 129, 3001))
    rng = np.random.RandomState(3)
    Ai = hr.matrix(src, dst, rng.randint(1, 5, size=len(src)).astype(np.int32), n)
    Ab = hr.matrix(src, dst, np.ones(len(src), dtype=bool), n)
    Ad = hr.matrix(src, dst, 10.0 ** rng.uniform(-3, 3, size=len(src)), n)
    assert np.array_equal(oracle.common_neighbour_scores(Ai, links, 'CN'), hr.scores(Ai, links, 'CN'))
    assert np.array_equal(oracle.common_neighbour_scores(Ab, links, 'CN'), hr.scores(Ab, links, 'CN'))
    for kind in ('AA', 'RA'):
        for A in (Ai, Ab, Ad):
            got, want = oracle.common_neighbour_scores(A, links, kind), hr.scores(A, links, kind)
            assert np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))), (kind, A.dtype)
