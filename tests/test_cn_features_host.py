"""What heuristics.common_neighbours / common_neighbour_features promise that needs no device: the restatement the GPU tests compare
against (tests/cn_features_restatement.py) is pinned to scipy, the argument errors come before a device is touched, the C ABI rejects
bad arguments on the host, and the byte model is counted by hand."""
import numpy as np
import pytest
import torch

import cn_features_restatement as cr
import heuristics_restatement as hr


@pytest.fixture(scope='module')
def shared():
    return hr.shared_count_graph()


def _matrix(shared, weighting, seed=11):
    src, dst, links, n = shared
    return hr.matrix(src, dst, hr.weights(weighting, src, dst, n, seed), n, weighting), links, n


def _unit_matrix(shared):
    """every stored value 1 (hr.weights('unit') sums the duplicate edges of the planted graph to 2)"""
    A, links, n = _matrix(shared, 'unit')
    A.data[:] = 1
    return A, links, n


@pytest.mark.parametrize('weighting', ['unit', 'random'])
@pytest.mark.parametrize('kind', ['CN', 'AA', 'RA'])
def test_restatement_against_scipy_in_float64(shared, weighting, kind):
    """every element within gamma_k (|S| @ |x|), gamma_k = k 2^-24 / (1 - k 2^-24), k = m + 2 for a link of m common neighbours: one
    rounding of the coefficient, one per product, m - 1 adds, one unit of slack"""
    A, links, n = _matrix(shared, weighting)
    x = np.random.RandomState(21).standard_normal((n, 8)).astype(np.float32)
    got = cr.pooled(A, links, x, kind).astype(np.float64)
    want, scale, S = cr.scipy_pooled_f64(A, links, x, kind)
    rowptr, ids, _ = cr.lists(A, links, kind)
    m = np.diff(rowptr)
    assert m.max() == 5005 and m.min() == 0 and m.sum() == 45682
    k = (m + 2) * 2.0 ** -24
    bound = (k / (1 - k))[:, None] * scale
    err = np.abs(got - want)
    bad = np.nonzero(err > bound)
    worst = float((err[scale > 0] / bound[scale > 0]).max())
    print(f'{weighting} {kind}: worst error / bound = {worst:.3f}')
    assert len(bad[0]) == 0, f'{len(bad[0])} elements beyond the bound, worst ratio {worst}'
    assert np.all(got[m == 0] == 0) and not np.signbit(got[m == 0]).any()


def test_lists_against_scipy(shared):
    """counts = CN on the unit matrix, exactly; on positive weights the ids are the stored columns of S = A[src] .* A[dst]"""
    A, links, n = _unit_matrix(shared)
    rowptr, ids, coef = cr.lists(A, links, None)
    assert coef is None and rowptr.dtype == np.int64 and ids.dtype == np.int64
    assert np.array_equal(np.diff(rowptr).astype(np.float32), hr.scores(A, links, 'CN'))
    A, links, n = _matrix(shared, 'random')
    rowptr, ids, coef = cr.lists(A, links, 'CN')
    _, _, S = cr.scipy_pooled_f64(A, links, np.zeros((n, 1), dtype=np.float32), 'CN')
    S.sort_indices()
    assert np.array_equal(S.indptr, rowptr) and np.array_equal(S.indices, ids)
    assert coef.dtype == np.float32 and np.array_equal(coef, S.data.astype(np.float32))
    for q in (0, 17, 35, len(links) - 1):  # ascending inside every link
        assert np.all(np.diff(ids[rowptr[q]:rowptr[q + 1]]) > 0)


def test_stored_zeros_are_members(shared):
    A, links, n = _matrix(shared, 'zeros')
    assert (A.data == 0).sum() > 1000
    counts = np.diff(cr.lists(A, links, 'CN')[0])
    assert np.array_equal(counts, np.diff(cr.lists(_unit_matrix(shared)[0], links, None)[0]))


def test_cn_identity(shared):
    """x = ones [N, 1] on the unit matrix: the pooled column is CN, bit for bit"""
    A, links, n = _unit_matrix(shared)
    got = cr.pooled(A, links, np.ones((n, 1), dtype=np.float32), 'CN')[:, 0]
    want = hr.scores(A, links, 'CN')
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_argument_errors_need_no_device(shared):
    import subgraph_sketching_amd as ssa
    hz = ssa.heuristics
    A, links, n = _matrix(shared, 'unit')
    links = torch.from_numpy(links)
    x = torch.zeros((n, 4), dtype=torch.float32)
    for bad_links in (links[:, 0], links.reshape(-1, 2, 1), torch.zeros((3, 3), dtype=torch.int64), links.to(torch.float32)):
        with pytest.raises(ValueError):
            hz.common_neighbour_features(A, bad_links, x)
        with pytest.raises(ValueError):
            hz.common_neighbours(A, bad_links)
    for bad_x in (x.double(), x.half(), x.to(torch.int32), x[:, 0], x[None], x[:-1], torch.zeros((n + 1, 4)), x.numpy()):
        with pytest.raises(ValueError):
            hz.common_neighbour_features(A, links, bad_x)
    for bad_w in (torch.ones(n - 1, dtype=torch.float64), np.ones(n + 1, dtype=np.float32), torch.ones((n, 1)), torch.ones(n, dtype=torch.int64),
                  'PPR'):
        with pytest.raises(ValueError):
            hz.common_neighbour_features(A, links, x, weighting=bad_w)
        with pytest.raises(ValueError):
            hz.common_neighbours(A, links, weighting=bad_w)
    with pytest.raises(ValueError):
        hz.common_neighbour_features(A, links, x, weighting=None)
    L = links.size(0)
    for bad_out in (torch.zeros((L, 5)), torch.zeros((L + 1, 4)), torch.zeros((L, 4), dtype=torch.float64), torch.zeros((4, L)).t(),
                    torch.zeros(L * 4)):
        with pytest.raises(ValueError):
            hz.common_neighbour_features(A, links, x, out=bad_out)
    assert hz.CommonNeighbours._fields == ('rowptr', 'ids', 'coef')


def test_c_abi_rejects_bad_arguments_on_the_host():
    from ctypes import c_void_p
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(16)  # never dereferenced: every call below ends in the host-side checks
    assert lib.ss_common_neighbour_count(None, None, 4, None, 3, None, None, None) == -1
    assert lib.ss_common_neighbour_count(fake, fake, 4, fake, -1, fake, None, None) == -1
    assert lib.ss_common_neighbour_count(fake, fake, 1 << 31, fake, 3, fake, None, None) == -1
    assert lib.ss_common_neighbour_count(None, None, 4, None, 0, None, None, None) == 0          # no links: nothing to do
    assert lib.ss_common_neighbour_fill(fake, fake, None, None, 4, fake, 3, None, fake, None, None, None) == -1   # offsets missing
    assert lib.ss_common_neighbour_fill(fake, fake, None, None, 4, fake, 3, fake, None, None, None, None) == -1   # ids missing
    assert lib.ss_common_neighbour_fill(None, None, None, None, 4, None, 0, None, None, None, None, None) == 0
    assert lib.ss_common_neighbour_pool(fake, fake, None, None, 4, fake, 3, None, 8, fake, None, None) == -1      # x missing
    assert lib.ss_common_neighbour_pool(fake, fake, None, None, 4, fake, 3, fake, 8, None, None, None) == -1      # out missing
    assert lib.ss_common_neighbour_pool(fake, fake, None, None, 4, fake, 3, fake, -1, fake, None, None) == -1     # F < 0
    assert lib.ss_common_neighbour_pool(None, None, None, None, 4, None, 0, None, 8, None, None, None) == 0
    assert lib.ss_version() == 129


def test_byte_model_on_a_hand_counted_case():
    """3 links whose six rows hold 10 entries in all and which share 4 neighbours, F = 8:
    links 3 * 16 = 48, row pointers 3 * 32 = 96, columns 10 * 4 = 40 -> 184 for every launch"""
    import subgraph_sketching_amd as ssa
    b = ssa.roofline.cn_features_bytes(links=3, row_entries=10, hits=4, F=8)
    assert b == {'count': 184 + 24, 'fill': 184 + 24 + 4 * 12, 'pool': 184 + 4 * 32 + 3 * 32}
    w = ssa.roofline.cn_features_bytes(links=3, row_entries=10, hits=4, F=8, weighted=True)
    assert w['count'] == b['count']                      # membership reads no values
    assert w['fill'] - b['fill'] == 80 + 32 == w['pool'] - b['pool']
    assert ssa.roofline.cn_features_bytes(0, 0, 0, 128) == {'count': 0, 'fill': 0, 'pool': 0}
