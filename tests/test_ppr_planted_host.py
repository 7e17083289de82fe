"""The planted PPR graph (tests/ppr_planted.py) without a GPU: the graph is what it says (kept in-degrees, hubs, segments, the
zero-sum rows), the comparison of tests/test_ppr_planted_gpu.py bites (each named mutation of the restated operator moves a
compared number by more than 1e-8 relative, four decades above the GPU test's 1e-10), and the stop patterns that test relies on
exist with the margin that makes iteration counts comparable for equality."""
import numpy as np
import pytest
import torch

import ppr_planted as pp


@pytest.fixture(scope='module', params=list(pp.VARIANTS))
def case(request):
    A, desc = pp.variant(request.param)
    W, z = pp.kept_operator(A, pp.ROWS_CFG['p'])
    return A, desc, W, z


def test_shape_of_the_graph():
    A, desc = pp.variant('one')
    assert A.shape == (pp.N, pp.N) and A.dtype == np.float64 and pp.N == 16449
    assert (pp.N + 63) // 64 == 258 and pp.N % 64 == 1          # the finalize stride runs twice; the last workgroup holds one row
    assert (1 / pp.N) * pp.N == 1.0                             # a dangling source is an exact fixed point
    deg_out, deg_in = np.diff(A.indptr), np.bincount(A.indices, minlength=pp.N)
    isolated = np.arange(1021, 1100)
    assert not deg_out[isolated].any() and not deg_in[isolated].any() and pp.ISOLATED in isolated
    assert np.count_nonzero((deg_out[:1000] == 0) & (deg_in[:1000] == 0)) > 900
    assert deg_out[pp.SINK] == 0 and deg_out[pp.DANGLING] == 0 and deg_in[pp.DANGLING] == 1
    r = np.asarray(A.sum(axis=1)).ravel()
    assert not r[pp.ZERO_ROWS].any() and (deg_out[pp.ZERO_ROWS] == 3).all()   # exactly 0: 1.5 + 1.5 - 3.0


def test_kept_degrees_equal_the_plan(case):
    A, desc, W, z = case
    deg = np.diff(W.indptr)
    for row, d in desc['in_rows'].items():
        assert deg[row] == d, (row, d, deg[row])
    assert set(pp.SMALL_DEGREES) | set(desc['hub_degrees']) == set(desc['targets'].values())
    assert set(pp.FIXED_PLACES) <= set(desc['targets'])
    others = np.ones(pp.N, dtype=bool)
    others[list(desc['in_rows'])] = False
    assert deg[others].max() <= pp.SEGMENT
    assert (W.data > 0).all()                                   # what the relative tolerance of the GPU tests rests on
    stored = np.bincount(A.indices, minlength=pp.N)             # A is canonical: one stored entry per (u, v)
    assert stored[pp.KEPT_256] == 296 and deg[pp.KEPT_256] == 256
    assert stored[pp.KEPT_257] == 297 and deg[pp.KEPT_257] == 257
    assert stored[pp.SINK] == 40 and deg[pp.SINK] == 0
    for row in (pp.KEPT_256, pp.KEPT_257):
        assert not np.isin(W.indices[W.indptr[row]:W.indptr[row + 1]], pp.ZERO_ROWS).any()
    assert z[pp.SINK] == 1 / pp.N and z[pp.ZERO_ROWS[0]] == 1 / pp.N and z[pp.B] == (1 - pp.ROWS_CFG['p']) / pp.N


def test_hubs_and_segments_equal_the_table_and_the_operator(case):
    """_PprOperator, built on the CPU, against the plain restatement of its hub lists"""
    from subgraph_sketching_amd.heuristics import DeviceAdjacency
    A, desc, W, z = case
    deg = np.diff(W.indptr)
    hubs, hub_seg, seg_hub = pp.hub_plan(deg)
    assert (len(hubs), int(hub_seg[-1])) == pp.COUNTS[desc['name']] == (desc['n_hubs'], desc['n_segments'])
    assert list(hubs) == desc['hubs']
    op = DeviceAdjacency(A, torch.device('cpu')).ppr_operator(pp.ROWS_CFG['p'])
    assert (op.n_hubs, op.n_segments, op.nnz) == (len(hubs), int(hub_seg[-1]), W.nnz)
    assert np.array_equal(op.hub_rows.numpy()[:op.n_hubs], hubs)
    assert np.array_equal(op.hub_seg.numpy(), hub_seg)
    assert np.array_equal(op.seg_hub.numpy()[:op.n_segments], seg_hub)
    assert np.array_equal(op.rowptr.numpy(), W.indptr) and np.array_equal(op.col.numpy()[:op.nnz], W.indices)
    assert np.array_equal(op.w.numpy()[:op.nnz], W.data) and np.array_equal(op.z, z)
    last = [int(deg[h] - (deg[h] - 1) // pp.SEGMENT * pp.SEGMENT) for h in hubs]   # edges of every hub's last segment
    if desc['name'] == 'nine':
        assert sorted(last) == sorted([1, 1, 2, 255, 256, 1, 256, 1, 1])      # 257 (1004), 257, 258, 511, 512, 513, 768, 769, 1025
        ids = sorted(desc['hubs'])
        assert any(a < b and a // 64 == b // 64 and (b - a) % 4 == 0 for a in ids for b in ids)   # two hubs share a wavefront


def test_the_mass_spreads(case):
    """after the 12 steps of the rows configuration a restated vector of a slow source is non-zero on most nodes, and on every
    in-neighbour of every hub row: the long sums add real terms, not zeros"""
    A, desc, W, z = case
    srcs, vec, iters, _ = pp.restated(desc['name'], 'rows', 'rows')
    slow = iters > 1
    assert slow.sum() == len(srcs) - len(pp.QUICK)
    nonzero = (vec[slow] != 0).mean(axis=1)
    assert nonzero.min() > 0.85, nonzero.min()
    for h in desc['hubs']:
        nbrs = W.indices[W.indptr[h]:W.indptr[h + 1]]
        assert (vec[slow][:, nbrs] != 0).all(), h


def test_source_lists(case):
    A, desc, W, z = case
    wide, rows = pp.sources(desc, 'widths'), pp.sources(desc, 'rows')
    assert len(wide) == len(set(wide)) == 129 and rows == wide[:70] and pp.sources(desc, 'stops') == rows
    named = set(desc['hubs']) | set(pp.FIXED_PLACES) | set(pp.QUICK) | {pp.KEPT_256, pp.KEPT_257, pp.B} | set(desc['targets'])
    assert named <= set(rows)
    assert sum(pp.FEEDER_LO <= s < pp.FEEDER_HI for s in rows) >= 20


@pytest.mark.parametrize('name', pp.MUTATIONS)
def test_each_mutation_moves_a_compared_number(name):
    """on `nine` with the source list and configuration of the GPU test of every planted row"""
    A, desc = pp.variant('nine')
    cfg = pp.ROWS_CFG
    srcs, vec, iters, _ = pp.restated('nine', 'rows', 'rows')
    W, z = pp.kept_operator(A, cfg['p'])
    same, same_iters, _ = pp.power(W, z, srcs, cfg['tol'], cfg['max_iter'])
    assert np.array_equal(same, vec) and np.array_equal(same_iters, iters)      # power() is pagerank_power on the true operator
    M = pp.mutate(W, cfg['p'], name)
    expect_nnz = {'segment_end': W.nnz - 18, 'stored_degree': W.nnz + 40, 'no_teleport': W.nnz}   # 18 full segments among 25
    if name in expect_nnz:
        assert M.nnz == expect_nnz[name]
    else:
        assert M.nnz < W.nnz - 14400                                            # every feeder row has degree 2
    got, _, _ = pp.power(M, z, srcs, cfg['tol'], cfg['max_iter'], no_teleport_from=64 if name == 'no_teleport' else None)
    worst = pp.worst_relative(got, vec)
    print(f'mutation {name}: worst relative difference {worst:.3e}')
    assert worst > 1e-8
    if name == 'no_teleport':
        assert np.array_equal(got[:64], vec[:64])                               # the first slice is untouched


@pytest.mark.parametrize('name', list(pp.VARIANTS))
def test_stop_pattern_of_the_rows_configuration(name):
    """quick sources stop after one step at exactly e_src, every other column runs all 12; no residual near tol"""
    cfg = pp.ROWS_CFG
    for kind in ('rows', 'widths') if name == 'nine' else ('rows',):
        srcs, vec, iters, res = pp.restated(name, kind, 'rows')
        for j, s in enumerate(srcs):
            if s in pp.QUICK:
                assert iters[j] == 1 and np.array_equal(vec[j], np.eye(1, pp.N, s)[0]), s
            else:
                assert iters[j] == cfg['max_iter'], (s, iters[j])
        assert pp.closest_residual(res, cfg['tol']) > pp.MARGIN


def test_stop_pattern_of_the_stops_configuration():
    cfg = pp.STOPS_CFG
    srcs, vec, iters, res = pp.restated('five', 'stops', 'stops')
    closest = pp.closest_residual(res, cfg['tol'])
    slow = iters[iters > 1]
    print(f'stops: counts {sorted(set(iters.tolist()))}, closest residual within {closest:.3e} of tol')
    assert closest > pp.MARGIN
    assert slow.max() < cfg['max_iter'] and len(set(slow.tolist())) >= 4        # stopped on tol, at several different steps
    assert sorted(s for s, k in zip(srcs, iters) if k == 1) == sorted(pp.QUICK)
    order, pairs = pp.stop_order(srcs, iters)
    count = dict(zip(srcs, iters.tolist()))
    k = [count[s] for s in order]
    assert len(order) == 128
    a, b = pairs['left_first']
    assert (a, b) == (0, 1) and 1 < k[a] < k[b]
    a, b = pairs['right_first']
    assert (a, b) == (2, 3) and k[a] > k[b] > 1
    a, b = pairs['quick_slow']
    assert (a, b) == (4, 5) and k[a] == 1 < k[b]
    a, b = pairs['slow_quick']
    assert (a, b) == (6, 7) and k[a] > 1 == k[b]
    assert all(c > 1 for c in k[:4] + k[8:64]) and all(c == 1 for c in k[64:])
    assert len(set(order[:64])) == 64                                           # PPR_COLUMNS = 1 runs each of them alone
    mirrored = order[::-1]
    km = [count[s] for s in mirrored]
    assert all(c == 1 for c in km[:64]) and km[126] > km[127] > 1 and km[124] < km[125]   # the pairs flip with the order
