"""heuristics.common_neighbours / common_neighbour_features (csrc/ss_cn_pool.hip) on the GPU against their numpy restatement
(tests/cn_features_restatement.py, pinned to scipy by tests/test_cn_features_host.py).  Everything is compared as bits: the
lists are integers, a coefficient is one rounding of an fp64 product, and a pooled element is one lane's float32 sum over
ascending common neighbours -- there is exactly one right answer."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cn_features_restatement as cr
import heuristics_restatement as hr
import large_table_helpers as lt

pytestmark = pytest.mark.gpu

POOL_COLUMNS_PER_PASS = 256  # 64 lanes x one float4: F = 257 and 260 need a second pass over the hits


@pytest.fixture(scope='module')
def hz():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m.heuristics


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return hr.shared_count_graph()


@pytest.fixture(scope='module')
def features(shared):
    """float32 [N, 260]: the first F columns are the x of every F"""
    return np.random.RandomState(41).standard_normal((shared[3], 260)).astype(np.float32)


def _matrix(shared, weighting, seed=11):
    src, dst, links, n = shared
    return hr.matrix(src, dst, hr.weights(weighting, src, dst, n, seed), n, weighting)


def _custom(n, seed=43):
    """a seeded multiplier of the caller's own: both signs, six decades, some exact zeros"""
    rng = np.random.RandomState(seed)
    m = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-3, 3, size=n)
    m[::13] = 0
    return m


def _bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f'{what}: {g.dtype} {tuple(g.shape)} against {w.dtype} {tuple(w.shape)}'
    bad = torch.nonzero(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} of {g.numel()} elements differ, first at {bad[:4].tolist()}'


def _assert_lists(got, want, what):
    rowptr, ids, coef = want
    assert got.rowptr.dtype == torch.int64 and got.ids.dtype == torch.int64
    _assert_same(got.rowptr, rowptr, what + ' rowptr')
    _assert_same(got.ids, ids, what + ' ids')
    if coef is None:
        assert got.coef is None, what
    else:
        assert got.coef.dtype == torch.float32
        _assert_same(got.coef, coef, what + ' coef')


@pytest.mark.parametrize('weighting', ['unit', 'random', 'zeros'])
def test_bit_equal_on_chosen_term_counts(hz, dev, shared, features, weighting):
    """pairs of 1, 2, 7, 8, 9, 15, 16, 17, 127 ... 257, 1000, 3001 and 5000 (+ 5) common neighbours, both ways round, self pairs,
    isolated nodes and pool pairs; CN, AA, RA and a custom multiplier at F = 20; lists with and without coefficients"""
    src, dst, links, n = shared
    A = _matrix(shared, weighting)
    adj = hz.DeviceAdjacency(A, dev)
    lk = torch.from_numpy(links).to(dev)
    x = np.ascontiguousarray(features[:, :20])
    xd = torch.from_numpy(x).to(dev)
    custom = _custom(n)
    for name, w in (('CN', 'CN'), ('AA', 'AA'), ('RA', 'RA'), ('custom', custom)):
        want = cr.lists(A, links, w)
        assert np.diff(want[0]).max() == 5005
        _assert_lists(hz.common_neighbours(adj, lk, weighting=w), want, f'{weighting} {name}')
        out = hz.common_neighbour_features(adj, lk, xd, weighting=w)
        assert out.dtype == torch.float32 and out.device == lk.device
        _assert_same(out, cr.pool_lists(*want, x), f'{weighting} {name} pooled')
    _assert_lists(hz.common_neighbours(adj, lk), cr.lists(A, links, None), f'{weighting} ids only')
    _assert_lists(hz.common_neighbours(adj, lk, weighting=torch.from_numpy(custom.astype(np.float32))),
                  cr.lists(A, links, custom.astype(np.float32)), f'{weighting} float32 multiplier')


@pytest.mark.parametrize('F', [0, 1, 3, 4, 20, 64, 128, 260, POOL_COLUMNS_PER_PASS + 1])
def test_bit_equal_for_every_feature_width(hz, dev, shared, features, F):
    """random weights / RA: F = 0, widths that are no multiple of 4 (scalar accesses), every unit size (16, 32, 64 lanes) and two
    widths just beyond one pass of the unit; x handed over as a non-contiguous column slice"""
    src, dst, links, n = shared
    A = _matrix(shared, 'random')
    want = cr.pool_lists(*cr.lists(A, links, 'RA'), np.ascontiguousarray(features[:, :F]))
    x = torch.from_numpy(features).to(dev)[:, :F]
    assert F in (0, 260) or not x.is_contiguous()
    out = hz.common_neighbour_features(A, torch.from_numpy(links).to(dev), x, weighting='RA')
    assert tuple(out.shape) == (len(links), F)
    _assert_same(out, want, f'F = {F}')


def test_cn_identity_on_the_unit_matrix(hz, dev, shared):
    """x = ones [N, 1], every stored value 1: the pooled column is CN itself, bit for bit, and the counts are CN too"""
    src, dst, links, n = shared
    A = _matrix(shared, 'unit')
    A.data[:] = 1
    lk = torch.from_numpy(links).to(dev)
    cn = hz.CN(A, lk)[0]
    out = hz.common_neighbour_features(A, lk, torch.ones((n, 1), dtype=torch.float32, device=dev))
    _assert_same(out[:, 0], cn, 'pooled ones against CN')
    lists = hz.common_neighbours(A, lk)
    _assert_same((lists.rowptr[1:] - lists.rowptr[:-1]).to(torch.float32), cn, 'counts against CN')
    _assert_same(cn, hr.scores(A, links, 'CN'), 'CN against scipy')


def test_long_rows_on_both_sides(hz, dev):
    """a power-law graph, links among its 64 largest rows (the shorter row is walked in many chunks, the binary search runs over
    thousands of entries) and uniform ones"""
    n = 20000
    src, dst = hr.powerlaw_graph(n, 200000, 51)
    A = hr.matrix(src, dst, hr.weights('random', src, dst, n, 52), n)
    deg = np.diff(A.indptr)
    big = np.argsort(-deg)[:64]
    rng = np.random.RandomState(53)
    links = np.concatenate([big[rng.randint(0, 64, size=(2000, 2))], rng.randint(0, n, size=(2000, 2))]).astype(np.int64)
    assert np.minimum(deg[links[:2000, 0]], deg[links[:2000, 1]]).max() > 4 * 64 and deg.max() > 2000
    x = np.random.RandomState(54).standard_normal((n, 20)).astype(np.float32)
    lk = torch.from_numpy(links).to(dev)
    for w in ('RA', 'CN'):
        want = cr.lists(A, links, w)
        assert np.diff(want[0])[:2000].max() > 64
        _assert_lists(hz.common_neighbours(A, lk, weighting=w), want, f'powerlaw {w}')
        _assert_same(hz.common_neighbour_features(A, lk, torch.from_numpy(x).to(dev), weighting=w), cr.pool_lists(*want, x),
                     f'powerlaw {w} pooled')
    x128 = np.random.RandomState(55).standard_normal((n, 128)).astype(np.float32)
    _assert_same(hz.common_neighbour_features(A, lk[:2200], torch.from_numpy(x128).to(dev), weighting='AA'),
                 cr.pooled(A, links[:2200], x128, 'AA'), 'powerlaw AA pooled, F = 128')


def test_a_row_has_one_value(hz, dev, shared, features):
    """batch size, the order and repetition of the links, out=, CPU tensors in, and (v, u) for (u, v) on a symmetric unit matrix"""
    src, dst, links, n = shared
    A = _matrix(shared, 'random')
    adj = hz.DeviceAdjacency(A, dev)
    L = len(links)
    lk = torch.from_numpy(links).to(dev)
    x = torch.from_numpy(np.ascontiguousarray(features[:, :20])).to(dev)
    base = hz.common_neighbour_features(adj, lk, x, weighting='AA')
    for bs in (1, 7, 1000, L):
        _assert_same(hz.common_neighbour_features(adj, lk, x, weighting='AA', batch_size=bs), base, f'batch_size {bs}')
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(61)).to(dev)
    _assert_same(hz.common_neighbour_features(adj, lk[perm], x, weighting='AA'), base[perm], 'permuted links')
    rep = lk[35:36].repeat(100, 1)  # the pair of 5000 shared neighbours, the other way round
    assert links[35].tolist() == [35, 34]
    _assert_same(hz.common_neighbour_features(adj, rep, x, weighting='AA'), base[35:36].repeat(100, 1), 'a link 100 times')
    out = torch.full((L, 20), float('nan'), device=dev)
    assert hz.common_neighbour_features(adj, lk, x, weighting='AA', out=out) is out
    _assert_same(out, base, 'out=')
    cpu = hz.common_neighbour_features(A, torch.from_numpy(links), x.cpu(), weighting='AA')
    assert cpu.device.type == 'cpu'
    _assert_same(cpu, base, 'CPU tensors in')
    lists_cpu = hz.common_neighbours(A, torch.from_numpy(links), weighting='AA')
    assert lists_cpu.ids.device.type == 'cpu' and lists_cpu.coef.device.type == 'cpu'
    _assert_lists(lists_cpu, cr.lists(A, links, 'AA'), 'CPU lists')
    S = _matrix(shared, 'unit')
    S = sp.csr_matrix(S + S.T)
    S.data[:] = 1
    fwd = hz.common_neighbour_features(S, lk, x, weighting='RA')
    _assert_same(hz.common_neighbour_features(S, lk.flip(1), x, weighting='RA'), fwd, '(v, u) against (u, v)')
    _assert_same(fwd, cr.pooled(S, links, features[:, :20].copy(), 'RA'), 'symmetric unit matrix')


def _raw(hz, dev):
    from subgraph_sketching_amd import _native
    return _native, _native.lib(), hz._ptr, hz._stream(dev), hz._error_flag(dev)


def test_exact_writes(hz, dev, shared, features):
    """the pool launch writes every row of its slice of a NaN-filled tensor -- the +0.0 rows of links without common neighbours
    too -- and nothing else; the fill launch writes exactly [0, T) between its sentinels"""
    src, dst, links, n = shared
    A = _matrix(shared, 'random')
    adj = hz.DeviceAdjacency(A, dev)
    lk = torch.from_numpy(links).to(dev)
    L, pad = len(links), 1000
    native, lib, ptr, stream, err = _raw(hz, dev)
    mult = adj.multiplier('RA')
    rowptr, ids, coef = cr.lists(A, links, 'RA')
    assert (np.diff(rowptr) == 0).sum() > 100
    for F in (20, 7):  # float4 and scalar stores
        x = np.ascontiguousarray(features[:, :F])
        xd = torch.from_numpy(x).to(dev)
        big = torch.full((L + 2 * pad, F), float('nan'), device=dev)
        native.check(lib.ss_common_neighbour_pool(ptr(adj.rowptr), ptr(adj.col), ptr(adj.val), ptr(mult), n, ptr(lk), L, ptr(xd), F,
                                                  ptr(big[pad:pad + L]), ptr(err), stream), 'pool')
        assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + L:]).all()), F
        _assert_same(big[pad:pad + L], cr.pool_lists(rowptr, ids, coef, x), f'slice, F = {F}')
    T = len(ids)
    counts = torch.full((L + 2,), -7, dtype=torch.int64, device=dev)
    native.check(lib.ss_common_neighbour_count(ptr(adj.rowptr), ptr(adj.col), n, ptr(lk), L, ptr(counts[1:]), ptr(err), stream), 'count')
    assert counts[0].item() == -7 and counts[-1].item() == -7
    _assert_same(counts[1:-1], np.diff(rowptr), 'counts')
    ids_buf = torch.full((T + 2 * pad,), -7, dtype=torch.int64, device=dev)
    coef_buf = torch.full((T + 2 * pad,), float('nan'), device=dev)
    offsets = torch.from_numpy(rowptr[:-1].copy()).to(dev)
    native.check(lib.ss_common_neighbour_fill(ptr(adj.rowptr), ptr(adj.col), ptr(adj.val), ptr(mult), n, ptr(lk), L, ptr(offsets),
                                              ptr(ids_buf[pad:]), ptr(coef_buf[pad:]), ptr(err), stream), 'fill')
    assert bool((ids_buf[:pad] == -7).all()) and bool((ids_buf[pad + T:] == -7).all())
    assert bool(torch.isnan(coef_buf[:pad]).all()) and bool(torch.isnan(coef_buf[pad + T:]).all())
    _assert_same(ids_buf[pad:pad + T], ids, 'ids between the sentinels')
    _assert_same(coef_buf[pad:pad + T], coef, 'coef between the sentinels')
    assert not hz._take_error(dev)


def test_out_of_range_ids(hz, dev, shared, features):
    """N, -1 and 2^40 inside a wavefront of good links: IndexError, their rows zeros, their neighbours' rows right, the next call clean"""
    src, dst, links, n = shared
    A = _matrix(shared, 'random')
    adj = hz.DeviceAdjacency(A, dev)
    good = links[:200].copy()
    bad = good.copy()
    rows = [3, 37, 38, 70, 130, 199]
    bad[3, 0], bad[37, 1], bad[38, 0], bad[70, 1], bad[130] = n, -1, 1 << 40, n + 5, (-1, n)
    bad[199, 1] = -n
    x = np.ascontiguousarray(features[:, :20])
    xd = torch.from_numpy(x).to(dev)
    for F in (20, 3):  # float4 and scalar stores of the zero rows
        xs = np.ascontiguousarray(x[:, :F])
        out = torch.full((200, F), float('nan'), device=dev)
        with pytest.raises(IndexError):
            hz.common_neighbour_features(adj, torch.from_numpy(bad).to(dev), torch.from_numpy(xs).to(dev), weighting='RA', out=out)
        _assert_same(out, _zeroed(cr.pooled(A, good, xs, 'RA'), rows), f'rows around bad ids, F = {F}')
        assert not hz._take_error(dev)
    with pytest.raises(IndexError):
        hz.common_neighbours(adj, torch.from_numpy(bad).to(dev), weighting='RA')
    with pytest.raises(IndexError):
        hz.common_neighbour_features(A, torch.from_numpy(bad), xd.cpu())
    # the launches themselves: count 0 for the bad links, the good ones as ever
    native, lib, ptr, stream, err = _raw(hz, dev)
    counts = torch.full((200,), -7, dtype=torch.int64, device=dev)
    native.check(lib.ss_common_neighbour_count(ptr(adj.rowptr), ptr(adj.col), n, ptr(torch.from_numpy(bad).to(dev)), 200, ptr(counts),
                                               ptr(err), stream), 'count')
    expect = np.diff(cr.lists(A, good, None)[0])
    expect[rows] = 0
    _assert_same(counts, expect, 'counts around bad ids')
    assert hz._take_error(dev) and not hz._take_error(dev)
    _assert_same(hz.common_neighbour_features(adj, torch.from_numpy(good).to(dev), xd, weighting='RA'), cr.pooled(A, good, x, 'RA'),
                 'the call after the error')
    _assert_lists(hz.common_neighbours(adj, torch.from_numpy(good).to(dev), weighting='RA'), cr.lists(A, good, 'RA'), 'lists after the error')


def _zeroed(a, rows):
    a = a.copy()
    a[rows] = 0
    return a


def test_empty_cases(hz, dev, shared, features):
    src, dst, links, n = shared
    A = _matrix(shared, 'random')
    x = torch.from_numpy(np.ascontiguousarray(features[:, :20])).to(dev)
    none = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    out = hz.common_neighbour_features(A, none, x, weighting='RA')
    assert tuple(out.shape) == (0, 20) and out.dtype == torch.float32
    got = hz.common_neighbours(A, none, weighting='RA')
    assert got.rowptr.tolist() == [0] and got.ids.numel() == 0 and got.coef.numel() == 0 and got.coef.dtype == torch.float32
    E = sp.csr_matrix((n, n), dtype=np.float32)  # a matrix without entries
    lk = torch.from_numpy(links[:300]).to(dev)
    for w in ('CN', 'AA', 'RA'):
        out = hz.common_neighbour_features(E, lk, x, weighting=w)
        _assert_same(out, np.zeros((300, 20), dtype=np.float32), f'empty matrix {w}')
    got = hz.common_neighbours(E, lk, weighting='AA')
    assert got.rowptr.tolist() == [0] * 301 and got.ids.numel() == 0 and got.coef.numel() == 0
    iso = torch.tensor([[n - 2, n - 1], [n - 1, n - 1], [n - 1, n - 2]], device=dev)  # T = 0 on a matrix that has entries
    got = hz.common_neighbours(A, iso)
    assert got.rowptr.tolist() == [0, 0, 0, 0] and got.ids.numel() == 0 and got.coef is None
    _assert_same(hz.common_neighbour_features(A, iso, x), np.zeros((3, 20), dtype=np.float32), 'isolated nodes')


# ---- offsets beyond 2 GiB, 4 GiB and 2^31 elements ---------------------------------------------------------------------------------
BIG_N, BIG_F, BIG_L = 4400000, 512, 4200000
BOUNDARY = (1048575, 1048576, 2097151, 2097152, 4194303, 4194304)  # x byte offsets 2 GiB, 4 GiB, element offset 2^31
# x (9.0 GB), out (8.6 GB), the chunks of the fill and of the comparison, + 10 %
BIG_NEEDS = int(1.1 * (BIG_N * BIG_F * 4 + BIG_L * BIG_F * 4 + 3 * (1 << 30)))


def _closed_form(rows, cols):
    """small integers in [-8, 8]: every product and sum of the case is exact in float32"""
    return ((rows[:, None] * 7 + cols[None, :] * 3) % 17 - 8)


def test_large_offsets(hz, dev):
    lt.require_free_memory(dev, BIG_NEEDS, 'common_neighbour_features across 2^31 elements of x and out')
    members = [BOUNDARY, BOUNDARY[:2], BOUNDARY[2:4], BOUNDARY[4:], (BOUNDARY[0], BOUNDARY[5]), (BOUNDARY[1], BOUNDARY[3], BOUNDARY[4]), ()]
    r, c, v = [], [], []
    rng = np.random.RandomState(71)
    for p, ws in enumerate(members):
        for node, own in ((2 * p, 100 + p), (2 * p + 1, BIG_N - 1 - p)):  # + one column of its own on either side
            for w in tuple(ws) + (own,):
                r.append(node), c.append(w), v.append(rng.randint(1, 4))
    A = sp.csr_matrix((np.array(v, dtype=np.float32), (r, c)), shape=(BIG_N, BIG_N))
    pairs = np.stack([np.arange(0, 2 * len(members), 2), np.arange(1, 2 * len(members), 2)], axis=1).astype(np.int64)
    pairs = np.concatenate([pairs, pairs[:3, ::-1]])
    P = len(pairs)
    cols = np.arange(BIG_F, dtype=np.int64)
    want = np.zeros((P, BIG_F), dtype=np.float32)
    for q, (a, b) in enumerate(pairs):
        for w in members[min(a, b) // 2]:
            want[q] += np.float32(A[a, w] * A[b, w]) * _closed_form(np.array([w], dtype=np.int64), cols)[0].astype(np.float32)
    assert np.abs(want).max() < 2 ** 20 and np.abs(want).max() > 0
    x = torch.empty((BIG_N, BIG_F), dtype=torch.float32, device=dev)
    dcols = torch.arange(BIG_F, device=dev)
    for lo in range(0, BIG_N, 400000):
        hi = min(lo + 400000, BIG_N)
        x[lo:hi] = _closed_form(torch.arange(lo, hi, device=dev), dcols).to(torch.float32)
    adj = hz.DeviceAdjacency(A, dev)
    small = hz.common_neighbour_features(adj, torch.from_numpy(pairs).to(dev), x)
    _assert_same(small, want, 'common neighbours at the boundary rows of x')
    lists = hz.common_neighbours(adj, torch.from_numpy(pairs).to(dev), weighting='CN')
    assert lists.ids[:6].tolist() == list(BOUNDARY) and lists.rowptr[1:8].tolist() == [6, 8, 10, 12, 14, 17, 17]
    # out rows beyond 2^31 elements: ONE launch over 4.2 M links that cycle through the planted pairs
    q = torch.arange(BIG_L, device=dev)
    links = torch.from_numpy(pairs).to(dev)[q % P]
    out = torch.empty((BIG_L, BIG_F), dtype=torch.float32, device=dev)
    assert hz.common_neighbour_features(adj, links, x, batch_size=BIG_L, out=out) is out
    wd = torch.from_numpy(want).to(dev).view(torch.int32)
    for lo in range(0, BIG_L, 400000):
        hi = min(lo + 400000, BIG_L)
        assert bool((out[lo:hi].view(torch.int32) == wd[q[lo:hi] % P]).all()), f'rows {lo} .. {hi}'
    del x, out, links, q
    torch.cuda.empty_cache()
