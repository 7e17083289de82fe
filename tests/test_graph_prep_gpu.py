"""coalesce / to_undirected / coalesce_graph / is_undirected on the GPU (csrc/ss_coalesce.hip, graph_prep.py) against the
numpy restatement (graph_prep_restatement.py).  Every comparison is of bits and ids, none of tolerances: pairs, counts, rowptr as whole
integer arrays, values as their bytes.  The planted multigraph (graph_prep_planted.py) is built from the library's own constants
(ss_coalesce_block(), ss_coalesce_chunk()), so its runs meet the workgroup boundaries of the mark / fill passes and the chunk and tier
thresholds of the two reduce kernels wherever those constants put them."""
import functools

import numpy as np
import pytest
import torch

import graph_prep_planted as planted
import graph_prep_restatement as R

pytestmark = pytest.mark.gpu

ORDERS = ('shuffled', 'ascending', 'descending', 'equal')
KINDS = {'float32': 'fractional32', 'float64': 'fractional64', 'int64': 'near2to62'}


def _ssa():
    import subgraph_sketching_amd as ssa
    return ssa


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _constants():
    lib = _ssa()._native.lib()
    return lib.ss_coalesce_block(), lib.ss_coalesce_chunk()


@functools.lru_cache(maxsize=None)
def _list(order):
    """(N, row, col) of a planted list; 'equal': one pair 100 000 times"""
    if order == 'equal':
        return 9, np.full(100000, 7, dtype=np.int64), np.full(100000, 2, dtype=np.int64)
    row, col, _ = planted.edges(*_constants(), order)
    return planted.N, row, col


@functools.lru_cache(maxsize=None)
def _weights(order, kind):
    return planted.weights(len(_list(order)[1]), kind)


@functools.lru_cache(maxsize=None)
def _expected(order, kind, op):
    """the restatement's result, computed once per (list, weights, op) and left unchanged"""
    N, row, col = _list(order)
    out = R.coalesce(row, col, None if kind is None else _weights(order, kind), N, op)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def _ei(order, device=None):
    _, row, col = _list(order)
    return torch.from_numpy(np.stack([row, col])).to(device or _dev())


def _same_bits(t, a):
    got = t.cpu().numpy()
    assert got.dtype == a.dtype and got.shape == a.shape, (got.dtype, a.dtype, got.shape, a.shape)
    if got.tobytes() != a.tobytes():
        bad = [k for k in range(len(a)) if got[k].tobytes() != a[k].tobytes()]
        raise AssertionError(f'{len(bad)} of {len(a)} values differ in their bits, first at {bad[:5]}: {got[bad[:5]]} against {a[bad[:5]]}')


def _check_structure(g, exp, N):
    assert g.edge_index.dtype == torch.int64 and g.count.dtype == torch.int32 and g.rowptr.dtype == torch.int64
    assert np.array_equal(g.edge_index.cpu().numpy(), np.stack([exp['row'], exp['col']]))
    assert np.array_equal(g.count.cpu().numpy(), exp['count'])
    rowptr = g.rowptr.cpu().numpy()
    assert rowptr.shape == (N + 1,) and np.array_equal(rowptr, np.searchsorted(exp['row'], np.arange(N + 1)))
    assert g.num_nodes == N and g.num_edges == len(exp['row'])


@pytest.mark.parametrize('order', ORDERS)
def test_planted_structure_without_values(order):
    ssa = _ssa()
    N, row, col = _list(order)
    exp = _expected(order, None, 'add')
    if order != 'equal':
        assert list(zip(exp['row'], exp['col'], exp['count'])) == planted.plan(*_constants())  # the plan IS the expected output
    g, info = ssa.coalesce_graph(N, _ei(order), return_info=True)
    _check_structure(g, exp, N)
    assert g.edge_weight is None
    assert info == {'runs': len(exp['row']), 'long_runs': 0, 'longest_run': int(exp['count'].max())}
    index, value = ssa.coalesce(_ei(order), None, N, N)
    assert value is None and np.array_equal(index.cpu().numpy(), np.stack([exp['row'], exp['col']]))


@pytest.mark.parametrize('op', R.OPS)
@pytest.mark.parametrize('dtype', sorted(KINDS))
def test_every_dtype_and_op_as_vector_and_column(dtype, op):
    ssa = _ssa()
    kind = KINDS[dtype]
    for order in ('shuffled', 'equal'):
        N = _list(order)[0]
        exp = _expected(order, kind, op)
        w = torch.from_numpy(_weights(order, kind)).to(_dev())
        index, value = ssa.coalesce(_ei(order), w, N, N, op=op)
        assert value.dim() == 1 and value.is_cuda and np.array_equal(index.cpu().numpy(), np.stack([exp['row'], exp['col']]))
        _same_bits(value, exp['value'])
        index, value = ssa.coalesce(_ei(order), w.reshape(-1, 1), N, N, op=op)
        assert value.shape == (len(exp['row']), 1)
        _same_bits(value[:, 0], exp['value'])
        g = ssa.coalesce_graph(N, _ei(order), w.reshape(-1, 1), reduce=op)
        _check_structure(g, exp, N)
        _same_bits(g.edge_weight, exp['value'])


def test_the_sums_depend_on_the_order_and_follow_it():
    """the fractional weights are such that another order gives other bits (so the comparisons above see the order), and the three
    hand-over orders each match their own restatement"""
    ssa = _ssa()
    seen = set()
    for order in ('shuffled', 'ascending', 'descending'):
        N = _list(order)[0]
        exp = _expected(order, 'fractional32', 'add')
        g = ssa.coalesce_graph(N, _ei(order), torch.from_numpy(_weights(order, 'fractional32')).to(_dev()))
        _check_structure(g, exp, N)
        _same_bits(g.edge_weight, exp['value'])
        seen.add(exp['value'].tobytes())
    assert len(seen) == 3
    w = np.array([1.0] + [0.0] * 255 + [2.0 ** -24, 2.0 ** -24], dtype=np.float32)  # 258 entries: the chunk rule, not the plain loop
    ei = torch.zeros((2, 258), dtype=torch.int64, device=_dev())
    _, value = ssa.coalesce(ei, torch.from_numpy(w).to(_dev()), 1, 1)
    assert value.cpu().numpy().tobytes() == (np.float32(1.0) + np.float32(2.0 ** -23)).tobytes() != R.fold_sequential(w, 'add').tobytes()


@pytest.mark.parametrize('op', ['min', 'max'])
@pytest.mark.parametrize('kind', ['special32', 'special64'])
def test_nan_and_signed_zero_rules(kind, op):
    ssa = _ssa()
    N = _list('shuffled')[0]
    exp = _expected('shuffled', kind, op)
    assert np.isnan(exp['value']).any() and not np.isnan(exp['value']).all()
    g = ssa.coalesce_graph(N, _ei('shuffled'), torch.from_numpy(_weights('shuffled', kind)).to(_dev()), reduce=op)
    _same_bits(g.edge_weight, exp['value'])
    # hand-written runs: pair (0, k) holds run k
    dtype = np.float32 if kind.endswith('32') else np.float64
    runs = [[0.0, -0.0], [-0.0, 0.0], [-0.0, 0.0, 0.0, -0.0], [1.0, np.nan, -1.0], [np.nan], [np.nan, 5.0], [2.0, -3.0, 2.0], [0.0, -0.0, -1.0, 1.0]]
    col = np.concatenate([np.full(len(r), k) for k, r in enumerate(runs)])
    w = np.concatenate(runs).astype(dtype)
    p = np.random.RandomState(3).permutation(len(col))  # (the runs interleaved; the restatement folds each in ITS new list order)
    col, w = col[p], w[p]
    expected = R.coalesce(np.zeros_like(col), col, w, 9, op, fold_fn=R.fold_loop)
    _, value = ssa.coalesce(torch.from_numpy(np.stack([np.zeros_like(col), col])).to(_dev()), torch.from_numpy(w).to(_dev()), 9, 9, op=op)
    _same_bits(value, expected['value'])
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        _, value = ssa.coalesce(torch.zeros((2, 2), dtype=torch.int64, device=_dev()), torch.tensor([first, second], dtype=torch.from_numpy(w).dtype,
                                                                                                   device=_dev()), 1, 1, op=op)
        assert bool(np.signbit(value.cpu().numpy()[0])) == bool(np.signbit(first))  # the one listed first wins


def test_int64_mean_is_floor_division_and_sums_wrap():
    ssa = _ssa()
    ei = torch.tensor([[0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 2, 2]], device=_dev())
    w = torch.tensor([-7, 2, 7, -2, (1 << 62) + 5, 1 << 62], device=_dev())
    _, mean = ssa.coalesce(ei, w, 3, 3, op='mean')
    _, add = ssa.coalesce(ei, w, 3, 3, op='add')
    assert mean.tolist()[:2] == [-3, 2] and add.tolist() == [-5, 5, -(1 << 63) + 5]
    assert mean.tolist()[2] == (-(1 << 63) + 5) // 2


@pytest.mark.parametrize('order', ['shuffled', 'equal'])
def test_same_bits_across_long_entries(order):
    """long_entries = 1: every run of two and more entries is the wavefront tier's; 64, 256: mixed; 10^9: the lane tier alone"""
    ssa = _ssa()
    N = _list(order)[0]
    for kind, op in (('fractional32', 'add'), ('fractional64', 'mean'), ('near2to62', 'add'), ('special32', 'min'), ('fractional64', 'max')):
        exp = _expected(order, kind, op)
        w = torch.from_numpy(_weights(order, kind)).to(_dev())
        for long_entries in (1, 64, 256, 10 ** 9):
            g, info = ssa.coalesce_graph(N, _ei(order), w, reduce=op, long_entries=long_entries, return_info=True)
            _check_structure(g, exp, N)
            _same_bits(g.edge_weight, exp['value'])
            assert info['long_runs'] == int((exp['count'] > long_entries).sum()), (long_entries, info)  # MORE than long_entries: 256 is a lane's
            assert info['longest_run'] == int(exp['count'].max())


class _Guarded(object):
    """an output array between two runs of guard words, all preset to a sentinel"""
    GUARD = 64

    def __init__(self, n, dtype, sentinel):
        self.n, self.sentinel = n, sentinel
        self.whole = torch.full((n + 2 * self.GUARD,), sentinel, dtype=dtype, device=_dev())
        self.own = self.whole[self.GUARD:self.GUARD + n]

    def ptr(self):
        from ctypes import c_void_p
        return c_void_p(self.own.data_ptr())

    def guards_untouched(self):
        w = self.whole.cpu().numpy()
        s = np.array(self.sentinel, dtype=w.dtype)
        return bool((w[:self.GUARD] == s).all() and (w[self.GUARD + self.n:] == s).all())

    def numpy(self):
        return self.own.cpu().numpy()


def _launch_all(lib, row, col, perm, value, N, n_runs_expected, long_entries):
    """mark, cumsum, fill, reduce, reduce_long by hand into guarded outputs; -> dict of _Guarded and the intermediate reads"""
    from ctypes import c_void_p
    ptr = lambda t: c_void_p(t.data_ptr())
    block, _ = _constants()
    E = len(row)
    d_row, d_col, d_perm = (torch.from_numpy(a).to(_dev()) for a in (row, col, perm.astype(np.int32)))
    d_value = torch.from_numpy(value).to(_dev())
    heads = _Guarded((E + block - 1) // block, torch.int32, -7)
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    assert lib.ss_coalesce_mark(ptr(d_row), ptr(d_col), ptr(d_perm), E, N, heads.ptr(), ptr(err), None) == 0
    incl = torch.cumsum(heads.own, 0, dtype=torch.int64)
    n_runs = int(incl[-1])
    out = dict(heads=heads, err=int(err.item()), n_runs=n_runs)
    if n_runs_expected is not None:
        assert n_runs == n_runs_expected
    out['row'], out['col'] = _Guarded(n_runs, torch.int64, -99), _Guarded(n_runs, torch.int64, -99)
    out['run_start'], out['rowptr'] = _Guarded(n_runs + 1, torch.int32, -99), _Guarded(N + 1, torch.int64, -99)
    assert lib.ss_coalesce_fill(ptr(d_row), ptr(d_col), ptr(d_perm), E, N, ptr(incl), n_runs, out['row'].ptr(), out['col'].ptr(),
                                out['run_start'].ptr(), out['rowptr'].ptr(), None) == 0
    torch.cuda.synchronize()
    if out['err']:
        return out
    max_long = E // long_entries + 1
    out['value'], out['count'] = _Guarded(n_runs, d_value.dtype, -12345.0), _Guarded(n_runs, torch.int32, -99)
    out['long_runs'] = _Guarded(max_long, torch.int32, -99)
    info = torch.full((2,), 77, dtype=torch.int32, device=_dev())  # (cleared by the call)
    assert lib.ss_coalesce_reduce(ptr(d_perm), out['run_start'].ptr(), n_runs, ptr(d_value), E, 1, 0, long_entries, out['value'].ptr(),
                                  out['count'].ptr(), out['long_runs'].ptr(), max_long, ptr(info), None) == 0
    out['value_after_reduce'], out['info'] = out['value'].numpy().copy(), info.tolist()
    assert lib.ss_coalesce_reduce_long(ptr(d_perm), out['run_start'].ptr(), n_runs, ptr(d_value), E, 1, 0, out['value'].ptr(),
                                       out['long_runs'].ptr(), ptr(info), max_long, None) == 0
    torch.cuda.synchronize()
    return out


def test_direct_launches_write_their_own_places_and_nothing_else():
    lib = _ssa()._native.lib()
    block, chunk = _constants()
    N, row, col = _list('shuffled')
    w = _weights('shuffled', 'fractional32')
    exp = _expected('shuffled', 'fractional32', 'add')
    n_runs = len(exp['row'])
    is_long = exp['count'] > chunk
    for attempt in range(2):  # twice: the same places, the same bits
        got = _launch_all(lib, row, col, exp['perm'], w, N, n_runs, long_entries=chunk)
        assert got['err'] == 0
        assert np.array_equal(got['heads'].numpy(), np.bincount(exp['starts'][:-1] // block, minlength=got['heads'].n))
        assert np.array_equal(got['row'].numpy(), exp['row']) and np.array_equal(got['col'].numpy(), exp['col'])
        assert np.array_equal(got['run_start'].numpy(), exp['starts'])
        assert np.array_equal(got['rowptr'].numpy(), exp['rowptr'])
        assert np.array_equal(got['count'].numpy(), exp['count'])
        assert got['info'] == [int(is_long.sum()), int(exp['count'].max())]
        listed = got['long_runs'].numpy()
        assert sorted(listed[:got['info'][0]].tolist()) == np.flatnonzero(is_long).tolist() and (listed[got['info'][0]:] == -99).all()
        # the lane tier wrote its own slots and left the listed ones alone; the wavefront tier then wrote exactly those
        after = got['value_after_reduce']
        assert (after[is_long] == np.float32(-12345.0)).all()
        assert after[~is_long].tobytes() == exp['value'][~is_long].tobytes()
        assert got['value'].numpy().tobytes() == exp['value'].tobytes()
        for name in ('heads', 'row', 'col', 'run_start', 'rowptr', 'value', 'count', 'long_runs'):
            assert got[name].guards_untouched(), name


def test_ids_out_of_range_raise_and_store_nothing_past_the_outputs():
    ssa = _ssa()
    lib = ssa._native.lib()
    N, row, col = _list('shuffled')
    for where, bad in ((row, N), (col, N), (row, -1), (col, -N), (row, 1 << 40), (col, -(1 << 40))):
        ei = np.stack([row, col])
        ei[0 if where is row else 1, 3000 + 37] = bad  # one bad id inside a wavefront of good ones
        for device in (_dev(), torch.device('cpu')):
            with pytest.raises(IndexError):
                ssa.coalesce(torch.from_numpy(ei).to(device), None, N, N)
        with pytest.raises(IndexError):
            ssa.to_undirected(torch.from_numpy(ei).to(_dev()), torch.ones(ei.shape[1], device=_dev()), num_nodes=N)
        # the kernels themselves, on whatever order a sort of such a list gives: the flag is set, the guards stay
        got = _launch_all(lib, ei[0], ei[1], R.sorted_positions(ei[0], ei[1]), _weights('shuffled', 'fractional32'), N, None, 256)
        assert got['err'] == 1
        for name in ('heads', 'row', 'col', 'run_start', 'rowptr'):
            assert got[name].guards_untouched(), (name, bad)
    assert ssa.coalesce(torch.from_numpy(np.stack([row, col])).to(_dev()), None, N, N)[0].size(1) == len(_expected('shuffled', None, 'add')['row'])


def test_cpu_tensors_in_cpu_tensors_out_and_repeatable():
    ssa = _ssa()
    N = _list('shuffled')[0]
    exp = _expected('shuffled', 'fractional64', 'add')
    w = torch.from_numpy(_weights('shuffled', 'fractional64'))
    ei = _ei('shuffled', torch.device('cpu'))
    first = ssa.coalesce(ei, w, N, N)
    second = ssa.coalesce(ei.to(_dev()), w.to(_dev()), N, N)
    assert not first[0].is_cuda and not first[1].is_cuda and second[0].is_cuda and second[1].is_cuda
    _same_bits(first[1], exp['value'])
    assert torch.equal(first[0], second[0].cpu()) and first[1].numpy().tobytes() == second[1].cpu().numpy().tobytes()
    g = ssa.coalesce_graph(N, ei, w)
    assert not g.edge_index.is_cuda and not g.edge_weight.is_cuda and not g.count.is_cuda and not g.rowptr.is_cuda
    assert g.is_symmetric() is False
    und = ssa.to_undirected(ei, w, N)
    assert not und[0].is_cuda and not und[1].is_cuda
    assert und[1].numpy().tobytes() == ssa.to_undirected(ei, w, N)[1].numpy().tobytes()


def test_to_undirected_hand_written_and_planted():
    ssa = _ssa()
    ei = torch.tensor([[0, 1, 2, 2, 4, 5], [1, 0, 3, 3, 4, 0]], device=_dev())
    w = torch.tensor([1.5, 2.0, 0.25, 0.5, 3.0, 7.0], device=_dev())
    index, value = ssa.to_undirected(ei, w)  # num_nodes: max + 1 = 6
    assert index.tolist() == [[0, 0, 1, 2, 3, 4, 5], [1, 5, 0, 3, 2, 4, 0]] and value.tolist() == [3.5, 7.0, 3.5, 0.75, 0.75, 6.0, 7.0]
    assert ssa.to_undirected(ei).tolist() == index.tolist()
    index, value = ssa.to_undirected(ei, w.reshape(-1, 1).double(), 9, reduce='mean')
    assert value.dtype == torch.float64 and value.shape == (7, 1) and value[:, 0].tolist() == [1.75, 7.0, 1.75, 0.375, 0.375, 3.0, 7.0]
    assert not ssa.is_undirected(ei, w) and ssa.is_undirected(index, value)
    for kind, op in (('fractional32', 'add'), ('near2to62', 'add'), ('fractional64', 'min')):
        N, row, col = _list('shuffled')
        wn = _weights('shuffled', kind)
        exp = R.to_undirected(row, col, wn, N, op)
        index, value = ssa.to_undirected(_ei('shuffled'), torch.from_numpy(wn).to(_dev()), N, reduce=op)
        assert np.array_equal(index.cpu().numpy(), np.stack([exp['row'], exp['col']]))
        _same_bits(value, exp['value'])
        g = ssa.coalesce_graph(N, _ei('shuffled'), torch.from_numpy(wn).to(_dev()), reduce=op, symmetrize=True)
        _same_bits(g.edge_weight, exp['value'])
        assert np.array_equal(g.count.cpu().numpy(), exp['count']) and g.is_symmetric(weights=False)
        assert g.is_symmetric() == R.is_symmetric(exp)


def test_symmetry_words():
    ssa = _ssa()
    n = 6645
    a = np.arange(n - 1, dtype=np.int64)
    arcs = np.concatenate([np.stack([a, a + 1]), np.stack([a + 1, a])], axis=1)  # a path: 13 288 arcs
    assert arcs.shape[1] == 13288
    arcs = arcs[:, np.random.RandomState(1).permutation(arcs.shape[1])]
    w = (1.0 + (arcs.min(0) % 17)).astype(np.float32)  # one weight per undirected edge
    dev = _dev()
    t, tw = torch.from_numpy(arcs).to(dev), torch.from_numpy(w).to(dev)
    assert ssa.is_undirected(t) and ssa.is_undirected(t, tw, n) and ssa.coalesce_graph(n, t, tw).is_symmetric()
    for missing in (0, 5000, 13287):  # one arc of 13 288 missing
        keep = np.ones(13288, dtype=bool)
        keep[missing] = False
        assert not ssa.is_undirected(t[:, keep]) and not ssa.is_undirected(t[:, keep], tw[keep])
        assert ssa.is_undirected(ssa.to_undirected(t[:, keep], num_nodes=n))
    skew = tw.clone()
    skew[777] += 0.5  # symmetric in structure, not in weights
    g = ssa.coalesce_graph(n, t, skew)
    assert g.is_symmetric(weights=False) and not g.is_symmetric() and not ssa.is_undirected(t, skew)
    assert not ssa.is_undirected(torch.tensor([[0, 1], [1, 2]], device=dev))  # directed
    assert ssa.is_undirected(torch.tensor([[3], [3]], device=dev))           # a self loop is its own reverse
    nan = torch.tensor([float('nan'), float('nan')], device=dev)
    assert ssa.is_undirected(torch.tensor([[0, 1], [1, 0]], device=dev), nan)  # NaN equals NaN here


def test_empty_single_and_one_node():
    ssa = _ssa()
    dev = _dev()
    empty = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    g, info = ssa.coalesce_graph(5, empty, torch.zeros(0, device=dev), return_info=True)
    assert g.edge_index.shape == (2, 0) and g.edge_weight.shape == (0,) and g.count.shape == (0,) and g.rowptr.tolist() == [0] * 6
    assert info == {'runs': 0, 'long_runs': 0, 'longest_run': 0} and g.is_symmetric() and g.to_scipy().nnz == 0
    assert ssa.to_undirected(empty).shape == (2, 0) and ssa.is_undirected(empty)
    index, value = ssa.coalesce(empty, torch.zeros((0, 1), dtype=torch.int64, device=dev), 4, 4)
    assert index.shape == (2, 0) and value.shape == (0, 1) and value.dtype == torch.int64
    one = torch.tensor([[2], [0]], device=dev)
    g = ssa.coalesce_graph(3, one, torch.tensor([4.5], device=dev))
    assert g.edge_index.tolist() == [[2], [0]] and g.edge_weight.tolist() == [4.5] and g.count.tolist() == [1] and g.rowptr.tolist() == [0, 0, 0, 1]
    assert ssa.to_undirected(one).tolist() == [[0, 2], [2, 0]]
    loops = torch.zeros((2, 5), dtype=torch.int64, device=dev)  # N = 1: only self loops exist
    g = ssa.coalesce_graph(1, loops, torch.arange(5, device=dev))
    assert g.edge_index.tolist() == [[0], [0]] and g.edge_weight.tolist() == [10] and g.count.tolist() == [5] and g.rowptr.tolist() == [0, 1]
    index, value = ssa.to_undirected(loops, torch.arange(5, device=dev))
    assert index.tolist() == [[0], [0]] and value.tolist() == [20]  # a self loop meets its own copy


def test_round_trip_to_scipy():
    import scipy.sparse as ssp
    ssa = _ssa()
    N, row, col = _list('shuffled')
    w = _weights('shuffled', 'small_int')
    g = ssa.coalesce_graph(N, _ei('shuffled'), torch.from_numpy(w).to(_dev()))
    A = g.to_scipy()
    assert A.has_canonical_format and A.has_sorted_indices and A.shape == (N, N)
    ones = ssp.coo_matrix((np.ones_like(w), (row, col)), shape=(N, N)).tocsr()  # scipy's own sums; structure from unit entries
    ones.sum_duplicates()
    own = ssp.coo_matrix((w, (row, col)), shape=(N, N)).tocsr()
    own.sum_duplicates()
    assert np.array_equal(A.indptr, ones.indptr) and np.array_equal(A.indices, ones.indices)
    assert (A != own).nnz == 0 and np.array_equal(A.toarray(), own.toarray())
    C = ssa.coalesce_graph(N, _ei('shuffled')).to_scipy()
    assert np.array_equal(C.data, ones.data) and C.has_canonical_format
    B = A.copy()
    B.sum_duplicates()  # nothing to do on a canonical matrix
    assert np.array_equal(B.data, A.data) and np.array_equal(B.indices, A.indices)


def test_rows_beyond_the_4_gib_offset():
    """E = 2^29 + 4 099 edges: each row of edge_index (and the int64 weights) crosses the 4 GiB byte offset; N = 2^20.  Structure and sums
    against a blocked torch restatement: torch.unique of row * N + col (no overflow at this N), four row ranges one after the other."""
    ssa = _ssa()
    dev = _dev()
    E, N = (1 << 29) + 4099, 1 << 20
    gen = torch.Generator(device=dev).manual_seed(11)
    ei = torch.empty((2, E), dtype=torch.int64, device=dev)
    ei[0].random_(0, N, generator=gen)
    ei[1].random_(0, 64, generator=gen)
    ei[1].add_(ei[0] * 7).remainder_(N)  # 64 columns per row: runs of eight entries on average
    w = torch.empty(E, dtype=torch.int64, device=dev).random_(-5, 6, generator=gen)
    assert ei[0].numel() * 8 > 1 << 32
    g = ssa.coalesce_graph(N, ei, w)
    assert int(g.count.sum(dtype=torch.int64)) == E and int(g.rowptr[-1]) == g.num_edges and int(g.rowptr[0]) == 0
    keys = g.edge_index[0] * N + g.edge_index[1]
    assert bool((keys[1:] > keys[:-1]).all())  # sorted by (row, col), every pair once
    assert torch.equal(g.rowptr, torch.searchsorted(g.edge_index[0].contiguous(), torch.arange(N + 1, device=dev)))
    quarter = N // 4
    for b in range(4):
        sel = (ei[0] >= b * quarter) & (ei[0] < (b + 1) * quarter)
        uniq, inverse, counts = torch.unique(ei[0][sel] * N + ei[1][sel], return_inverse=True, return_counts=True)
        sums = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).scatter_add_(0, inverse, w[sel])  # (integer atomics: exact)
        lo, hi = int(g.rowptr[b * quarter]), int(g.rowptr[(b + 1) * quarter])
        assert torch.equal(keys[lo:hi], uniq) and torch.equal(g.count[lo:hi].to(torch.int64), counts) and torch.equal(g.edge_weight[lo:hi], sums)
        del sel, uniq, inverse, counts, sums
