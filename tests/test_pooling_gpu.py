"""pooling.global_sort_pool / global_add_pool / global_mean_pool / center_pool (csrc/ss_pool.hip) on the GPU against their restatement
(tests/pooling_restatement.py, pinned to torch and float64 by tests/test_pooling_host.py).  Every comparison is of BITS: the order is
an integer order on distinct keys, a sum is accumulated by one lane in ascending row order, a gradient row has one writer -- each
output has exactly one right value."""
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

import large_table_helpers as lt
import pooling_restatement as pr

pytestmark = pytest.mark.gpu

C = pr.C
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5)  # both tiers of the select and their boundary; the last two are large
ROWPTR = pr.sizes_to_rowptr(SIZES)
T, L = int(ROWPTR[-1]), len(SIZES)
WIDTHS = (0, 1, 3, 4, 20, 64, 260)  # empty; scalar lanes 1 and 4; float4 lane groups of 1, 8 (5 pieces), 16, 64 + a second pass
KS = (1, 2, 64, 65, C)              # n < k, n == k and n > k occur in both tiers (k = C against n = C - 1, C, C + 1, 3C + 5)
KINDS = ('random', 'equal', 'straddle', 'special', 'ascending', 'descending')
BASE = pr.features(T, 260, seed=1)
SENTINEL = 0x7FC0BEEF  # a NaN no kernel produces


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f'{what}: {tuple(g.shape)} against {tuple(w.shape)}'
    bad = torch.nonzero(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} of {g.numel()} elements differ, first at {bad[:4].tolist()}'


def key_column(kind, k, sizes=SIZES, seed=7):
    """the last channel of every graph, by kind"""
    rng = np.random.RandomState(seed)
    total = int(np.sum(sizes))
    distinct = ((rng.permutation(total).astype(np.float32) - total / 2) / 8).astype(np.float32)
    out, at = [], 0
    for n in sizes:
        v = distinct[at:at + n].copy()
        at += n
        if kind == 'equal':
            v[:] = 2.5
        elif kind == 'straddle' and n:  # the keys ranked k - 3 .. k + 5 all take the value of rank k - 3: a run of ties across position k
            o = np.argsort(-v, kind='stable')
            run = o[max(0, min(k - 3, n - 1)):k + 6]
            v[run] = v[run[0]]
        elif kind == 'special' and n:
            pick = rng.randint(0, n, size=max(1, n // 3))
            v[pick] = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.5, -1.5], dtype=np.float32), size=len(pick))
            v[rng.randint(0, n)] = np.array([0xFFC00123], dtype=np.uint32).view(np.float32)[0]  # a negative NaN with a payload
        elif kind == 'ascending':
            v = (np.arange(n) * 0.25).astype(np.float32)
        elif kind == 'descending':
            v = (-np.arange(n) * 0.25).astype(np.float32)
        out.append(v)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.float32)


def planted(F, kind='random', k=1):
    x = BASE[:, :F].copy()
    if F:
        x[:, -1] = key_column(kind, k)
    return x


def sparse_like(g, rows):
    s = np.zeros_like(g)
    s[rows] = g[rows]
    return s


@pytest.fixture(scope='module')
def rowptr(dev):
    return torch.from_numpy(ROWPTR).to(dev)


# ---- sort pool ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('F', WIDTHS)
def test_sort_pool_forward_and_backward_bits(ssa, dev, rowptr, F, k):
    x = planted(F)
    want, want_perm = pr.sort_pool(x, ROWPTR, k)
    tx = torch.from_numpy(x).to(dev).requires_grad_(True)
    y, perm = ssa.global_sort_pool(tx, None, k, rowptr=rowptr, return_perm=True)
    assert y.shape == (L, k * F) and y.dtype == torch.float32 and perm.shape == (L, k) and perm.dtype == torch.int32 and not perm.requires_grad
    assert np.array_equal(perm.cpu().numpy(), want_perm), f'perm F={F} k={k}'
    _assert_same(y, want, f'sort pool F={F} k={k}')
    for q, n in enumerate(SIZES):  # the -1 padding and the zero slots
        assert (want_perm[q, min(n, k):] == -1).all() and (want_perm[q, :min(n, k)] >= 0).all()
        assert not _bits(y[q, min(n, k) * F:]).any()
    g = np.random.RandomState(k + F).standard_normal((L, k * F + 3)).astype(np.float32)[:, :k * F]
    for name, gg in (('dense', g), ('sparse', sparse_like(g, [2, 9, 12]))):
        tg = torch.from_numpy(np.ascontiguousarray(gg)).to(dev)
        first, = torch.autograd.grad(y, tx, tg, retain_graph=True)
        assert first.shape == (T, F)
        _assert_same(first, pr.sort_pool_backward(gg, ROWPTR, want_perm, T), f'sort pool x.grad ({name}) F={F} k={k}')
        second, = torch.autograd.grad(y, tx, tg, retain_graph=True)
        _assert_same(second, first, 'second backward')
    y2 = ssa.global_sort_pool(tx.detach(), None, k, rowptr=rowptr)
    _assert_same(y2, y, 'second forward')
    assert not y2.requires_grad
    ssa.pooling.check_errors()


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('kind', KINDS)
def test_orders_in_both_tiers(ssa, dev, rowptr, kind, k):
    for F in (1, 4):
        x = planted(F, kind, k)
        want, want_perm = pr.sort_pool(x, ROWPTR, k)
        y, perm = ssa.global_sort_pool(torch.from_numpy(x).to(dev), None, k, rowptr=rowptr, return_perm=True)
        got = perm.cpu().numpy()
        bad = np.nonzero((got != want_perm).any(1))[0]
        assert len(bad) == 0, f'{kind} k={k} F={F}: perm differs in graphs of n = {[SIZES[q] for q in bad]}'
        _assert_same(y, want, f'{kind} k={k} F={F}')


@pytest.mark.parametrize('kind', ('random', 'special', 'equal'))
def test_a_row_of_perm_depends_on_its_graph_alone(ssa, dev, rowptr, kind):
    """the same graphs in another batch order, among other neighbours, under another L"""
    k = 64
    x = planted(3, kind, k)
    base = ssa.global_sort_pool(torch.from_numpy(x).to(dev), None, k, rowptr=rowptr, return_perm=True)[1].cpu().numpy()
    for order in (list(range(L))[::-1], [12, 3, 11, 0, 5], [9], [10, 12, 12, 10, 1]):
        xs = np.concatenate([x[ROWPTR[q]:ROWPTR[q + 1]] for q in order])
        rp = torch.from_numpy(pr.sizes_to_rowptr([SIZES[q] for q in order])).to(dev)
        got = ssa.global_sort_pool(torch.from_numpy(xs).to(dev), None, k, rowptr=rp, return_perm=True)[1].cpu().numpy()
        assert np.array_equal(got, base[order]), order


def test_sort_and_center_gradients_equal_torch_autograd(ssa, dev, rowptr):
    """on tie-free keys: forward and x.grad through the torch composition a user writes today (dense batch + sort + gather;
    x[a] * x[b]) -- bit for bit"""
    sizes = [n for n in SIZES if n]  # (the torch restatement is called with every graph non-empty, as PyG's batches are)
    rp = pr.sizes_to_rowptr(sizes)
    keep = np.concatenate([np.arange(ROWPTR[q], ROWPTR[q + 1]) for q, n in enumerate(SIZES) if n])
    batch = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes)).to(dev)
    for F, k in ((20, 65), (3, C)):
        x = torch.from_numpy(planted(F)[keep]).to(dev)
        g = torch.from_numpy(np.random.RandomState(F).standard_normal((len(sizes), k * F)).astype(np.float32)).to(dev)
        a = x.clone().requires_grad_(True)
        ya = ssa.global_sort_pool(a, batch, k)
        b = x.clone().requires_grad_(True)
        yb = pr.torch_sort_pool(b, batch, k)
        _assert_same(ya, yb, f'sort pool against torch F={F} k={k}')
        ga, = torch.autograd.grad(ya, a, g)
        gb, = torch.autograd.grad(yb, b, g)
        _assert_same(ga, gb, f'sort pool x.grad against torch autograd F={F} k={k}')
    F = 20
    roots = np.array([[0, 0]] + [[(5 * q) % n, (n - 1 - q) % n] for q, n in enumerate(sizes[1:], 1)], dtype=np.int32)
    roots[1] = (1, 1)  # a second self link
    sg = ssa.ExactSubgraphs(torch.from_numpy(rp).to(dev), None, None, torch.from_numpy(roots).to(dev), None, None, None, None, None)
    x = torch.from_numpy(planted(F)[keep]).to(dev)
    g = torch.from_numpy(np.random.RandomState(2).standard_normal((len(sizes), F)).astype(np.float32)).to(dev)
    a = x.clone().requires_grad_(True)
    ya = ssa.center_pool(a, sg)
    b = x.clone().requires_grad_(True)
    ia, ib = (torch.from_numpy(rp[:-1] + roots[:, j]).to(dev) for j in (0, 1))
    yb = b[ia] * b[ib]
    _assert_same(ya, yb, 'centre pool against torch')
    _assert_same(torch.autograd.grad(ya, a, g)[0], torch.autograd.grad(yb, b, g)[0], 'centre pool x.grad against torch autograd')


# ---- add and mean pool --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('F', WIDTHS)
def test_segment_pools_forward_and_backward_bits(ssa, dev, rowptr, F):
    x = planted(F)
    tx = torch.from_numpy(x).to(dev).requires_grad_(True)
    g = np.random.RandomState(F).standard_normal((L, F + 1)).astype(np.float32)[:, :F]
    for mean, fn in ((False, ssa.global_add_pool), (True, ssa.global_mean_pool)):
        y = fn(tx, rowptr=rowptr)
        assert y.shape == (L, F) and y.dtype == torch.float32
        _assert_same(y, pr.segment_pool(x, ROWPTR, mean), f'mean={mean} F={F}')
        assert not _bits(y[0]).any()  # an empty graph gives +0.0
        for name, gg in (('dense', g), ('sparse', sparse_like(g, [1, 6, 12]))):
            tg = torch.from_numpy(gg).to(dev)  # (a non-contiguous grad_out)
            first, = torch.autograd.grad(y, tx, tg, retain_graph=True)
            _assert_same(first, pr.segment_pool_backward(gg, ROWPTR, T, mean), f'mean={mean} F={F} x.grad ({name})')
            second, = torch.autograd.grad(y, tx, tg, retain_graph=True)
            _assert_same(second, first, 'second backward')
        _assert_same(fn(tx.detach(), rowptr=rowptr), y, 'second forward')
    ssa.pooling.check_errors()


def test_inputs_batch_vector_rowptr_size_and_subgraphs(ssa, dev, rowptr):
    F, k = 20, 64
    x = torch.from_numpy(planted(F)).to(dev)
    batch = torch.from_numpy(np.repeat(np.arange(L), SIZES)).to(dev)
    want = {'add': ssa.global_add_pool(x, rowptr=rowptr), 'mean': ssa.global_mean_pool(x, rowptr=rowptr),
            'sort': ssa.global_sort_pool(x, None, k, rowptr=rowptr)}
    sg = ssa.ExactSubgraphs(rowptr, None, None, None, None, None, None, None, None)
    for b, kw, graphs in ((batch, {}, L), (batch, {'size': L}, L), (batch, {'size': L + 3}, L + 3), (sg, {}, L), (sg, {'size': L}, L)):
        got = {'add': ssa.global_add_pool(x, b, **kw), 'mean': ssa.global_mean_pool(x, b, **kw), 'sort': ssa.global_sort_pool(x, b, k, **kw)}
        for name in want:
            assert got[name].shape[0] == graphs
            _assert_same(got[name][:L], want[name], f'{name} {type(b).__name__} {kw}')
            assert not _bits(got[name][L:]).any()  # trailing empty graphs
    # a batch vector whose first graphs are empty (ids start at 2) and one that decreases
    shifted = ssa.global_add_pool(x, batch + 2)
    assert shifted.shape[0] == L + 2 and not _bits(shifted[:2]).any()
    _assert_same(shifted[2:], want['add'], 'ids from 2')
    with pytest.raises(ValueError):
        ssa.global_add_pool(x, batch.flip(0))
    with pytest.raises(ValueError):
        ssa.global_sort_pool(x, batch, k, rowptr=rowptr)
    with pytest.raises(ValueError):
        ssa.global_add_pool(x, batch.cpu())
    with pytest.raises(ValueError):
        ssa.global_add_pool(x, sg, size=L + 1)
    with pytest.raises(ValueError):
        ssa.global_sort_pool(x, sg, C + 1)
    empty = ssa.global_sort_pool(x[:0], rowptr=torch.zeros(1, dtype=torch.int64, device=dev), k=3)
    assert empty.shape == (0, 3 * F) and ssa.global_add_pool(x[:0], batch[:0]).shape == (0, F)
    y = ssa.global_add_pool(x.t().contiguous().t(), rowptr=rowptr)  # a non-contiguous x is copied, not refused
    _assert_same(y, want['add'], 'non-contiguous x')
    with torch.no_grad():
        assert not ssa.global_mean_pool(x.clone().requires_grad_(True), rowptr=rowptr).requires_grad
    ssa.pooling.check_errors()


# ---- centre pool --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('F', WIDTHS)
def test_center_pool_bits(ssa, dev, rowptr, F):
    """roots at the first, last and inner positions of their rows, (-1, -1) rows, self links"""
    roots = np.array([[-1, -1], [0, 0], [1, 0], [0, 62], [63, 63], [31, 64], [-1, -1], [255, 0], [128, 129], [C - 2, 0], [C - 1, C - 1], [C, 1],
                      [3 * C + 4, 0]], dtype=np.int32)
    x = planted(F)
    tx = torch.from_numpy(x).to(dev).requires_grad_(True)
    sg = ssa.ExactSubgraphs(rowptr, None, None, torch.from_numpy(roots).to(dev), None, None, None, None, None)
    y = ssa.center_pool(tx, sg)
    assert y.shape == (L, F)
    _assert_same(y, pr.center_pool(x, ROWPTR, roots), f'centre pool F={F}')
    assert not _bits(y[[0, 6]]).any()
    g = np.random.RandomState(F).standard_normal((L, F)).astype(np.float32)
    for name, gg in (('dense', g), ('sparse', sparse_like(g, [1, 4, 11]))):
        tg = torch.from_numpy(gg).to(dev)
        first, = torch.autograd.grad(y, tx, tg, retain_graph=True)
        _assert_same(first, pr.center_pool_backward(x, gg, ROWPTR, roots), f'centre pool x.grad ({name}) F={F}')
        second, = torch.autograd.grad(y, tx, tg, retain_graph=True)
        _assert_same(second, first, 'second backward')
    ssa.pooling.check_errors()


def test_center_pool_on_real_subgraphs(ssa, dev):
    """roots of a real exact_subgraphs batch: NOT at local indices 0 and 1 (rows ascend by id); the result equals indexing with
    rowptr[:-1] + roots, and the whole pipeline's readouts run on the batch"""
    n = 300
    rng = np.random.RandomState(11)
    e = rng.randint(0, n, size=(2, 900)).astype(np.int64)
    ei = torch.from_numpy(np.concatenate([e, e[::-1]], axis=1)).to(dev)
    links = torch.from_numpy(np.concatenate([e[:, :40].T, [[7, 7], [0, n - 1]]]).astype(np.int64)).to(dev)
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    sg = eh.exact_subgraphs(links, n, ei)
    roots, rp = sg.roots.cpu().numpy(), sg.rowptr.cpu().numpy()
    assert (roots >= 0).all() and not np.array_equal(roots[:, 0], np.zeros(len(roots))) and (roots[40, 0] == roots[40, 1])
    ids = sg.ids.cpu().numpy()
    assert np.array_equal(ids[rp[:-1] + roots[:, 0]], links[:, 0].cpu().numpy()) and np.array_equal(ids[rp[:-1] + roots[:, 1]], links[:, 1].cpu().numpy())
    x = torch.from_numpy(pr.features(len(ids), 20, seed=5)).to(dev)
    y = ssa.center_pool(x, sg)
    ia, ib = (sg.rowptr[:-1] + sg.roots[:, j].to(torch.int64) for j in (0, 1))
    _assert_same(y, x[ia] * x[ib], 'centre pool on exact_subgraphs')
    k = ssa.sort_pool_k(sg)
    assert k == pr.sort_pool_k(np.diff(rp).tolist()) <= C
    want, want_perm = pr.sort_pool(x.cpu().numpy(), rp, k)
    out, perm = ssa.global_sort_pool(x, sg, k, return_perm=True)
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    _assert_same(out, want, 'sort pool on exact_subgraphs')
    _assert_same(ssa.global_add_pool(x, sg), ssa.global_add_pool(x, sg.batch()), 'ExactSubgraphs against its batch vector')
    _assert_same(ssa.global_mean_pool(x, sg), pr.segment_pool(x.cpu().numpy(), rp, True), 'mean pool on exact_subgraphs')
    ssa.pooling.check_errors()


# ---- direct launches into guarded arrays --------------------------------------------------------------------------------------------

def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(rows, F, dev, guard=67):
    """a sentinel-filled int32 buffer [guard + rows + guard, F] and the address of row `guard`"""
    buf = torch.full(((rows + 2 * guard) * max(F, 1),), SENTINEL, dtype=torch.int32, device=dev)
    return buf, ctypes.c_void_p(buf.data_ptr() + guard * F * 4), guard * F


def _check_guarded(buf, first, want, what):
    got = buf.cpu()
    n = want.size
    assert torch.all(got[:first] == SENTINEL) and torch.all(got[first + n:] == SENTINEL), f'{what}: a guard row was written'
    g, w = got[first:first + n], torch.from_numpy(np.ascontiguousarray(want).reshape(-1).view(np.int32))
    bad = torch.nonzero(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} of {n} places differ, first at {bad[:4].tolist()}'


@pytest.mark.parametrize('F', [1, 4, 20, 260])
def test_direct_launches_write_their_own_places_exactly(ssa, dev, rowptr, F):
    lib, k = ssa._native.lib(), 65
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    x = planted(F)
    tx = torch.from_numpy(x).to(dev)
    want, want_perm = pr.sort_pool(x, ROWPTR, k)
    # select: exactly L * k words of perm
    buf, at, first = _guarded(L, k, dev)
    assert lib.ss_pool_select(_p(rowptr), L, _p(tx), T, F, k, at, _p(err), stream) == 0
    _check_guarded(buf, first, want_perm, 'select')
    perm = torch.from_numpy(want_perm).to(dev)
    # gather: every place of out, zeros included
    buf, at, first = _guarded(L, k * F, dev)
    assert lib.ss_pool_gather(_p(rowptr), L, _p(perm), k, _p(tx), T, F, at, _p(err), stream) == 0
    _check_guarded(buf, first, want, 'gather')
    # scatter: every row of grad_x (the call's own clear), nothing else
    g = np.random.RandomState(3).standard_normal((L, k * F)).astype(np.float32)
    tg = torch.from_numpy(g).to(dev)
    buf, at, first = _guarded(T, F, dev)
    assert lib.ss_pool_scatter(_p(rowptr), L, _p(perm), k, _p(tg), T, F, at, _p(err), stream) == 0
    _check_guarded(buf, first, pr.sort_pool_backward(g, ROWPTR, want_perm, T), 'scatter')
    # segment pool and its gradient
    gl = np.random.RandomState(4).standard_normal((L, F)).astype(np.float32)
    tgl = torch.from_numpy(gl).to(dev)
    for mean in (0, 1):
        buf, at, first = _guarded(L, F, dev)
        assert lib.ss_segment_pool(_p(rowptr), L, _p(tx), T, F, mean, at, _p(err), stream) == 0
        _check_guarded(buf, first, pr.segment_pool(x, ROWPTR, bool(mean)), f'segment pool mean={mean}')
        buf, at, first = _guarded(T, F, dev)
        assert lib.ss_segment_pool_grad(_p(rowptr), L, _p(tgl), T, F, mean, at, stream) == 0
        _check_guarded(buf, first, pr.segment_pool_backward(gl, ROWPTR, T, bool(mean)), f'segment pool grad mean={mean}')
    # centre pool and its gradient
    roots = np.array([[-1, -1], [0, 0], [1, 0], [0, 62], [63, 63], [31, 64], [-1, -1], [255, 0], [128, 129], [C - 2, 0], [C - 1, C - 1], [C, 1],
                      [3 * C + 4, 0]], dtype=np.int32)
    troots = torch.from_numpy(roots).to(dev)
    buf, at, first = _guarded(L, F, dev)
    assert lib.ss_center_pool(_p(rowptr), L, _p(troots), _p(tx), T, F, at, _p(err), stream) == 0
    _check_guarded(buf, first, pr.center_pool(x, ROWPTR, roots), 'centre pool')
    buf, at, first = _guarded(T, F, dev)
    assert lib.ss_center_pool_grad(_p(rowptr), L, _p(troots), _p(tx), _p(tgl), T, F, at, _p(err), stream) == 0
    _check_guarded(buf, first, pr.center_pool_backward(x, gl, ROWPTR, roots), 'centre pool grad')
    # a float base that is not 16-byte aligned takes the scalar path and writes the same
    if F % 4 == 0:
        buf = torch.full(((L + 2) * k * F + 1,), SENTINEL, dtype=torch.int32, device=dev)
        at = ctypes.c_void_p(buf.data_ptr() + (k * F + 1) * 4)
        assert lib.ss_pool_gather(_p(rowptr), L, _p(perm), k, _p(tx), T, F, at, _p(err), stream) == 0
        _check_guarded(buf, k * F + 1, want, 'gather into an unaligned base')
    torch.cuda.synchronize(dev)
    assert int(err.item()) == 0


def test_ids_out_of_range_are_not_followed(ssa, dev, rowptr):
    """bad ids in the middle of a wavefront of good ones: the error flag rises, their places keep the sentinel, the good ones are
    written; the Python layer reports the flag late, as IndexError"""
    lib, k, F = ssa._native.lib(), 8, 4
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    x = planted(F)
    tx = torch.from_numpy(x).to(dev)
    want, want_perm = pr.sort_pool(x, ROWPTR, k)
    bad_perm = want_perm.copy()
    spoiled = [(5, 3, SIZES[5]), (7, 0, -2), (9, 7, 1 << 30), (12, 4, -(1 << 31))]  # (graph, slot, id): n itself, below -1, far beyond
    for q, j, p in spoiled:
        bad_perm[q, j] = p
    tperm = torch.from_numpy(bad_perm).to(dev)
    want_i = want.view(np.int32).reshape(L, k, F).copy()
    for q, j, _ in spoiled:
        want_i[q, j] = SENTINEL
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    buf, at, first = _guarded(L, k * F, dev)
    assert lib.ss_pool_gather(_p(rowptr), L, _p(tperm), k, _p(tx), T, F, at, _p(err), stream) == 0
    _check_guarded(buf, first, want_i.view(np.float32), 'gather with bad ids')
    assert int(err.item()) == 1
    err.zero_()
    g = np.random.RandomState(3).standard_normal((L, k * F)).astype(np.float32)
    buf, at, first = _guarded(T, F, dev)
    assert lib.ss_pool_scatter(_p(rowptr), L, _p(tperm), k, _p(torch.from_numpy(g).to(dev)), T, F, at, _p(err), stream) == 0
    clean = want_perm.copy()
    for q, j, _ in spoiled:
        clean[q, j] = -1  # the spoiled slots scatter nothing: the rows they named before stay zero
    _check_guarded(buf, first, pr.sort_pool_backward(g, ROWPTR, clean, T), 'scatter with bad ids')
    assert int(err.item()) == 1
    err.zero_()
    # roots outside their graph, one half of a pair -1, and a rowptr pair that leaves [0, T]
    roots = np.array([[0, 0]] * L, dtype=np.int32)
    roots[0] = (-1, -1)
    roots[3], roots[4], roots[8] = (63, 0), (-1, 5), (0, 1 << 30)
    bad_rp = ROWPTR.copy()
    bad_rp[12] = T + 5  # graph 11 = [.., T + 5), graph 12 = [T + 5, T): both refused
    trp = torch.from_numpy(bad_rp).to(dev)
    ok = [q for q in range(1, L) if q not in (3, 4, 8, 11, 12)]
    want_c = np.full((L, F), SENTINEL, dtype=np.int32)
    want_c[0] = 0
    followed = roots.copy()
    followed[[3, 4, 8]] = -1  # (the restatement follows what it is given)
    want_c[ok] = pr.center_pool(x, ROWPTR, followed)[ok].view(np.int32)
    buf, at, first = _guarded(L, F, dev)
    assert lib.ss_center_pool(_p(trp), L, _p(torch.from_numpy(roots).to(dev)), _p(tx), T, F, at, _p(err), stream) == 0
    _check_guarded(buf, first, want_c.view(np.float32), 'centre pool with bad roots')
    assert int(err.item()) == 1
    err.zero_()
    want_s = np.full((L, F), SENTINEL, dtype=np.int32)
    keep = [q for q in range(L) if q not in (11, 12)]
    want_s[keep] = pr.segment_pool(x, ROWPTR, False)[keep].view(np.int32)
    buf, at, first = _guarded(L, F, dev)
    assert lib.ss_segment_pool(_p(trp), L, _p(tx), T, F, 0, at, _p(err), stream) == 0
    _check_guarded(buf, first, want_s.view(np.float32), 'segment pool with a bad rowptr')
    assert int(err.item()) == 1
    err.zero_()
    buf, at, first = _guarded(L, k, dev)
    assert lib.ss_pool_select(_p(trp), L, _p(tx), T, F, k, at, _p(err), stream) == 0
    refused = want_perm.copy()
    refused[[11, 12]] = -1
    _check_guarded(buf, first, refused, 'select with a bad rowptr')
    assert int(err.item()) == 1
    # the Python layer: reported late, once
    ssa.pooling.check_errors()
    sg = ssa.ExactSubgraphs(rowptr, None, None, torch.from_numpy(roots).to(dev), None, None, None, None, None)
    y = ssa.center_pool(tx, sg)
    assert bool(torch.isfinite(y[ok]).all())
    with pytest.raises(IndexError):
        ssa.pooling.check_errors()
    ssa.pooling.check_errors()


# ---- offsets past 2^31 elements -----------------------------------------------------------------------------------------------------

def _formula(ids, F):
    """x[i, j] = ((131 i + 7 j) mod 1021 - 510) / 64: exact in fp32, the same numbers on the host and on the device"""
    v = (131 * np.asarray(ids, dtype=np.int64)[:, None] + 7 * np.arange(F, dtype=np.int64)[None, :]) % 1021 - 510
    return (v.astype(np.float32) / np.float32(64)).astype(np.float32)


def test_offsets_past_two_to_the_31_elements(ssa, dev):
    """T = 2 200 000, F = 1 024 (9.0 GB), graphs of 1 000 nodes, k = 8: x and grad_x pass 2^31 elements, graphs 524, 1048 and 2097
    straddle the 2, 4 and 8 GiB byte offsets (rows 524 288, 1 048 576, 2 097 152; the last is the 2^31-element offset too).  Those
    graphs, their neighbours, the first, the last and a sample of the others against the restatement on slices: sort pool and add
    pool, forward and backward."""
    n, F, per, k = 2_200_000, 1024, 1000, 8
    lt.require_free_memory(dev, 3 * n * F * 4, 'the large-offset pooling case')
    graphs = n // per
    rp = np.arange(graphs + 1, dtype=np.int64) * per
    bounds = [(1 << 31) // F // 4, (1 << 31) // F // 2, (1 << 31) // F]
    must = sorted({0, graphs - 1} | {b // per + d for b in bounds for d in (-1, 0, 1)})
    assert all(rp[b // per] < b < rp[b // per + 1] for b in bounds)
    rng = np.random.RandomState(5)
    check = sorted(set(must) | set(rng.choice(graphs, size=20, replace=False).tolist()))
    x = torch.empty((n, F), dtype=torch.float32, device=dev)
    assert x.numel() > 1 << 31
    cols = 7 * torch.arange(F, dtype=torch.int32, device=dev)[None, :]
    for r0 in range(0, n, 1 << 18):
        ids = torch.arange(r0, min(r0 + (1 << 18), n), dtype=torch.int32, device=dev)[:, None]
        x[r0:r0 + (1 << 18)] = ((131 * ids + cols) % 1021 - 510).to(torch.float32) / 64
    x.requires_grad_(True)
    trp = torch.from_numpy(rp).to(dev)
    rows = np.concatenate([np.arange(rp[q], rp[q + 1]) for q in check])
    xs = _formula(rows, F)  # the checked graphs, concatenated: local offsets rps
    rps = np.arange(len(check) + 1, dtype=np.int64) * per
    _assert_same(x.detach()[torch.from_numpy(rows[::97]).to(dev)], xs[::97], 'the formula on the device')
    tcheck = torch.from_numpy(np.array(check)).to(dev)

    y, perm = ssa.global_sort_pool(x, None, k, rowptr=trp, return_perm=True)
    want, want_perm = pr.sort_pool(xs, rps, k)
    assert np.array_equal(perm[tcheck].cpu().numpy(), want_perm)
    _assert_same(y[tcheck], want, 'large sort pool')
    g = torch.from_numpy(rng.standard_normal((graphs, k * F)).astype(np.float32)).to(dev)
    grad, = torch.autograd.grad(y, x, g)
    want_grad = pr.sort_pool_backward(g[tcheck].cpu().numpy(), rps, want_perm, len(rows))
    _assert_same(grad[torch.from_numpy(rows).to(dev)], want_grad, 'large sort pool x.grad')
    # every element of g lands exactly once and nothing else is written: as many non-zeros in grad_x as in g
    assert sum(int(torch.count_nonzero(c)) for c in grad.chunk(8)) == int(torch.count_nonzero(g))
    del grad, y

    y = ssa.global_add_pool(x, rowptr=trp)
    _assert_same(y[tcheck], pr.segment_pool(xs, rps), 'large add pool')
    gl = torch.from_numpy(rng.standard_normal((graphs, F)).astype(np.float32)).to(dev)
    grad, = torch.autograd.grad(y, x, gl)
    _assert_same(grad[torch.from_numpy(rows).to(dev)], pr.segment_pool_backward(gl[tcheck].cpu().numpy(), rps, len(rows)), 'large add pool x.grad')
    del grad, y, x
    ssa.pooling.check_errors()
    torch.cuda.empty_cache()
