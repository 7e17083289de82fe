"""cn_pool.common_neighbour_pool (csrc/ss_cn_rows.hip) on the GPU.  Forward and backward bits are the restatement's
(tests/cn_pool_restatement.py, pinned to float64 by tests/test_cn_pool_host.py): the contract fixes the accumulation order, so there is
exactly one right answer, whichever tier a row goes through, whichever piece type ran and whatever else the batch holds."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

import cn_pool_restatement as cr
import large_table_helpers as lt
import model_steps_reference as ms

pytestmark = pytest.mark.gpu

WIDTHS = (0, 1, 3, 4, 20, 64, 128, 256, 260, 1024)  # no column; scalar pieces; lane groups of 1, 8 (5 pieces), 16, 32, 64; a second pass of one piece; four passes
HUB_ENTRIES = (1, 255, 256, 257, 1 << 40)
SENTINEL = 0x7FC0BEEF  # a NaN no sum produces


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _to(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


class Case(object):
    """the planted list, its plan (default hub_entries), x [N, 1024] and g [L, 1024] (the first F columns are the x and g of every F:
    the columns do not depend on each other), and the restated forward and backward, computed once and left unchanged"""

    def __init__(self, ssa, dev):
        self.dev = dev
        self.rowptr, self.ids, self.coef = cr.planted()
        self.L, self.T = len(self.rowptr) - 1, len(self.ids)
        self.lists = _to(dev, self.rowptr, self.ids, self.coef)
        self.plan = ssa.CommonNeighbourBatch.from_lists(cr.N, *self.lists)
        self.host = {'x': cr.features(cr.N, 1024), 'g': cr.features(self.L, 1024, seed=5)}
        self.x, self.g = _to(dev, self.host['x'], self.host['g'])
        self.out = cr.forward(self.rowptr, self.ids, self.coef, self.host['x'])
        self.grad = cr.grad(self.rowptr, self.ids, self.coef, self.host['g'], cr.N)
        self.rows, self.groups = np.diff(self.rowptr), np.bincount(self.ids, minlength=cr.N)

    def plan_with(self, ssa, hub_entries):
        return ssa.CommonNeighbourBatch.from_lists(cr.N, *self.lists, hub_entries=hub_entries)


@pytest.fixture(scope='module')
def case(ssa, dev):
    return Case(ssa, dev)


def _bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f'{what}: {tuple(g.shape)} against {tuple(w.shape)}'
    bad = torch.nonzero(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} of {g.numel()} elements differ, first at {bad[:4].tolist()}'


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _run(ssa, x, plan, g):
    """(forward output, x.grad) of one forward + backward"""
    xs = x.detach().clone().requires_grad_(True)
    y = ssa.common_neighbour_pool(xs, plan)
    y.backward(g)
    return y.detach(), xs.grad


def _hubs(m, hub_entries):
    rows = np.nonzero(m > hub_entries)[0]
    return rows, (m[rows] + 255) // 256


def test_plan(case, ssa, dev):
    plan = case.plan
    assert (plan.num_nodes, plan.num_links, plan.num_entries, plan.device, plan.hub_entries) == (cr.N, case.L, case.T, dev, 256)
    assert plan.rowptr.tolist() == case.rowptr.tolist() and plan.ids.tolist() == case.ids.tolist() and plan.rowptr.dtype == plan.ids.dtype == torch.int64
    assert _bits(plan.coef).tolist() == _bits(case.coef).tolist() and plan.coef.dtype == torch.float32
    assert plan.owner.dtype == torch.int64 and plan.owner.tolist() == cr.owners(case.rowptr).tolist()
    nodes, nrowptr, order = cr.grouping(case.ids, cr.N)
    assert plan.num_touched == len(nodes) and plan.nodes.tolist() == nodes.tolist() and plan.node_rowptr.tolist() == nrowptr.tolist()
    assert plan.order.dtype == torch.int32 and plan.order.tolist() == order.tolist()
    for h in HUB_ENTRIES:
        p = case.plan_with(ssa, h)
        for (lists, H, C), m in ((p.link_hubs, case.rows), (p.node_hubs, case.groups[nodes])):  # (links by row, nodes by position in `nodes`)
            rows, chunks = _hubs(m, h)
            assert (H, C) == (len(rows), chunks.sum()), h
            if H:
                assert lists[0].tolist() == rows.tolist() and lists[1].tolist() == np.concatenate([[0], np.cumsum(chunks)]).tolist()
                assert lists[2].tolist() == np.repeat(np.arange(H), chunks).tolist()
            assert all(t.dtype == torch.int32 for t in lists)
        assert p.order.tolist() == order.tolist()  # the grouping does not depend on hub_entries
    assert plan.link_hubs[1:] == (6, 2 + 2 + 2 + 2 + 3 + 5) and plan.node_hubs[1:] == (6, 16)  # 257, 258, 300, 512, 513, 1 025 on both sides
    before = ssa.CommonNeighbourBatch.builds
    host = ssa.CommonNeighbourBatch.from_lists(cr.N, *(t.cpu() for t in case.lists))  # host tensors: the plan lives on the current GPU
    assert host.device == dev and host.order.tolist() == order.tolist() and ssa.CommonNeighbourBatch.builds == before + 1
    named = ssa.CommonNeighbourBatch.from_lists(cr.N, *case.lists, device='cuda')       # a bare 'cuda' is the current GPU
    assert named.device == dev
    edited = [t.clone() for t in case.lists]
    private = ssa.CommonNeighbourBatch.from_lists(cr.N, *edited)
    edited[1][5] = (edited[1][5] + 1) % cr.N  # the plan keeps private copies
    edited[2][7] += 1.0
    y, grad = _run(ssa, case.x[:, :8].contiguous(), private, case.g[:, :8])
    _assert_same(y, case.out[:, :8], 'private copy, forward')
    _assert_same(grad, case.grad[:, :8], 'private copy, backward')


def test_plan_refuses_bad_lists_on_the_device(case, ssa, dev):
    rowptr, ids, coef = case.lists
    for bad in (-1, cr.N, 1 << 40):
        wrong = ids.clone()
        wrong[case.T // 2] = bad
        with pytest.raises(IndexError):
            ssa.CommonNeighbourBatch.from_lists(cr.N, rowptr, wrong, coef)
    for k, v in ((3, int(rowptr[2]) - 1), (0, 1), (case.L, case.T - 1), (case.L, case.T + 1)):
        wrong = rowptr.clone()
        wrong[k] = v
        with pytest.raises(ValueError):
            ssa.CommonNeighbourBatch.from_lists(cr.N, wrong, ids, coef)
    for x in (case.x.cpu()[:, :4], case.x[:, :4].double(), case.x[:-1, :4]):
        with pytest.raises(ValueError):
            ssa.common_neighbour_pool(x, case.plan)


@pytest.mark.parametrize('F', WIDTHS)
def test_forward_and_backward_bits(case, ssa, F):
    x, g = case.x[:, :F].contiguous(), case.g[:, :F]  # (g: a non-contiguous grad_out unless F = 1024)
    y, grad = _run(ssa, x, case.plan, g)
    assert y.shape == (case.L, F) and grad.shape == (cr.N, F) and y.dtype == grad.dtype == torch.float32
    _assert_same(y, case.out[:, :F], f'forward, F = {F}')
    _assert_same(grad, case.grad[:, :F], f'backward, F = {F}')
    if F:
        assert bool((_bits(y)[torch.from_numpy(case.rows == 0)] == 0).all()) and bool((_bits(grad)[torch.from_numpy(case.groups == 0)] == 0).all())  # +0.0, not -0.0
        y2 = ssa.common_neighbour_pool(case.x[:, :F], case.plan)  # a non-contiguous x (unless F = 1024) without a gradient
        assert not y2.requires_grad
        _assert_same(y2, y, 'a non-contiguous x')


@pytest.mark.parametrize('F', (20, 260))
@pytest.mark.parametrize('hub_entries', HUB_ENTRIES)
def test_bits_do_not_depend_on_the_tier(case, ssa, hub_entries, F):
    plan = case.plan_with(ssa, hub_entries)
    assert plan.link_hubs[1] == (case.rows > hub_entries).sum() and plan.node_hubs[1] == (case.groups > hub_entries).sum()
    y, grad = _run(ssa, case.x[:, :F].contiguous(), plan, case.g[:, :F])
    _assert_same(y, case.out[:, :F], f'forward, hub_entries = {hub_entries}')
    _assert_same(grad, case.grad[:, :F], f'backward, hub_entries = {hub_entries}')


@pytest.mark.parametrize('hub_entries', (256, 1 << 40))
def test_misaligned_bases_run_the_scalar_instance(case, ssa, dev, hub_entries):
    """x and g one float past a 16-byte boundary with F % 4 == 0: the scalar instance, the same bits"""
    F = 64
    plan = case.plan_with(ssa, hub_entries)
    xs = torch.empty(cr.N * F + 1, dtype=torch.float32, device=dev)[1:].view(cr.N, F)
    gs = torch.empty(case.L * F + 1, dtype=torch.float32, device=dev)[1:].view(case.L, F)
    xs.copy_(case.x[:, :F])
    gs.copy_(case.g[:, :F])
    assert xs.data_ptr() % 16 == 4 and gs.data_ptr() % 16 == 4 and xs.is_contiguous() and gs.is_contiguous()
    _assert_same(plan.forward(xs), case.out[:, :F], 'forward, misaligned x')
    _assert_same(plan.grad(gs), case.grad[:, :F], 'backward, misaligned g')
    y, grad = _run(ssa, xs, plan, gs)
    _assert_same(y, case.out[:, :F], 'forward through autograd')
    _assert_same(grad, case.grad[:, :F], 'backward through autograd')


def test_unit_coefficients(case, ssa, dev):
    rowptr, ids, coef = cr.planted(coefficients='unit')
    F = 20
    plan = ssa.CommonNeighbourBatch.from_lists(cr.N, *_to(dev, rowptr, ids, coef))
    y, grad = _run(ssa, case.x[:, :F].contiguous(), plan, case.g[:, :F])
    _assert_same(y, cr.forward(rowptr, ids, coef, case.host['x'][:, :F]), 'unit coefficients, forward')
    _assert_same(grad, cr.grad(rowptr, ids, coef, case.host['g'][:, :F], cr.N), 'unit coefficients, backward')


def test_a_zero_coefficient_adds_a_signed_zero_and_nothing_else(ssa, dev):
    """coef 0 times a finite row is +-0, which changes no sum begun at +0; times Inf it is NaN, as in the restatement"""
    rowptr, ids = np.array([0, 3, 5], dtype=np.int64), np.array([1, 2, 3, 2, 4], dtype=np.int64)
    coef = np.array([1.5, 0.0, -2.0, 0.0, 0.0], dtype=np.float32)
    x = cr.features(6, 4)
    x[4] = np.inf
    x[2] = -x[2]
    plan = ssa.CommonNeighbourBatch.from_lists(6, *_to(dev, rowptr, ids, coef))
    with np.errstate(invalid='ignore'):
        want = cr.forward(rowptr, ids, coef, x)
    assert np.isnan(want[1]).all() and np.isfinite(want[0]).all()
    got = ssa.common_neighbour_pool(torch.from_numpy(x).to(dev), plan)
    _assert_same(got[0], want[0], 'the finite row')
    assert bool(torch.isnan(got[1]).all())
    g = cr.features(2, 4, seed=8)
    _assert_same(plan.grad(torch.from_numpy(g).to(dev)), cr.grad(rowptr, ids, coef, g, 6), 'backward')


def test_rows_do_not_depend_on_the_batch(case, ssa, dev):
    """permuting, repeating or slicing the links leaves every surviving row's bits unchanged"""
    F = 20
    rng = np.random.RandomState(3)
    x = case.x[:, :F].contiguous()
    for name, sel in (('permuted', rng.permutation(case.L)), ('repeated', np.concatenate([np.arange(case.L), [0, 2, case.L - 1, 0]])),
                      ('sliced', np.arange(1, case.L, 3)), ('one long row', np.array([0]))):
        rows = [np.arange(case.rowptr[q], case.rowptr[q + 1]) for q in sel]
        at = np.concatenate(rows)
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        ids, coef = case.ids[at], case.coef[at]
        plan = ssa.CommonNeighbourBatch.from_lists(cr.N, *_to(dev, rowptr, ids, coef))
        g = case.g[torch.from_numpy(sel).to(dev), :F]
        y, grad = _run(ssa, x, plan, g)
        _assert_same(y, case.out[sel, :F], name)
        _assert_same(grad, cr.grad(rowptr, ids, coef, case.host['g'][sel, :F], cr.N), name + ', backward')


def test_two_runs_give_identical_bits(case, ssa):
    F = 128
    x, g = case.x[:, :F].contiguous(), case.g[:, :F].contiguous()
    first, second = _run(ssa, x, case.plan, g), _run(ssa, x, case.plan, g)
    _assert_same(second[0], first[0], 'forward, second run')
    _assert_same(second[1], first[1], 'backward, second run')
    xs = x.clone().requires_grad_(True)
    y = ssa.common_neighbour_pool(xs, case.plan)
    y.backward(g, retain_graph=True)
    once = xs.grad.clone()
    xs.grad = None
    y.backward(g)
    _assert_same(xs.grad, once, 'two backward runs of one forward')


# ---- direct launches into sentinel-filled buffers ---------------------------------------------------------------------------------
def _guarded(rows, F, dev):
    """a [rows + 2, F] buffer of sentinels and the view of its inner rows: a guard row on either side"""
    buf = torch.full(((rows + 2) * max(F, 1),), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    return buf, buf[F:F + rows * F].view(rows, F)


def _check_written(buf, inner, written, want, what):
    """rows `written` (bool) of inner hold `want`; every other place of buf holds the sentinel"""
    got = _bits(inner)
    written = torch.from_numpy(np.asarray(written))
    _assert_same(inner[written.to(inner.device)], want[written.numpy()], what)
    assert bool((got[~written] == SENTINEL).all()), f'{what}: a row that is not its own was written'
    F = inner.size(1)
    edge = _bits(buf)
    assert bool((edge[:F] == SENTINEL).all()) and bool((edge[-F:] == SENTINEL).all()), f'{what}: a guard row was written'


def _chunk_partials(terms_of_row, rows):
    """[n_chunks, F]: the sequential sums of the 256-entry chunks of the rows `rows`, in order; terms_of_row(r): float32 [m, F]"""
    out = []
    for r in rows:
        t = terms_of_row(r)
        out += [cr.chunked_sum(t[a:a + cr.C]) for a in range(0, len(t), cr.C)]
    return np.stack(out)


@pytest.mark.parametrize('F', (20, 3, 260))
def test_direct_launches_write_their_own_places_only(case, ssa, dev, F):
    lib, stream, plan = ssa._native.lib(), _stream(dev), case.plan
    L, T, N, M = case.L, case.T, cr.N, plan.num_touched
    x, g = case.x[:, :F].contiguous(), case.g[:, :F].contiguous()
    hx, hg = case.host['x'][:, :F], case.host['g'][:, :F]
    own = cr.owners(case.rowptr)
    nodes, nrowptr, order = cr.grouping(case.ids, N)
    # forward
    (hub_rows, hub_chunk, chunk_hub), H, C = plan.link_hubs
    buf, out = _guarded(L, F, dev)
    assert lib.ss_cn_rows_forward(_p(plan.rowptr), _p(plan.ids), _p(plan.coef), L, T, N, 256, _p(x), F, _p(out), stream) == 0
    _check_written(buf, out, case.rows <= 256, case.out[:, :F], 'ss_cn_rows_forward')
    wbuf, ws = _guarded(C, F, dev)
    assert lib.ss_cn_rows_forward_hub_partials(_p(plan.rowptr), _p(plan.ids), _p(plan.coef), L, T, N, _p(hub_rows), _p(hub_chunk), _p(chunk_hub), H, C,
                                               _p(x), F, _p(ws), C * F * 4, stream) == 0
    terms = lambda q: case.coef[case.rowptr[q]:case.rowptr[q + 1], None] * hx[case.ids[case.rowptr[q]:case.rowptr[q + 1]]]
    _check_written(wbuf, ws, np.ones(C, dtype=bool), _chunk_partials(terms, np.nonzero(case.rows > 256)[0]), 'ss_cn_rows_forward_hub_partials')
    assert lib.ss_cn_rows_forward_hub_finish(L, _p(hub_rows), _p(hub_chunk), H, C, _p(ws), C * F * 4, F, _p(out), stream) == 0
    _check_written(buf, out, np.ones(L, dtype=bool), case.out[:, :F], 'ss_cn_rows_forward_hub_finish')
    # backward
    (hub_rows, hub_chunk, chunk_hub), H, C = plan.node_hubs
    buf, grad = _guarded(N, F, dev)
    assert lib.ss_cn_rows_grad(_p(plan.nodes), _p(plan.node_rowptr), _p(plan.order), M, _p(plan.owner), _p(plan.coef), T, L, N, 256, _p(g), F, _p(grad),
                               stream) == 0
    _check_written(buf, grad, (case.groups > 0) & (case.groups <= 256), case.grad[:, :F], 'ss_cn_rows_grad')
    wbuf, ws = _guarded(C, F, dev)
    assert lib.ss_cn_rows_grad_hub_partials(_p(plan.node_rowptr), _p(plan.order), M, _p(plan.owner), _p(plan.coef), T, L, N, _p(hub_rows), _p(hub_chunk),
                                            _p(chunk_hub), H, C, _p(g), F, _p(ws), C * F * 4, stream) == 0
    entries = lambda r: order[nrowptr[r]:nrowptr[r + 1]]
    terms = lambda r: case.coef[entries(r), None] * hg[own[entries(r)]]
    _check_written(wbuf, ws, np.ones(C, dtype=bool), _chunk_partials(terms, np.nonzero(case.groups[nodes] > 256)[0]), 'ss_cn_rows_grad_hub_partials')
    assert lib.ss_cn_rows_grad_hub_finish(_p(plan.nodes), M, _p(hub_rows), _p(hub_chunk), H, C, N, _p(ws), C * F * 4, F, _p(grad), stream) == 0
    _check_written(buf, grad, case.groups > 0, case.grad[:, :F], 'ss_cn_rows_grad_hub_finish')


def test_direct_launches_refuse_bad_arguments_before_any_launch(case, ssa, dev):
    lib, stream, plan = ssa._native.lib(), _stream(dev), case.plan
    L, T, N, M, F = case.L, case.T, cr.N, plan.num_touched, 8
    x, g = case.x[:, :F].contiguous(), case.g[:, :F].contiguous()
    (lh, lc, lch), LH, LC = plan.link_hubs
    (nh, nc, nch), NH, NC = plan.node_hubs
    buf, out = _guarded(L, F, dev)
    gbuf, grad = _guarded(N, F, dev)
    wbuf, ws = _guarded(max(LC, NC), F, dev)
    big = 1 << 31
    fwd = lambda **k: lib.ss_cn_rows_forward(_p(plan.rowptr), k.get('ids', _p(plan.ids)), _p(plan.coef), k.get('L', L), k.get('T', T), k.get('N', N),
                                             k.get('hub', 256), _p(x), k.get('F', F), _p(out), stream)
    fpart = lambda **k: lib.ss_cn_rows_forward_hub_partials(_p(plan.rowptr), _p(plan.ids), _p(plan.coef), L, T, N, _p(lh), _p(lc), k.get('chunk_hub', _p(lch)),
                                                            k.get('H', LH), k.get('C', LC), _p(x), F, _p(ws), k.get('bytes', LC * F * 4), stream)
    ffin = lambda **k: lib.ss_cn_rows_forward_hub_finish(k.get('L', L), _p(lh), _p(lc), k.get('H', LH), k.get('C', LC), _p(ws), k.get('bytes', LC * F * 4), F,
                                                         k.get('out', _p(out)), stream)
    bwd = lambda **k: lib.ss_cn_rows_grad(_p(plan.nodes), _p(plan.node_rowptr), _p(plan.order), k.get('M', M), k.get('owner', _p(plan.owner)), _p(plan.coef),
                                          k.get('T', T), k.get('L', L), k.get('N', N), k.get('hub', 256), _p(g), F, _p(grad), stream)
    bpart = lambda **k: lib.ss_cn_rows_grad_hub_partials(_p(plan.node_rowptr), _p(plan.order), M, _p(plan.owner), _p(plan.coef), T, L, N, _p(nh), _p(nc),
                                                         _p(nch), k.get('H', NH), k.get('C', NC), k.get('g', _p(g)), F, _p(ws), k.get('bytes', NC * F * 4), stream)
    bfin = lambda **k: lib.ss_cn_rows_grad_hub_finish(_p(plan.nodes), k.get('M', M), _p(nh), _p(nc), k.get('H', NH), k.get('C', NC), k.get('N', N), _p(ws),
                                                      k.get('bytes', NC * F * 4), F, _p(grad), stream)
    calls = [fwd(ids=None), fwd(L=-1), fwd(T=big), fwd(N=big), fwd(hub=0), fwd(F=-1),
             fpart(chunk_hub=None), fpart(H=LC + 1), fpart(C=-1), fpart(bytes=LC * F * 4 - 1),
             ffin(L=big), ffin(H=LC + 1), ffin(bytes=LC * F * 4 - 1), ffin(out=None),
             bwd(owner=None), bwd(M=N + 1), bwd(M=-1), bwd(T=-1), bwd(L=big), bwd(hub=0), bwd(hub=-7),
             bpart(g=None), bpart(H=NC + 1), bpart(C=big), bpart(bytes=NC * F * 4 - 1),
             bfin(M=-1), bfin(H=NC + 1), bfin(N=big), bfin(bytes=NC * F * 4 - 1)]
    assert calls == [-1] * len(calls)
    assert lib.ss_cn_rows_forward(None, None, None, 0, 0, N, 256, None, F, None, stream) == 0     # empty work, null pointers
    assert lib.ss_cn_rows_grad(None, None, None, 0, None, None, 0, 0, N, 256, None, F, None, stream) == 0
    torch.cuda.synchronize(dev)
    for b in (buf, gbuf, wbuf):
        assert bool((_bits(b) == SENTINEL).all()), 'a refused call wrote'


def test_ids_and_owners_out_of_range_are_not_followed(ssa, dev):
    """Rows of 70 and 300 entries -- more than a wavefront, and a hub row -- with ids (forward) and owners, order words (backward) out
    of range among good ones.  Such an entry keeps its place and adds nothing; its stand-in loads go to position 0 / row 0, which hold
    NaN here and are named by nothing, so a NaN in the result is a stand-in that was used.  No stray write; the plan raises."""
    lib, stream = ssa._native.lib(), _stream(dev)
    N, F = 500, 20
    rng = np.random.RandomState(11)
    counts = np.array([0, 70, 300, 5, 70, 1])  # link 0 is empty: no entry owns row 0 of g
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    L, T = len(counts), int(rowptr[-1])
    ids = rng.randint(1, N, size=T).astype(np.int64)  # node 0 is named by nothing
    ids[70:370:3] = 77                                # a node group of 100 entries inside the 300-entry row
    coef = rng.uniform(0.5, 1.5, size=T).astype(np.float32)
    x, g = cr.features(N, F, seed=2), cr.features(L, F, seed=4)
    x[0] = g[0] = np.nan
    bad_at = np.array([3, 40, 69, 70, 71, 200, 325, 326, 369, 371, 445])
    bad_ids = ids.copy()
    bad_ids[bad_at] = np.resize(np.array([-1, N, 1 << 40, -(1 << 40), N + 7], dtype=np.int64), len(bad_at))
    use = np.ones(T, dtype=bool)
    use[bad_at] = False
    with pytest.raises(IndexError):
        ssa.CommonNeighbourBatch.from_lists(N, *_to(dev, rowptr, bad_ids, coef))
    trowptr, tids, tcoef, tx, tg = _to(dev, rowptr, bad_ids, coef, x, g)
    want = cr.forward(rowptr, ids, coef, x, use=use)
    assert np.isfinite(want).all()
    hubs = _to(dev, np.array([2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.array([0, 0], dtype=np.int32))
    for hub_entries in (256, 1 << 40):
        buf, out = _guarded(L, F, dev)
        assert lib.ss_cn_rows_forward(_p(trowptr), _p(tids), _p(tcoef), L, T, N, hub_entries, _p(tx), F, _p(out), stream) == 0
        if hub_entries == 256:
            wbuf, ws = _guarded(2, F, dev)
            assert lib.ss_cn_rows_forward_hub_partials(_p(trowptr), _p(tids), _p(tcoef), L, T, N, *map(_p, hubs), 1, 2, _p(tx), F, _p(ws), 2 * F * 4, stream) == 0
            assert lib.ss_cn_rows_forward_hub_finish(L, _p(hubs[0]), _p(hubs[1]), 1, 2, _p(ws), 2 * F * 4, F, _p(out), stream) == 0
            # the two chunks of the 300-entry row as rows of their own: entries 70 .. 325 and 326 .. 369
            chunks = cr.forward(np.array([0, 256, 300], dtype=np.int64), ids[70:370], coef[70:370], x, use=use[70:370])
            _check_written(wbuf, ws, np.ones(2, dtype=bool), chunks, 'partials with bad ids')
        _check_written(buf, out, np.ones(L, dtype=bool), want, f'forward with bad ids, hub_entries = {hub_entries}')
    # backward: the grouping of the GOOD ids, owners out of range at bad_at, and two order words outside [0, T)
    nodes, nrowptr, order = cr.grouping(ids, N)
    own = cr.owners(rowptr)
    bad_own = own.copy()
    bad_own[bad_at] = np.resize(np.array([-1, L, 1 << 40, -5], dtype=np.int64), len(bad_at))
    bad_order = order.copy()
    lost = [int(np.nonzero(order == k)[0][0]) for k in (100, 420)]  # the places of entries 100 and 420 in the order
    bad_order[lost] = [-1, T]
    use_b = use.copy()
    use_b[[100, 420]] = False
    want = cr.grad(rowptr, ids, coef, g, N, use=use_b)
    assert np.isfinite(want).all()
    tnodes, tnrowptr, torder, town = _to(dev, nodes, nrowptr, bad_order.astype(np.int32), bad_own)
    M = len(nodes)
    buf, grad = _guarded(N, F, dev)
    assert lib.ss_cn_rows_grad(_p(tnodes), _p(tnrowptr), _p(torder), M, _p(town), _p(tcoef), T, L, N, 1 << 40, _p(tg), F, _p(grad), stream) == 0
    named = np.zeros(N, dtype=bool)
    named[nodes] = True
    _check_written(buf, grad, named, want, 'backward with bad owners and order words')
    # a node id that is no row of grad_x, a row pointer pair that leaves [0, T], a hub list that names no row: left alone
    wrong_nodes, wrong_rowptr = nodes.copy(), nrowptr.copy()
    wrong_nodes[[0, 5]] = [-3, N]
    wrong_rowptr[M] = T + 9
    tn, tr = _to(dev, wrong_nodes, wrong_rowptr)
    buf, grad = _guarded(N, F, dev)
    assert lib.ss_cn_rows_grad(_p(tn), _p(tr), _p(torder), M, _p(town), _p(tcoef), T, L, N, 1 << 40, _p(tg), F, _p(grad), stream) == 0
    named[[nodes[0], nodes[5], nodes[M - 1]]] = False
    _check_written(buf, grad, named, want, 'backward with rows that are not followed')
    stray = _to(dev, np.array([-1, L + 3], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32))
    buf, out = _guarded(L, F, dev)
    wbuf, ws = _guarded(2, F, dev)
    assert lib.ss_cn_rows_forward_hub_partials(_p(trowptr), _p(tids), _p(tcoef), L, T, N, *map(_p, stray), 2, 2, _p(tx), F, _p(ws), 2 * F * 4, stream) == 0
    assert lib.ss_cn_rows_forward_hub_finish(L, _p(stray[0]), _p(stray[1]), 2, 2, _p(ws), 2 * F * 4, F, _p(out), stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((_bits(buf) == SENTINEL).all()) and bool((_bits(wbuf) == SENTINEL).all())


# ---- from a graph -----------------------------------------------------------------------------------------------------------------
COMMON = (0, 1, 256, 257, 600)


def _planted_graph():
    """about 2 000 nodes: link i = (2i, 2i + 1) has COMMON[i] common neighbours, taken from one shared pool (so a pool node is a common
    neighbour of several links), and every endpoint has leaves of its own: neighbours that are not common"""
    import scipy.sparse as sp
    n = 2000
    pool = np.arange(100, 800)
    edges = []
    for i, c in enumerate(COMMON):
        u, v = 2 * i, 2 * i + 1
        edges += [(u, w) for w in pool[17 * i:17 * i + c]] + [(v, w) for w in pool[17 * i:17 * i + c]]
        edges += [(u, 1000 + 40 * i + k) for k in range(7)] + [(v, 1500 + 40 * i + k) for k in range(9)]
    edges.append((0, 1))  # the endpoints of a link may be neighbours
    e = np.array(edges, dtype=np.int64)
    A = sp.csr_matrix((np.ones(2 * len(e)), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n))
    A.sum_duplicates()
    links = np.array([(2 * i, 2 * i + 1) for i in range(len(COMMON))] + [(9, 8), (6, 6), (4, 7), (1500, 1501)], dtype=np.int64)
    return A.tocsr(), links


def test_from_a_graph(ssa, dev):
    A, links = _planted_graph()
    n = A.shape[0]
    tl = torch.from_numpy(links)
    custom = torch.from_numpy(np.random.RandomState(4).uniform(0.5, 2.0, size=n))
    F = 20
    x = cr.features(n, F, seed=6)
    tx = torch.from_numpy(x).to(dev)
    for w in ('CN', 'AA', 'RA', custom):
        want = ssa.heuristics.common_neighbours(A, tl, w)
        plan = ssa.CommonNeighbourBatch(A, tl, w)
        counts = np.diff(want.rowptr.numpy())
        assert counts[:len(COMMON)].tolist() == list(COMMON) and counts[len(COMMON)] == 600 and counts[len(COMMON) + 1] == 257 + 7  # (9, 8); (6, 6): its own row
        assert plan.device == dev and plan.num_links == len(links) and plan.num_nodes == n and plan.num_entries == int(want.rowptr[-1])
        assert plan.rowptr.tolist() == want.rowptr.tolist() and plan.ids.tolist() == want.ids.tolist()
        assert _bits(plan.coef).tolist() == _bits(want.coef).tolist()
        assert plan.link_hubs[1] == (counts > 256).sum() and plan.node_hubs[1] == 0
        got = ssa.common_neighbour_pool(tx, plan)
        feats = ssa.heuristics.common_neighbour_features(A, tl, tx, w)
        short = torch.from_numpy(counts <= 256)
        assert int(short.sum()) >= 5 and int((~short).sum()) >= 4
        _assert_same(got[short.to(dev)], feats[short.to(feats.device)], 'links of at most 256 common neighbours against common_neighbour_features')
        _assert_same(got, cr.forward(want.rowptr.numpy(), want.ids.numpy(), want.coef.numpy(), x), 'every link against the chunked restatement')
    small = ssa.CommonNeighbourBatch(A, tl, 'RA', hub_entries=3)
    assert small.node_hubs[1] > 0
    g = cr.features(len(links), F, seed=7)
    _assert_same(small.grad(torch.from_numpy(g).to(dev)), cr.grad(small.rowptr.cpu().numpy(), small.ids.cpu().numpy(), small.coef.cpu().numpy(), g, n), 'backward, RA')
    empty = ssa.CommonNeighbourBatch(A, tl[:0], 'CN')
    assert empty.num_links == 0 and ssa.common_neighbour_pool(tx, empty).shape == (0, F)
    none = ssa.CommonNeighbourBatch(A, torch.tensor([[1000, 1500], [0, 1]]), 'CN')  # two links without a common neighbour
    xs = tx.clone().requires_grad_(True)
    y = ssa.common_neighbour_pool(xs, none)
    y.sum().backward()
    assert none.num_entries == 0 and bool((_bits(y) == 0).all()) and bool((_bits(xs.grad) == 0).all())
    with pytest.raises(IndexError):
        ssa.CommonNeighbourBatch(A, torch.tensor([[0, 1], [2, n]]), 'CN')
    ssa.CommonNeighbourBatch(A, tl, 'CN')  # (the report word was cleared)


# ---- an NCN-shaped step -----------------------------------------------------------------------------------------------------------
class Ncn(ms._Model):
    """GCNConv(F_IN, HIDDEN) -> cat(link_hadamard(h), common_neighbour_pool(h)) -> Linear -> logits.  b: x, graph, links, cn"""

    def __init__(self, ops):
        super().__init__()
        self.ops = ops
        self.conv = ops.gcn(ms.F_IN, ms.HIDDEN)
        self.lin = torch.nn.Linear(2 * ms.HIDDEN, 1)

    def stack(self, x, graph):
        return self.conv(x, *ms._args(graph))

    def forward(self, b, taps=None):
        h = self._stack(b.x, b.graph)
        d = torch.cat([self.ops.hadamard(h, b.links), self.ops.cn_pool(h, b.cn)], 1)
        if taps is not None:
            taps['stack'], taps['readout'] = h, d
        return self.lin(d).view(-1)


def _plain_cn_pool(x, cn):
    rowptr, ids, coef = cn
    owner = torch.repeat_interleave(torch.arange(len(rowptr) - 1), rowptr[1:] - rowptr[:-1])
    return x.new_zeros((len(rowptr) - 1, x.size(1))).index_add_(0, owner, coef.to(x.dtype)[:, None] * x[ids])


def _make_ncn(ops):
    if not hasattr(ops, 'cn_pool'):  # (model_steps_reference.plain_ops: the float64 form)
        ops = copy.copy(ops)
        ops.cn_pool = _plain_cn_pool
    return Ncn(ops)


def test_an_ncn_shaped_step(ssa, dev):
    import scipy.sparse as sp
    inp = ms.elph_inputs()
    n, L = inp.n, len(inp.links)
    A = sp.csr_matrix((np.ones(inp.ei.shape[1]), (inp.ei[0], inp.ei[1])), shape=(n, n))
    A = ((A + A.T) > 0).astype(np.float64).tocsr()
    tei, tw, tlinks = _to(dev, inp.ei, inp.w, inp.links)
    x = torch.from_numpy(inp.x).to(dev)
    cn = ssa.CommonNeighbourBatch(A, tlinks, 'RA')
    assert cn.num_entries > 500 and cn.link_hubs[1] == cn.node_hubs[1] == 0
    tiers = ssa.CommonNeighbourBatch(A, tlinks, 'RA', hub_entries=16)
    assert tiers.link_hubs[1] > 0 and tiers.node_hubs[1] > 0
    ops = types.SimpleNamespace(gcn=ssa.GCNConv, hadamard=ssa.link_hadamard, cn_pool=ssa.common_neighbour_pool)
    state = copy.deepcopy(ms.build(_make_ncn, ms.plain_ops(), 47).state_dict())
    labels = ms.labels_for(L, ms.STEP_SEED, dev)

    def fresh():
        model = _make_ncn(ops)
        model.load_state_dict(copy.deepcopy(state))
        return model.to(dev)

    batch = types.SimpleNamespace(x=x, graph=ssa.GCNGraph(n, tei, tw), links=ssa.LinkBatch(n, tlinks), cn=cn, num_links=L)
    first, second = ms.step(fresh(), batch, labels), ms.step(fresh(), batch, labels)
    assert all(v is not None for v in first.values())
    assert ms.differing(second, first) == []  # identical loss bits, identical bits of every parameter gradient
    other = copy.copy(batch)
    other.cn = tiers
    assert ms.differing(ms.step(fresh(), other, labels), first) == []  # ... whichever tier the rows went through
    host_cn = (cn.rowptr.cpu(), cn.ids.cpu(), cn.coef.cpu())
    host_batch = types.SimpleNamespace(x=x.cpu(), graph=ms.HostGraph(n, inp.ei, inp.w), links=ms.HostLinks(n, inp.links), cn=host_cn, num_links=L)
    r64, r32 = ms.float64_runs(_make_ncn, fresh(), host_batch, labels)
    rows = ms.error_table(fresh(), first, r64, r32)
    print('\n' + ms.format_table('the NCN-shaped step on the GPU', rows))
    assert all(e_32 > 0 for _, _, _, e_32, _, _ in rows)
    assert [r[0] for r in rows if not r[5]] == []


# ---- one large case ---------------------------------------------------------------------------------------------------------------
def test_offsets_past_two_to_the_31_elements(ssa, dev):
    """N = L = 2 200 000, F = 1 024: x, g, out and grad_x hold 2.25e9 elements (9.0 GB) each, so element offsets pass 2^31 and byte
    offsets 2, 4 and 8 GiB (rows 524 288, 1 048 576 and 2 097 152).  A short list whose links and ids sit at both ends and on either
    side of every boundary: each chosen link names each chosen node and a few more, so both directions read and write rows out there.
    x and g are zeros but for the rows the list reads."""
    n, F = 2_200_000, 1024
    L = n
    lt.require_free_memory(dev, 5 * n * F * 4, 'the large-offset common-neighbour pool case')
    rng = np.random.RandomState(31)
    bounds = [(1 << 31) // F // 4, (1 << 31) // F // 2, (1 << 31) // F]
    chosen = np.unique(np.concatenate([[0, 1, n - 2, n - 1], [b + d for b in bounds for d in (-1, 0, 1)]]))
    counts = np.zeros(L, dtype=np.int64)
    rows = {}
    for q in chosen:
        rows[q] = np.concatenate([chosen[rng.permutation(len(chosen))], rng.randint(0, n, size=5)])
        counts[q] = len(rows[q])
    rows[chosen[3]] = np.concatenate([rows[chosen[3]], np.full(282, n - 1)])  # 300 entries: a hub row of links, and the last node's group is one of nodes
    counts[chosen[3]] = 300
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = np.concatenate([rows[q] for q in chosen]).astype(np.int64)
    coef = rng.uniform(0.5, 1.5, size=len(ids)).astype(np.float32)
    plan = ssa.CommonNeighbourBatch.from_lists(n, *_to(dev, rowptr, ids, coef))
    groups = np.bincount(ids, minlength=n)
    assert plan.link_hubs[1] == 1 and plan.node_hubs[1] == (groups > 256).sum() == 1 and plan.num_touched == (groups > 0).sum()
    named = np.nonzero(groups)[0]
    hx, hg = cr.features(len(named), F, seed=8), cr.features(len(chosen), F, seed=9)
    x = torch.zeros((n, F), dtype=torch.float32, device=dev)
    assert x.numel() > 1 << 31
    x[torch.from_numpy(named).to(dev)] = torch.from_numpy(hx).to(dev)
    x.requires_grad_(True)
    x_rows = lambda i: hx[np.searchsorted(named, i)]
    g_rows = lambda q: hg[np.searchsorted(chosen, q)]
    tchosen = torch.from_numpy(chosen).to(dev)
    y = ssa.common_neighbour_pool(x, plan)
    assert y.shape == (L, F) and y.numel() > 1 << 31
    _assert_same(y[tchosen], cr.forward_rows(rowptr, ids, coef, x_rows, chosen), 'large forward')
    others = torch.from_numpy(np.setdiff1d(np.concatenate([chosen + 2, chosen - 2]) % L, chosen)).to(dev)
    assert bool((_bits(y[others]) == 0).all())
    g = torch.zeros((L, F), dtype=torch.float32, device=dev)
    g[tchosen] = torch.from_numpy(hg).to(dev)
    y.backward(g)
    del y
    _assert_same(x.grad[torch.from_numpy(named).to(dev)], cr.grad_rows(rowptr, ids, coef, g_rows, named, F), 'large backward')
    unnamed = torch.from_numpy(np.setdiff1d(np.concatenate([chosen + 3, chosen - 3]) % n, named)).to(dev)
    assert bool((_bits(x.grad[unnamed]) == 0).all())
    del x, g, plan
    torch.cuda.empty_cache()
