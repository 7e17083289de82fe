"""aggr.aggregate / SAGEConv / GINConv (csrc/ss_aggr.hip) on the GPU against their restatement (tests/aggr_restatement.py, pinned to
dense float64 matrices and to oracle.spmm by tests/test_aggr_host.py).  Every comparison of kernel output is of bits, forward and
backward: the contract fixes the accumulation order (256-entry chunks summed sequentially, chunk sums added in chunk order), so there
is exactly one right answer, whichever tier a row goes through.  Only the layers' gradients, which pass through torch's matrix
products, are compared within a bound."""
import copy
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

import aggr_restatement as ar
import gcn_restatement as gr
import large_table_helpers as lt
from test_exact_nodes_host import _ba40

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WIDTHS = (4, 8, 20, 64, 256, 260, 1024, 3, 0)  # lane groups of 1, 2, 8 (5 chunks), 16, 64, 64 + a second pass of one chunk, four passes; padded; empty
FLOWS = ('target', 'source')
ROOT = 1.375  # 1 + eps, exact in fp32
HUB_ENTRIES = (256, 512, 1024, 10 ** 9)
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


class Case(object):
    """the planted graph, its plan (default hub_entries), x and g [N, 1024] (the first F
    columns are the x and g of every F: the columns of a product do not depend on each other) and the restatements, computed on
    first use and kept"""

    def __init__(self, ssa, dev, kind):
        self.kind, self.dev = kind, dev
        self.ei, w = ar.planted(kind)
        self.w = None if kind == 'unit' else w
        self.tei = torch.from_numpy(self.ei).to(dev)
        self.tw = None if self.w is None else torch.from_numpy(self.w).to(dev)
        self.plan = ssa.AggrGraph(ar.N, self.tei, self.tw)
        x, g = ar.features(ar.N, 1024, seed=3), ar.features(ar.N, 1024, seed=5)
        gs = np.zeros_like(g)
        rows7 = np.array([0, 11, 25, 700, gr.TWO_LOOPS, 1333, ar.N - 1])  # g non-zero in 7 rows only: the shape node_features[curr_links] gives
        gs[rows7] = g[rows7]
        self.host = {'x': x, 'g': g, 'gs': gs}
        self.x, self.g, self.gs = (torch.from_numpy(a).to(dev) for a in (x, g, gs))
        self.root = torch.tensor([ROOT], dtype=torch.float32, device=dev)
        self._memo = {}

    def forward(self, flow, aggr, root, F=1024):
        key = ('f', flow, aggr, root)
        if key not in self._memo:
            self._memo[key] = ar.aggregate(self.ei, self.w, ar.N, self.host['x'], flow, aggr, ROOT if root else None)
        return self._memo[key][:, :F]

    def backward(self, name, flow, aggr, root, F=1024):
        key = ('b', name, flow, aggr, root)
        if key not in self._memo:
            self._memo[key] = ar.aggregate_grad(self.ei, self.w, ar.N, self.host[name], flow, aggr, ROOT if root else None)
        return self._memo[key][:, :F]


@pytest.fixture(scope='module', params=['unit', 'random'])
def case(request, ssa, dev):
    return Case(ssa, dev, request.param)


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


def test_plan(case, ssa, dev):
    plan = case.plan
    assert plan.num_nodes == ar.N and plan.device == dev and plan.num_edges == case.ei.shape[1] and plan.hub_entries == ssa.aggr.DEFAULT_HUB_ENTRIES
    small = ssa.AggrGraph(ar.N, case.tei, case.tw, hub_entries=256)
    for flow, ids, side, tiny in (('target', case.ei[1], plan.target, small.target), ('source', case.ei[0], plan.source, small.source)):
        want = np.argsort(ids, kind='stable')  # BOTH groupings sorted, unit weights or not: each is an accumulation order
        m = np.bincount(ids, minlength=ar.N)
        assert np.array_equal(side.order.cpu().numpy(), want) and np.array_equal(np.diff(side.rowptr.cpu().numpy()), m)
        _assert_same(side.den, ar.den(case.ei, case.w, ar.N, flow), f'den {flow}')
        _assert_same(tiny.den, side.den, 'den does not depend on hub_entries')
        big = np.nonzero(m > plan.hub_entries)[0]        # at the default, whatever it is: the hubs ascending, their chunks counted off
        assert 1 <= len(big) == side.n_hubs and side.hub_rows.tolist() == big.tolist() and 770 in big
        assert side.hub_chunk.tolist() == [0] + np.cumsum((m[big] + 255) // 256).tolist() and side.n_chunks == side.hub_chunk[-1].item()
        assert side.chunk_hub.tolist() == np.repeat(np.arange(len(big)), (m[big] + 255) // 256).tolist()
        hubs = np.nonzero(m > 256)[0]                    # at hub_entries = 256: 257 .. 2305 entries and the row of 300, 2 .. 10 chunks each
        chunks = (m[hubs] + 255) // 256
        assert sorted(chunks.tolist()) == [2, 2, 2, 2, 3, 3, 4, 4, 5, 10] and (m[hubs] % 256 == 1).sum() == 5  # a last chunk of ONE entry: 257, 513, 769, 1025, 2305
        assert tiny.hub_rows.tolist() == hubs.tolist() and tiny.hub_chunk.tolist() == [0] + np.cumsum(chunks).tolist()
        assert tiny.chunk_hub.tolist() == np.repeat(np.arange(len(hubs)), chunks).tolist() and tiny.n_chunks == chunks.sum()
        assert tiny.hub_rows.dtype == tiny.hub_chunk.dtype == tiny.chunk_hub.dtype == torch.int32
    if case.kind == 'unit':
        assert plan.w is None                            # unit weights are never gathered
        ones = ssa.AggrGraph(ar.N, case.tei, torch.ones(case.ei.shape[1], device=dev))
        _assert_same(ones.target.den, plan.target.den, 'den with explicit ones')
        _assert_same(ssa.aggregate(case.x[:, :8].contiguous(), ones, 'mean'), case.forward('target', 'mean', False, 8), 'explicit ones')
    edited = case.tei.clone()
    private = ssa.AggrGraph(ar.N, edited, case.tw)
    edited[1, 5] = (edited[1, 5] + 1) % ar.N             # the plan keeps a private copy of the edge list
    _assert_same(ssa.aggregate(case.x[:, :8].contiguous(), private), case.forward('target', 'sum', False, 8), 'private copy')


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('root', [False, True])
@pytest.mark.parametrize('aggr', ['sum', 'mean'])
@pytest.mark.parametrize('flow', FLOWS)
def test_forward_and_backward_bits(case, ssa, F, flow, aggr, root):
    x = case.x[:, :F].clone().requires_grad_(True)
    r = case.root.clone().requires_grad_(True) if root else None
    y = ssa.aggregate(x, case.plan, aggr, flow, r)
    assert y.shape == (ar.N, F) and y.dtype == torch.float32 and y.device == x.device
    _assert_same(y, case.forward(flow, aggr, root, F), f'{flow} {aggr} root={root} F={F}')
    for name in ('g', 'gs'):
        g = getattr(case, name)[:, :F]  # (a non-contiguous grad_out unless F = 1024)
        want = case.backward(name, flow, aggr, root, F)
        x.grad = None
        (y * g).sum().backward(retain_graph=True)
        first = x.grad.clone()
        assert first.shape == (ar.N, F)
        _assert_same(first, want, f'{flow} {aggr} root={root} F={F} x.grad for {name}')
        x.grad = None
        (y * g).sum().backward(retain_graph=True)
        _assert_same(x.grad, first, f'{flow} {aggr} root={root} F={F} second backward')
    if root and F:
        want = float(np.sum(case.host['gs'][:, :F].astype(np.float64) * case.host['x'][:, :F].astype(np.float64)))
        size = float(np.sum(np.abs(case.host['gs'][:, :F].astype(np.float64) * case.host['x'][:, :F])))
        r.grad = None
        (y * case.gs[:, :F]).sum().backward()
        assert r.grad.shape == (1,) and abs(float(r.grad) - want) <= (7 * F + 8) * U * size  # (g * x).sum() in torch: 7 F non-zero terms


@pytest.mark.parametrize('hub', HUB_ENTRIES + (None,))
def test_rows_do_not_depend_on_the_tier(case, ssa, hub):
    """the same bits at every hub_entries: at 256 the ten rows of 257 .. 2305 entries (and the 300) are hubs of 2 .. 10 chunks,
    five of them with a last chunk of one entry; at 10^9 nothing is a hub"""
    plan = ssa.AggrGraph(ar.N, case.tei, case.tw, hub_entries=hub)
    assert plan.hub_entries == (ssa.aggr.DEFAULT_HUB_ENTRIES if hub is None else hub)
    assert plan.target.n_hubs == {256: 10, 512: 6, 1024: 2, 2048: 1, 10 ** 9: 0}.get(plan.hub_entries, plan.target.n_hubs) == plan.source.n_hubs
    for F in (20, 260):
        for flow in FLOWS:
            for aggr, root in (('sum', False), ('mean', False), ('sum', True), ('mean', True)):
                x = case.x[:, :F].clone().requires_grad_(True)
                y = ssa.aggregate(x, plan, aggr, flow, case.root if root else None)
                _assert_same(y, case.forward(flow, aggr, root, F), f'hub_entries={hub} {flow} {aggr} root={root} F={F}')
                (y * case.g[:, :F]).sum().backward()
                _assert_same(x.grad, case.backward('g', flow, aggr, root, F), f'hub_entries={hub} {flow} {aggr} root={root} F={F} x.grad')


def test_aggregate_argument_errors(case, ssa):
    plan, x = case.plan, case.x[:, :8]
    for bad in (x.double(), x.half(), x[:, 0], x[None], x[:-1], x.cpu(), x.cpu().numpy()):
        with pytest.raises(ValueError):
            ssa.aggregate(bad, plan)
    for kw in (dict(flow='source_to_target'), dict(aggr='max'), dict(root=1.0), dict(root=case.root.cpu()), dict(root=case.root.double())):
        with pytest.raises(ValueError):
            ssa.aggregate(x, plan, **kw)
    with pytest.raises(ValueError):
        ssa.aggregate(x, case.tei)
    y = ssa.aggregate(x.t().contiguous().t(), plan)  # a non-contiguous x is copied, not refused
    _assert_same(y, case.forward('target', 'sum', False, 8), 'non-contiguous x')
    _assert_same(ssa.aggregate(x.contiguous(), plan, 'add'), y, "'add' is 'sum'")
    with torch.no_grad():
        assert not ssa.aggregate(x, plan).requires_grad


def _chunk_partials(case, flow, x, F):
    """[n_chunks, F]: p_c of every chunk of the rows of more than 256 entries, hubs ascending, in the restatement's arithmetic"""
    dst, src = ar._ends(case.ei, flow)
    wv = np.ones(len(dst), dtype=np.float32) if case.w is None else case.w
    m = np.bincount(dst, minlength=ar.N)
    out = []
    for i in np.nonzero(m > 256)[0]:
        e = np.nonzero(dst == i)[0]
        terms = x[src[e]][:, :F] * wv[e][:, None]
        out += [ar.chunked_sum(terms[a:a + 256]) for a in range(0, len(e), 256)]
    return np.stack(out), m


@pytest.mark.parametrize('F', [4, 20, 260])
def test_direct_launches_into_guarded_rows(case, ssa, dev, F):
    """every launch through the binding into the middle of sentinel-filled buffers, at hub_entries = 256 (hubs of 2 .. 10 chunks): the
    regular launch writes the rows of at most 256 entries and leaves the hub rows and the guard rows alone; the partials launch
    writes its chunk slots exactly, and with one hub struck from the list that hub's slots stay untouched; the finish launch writes
    the hub rows only"""
    lib, guard, st = ssa._native.lib(), 67, _stream(dev)
    plan = ssa.AggrGraph(ar.N, case.tei, case.tw, hub_entries=256)
    x = case.x[:, :F].contiguous()
    for flow, side in (('target', plan.target), ('source', plan.source)):
        want = case.forward(flow, 'mean', True, F)
        partials, m = _chunk_partials(case, flow, case.host['x'], F)
        hub_row = torch.from_numpy(m > 256)
        buf = torch.full((ar.N + 2 * guard, F), SENTINEL, dtype=torch.int32, device=dev)
        out = ctypes.c_void_p(buf.data_ptr() + guard * F * 4)
        rows = lambda: lib.ss_aggr_rows(_p(side.rowptr), _p(side.order), _p(side.other), _p(plan.w), ar.N, 256, _p(x), F, None, _p(side.den),
                                        _p(case.root), _p(x), out, st)
        assert rows() == 0
        torch.cuda.synchronize(dev)
        got = buf.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + ar.N:] == SENTINEL)
        body = got[guard:guard + ar.N]
        assert torch.all(body[hub_row] == SENTINEL)                                               # hub rows untouched
        _assert_same(body[~hub_row].view(torch.float32), want[~hub_row.numpy()], f'regular rows {flow} F={F}')

        C = side.n_chunks
        ws = torch.full((C + 2 * guard, F), SENTINEL, dtype=torch.int32, device=dev)
        wsp = ctypes.c_void_p(ws.data_ptr() + guard * F * 4)
        struck = side.hub_rows.clone()
        struck[3] = -1                                                                            # this hub is not followed ...
        part = lambda hubs: lib.ss_aggr_hub_partials(_p(side.rowptr), _p(side.order), _p(side.other), _p(plan.w), ar.N, _p(hubs), _p(side.hub_chunk),
                                                     _p(side.chunk_hub), side.n_hubs, C, _p(x), F, None, wsp, C * F * 4, st)
        assert part(struck) == 0
        torch.cuda.synchronize(dev)
        got = ws.cpu()
        lo, hi = side.hub_chunk[3].item(), side.hub_chunk[4].item()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + C:] == SENTINEL)
        assert hi - lo >= 2 and torch.all(got[guard + lo:guard + hi] == SENTINEL)                 # ... and its chunk slots stay untouched
        keep = np.r_[0:lo, hi:C]
        _assert_same(got[guard:guard + C][keep].view(torch.float32), partials[keep], f'partials without one hub {flow} F={F}')
        assert part(side.hub_rows) == 0
        torch.cuda.synchronize(dev)
        got = ws.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + C:] == SENTINEL)
        _assert_same(got[guard:guard + C].view(torch.float32), partials, f'partials {flow} F={F}')

        buf.fill_(SENTINEL)
        assert lib.ss_aggr_hub_finish(_p(side.hub_rows), _p(side.hub_chunk), side.n_hubs, C, ar.N, wsp, C * F * 4, F, _p(side.den), _p(case.root), _p(x),
                                      out, st) == 0
        torch.cuda.synchronize(dev)
        got = buf.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + ar.N:] == SENTINEL)
        body = got[guard:guard + ar.N]
        assert torch.all(body[~hub_row] == SENTINEL)                                              # the finish launch writes hub rows only
        _assert_same(body[hub_row].view(torch.float32), want[hub_row.numpy()], f'hub rows {flow} F={F}')
        assert rows() == 0                                                                        # both tiers into one buffer: the whole product
        torch.cuda.synchronize(dev)
        _assert_same(buf[guard:guard + ar.N].view(torch.float32), want, f'both tiers {flow} F={F}')
        assert lib.ss_aggr_rows(_p(side.rowptr), _p(side.order), _p(side.other), _p(plan.w), ar.N, 256, _p(x), F + 1, None, None, None, None, out, None) == -1


def test_nan_rows_reach_only_the_rows_that_gather_them(case, ssa, dev):
    """NaN in whole rows of x (the last row among them: rows past N shadow it; every unused lane of a stretch loads its own row) and
    in the last four columns of F = 260 alone (lanes past the last chunk read it): exactly the outputs the restatement makes NaN are
    NaN, every other element keeps its bits -- in both tiers"""
    F = 260
    x = case.host['x'][:, :F].copy()
    x[[ar.N - 1, gr.IN_NODES[3]]] = np.nan
    x[[0, 1500], 256:] = np.nan
    tx = torch.from_numpy(x).to(dev)
    for hub in (256, 10 ** 9):
        plan = ssa.AggrGraph(ar.N, case.tei, case.tw, hub_entries=hub)
        for flow in FLOWS:
            for aggr, root in (('sum', False), ('mean', True)):
                want = ar.aggregate(case.ei, case.w, ar.N, x, flow, aggr, ROOT if root else None)
                got = ssa.aggregate(tx, plan, aggr, flow, case.root if root else None).cpu().numpy()
                nan = np.isnan(want)
                assert nan.any() and not nan.all(axis=1)[ar.N - 1 if not root else 5] and np.array_equal(np.isnan(got), nan), (hub, flow, aggr)
                assert 0 < nan[:, :256].all(axis=1).sum() < ar.N // 2 and (nan[:, 256:].all(axis=1) & ~nan[:, :256].any(axis=1)).any()
                _assert_same(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), f'beside the NaNs {hub} {flow} {aggr}')


def test_out_of_range_ids_raise_and_are_not_followed(case, ssa, dev):
    """ids outside [0, N), negative ones included, among the entries of the longest rows: the plan raises IndexError, and the
    products, run on the refused plan all the same (both tiers, direct launches), follow none of them (finite everywhere)"""
    ei = case.ei
    hub_in = np.nonzero(ei[1] == 770)[0]
    hub_out = np.nonzero(ei[0] == 770)[0]
    for where, ids in (((0, hub_in[[40, 41, 1700]]), (ar.N, -3, ar.N + (1 << 33))), ((1, hub_out[[7, 130, 2304]]), (-1, ar.N, -(1 << 40))),
                       ((0, hub_in[[2304]]), (ar.N,))):
        bad = case.tei.clone()
        bad[where[0], torch.from_numpy(where[1]).to(dev)] = torch.tensor(ids, device=dev)
        with pytest.raises(IndexError):
            ssa.AggrGraph(ar.N, bad, case.tw)
        with pytest.raises(IndexError):
            ssa.SAGEConv(8, 8).to(dev)(case.x[:, :8].contiguous(), bad)
        for hub in (256, None):
            refused = ssa.AggrGraph.__new__(ssa.AggrGraph)
            with pytest.raises(IndexError):
                refused.__init__(ar.N, bad, case.tw, hub_entries=hub)
            x = case.x[:, :20].contiguous()
            for target in (True, False):
                den = (refused.target if target else refused.source).den
                for y in (refused.product(x, target, mean=True, root=case.root), refused.product(x, not target, root=case.root, gather_den=den)):
                    torch.cuda.synchronize(dev)
                    assert bool(torch.isfinite(y).all())


def test_tiny_graphs(ssa, dev):
    """the empty edge list (sum and mean give zeros, the root term alone remains), N = 1, a single self loop, every edge into one
    node (600 copies: a hub of three chunks)"""
    x = torch.from_numpy(ar.features(5, 12)).to(dev)
    root = torch.tensor([ROOT], device=dev)
    for n in (5, 2, 1):
        empty = ssa.AggrGraph(n, torch.zeros((2, 0), dtype=torch.int64, device=dev))
        for flow in FLOWS:
            for aggr in ('sum', 'mean'):
                xs = x[:n].clone().requires_grad_(True)
                y = ssa.aggregate(xs, empty, aggr, flow)
                _assert_same(y, np.zeros((n, 12), dtype=np.float32), f'no edges, N={n}')
                y.sum().backward()
                _assert_same(xs.grad, np.zeros((n, 12), dtype=np.float32), f'no edges, N={n}, grad')
                _assert_same(ssa.aggregate(x[:n], empty, aggr, flow, root), np.float32(ROOT) * x[:n].cpu().numpy(), f'no edges, N={n}, root')
    star = np.stack([np.arange(600) % 3, np.ones(600, dtype=np.int64)])  # every edge into node 1, self loops among them
    graphs = [(1, [[0], [0]], [3.0]), (1, [[0, 0], [0, 0]], [3.0, 0.5]), (2, [[0, 1, 0], [1, 0, 1]], [0.5, 2.0, 4.0]), (2, [[1], [1]], None),
              (3, star, None), (3, star, np.random.RandomState(2).uniform(0.25, 2, 600))]
    for n, ei, w in graphs:
        ei, w = np.array(ei, dtype=np.int64), (None if w is None else np.array(w, dtype=np.float32))
        for hub in (256, None):
            plan = ssa.AggrGraph(n, torch.from_numpy(ei).to(dev), None if w is None else torch.from_numpy(w).to(dev), hub_entries=hub)
            assert plan.target.n_hubs == (1 if ei.shape[1] > plan.hub_entries else 0)
            for flow in FLOWS:
                for aggr, r in (('sum', None), ('mean', None), ('sum', root)):
                    xs = x[:n].clone().requires_grad_(True)
                    y = ssa.aggregate(xs, plan, aggr, flow, r)
                    _assert_same(y, ar.aggregate(ei, w, n, x[:n].cpu().numpy(), flow, aggr, None if r is None else ROOT), f'N={n} {flow} {aggr}')
                    y.sum().backward()
                    _assert_same(xs.grad, ar.aggregate_grad(ei, w, n, np.ones((n, 12), dtype=np.float32), flow, aggr, None if r is None else ROOT),
                                 f'N={n} {flow} {aggr} grad')


# ---- the layers -------------------------------------------------------------------------------------------------------------------

def _restated(case, t, aggr, root=None):
    """the restated product of a device tensor, back on the device"""
    return torch.from_numpy(ar.aggregate(case.ei, case.w, ar.N, t.detach().cpu().numpy(), 'target', aggr, root)).to(case.dev)


@pytest.mark.parametrize('root_weight', [True, False])
@pytest.mark.parametrize('aggr', ['mean', 'sum'])
def test_sage_layers_equal_the_composition(case, ssa, dev, aggr, root_weight):
    """SAGEConv(20, 64) -> SAGEConv(64, 32): the same bits as lin_l(restated aggregation) + lin_r(x) with the same torch ops around
    the restated product; normalize=True is F.normalize of that"""
    torch.manual_seed(17)
    convs = [ssa.SAGEConv(20, 64, aggr=aggr, root_weight=root_weight).to(dev), ssa.SAGEConv(64, 32, aggr=aggr, root_weight=root_weight).to(dev)]
    x = case.x[:, :20].contiguous()
    with torch.no_grad():
        got, want = x, x
        for c in convs:
            got = c(got, case.plan)
            z = c.lin_l(_restated(case, want, aggr))
            want = z + c.lin_r(want) if root_weight else z
        assert got.shape == (ar.N, 32)
        _assert_same(got, want, f'two SAGE layers {aggr} root_weight={root_weight}')
        if case.kind == 'unit':
            _assert_same(convs[1](convs[0](x, case.tei), case.tei), want, 'two layers on the edge_index tensor')
        convs[1].normalize = True
        _assert_same(convs[1](convs[0](x, case.plan), case.plan), torch.nn.functional.normalize(want, p=2.0, dim=-1), 'normalize=True')


def _mlp(a, b):
    return torch.nn.Sequential(torch.nn.Linear(a, b), torch.nn.BatchNorm1d(b), torch.nn.ReLU(), torch.nn.Linear(b, b))


@pytest.mark.parametrize('train_eps', [False, True])
def test_gin_layers_equal_the_composition(case, ssa, dev, train_eps):
    """GINConv(mlp(20, 64)) -> GINConv(mlp(64, 32)), BatchNorm in training mode: the same bits as nn(restated sum + (1 + eps) x)"""
    torch.manual_seed(19)
    convs = [ssa.GINConv(_mlp(20, 64), eps=0.375, train_eps=train_eps).to(dev), ssa.GINConv(_mlp(64, 32), eps=-0.25, train_eps=train_eps).to(dev)]
    twins = copy.deepcopy(convs)  # (BatchNorm's running statistics move with every forward)
    x = case.x[:, :20].contiguous()
    with torch.no_grad():
        got, want = x, x
        for c, t in zip(convs, twins):
            got = c(got, case.plan)
            want = t.nn(_restated(case, want, 'sum', float(1.0 + t.eps.detach())))
        assert got.shape == (ar.N, 32)
        _assert_same(got, want, f'two GIN layers train_eps={train_eps}')
        _assert_same(convs[0].nn[1].running_mean, twins[0].nn[1].running_mean, 'running mean')


def _gamma_check(what, kind, got, want, scale, k):
    worst = {}
    for name in want:
        err, bound = np.abs(got[name].detach().cpu().numpy().astype(np.float64) - want[name]), k * U / (1 - k * U) * scale[name]
        assert got[name].shape == want[name].shape and np.all(err[bound == 0] == 0), name
        worst[name] = float((err[bound > 0] / bound[bound > 0]).max())
    print(f'[aggr] {kind} weights, {what} gradients, worst error / bound: ' + ', '.join(f'{n} {r:.4f}' for n, r in worst.items()))
    assert max(worst.values()) < 1, worst


def _k_layers(case, layers, width):
    """roundings on a gradient's way through `layers` layers: per layer at most one contraction over the N nodes, one row sum
    (the longest row and its chunk adds), two contractions over `width` channels and 16 elementwise operations"""
    return layers * (ar.N + 2305 + 10 + 2 * width + 16)


@pytest.mark.parametrize('aggr', ['mean', 'sum'])
def test_sage_gradients_against_float64(case, ssa, dev, aggr):
    """loss = <h2, G> over two layers: every parameter's gradient and x.grad within gamma_k of the float64 evaluation of the same
    model on the dense matrix (the fp32 den taken as exact), against the same evaluation on magnitudes"""
    torch.manual_seed(23)
    convs = [ssa.SAGEConv(20, 64, aggr=aggr).to(dev), ssa.SAGEConv(64, 32, aggr=aggr).to(dev)]
    x = case.x[:, :20].clone().requires_grad_(True)
    G = case.gs[:, :32].contiguous()
    h = x
    for c in convs:
        h = c(h, case.plan)
    (h * G).sum().backward()
    A, M, _, _ = ar.dense(case.ei, case.w, ar.N)
    dinv = 1.0 / ar.den(case.ei, case.w, ar.N, 'target').astype(np.float64) if aggr == 'mean' else np.ones(ar.N)
    names = ['x'] + [f'{i}.{n}' for i, c in enumerate(convs) for n, _ in c.named_parameters()]
    real = [x] + [p for c in convs for p in c.parameters()]

    def grads(P, magnitudes):
        f = lambda t: torch.from_numpy(np.abs(t) if magnitudes else t)
        leaves = [f(t.detach().cpu().numpy().astype(np.float64)).requires_grad_(True) for t in real]
        it = iter(leaves[1:])
        P, h = f(P) * torch.from_numpy(dinv)[:, None], leaves[0]
        for c in convs:
            wl, bl, wr = next(it), next(it), next(it)
            h = (P @ h) @ wl.T + bl + h @ wr.T
        (h * f(G.cpu().numpy().astype(np.float64))).sum().backward()
        return {n: t.grad.numpy() for n, t in zip(names, leaves)}

    _gamma_check(f'SAGE {aggr}', case.kind, dict(zip(names, [t.grad for t in real])), grads(A.T, False), grads(M.T, True), _k_layers(case, 2, 64))


@pytest.mark.parametrize('train_eps', [False, True])
def test_gin_gradients_against_float64(case, ssa, dev, train_eps):
    """one GINConv around Linear -> BatchNorm -> ReLU -> Linear, BatchNorm in evaluation mode with planted statistics (an affine map,
    so the evaluation on magnitudes is defined; the ReLU pattern is the float64 forward's): every parameter's gradient, the eps
    gradient and x.grad within gamma_k"""
    torch.manual_seed(29)
    conv = ssa.GINConv(_mlp(20, 64), eps=0.375, train_eps=train_eps).to(dev)
    bn = conv.nn[1]
    with torch.no_grad():
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    conv.eval()
    x = case.x[:, :20].clone().requires_grad_(True)
    G = case.gs[:, :64].contiguous()
    (conv(x, case.plan) * G).sum().backward()
    A, M, _, _ = ar.dense(case.ei, case.w, ar.N)
    names = ['x', 'eps', 'nn.0.weight', 'nn.0.bias', 'nn.1.weight', 'nn.1.bias', 'nn.3.weight', 'nn.3.bias']
    real = [x, conv.eps, conv.nn[0].weight, conv.nn[0].bias, bn.weight, bn.bias, conv.nn[3].weight, conv.nn[3].bias]
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    inv_std = torch.from_numpy(1.0 / np.sqrt(f64(bn.running_var) + bn.eps))
    mean = torch.from_numpy(f64(bn.running_mean))

    def grads(P, magnitudes, mask=None):
        f = lambda t: torch.from_numpy(np.abs(t) if magnitudes else t)
        xs, eps, w0, b0, g1, b1, w3, b3 = leaves = [f(f64(t)).requires_grad_(True) for t in real]
        one = 1.0 if not magnitudes else abs(1.0 + float(conv.eps.detach())) - abs(float(conv.eps.detach()))  # |1 + eps| as a function of |eps|
        a = f(P) @ xs + (one + eps) * xs
        pre = a @ w0.T + b0
        z = (pre + mean.abs()) * inv_std * g1 + b1 if magnitudes else (pre - mean) * inv_std * g1 + b1
        mask = (z > 0).to(torch.float64).detach() if mask is None else mask
        out = (z * mask) @ w3.T + b3
        (out * f(f64(G))).sum().backward()
        return {n: (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))) for n, t in zip(names, leaves)}, mask

    want, mask = grads(A.T, False)
    scale, _ = grads(M.T, True, mask)
    got = dict(zip(names, [t.grad for t in real]))
    if not train_eps:
        assert conv.eps.grad is None and not conv.eps.requires_grad
        for d in (want, scale, got):
            del d['eps']
    _gamma_check(f'GIN train_eps={train_eps}', case.kind, got, want, scale, _k_layers(case, 1, 64))


def test_seal_shaped_steps_repeat_bit_for_bit(ssa, dev):
    """a SEAL-shaped step on a BA-40 exact_subgraphs batch: from_subgraphs -> Embedding(z) -> SAGEConv x 2 -> center_pool (SEALSAGE,
    reference models/seal.py:116-173) and GINConv x 2 -> global_mean_pool (SEALGIN, :259-328), then backward: two runs give identical
    bits for the outputs and for every gradient"""
    n, ei, links = _ba40()
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    sg = eh.exact_subgraphs(torch.from_numpy(links).to(dev), n, torch.from_numpy(ei).to(dev))
    T, L = sg.ids.numel(), sg.num_links
    assert T > 100 and int(sg.weight.max()) >= 1 and sg.z.shape == (T,)
    graph = ssa.AggrGraph.from_subgraphs(sg)
    assert graph.num_nodes == T and graph.num_edges == sg.nbr.numel() and graph.w is not None
    sei, sw = sg.edge_index().cpu().numpy(), sg.weight.float().cpu().numpy()
    xs = torch.from_numpy(ar.features(T, 8, seed=4)).to(dev)
    _assert_same(ssa.aggregate(xs, graph, 'mean'), ar.aggregate(sei, sw, T, xs.cpu().numpy(), 'target', 'mean'), 'the batch plan against the restatement')
    torch.manual_seed(31)
    emb = torch.nn.Embedding(int(sg.z.max()) + 1, 32).to(dev)
    sage = torch.nn.ModuleList([ssa.SAGEConv(32, 32), ssa.SAGEConv(32, 32)]).to(dev)
    gin = torch.nn.ModuleList([ssa.GINConv(_mlp(32, 32), train_eps=True), ssa.GINConv(_mlp(32, 32), train_eps=True)]).to(dev)
    head_s, head_g = torch.nn.Linear(32, 1).to(dev), torch.nn.Linear(32, 1).to(dev)
    label = (torch.arange(L, device=dev) % 2).float()

    def step(kind):
        for m in (emb, sage, gin, head_s, head_g):
            m.zero_grad(set_to_none=True)
        h = emb(sg.z)
        if kind == 'sage':
            for c in sage:
                h = torch.relu(c(h, graph))
            out = head_s(ssa.center_pool(h, sg))
            params = [emb.weight] + list(sage.parameters()) + list(head_s.parameters())
        else:
            for c in gin:
                h = c(h, graph)
            out = head_g(ssa.global_mean_pool(h, sg))
            params = [emb.weight] + list(gin.parameters()) + list(head_g.parameters())
        torch.nn.functional.binary_cross_entropy_with_logits(out.view(-1), label).backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
        return [out.detach().clone()] + [p.grad.detach().clone() for p in params]

    for kind in ('sage', 'gin'):
        first, second = step(kind), step(kind)
        assert len(first) == len(second) > 6
        for i, (a, b) in enumerate(zip(first, second)):
            _assert_same(a, b, f'{kind} run 2 against run 1, tensor {i}')
    with pytest.raises(NotImplementedError):
        sage[0](emb(sg.z), sg.edge_index(), sg.weight.float())  # multiplicities come in through an AggrGraph ...
    with torch.no_grad():
        _assert_same(sage[0](emb(sg.z), sg), sage[0](emb(sg.z), graph), 'the batch itself as edge_index')  # ... or through the batch


def test_cache(case, ssa, dev):
    torch.manual_seed(37)
    convs = [ssa.SAGEConv(20, 64).to(dev), ssa.GINConv(torch.nn.Linear(64, 64)).to(dev)]
    gcn = ssa.GCNConv(20, 20).to(dev)
    x = case.x[:, :20].contiguous()
    ei = case.tei.clone()
    unit = Case.__new__(Case)
    unit.ei, unit.w, unit.dev = case.ei, None, dev
    with torch.no_grad():
        before, gcn_before = ssa.AggrGraph.builds, ssa.GCNGraph.builds
        first = convs[1](convs[0](x, ei), ei)
        assert ssa.AggrGraph.builds == before + 1                    # two layers fed one tensor: one build
        again = convs[1](convs[0](x, ei), ei)
        assert ssa.AggrGraph.builds == before + 1
        _assert_same(again, first, 'cached plan')
        gcn(x, ei)
        gcn(x, ei)
        assert ssa.GCNGraph.builds == gcn_before + 1 and ssa.AggrGraph.builds == before + 1  # the GCN cache keeps its own plan of the same tensor
        convs[0](x, ei)
        assert ssa.AggrGraph.builds == before + 1 and ssa.GCNGraph.builds == gcn_before + 1  # ... and neither evicts the other
        convs[0](x, case.plan)
        assert ssa.AggrGraph.builds == before + 1                    # a plan never builds
        fresh = ei.clone()
        same = convs[1](convs[0](x, fresh), fresh)
        assert ssa.AggrGraph.builds == before + 2                    # a fresh tensor of equal content rebuilds ...
        _assert_same(same, first, 'fresh equal tensor')              # ... and gives the same
        victim = int(np.nonzero(case.ei[1] == gr.IN_NODES[5])[0][2])
        fresh[1, victim] = gr.IN_NODES[0]                            # an in-place edit: node 10 gains its first in-edge
        edited = convs[0](x, fresh)
        assert ssa.AggrGraph.builds == before + 3
        unit.ei = case.ei.copy()
        unit.ei[1, victim] = gr.IN_NODES[0]
        want = convs[0].lin_l(_restated(unit, x, 'mean')) + convs[0].lin_r(x)
        _assert_same(edited, want, 'edited graph')
        convs[1](edited, fresh)
        assert ssa.AggrGraph.builds == before + 3
        gcn(x, fresh)
        assert ssa.GCNGraph.builds == gcn_before + 2 and ssa.AggrGraph.builds == before + 3


# ---- offsets past 2^31 elements ---------------------------------------------------------------------------------------------------

def _formula(ids, F):
    """x[i, j] = ((131 i + 7 j) mod 1021 - 510) / 64: exact in fp32, the same numbers on the host and on the device"""
    v = (131 * np.asarray(ids, dtype=np.int64)[:, None] + 7 * np.arange(F, dtype=np.int64)[None, :]) % 1021 - 510
    return (v.astype(np.float32) / np.float32(64)).astype(np.float32)


def test_offsets_past_two_to_the_31_elements(ssa, dev):
    """N = 2 200 000, F = 1 024: x and out hold 2.25e9 elements (9.0 GB each), so element offsets pass 2^31 and byte offsets 2, 4 and
    8 GiB (rows 524 288, 1 048 576, 2 097 152).  A directed ring plus edges between the last 64 rows and the rows around every
    boundary, both ways, and one hub past the 8 GiB boundary with 700 entries from all over the graph (three chunks at
    hub_entries = 512); 256 sampled rows of both flows, the hub among them, against the restatement evaluated on those rows."""
    n, F = 2_200_000, 1024
    lt.require_free_memory(dev, 3 * n * F * 4, 'the large-offset aggregation case')
    bounds = [(1 << 31) // F // 4, (1 << 31) // F // 2, (1 << 31) // F]
    near = np.array([0] + [b + d for b in bounds for d in (-1, 0, 1)], dtype=np.int64)
    last = np.arange(n - 64, n, dtype=np.int64)
    ring = np.arange(n, dtype=np.int64)
    a, b = np.repeat(near, 64), np.tile(last, len(near))
    rng = np.random.RandomState(23)
    hub = bounds[2] + 1000
    far = rng.choice(n, size=700, replace=False).astype(np.int64)
    ei = np.concatenate([np.stack([ring, (ring + 1) % n]), np.stack([a, b]), np.stack([b, a]), np.stack([far, np.full(700, hub)]),
                         np.stack([np.full(700, hub), far])], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    w = rng.uniform(0.5, 1.5, size=ei.shape[1]).astype(np.float32)
    must = np.unique(np.concatenate([near, [1, n - 65, n - 64, n - 2, n - 1, hub, hub + 1]]))  # the first, the last, either side of every boundary, the hub
    spread = rng.choice(n, size=400, replace=False)
    past = bounds[2] + 2 + rng.choice(n - bounds[2] - 2, size=40, replace=False)  # 40 rows past 2^31 elements
    fill = np.setdiff1d(np.concatenate([past, spread, far[:30]]), must, assume_unique=False)
    rows = np.sort(np.concatenate([must, rng.permutation(fill)[:256 - len(must)]]))
    assert len(rows) == 256 == len(np.unique(rows)) and rows[0] == 0 and rows[-1] == n - 1 and (rows > bounds[2]).sum() >= 8
    plan = ssa.AggrGraph(n, torch.from_numpy(ei).to(dev), torch.from_numpy(w).to(dev), hub_entries=512)
    assert plan.target.hub_rows.tolist() == [hub] == plan.source.hub_rows.tolist() and plan.target.n_chunks == 3
    x = torch.empty((n, F), dtype=torch.float32, device=dev)
    assert x.numel() > 1 << 31
    cols = 7 * torch.arange(F, dtype=torch.int32, device=dev)[None, :]
    for r0 in range(0, n, 1 << 18):
        ids = torch.arange(r0, min(r0 + (1 << 18), n), dtype=torch.int32, device=dev)[:, None]
        x[r0:r0 + (1 << 18)] = ((131 * ids + cols) % 1021 - 510).to(torch.float32) / 64
    trows = torch.from_numpy(rows).to(dev)
    _assert_same(x[trows], _formula(rows, F), 'the formula on the device')
    root = torch.tensor([ROOT], device=dev)
    for flow, aggr, r in (('target', 'mean', None), ('source', 'sum', root)):
        y = ssa.aggregate(x, plan, aggr, flow, r)
        got = y[trows].cpu()
        del y
        want = ar.propagate_rows(ei, w, n, lambda ids: _formula(ids, F), rows, flow, aggr, None if r is None else ROOT)
        _assert_same(got, want, f'large {flow} {aggr}')
    del x, plan
    torch.cuda.empty_cache()
