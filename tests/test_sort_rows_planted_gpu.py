"""ss_csr_sort_rows and sign.group_ids_stable on the planted CSRs and id arrays of sort_rows_planted.py, and the consumers of the
stable grouping (AggrGraph, GCNGraph, LinkBatch, NegativeSampler) on one graph whose hub rows take the merge path.  Every comparison
is exact: integers equal, floats bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import aggr_restatement as ar
import gcn_restatement as gr
import link_decoder_restatement as lr
import negatives_restatement as nr
import sort_rows_planted as P

pytestmark = pytest.mark.gpu

GUARD = 4096            # int32 words of sentinel on either side of col
SENTINEL = -7           # (a negative id: sorts in front of everything if a kernel ever reads it as an entry)
WS_FRONT, WS_BACK = 256, 4096
WS_FILL = 0xA5


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class Launch(object):
    """one CSR on the device: col in the middle of a sentinel-filled buffer, the workspace -- exactly ss_csr_sort_workspace_bytes(E)
    bytes at a 256-byte-aligned address -- in the middle of another"""

    def __init__(self, ssa, dev, rowptr, col):
        self.lib, self.dev = ssa._native.lib(), dev
        self.N, self.E = len(rowptr) - 1, len(col)
        self.rowptr = torch.from_numpy(np.array(rowptr)).to(dev)
        self.buf = torch.full((2 * GUARD + self.E,), SENTINEL, dtype=torch.int32, device=dev)
        self.col = self.buf[GUARD:GUARD + self.E]
        self.col.copy_(torch.from_numpy(np.array(col)))
        self.ws_bytes = self.lib.ss_csr_sort_workspace_bytes(self.E)
        assert self.ws_bytes == P.workspace_bytes(self.E)
        self.ws_buf = torch.full((WS_FRONT + self.ws_bytes + WS_BACK,), WS_FILL, dtype=torch.uint8, device=dev)
        self.ws = self.ws_buf[WS_FRONT:WS_FRONT + self.ws_bytes]
        assert self.ws.data_ptr() % 256 == 0

    def sort(self, only_if=None):
        rc = self.lib.ss_csr_sort_rows(_p(self.rowptr), _p(self.col), self.N, self.E, _p(only_if), _p(self.ws), self.ws_bytes, _st(self.dev))
        assert rc == 0

    def check(self, want, what):
        torch.cuda.synchronize(self.dev)
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.E:] == SENTINEL).all(), f'{what}: a guard of col was written'
        ws = self.ws_buf.cpu().numpy()
        assert (ws[:WS_FRONT] == WS_FILL).all() and (ws[WS_FRONT + self.ws_bytes:] == WS_FILL).all(), f'{what}: bytes around the workspace'
        body = got[GUARD:GUARD + self.E]
        if not np.array_equal(body, want):
            bad = np.nonzero(body != want)[0]
            rows = np.unique(np.searchsorted(self.rowptr.cpu().numpy(), bad, side='right') - 1)
            lens = np.diff(self.rowptr.cpu().numpy())[rows]
            raise AssertionError(f'{what}: {len(bad)} entries differ, in rows {rows[:8].tolist()} of lengths {lens[:8].tolist()}')


# ---- (a) direct launches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(P.VARIANTS))
@pytest.mark.parametrize('pattern', P.PATTERNS)
def test_rows_are_sorted_inside_guarded_buffers(ssa, dev, pattern, variant):
    rowptr, col, want = P.planted(variant, pattern)
    run = Launch(ssa, dev, rowptr, col)
    assert run.N % 4 == (0 if variant == 'n4' else int(variant[4]))
    run.sort()
    run.check(want, 'first call')
    run.sort()
    run.check(want, 'second call')


# ---- (b) only_if ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gated(ssa, dev):
    rowptr, col, want = P.planted('last3_long', 'distinct')
    assert not np.array_equal(col, want)
    return rowptr, col, want


@pytest.mark.parametrize('word', [0, 1, -(1 << 31), -1, None])
def test_only_if_decides(ssa, dev, gated, word):
    rowptr, col, want = gated
    run = Launch(ssa, dev, rowptr, col)
    run.sort(None if word is None else torch.tensor([word], dtype=torch.int32, device=dev))
    run.check(col if word == 0 else want, f'only_if = {word}')


@pytest.mark.parametrize('first,then', [(0, 1), (1, 0)])
def test_only_if_is_read_when_the_launch_runs(ssa, dev, gated, first, then):
    """the word is written before and after the call on the call's own stream: what counts is its value in stream order at the
    launch, neither a value the host could have read at enqueue time nor the last one written"""
    rowptr, col, want = gated
    run = Launch(ssa, dev, rowptr, col)
    word = torch.full((1,), then, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    word.fill_(first)
    run.sort(word)
    word.fill_(then)
    run.check(want if first else col, f'word {first}, call, word {then}')
    assert int(word.item()) == then


# ---- (c) the stable grouping --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', P.GROUPINGS)
def test_group_ids_stable_on_planted_ids(ssa, dev, name):
    ids, n = P.grouping(name)
    want_rowptr, want_order = P.grouping_reference(ids, n)
    wrapped = np.where(ids < 0, ids + n, ids)
    E = len(ids)
    tids = torch.from_numpy(np.array(ids)).to(dev)
    rowptr, order = ssa.sign.group_ids_stable(tids, n)
    assert order.dtype == torch.int32 and rowptr.dtype == torch.int64
    assert np.array_equal(rowptr.cpu().numpy(), want_rowptr)
    assert np.array_equal(order.cpu().numpy().astype(np.int64), want_order)
    # the sort switched off: grouped all the same, each group the same SET of positions
    rowptr0, order0 = ssa.sign.group_ids_stable(tids, n, only_if=torch.zeros(1, dtype=torch.int32, device=dev))
    got = order0.cpu().numpy().astype(np.int64)
    assert np.array_equal(rowptr0.cpu().numpy(), want_rowptr)
    assert np.array_equal(got[np.lexsort((got, wrapped[got]))], want_order)
    # an id outside the range
    for where, value in ((E // 2, n), (E - 1, -n - 1)):
        bad = np.array(ids)
        bad[where] = value
        with pytest.raises(IndexError):
            ssa.sign.group_ids_stable(torch.from_numpy(bad).to(dev), n)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _, order_bad = ssa.sign.group_ids_stable(torch.from_numpy(bad).to(dev), n, err=err)
        assert int(err.item()) != 0
        assert np.array_equal(np.sort(order_bad.cpu().numpy()), np.arange(E))


# ---- (d) the consumers ----------------------------------------------------------------------------------------------------------------
N_NODES = 50_000
HUB_IN, HUB_OUT = 7, 31_337
IN_ARCS, OUT_ARCS = 49_153, 16_385      # 4 chunks with a last chunk of one entry; 2 chunks, one pass, copied back
FS = (4, 20)
FLOWS = ('target', 'source')


class Graph(object):
    """HUB_IN has 49 153 in-arcs from sources drawn with replacement out of 20 000 nodes, HUB_OUT 16 385 out-arcs to targets drawn with
    replacement out of 6 000, 4 000 arcs are random (none into HUB_IN, none out of HUB_OUT); the edge list is shuffled"""

    def __init__(self):
        rng = np.random.RandomState(21)
        # (and so that wedges run through the hubs: 40 arcs into HUB_OUT, 40 out of HUB_IN, one of them to HUB_OUT)
        src = np.concatenate([rng.randint(100, 20_100, size=IN_ARCS), np.full(OUT_ARCS, HUB_OUT), rng.randint(0, HUB_OUT, size=4000),
                              rng.randint(20_100, 30_000, size=40), np.full(40, HUB_IN)])
        dst = np.concatenate([np.full(IN_ARCS, HUB_IN), rng.randint(40_000, 46_000, size=OUT_ARCS), rng.randint(HUB_IN + 1, N_NODES, size=4000),
                              np.full(40, HUB_OUT), [HUB_OUT], rng.randint(30_000, 40_000, size=39)])
        keep = rng.permutation(len(src))
        self.ei = np.stack([src[keep], dst[keep]]).astype(np.int64)
        self.E = self.ei.shape[1]
        self.w = {'unit': None, 'random': rng.uniform(0.25, 2.0, size=self.E).astype(np.float32)}
        deg_in, deg_out = np.bincount(self.ei[1], minlength=N_NODES), np.bincount(self.ei[0], minlength=N_NODES)
        assert deg_in[HUB_IN] == IN_ARCS and deg_out[HUB_OUT] == OUT_ARCS
        pairs = self.ei[0] * N_NODES + self.ei[1]
        assert len(np.unique(pairs[self.ei[1] == HUB_IN])) < IN_ARCS - 1000 and len(np.unique(pairs[self.ei[0] == HUB_OUT])) < OUT_ARCS - 1000
        touched = np.unique(self.ei)
        self.rows = np.concatenate([[HUB_IN, HUB_OUT], rng.choice(touched[(touched != HUB_IN) & (touched != HUB_OUT)], size=62, replace=False),
                                    [0, N_NODES - 1]]).astype(np.int64)
        self.x = ((rng.randint(-512, 512, size=(N_NODES, max(FS))) + rng.uniform(size=(N_NODES, max(FS)))) / 64).astype(np.float32)
        self.g = ((rng.randint(-512, 512, size=(N_NODES, max(FS))) + rng.uniform(size=(N_NODES, max(FS)))) / 64).astype(np.float32)
        self._den = {}

    def den(self, weights, flow):
        if (weights, flow) not in self._den:
            self._den[weights, flow] = ar.den(self.ei, self.w[weights], N_NODES, flow)
        return self._den[weights, flow]


@pytest.fixture(scope='module')
def graph():
    return Graph()


def _assert_same(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} elements differ, first in row {int(np.nonzero(diff.any(axis=-1))[0][0])}'


def _tw(graph, weights, dev):
    return None if graph.w[weights] is None else torch.from_numpy(graph.w[weights]).to(dev)


def _assert_plan_order(rowptr, order, ids):
    want_rowptr, want_order = P.grouping_reference(ids, N_NODES)
    assert np.array_equal(rowptr.cpu().numpy(), want_rowptr)
    assert np.array_equal(order.cpu().numpy().astype(np.int64), want_order)


@pytest.mark.parametrize('weights', ['unit', 'random'])
def test_aggregate_on_merge_path_rows(ssa, dev, graph, weights):
    ei, w = graph.ei, graph.w[weights]
    plan = ssa.AggrGraph(N_NODES, torch.from_numpy(ei).to(dev), _tw(graph, weights, dev))
    _assert_plan_order(plan.target.rowptr, plan.target.order, ei[1])
    _assert_plan_order(plan.source.rowptr, plan.source.order, ei[0])
    rows, trows = graph.rows, torch.from_numpy(graph.rows).to(dev)
    for flow in FLOWS:
        for aggr in ('sum', 'mean'):
            F = max(FS)
            want = ar.propagate_rows(ei, w, N_NODES, lambda ids: graph.x[ids], rows, flow, aggr)
            gd = graph.g / graph.den(weights, flow)[:, None] if aggr == 'mean' else graph.g
            want_grad = ar.propagate_rows(ei, w, N_NODES, lambda ids: gd[ids], rows, ar.OTHER[flow], 'sum')
            for F in FS:  # (the columns of a product do not depend on each other: the first F columns are the case of width F)
                x = torch.from_numpy(graph.x[:, :F].copy()).to(dev).requires_grad_(True)
                y = ssa.aggregate(x, plan, aggr, flow)
                _assert_same(y[trows], want[:, :F], f'aggregate {weights} {flow} {aggr} F={F}')
                y.backward(torch.from_numpy(graph.g[:, :F].copy()).to(dev))
                _assert_same(x.grad[trows], want_grad[:, :F], f'aggregate {weights} {flow} {aggr} F={F}, x.grad')


@pytest.mark.parametrize('weights', ['unit', 'random'])
def test_gcn_product_on_merge_path_rows(ssa, dev, graph, weights):
    ei = graph.ei
    w = np.ones(graph.E, dtype=np.float32) if graph.w[weights] is None else graph.w[weights]
    plan = ssa.GCNGraph(N_NODES, torch.from_numpy(ei).to(dev), _tw(graph, weights, dev))
    _assert_plan_order(plan.rowptr_c, plan.order_c, ei[1])
    _assert_plan_order(plan.rowptr_r, plan.order_r, ei[0])
    rows, trows = graph.rows, torch.from_numpy(graph.rows).to(dev)
    for flow in FLOWS:
        want = gr.propagate_rows(ei, w, N_NODES, lambda ids: graph.x[ids], rows, flow)
        want_grad = gr.propagate_rows(ei, w, N_NODES, lambda ids: graph.g[ids], rows, ar.OTHER[flow])
        for F in FS:
            x = torch.from_numpy(graph.x[:, :F].copy()).to(dev).requires_grad_(True)
            y = ssa.gcn_propagate(x, plan, flow)
            _assert_same(y[trows], want[:, :F], f'gcn {weights} {flow} F={F}')
            y.backward(torch.from_numpy(graph.g[:, :F].copy()).to(dev))
            _assert_same(x.grad[trows], want_grad[:, :F], f'gcn {weights} {flow} F={F}, x.grad')


def test_link_decoder_on_a_merge_path_row(ssa, dev, graph):
    """a batch that names node HUB_OUT in 16 385 slots (as endpoint 0, as endpoint 1 and in self links): its gradient row"""
    rng = np.random.RandomState(22)
    hub = np.stack([np.full(16380, HUB_OUT), rng.randint(0, 3000, size=16380)], axis=1)
    hub[1::2] = hub[1::2, ::-1]
    links = np.concatenate([hub, [[HUB_OUT, HUB_OUT]] * 2, [[5, HUB_OUT]], rng.randint(0, N_NODES, size=(3000, 2))]).astype(np.int64)
    links = links[rng.permutation(len(links))]
    L = len(links)
    assert int((links == HUB_OUT).sum()) == OUT_ARCS
    rows = np.concatenate([[HUB_OUT], links[:16].reshape(-1), [N_NODES - 1]])
    trows, tl = torch.from_numpy(rows).to(dev), torch.from_numpy(links).to(dev)
    plan = ssa.LinkBatch(N_NODES, tl)
    _, want_order = P.grouping_reference(links.reshape(-1), N_NODES)
    assert np.array_equal(plan.order.cpu().numpy().astype(np.int64), want_order)
    g2 = rng.uniform(-4, 4, size=(2 * L, max(FS))).astype(np.float32)
    for F in FS:
        x = torch.from_numpy(graph.x[:, :F].copy()).to(dev).requires_grad_(True)
        g = np.ascontiguousarray(g2[:, :F])
        y = ssa.link_gather(x, plan)
        y.backward(torch.from_numpy(g).to(dev).view(L, 2, F))
        _assert_same(x.grad[trows], lr.grad_rows(links, rows, lambda i: g[i], F), f'gather F={F}, x.grad')
        x.grad = None
        y = ssa.link_hadamard(x, plan)
        y.backward(torch.from_numpy(g[:L].copy()).to(dev))
        _assert_same(x.grad[trows], lr.grad_rows(links, rows, lambda i: g[i], F, lambda i: graph.x[i, :F]), f'product F={F}, x.grad')
    ssa.link_decoder.check_errors()


def test_negative_sampler_on_merge_path_rows(ssa, dev, graph):
    ei = graph.ei
    sampler = ssa.NegativeSampler(N_NODES, torch.from_numpy(ei).to(dev))
    by_row = np.lexsort((ei[1], ei[0]))
    want_rowptr = np.zeros(N_NODES + 1, dtype=np.int64)
    want_rowptr[1:] = np.cumsum(np.bincount(ei[0], minlength=N_NODES))
    assert np.array_equal(sampler.graph.rowptr.cpu().numpy(), want_rowptr)
    col = sampler.graph.col.cpu().numpy()[:graph.E]
    assert np.array_equal(col, ei[1][by_row])
    hub_row = col[want_rowptr[HUB_OUT]:want_rowptr[HUB_OUT + 1]]
    assert len(hub_row) > P.LDS and len(np.unique(hub_row)) < len(hub_row)  # the merge path, on a row with duplicates
    rng = np.random.RandomState(23)
    # the hubs, 25 nodes with an arc into HUB_IN and 25 with an arc into HUB_OUT: wedges pick from the hubs' rows, and every
    # candidate of source HUB_OUT is looked up in its 16 385-entry row
    sources = np.concatenate([[HUB_IN, HUB_OUT], rng.choice(ei[0][ei[1] == HUB_IN], size=25), rng.choice(ei[0][ei[1] == HUB_OUT], size=25)])
    positives = np.stack([sources, np.zeros_like(sources)], axis=1).astype(np.int64)
    for mode in ('same_source', 'wedge'):
        want, unsampled = nr.sample(N_NODES, ei, positives, num_neg=3, mode=mode, seed=5)
        got, info = sampler.sample(torch.from_numpy(positives).to(dev), num_neg=3, mode=mode, seed=5, return_info=True)
        assert np.array_equal(got.cpu().numpy(), want) and info['unsampled'] == unsampled, mode
    sampler.check_errors()
