"""What aggr.aggregate / SAGEConv / GINConv promise that needs no device: the restatement the GPU tests compare against
(tests/aggr_restatement.py) is pinned to dense float64 matrices and to oracle.spmm, the planted graph has the rows it is meant to
have, the header and the binding carry the new symbols, the layers have PyG's parameter names and torch.nn.Linear's initialisation,
and the byte model is counted by hand."""
import math
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from oracle import oracle

import aggr_restatement as ar
import gcn_restatement as gr

U = 2.0 ** -24
FLOWS = ('target', 'source')


@pytest.fixture(scope='module', params=['unit', 'random'])
def graph(request):
    ei, w = ar.planted(request.param)
    return request.param, ei, (None if request.param == 'unit' else w), w


def test_planted_graph_has_its_rows(graph):
    kind, ei, w, w_all = graph
    indeg, outdeg = np.bincount(ei[1], minlength=ar.N), np.bincount(ei[0], minlength=ar.N)
    assert tuple(indeg[list(ar.HUBS)]) == ar.BIG and tuple(outdeg[list(ar.HUBS)]) == ar.BIG  # exactly, in both directions
    assert set(ar.BIG) == {255, 256, 257, 511, 512, 513, 767, 769, 1024, 1025, 2305}
    assert ar.HUBS[0] == 0 and ar.HUBS[-1] == ar.N - 1 and ar.HUBS[2] == ar.HUBS[1] + 1       # first id, last id, two side by side
    assert indeg.max() == 2305 and ei.min() == 0 and ei.max() == ar.N - 1
    # the rows of gcn_restatement.planted are still there (self loops COUNT now: node TWO_LOOPS has its two loops and one more in-edge)
    assert tuple(indeg[list(gr.IN_NODES)]) == gr.PROFILE and tuple(outdeg[list(gr.OUT_NODES)]) == gr.PROFILE
    assert indeg[gr.TWO_LOOPS] == 3 and ((ei[0] == gr.TWO_LOOPS) & (ei[1] == gr.TWO_LOOPS)).sum() == 2
    pairs = ei[0] * ar.N + ei[1]
    assert len(np.unique(pairs)) < len(pairs)                                                 # duplicate edges
    hub = ar.HUBS[ar.BIG.index(2305)]
    assert len(np.unique(ei[0][ei[1] == hub])) < 2305                                         # the longest row repeats sources
    assert (indeg == 0).sum() > 100 and (outdeg == 0).sum() > 100                             # rows without entries
    order = np.argsort(ei[1], kind='stable')
    assert (np.diff(ei[1][order]) < 0).sum() == 0 and (np.diff(order)[np.diff(ei[1][order]) == 0] > 0).all()
    assert (np.diff(ei[1]) < 0).any()                                                         # the edge list itself is shuffled
    if kind == 'unit':
        assert np.all(w_all == 1)
    else:
        assert (w_all != 1).any() and w_all.min() >= 0.25 and np.all(ar.den(ei, w, ar.N, 'target') > 0)


def _k(m):
    """the rounding count of an output element of a row of m entries: every term passes at most m - 1 adds inside its chunk and
    ceil(m / 256) chunk adds, and carries its own product, the gather's division, the mean's division and the root's add (the root
    term itself: one product and that add)"""
    return m + np.ceil(m / ar.C) + 4


@pytest.mark.parametrize('root', [None, 1.375])
@pytest.mark.parametrize('aggr', ['sum', 'mean'])
@pytest.mark.parametrize('flow', FLOWS)
def test_restatement_against_dense_float64(graph, flow, aggr, root):
    """forward (A x, A^T x, D^-1 A^T x, D_r^-1 A x, each + r x) and the restated backward (the transposed product of g, or of
    g / den) within gamma_k (|A| @ |x|), k = m + ceil(m / 256) + 4, the fp32 den taken as an exact number"""
    kind, ei, w, _ = graph
    x, g = ar.features(ar.N, 8), ar.features(ar.N, 8, seed=5)
    A, M, per_row, per_col = ar.dense(ei, w, ar.N)
    P, PM, m, mt = (A, M, per_row, per_col) if flow == 'source' else (A.T, M.T, per_col, per_row)
    d = ar.den(ei, w, ar.N, flow).astype(np.float64) if aggr == 'mean' else np.ones(ar.N)
    r = 0.0 if root is None else root
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    cases = {'forward': (ar.aggregate(ei, w, ar.N, x, flow, aggr, root), (P @ x64) / d[:, None] + r * x64,
                         (PM @ np.abs(x64)) / d[:, None] + abs(r) * np.abs(x64), m),
             'backward': (ar.aggregate_grad(ei, w, ar.N, g, flow, aggr, root), P.T @ (g64 / d[:, None]) + r * g64,
                          PM.T @ np.abs(g64 / d[:, None]) + abs(r) * np.abs(g64), mt)}
    for name, (got, want, scale, entries) in cases.items():
        k = _k(entries.astype(np.float64)) * U
        bound = (k / (1 - k))[:, None] * scale
        err = np.abs(got.astype(np.float64) - want)
        worst = float((err[scale > 0] / bound[scale > 0]).max())
        print(f'[aggr] {kind} {flow} {aggr} root={root} {name}: worst error / bound = {worst:.3f}')
        assert got.dtype == np.float32 and worst < 1 and np.all(err[scale == 0] == 0)


@pytest.mark.parametrize('root', [None, 1.375])
@pytest.mark.parametrize('aggr', ['sum', 'mean'])
def test_flows_are_adjoint(graph, aggr, root):
    """<aggregate(x), g> = <x, aggregate_grad(g)>: exactly so in float64 on the dense matrix, and for the float32 restatements
    within the rounding of the two sums (the longest row has 2305 entries)"""
    kind, ei, w, _ = graph
    A, M, _, _ = ar.dense(ei, w, ar.N)
    x, g = ar.features(ar.N, 5, seed=1), ar.features(ar.N, 5, seed=2)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    r = 0.0 if root is None else root
    for flow in FLOWS:
        P, PM = (A, M) if flow == 'source' else (A.T, M.T)
        d = ar.den(ei, w, ar.N, flow).astype(np.float64) if aggr == 'mean' else np.ones(ar.N)
        size = np.sum(((PM @ np.abs(x64)) / d[:, None] + abs(r) * np.abs(x64)) * np.abs(g64))
        lhs = np.sum(((P @ x64) / d[:, None] + r * x64) * g64)
        rhs = np.sum(x64 * (P.T @ (g64 / d[:, None]) + r * g64))
        assert abs(lhs - rhs) <= 1e-12 * size
        l32 = np.sum(ar.aggregate(ei, w, ar.N, x, flow, aggr, root).astype(np.float64) * g64)
        r32 = np.sum(x64 * ar.aggregate_grad(ei, w, ar.N, g, flow, aggr, root).astype(np.float64))
        assert abs(l32 - r32) <= 2 * _k(2305.0) * U * size


def test_short_rows_are_the_sequential_sum(graph):
    """a row of at most 256 entries equals oracle.spmm over the whole edge list bit for bit; chunked_sum of exactly 256 terms is the
    plain loop; the longest row is NOT the plain sequential sum (the chunking is visible)"""
    kind, ei, w, w_all = graph
    x = ar.features(ar.N, 16)
    for flow in FLOWS:
        dst, src = ar._ends(ei, flow)
        plain = oracle.spmm(np.stack([dst, src]), w_all, ar.N, x)
        got = ar.sum_product(ei, w, ar.N, x, flow)
        m = np.bincount(dst, minlength=ar.N)
        assert (m == 256).any() and (m == 255).any() and (m == 257).any()
        assert np.array_equal(got[m <= ar.C].view(np.uint32), plain[m <= ar.C].view(np.uint32))
        assert not np.array_equal(got[m == 2305].view(np.uint32), plain[m == 2305].view(np.uint32))
    t = ar.features(256, 4, seed=9)
    acc = np.zeros(4, dtype=np.float32)
    for row in t:
        acc = acc + row
    assert np.array_equal(ar.chunked_sum(t).view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(ar.chunked_sum(t[:0]).view(np.uint32), np.zeros(4, dtype=np.uint32))  # no entries: +0


def test_rows_restatement_is_the_restatement(graph):
    kind, ei, w, _ = graph
    x = ar.features(ar.N, 4)
    rows = np.array([0, 10, 25, 55, 333, gr.TWO_LOOPS, 700, 701, 770, ar.N - 1])
    for flow in FLOWS:
        for aggr, root in (('sum', None), ('mean', None), ('sum', 0.75), ('mean', 1.5)):
            full = ar.aggregate(ei, w, ar.N, x, flow, aggr, root)
            part = ar.propagate_rows(ei, w, ar.N, lambda ids: x[ids], rows, flow, aggr, root)
            assert np.array_equal(full[rows].view(np.uint32), part.view(np.uint32)), (flow, aggr, root)


def test_den_is_the_count_for_unit_weights():
    ei, _ = ar.planted('unit')
    for flow in FLOWS:
        dst, _ = ar._ends(ei, flow)
        m = np.bincount(dst, minlength=ar.N)
        assert np.array_equal(ar.den(ei, None, ar.N, flow), np.maximum(m, 1).astype(np.float32))


def test_header_and_binding_have_the_symbols():
    import subgraph_sketching_amd as ssa
    sig = ssa._native.SIGNATURES
    for name, n_args in (('ss_aggr_degree', 6), ('ss_aggr_rows', 14), ('ss_aggr_hub_partials', 16), ('ss_aggr_hub_finish', 13),
                         ('ss_aggr_workspace_bytes', 2)):
        assert name in sig and len(sig[name][1]) == n_args, name
    assert ssa.SAGEConv is ssa.aggr.SAGEConv and ssa.GINConv is ssa.aggr.GINConv and ssa.aggregate is ssa.aggr.aggregate
    assert ssa.AggrGraph is ssa.aggr.AggrGraph
    lib = ssa._native.lib()
    assert lib.ss_aggr_chunk() == 256 == ssa.aggr.AGGR_CHUNK == ar.C and sig['ss_aggr_chunk'][1] == []
    assert lib.ss_aggr_workspace_bytes(7, 260) == 7 * 260 * 4 and lib.ss_aggr_workspace_bytes(0, 8) == 0
    assert lib.ss_aggr_workspace_bytes(7, 6) == 0 and lib.ss_aggr_workspace_bytes(-1, 8) == 0 and lib.ss_aggr_workspace_bytes(7, 0) == 0


def test_c_abi_rejects_bad_arguments_on_the_host():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(16)  # never dereferenced: every call below ends in the host-side checks

    def sweep(fn, ok, needed, bad_values, nothing_to_do):
        for i in needed:
            assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == -1, (fn.__name__, i)
        for i, bad in bad_values:
            assert fn(*[bad if j == i else a for j, a in enumerate(ok)]) == -1, (fn.__name__, i, bad)
        for i in nothing_to_do:  # (no nodes / no chunks / no hubs: SS_OK before any pointer is looked at)
            assert fn(*[0 if j == i else (None if isinstance(a, c_void_p) else a) for j, a in enumerate(ok)]) == 0, (fn.__name__, i)

    #             rowptr order other w     N  hub x     F  gden  den   root  root_x out   stream
    sweep(lib.ss_aggr_rows, [fake, fake, fake, fake, 5, 64, fake, 8, fake, fake, fake, fake, fake, None], (0, 1, 2, 6, 11, 12),
          ((4, -1), (4, 1 << 31), (5, 0), (5, -3), (7, 0), (7, -4), (7, 6)), (4,))
    #                 rowptr order other w     N  hubs  chunk c_hub nh nc x     F  gden  ws    bytes    stream
    sweep(lib.ss_aggr_hub_partials, [fake, fake, fake, fake, 5, fake, fake, fake, 2, 3, fake, 8, fake, fake, 3 * 32, None],
          (0, 1, 2, 5, 6, 7, 10, 13), ((4, -1), (4, 1 << 31), (8, -1), (8, 4), (9, -1), (9, 1 << 31), (11, 0), (11, 6), (14, 3 * 32 - 1)), (4,))
    assert lib.ss_aggr_hub_partials(None, None, None, None, 5, None, None, None, 0, 0, None, 8, None, None, 0, None) == 0  # no chunks
    #                 hubs  chunk nh nc N  ws    bytes   F  den   root  root_x out   stream
    sweep(lib.ss_aggr_hub_finish, [fake, fake, 2, 3, 5, fake, 3 * 32, 8, fake, fake, fake, fake, None],
          (0, 1, 5, 10, 11), ((2, -1), (2, 4), (3, -1), (4, -1), (4, 1 << 31), (6, 3 * 32 - 1), (7, 0), (7, 6)), (2, 4))
    #                 rowptr order w     N  den   stream
    sweep(lib.ss_aggr_degree, [fake, fake, fake, 5, fake, None], (0, 1, 4), ((3, -1), (3, 1 << 31)), (3,))
    assert lib.ss_version() == 129  # (new entry points, no changed one: the ABI number stays)


@pytest.mark.parametrize('device', ['cpu', 'meta'])
def test_sage_parameters(device):
    import subgraph_sketching_amd as ssa
    with torch.device(device):
        conv = ssa.SAGEConv(20, 64)
        bare = ssa.SAGEConv(64, 32, aggr='add', root_weight=False, bias=False)
    assert sorted(conv.state_dict()) == ['lin_l.bias', 'lin_l.weight', 'lin_r.weight']
    assert sorted(bare.state_dict()) == ['lin_l.weight'] and not hasattr(bare, 'lin_r') and bare.lin_l.bias is None
    assert conv.lin_l.weight.shape == (64, 20) and conv.lin_r.weight.shape == (64, 20) and conv.lin_l.bias.shape == (64,)
    assert conv.lin_r.bias is None and conv.lin_l.weight.device.type == device and conv.lin_l.weight.dtype == torch.float32
    assert all(p.requires_grad for p in conv.parameters())
    assert (conv.in_channels, conv.out_channels, conv.aggr, bare.aggr) == (20, 64, 'mean', 'sum') and repr(conv) == 'SAGEConv(20, 64, aggr=mean)'
    if device == 'cpu':
        bound = 1 / math.sqrt(20)  # torch.nn.Linear: kaiming_uniform(a = sqrt 5) = U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), the bias too
        for wt in (conv.lin_l.weight.detach(), conv.lin_r.weight.detach()):
            assert float(wt.abs().max()) <= bound and float(wt.abs().max()) > 0.9 * bound and abs(float(wt.mean())) < 0.1 * bound
            assert abs(float(wt.std()) - bound / math.sqrt(3)) < 0.1 * bound
        assert float(conv.lin_l.bias.detach().abs().max()) <= bound
        with torch.no_grad():
            for p in conv.parameters():
                p.fill_(7.0)
        conv.reset_parameters()
        assert all(float(p.detach().abs().max()) <= bound for p in conv.parameters())


@pytest.mark.parametrize('device', ['cpu', 'meta'])
def test_gin_parameters(device):
    import subgraph_sketching_amd as ssa
    with torch.device(device):
        mlp = lambda: torch.nn.Sequential(torch.nn.Linear(20, 32), torch.nn.BatchNorm1d(32), torch.nn.ReLU(), torch.nn.Linear(32, 32))
        fixed, trained = ssa.GINConv(mlp()), ssa.GINConv(mlp(), eps=0.25, train_eps=True)
    keys = ['eps', 'nn.0.bias', 'nn.0.weight', 'nn.1.bias', 'nn.1.num_batches_tracked', 'nn.1.running_mean', 'nn.1.running_var', 'nn.1.weight',
            'nn.3.bias', 'nn.3.weight']
    assert sorted(fixed.state_dict()) == keys == sorted(trained.state_dict())
    assert fixed.eps.shape == (1,) and not isinstance(fixed.eps, torch.nn.Parameter) and 'eps' in dict(fixed.named_buffers())
    assert isinstance(trained.eps, torch.nn.Parameter) and trained.eps.requires_grad and 'eps' in dict(trained.named_parameters())
    if device == 'cpu':
        assert float(fixed.eps) == 0.0 and float(trained.eps.detach()) == 0.25
        with torch.no_grad():
            trained.eps.fill_(3.0)
            trained.nn[0].weight.fill_(7.0)
            trained.nn[1].running_mean.fill_(7.0)
        trained.reset_parameters()
        assert float(trained.eps.detach()) == 0.25 and float(trained.nn[0].weight.detach().abs().max()) <= 1 / math.sqrt(20)
        assert torch.all(trained.nn[1].running_mean == 0)


def test_layers_load_pyg_state_dicts():
    import subgraph_sketching_amd as ssa
    conv = ssa.SAGEConv(20, 64)
    state = {'lin_l.weight': torch.full((64, 20), 0.25), 'lin_l.bias': torch.arange(64, dtype=torch.float32), 'lin_r.weight': torch.full((64, 20), -0.5)}
    assert conv.load_state_dict(state, strict=True).missing_keys == []
    assert torch.all(conv.lin_l.weight == 0.25) and torch.all(conv.lin_r.weight == -0.5) and torch.equal(conv.lin_l.bias.detach(), state['lin_l.bias'])
    with pytest.raises(RuntimeError):
        ssa.SAGEConv(20, 64, root_weight=False).load_state_dict(state, strict=True)
    gin = ssa.GINConv(torch.nn.Sequential(torch.nn.Linear(4, 4)), train_eps=True)
    state = {'nn.0.weight': torch.eye(4), 'nn.0.bias': torch.zeros(4), 'eps': torch.tensor([0.5])}
    assert gin.load_state_dict(state, strict=True).missing_keys == [] and float(gin.eps.detach()) == 0.5
    fixed = ssa.GINConv(torch.nn.Sequential(torch.nn.Linear(4, 4)))
    assert fixed.load_state_dict(state, strict=True).missing_keys == [] and float(fixed.eps) == 0.5  # (PyG keeps eps in the state dict either way)


def test_layers_reject_what_is_not_built():
    import subgraph_sketching_amd as ssa
    for kw in (dict(aggr='max'), dict(aggr='lstm'), dict(project=True), dict(flow='target_to_source')):
        with pytest.raises(NotImplementedError):
            ssa.SAGEConv(4, 4, **kw)
    with pytest.raises(NotImplementedError):
        ssa.SAGEConv((4, 4), 4)
    with pytest.raises(TypeError):
        ssa.SAGEConv(4, 4, heads=2)
    with pytest.raises(NotImplementedError):
        ssa.GINConv(torch.nn.Linear(4, 4), aggr='mean')
    ei, x = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((4, 4))
    for conv in (ssa.SAGEConv(4, 4), ssa.SAGEConv(4, 4, aggr='sum', normalize=True), ssa.GINConv(torch.nn.Linear(4, 4))):
        with pytest.raises(NotImplementedError):
            conv((x, x), ei)                       # a tuple x: bipartite
        with pytest.raises(NotImplementedError):
            conv(x, ei, torch.ones(3))             # PyG's layers take no edge_weight
        with pytest.raises(ValueError):
            conv(x[0], ei)


def test_argument_errors_need_no_device():
    import subgraph_sketching_amd as ssa
    ei = torch.zeros((2, 3), dtype=torch.int64)
    for bad in (ei.to(torch.int32), ei[0], ei.t(), ei.numpy()):
        with pytest.raises(ValueError):
            ssa.AggrGraph(4, bad)
    for bad_w in (torch.ones(2), torch.ones(3, dtype=torch.int64), torch.ones((3, 1)), torch.ones(3, requires_grad=True)):
        with pytest.raises(ValueError):
            ssa.AggrGraph(4, ei, bad_w)
    for bad_hub in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            ssa.AggrGraph(4, ei, hub_entries=bad_hub)
    with pytest.raises(ValueError):
        ssa.AggrGraph(-1, ei)
    with pytest.raises(ValueError):
        ssa.aggregate(torch.zeros((4, 4)), 'not a plan')
    plan = ssa.AggrGraph.__new__(ssa.AggrGraph)
    plan.num_nodes, plan.device = 4, torch.device('cpu')
    for kw in (dict(aggr='max'), dict(flow='source_to_target'), dict(root=1.0), dict(root=torch.ones(2)), dict(root=torch.ones(1, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ssa.aggregate(torch.zeros((4, 4)), plan, **kw)
    for bad_x in (torch.zeros((4, 4), dtype=torch.float64), torch.zeros(4), torch.zeros((3, 4)), np.zeros((4, 4), dtype=np.float32)):
        with pytest.raises(ValueError):
            ssa.aggregate(bad_x, plan)


def test_byte_model_on_a_hand_counted_case():
    """5 nodes, 7 edges (self loops are entries like any other), F = 8: gathered 7 * 32 = 224, written 5 * 32 = 160, entry words
    7 * 12 = 84 (order 4 + id 8; + 4 per weight unless unit) and 5 * 16 = 80 row-pointer words (+ 4 per node for the mean's den)"""
    import subgraph_sketching_amd as ssa
    f = ssa.roofline.aggr_bytes
    b = f(N=5, E=7, F=8)
    assert b == {'gathered': 224, 'written': 160, 'entries': 164, 'workspace': 0, 'total': 548}
    assert f(5, 7, 8, unit=False)['entries'] - b['entries'] == 28 and f(5, 7, 8, mean=True)['entries'] - b['entries'] == 20
    assert f(5, 7, 8, root=True)['gathered'] - b['gathered'] == 160 and f(5, 7, 8, root=True)['total'] == 708
    hub = f(5, 7, 8, hub_chunks=3)                                                        # three partial rows written, then read
    assert hub['workspace'] == 192 and hub['total'] == b['total'] + 192
    assert f(5, 7, 6) == b                                                                # F is padded to a multiple of 4
    wide = f(5, 7, 260)                                                                   # a second pass over the entries past 256 columns
    assert wide['entries'] == 2 * 84 + 80 and wide['gathered'] == 7 * 1040
    assert f(0, 0, 128)['total'] == 0 and f(5, 7, 0)['total'] == 0
