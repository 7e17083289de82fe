"""What gcn.GCNConv / gcn_propagate promise that needs no device: the restatement the GPU tests compare against
(tests/gcn_restatement.py) is pinned to dense float64 matrices, the planted graph has the rows it is meant to have, the header and the
binding carry the new symbol, the layer has PyG's parameter names and initialisation, and the byte model is counted by hand."""
import math
import os
import re

import numpy as np
import pytest
import torch

import gcn_restatement as gr

U = 2.0 ** -24


@pytest.fixture(scope='module', params=['unit', 'random'])
def graph(request):
    ei, w = gr.planted(request.param)
    return request.param, ei, w


def test_planted_graph_has_its_rows(graph):
    kind, ei, w = graph
    ei2, wn = gr.norm(ei, w, gr.N)
    keep = ei[0] != ei[1]
    indeg = np.bincount(ei[1][keep], minlength=gr.N)
    outdeg = np.bincount(ei[0][keep], minlength=gr.N)
    assert tuple(indeg[list(gr.IN_NODES)]) == gr.PROFILE and tuple(outdeg[list(gr.OUT_NODES)]) == gr.PROFILE
    assert not outdeg[list(gr.IN_NODES)].any() and not indeg[list(gr.OUT_NODES)].any()
    pairs = ei[0] * gr.N + ei[1]
    assert len(np.unique(pairs)) < len(pairs)                                    # duplicate edges
    A = gr.dense(ei, w, gr.N)[0]
    assert np.abs(A - A.T).max() > 0.1                                           # directed
    loop = wn[len(wn) - gr.N:]                                                   # the remaining loops, in node order, behind all edges
    assert np.array_equal(ei2[:, -gr.N:], np.stack([np.arange(gr.N)] * 2)) and (~keep).sum() == 3 and ei2.shape[1] == keep.sum() + gr.N
    deg2 = np.float32(w[(ei[1] == gr.TWO_LOOPS) & keep].sum(dtype=np.float32))
    if kind == 'random':
        assert (w != 1).any() and w[~keep].tolist().count(0.0) == 1
        assert loop[gr.ZERO_LOOP] == 0 and not np.isnan(wn).any()                # degree 0: dinv inf -> 0
        assert abs(loop[gr.TWO_LOOPS] * (deg2 + 0.5) / 0.5 - 1) < 4 * U          # the LAST explicit loop's weight (0.5, not 2.0)
    else:
        assert np.all(w == 1) and loop[gr.ZERO_LOOP] == 1 and abs(loop[gr.TWO_LOOPS] * (deg2 + 1) - 1) < 4 * U


@pytest.mark.parametrize('flow', ['source', 'target'])
def test_restatement_against_dense_float64(graph, flow):
    """every element within gamma_k (|A| @ |x|), gamma_k = k u / (1 - k u), u = 2^-24, k = (entries of the output row) + 6: with the
    fp32 norms taken as exact numbers (the dense matrix holds them) a row of m entries costs one rounding per product and m - 1 adds
    (m = in-degree + 1 for flow='target', out-degree + 1 for 'source'), i.e. k = m would do; the rest is slack"""
    kind, ei, w = graph
    x = gr.features(gr.N, 8)
    A, M, per_row, per_col = gr.dense(ei, w, gr.N)
    got = gr.propagate(ei, w, gr.N, x, flow).astype(np.float64)
    P, PM, m = (A, M, per_row) if flow == 'source' else (A.T, M.T, per_col)
    want, scale = P @ x.astype(np.float64), PM @ np.abs(x.astype(np.float64))
    k = (m - 1 + 6) * U
    bound = (k / (1 - k))[:, None] * scale
    err = np.abs(got - want)
    worst = float((err[scale > 0] / bound[scale > 0]).max())
    print(f'{kind} {flow}: worst error / bound = {worst:.3f}')
    assert worst < 1 and np.all(err[scale == 0] == 0)


def test_flows_are_adjoint_in_float64(graph):
    """<A x, g> = <x, A^T g>: what makes each product the other's backward"""
    kind, ei, w = graph
    A = gr.dense(ei, w, gr.N)[0]
    x, g = gr.features(gr.N, 5, seed=1).astype(np.float64), gr.features(gr.N, 5, seed=2).astype(np.float64)
    lhs, rhs = np.sum((A @ x) * g), np.sum(x * (A.T @ g))
    assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(A) @ np.abs(x) * np.abs(g))
    # and the restatements themselves, in float32 arithmetic: the same identity within the rounding of two 300-entry sums
    x32, g32 = x.astype(np.float32), g.astype(np.float32)
    l32 = np.sum(gr.propagate(ei, w, gr.N, x32, 'source').astype(np.float64) * g)
    r32 = np.sum(x * gr.propagate(ei, w, gr.N, g32, 'target').astype(np.float64))
    assert abs(l32 - r32) <= 2 * 310 * U * np.sum(np.abs(A) @ np.abs(x) * np.abs(g))


def test_rows_restatement_is_the_restatement(graph):
    kind, ei, w = graph
    x = gr.features(gr.N, 4)
    rows = np.array([0, 10, 25, 55, gr.TWO_LOOPS, gr.ZERO_LOOP, gr.N - 1])
    for flow in ('source', 'target'):
        full = gr.propagate(ei, w, gr.N, x, flow)
        part = gr.propagate_rows(ei, w, gr.N, lambda ids: x[ids], rows, flow)
        assert np.array_equal(full[rows].view(np.uint32), part.view(np.uint32))


def test_header_and_binding_have_the_symbol():
    import subgraph_sketching_amd as ssa
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, 'include', 'subgraph_sketch.h')) as f:
        text = f.read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int ss_gcn_spmm_t\(([^)]*)\);', text, flags=re.S)
    assert m and 'models/elph.py:153-160, 214' in m[1]
    assert [a.split()[-1].lstrip('*') for a in m[2].split(',')] == ['rowptr_c', 'order_c', 'row', 'w', 'dinv', 'loop_w', 'scan', 'N', 'x', 'F', 'out',
                                                                    'stream']
    res, args = ssa._native.SIGNATURES['ss_gcn_spmm_t']
    assert (res, args) == ssa._native.SIGNATURES['ss_sign_spmm'] and len(args) == 12
    assert ssa.GCNConv is ssa.gcn.GCNConv and ssa.gcn_propagate is ssa.gcn.gcn_propagate and ssa.GCNGraph is ssa.gcn.GCNGraph


def test_c_abi_rejects_bad_arguments_on_the_host():
    from ctypes import c_void_p
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(16)  # never dereferenced: every call below ends in the host-side checks
    ok = [fake] * 7 + [5, fake, 8, fake, None]
    for fn in (lib.ss_gcn_spmm_t, lib.ss_sign_spmm):  # the same checks
        for i in (0, 1, 2, 3, 4, 5, 6, 8, 10):
            assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == -1
        for i, bad in ((7, -1), (7, 1 << 31), (9, 0), (9, -4), (9, 6)):
            assert fn(*[bad if j == i else a for j, a in enumerate(ok)]) == -1
        assert fn(*[0 if j == 7 else (None if isinstance(a, c_void_p) else a) for j, a in enumerate(ok)]) == 0  # no nodes: nothing to do
    assert lib.ss_version() == 129


@pytest.mark.parametrize('device', ['cpu', 'meta'])
def test_layer_parameters(device):
    import subgraph_sketching_amd as ssa
    with torch.device(device):
        conv = ssa.GCNConv(20, 64)
        bare = ssa.GCNConv(64, 64, bias=False)
    assert sorted(conv.state_dict()) == ['bias', 'lin.weight']
    assert sorted(bare.state_dict()) == ['lin.weight'] and bare.bias is None
    assert conv.lin.weight.shape == (64, 20) and conv.bias.shape == (64,) and conv.lin.weight.device.type == device
    assert conv.lin.weight.requires_grad and conv.bias.requires_grad and conv.lin.weight.dtype == torch.float32
    assert (conv.in_channels, conv.out_channels) == (20, 64) and repr(conv) == 'GCNConv(20, 64)'
    if device == 'cpu':
        bound = math.sqrt(6.0 / (20 + 64))  # glorot-uniform over fan_in + fan_out
        wt = conv.lin.weight.detach()
        assert float(wt.abs().max()) <= bound and float(wt.abs().max()) > 0.9 * bound and abs(float(wt.mean())) < 0.1 * bound
        assert abs(float(wt.std()) - bound / math.sqrt(3)) < 0.1 * bound and torch.all(conv.bias == 0)
        with torch.no_grad():
            conv.lin.weight.fill_(7.0)
            conv.bias.fill_(7.0)
        conv.reset_parameters()
        assert float(conv.lin.weight.detach().abs().max()) <= bound and torch.all(conv.bias == 0)


def test_layer_loads_a_pyg_state_dict():
    import subgraph_sketching_amd as ssa
    conv = ssa.GCNConv(20, 64)
    state = {'lin.weight': torch.full((64, 20), 0.25), 'bias': torch.arange(64, dtype=torch.float32)}
    assert conv.load_state_dict(state, strict=True).missing_keys == []
    assert torch.all(conv.lin.weight == 0.25) and torch.equal(conv.bias.detach(), state['bias'])
    with pytest.raises(RuntimeError):
        ssa.GCNConv(20, 64, bias=False).load_state_dict(state, strict=True)


def test_layer_rejects_what_changes_the_mathematics():
    import subgraph_sketching_amd as ssa
    for kw in (dict(improved=True), dict(add_self_loops=False), dict(normalize=False), dict(cached=True), dict(aggr='mean'),
               dict(flow='target_to_source')):
        with pytest.raises(NotImplementedError):
            ssa.GCNConv(4, 4, **kw)
    with pytest.raises(TypeError):
        ssa.GCNConv(4, 4, heads=2)
    ssa.GCNConv(4, 4, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True, aggr='add', flow='source_to_target')


def test_argument_errors_need_no_device():
    import subgraph_sketching_amd as ssa
    ei = torch.zeros((2, 3), dtype=torch.int64)
    for bad in (ei.to(torch.int32), ei[0], ei.t(), ei.numpy()):
        with pytest.raises(ValueError):
            ssa.GCNGraph(4, bad)
    for bad_w in (torch.ones(2), torch.ones(3, dtype=torch.int64), torch.ones((3, 1)), torch.ones(3, requires_grad=True)):
        with pytest.raises(ValueError):
            ssa.GCNGraph(4, ei, bad_w)
    with pytest.raises(ValueError):
        ssa.GCNGraph(-1, ei)
    with pytest.raises(ValueError):
        ssa.gcn_propagate(torch.zeros((4, 4)), 'not a plan')
    with pytest.raises(ValueError):
        ssa.GCNConv(4, 4)(torch.zeros((4, 4)), ei, torch.ones(3, requires_grad=True))


def test_byte_model_on_a_hand_counted_case():
    """5 nodes, 7 edges of which 1 is a self loop, F = 8: gathered (6 + 5) * 32 = 352, written 5 * 32 = 160, entry words 7 * 16 = 112
    (order 4 + id 8 + dinv 4; + 4 per weight unless all are 1) and 5 * 24 = 120 per-node words (two row pointers, dinv, loop_w)"""
    import subgraph_sketching_amd as ssa
    b = ssa.roofline.gcn_spmm_bytes(N=5, E=7, F=8, self_loops=1)
    assert b == {'gathered': 352, 'written': 160, 'entries': 232, 'total': 744}
    w = ssa.roofline.gcn_spmm_bytes(N=5, E=7, F=8, self_loops=1, unit=False)
    assert w['entries'] - b['entries'] == 28 and w['gathered'] == b['gathered']
    assert ssa.roofline.gcn_spmm_bytes(5, 7, 6, 1) == b                                  # F is padded to a multiple of 4
    wide = ssa.roofline.gcn_spmm_bytes(5, 7, 260, 1)                                     # a second pass over the entries past 256 columns
    assert wide['entries'] == 2 * 112 + 120 and wide['gathered'] == 11 * 1040
    assert ssa.roofline.gcn_spmm_bytes(0, 0, 128)['total'] == 0 and ssa.roofline.gcn_spmm_bytes(5, 7, 0)['total'] == 0
