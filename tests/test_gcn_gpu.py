"""gcn.gcn_propagate / gcn.GCNConv (csrc/ss_spmm.hip: ss_gcn_spmm_t and ss_sign_spmm) on the GPU against their restatement
(tests/gcn_restatement.py, pinned to dense float64 matrices by tests/test_gcn_host.py).  The two products are compared as bits,
forward and backward: a kernel accumulates every output element in one lane, in ascending edge order with the loop last, which is the
sequential fp32 scatter-add the restatement runs -- there is exactly one right answer.  Only the layer's gradients, which pass
through torch's matrix products, are compared within a bound."""
import ctypes

import numpy as np
import pytest
import torch

import gcn_restatement as gr
import large_table_helpers as lt

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WIDTHS = (4, 8, 20, 64, 256, 260, 1024, 3, 0)  # lane groups of 1, 2, 8 (5 chunks), 16, 64, 64 + a second pass of one chunk, four passes; padded; empty
FLOWS = ('target', 'source')
OTHER = {'target': 'source', 'source': 'target'}


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module', params=['unit', 'random'])
def case(request, ssa, dev):
    """the planted graph, its plan, x and g [N, 1024] (the first F columns are the x and g of every F: the columns of a product do
    not depend on each other) and the restatement of both flows of both, computed once"""
    ei, w = gr.planted(request.param)
    x, g = gr.features(gr.N, 1024, seed=3), gr.features(gr.N, 1024, seed=5)
    gs = np.zeros_like(g)
    rows7 = np.array([0, 11, 25, 47, gr.TWO_LOOPS, 333, gr.N - 1])  # g non-zero in 7 rows only: the shape node_features[curr_links] gives
    gs[rows7] = g[rows7]
    tei, tw = torch.from_numpy(ei).to(dev), torch.from_numpy(w).to(dev)
    c = dict(kind=request.param, ei=ei, w=w, tei=tei, tw=tw, plan=ssa.GCNGraph(gr.N, tei, tw), x=torch.from_numpy(x).to(dev),
             g=torch.from_numpy(g).to(dev), gs=torch.from_numpy(gs).to(dev))
    for flow in FLOWS:
        c['x', flow], c['g', flow], c['gs', flow] = (gr.propagate(ei, w, gr.N, a, flow) for a in (x, g, gs))
    return c


def _bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f'{what}: {tuple(g.shape)} against {tuple(w.shape)}'
    bad = torch.nonzero(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} of {g.numel()} elements differ, first at {bad[:4].tolist()}'


def test_plan(case, ssa, dev):
    plan = case['plan']
    assert plan.num_nodes == gr.N and plan.device == dev and plan.num_edges == case['ei'].shape[1]
    for ids, rowptr, order in ((case['ei'][0], plan.rowptr_r, plan.order_r), (case['ei'][1], plan.rowptr_c, plan.order_c)):
        want = np.argsort(ids, kind='stable')  # BOTH groupings sorted, unit weights or not: each is an accumulation order
        assert np.array_equal(order.cpu().numpy(), want) and np.array_equal(np.diff(rowptr.cpu().numpy()), np.bincount(ids, minlength=gr.N))
    unweighted = ssa.GCNGraph(gr.N, case['tei'])
    if case['kind'] == 'unit':
        _assert_same(unweighted.dinv, plan.dinv, 'dinv without weights')


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('flow', FLOWS)
def test_forward_and_backward_bits(case, ssa, F, flow):
    x = case['x'][:, :F].clone().requires_grad_(True)
    y = ssa.gcn_propagate(x, case['plan'], flow)
    assert y.shape == (gr.N, F) and y.dtype == torch.float32 and y.device == x.device
    _assert_same(y, case['x', flow][:, :F], f'{flow} F={F}')
    if flow == 'source' and F:
        _assert_same(y, ssa.sign.generate_sign_features(case['x'][:, :F], case['tei'], case['tw'], 0), f'generate_sign_features F={F}')
    for name in ('g', 'gs'):
        g = case[name][:, :F]  # (a non-contiguous grad_out unless F = 1024)
        x.grad = None
        (y * g).sum().backward(retain_graph=True)
        first = x.grad.clone()
        assert first.shape == (gr.N, F)
        _assert_same(first, case[name, OTHER[flow]][:, :F], f'{flow} F={F} x.grad for {name}')
        x.grad = None
        (y * g).sum().backward(retain_graph=True)
        _assert_same(x.grad, first, f'{flow} F={F} second backward')


def test_propagate_argument_errors(case, ssa):
    plan, x = case['plan'], case['x'][:, :8]
    for bad in (x.double(), x.half(), x[:, 0], x[None], x[:-1], x.cpu(), x.cpu().numpy()):
        with pytest.raises(ValueError):
            ssa.gcn_propagate(bad, plan)
    with pytest.raises(ValueError):
        ssa.gcn_propagate(x, plan, flow='source_to_target')
    with pytest.raises(ValueError):
        ssa.gcn_propagate(x, case['tei'])
    y = ssa.gcn_propagate(x.t().contiguous().t(), plan)  # a non-contiguous x is copied, not refused
    _assert_same(y, case['x', 'target'][:, :8], 'non-contiguous x')
    with torch.no_grad():
        assert not ssa.gcn_propagate(x, plan).requires_grad


SENTINEL = 0x7FC0BEEF  # a NaN no sum produces


@pytest.mark.parametrize('F', [4, 20, 260])
def test_direct_launch_into_guarded_rows(case, ssa, dev, F):
    """ss_gcn_spmm_t through the binding into the middle of a sentinel-filled buffer: its own N x F places hold the restatement,
    the guard rows before and after keep the sentinel"""
    lib, plan, guard = ssa._native.lib(), case['plan'], 67
    x = case['x'][:, :F].contiguous()
    buf = torch.full((gr.N + 2 * guard, F), SENTINEL, dtype=torch.int32, device=dev)
    out = ctypes.c_void_p(buf.data_ptr() + guard * F * 4)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    code = lib.ss_gcn_spmm_t(p(plan.rowptr_c), p(plan.order_c), p(plan.row), p(plan.w), p(plan.dinv), p(plan.loop_w), p(plan.scan), gr.N, p(x), F, out,
                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert code == 0
    torch.cuda.synchronize(dev)
    got = buf.cpu()
    assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + gr.N:] == SENTINEL)
    _assert_same(got[guard:guard + gr.N].view(torch.float32), case['x', 'target'][:, :F], f'direct F={F}')
    assert lib.ss_gcn_spmm_t(p(plan.rowptr_c), p(plan.order_c), p(plan.row), p(plan.w), p(plan.dinv), p(plan.loop_w), p(plan.scan), gr.N, p(x), F + 1, out,
                             None) == -1


def test_out_of_range_ids_raise_and_are_not_followed(case, ssa, dev):
    """ids outside [0, N), negative ones included, among the 300 good edges of the two hubs: the plan raises IndexError, and
    both products, run on the refused plan all the same, follow none of them (finite everywhere, nothing faults)"""
    ei = case['ei']
    hub_in = np.nonzero(ei[1] == gr.IN_NODES[-1])[0]
    hub_out = np.nonzero(ei[0] == gr.OUT_NODES[-1])[0]
    for where, ids in (((0, hub_in[[40, 41, 170]]), (gr.N, -3, gr.N + (1 << 33))), ((1, hub_out[[7, 130, 131]]), (-1, gr.N, -(1 << 40))),
                       ((0, hub_in[[299]]), (gr.N,))):
        bad = case['tei'].clone()
        bad[where[0], torch.from_numpy(where[1]).to(dev)] = torch.tensor(ids, device=dev)
        with pytest.raises(IndexError):
            ssa.GCNGraph(gr.N, bad, case['tw'])
        with pytest.raises(IndexError):
            ssa.GCNConv(8, 8).to(dev)(case['x'][:, :8], bad, case['tw'])
        refused = ssa.GCNGraph.__new__(ssa.GCNGraph)
        with pytest.raises(IndexError):
            refused.__init__(gr.N, bad, case['tw'])
        for target in (True, False):
            y = refused.product(case['x'][:, :20].contiguous(), target)
            torch.cuda.synchronize(dev)
            assert bool(torch.isfinite(y).all())


def test_tiny_graphs(ssa, dev):
    """the empty edge list (every node keeps its loop of weight 1: the identity), N = 1 and N = 2"""
    x = torch.from_numpy(gr.features(5, 12)).to(dev)
    for n in (5, 2, 1):
        empty = ssa.GCNGraph(n, torch.zeros((2, 0), dtype=torch.int64, device=dev))
        for flow in FLOWS:
            _assert_same(ssa.gcn_propagate(x[:n], empty, flow), x[:n], f'no edges, N={n}')
    for n, ei, w in ((1, [[0], [0]], [3.0]), (1, [[0, 0], [0, 0]], [3.0, 0.0]), (2, [[0, 1, 0], [1, 0, 1]], [0.5, 2.0, 4.0]), (2, [[1], [1]], [0.0])):
        ei, w = np.array(ei, dtype=np.int64), np.array(w, dtype=np.float32)
        plan = ssa.GCNGraph(n, torch.from_numpy(ei).to(dev), torch.from_numpy(w).to(dev))
        for flow in FLOWS:
            xs = x[:n].clone().requires_grad_(True)
            y = ssa.gcn_propagate(xs, plan, flow)
            _assert_same(y, gr.propagate(ei, w, n, x[:n].cpu().numpy(), flow), f'N={n} {flow}')
            y.sum().backward()
            _assert_same(xs.grad, gr.propagate(ei, w, n, np.ones((n, 12), dtype=np.float32), OTHER[flow]), f'N={n} {flow} grad')


# ---- the layer ------------------------------------------------------------------------------------------------------------------

def _stack(ssa, dev, seed=17):
    torch.manual_seed(seed)
    convs = [ssa.GCNConv(20, 64).to(dev), ssa.GCNConv(64, 64).to(dev)]
    with torch.no_grad():
        for c in convs:
            c.bias.uniform_(-0.5, 0.5)  # (zeros would hide the bias from the forward comparison)
    return convs


def test_layers_equal_the_composition(case, ssa, dev):
    """GCNConv(20, 64) -> GCNConv(64, 64) as ELPH stacks them (no activation in between): the same bits as F.linear -> restatement
    -> + bias with the same torch ops around the restated product"""
    convs = _stack(ssa, dev)
    x = case['x'][:, :20].contiguous()
    with torch.no_grad():
        got, want = x, x
        for c in convs:
            got = c(got, case['tei'], case['tw'])
            z = torch.nn.functional.linear(want, c.lin.weight)
            want = torch.from_numpy(gr.propagate(case['ei'], case['w'], gr.N, z.cpu().numpy(), 'target')).to(dev) + c.bias
        assert got.shape == (gr.N, 64)
        _assert_same(got, want, 'two layers')
        _assert_same(convs[1](convs[0](x, case['plan']), case['plan']), want, 'two layers on the plan')
        bare = ssa.GCNConv(20, 64, bias=False).to(dev)
        z = torch.nn.functional.linear(x, bare.lin.weight)
        _assert_same(bare(x, case['plan']), gr.propagate(case['ei'], case['w'], gr.N, z.cpu().numpy(), 'target'), 'bias=False')


def test_layer_gradients_against_float64(case, ssa, dev):
    """loss = <h2[rows of 32 links], G>: lin.weight.grad, bias.grad of both layers and x.grad within gamma_k of the float64 evaluation
    of the same model on the dense matrix (the fp32 norms taken as exact), k = inner length + max in-degree + 8 against the float64
    product of the magnitudes.  Inner length: the longest contraction on the gradient's way -- N for the parameters (a sum over all
    nodes), 64 channels for x.grad.  The worst ratio of every gradient is printed (profiles/gcn_tests.txt records a run)."""
    convs = _stack(ssa, dev)
    x = case['x'][:, :20].clone().requires_grad_(True)
    links = np.random.RandomState(9).randint(0, gr.N, size=(32, 2))
    links[0], links[1] = (gr.IN_NODES[-1], gr.OUT_NODES[-1]), (gr.TWO_LOOPS, gr.N - 1)
    rows = torch.from_numpy(links.reshape(-1)).to(dev)
    G = case['g'][:64, :64].contiguous()
    h = x
    for c in convs:
        h = c(h, case['tei'], case['tw'])
    (h[rows] * G).sum().backward()

    A, M, per_row, per_col = gr.dense(case['ei'], case['w'], gr.N)
    P, PM = A.T, M.T  # GCNConv propagates with the transpose
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    x64, W1, b1, W2, b2 = f64(x), f64(convs[0].lin.weight), f64(convs[0].bias), f64(convs[1].lin.weight), f64(convs[1].bias)
    Gd = np.zeros((gr.N, 64))
    np.add.at(Gd, links.reshape(-1), f64(G))  # (h[rows] repeats a row for every link it is in: its gradient is the sum)

    def grads(P, x, W1, b1, W2, G):
        h1 = P @ (x @ W1.T) + b1
        dz2 = P.T @ G
        dh1 = dz2 @ W2
        dz1 = P.T @ dh1
        return {'lin2.weight': dz2.T @ h1, 'bias2': G.sum(0), 'lin1.weight': dz1.T @ x, 'bias1': dh1.sum(0), 'x': dz1 @ W1}

    want = grads(P, x64, W1, b1, W2, Gd)
    Ga = np.zeros((gr.N, 64))
    np.add.at(Ga, links.reshape(-1), np.abs(f64(G)))
    scale = grads(PM, np.abs(x64), np.abs(W1), np.abs(b1), np.abs(W2), Ga)
    got = {'lin2.weight': convs[1].lin.weight.grad, 'bias2': convs[1].bias.grad, 'lin1.weight': convs[0].lin.weight.grad,
           'bias1': convs[0].bias.grad, 'x': x.grad}
    max_in = int(per_col.max()) - 1
    assert max_in == 300
    worst = {}
    for name in want:
        k = ((64 if name == 'x' else gr.N) + max_in + 8) * U
        err, bound = np.abs(f64(got[name]) - want[name]), k / (1 - k) * scale[name]
        assert got[name].shape == want[name].shape and np.all(err[bound == 0] == 0)  # (rows of x no link row reaches in two hops)
        worst[name] = float((err[bound > 0] / bound[bound > 0]).max())
    print(f'[gcn] {case["kind"]} weights, layer gradients, worst error / bound: ' + ', '.join(f'{n} {r:.4f}' for n, r in worst.items()))
    assert max(worst.values()) < 1, worst


def test_cache(case, ssa, dev):
    convs = _stack(ssa, dev)
    x = case['x'][:, :20].contiguous()
    ei = case['tei'].clone()
    with torch.no_grad():
        before = ssa.GCNGraph.builds
        first = convs[1](convs[0](x, ei), ei)
        assert ssa.GCNGraph.builds == before + 1                      # two layers fed one tensor: one build
        again = convs[1](convs[0](x, ei), ei)
        assert ssa.GCNGraph.builds == before + 1
        _assert_same(again, first, 'cached plan')
        on_plan = convs[1](convs[0](x, case['plan']), case['plan'])   # (the fixture's plan has the weights; unit weights: the same graph)
        assert ssa.GCNGraph.builds == before + 1                      # a plan never builds
        if case['kind'] == 'unit':
            _assert_same(on_plan, first, 'plan against tensor')
        fresh = ei.clone()
        same = convs[1](convs[0](x, fresh), fresh)
        assert ssa.GCNGraph.builds == before + 2                      # a fresh tensor of equal content rebuilds ...
        _assert_same(same, first, 'fresh equal tensor')               # ... and gives the same
        victim = int(np.nonzero(case['ei'][1] == gr.IN_NODES[5])[0][2])
        fresh[1, victim] = gr.IN_NODES[0]                             # an in-place edit: node 10 gains its first in-edge
        edited = convs[0](x, fresh)
        assert ssa.GCNGraph.builds == before + 3
        ei2 = case['ei'].copy()
        ei2[1, victim] = gr.IN_NODES[0]
        z = torch.nn.functional.linear(x, convs[0].lin.weight)
        want = torch.from_numpy(gr.propagate(ei2, np.ones(ei2.shape[1], dtype=np.float32), gr.N, z.cpu().numpy(), 'target')).to(dev) + convs[0].bias
        _assert_same(edited, want, 'edited graph')
        convs[1](edited, fresh)
        assert ssa.GCNGraph.builds == before + 3
        w = case['tw'].clone()
        convs[0](x, fresh, w)                                         # the weights are part of the identity
        convs[1](edited, fresh, w)
        assert ssa.GCNGraph.builds == before + 4
        w[3] = 0.75
        y = convs[0](x, fresh, w)
        assert ssa.GCNGraph.builds == before + 5
        w2 = case['w'].copy()
        w2[3] = 0.75
        _assert_same(y, torch.from_numpy(gr.propagate(ei2, w2, gr.N, z.cpu().numpy(), 'target')).to(dev) + convs[0].bias, 'edited weights')


# ---- offsets past 2^31 elements --------------------------------------------------------------------------------------------------

def _formula(ids, F):
    """x[i, j] = ((131 i + 7 j) mod 1021 - 510) / 64: exact in fp32, the same numbers on the host and on the device"""
    v = (131 * np.asarray(ids, dtype=np.int64)[:, None] + 7 * np.arange(F, dtype=np.int64)[None, :]) % 1021 - 510
    return (v.astype(np.float32) / np.float32(64)).astype(np.float32)


def test_offsets_past_two_to_the_31_elements(ssa, dev):
    """N = 2 200 000, F = 1 024: x and out hold 2.25e9 elements (9.0 GB each), so element offsets pass 2^31 and byte offsets 2, 4 and
    8 GiB (rows 524 288, 1 048 576, 2 097 152).  A directed ring plus edges between the last 64 rows and the rows around every
    boundary, both ways; 256 sampled rows of both flows against the restatement evaluated on those rows."""
    n, F = 2_200_000, 1024
    lt.require_free_memory(dev, 3 * n * F * 4, 'the large-offset GCN case')
    bounds = [(1 << 31) // F // 4, (1 << 31) // F // 2, (1 << 31) // F]
    near = np.array([0] + [b + d for b in bounds for d in (-1, 0, 1)], dtype=np.int64)
    last = np.arange(n - 64, n, dtype=np.int64)
    ring = np.arange(n, dtype=np.int64)
    a, b = np.repeat(near, 64), np.tile(last, len(near))
    ei = np.concatenate([np.stack([ring, (ring + 1) % n]), np.stack([a, b]), np.stack([b, a])], axis=1)
    rng = np.random.RandomState(23)
    ei = ei[:, rng.permutation(ei.shape[1])]
    w = rng.uniform(0.5, 1.5, size=ei.shape[1]).astype(np.float32)
    must = np.unique(np.concatenate([near, [1, n - 65, n - 64, n - 2, n - 1]]))  # the first, the last, either side of every boundary
    spread = rng.choice(n, size=400, replace=False)
    past = bounds[2] + 2 + rng.choice(n - bounds[2] - 2, size=40, replace=False)  # 40 rows past 2^31 elements
    fill = np.setdiff1d(np.concatenate([past, spread]), must, assume_unique=False)
    rows = np.sort(np.concatenate([must, rng.permutation(fill)[:256 - len(must)]]))
    assert len(rows) == 256 == len(np.unique(rows)) and rows[0] == 0 and rows[-1] == n - 1 and (rows > bounds[2]).sum() >= 8
    plan = ssa.GCNGraph(n, torch.from_numpy(ei).to(dev), torch.from_numpy(w).to(dev))
    x = torch.empty((n, F), dtype=torch.float32, device=dev)
    assert x.numel() > 1 << 31
    cols = 7 * torch.arange(F, dtype=torch.int32, device=dev)[None, :]
    for r0 in range(0, n, 1 << 18):
        ids = torch.arange(r0, min(r0 + (1 << 18), n), dtype=torch.int32, device=dev)[:, None]
        x[r0:r0 + (1 << 18)] = ((131 * ids + cols) % 1021 - 510).to(torch.float32) / 64
    trows = torch.from_numpy(rows).to(dev)
    _assert_same(x[trows], _formula(rows, F), 'the formula on the device')
    for flow in FLOWS:
        y = ssa.gcn_propagate(x, plan, flow)
        got = y[trows].cpu()
        del y
        want = gr.propagate_rows(ei, w, n, lambda ids: _formula(ids, F), rows, flow)
        _assert_same(got, want, f'large {flow}')
    del x, plan
    torch.cuda.empty_cache()
