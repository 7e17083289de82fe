"""probe: aggr.aggregate / SAGEConv / GINConv on the bench's own graphs (collab size) -> profiles/aggr_probe.txt

For the uniform graph and the rank^-0.9 one (bench.synthetic_graph(kind='powerlaw', alpha=0.9): hub rows of 10^4+ entries), F = 128,
256, 1024: the plan build, every product forward and backward against the byte model (roofline.aggr_bytes), gcn_propagate on the same
graph in the same process, and the forms torch offers without PyG (gather + index_add_, with a division for the mean: float
atomics).  On the hub graph a sweep of hub_entries (256 ... 8192, 10^9 = no hub tier); the mean's backward with its division
inside the gather against a pass of its own; one SEALSAGE-shaped and one SEALGIN-shaped step on a sampled-subgraph batch.
Nothing is gated: the file is a measurement to quote.  It decided aggr.DEFAULT_HUB_ENTRIES and where the mean's backward divides."""
import os
import sys
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import subgraph_sketching_amd as ssa
from subgraph_sketching_amd import aggr, roofline

dev = torch.device('cuda:0')
n = bench.N_NODES
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def fwd_bwd(product, x, g):
    x.grad = None
    product(x).backward(g)


def pct(model, ms):
    return 100 * model / ms / 1e6 / roofline.HBM_PEAK_GBS


say(f'default in this run: hub_entries = {aggr.DEFAULT_HUB_ENTRIES}')
for name, kwargs in (('uniform', dict(kind='uniform')), ('rank^-0.9', dict(kind='powerlaw', alpha=0.9))):
    ei_np = bench.synthetic_graph(**kwargs)
    E = ei_np.shape[1]
    indeg = np.bincount(ei_np[1], minlength=n)
    ei = torch.from_numpy(ei_np).to(dev)
    t_plan = timed(lambda: ssa.AggrGraph(n, ei), 5)
    plan = ssa.AggrGraph(n, ei)
    gplan = ssa.GCNGraph(n, ei)
    say(f'graph {name}: N = {n}, E_dir = {E}, largest in-degree {indeg.max()}, median {int(np.median(indeg))}; plan build (two stable groupings, '
        f'den, hub lists, one host read) {t_plan:.3f} ms; at hub_entries = {plan.hub_entries}: {plan.target.n_hubs} hub rows in {plan.target.n_chunks} chunks')
    root = torch.tensor([1.25], device=dev)
    for F in (128, 256, 1024):
        x = torch.randn(n, F, device=dev, requires_grad=True)
        g = torch.randn(n, F, device=dev)
        for what, kw, mean, rt in (('sum', dict(aggr='sum'), False, False), ('mean', dict(aggr='mean'), True, False),
                                   ('sum + root', dict(aggr='sum', root=root), False, True)):
            model = roofline.aggr_bytes(n, E, F, mean=mean, root=rt, hub_chunks=plan.target.n_chunks)['total']
            for flow in ('target', 'source'):
                with torch.no_grad():
                    t_f = timed(lambda: ssa.aggregate(x, plan, flow=flow, **kw), 10)
                t_fb = timed(lambda: fwd_bwd(lambda t: ssa.aggregate(t, plan, flow=flow, **kw), x, g), 10)
                t_fb = max(t_fb, t_f + 1e-6)
                say(f'  F = {F:>4} {what:<10} flow={flow:<6}: forward {t_f:.3f} ms = {pct(model, t_f):.1f} % of the HBM peak by the byte model ({model:,} B); '
                    f'forward + backward {t_fb:.3f} ms (backward {t_fb - t_f:.3f} ms)')
        with torch.no_grad():
            t_g = timed(lambda: ssa.gcn_propagate(x, gplan), 10)
        t_gfb = timed(lambda: fwd_bwd(lambda t: ssa.gcn_propagate(t, gplan), x, g), 10)
        say(f'  F = {F:>4} gcn_propagate flow=target on the same graph: forward {t_g:.3f} ms, forward + backward {t_gfb:.3f} ms')
        cnt = torch.bincount(ei[1], minlength=n).clamp(min=1).to(torch.float32)[:, None]

        def torch_sum(t):  # PyG's edge-list form: the [E, F] message tensor, then a scatter-add with float atomics
            return torch.zeros_like(t).index_add_(0, ei[1], t[ei[0]])

        t_ts = timed(lambda: fwd_bwd(torch_sum, x, g), 3)
        t_tm = timed(lambda: fwd_bwd(lambda t: torch_sum(t) / cnt, x, g), 3)
        with torch.no_grad():
            close = bool(torch.allclose(torch_sum(x) / cnt, ssa.aggregate(x, plan, 'mean'), rtol=1e-4, atol=1e-4))
        say(f'  F = {F:>4} torch, forward + backward: gather + index_add_ {t_ts:.3f} ms, with the division (mean) {t_tm:.3f} ms (allclose to ours: {close})')
        # the mean's backward: the division inside the gather (what aggregate does) against a division pass of its own in front of
        # the transposed sum product (the alternative the contract allows: the same bits)
        with torch.no_grad():
            t_in = timed(lambda: plan.product(g, False, gather_den=plan.target.den), 10)
            t_own = timed(lambda: plan.product(g / plan.target.den[:, None], False), 10)
        say(f'  F = {F:>4} mean, backward alone: division inside the gather {t_in:.3f} ms, as a pass of its own {t_own:.3f} ms')
        if name != 'uniform':
            parts = []
            for hub in (256, 512, 1024, 2048, 8192, 10 ** 9):
                p = ssa.AggrGraph(n, ei, hub_entries=hub)
                with torch.no_grad():
                    t_f = timed(lambda: ssa.aggregate(x, p), 10)
                t_fb = timed(lambda: fwd_bwd(lambda t: ssa.aggregate(t, p), x, g), 10)
                parts.append(f'{hub}: {p.target.n_hubs} hubs / {p.target.n_chunks} chunks, forward {t_f:.3f} ms, forward + backward {t_fb:.3f} ms')
                del p
            say(f'  F = {F:>4} sum, flow=target, hub_entries sweep -- ' + '; '.join(parts))
        del x, g
    if name == 'uniform':
        # SEAL-shaped steps on a sampled-subgraph batch: 2 048 links, 2 hops, at most 100 nodes per hop (the reference's caps)
        B, hidden = 2048, 256
        eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=bench.HLL_P, minhash_num_perm=bench.P, floor_sf=False, use_zero_one=True))
        links = torch.from_numpy(bench.synthetic_links(n, B)).to(dev)
        sg = eh.exact_subgraphs(links, n, ei, max_nodes_per_hop=100)
        t_sg = timed(lambda: ssa.AggrGraph.from_subgraphs(sg), 5)
        graph = ssa.AggrGraph.from_subgraphs(sg)
        T = sg.ids.numel()
        emb = torch.nn.Embedding(int(sg.z.max()) + 1, hidden).to(dev)
        sage = torch.nn.ModuleList([ssa.SAGEConv(hidden, hidden) for _ in range(3)]).to(dev)
        mlp = lambda: torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.BatchNorm1d(hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden))
        gin = torch.nn.ModuleList([ssa.GINConv(mlp(), train_eps=True) for _ in range(3)]).to(dev)
        head = torch.nn.Linear(hidden, 1).to(dev)

        def step(convs, pool):
            for m in (emb, convs, head):
                m.zero_grad(set_to_none=True)
            h = emb(sg.z)
            for c in convs:
                h = torch.relu(c(h, graph))
            head(pool(h, sg)).sum().backward()

        t_s = timed(lambda: step(sage, ssa.center_pool), 10)
        t_g = timed(lambda: step(gin, ssa.global_mean_pool), 10)
        say(f'SEAL-shaped steps, B = {B} links, sampled subgraphs (2 hops, 100 nodes per hop): T = {T} nodes, A = {graph.num_edges} arcs; plan from the '
            f'batch {t_sg:.3f} ms; Embedding -> 3 x SAGEConv({hidden}) -> center_pool -> Linear, forward + backward {t_s:.3f} ms; '
            f'Embedding -> 3 x GINConv(MLP {hidden}) -> global_mean_pool -> Linear, forward + backward {t_g:.3f} ms')

text = '\n'.join(lines) + '\n'
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'aggr_probe.txt')
with open(path, 'w') as f:
    f.write(text)
