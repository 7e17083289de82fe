"""probe: gcn.gcn_propagate / gcn.GCNConv on the bench's own graphs (collab size) -> profiles/gcn_probe.txt

For the uniform graph and the rank^-0.9 one (bench.synthetic_graph(kind='powerlaw', alpha=0.9): hub rows of 10^4+ entries, one
wavefront per row), F = 128, 256, 1024: the plan build, forward and backward of each flow against the byte model, the same forward +
backward through the two forms torch offers without PyG -- gather * norm + index_add_ (PyG's edge-list form, float atomics) and
torch.sparse.mm on a CSR tensor -- and one ELPH-shaped training step (the sketch call sequence of bench.py --api elph at B = 2 048 +
two convs at 1024 + backward).  Nothing is gated: the file is a measurement to quote."""
import os
import sys
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import subgraph_sketching_amd as ssa
from subgraph_sketching_amd import roofline, sign

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


for name, kwargs in (('uniform', dict(kind='uniform')), ('rank^-0.9', dict(kind='powerlaw', alpha=0.9))):
    ei_np = bench.synthetic_graph(**kwargs)
    E = ei_np.shape[1]
    self_loops = int((ei_np[0] == ei_np[1]).sum())
    indeg = np.bincount(ei_np[1], minlength=n)
    ei = torch.from_numpy(ei_np).to(dev)
    t_plan = timed(lambda: ssa.GCNGraph(n, ei), 5)
    plan = ssa.GCNGraph(n, ei)
    say(f'graph {name}: N = {n}, E_dir = {E} ({self_loops} self loops), largest in-degree {indeg.max()}, median {int(np.median(indeg))}; '
        f'plan build (two stable groupings, scan, degrees, one host read) {t_plan:.3f} ms')
    ei2, wn = sign.gcn_norm(ei, torch.ones(E, device=dev), n)
    order = torch.argsort(ei2[1], stable=True)
    crow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.bincount(ei2[1], minlength=n), 0)
    try:
        At = torch.sparse_csr_tensor(crow, ei2[0][order], wn[order], size=(n, n))  # rows = targets: GCNConv's product
    except Exception as exc:
        At = exc
    for F in (128, 256, 1024):
        x = torch.randn(n, F, device=dev, requires_grad=True)
        g = torch.randn(n, F, device=dev)
        model = roofline.gcn_spmm_bytes(n, E, F, self_loops)['total']
        for flow in ('target', 'source'):
            with torch.no_grad():
                t_f = timed(lambda: ssa.gcn_propagate(x, plan, flow), 10)
            t_fb = timed(lambda: fwd_bwd(lambda t: ssa.gcn_propagate(t, plan, flow), x, g), 10)
            t_fb = max(t_fb, t_f + 1e-6)
            say(f'  F = {F:>4} flow={flow:<6}: forward {t_f:.3f} ms = {model / t_f / 1e6:.0f} GB/s of the byte model ({model:,} B, '
                f'{100 * model / t_f / 1e6 / roofline.HBM_PEAK_GBS:.1f} % of the HBM peak); forward + backward {t_fb:.3f} ms '
                f'(backward {t_fb - t_f:.3f} ms = {100 * model / (t_fb - t_f) / 1e6 / roofline.HBM_PEAK_GBS:.1f} % of the peak)')

        def edge_list(t):  # PyG's edge-list form: the [E', F] message tensor, then a scatter-add with float atomics
            return torch.zeros_like(t).index_add_(0, ei2[1], t[ei2[0]] * wn[:, None])

        t_el = timed(lambda: fwd_bwd(edge_list, x, g), 3)
        try:
            if isinstance(At, Exception):
                raise At
            t_sp = f'{timed(lambda: fwd_bwd(lambda t: torch.sparse.mm(At, t), x, g), 3):.3f} ms'
        except Exception as exc:  # (the backward of a CSR product is not in every torch build)
            t_sp = f'not available ({type(exc).__name__}: {str(exc)[:80]})'
        with torch.no_grad():
            close = bool(torch.allclose(edge_list(x), ssa.gcn_propagate(x, plan), rtol=1e-4, atol=1e-5))
        say(f'  F = {F:>4} torch, forward + backward: gather * norm + index_add_ {t_el:.3f} ms (allclose to flow=target: {close}); '
            f'torch.sparse.mm on a CSR tensor {t_sp}')
        del x, g
    if name == 'uniform':
        # one ELPH-shaped training step: the sketch sequence of ELPH.forward at the reference's batch, two GCNConv(1024, 1024) on the
        # whole graph, a loss on the rows of the batch's links, backward
        h, B = 2, 2048
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=bench.HLL_P, minhash_num_perm=bench.P, floor_sf=False, use_zero_one=True))
        links = torch.from_numpy(bench.synthetic_links(n, B)).to(dev)
        mh0, hll0 = eh.initialise_minhash(n), eh.initialise_hll(n)
        convs = torch.nn.ModuleList([ssa.GCNConv(1024, 1024), ssa.GCNConv(1024, 1024)]).to(dev)
        feats = torch.randn(n, 1024, device=dev)

        def sketches():
            hash_ei = torch.cat([ei, torch.arange(n, device=dev).repeat(2, 1)], dim=1)
            table = {0: {'minhash': mh0, 'hll': hll0}}
            cards = torch.zeros((n, h), device=dev)
            for k in range(1, h + 1):
                table[k] = {'hll': eh.hll_prop(table[k - 1]['hll'], hash_ei), 'minhash': eh.minhash_prop(table[k - 1]['minhash'], hash_ei)}
                cards[:, k - 1] = eh.hll_count(table[k]['hll'])
            return eh.get_subgraph_features(links, table, cards)

        def features(graph):
            convs.zero_grad(set_to_none=True)
            out = feats
            for c in convs:
                out = c(out, graph)
            (out[links[:, 0]] * out[links[:, 1]]).sum().backward()

        t_sk = timed(sketches, 20)
        t_ft_plan = timed(lambda: features(plan), 5)
        t_ft_tensor = timed(lambda: features(ei), 5)            # the same tensor object every step: the cache holds
        t_ft_fresh = timed(lambda: features(ei.clone()), 5)     # a fresh equal tensor every step: one rebuild per step
        say(f'ELPH-shaped step, B = {B}, hidden 1024: sketch sequence {t_sk:.3f} ms; two GCNConv(1024, 1024) forward + backward on the plan '
            f'{t_ft_plan:.3f} ms, on the same edge_index tensor {t_ft_tensor:.3f} ms, on a fresh equal tensor every step {t_ft_fresh:.3f} ms '
            f'(the rebuild: +{t_ft_fresh - t_ft_tensor:.3f} ms)')
        del convs, feats

text = '\n'.join(lines) + '\n'
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'gcn_probe.txt')
with open(path, 'w') as f:
    f.write(text)
