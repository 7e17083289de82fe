"""probe: cn_pool.common_neighbour_pool on the bench's graph size (collab, N = 235 868) -> profiles/cn_pool_probe.txt

Random uniform links share almost no neighbours (profiles/cn_features_probe.txt: 18 hits in 65 536 links), so the links are drawn from
sample_negatives(mode='wedge'), where every pair has a common neighbour, and from the graph's own edges; on the uniform graph and on
the rank^-0.9 one (bench.synthetic_graph(kind='powerlaw', alpha=0.9)); L = 2 048 and 65 536; F = 128, 256, 1 024.  Measured: the plan
build, the forward, and forward + backward, against the torch composition on the same GPU (`coef[:, None] * x[ids]` followed by
index_add_, and its autograd backward) and, for the forward alone, against heuristics.common_neighbour_features; the share of the
HBM peak on roofline.cn_rows_bytes.  Nothing is gated: the file is a measurement to quote."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import bench
import subgraph_sketching_amd as ssa
from subgraph_sketching_amd import cn_pool, heuristics, roofline

dev = torch.device('cuda:0')
n = bench.N_NODES
lines = []
TORCH_LIMIT = 24 << 30  # bytes of the [T, F] tensor beyond which the torch composition is not run


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, window=0.03, repeats=5):
    """ms per call: after a warm-up one call is timed to size the run; then the MEDIAN over `repeats` runs of as many calls as fill
    `window` seconds (at least 3, at most 1000), a host clock around each run, ending in a device synchronise"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = int(min(1000, max(3, window / max(time.perf_counter() - t0, 1e-6))))
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e3)
    return statistics.median(out)


def fwd_bwd(f, x, g):
    x.grad = None
    f(x).backward(g)


def pct(model, ms):
    return 100 * model / ms / 1e6 / roofline.HBM_PEAK_GBS


say(f'default in this run: hub_entries = {cn_pool.DEFAULT_HUB_ENTRIES}; N = {n}; weighting RA; times in ms per call, the median of 5 runs of a 30 ms window '
    f'(3 to 1000 calls) after a warm-up, one process on the card')
for kind in ('uniform', 'rank^-0.9'):
    ei = bench.synthetic_graph(n, bench.E_UND, 'uniform' if kind == 'uniform' else 'powerlaw', 0.9, seed=1)
    A = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    A.sum_duplicates()
    A.data[:] = 1.0
    tei = torch.from_numpy(ei).to(dev)
    adj = heuristics._adjacency(A, dev)
    rng = np.random.RandomState(7)
    for source in ('wedge negatives', 'own edges'):
        for L in (2048, 65536):
            if source == 'own edges':
                links = torch.from_numpy(np.ascontiguousarray(ei[:, rng.choice(ei.shape[1], size=L, replace=False)].T)).to(dev)
            else:
                pos = torch.from_numpy(np.ascontiguousarray(ei[:, rng.choice(ei.shape[1], size=L, replace=False)].T)).to(dev)
                links = ssa.sample_negatives(n, tei, pos, mode='wedge', seed=5)
                links = links[links[:, 1] >= 0].contiguous()
            L_eff = links.size(0)
            t_plan = timed(lambda: ssa.CommonNeighbourBatch(adj, links, 'RA'))
            plan = ssa.CommonNeighbourBatch(adj, links, 'RA')
            T, M = plan.num_entries, plan.num_touched
            groups = torch.bincount(plan.ids, minlength=n)
            rows = plan.rowptr[1:] - plan.rowptr[:-1]
            say(f'graph {kind}, links {source}, L = {L_eff}: T = {T} ({T / max(L_eff, 1):.2f} per link, longest row {int(rows.max())}), {M} named nodes, largest node '
                f'group {int(groups.max())}; plan build (count, fill, grouping, lists, two host reads) {t_plan:.3f} ms; hubs: {plan.link_hubs[1]} link rows in '
                f'{plan.link_hubs[2]} chunks, {plan.node_hubs[1]} node rows in {plan.node_hubs[2]} chunks')
            owner, ids, coef = plan.owner, plan.ids, plan.coef
            for F in (128, 256, 1024):
                x = torch.randn(n, F, device=dev, requires_grad=True)
                g = torch.randn(L_eff, F, device=dev)
                ours = lambda t: ssa.common_neighbour_pool(t, plan)
                theirs = lambda t: t.new_zeros((L_eff, F)).index_add_(0, owner, coef[:, None] * t[ids])
                b_f = roofline.cn_rows_bytes(n, L_eff, T, F, hub_chunks=plan.link_hubs[2])['total']
                b_b = roofline.cn_rows_bytes(n, L_eff, T, F, backward=True, M=M, hub_chunks=plan.node_hubs[2])['total']
                run_torch = T * F * 4 <= TORCH_LIMIT
                with torch.no_grad():
                    t_f = timed(lambda: ours(x))
                    t_tf = timed(lambda: theirs(x)) if run_torch else float('nan')
                    t_feat = timed(lambda: heuristics.common_neighbour_features(adj, links, x.detach(), 'RA'))
                t_fb = timed(lambda: fwd_bwd(ours, x, g))
                t_tfb = timed(lambda: fwd_bwd(theirs, x, g)) if run_torch else float('nan')
                t_own = timed(lambda: fwd_bwd(lambda t: ssa.common_neighbour_pool(t, ssa.CommonNeighbourBatch(adj, links, 'RA')), x, g))
                say(f'  F = {F:>4}: forward {t_f:.3f} (torch {t_tf:.3f}, common_neighbour_features {t_feat:.3f}) = {pct(b_f, t_f):.1f} % of the HBM peak by the byte '
                    f'model ({b_f:,} B); forward + backward {t_fb:.3f} (torch {t_tfb:.3f}) = {pct(b_f + b_b, t_fb):.1f} % ({b_f + b_b:,} B); forward + backward '
                    f'with the plan built per call {t_own:.3f}')
                del x, g
            del plan

text = '\n'.join(lines) + '\n'
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'cn_pool_probe.txt')
with open(path, 'w') as f:
    f.write(text)
