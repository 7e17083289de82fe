"""probe: heuristics.common_neighbour_features on the bench's own graph (collab size), F = 128 -> profiles/cn_features_probe.txt

For 65 536 and 1 M links with uniform endpoints and with endpoints drawn by degree rank^-0.9 (the large rows meet each other):
the fused call (ss_common_neighbour_pool), the list followed by x[ids] * coef and a segmented sum in torch, scipy's
(A[src].multiply(A_[dst])) @ x on the host (65 536 links only), the hits per link, and the fused launch against its byte model.
Nothing is gated: the file is a measurement to quote."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import bench
from subgraph_sketching_amd import heuristics, roofline

dev = torch.device('cuda:0')
n, F = bench.N_NODES, 128
ei = bench.synthetic_graph()
A = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.float32), (ei[0], ei[1])), shape=(n, n))
deg = np.diff(A.indptr)
by_degree = np.argsort(-deg, kind='stable')
adj = heuristics.DeviceAdjacency(A, dev)
x = torch.randn(n, F, device=dev)
lines = [f'graph: bench.synthetic_graph(), N = {n}, stored entries = {A.nnz}, largest row = {deg.max()}, F = {F}, weighting RA']


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def draw(kind, count, seed):
    rng = np.random.RandomState(seed)
    if kind == 'uniform':
        return rng.randint(0, n, size=(count, 2)).astype(np.int64)
    w = np.arange(1, n + 1, dtype=np.float64) ** -0.9
    cdf = np.cumsum(w / w.sum())
    return by_degree[np.minimum(np.searchsorted(cdf, rng.random_sample((count, 2))), n - 1)].astype(np.int64)


def torch_from_lists(cn):
    rows = torch.repeat_interleave(torch.arange(len(cn.rowptr) - 1, device=dev), cn.rowptr[1:] - cn.rowptr[:-1])
    out = torch.zeros((len(cn.rowptr) - 1, F), device=dev)
    return out.index_add_(0, rows, x[cn.ids] * cn.coef[:, None])  # (float atomics: a sum in no fixed order)


for kind in ('uniform', 'rank^-0.9'):
    for count in (65536, 1 << 20):
        links = draw(kind, count, 7)
        lk = torch.from_numpy(links).to(dev)
        out = torch.empty((count, F), device=dev)
        t_fused = timed(lambda: heuristics.common_neighbour_features(adj, lk, x, weighting='RA', batch_size=count, out=out), 10)
        t_lists = timed(lambda: heuristics.common_neighbours(adj, lk, weighting='RA'), 5)
        cn = heuristics.common_neighbours(adj, lk, weighting='RA')
        t_torch = timed(lambda: torch_from_lists(cn), 5)
        T = int(cn.ids.numel())
        per_link = (cn.rowptr[1:] - cn.rowptr[:-1]).float()
        entries = int(deg[links[:, 0]].sum() + deg[links[:, 1]].sum())
        model = roofline.cn_features_bytes(count, entries, T, F, weighted=True)['pool']
        close = bool(torch.allclose(torch_from_lists(cn), out, rtol=1e-4, atol=1e-5))
        lines.append(f'{kind:>10} endpoints, {count:>7} links: hits/link mean {per_link.mean().item():.3f} max {int(per_link.max().item())}, '
                     f'T = {T}; fused {t_fused:.3f} ms = {model / t_fused / 1e6:.0f} GB/s of its byte model ({model:,} B, '
                     f'{100 * model / t_fused / 1e6 / roofline.HBM_PEAK_GBS:.1f} % of the HBM peak); list {t_lists:.3f} ms + torch gather and '
                     f'segmented sum {t_torch:.3f} ms (allclose to the fused rows: {close})')
        if count == 65536:
            xh = x.cpu().numpy()
            t0 = time.perf_counter()
            A_ = A.multiply(heuristics.DeviceAdjacency.multiplier(adj, 'RA').cpu().numpy()).tocsr()
            ref = (A[links[:, 0]].multiply(A_[links[:, 1]])) @ xh
            t_host = (time.perf_counter() - t0) * 1e3
            err = float(np.abs(ref - out.cpu().numpy()).max())
            lines.append(f'{"":>10}            scipy on the host: {t_host:.1f} ms (max |difference| to the fused rows {err:.2e})')

text = '\n'.join(lines) + '\n'
print(text, end='')
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'cn_features_probe.txt')
with open(path, 'w') as f:
    f.write(text)
