"""probe (one GPU): the readouts of subgraph_sketching_amd.pooling on SEAL-shaped batches -> profiles/pooling_probe.txt

Collab-size graph, 65 536 links, h = 1 and 2, uniform and rank^-0.9 endpoints with max_nodes_per_hop = 100 (exact_subgraphs' sampled
rows), F = 32 and 128.  Every readout forward and forward + backward (k = sort_pool_k(batch) for sort pool) beside the torch
composition a user writes without PyG, on the same GPU and the same batch: dense batch + sort + gather (tests/pooling_restatement.py's
torch_sort_pool), index_add_ (float atomics), and the reference's centre pooling with its np.unique host round trip.  The share of
the byte model (roofline.segment_pool_bytes / sort_pool_bytes over the time, against the HBM peak) stands next to each forward time.
Nothing is gated: the file is a measurement to quote."""
import argparse
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from probe_exact_nodes import E_UND, LINKS, N, edges, timed  # noqa: E402
import pooling_restatement as pr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pooling_probe.txt'))
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--dense-gb', type=float, default=40.0, help='dense batches above this size are not built (the torch sort pool is then not run)')
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd import roofline
    assert torch.cuda.is_available(), 'this probe measures on a GPU; there is nothing to report without one'
    dev = torch.device('cuda:0')
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def out(s=''):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')

    def both(fn, x, g):
        """forward and forward + backward medians of fn(x)"""
        with torch.no_grad():
            f = timed(lambda: fn(x), a.iters, a.warmup)[0]

        def step():
            x.grad = None
            fn(x).backward(g)
        return f, timed(step, a.iters, a.warmup)[0]

    def share(model, ms):
        return f'{model / 1e6:.1f} MB = {100 * model / (ms * 1e-3) / 1e9 / roofline.HBM_PEAK_GBS:.1f} % of the HBM peak'

    out(f'# tools/probe_pooling.py on {torch.cuda.get_device_name(0)}; N = {N}, E_und = {E_UND}, {LINKS} links per batch (half random, half edges), '
        f'max_nodes_per_hop = 100, node_label None; median of {a.iters} calls after {a.warmup} warm-ups; sort capacity C = {ssa.pooling.SORT_CAPACITY}')
    for skew in (False, True):
        ei = edges(N, E_UND, skew, dev)
        gen = torch.Generator(device=dev).manual_seed(3)
        links = torch.cat([torch.randint(0, N, (LINKS // 2, 2), generator=gen, device=dev),
                           ei[:, torch.randint(0, ei.size(1), (LINKS // 2,), generator=gen, device=dev)].t()]).contiguous()
        for h in (1, 2):
            eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
            sg = eh.exact_subgraphs(links, N, ei, node_label=None, max_nodes_per_hop=100)
            batch, sizes = sg.batch(), torch.diff(sg.rowptr)
            T, L, max_n = int(sg.ids.numel()), sg.num_links, int(sizes.max())
            k = min(ssa.sort_pool_k(sg), ssa.pooling.SORT_CAPACITY)
            tag = f'{"rank^-0.9" if skew else "uniform":9s} h={h}'
            out(f'{tag} | T = {T} nodes in L = {L} graphs (mean {T / L:.1f}, max {max_n}) | k = sort_pool_k = {k}')
            for F in (32, 128):
                x = torch.randn(T, F, device=dev, requires_grad=True)
                for name, ours, theirs, model in (
                        ('add pool ', lambda t: ssa.global_add_pool(t, sg), lambda t: pr.torch_segment_pool(t, batch, L), roofline.segment_pool_bytes(T, L, F)),
                        ('mean pool', lambda t: ssa.global_mean_pool(t, sg), lambda t: pr.torch_segment_pool(t, batch, L, True), roofline.segment_pool_bytes(T, L, F)),
                        ('centre   ', lambda t: ssa.center_pool(t, sg), lambda t: pr.torch_center_pool(t, batch), 2 * L * 4 * F + L * 4 * F + 16 * L),
                        ('sort pool', lambda t: ssa.global_sort_pool(t, sg, k), lambda t: pr.torch_sort_pool(t, batch, k, size=L), roofline.sort_pool_bytes(T, L, F, k))):
                    g = torch.randn_like(ours(x.detach()))
                    f_ms, fb_ms = both(ours, x, g)
                    line = f'{tag} F={F:<3} {name} | HIP forward {f_ms:.3f} ms ({share(model, f_ms)}), forward + backward {fb_ms:.3f} ms'
                    dense_gb = L * max_n * F * 4 / 1e9
                    if name.startswith('sort') and dense_gb > a.dense_gb:
                        line += f' | torch: NOT RUN (a dense batch of {dense_gb:.1f} GB)'
                    else:
                        try:
                            tf_ms, tfb_ms = both(theirs, x, g)
                            line += f' | torch composition forward {tf_ms:.3f} ms, forward + backward {tfb_ms:.3f} ms ({tfb_ms / fb_ms:.1f}x)'
                        except Exception as exc:  # (an allocation that does not fit)
                            line += f' | torch: failed ({type(exc).__name__}: {str(exc)[:60]})'
                    out(line)
                del x
            ssa.pooling.check_errors()
            del sg, batch


if __name__ == '__main__':
    main()
