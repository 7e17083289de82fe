#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.exact_subgraph_nodes (csrc/ss_exact_nodes.hip) -- whole-call time, its passes, nodes per second.

    python tools/probe_exact_nodes.py [--out profiles/exact_nodes_probe.txt] [--iters 7] [--warmup 2]

At ogbl-collab size (N = 235 868, E_und = 1 179 052), 65 536 links per call (half random pairs, half edges):
    uniform endpoints     h = 1 and h = 2, no cap
    rank^-0.9 endpoints   h = 2 with max_nodes (hubs: the uncapped lists would hold a large part of the graph per link)
Per shape: the whole call in HIP events (median, p10..p90 of --iters calls after --warmup, every call allocating its outputs afresh),
exact_subgraph_features on the same links in the same process (the floor: what the two BFSs alone cost, once), the count pass, the
row pointer (cumulative sum, the host read of the total, the allocation) and the fill pass from the stats hook, the tier split, listed
nodes per second, and bytes written per listed node (ids + dist + the counts and the row pointer) against the 10 bytes a node holds.
The sort has no figure of its own: on chip it runs inside the fill kernel, and the large tier emits in id order without one."""
import argparse
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, E_UND, LINKS = 235_868, 1_179_052, 65536


def edges(n, e_und, skew, device, seed=11):
    """symmetric int64 [2, 2 e_und]: endpoints uniform, or (skew) one endpoint with probability proportional to rank^-0.9"""
    gen = torch.Generator(device=device).manual_seed(seed)
    src = torch.randint(0, n, (e_und,), generator=gen, device=device)
    if skew:
        cdf = torch.cumsum(torch.arange(1, n + 1, dtype=torch.float64, device=device) ** -0.9, 0)
        r = torch.rand((e_und,), generator=gen, device=device, dtype=torch.float64) * cdf[-1]
        dst = torch.searchsorted(cdf, r).clamp_(max=n - 1)
    else:
        dst = torch.randint(0, n, (e_und,), generator=gen, device=device)
    e = torch.stack([src, dst])
    return torch.cat([e, e.flip(0)], dim=1)


def timed(fn, iters, warmup):
    """(median, p10, p90) ms of fn() in HIP events"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exact_nodes_probe.txt'))
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd import exact_nodes
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    out(f'# tools/probe_exact_nodes.py on {torch.cuda.get_device_name(0)}; N = {N}, E_und = {E_UND}, {LINKS} links per call (half random, '
        f'half edges); median (p10..p90) of {a.iters} calls after {a.warmup} warm-ups; knobs: EXACT_LDS_MAX_NODES = '
        f'{ssa.knobs.EXACT_LDS_MAX_NODES}, EXACT_LARGE_SLOTS = {ssa.knobs.EXACT_LARGE_SLOTS}')
    for skew, h, cap in ((False, 1, None), (False, 2, None), (True, 2, 4096)):
        ei = edges(N, E_UND, skew, dev)
        gen = torch.Generator(device=dev).manual_seed(3)
        links = torch.cat([torch.randint(0, N, (LINKS // 2, 2), generator=gen, device=dev),
                           ei[:, torch.randint(0, ei.size(1), (LINKS // 2,), generator=gen, device=dev)].t()]).contiguous()
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
        tag = f'{"rank^-0.9" if skew else "uniform":9s} h={h} max_nodes={cap}'
        rowptr, ids, dist, info = eh.exact_subgraph_nodes(links, N, ei, max_nodes=cap, return_info=True)
        sizes = torch.diff(rowptr).cpu().numpy()
        nodes = int(ids.numel())
        out(f'{tag} | listed nodes {nodes} (per link mean {sizes.mean():.1f}, p99 {np.percentile(sizes, 99):.0f}, max {sizes.max()}) | capped links '
            f'{info["truncated"].numel()} | counted on chip {info["lds_links"]}, large tier {info["large_links"]}')
        del rowptr, ids, dist
        t_n = timed(lambda: eh.exact_subgraph_nodes(links, N, ei, max_nodes=cap), a.iters, a.warmup)
        t_f = timed(lambda: eh.exact_subgraph_features(links, N, ei), a.iters, a.warmup)
        parts = []
        for _ in range(a.iters):
            st = {}
            exact_nodes.exact_subgraph_nodes(eh, links, N, ei, max_nodes=cap, stats=st)
            parts.append((st['count_ms'], st['rowptr_ms'], st['fill_ms']))
        c, r, f = (float(x) for x in np.median(np.array(parts), axis=0))
        written = 10 * nodes + 4 * LINKS + 8 * (LINKS + 1)
        out(f'{tag} | exact_subgraph_nodes {t_n[0]:.3f} ms ({t_n[1]:.3f}..{t_n[2]:.3f}) | exact_subgraph_features {t_f[0]:.3f} ms '
            f'({t_f[1]:.3f}..{t_f[2]:.3f}) | nodes / features {t_n[0] / t_f[0]:.2f}')
        out(f'{tag} | count pass {c:.3f} ms ({c / (c + r + f):.0%}) | row pointer + host read + allocation {r:.3f} ms ({r / (c + r + f):.0%}) | '
            f'fill pass with its sort {f:.3f} ms ({f / (c + r + f):.0%})')
        out(f'{tag} | {nodes / (t_n[0] * 1e-3) / 1e6:.1f} M listed nodes/s | {written / max(nodes, 1):.2f} bytes written per listed node '
            f'(10 held) | {written / (t_n[0] * 1e-3) / 1e9:.2f} GB/s of output')
        del ei, links
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
