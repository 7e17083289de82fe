#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.exact_subgraphs (csrc/ss_subgraph.hip) -- whole-call time, its five passes, nodes and arcs per second.

    python tools/probe_subgraphs.py [--out profiles/subgraphs_probe.txt] [--iters 7] [--warmup 2] [--sample 512]

At ogbl-collab size (N = 235 868, E_und = 1 179 052), 65 536 links per call (half random pairs, half edges), the shapes of
tools/probe_exact_nodes.py:
    uniform endpoints     h = 1 and h = 2, node_label='drnl'
    rank^-0.9 endpoints   h = 2 with max_nodes = 4 096
Per shape: the whole call in HIP events (median, p10..p90 of --iters calls after --warmup, every call allocating its outputs afresh);
the share of each of the five passes from the stats hook (node count, node fill, adjacency count, adjacency fill, labels; the row
pointers with their host reads apart); listed nodes and arcs per second; bytes written per arc against the 8 an arc holds.  Compared
in the same process with exact_subgraph_nodes on the same links (the floor: the first two passes are exactly that call) and with the
numpy restatement (tests/subgraph_restatement.py) on a sample of --sample links, the stand-in for the reference's per-link CPU loop
(a generous one: it runs whole-graph shortest paths per root, about a second per link at this size, where the reference walks h hops)."""
import argparse
import os
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from probe_exact_nodes import E_UND, LINKS, N, edges, timed  # noqa: E402

PASSES = ('count_ms', 'fill_ms', 'adj_count_ms', 'adj_fill_ms', 'labels_ms')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'subgraphs_probe.txt'))
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=512, help='links of the numpy restatement (it runs whole-graph shortest paths per root)')
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd import subgraphs
    import subgraph_restatement as sr
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    out(f'# tools/probe_subgraphs.py on {torch.cuda.get_device_name(0)}; N = {N}, E_und = {E_UND}, {LINKS} links per call (half random, '
        f'half edges); node_label drnl, mask_target True; median (p10..p90) of {a.iters} calls after {a.warmup} warm-ups; knobs: '
        f'EXACT_LDS_MAX_NODES = {ssa.knobs.EXACT_LDS_MAX_NODES}, SUBGRAPH_ADJ_SWITCH = {ssa.knobs.SUBGRAPH_ADJ_SWITCH}')
    for skew, h, cap in ((False, 1, None), (False, 2, None), (True, 2, 4096)):
        ei = edges(N, E_UND, skew, dev)
        gen = torch.Generator(device=dev).manual_seed(3)
        links = torch.cat([torch.randint(0, N, (LINKS // 2, 2), generator=gen, device=dev),
                           ei[:, torch.randint(0, ei.size(1), (LINKS // 2,), generator=gen, device=dev)].t()]).contiguous()
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
        tag = f'{"rank^-0.9" if skew else "uniform":9s} h={h} max_nodes={cap}'
        sg = eh.exact_subgraphs(links, N, ei, max_nodes=cap, return_info=True)
        sizes = torch.diff(sg.rowptr).cpu().numpy()
        nodes, arcs = int(sg.ids.numel()), int(sg.nbr.numel())
        out(f'{tag} | listed nodes {nodes} (per link mean {sizes.mean():.1f}, max {sizes.max()}) | arcs {arcs} ({arcs / max(nodes, 1):.2f} per node) | '
            f'capped links {sg.info["truncated"].numel()} | node list on chip {sg.info["lds_links"]}, large tier {sg.info["large_links"]} | '
            f'rows labelled off chip {int((sizes > min(ssa.knobs.EXACT_LDS_MAX_NODES, 2048)).sum())}')
        del sg
        t_s = timed(lambda: eh.exact_subgraphs(links, N, ei, max_nodes=cap), a.iters, a.warmup)
        t_n = timed(lambda: eh.exact_subgraph_nodes(links, N, ei, mask_target=True, max_nodes=cap), a.iters, a.warmup)
        parts = []
        for _ in range(a.iters):
            st = {}
            subgraphs.exact_subgraphs(eh, links, N, ei, max_nodes=cap, stats=st)
            parts.append([st[k] for k in PASSES] + [st['rowptr_ms'] + st['adj_ptr_ms']])
        med = [float(x) for x in np.median(np.array(parts), axis=0)]
        total = sum(med)
        out(f'{tag} | exact_subgraphs {t_s[0]:.3f} ms ({t_s[1]:.3f}..{t_s[2]:.3f}) | exact_subgraph_nodes {t_n[0]:.3f} ms '
            f'({t_n[1]:.3f}..{t_n[2]:.3f}) | subgraphs / nodes {t_s[0] / t_n[0]:.2f}')
        out(f'{tag} | ' + ' | '.join(f'{name[:-3]} {ms:.3f} ms ({ms / total:.0%})' for name, ms in zip(PASSES, med))
            + f' | row pointers, host reads, allocations {med[5]:.3f} ms ({med[5] / total:.0%})')
        written = 8 * arcs + (4 + 8 + 8) * nodes + 8 * LINKS  # nbr + weight; counts, adj_ptr and z per node; roots
        out(f'{tag} | {nodes / (t_s[0] * 1e-3) / 1e6:.1f} M listed nodes/s | {arcs / (t_s[0] * 1e-3) / 1e6:.1f} M arcs/s | '
            f'{written / max(arcs, 1):.2f} bytes written per arc by the three new passes (8 held)')
        pick = np.random.RandomState(7).choice(LINKS, a.sample, replace=False)
        lk, e = links.cpu().numpy()[pick], ei.cpu().numpy()
        t0 = time.perf_counter()
        sub = sr.restate(N, e, lk, h, mask_target=True, max_nodes=cap)
        sr.labels(sub, 'drnl', 1000)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        out(f'{tag} | numpy restatement, {a.sample} links: {cpu_ms:.0f} ms = {cpu_ms / a.sample:.2f} ms per link | exact_subgraphs '
            f'{t_s[0] / LINKS * 1e3:.2f} us per link | ratio {cpu_ms / a.sample / (t_s[0] / LINKS):.0f}')
        del ei, links
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
