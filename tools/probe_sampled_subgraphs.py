#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.sampled_subgraph_nodes and exact_subgraphs(max_nodes_per_hop=, ratio_per_hop=) (csrc/ss_sampled_nodes.hip,
DESIGN 3.19) -- whole-call time, the share of each pass, kept nodes and walked arcs per second.

    python tools/probe_sampled_subgraphs.py [--out profiles/sampled_subgraphs_probe.txt] [--iters 7] [--warmup 2]

At ogbl-collab size (N = 235 868, E_und = 1 179 052), 65 536 links per call (half random pairs, half edges), h = 2, the graphs of
tools/probe_exact_nodes.py:
    rank^-0.9 endpoints   max_nodes_per_hop = 100
    rank^-0.9 endpoints   ratio_per_hop = 0.2
    uniform endpoints     max_nodes_per_hop = 1000, a cap that never bites (the walk without a selection)
Per shape: sampled_subgraph_nodes and the whole exact_subgraphs call in HIP events (median, p10..p90 of --iters calls after --warmup,
every call allocating its outputs afresh); the share of each pass from the stats hook (node count, node fill, adjacency count,
adjacency fill, labels; the row pointers with their host reads apart); kept nodes per second and walked arcs per second (the in-arcs
of the kept nodes of hops 0 .. h - 1, read by the count pass and again by the fill pass); the byte model of roofline.sampled_nodes_bytes
over the time of the two node passes.  Compared in the same process, on the same links, with exact_subgraphs(max_nodes=4096): its time,
and the share of links it EMPTIES against the share emptied here (none: no max_nodes is given).  The whole exact_subgraphs call is
skipped, and said to be, for a shape that lists more than --max-nodes nodes (a ratio without a cap keeps a fifth of a hub's
neighbourhood: the induced adjacency of such rows is large)."""
import argparse
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from probe_exact_nodes import E_UND, LINKS, N, edges, timed  # noqa: E402

PASSES = ('count_ms', 'fill_ms', 'adj_count_ms', 'adj_fill_ms', 'labels_ms')
H = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sampled_subgraphs_probe.txt'))
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--max-nodes', type=int, default=40_000_000, help='listed nodes above which the whole exact_subgraphs call is skipped')
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd import roofline, sampled_nodes, subgraphs
    assert torch.cuda.is_available(), 'this probe measures on a GPU; there is nothing to report without one'
    dev = torch.device('cuda:0')
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def out(s=''):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')

    out(f'# tools/probe_sampled_subgraphs.py on {torch.cuda.get_device_name(0)}; N = {N}, E_und = {E_UND}, {LINKS} links per call (half random, '
        f'half edges); h = {H}, node_label drnl, mask_target True, seed 0; median (p10..p90) of {a.iters} calls after {a.warmup} warm-ups; '
        f'knobs: EXACT_LDS_MAX_NODES = {ssa.knobs.EXACT_LDS_MAX_NODES}, EXACT_LARGE_SLOTS = {ssa.knobs.EXACT_LARGE_SLOTS}')
    eh = ssa.ElphHashes(Namespace(max_hash_hops=H, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    graphs = {}
    for skew, cap, ratio in ((True, 100, 1.0), (True, None, 0.2), (False, 1000, 1.0)):
        if skew not in graphs:
            ei = edges(N, E_UND, skew, dev)
            gen = torch.Generator(device=dev).manual_seed(3)
            links = torch.cat([torch.randint(0, N, (LINKS // 2, 2), generator=gen, device=dev),
                               ei[:, torch.randint(0, ei.size(1), (LINKS // 2,), generator=gen, device=dev)].t()]).contiguous()
            graphs[skew] = (ei, links, torch.bincount(ei[1], minlength=N))
        ei, links, deg = graphs[skew]
        kw = dict(max_nodes_per_hop=cap, ratio_per_hop=ratio)
        tag = f'{"rank^-0.9" if skew else "uniform":9s} cap={cap} ratio={ratio}'
        rowptr, ids, hop, info = eh.sampled_subgraph_nodes(links, N, ei, return_info=True, **kw)
        sizes = torch.diff(rowptr)
        kept, expanded = int(ids.numel()), ids[hop < H]
        walked = int(deg[expanded].sum())
        out(f'{tag} | kept nodes {kept} (per link mean {kept / LINKS:.1f}, max {int(sizes.max())}) | in-arcs walked per pass {walked} '
            f'({walked / max(kept, 1):.1f} per kept node) | links that dropped a node {info["sampled_links"]} | on chip {info["lds_links"]}, '
            f'slot tier {info["large_links"]} | rows emptied {info["truncated"].numel()} of {LINKS}')
        del rowptr, ids, hop, sizes
        t_n = timed(lambda: eh.sampled_subgraph_nodes(links, N, ei, **kw), a.iters, a.warmup)
        parts = []
        for _ in range(a.iters):
            st = {}
            sampled_nodes.sampled_subgraph_nodes(eh, links, N, ei, stats=st, **kw)
            parts.append([st['count_ms'], st['fill_ms'], st['rowptr_ms']])
        c_ms, f_ms, r_ms = [float(x) for x in np.median(np.array(parts), axis=0)]
        model = roofline.sampled_nodes_bytes(LINKS, kept, int(expanded.numel()), walked)  # (the walk alone: a floor for the slot tier)
        out(f'{tag} | sampled_subgraph_nodes {t_n[0]:.3f} ms ({t_n[1]:.3f}..{t_n[2]:.3f}) | count {c_ms:.3f} ms, fill {f_ms:.3f} ms, row pointer '
            f'+ host read + allocation {r_ms:.3f} ms | {kept / (t_n[0] * 1e-3) / 1e6:.1f} M kept nodes/s | {2 * walked / (t_n[0] * 1e-3) / 1e9:.2f} G '
            f'walked arcs/s (both passes) | walk bytes {model["count"] / 1e6:.1f} + {model["fill"] / 1e6:.1f} MB = '
            f'{(model["count"] + model["fill"]) / ((c_ms + f_ms) * 1e-3) / 1e9:.1f} GB/s over the two passes')
        if kept <= a.max_nodes:
            t_s = timed(lambda: eh.exact_subgraphs(links, N, ei, **kw), a.iters, a.warmup)
            parts = []
            for _ in range(a.iters):
                st = {}
                sg = subgraphs.exact_subgraphs(eh, links, N, ei, stats=st, **kw)
                parts.append([st[k] for k in PASSES] + [st['rowptr_ms'] + st['adj_ptr_ms']])
            arcs = int(sg.nbr.numel())
            del sg
            med = [float(x) for x in np.median(np.array(parts), axis=0)]
            total = sum(med)
            out(f'{tag} | exact_subgraphs with the sampled rows {t_s[0]:.3f} ms ({t_s[1]:.3f}..{t_s[2]:.3f}) | arcs {arcs} | '
                + ' | '.join(f'{name[:-3]} {ms:.3f} ms ({ms / total:.0%})' for name, ms in zip(PASSES, med))
                + f' | row pointers, host reads, allocations {med[5]:.3f} ms ({med[5] / total:.0%})')
        else:
            out(f'{tag} | exact_subgraphs with the sampled rows: NOT RUN ({kept} listed nodes > --max-nodes {a.max_nodes})')
        if (skew, 'exact') not in graphs:  # the comparison: the unsampled rows under max_nodes = 4096, once per graph
            sg = eh.exact_subgraphs(links, N, ei, max_nodes=4096, return_info=True)
            gone, listed = int(sg.info['truncated'].numel()), int(sg.ids.numel())
            del sg
            graphs[skew, 'exact'] = (timed(lambda: eh.exact_subgraphs(links, N, ei, max_nodes=4096), a.iters, a.warmup), gone, listed)
        t_e, gone, listed = graphs[skew, 'exact']
        out(f'{tag} | exact_subgraphs(max_nodes=4096) on the same links {t_e[0]:.3f} ms ({t_e[1]:.3f}..{t_e[2]:.3f}), {listed} listed nodes | links it '
            f'empties {gone} of {LINKS} ({gone / LINKS:.1%}) against 0 here')


if __name__ == '__main__':
    main()
