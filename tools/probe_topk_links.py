#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.topk_links against the composition it replaces and against topk_candidates (csrc/ss_topk_head.hip,
DESIGN 3.12).

    python tools/probe_topk_links.py [--out profiles/topk_links_probe.txt] [--quick] [--iters 7] [--allocations 3]

Uniform endpoints, (P, p) = (128, 8), k = 100, exclude = the edge list, random sources:
    ogbl-collab size    (N = 235 868,   E_und = 1 179 052),  h = 2,  S = 64 and 1 024
    ogbl-citation2 size (N = 2 927 963, E_und = 30 387 995), h = 3,  S = 64
For each, in the same process on the same tables, HIP events around the whole call, median of --iters samples after 2 warm-ups,
repeated --allocations times on freshly allocated sources (and, for (b), links), as tools/probe_score.py does:
    (a)  topk_links
    (b)  the composition: the [S * N, 2] links built, score_links over them, the excluded pairs and u itself masked, torch.topk on the
         [S, N] floats (no id tie-break: the cheapest form of it); (b') is (b) with the links built beforehand
    (c)  topk_candidates at hops (1, 1): the floor, one estimate per pair instead of h^2 and a head
and (a)'s scores are compared with (b)'s.  roofline.topk_links_bytes gives the modelled bytes of (a)'s scan.
--quick: the collab shape at S = 64 only, 3 samples, 1 allocation."""
import argparse
import os
import statistics
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = (('ogbl-collab size', 235_868, 1_179_052, 2, (64, 1024)),
          ('ogbl-citation2 size', 2_927_963, 30_387_995, 3, (64,)))
K = 100


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def spread(xs):
    return f'{statistics.median(xs):10.2f} ms ({min(xs):.2f} .. {max(xs):.2f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'topk_links_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--allocations', type=int, default=3)
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from score_restatement import raw_head
    dev = torch.device('cuda:0')
    iters, allocs, warmup = (3, 1, 1) if a.quick else (a.iters, a.allocations, 2)
    lines = [f'topk_links against score_links + torch.topk and against topk_candidates, (P, p) = (128, 8), k = {K}, exclude = the edge list, '
             f'uniform graphs, {torch.cuda.get_device_name(0)}; ms = median over {allocs} allocations (min .. max over allocations) of the '
             f'median of {iters} samples']
    for name, n, e_und, h, counts in (SHAPES[:1] if a.quick else SHAPES):
        rng = np.random.RandomState(1)
        e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
        ei = torch.from_numpy(np.concatenate([e, e[::-1]], axis=1)).to(dev)
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
        table, cards = eh.build_hash_tables(n, ei)
        nf = h * (h + 2)
        head = ssa.StructureHead(**raw_head(nf, 3))
        every = torch.arange(n, device=dev)
        for S in (counts[:1] if a.quick else counts):
            g = torch.Generator(device=dev).manual_seed(S)
            ta, tb, tb1, tc = [], [], [], []
            same = True
            for _ in range(allocs):
                src = torch.randint(0, n, (S,), device=dev, generator=g)  # a fresh allocation (and fresh sources) every time
                # the composition's exclusion: positions in the [S, N] score matrix of (u, u) and of every listed edge u -> v
                row_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
                row_of[src] = torch.arange(S, device=dev)  # (a duplicate source keeps one row: the timing does not mind)
                hit = row_of[ei[0]] >= 0
                masked = torch.cat([row_of[ei[0][hit]] * n + ei[1][hit], torch.arange(S, device=dev) * n + src])

                def make_links():
                    return torch.stack([src[:, None].expand(S, n).reshape(-1), every.repeat(S)], 1)

                def compose(links=None):
                    sc = eh.score_links(make_links() if links is None else links, table, cards, head)
                    sc[masked] = float('-inf')
                    return torch.topk(sc.view(S, n), K, dim=1)

                ta.append(timed(lambda: eh.topk_links(src, table, cards, K, head, exclude=ei), warmup, iters))
                tb.append(timed(compose, warmup, iters))
                links = make_links()
                tb1.append(timed(lambda: compose(links), warmup, iters))
                del links
                tc.append(timed(lambda: eh.topk_candidates(src, table, K, hops=(1, 1), exclude=ei), warmup, iters))
                got = eh.topk_links(src, table, cards, K, head, exclude=ei)[1]
                same = same and bool(torch.equal(got, compose().values))
                del src, masked, row_of
                torch.cuda.empty_cache()
            ma = statistics.median(ta)
            model = ssa.roofline.topk_links_bytes(n, S, h, 128, 256)
            lines.append(f'{name}, h = {h}, S = {S} ({S * n / 1e6:.1f} M pairs): modelled bytes of the scan {model / 1e6:.1f} MB '
                         f'({ssa.roofline.topk_links_sources(h, 128, 256)} sources staged per workgroup), of the composition\'s query '
                         f'{ssa.roofline.score_query_bytes(S * n, h=h) / 1e6:.1f} MB + {16 * S * n / 1e6:.1f} MB of links\n'
                         f"  (a)  topk_links                  {spread(ta)}   = {S * n / ma / 1e6:.2f} G pairs/s\n"
                         f"  (b)  links + score_links + topk  {spread(tb)}   = {statistics.median(tb) / ma:.2f} x (a)\n"
                         f"  (b') score_links + topk          {spread(tb1)}   = {statistics.median(tb1) / ma:.2f} x (a)\n"
                         f"  (c)  topk_candidates (1, 1)      {spread(tc)}   = {statistics.median(tc) / ma:.2f} x (a); "
                         f"scores of (a) == scores of (b): {same}")
            print(lines[-1], flush=True)
        del table, cards, ei, every
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
