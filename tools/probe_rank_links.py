#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.rank_links against topk_links and against the composition score_links + compare (csrc/ss_rank.hip,
DESIGN 3.13).

    python tools/probe_rank_links.py [--out profiles/rank_links_probe.txt] [--quick] [--iters 7] [--allocations 3]

The shapes of tools/probe_topk_links.py -- uniform endpoints, (P, p) = (128, 8), exclude = the edge list:
    ogbl-collab size    (N = 235 868,   E_und = 1 179 052),  h = 2,  S = 64 and 1 024
    ogbl-citation2 size (N = 2 927 963, E_und = 30 387 995), h = 3,  S = 64
with S links (u, t): distinct random sources, random targets.  For each, in the same process on the same tables, HIP events around the
whole call, median of --iters samples after 2 warm-ups, repeated --allocations times on freshly allocated links:
    (a)  rank_links;  (a0) the same without exclude: the threshold launch and the scan alone
    (b)  topk_links(k = 100) of the links' sources: the baseline the scan is measured against (same arithmetic per pair, plus the
         keys, the exclude pass over them and the selection)
    (c)  the composition: the [S * N, 2] links built, score_links over them, u, t and the excluded pairs masked, two compares and two
         row sums on the [S, N] floats; where the links fit (--max-link-bytes)
and (a)'s counts are compared with (c)'s.  roofline.rank_links_bytes gives the modelled bytes of (a)'s scan.
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_links_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--allocations', type=int, default=3)
    ap.add_argument('--max-link-bytes', type=int, default=8 << 30, help='the composition is skipped where its link list is larger')
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from score_restatement import raw_head
    dev = torch.device('cuda:0')
    iters, allocs, warmup = (3, 1, 1) if a.quick else (a.iters, a.allocations, 2)
    lines = [f'rank_links against topk_links (k = {K}) and against score_links + compare, (P, p) = (128, 8), exclude = the edge list, '
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
            fits = 16 * S * n <= a.max_link_bytes
            ta, ta0, tb, tc = [], [], [], []
            same = True
            for _ in range(allocs):
                # a fresh allocation (and fresh links) every time; distinct sources, so that row q of the composition is link q's
                links = torch.stack([torch.randperm(n, device=dev, generator=g)[:S], torch.randint(0, n, (S,), device=dev, generator=g)], 1)
                src, rows = links[:, 0].contiguous(), torch.arange(S, device=dev)
                ta.append(timed(lambda: eh.rank_links(links, table, cards, head, exclude=ei), warmup, iters))
                ta0.append(timed(lambda: eh.rank_links(links, table, cards, head), warmup, iters))
                tb.append(timed(lambda: eh.topk_links(src, table, cards, K, head, exclude=ei), warmup, iters))
                if fits:
                    # the composition's candidate set: positions in the [S, N] score matrix of (u, u), (u, t) and every listed edge u -> v
                    row_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
                    row_of[src] = rows
                    hit = row_of[ei[0]] >= 0
                    masked = torch.cat([row_of[ei[0][hit]] * n + ei[1][hit], rows * n + src, rows * n + links[:, 1]])

                    def compose():
                        pairs = torch.stack([src[:, None].expand(S, n).reshape(-1), every.repeat(S)], 1)
                        sc = eh.score_links(pairs, table, cards, head)
                        thr = sc.view(S, n)[rows, links[:, 1]].clone()
                        sc[masked] = float('nan')  # (no compare holds)
                        sc = sc.view(S, n)
                        return (sc > thr[:, None]).sum(1), (sc == thr[:, None]).sum(1)

                    tc.append(timed(compose, warmup, iters))
                    got, want = eh.rank_links(links, table, cards, head, exclude=ei), compose()
                    same = same and bool(torch.equal(got[0], want[0])) and bool(torch.equal(got[1], want[1]))
                    del row_of, hit, masked, want
                del links, src
                torch.cuda.empty_cache()
            ma = statistics.median(ta)
            model = ssa.roofline.rank_links_bytes(n, S, h, 128, 256)
            text = (f'{name}, h = {h}, S = {S} ({S * n / 1e6:.1f} M pairs): modelled bytes of the scan {model / 1e6:.1f} MB '
                    f'({ssa.roofline.rank_links_queries(h, 128, 256)} links staged per workgroup; topk_links\' scan '
                    f'{ssa.roofline.topk_links_bytes(n, S, h, 128, 256) / 1e6:.1f} MB), of the composition\'s query '
                    f'{ssa.roofline.score_query_bytes(S * n, h=h) / 1e6:.1f} MB + {16 * S * n / 1e6:.1f} MB of links\n'
                    f"  (a)  rank_links                  {spread(ta)}   = {S * n / ma / 1e6:.2f} G pairs/s\n"
                    f"  (a0) rank_links, no exclude      {spread(ta0)}   = {statistics.median(ta0) / ma:.2f} x (a)\n"
                    f"  (b)  topk_links, k = {K}         {spread(tb)}   = {statistics.median(tb) / ma:.2f} x (a)\n")
            if fits:
                text += (f"  (c)  links + score_links + compare {spread(tc)}   = {statistics.median(tc) / ma:.2f} x (a); "
                         f"counts of (a) == counts of (c): {same}")
            else:
                text += f'  (c)  not measured: its link list of {16 * S * n / 2 ** 30:.1f} GiB is over --max-link-bytes'
            lines.append(text)
            print(lines[-1], flush=True)
        del table, cards, ei, every
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
