#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.score_links against the feature query it replaces (csrc/ss_head.hpp).

    python tools/probe_score.py [--out profiles/score_probe.txt] [--quick] [--iters 30] [--allocations 5]

Two shapes, uniform endpoints, (P, p) = (128, 8), uniformly random links:
    ogbl-collab size    (N = 235 868,   E_und = 1 179 052),  h = 2,  B = 65 536 and 4 194 304
    ogbl-citation2 size (N = 2 927 963, E_und = 30 387 995), h = 3,  B = 261 424 and 8 388 608
For each, in the same process on the same tables, HIP events around the whole call, median of --iters samples after 5 warm-ups:
    (a) get_subgraph_features                       -- writes [B, h(h+2)] rows
    (b) (a) + the torch head on the rows            -- Linear, BatchNorm1d (eval), ReLU, the output columns: what a model does today
    (c) score_links                                 -- writes [B] floats
The three are measured --allocations times, each time on freshly allocated link / output tensors: the same launch is 5-10 % faster
or slower from one allocation to the next (profiles/round6_query_instep.txt), so (c) - (a) means something only against the spread of
(a) over allocations, which every line reports.  roofline.score_query_bytes / pair_query_bytes give the modelled bytes of (c) / (a).
--quick: the collab shape at B = 65 536 only, 8 samples, 2 allocations."""
import argparse
import os
import statistics
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (('ogbl-collab size', 235_868, 1_179_052, 2, (65_536, 4_194_304)),
          ('ogbl-citation2 size', 2_927_963, 30_387_995, 3, (261_424, 8_388_608)))


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


class Branch(torch.nn.Module):
    """the label branch of both reference models, nothing else behind `lin`"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.label_lin_layer = torch.nn.Linear(dim, dim)
        self.bn_labels = torch.nn.BatchNorm1d(dim)
        self.lin = torch.nn.Linear(dim, 1)

    def forward(self, sf):
        return self.lin(torch.relu(self.bn_labels(self.label_lin_layer(sf)))).squeeze(-1)


def spread(xs):
    return f'{statistics.median(xs) * 1000:9.1f} us ({min(xs) * 1000:.1f} .. {max(xs) * 1000:.1f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--allocations', type=int, default=5)
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    dev = torch.device('cuda:0')
    iters, allocs, warmup = (8, 2, 2) if a.quick else (a.iters, a.allocations, 5)
    lines = [f'score_links against get_subgraph_features, (P, p) = (128, 8), uniform graphs, random links, {torch.cuda.get_device_name(0)}; '
             f'us = median over {allocs} allocations (min .. max over allocations) of the median of {iters} samples']
    for name, n, e_und, h, batches in (SHAPES[:1] if a.quick else SHAPES):
        rng = np.random.RandomState(1)
        e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
        ei = torch.from_numpy(np.concatenate([e, e[::-1]], axis=1)).to(dev)
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
        table, cards = eh.build_hash_tables(n, ei)
        del ei
        nf = h * (h + 2)
        torch.manual_seed(3)
        model = Branch(nf).to(dev)
        with torch.no_grad():
            model(torch.rand(4096, nf, device=dev) * 100)  # running statistics of some kind
        model.eval()
        head = ssa.StructureHead.from_module(model)
        for B in (batches[:1] if a.quick else batches):
            g = torch.Generator(device=dev).manual_seed(B)
            ta, tb, tc = [], [], []
            worst = 0.0
            for _ in range(allocs):
                links = torch.randint(0, n, (B, 2), device=dev, generator=g)   # a fresh allocation (and fresh links) every time
                rows, scores = torch.empty((B, nf), device=dev), torch.empty((B,), device=dev)

                def feature_call():
                    return eh.get_subgraph_features(links, table, cards, out=rows)

                def torch_head():
                    with torch.no_grad():
                        return model(eh.get_subgraph_features(links, table, cards, out=rows))

                def score_call():
                    return eh.score_links(links, table, cards, head, out=scores)

                ta.append(timed(feature_call, warmup, iters))
                tb.append(timed(torch_head, warmup, iters))
                tc.append(timed(score_call, warmup, iters))
                worst = max(worst, float((score_call() - torch_head()).abs().max()))
                del links, rows, scores
            ma, mc = statistics.median(ta), statistics.median(tc)
            lines.append(f'{name}, h = {h}, B = {B}: modelled bytes (a) {ssa.roofline.pair_query_bytes(B, h=h) / 1e6:.1f} MB, '
                         f'(c) {ssa.roofline.score_query_bytes(B, h=h) / 1e6:.1f} MB\n'
                         f'  (a) get_subgraph_features   {spread(ta)}\n'
                         f'  (b) (a) + torch head        {spread(tb)}   = {statistics.median(tb) / ma:.2f} x (a)\n'
                         f'  (c) score_links             {spread(tc)}   = {mc / ma:.3f} x (a), {mc / statistics.median(tb):.3f} x (b); '
                         f'spread of (a) over allocations {(max(ta) - min(ta)) / ma * 100:.1f} %; max |(c) - (b)| = {worst:.3e}')
            print(lines[-1], flush=True)
        del table, cards
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
