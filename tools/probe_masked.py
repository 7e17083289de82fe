#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.get_subgraph_features(mask_target=edge_index) (csrc/ss_masked.hip).

    python tools/probe_masked.py [--out profiles/masked_probe.txt] [--quick] [--iters 50]

At ogbl-collab size (N = 235 868, E_und = 1 179 052) with uniform endpoints and with endpoint weights ~ rank^-0.9 (the generator of
bench.py), h = 2 and h = 3, 65 536 links drawn from the edges, it prints per line (HIP events around the whole call, 10 warm-ups, median
of --iters (>= 50) samples, nothing read by the host inside a sample):
  (i)   the masked call on the edge links, and roofline.masked_query_bytes / time
  (ii)  the plain get_subgraph_features on the same links: the floor -- same output bytes, 2h row gathers per link
  (iii) the only stand-in there was: update_hash_tables(removed=batch) + plain query + update_hash_tables(added=batch)
  (iv)  the masked call and the plain call on 65 536 links that are NOT edges: the masked call's extra is the classify pass
A line whose masked call would move more than --max-bytes by the byte model (links at hubs at h = 3) is reported with that figure and not run.
--quick: uniform, h = 2 only, 12 samples."""
import argparse
import os
import statistics
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, E_UND, L = 235_868, 1_179_052, 65_536


def graph(n, e_und, kind, seed=1):
    rng = np.random.RandomState(seed)
    if kind == 'uniform':
        e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    else:  # endpoint weights ~ rank^-0.9
        w = np.arange(1, n + 1, dtype=np.float64) ** -0.9
        cdf = np.cumsum(w / w.sum())
        e = np.minimum(np.stack([np.searchsorted(cdf, rng.random_sample(e_und)), rng.randint(0, n, size=e_und)]).astype(np.int64), n - 1)
    return np.concatenate([e, e[::-1]], axis=1)


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
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return f'{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'masked_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--skip-slow', action='store_true', help='leave out the rank^-0.9 / h = 3 line')
    ap.add_argument('--max-bytes', type=float, default=2e12, help='a line whose masked call would move more than this is reported, not run')
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    dev = torch.device('cuda:0')
    iters, warmup = (12, 3) if a.quick else (max(a.iters, 50), 10)
    lines = [f'masked query, (P, p) = (128, 8), N = {N}, E_und = {E_UND}, {L} links, {torch.cuda.get_device_name(0)}; '
             f'ms = median (min .. max) of {iters}']
    for kind in (('uniform',) if a.quick else ('uniform', 'rank^-0.9')):
        ei_np = graph(N, E_UND, kind)
        ei = torch.from_numpy(ei_np).to(dev)
        deg = np.bincount(ei_np[1], minlength=N)
        rng = np.random.RandomState(5)
        pick = rng.choice(ei_np.shape[1] // 2, size=L, replace=False)
        edges_np = np.ascontiguousarray(ei_np[:, pick].T)
        edges = torch.from_numpy(edges_np).to(dev)
        batch = torch.from_numpy(np.concatenate([ei_np[:, pick], ei_np[:, pick + ei_np.shape[1] // 2]], axis=1)).to(dev)
        keep = np.ones(ei_np.shape[1], dtype=bool)
        keep[pick] = False
        keep[pick + ei_np.shape[1] // 2] = False
        ei_minus = torch.from_numpy(np.ascontiguousarray(ei_np[:, keep])).to(dev)
        keys = np.unique(ei_np[0] * N + ei_np[1])
        c = rng.randint(0, N, size=(2 * L, 2)).astype(np.int64)
        c = c[(c[:, 0] != c[:, 1]) & ~np.isin(c[:, 0] * N + c[:, 1], keys) & ~np.isin(c[:, 1] * N + c[:, 0], keys)][:L]
        non = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
        d_mean = float(deg[edges_np].mean())
        two_hop = float(np.mean([deg[ei_np[0][ei_np[1] == x]].sum() for x in edges_np[:256].reshape(-1)]))
        for h in ((2,) if a.quick else (2, 3)):
            n_edge = int((edges_np[:, 0] != edges_np[:, 1]).sum())
            predicted = ssa.roofline.masked_query_bytes(L, n_edge, d_mean, h=h, two_hop_walks=two_hop)
            if a.skip_slow and kind != 'uniform' and h == 3 or predicted > a.max_bytes:
                lines.append(f'{kind} h = {h}: mean in-degree of the endpoints {d_mean:.1f}, 2-hop in-walks {two_hop:.0f}: the masked call would move '
                             f'{predicted / 1e9:.0f} GB per sample (roofline.masked_query_bytes) -- NOT RUN (above --max-bytes, or --skip-slow)')
                print(lines[-1], flush=True)
                continue
            eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
            eh.strict_bounds = False
            table, cards = eh.build_hash_tables(N, ei)
            _, dbg = eh.get_subgraph_features(edges, table, cards, mask_target=ei, return_debug=True)
            n_masked = int(dbg['masked'].sum())
            same = bool(torch.equal(eh.get_subgraph_features(non, table, cards, mask_target=ei).view(torch.int32),
                                    eh.get_subgraph_features(non, table, cards).view(torch.int32)))
            slow = predicted > 2e10  # seconds per sample: a tenth of the samples
            it, wu = (max(3, iters // 10), 1) if slow else (iters, warmup)
            t_masked = timed(lambda: eh.get_subgraph_features(edges, table, cards, mask_target=ei), wu, it)
            t_plain = timed(lambda: eh.get_subgraph_features(edges, table, cards), warmup, iters)

            def stand_in():
                eh.update_hash_tables(table, cards, N, ei_minus, removed=batch)
                eh.get_subgraph_features(edges, table, cards)
                eh.update_hash_tables(table, cards, N, ei, added=batch)
            t_stand = timed(stand_in, wu, it)
            t_non_m = timed(lambda: eh.get_subgraph_features(non, table, cards, mask_target=ei), warmup, iters)
            t_non_p = timed(lambda: eh.get_subgraph_features(non, table, cards), warmup, iters)
            nbytes = ssa.roofline.masked_query_bytes(L, n_masked, d_mean, h=h, two_hop_walks=two_hop)
            lines.append(f'{kind} h = {h}: mean in-degree of the endpoints {d_mean:.1f}, 2-hop in-walks {two_hop:.0f}, links masked {n_masked} / {L}'
                         f'{" (samples: " + str(it) + ")" if slow else ""}\n'
                         f'  (i)   masked call           {fmt(t_masked)} = {t_masked[0] / t_plain[0]:.1f} x plain; {nbytes / 1e6:.1f} MB -> {nbytes / t_masked[0] / 1e6:.1f} GB/s\n'
                         f'  (ii)  plain query           {fmt(t_plain)}\n'
                         f'  (iii) update + plain + update {fmt(t_stand)} = {t_stand[0] / t_masked[0]:.2f} x masked call\n'
                         f'  (iv)  non-edges: masked {fmt(t_non_m)}, plain {fmt(t_non_p)}: + {1000 * (t_non_m[0] - t_non_p[0]):.1f} us '
                         f'({t_non_m[0] / t_non_p[0]:.2f} x); rows bit-identical: {same}')
            print(lines[-1], flush=True)
            del table, cards
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
