#!/usr/bin/env python3
"""probe (one GPU): the LSH index over the MinHash tables (csrc/ss_lsh.hip, lsh.py) against the one-vs-all scan.

    python tools/probe_lsh.py [--out profiles/lsh_probe.txt] [--quick] [--iters 5] [--citation2]

Shapes: ogbl-collab size (N = 235 868, E_und = 1 179 052), h = 2, S = 1 024 distinct random sources, k = 100, exclude = the edge list,
(P, p) = (128, 8), on two graphs -- uniform endpoints (the shape of tools/probe_topk_links.py; neighbourhoods of two random nodes barely
overlap) and the power-law endpoints of the tests' generator (hubs shared by many neighbourhoods); with --citation2 also ogbl-citation2
size (N = 2 927 963, E_und = 30 387 995), h = 3, S = 64, uniform endpoints.  For each graph, in one process on the same tables:
    topk_links(k)                                   the scan every index is compared with, HIP events around the whole call
    per (hop, rows, bands) of the grid, max_bucket = 1 024:
        build_lsh_index                             time of the whole call and of its ss_lsh_band_keys launch alone (against
                                                    roofline.lsh_band_keys_bytes at roofline.HBM_PEAK_GBS), index bytes, skipped buckets
        lsh_candidates                              mean / max candidates per source
        topk_links_lsh(k)                           time of the whole call; recall@k = |its ids & the scan's ids| / |the scan's ids|, mean
                                                    over the sources
ms = median of --iters samples after one warm-up.  --quick: the uniform collab shape, three grid points, 2 samples."""
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

K = 100
GRID = ((1, 1, 32), (1, 2, 64), (1, 4, 32), (2, 2, 64), (2, 4, 32), (2, 8, 16))


def uniform_edges(n, e_und, seed=1):
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def power_law_edges(n, e_und, seed=7):
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, size=e_und)
    dst = np.minimum((n * rng.random_sample(e_und) ** 3).astype(np.int64), n - 1)
    e = np.stack([src, dst]).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def timed(fn, iters, warmup=1):
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


def recall(ids, want):
    """mean over the sources of |ids & want| / |want| (rows of node ids, -1 = padding); sources whose scan row is empty are left out"""
    hit = ((ids[:, :, None] == want[:, None, :]) & (want[:, None, :] >= 0)).any(dim=1).sum(dim=1).double()
    n = (want >= 0).sum(dim=1).double()
    return float((hit[n > 0] / n[n > 0]).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lsh_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--citation2', action='store_true')
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd._runtime import _ptr, _stream
    from score_restatement import raw_head
    dev = torch.device('cuda:0')
    iters = 2 if a.quick else a.iters
    shapes = [('ogbl-collab size, uniform endpoints', 235_868, 1_179_052, 2, 1024, uniform_edges)]
    if not a.quick:
        shapes.append(('ogbl-collab size, power-law endpoints', 235_868, 1_179_052, 2, 1024, power_law_edges))
    if a.citation2:
        shapes.append(('ogbl-citation2 size, uniform endpoints', 2_927_963, 30_387_995, 3, 64, uniform_edges))
    grid = GRID[1:4] if a.quick else GRID
    lines = [f'LSH index over the MinHash tables against the one-vs-all scan: (P, p) = (128, 8), k = {K}, exclude = the edge list, '
             f'max_bucket = 1024, {torch.cuda.get_device_name(0)}; ms = median of {iters} samples after one warm-up; the byte model of '
             f'ss_lsh_band_keys is roofline.lsh_band_keys_bytes at {ssa.roofline.HBM_PEAK_GBS:.0f} GB/s']
    lib = ssa._native.lib()
    for name, n, e_und, h, S, edges in shapes:
        ei = torch.from_numpy(edges(n, e_und)).to(dev)
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
        table, cards = eh.build_hash_tables(n, ei)
        head = ssa.StructureHead(**raw_head(h * (h + 2), 3))
        src = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
        t_scan = timed(lambda: eh.topk_links(src, table, cards, K, head, exclude=ei), iters)
        want = eh.topk_links(src, table, cards, K, head, exclude=ei)[0]
        lines.append(f'{name}: N = {n}, h = {h}, S = {S}\n  topk_links (the scan)            {t_scan:10.2f} ms')
        print(lines[-1], flush=True)
        for hop, rows, bands in grid:
            if hop > h:
                continue
            t_build = timed(lambda: eh.build_lsh_index(table, hop=hop, rows=rows, bands=bands), iters)
            index = eh.build_lsh_index(table, hop=hop, rows=rows, bands=bands)
            scratch = torch.empty_like(index.keys)
            t_keys = timed(lambda: ssa._native.check(lib.ss_lsh_band_keys(_ptr(index.mh_u32), n, 128, rows, bands, 64, _ptr(scratch), _stream(dev)),
                                                     'ss_lsh_band_keys'), max(iters, 5), warmup=2)
            del scratch
            model = ssa.roofline.lsh_band_keys_bytes(n, 128, rows, bands)
            floor = model / (ssa.roofline.HBM_PEAK_GBS * 1e6)
            rowptr = eh.lsh_candidates(src, index, exclude=ei)[0]
            sizes = torch.diff(rowptr).double()
            t_lsh = timed(lambda: eh.topk_links_lsh(src, table, cards, K, head, index, exclude=ei), iters)
            got = eh.topk_links_lsh(src, table, cards, K, head, index, exclude=ei)[0]
            lines.append(f'  hop {hop}, rows {rows}, bands {bands:3d}: build {t_build:8.2f} ms (ss_lsh_band_keys {t_keys * 1e3:7.1f} us, model {model / 1e6:6.1f} MB = '
                         f'{floor * 1e3:5.1f} us: {floor / t_keys:.0%} of the HBM rate), {index.nbytes / 2 ** 20:7.1f} MiB, '
                         f'{int(index.skipped_buckets.sum())} buckets skipped; candidates per source mean {float(sizes.mean()):9.1f} max '
                         f'{int(sizes.max())}, sources without any {float((sizes == 0).double().mean()):.0%}; topk_links_lsh {t_lsh:8.2f} ms = '
                         f'{t_scan / t_lsh:6.2f} x the scan; recall@{K} {recall(got, want):.3f}')
            print(lines[-1], flush=True)
            del index, got, rowptr
            torch.cuda.empty_cache()
        del table, cards, ei, want
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
