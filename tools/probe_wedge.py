#!/usr/bin/env python3
"""probe (one GPU): WedgeGraph.candidates and ElphHashes.topk_links_wedge (csrc/ss_wedge.hip, wedge.py) against the
one-vs-all scan topk_links on the same sources in the same process.

    python tools/probe_wedge.py [--out profiles/wedge_probe.txt] [--quick] [--iters 50] [--warmup 10]

Graphs: ogbl-collab size (N = 235 868, E_und = 1 179 052) and ogbl-citation2 size (N = 2 927 963, E_und = 30 387 995), each with
uniform endpoints and with endpoints drawn with probability proportional to rank^-0.9 (hubs), symmetrised; S = 1 024 and 65 536
sources drawn at random.  Every (graph, endpoints) shape runs in a child process of its own under its own time limit, and the first
child that fails, faults or runs out of time ends the probe: nothing is started after it.  max_walks is the largest cap under which
the byte model (8 bytes per walk written, the sort moves them about 6 times) keeps the sample under 2 TB; a shape whose model passes
that even with the cap is listed with its figure and not run.  Per shape and S:
    W and candidates per source (mean, p99), skipped sources, the share of sources each tier served
    candidates          ms (HIP events, median of --iters after --warmup), and the same with every source through the large tier
                        (_lds_slots = 1) -- the measurement that decides whether the LDS tier stays -- with the spread (p10..p90) of both
    topk_links_wedge    k = 100, ms;  topk_links k = 100 on the same sources, ms (S = 1 024 only: the scan is linear in S);  recall@100
                        of the wedge list against the scan
--quick: collab size, uniform endpoints, S = 1 024, 5 samples after 2 warm-ups."""
import argparse
import os
import statistics
import subprocess
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = {'collab': (235868, 1179052), 'citation2': (2927963, 30387995)}
BYTE_BUDGET = 2e12
WALK_BYTES = 56  # 8 written + about six passes of the sort and the run-length sum over them


def edges(n, e_und, skew, device, seed=1):
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
    """(median, p10, p90) ms of HIP-event spans"""
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
    out.sort()
    return statistics.median(out), out[len(out) // 10], out[-1 - len(out) // 10]


def child(a):
    import subgraph_sketching_amd as ssa
    from score_restatement import raw_head
    dev = torch.device('cuda:0')
    n, e_und = SHAPES[a.shape]
    ends = 'rank^-0.9' if a.skew else 'uniform'
    ei = edges(n, e_und, a.skew, dev)
    g = ssa.WedgeGraph(n, ei)
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    table, cards = eh.build_hash_tables(n, ei)
    head = ssa.StructureHead(**raw_head(8, 1))
    gen = torch.Generator(device=dev).manual_seed(3)
    print(f'## {a.shape} {ends}: N = {n}, E = {ei.size(1)}, max degree {int((g.rowptr[1:] - g.rowptr[:-1]).max())}', flush=True)
    for S in a.sources:
        src = torch.randint(0, n, (S,), generator=gen, device=dev)
        walks = torch.empty((S,), dtype=torch.int64, device=dev)
        ssa.wedge._launch_walks(g, src, walks, None)
        W = np.sort(walks.cpu().numpy())
        fit = W[np.cumsum(W) * WALK_BYTES <= BYTE_BUDGET]
        cap = int(fit[-1]) if fit.size else 0
        kept = W[W <= cap]
        model = float(kept.sum()) * WALK_BYTES
        tag = f'{a.shape} {ends} S={S}'
        print(f'{tag} | W mean {W.mean():.0f} p99 {np.percentile(W, 99):.0f} max {W.max()} | max_walks {cap} | model {model / 1e9:.2f} GB', flush=True)
        if model > BYTE_BUDGET or kept.sum() * 64 > 100e9:  # (the second: what one device holds of a block's arrays at a time is bounded, the sum of the host's work is not)
            print(f'{tag} | not run: {kept.sum():.3g} walks', flush=True)
            continue
        rowptr, ids, common, info = g.candidates(src, max_walks=cap, return_info=True)
        sizes = torch.diff(rowptr).cpu().numpy()
        served = max(1, info['lds_sources'] + info['large_sources'])
        print(f'{tag} | candidates mean {sizes.mean():.0f} p99 {np.percentile(sizes, 99):.0f} | skipped {info["skipped_sources"]} | '
              f'LDS tier {info["lds_sources"] / served:.3f} large tier {info["large_sources"] / served:.3f} of the served', flush=True)
        t_c = timed(lambda: g.candidates(src, max_walks=cap), a.iters, a.warmup)
        t_l = timed(lambda: g.candidates(src, max_walks=cap, _lds_slots=1), a.iters, a.warmup)
        print(f'{tag} | candidates {t_c[0]:.3f} ms ({t_c[1]:.3f}..{t_c[2]:.3f}) | large tier alone {t_l[0]:.3f} ms ({t_l[1]:.3f}..{t_l[2]:.3f}) | '
              f'large / tiered {t_l[0] / t_c[0]:.2f}', flush=True)
        t_w = timed(lambda: eh.topk_links_wedge(src, table, cards, 100, head, g, max_walks=cap), a.iters, a.warmup)
        line = f'{tag} | topk_links_wedge(k=100) {t_w[0]:.3f} ms ({t_w[1]:.3f}..{t_w[2]:.3f})'
        if S <= 1024:
            t_s = timed(lambda: eh.topk_links(src, table, cards, 100, head), max(3, a.iters // 10), 1)
            mine = eh.topk_links_wedge(src, table, cards, 100, head, g, max_walks=cap)[0]
            full = eh.topk_links(src, table, cards, 100, head)[0]
            hit = (mine.unsqueeze(2) == full.unsqueeze(1)).any(dim=1) & (full >= 0)
            line += f' | topk_links(k=100) {t_s[0]:.3f} ms | scan / wedge {t_s[0] / t_w[0]:.1f} | recall@100 {float(hit.sum()) / float((full >= 0).sum()):.4f}'
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wedge_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--limit', type=int, default=900, help='seconds per child')
    ap.add_argument('--shape', choices=sorted(SHAPES))
    ap.add_argument('--skew', type=int, default=0)
    ap.add_argument('--sources', type=int, nargs='+', default=[1024, 65536])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe needs a HIP device'
    if a.shape:
        return child(a)
    iters, warmup = (5, 2) if a.quick else (a.iters, a.warmup)
    lines = [f'# tools/probe_wedge.py on {torch.cuda.get_device_name(0)}; median (p10..p90) of {iters} HIP-event spans after {warmup} warm-ups; h = 2, P = 128, k = 100']
    shapes = [('collab', 0)] if a.quick else [(s, k) for s in ('collab', 'citation2') for k in (0, 1)]
    for shape, skew in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), '--shape', shape, '--skew', str(skew), '--iters', str(iters), '--warmup', str(warmup),
               '--sources'] + [str(s) for s in ([1024] if a.quick else a.sources)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
            text, code = done.stdout, done.returncode
        except subprocess.TimeoutExpired as e:
            text, code = (e.stdout or b'').decode() if isinstance(e.stdout, bytes) else (e.stdout or ''), 124
        print(text, flush=True)
        lines.append(text.rstrip())
        if code != 0:
            lines.append(f'# {shape} skew={skew}: the child ended with status {code}; nothing was started after it')
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0 if code == 0 else 1


if __name__ == '__main__':
    sys.exit(main())
