#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.update_hash_tables (csrc/ss_update.hip) against a full build_hash_tables in the same process.

    python tools/probe_update.py [--out profiles/update_probe.txt] [--quick] [--iters 50]

At ogbl-collab size (N = 235 868, E_und = 1 179 052, h = 2) and ogbl-citation2 size (N = 2 927 963, E_und = 30 387 995, h = 3), with
uniform endpoints and with endpoint weights ~ rank^-0.9 (the generator of bench.py), for 2, 2 048 and 60 000 changed undirected edges
(half removed, half added) it prints per line: |dirty_k| / N per hop, the update (HIP events around the call: CSR build of the new
graph + marking + row hops, no host read inside), the full rebuild (HIP events around build_hash_tables: its CSR build + every hop),
and the CSR build alone, which both sides pay.  10 warm-ups, median of --iters (>= 50) samples; every update sample applies the
change or takes it back (remove-then-re-add: the same targets, so the same seeds), so the tables never drift.  Tables are compared
with the rebuild once per line before timing.  --quick: collab size only, 12 samples (for a rocprofv3 kernel trace)."""
import argparse
import os
import statistics
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'collab': (235_868, 1_179_052, 2), 'citation2': (2_927_963, 30_387_995, 3)}
CHANGES = (2, 2048, 60000)


def graph(n, e_und, kind, seed=1):
    rng = np.random.RandomState(seed)
    if kind == 'uniform':
        e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    else:  # endpoint weights ~ rank^-0.9
        w = np.arange(1, n + 1, dtype=np.float64) ** -0.9
        cdf = np.cumsum(w / w.sum())
        e = np.minimum(np.stack([np.searchsorted(cdf, rng.random_sample(e_und)), rng.randint(0, n, size=e_und)]).astype(np.int64), n - 1)
    return np.concatenate([e, e[::-1]], axis=1)


def change(n, ei, count, kind, seed=3):
    """count undirected edges: half removed, half added (endpoints drawn like the graph's) -> (new edge_index, added, removed)"""
    rng = np.random.RandomState(seed)
    half = ei.shape[1] // 2
    pos = rng.choice(half, size=count // 2, replace=False)
    keep = np.ones(ei.shape[1], dtype=bool)
    keep[pos] = False
    keep[pos + half] = False
    removed = np.concatenate([ei[:, pos], ei[:, pos + half]], axis=1)
    add = graph(n, count - count // 2, kind, seed + 1)
    return np.concatenate([ei[:, keep], add], axis=1), add, removed


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'update_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    dev = torch.device('cuda:0')
    iters, warmup = (12, 3) if a.quick else (max(a.iters, 50), 10)
    lines = [f'update_hash_tables vs build_hash_tables, (P, p) = (128, 8), {torch.cuda.get_device_name(0)}; ms = median (min .. max) of {iters}']
    for shape in (('collab',) if a.quick else ('collab', 'citation2')):
        n, e_und, h = SHAPES[shape]
        for kind in ('uniform', 'rank^-0.9'):
            ei = graph(n, e_und, kind)
            old = torch.from_numpy(ei).to(dev)
            eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
            eh.strict_bounds = False
            csr_ms = timed(lambda: ssa.build_csr(old, n, dev, check=False), warmup, iters)
            build_ms = timed(lambda: eh.build_hash_tables(n, old), warmup, iters)
            lines.append(f'{shape} {kind}: N = {n}, E_und = {e_und}, h = {h}; rebuild {build_ms[0]:.3f} ms ({build_ms[1]:.3f} .. {build_ms[2]:.3f}), '
                         f'CSR build alone {csr_ms[0]:.3f} ms')
            for count in CHANGES:
                new_np, add_np, rem_np = change(n, ei, count, kind)
                new, add, rem = (torch.from_numpy(x).to(dev) for x in (new_np, add_np, rem_np))
                table, cards = eh.build_hash_tables(n, old)
                _, _, info = eh.update_hash_tables(table, cards, n, new, added=add, removed=rem, return_info=True)
                ref, ref_cards = eh.build_hash_tables(n, new)
                same = all(torch.equal(table[k].mh_u32, ref[k].mh_u32) and torch.equal(table[k].hll_u8, ref[k].hll_u8) for k in range(1, h + 1))
                cards_same = bool(torch.equal(cards.view(torch.int32), ref_cards.view(torch.int32)))
                del ref, ref_cards
                state = [True]  # the tables currently describe the NEW graph

                def step():
                    if state[0]:
                        eh.update_hash_tables(table, cards, n, old, added=rem, removed=add)
                    else:
                        eh.update_hash_tables(table, cards, n, new, added=add, removed=rem)
                    state[0] = not state[0]
                upd_ms = timed(step, warmup, iters)
                share = ' '.join(f'|dirty_{k}|/N = {info["dirty_rows"][k] / n:.4f}' for k in range(1, h + 1))
                lines.append(f'  {count:>6} changed edges: {share} (hub rows listed {sum(info["hub_list"].values())}); update {upd_ms[0]:.3f} ms '
                             f'({upd_ms[1]:.3f} .. {upd_ms[2]:.3f}) = {upd_ms[0] / build_ms[0]:.2f} x rebuild; tables equal to rebuild: {same}, '
                             f'cards bit-identical: {cards_same}')
                print(lines[-1], flush=True)
                del table, cards
            del old
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
