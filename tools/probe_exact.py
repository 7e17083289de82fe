#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.exact_subgraph_features (csrc/ss_exact.hip) -- rates, tier split, and the sketch error it measures.

    python tools/probe_exact.py [--out profiles/exact_probe.txt] [--quick]

At ogbl-collab size (N = 235 868, E_und = 1 179 052; uniform and power-law endpoints, the generator of tests/test_topk_gpu.py) it
prints, for 65 536 random pairs and 65 536 edge pairs at h = 1, 2, 3:
  - pairs/s of the whole call (host clock around the call, which ends in a device synchronisation; median of 3 after a warm-up);
  - the on-chip tier's and the large tier's time (HIP events around each launch) and the share of pairs that overflowed into the
    large tier;
  - the scipy restatement (tests/exact_restatement.py) on the CPU for a sample of the same pairs, with the thread count stated;
then the sketch error: mean absolute and mean relative error (over pairs whose exact value is non-zero) per feature column of
get_subgraph_features against the exact features, power-law collab graph, 65 536 mixed pairs, h = 2, (P, p) in {64, 128, 256} x
{6, 8, 10}.  --quick: the h = 2 rows only (for a rocprofv3 run)."""
import argparse
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, E_UND = 235_868, 1_179_052
PAIRS = 65536
CPU_SAMPLE = {1: 4096, 2: 1024, 3: 128}


def power_law_graph(n, e_und, seed):
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, size=e_und)
    dst = np.minimum((n * rng.random_sample(e_und) ** 3).astype(np.int64), n - 1)
    e = np.stack([src, dst]).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def uniform_graph(n, e_und, seed):
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def engine(ssa, h, P=128, p=8):
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exact_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd import exact
    import exact_restatement as er
    dev = torch.device('cuda:0')
    lines = []

    def out(s=''):
        print(s, flush=True)
        lines.append(s)

    out(f'# tools/probe_exact.py on {torch.cuda.get_device_name(0)}; N = {N}, E_und = {E_UND}, {PAIRS} pairs per row; '
        f'knobs: EXACT_LDS_MAX_NODES = {ssa.knobs.EXACT_LDS_MAX_NODES}, EXACT_LARGE_SLOTS = {ssa.knobs.EXACT_LARGE_SLOTS}')
    out(f'# CPU restatement: scipy {__import__("scipy").__version__} sparse products, single-threaded '
        f'(torch threads {torch.get_num_threads()} unused); timed on the first {CPU_SAMPLE} pairs of a row, rate extrapolated')
    out(f'{"graph":9s} {"pairs":6s} {"h":>2s} {"call Mpairs/s":>14s} {"call ms":>9s} {"lds ms":>9s} {"large ms":>9s} {"overflow":>9s} '
        f'{"lds Mp/s":>9s} {"large kp/s":>10s} {"cpu kpairs/s":>12s}')
    graphs = {'uniform': uniform_graph(N, E_UND, 3), 'powerlaw': power_law_graph(N, E_UND, 3)}
    for gname, ei in graphs.items():
        ei_dev = torch.from_numpy(ei).to(dev)
        rng = np.random.RandomState(5)
        kinds = {'random': rng.randint(0, N, size=(PAIRS, 2)).astype(np.int64),
                 'edges': ei[:, rng.randint(0, ei.shape[1], size=PAIRS)].T.copy()}
        for kname, links in kinds.items():
            ld = torch.from_numpy(links).to(dev)
            for h in ((2,) if a.quick else (1, 2, 3)):
                eh = engine(ssa, h)
                eh.exact_subgraph_features(ld, N, ei_dev)
                torch.cuda.synchronize()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    eh.exact_subgraph_features(ld, N, ei_dev)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                t = statistics.median(ts)
                st = {}
                exact.exact_subgraph_features(eh, ld, N, ei_dev, stats=st)
                ov = st['overflow']
                lds_rate = (PAIRS - ov) / (st['lds_ms'] * 1e-3) / 1e6
                large_rate = ov / (st['large_ms'] * 1e-3) / 1e3 if ov else float('nan')
                cpu = float('nan')
                if not a.quick:
                    m = CPU_SAMPLE[h]
                    t0 = time.perf_counter()
                    er.restate(N, ei, links[:m], h)
                    cpu = m / (time.perf_counter() - t0) / 1e3
                out(f'{gname:9s} {kname:6s} {h:2d} {PAIRS / t / 1e6:14.3f} {t * 1e3:9.2f} {st["lds_ms"]:9.2f} {st["large_ms"]:9.2f} '
                    f'{ov / PAIRS:9.4f} {lds_rate:9.3f} {large_rate:10.2f} {cpu:12.2f}')
    out('# lds Mp/s = pairs finished on chip / on-chip tier time (the launch also lists the overflowed pairs); large kp/s = '
        f'overflowed pairs / large-tier time ({st.get("slots")} slots)')
    if a.quick:
        return write(a.out, lines)

    out()
    out('# sketch error of get_subgraph_features against exact_subgraph_features: powerlaw collab graph, h = 2, use_zero_one, '
        f'{PAIRS // 2} random + {PAIRS // 2} edge pairs')
    out('# MAE = mean |est - exact| per column; MRE = mean |est - exact| / exact over pairs with exact != 0 (columns: LABEL_LOOKUP[2] '
        'order (1,1) (2,1) (1,2) (2,2) (0,1) (1,0) (0,2) (2,0))')
    ei = graphs['powerlaw']
    ei_dev = torch.from_numpy(ei).to(dev)
    rng = np.random.RandomState(9)
    links = np.concatenate([rng.randint(0, N, size=(PAIRS // 2, 2)), ei[:, rng.randint(0, ei.shape[1], size=PAIRS // 2)].T]).astype(np.int64)
    ld = torch.from_numpy(links).to(dev)
    ex = engine(ssa, 2).exact_subgraph_features(ld, N, ei_dev).cpu().numpy().astype(np.float64)
    nz = ex != 0
    out(f'# exact feature means: ' + ' '.join(f'{x:.1f}' for x in ex.mean(axis=0)))
    for P in (64, 128, 256):
        for p in (6, 8, 10):
            try:
                eh = engine(ssa, 2, P, p)
                table, cards = eh.build_hash_tables(N, ei_dev)
                est = eh.get_subgraph_features(ld, table, cards).cpu().numpy().astype(np.float64)
                err = np.abs(est - ex)
                mae = err.mean(axis=0)
                mre = np.array([(err[nz[:, c], c] / ex[nz[:, c], c]).mean() for c in range(8)])
                out(f'P={P:3d} p={p:2d} MAE ' + ' '.join(f'{x:8.2f}' for x in mae) + ' | MRE ' + ' '.join(f'{x:6.3f}' for x in mre))
                del table, cards
            except Exception as e:  # a sketch shape the engine does not build is reported, not fatal
                out(f'P={P:3d} p={p:2d} not measured: {type(e).__name__}: {e}')
    write(a.out, lines)


def write(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
