#!/usr/bin/env python3
"""probe (one GPU): batched personalised PageRank (heuristics.PPR, csrc/ss_ppr.hip) on ogbl-collab-size synthetic graphs.

    python tools/probe_ppr.py [--sources 10000] [--sweep 16,32,64,128] [--graphs uniform,powerlaw] [--quick]

For every graph (N = 235 868, ~2.4 M stored entries; `uniform`: uniform endpoints, `powerlaw`: in-degrees skewed to hubs of
tens of thousands of in-edges) it prints
  - ms per iteration (HIP events around ss_ppr_iterate: the step kernel + the hub kernel + the per-column finalize; tol = 0 so
    every column stays active) for each S of the sweep, with the modelled bytes of one step
    nnz * (4 + 8) + nnz * S * 8 + 2 * N * S * 8 (CSR entries, one S-column row gathered per entry, the own row read and written)
    and their rate as a fraction of 8 TB/s;
  - end-to-end seconds of PPR(A, links) for `--sources` links with distinct sources (host clock around the call, which ends in a
    device synchronisation), at the default S;
  - the seconds per source of the scipy restatement of the reference's loop (tests/ppr_restatement.py), timed on 3 sources and
    extrapolated to `--sources` (labelled as such).
--quick: one S, 500 sources, no scipy timing (for a rocprofv3 run).  --steps-only: only the per-iteration timing at the
default S (for a rocprofv3 --pmc run: every step kernel it counts has all S columns active)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_COLLAB, E_COLLAB = 235868, 2400000
PEAK_BYTES_PER_S = 8e12


def make_graph(kind, seed=11):
    rng = np.random.RandomState(seed)
    src = rng.randint(0, N_COLLAB, size=E_COLLAB)
    if kind == 'uniform':
        dst = rng.randint(0, N_COLLAB, size=E_COLLAB)
    else:
        dst = np.minimum((N_COLLAB * rng.random_sample(E_COLLAB) ** 3).astype(np.int64), N_COLLAB - 1)
    return sp.csr_matrix((np.ones(E_COLLAB, dtype=np.int64), (src, dst)), shape=(N_COLLAB, N_COLLAB))


def time_iterations(op, S, iters=40, skip=5):
    """ms per iteration with every column active (tol = 0)"""
    from subgraph_sketching_amd import _native
    from subgraph_sketching_amd._runtime import _error_flag, _ptr, _stream
    lib = _native.lib()
    dev = op.device
    nbytes = op.workspace_bytes(S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sources = torch.from_numpy(np.random.RandomState(S).choice(op.num_nodes, S, replace=False)).to(dev)
    g, stream = ctypes.byref(op.struct), _stream(dev)
    _native.check(lib.ss_ppr_begin(g, _ptr(sources), S, 0.0, _ptr(ws), nbytes, _ptr(_error_flag(dev)), stream), 'ss_ppr_begin')
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(1, iters + 1):
        if k == skip + 1:
            start.record()
        _native.check(lib.ss_ppr_iterate(g, S, k, iters + 1, 0.0, _ptr(ws), nbytes, stream), 'ss_ppr_iterate')
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / (iters - skip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sources', type=int, default=10000)
    ap.add_argument('--sweep', default='16,32,64,128')
    ap.add_argument('--graphs', default='uniform,powerlaw')
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--steps-only', action='store_true')
    args = ap.parse_args()
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd.heuristics import PPR, DeviceAdjacency
    from ppr_restatement import pagerank_power
    assert torch.cuda.is_available(), 'probe_ppr needs a HIP device'
    dev = torch.device('cuda:0')
    sweep = [int(s) for s in args.sweep.split(',')]
    n_sources = args.sources
    if args.quick or args.steps_only:
        sweep, n_sources = [ssa.knobs.PPR_COLUMNS], 500
    print(f'# {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; argv {" ".join(sys.argv[1:])}', flush=True)
    for kind in args.graphs.split(','):
        A = make_graph(kind)
        adj = DeviceAdjacency(A, dev)
        op = adj.ppr_operator(0.85)
        indeg = np.diff(op.rowptr.cpu().numpy())
        print(json.dumps({'graph': kind, 'N': op.num_nodes, 'nnz': op.nnz, 'max_in_degree': int(indeg.max()),
                          'hub_rows': op.n_hubs, 'hub_segments': op.n_segments}), flush=True)
        for S in sweep:
            ms = time_iterations(op, S)
            model = op.nnz * (4 + 8) + op.nnz * S * 8 + 2 * op.num_nodes * S * 8
            print(json.dumps({'graph': kind, 'S': S, 'ms_per_iteration': round(ms, 4), 'modelled_bytes': model,
                              'TB_per_s': round(model / ms / 1e9, 3), 'fraction_of_8TBps': round(model / ms / 1e9 / 8, 3)}),
                  flush=True)
        if args.steps_only:
            continue
        rng = np.random.RandomState(5)
        links = torch.from_numpy(np.stack([rng.choice(op.num_nodes, n_sources, replace=False),
                                           rng.randint(0, op.num_nodes, n_sources)], 1))
        PPR(adj, links[:64])  # warm-up: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores, _ = PPR(adj, links)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        print(json.dumps({'graph': kind, 'distinct_sources': n_sources, 'S': op.columns(n_sources), 'end_to_end_s': round(sec, 3),
                          'ms_per_source': round(1e3 * sec / n_sources, 4)}), flush=True)
        if not args.quick:
            few = [int(s) for s in links[:3, 0]]
            t0 = time.perf_counter()
            for s in few:
                pagerank_power(A, [s], p=0.85, tol=1e-7)
            per = (time.perf_counter() - t0) / len(few)
            print(json.dumps({'graph': kind, 'scipy_restatement_s_per_source': round(per, 3), 'timed_sources': len(few),
                              f'extrapolated_s_for_{n_sources}_sources': round(per * n_sources, 1)}), flush=True)


if __name__ == '__main__':
    main()
