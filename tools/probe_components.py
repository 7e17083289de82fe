#!/usr/bin/env python3
"""probe (one GPU): connected_components / largest_component_subgraph (csrc/ss_components.hip, components.py) against
scipy's connected_components on the host copy of the same graph.

    python tools/probe_components.py [--out profiles/components_probe.txt] [--quick] [--iters 5]

Graphs: ogbl-collab size (N = 235 868, E_und = 1 179 052) and ogbl-citation2 size (N = 2 927 963, E_und = 30 387 995), each with uniform
endpoints and with one endpoint drawn with probability proportional to rank^-0.9 (hubs), symmetrised; and a graph of citation2's N with
0.6 N random undirected edges (mean degree 1.2: many mid-sized components next to the largest).  Per graph:
    labels     ss_components_labels alone (init + hook + flatten launches), HIP events, ms and edges per second
    sizes      ss_components_sizes + the cumulative sum + ss_components_roots (one synchronising read inside)
    whole      one largest_component_subgraph call, ms
    scipy      scipy.sparse.csgraph.connected_components(directed=True, connection='weak') on the host copy, wall-clock ms, building the
               csr_matrix listed on its own; the labels are compared with the device's (canonicalised to the component minimum)
    csr        this package's build_csr of the same edge list, ms: the price of "one pass over the edges" that the union-find does not pay
ms = median of --iters samples after one warm-up.  --quick: the uniform collab shape only, 2 samples.  No test runs this."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (('collab', 235868, 1179052, (False, True)), ('citation2', 2927963, 30387995, (False, True)),
          ('dust', 2927963, int(0.6 * 2927963), (False,)))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'components_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=5)
    a = ap.parse_args()
    import scipy.sparse as ssp
    from scipy.sparse.csgraph import connected_components as scipy_components
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd import _native
    from subgraph_sketching_amd._runtime import _ptr, _stream
    from subgraph_sketching_amd.components import _chunks, _cumsum
    assert torch.cuda.is_available(), 'the probe needs a HIP device'
    dev = torch.device('cuda:0')
    lib = _native.lib()
    iters = 2 if a.quick else a.iters
    lines = [f'# tools/probe_components.py on {torch.cuda.get_device_name(0)}; median of {iters} after one warm-up',
             '# graph endpoints | components  largest | labels ms  Medges/s | sizes+roots ms | whole ms | scipy ms (+ csr_matrix ms)  equal | build_csr ms']

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for name, n, e_und, skews in (SHAPES[:1] if a.quick else SHAPES):
        for skew in (skews[:1] if a.quick else skews):
            ei = edges(n, e_und, skew, dev)
            E = ei.size(1)
            parent = torch.empty((n,), dtype=torch.int32, device=dev)
            label = torch.empty((n,), dtype=torch.int32, device=dev)
            size = torch.empty((n,), dtype=torch.int32, device=dev)
            counts = torch.empty((_chunks(n),), dtype=torch.int32, device=dev)

            def labels():
                _native.check(lib.ss_components_labels(_ptr(ei[0]), _ptr(ei[1]), E, n, _ptr(parent), _ptr(label), None, _stream(dev)), 'labels')

            def sizes():
                _native.check(lib.ss_components_sizes(_ptr(label), n, _ptr(size), _ptr(counts), _stream(dev)), 'sizes')
                incl, C = _cumsum(counts)
                roots = torch.empty((C,), dtype=torch.int64, device=dev)
                out = torch.empty((C,), dtype=torch.int64, device=dev)
                best = torch.zeros((1,), dtype=torch.int64, device=dev)
                _native.check(lib.ss_components_roots(_ptr(label), _ptr(size), n, _ptr(incl), _ptr(roots), _ptr(out), _ptr(best), _stream(dev)), 'roots')

            t_labels = timed(labels, iters)
            t_sizes = timed(sizes, iters)
            t_whole = timed(lambda: ssa.largest_component_subgraph(n, ei), iters)
            t_csr = timed(lambda: ssa.build_csr(ei, n, dev, check=False), iters)
            cc = ssa.connected_components(n, ei)
            host = ei.cpu().numpy()
            t0 = time.perf_counter()
            A = ssp.csr_matrix((np.ones(E, dtype=np.int8), (host[0], host[1])), shape=(n, n))
            t1 = time.perf_counter()
            C, lab = scipy_components(A, directed=True, connection='weak')
            t2 = time.perf_counter()
            smallest = np.full(C, n, dtype=np.int64)
            np.minimum.at(smallest, lab, np.arange(n, dtype=np.int64))
            equal = bool(np.array_equal(smallest[lab], cc.labels.cpu().numpy())) and C == cc.num_components
            say(f'{name} {"rank^-0.9" if skew else "uniform"}: N = {n}, E = {E} | {cc.num_components}  {int(cc.sizes.max())} | {t_labels:.3f}  '
                f'{E / t_labels / 1e3:.1f} | {t_sizes:.3f} | {t_whole:.3f} | {(t2 - t1) * 1e3:.1f} (+ {(t1 - t0) * 1e3:.1f})  {equal} | {t_csr:.3f}')
            del ei, cc, A, host
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
