#!/usr/bin/env python3
"""probe (one GPU): coalesce / to_undirected (csrc/ss_coalesce.hip, graph_prep.py) against the torch composition that
would stand in for them -- torch.unique(row * n + col, return_inverse=True) + scatter_add_ -- on the same GPU.

    python tools/probe_graph_prep.py [--out profiles/graph_prep_probe.txt] [--quick] [--iters 5]

Lists: ogbl-collab size (N = 235 868, E = 2 358 104 directed entries) and ogbl-citation2 size (N = 2 927 963, E = 30 387 995), each with
uniform endpoints and with one endpoint drawn with probability proportional to rank^-0.9 (hubs: long runs), with unit and with fractional
float32 weights.  Per list and call (coalesce of the list; to_undirected of it, 2 E entries):
    ours       one graph_prep call, HIP events around it (its one host read inside), ms
    groupings  the two stable groupings alone (sign.group_ids_stable by col, then by row): their share of `ours`
    merge      ours - groupings: ss_coalesce_mark + cumsum + the host read + ss_coalesce_fill + ss_coalesce_reduce + ss_coalesce_reduce_long
               and the allocations, ms
    torch      unique + scatter_add_ (float atomics: not repeatable for fractional weights; n^2 < 2^63 at these sizes), ms
    equal      pairs equal, and the values bit-equal (unit weights) / within 1e-4 relative (fractional: the composition's order is free)
ms = median of --iters samples after one warm-up.  --quick: the uniform collab list only, 2 samples.  No speed is gated by any test;
where this loses, the output says by how much.  No test runs this."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (('collab', 235868, 2358104), ('citation2', 2927963, 30387995))


def edge_list(n, e, skew, device, seed=1):
    """int64 [2, e]: endpoints uniform, or (skew) the second endpoint with probability proportional to rank^-0.9"""
    gen = torch.Generator(device=device).manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=gen, device=device)
    if skew:
        cdf = torch.cumsum(torch.arange(1, n + 1, dtype=torch.float64, device=device) ** -0.9, 0)
        r = torch.rand((e,), generator=gen, device=device, dtype=torch.float64) * cdf[-1]
        dst = torch.searchsorted(cdf, r).clamp_(max=n - 1)
    else:
        dst = torch.randint(0, n, (e,), generator=gen, device=device)
    return torch.stack([src, dst])


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


def torch_coalesce(ei, w, n):
    key = ei[0] * n + ei[1]
    uniq, inverse = torch.unique(key, return_inverse=True)
    out = torch.zeros(uniq.numel(), dtype=w.dtype, device=w.device).scatter_add_(0, inverse, w)
    return torch.stack([uniq // n, uniq % n]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'graph_prep_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=5)
    a = ap.parse_args()
    from subgraph_sketching_amd import graph_prep as gp
    assert torch.cuda.is_available(), 'the probe needs a HIP device'
    dev = torch.device('cuda:0')
    iters = 2 if a.quick else a.iters
    lines = [f'# tools/probe_graph_prep.py on {torch.cuda.get_device_name(0)}; median of {iters} after one warm-up',
             '# list endpoints weights call | entries -> pairs  longest run | ours ms | groupings ms (share) | merge ms | torch unique+scatter_add ms | '
             'ours / torch | equal']

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for name, n, e in (SHAPES[:1] if a.quick else SHAPES):
        for skew in ((False,) if a.quick else (False, True)):
            base = edge_list(n, e, skew, dev)
            gen = torch.Generator(device=dev).manual_seed(3)
            for weights in ('unit', 'fractional'):
                w0 = torch.ones(e, device=dev) if weights == 'unit' else torch.rand(e, generator=gen, device=dev) + 0.01
                for call in ('coalesce', 'to_undirected'):
                    doubled = call == 'to_undirected'
                    ei = torch.cat([base, base.flip(0)], dim=1) if doubled else base
                    w = torch.cat([w0, w0]) if doubled else w0
                    E = ei.size(1)
                    ours = (lambda: gp.to_undirected(base, w0, n)) if doubled else (lambda: gp.coalesce(base, w0, n, n))
                    err = torch.zeros(1, dtype=torch.int32, device=dev)
                    t_ours = timed(ours, iters)
                    t_group = timed(lambda: gp.sorted_positions(ei[0], ei[1], n, err), iters)
                    merged = gp._merge(n, ei, w, gp.OPS['add'], 256, dev)
                    t_merge = t_ours - t_group  # (the launches after the groupings, the host read and the output allocations)
                    t_torch = timed(lambda: torch_coalesce(ei, w, n), iters)
                    index, value = ours()
                    ref_index, ref_value = torch_coalesce(ei, w, n)
                    equal = bool(torch.equal(index, ref_index)) and (bool(torch.equal(value, ref_value)) if weights == 'unit' else
                                                                     bool(torch.allclose(value, ref_value, rtol=1e-4, atol=0)))
                    say(f'{name} {"rank^-0.9" if skew else "uniform"} {weights} {call} | {E} -> {index.size(1)}  {int(merged.count.max())} | '
                        f'{t_ours:.3f} | {t_group:.3f} ({100 * t_group / t_ours:.0f}%) | {t_merge:.3f} | {t_torch:.3f} | {t_ours / t_torch:.2f} | {equal}')
                    del ei, w, merged, index, value, ref_index, ref_value
            del base
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
