#!/usr/bin/env python3
"""probe (one GPU): NegativeSampler.sample (csrc/ss_negatives.hip, negatives.py) against the same job composed of torch
calls in the same process.

    python tools/probe_negatives.py [--out profiles/negatives_probe.txt] [--quick] [--iters 5]

Graphs: ogbl-collab size (N = 235 868, E_und = 1 179 052) and ogbl-citation2 size (N = 2 927 963, E_und = 30 387 995), each with
uniform endpoints and with endpoints drawn with probability proportional to rank^-0.9 (hubs), symmetrised.  Positives: edges of the
graph drawn at random, one negative each, 1 M and 16 M slots; max_tries = 16.  Per graph, mode and slot count:
    kernel        one .sample call (HIP events around it), ms and slots per second, the share of unsampled slots
    torch         the PyG method on the same GPU: torch.randint proposals, rejection by torch.searchsorted on the sorted keys
                  u * N + v of the edge list, the rejected slots drawn again, up to max_tries rounds (uniform / same_source are the same
                  job here: fixed sources); for wedge the two neighbour picks are gathers from the sampler's own CSR.  Its draws are
                  torch's, so the rows differ from the kernel's: only the job is the same.  ms, slots per second, unsampled share
The sampler (CSR build + row sort) and the sorted keys are built once per graph, outside the timed region, and their times are listed.
ms = median of --iters samples after one warm-up.  --quick: the uniform collab shape only, 1 M slots, 2 samples."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_TRIES = 16
SHAPES = (('collab', 235868, 1179052), ('citation2', 2927963, 30387995))


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


def torch_composition(mode, N, rowptr, col, keys, sources, gen, max_tries=MAX_TRIES):
    """(int64 [L, 2] with -1 for unsampled, as .sample returns it) by rounds of proposals over the slots still open"""
    L = sources.numel()
    v_out = torch.full((L,), -1, dtype=torch.int64, device=sources.device)
    todo = torch.arange(L, device=sources.device)
    for _ in range(max_tries):
        if todo.numel() == 0:
            break
        u = sources[todo]
        if mode == 'wedge':
            b, d = rowptr[u], rowptr[u + 1] - rowptr[u]
            has = d > 0
            todo, u, b, d = todo[has], u[has], b[has], d[has]  # (a source without neighbours stays unsampled)
            w = col[b + (torch.rand(u.shape, generator=gen, device=u.device, dtype=torch.float64) * d).long().clamp_(max=d - 1)].long()
            bw, dw = rowptr[w], rowptr[w + 1] - rowptr[w]
            pick = bw + (torch.rand(u.shape, generator=gen, device=u.device, dtype=torch.float64) * dw).long().clamp_(max=dw - 1)
            v = col[pick.clamp_(max=col.numel() - 1)].long()
            v = torch.where(dw > 0, v, u)  # (no out-neighbour: rejected below)
        else:
            v = torch.randint(0, N, u.shape, generator=gen, device=u.device)
        k = u * N + v
        hit = keys[torch.searchsorted(keys, k).clamp_(max=keys.numel() - 1)] == k
        ok = ~hit & (v != u)
        v_out[todo[ok]] = v[ok]
        todo = todo[~ok]
    return torch.stack([sources, v_out], dim=1)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'negatives_probe.txt'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--iters', type=int, default=5)
    a = ap.parse_args()
    import subgraph_sketching_amd as ssa
    assert torch.cuda.is_available(), 'the probe needs a HIP device'
    dev = torch.device('cuda:0')
    iters = 2 if a.quick else a.iters
    lines = [f'# tools/probe_negatives.py on {torch.cuda.get_device_name(0)}; max_tries = {MAX_TRIES}, one negative per positive, '
             f'median of {iters} after one warm-up',
             '# graph endpoints mode slots | kernel ms  Mslots/s  unsampled | torch ms  Mslots/s  unsampled | torch / kernel']

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for name, n, e_und in (SHAPES[:1] if a.quick else SHAPES):
        for skew in ((False,) if a.quick else (False, True)):
            ei = edges(n, e_und, skew, dev)
            torch.cuda.synchronize()
            t_build = timed(lambda: ssa.NegativeSampler(n, ei), 1, warmup=0)
            sampler = ssa.NegativeSampler(n, ei)
            t_keys = timed(lambda: torch.sort(ei[0] * n + ei[1]), 1, warmup=0)
            keys = torch.sort(ei[0] * n + ei[1]).values
            rowptr, col = sampler.graph.rowptr, sampler.graph.col
            deg = rowptr[1:] - rowptr[:-1]
            say(f'## {name} {"rank^-0.9" if skew else "uniform"}: N = {n}, E = {ei.size(1)}, max degree {int(deg.max())}; sampler (CSR + row sort) '
                f'{t_build:.2f} ms, sorted keys for torch {t_keys:.2f} ms')
            gen = torch.Generator(device=dev).manual_seed(3)
            for slots in ((1 << 20,) if a.quick else (1 << 20, 1 << 24)):
                pos = ei.t()[torch.randint(0, ei.size(1), (slots,), generator=gen, device=dev)].contiguous()
                for mode in ('uniform', 'same_source', 'wedge'):
                    seed = [0]

                    def kernel():
                        seed[0] += 1
                        return sampler.sample(pos, mode=mode, seed=seed[0], max_tries=MAX_TRIES)

                    t_k = timed(kernel, iters)
                    un_k = sampler.sample(pos, mode=mode, seed=1, max_tries=MAX_TRIES, return_info=True)[1]['unsampled'] / slots
                    t_t = timed(lambda: torch_composition(mode, n, rowptr, col, keys, pos[:, 0], gen), iters)
                    un_t = float((torch_composition(mode, n, rowptr, col, keys, pos[:, 0], gen)[:, 1] < 0).double().mean())
                    say(f'{name} {"rank^-0.9" if skew else "uniform"} {mode} {slots} | {t_k:.3f}  {slots / t_k / 1e3:.1f}  {un_k:.5f} | '
                        f'{t_t:.3f}  {slots / t_t / 1e3:.1f}  {un_t:.5f} | {t_t / t_k:.2f}')
                del pos
            del sampler, keys, ei
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
