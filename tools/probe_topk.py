#!/usr/bin/env python3
"""probe (one GPU): ElphHashes.topk_candidates (csrc/ss_topk.hip) against the brute-force composition it replaces.

    python tools/probe_topk.py [--shapes collab,ppa,citation2] [--sources 64,1024] [--k 100] [--no-brute] [--quick]

For every shape (uniform graphs of ogbl-collab / ogbl-ppa / ogbl-citation2 node counts; h = 2, h = 3 at citation2; P = 128, p = 8)
and every S it prints
  - pairs/s of the whole call (S * N over the host clock around topk_candidates, which ends in a device synchronisation; median of
    3 after a warm-up call), exclude = the graph's edge list;
  - the scan / exclude / select split (HIP events around the three stages of the same block loop);
  - the brute force: _get_intersections over all S * N pairs in chunks of whole sources + torch.topk per source (S = 64 only);
  - the scan's VALU roofline: the VALU instructions of its inner loop (one staged source against the wavefront's 4 candidates,
    counted in the gfx950 ISA of topk_scan_kernel<2>) at 4 cycles per wave64 instruction on 256 CUs x 4 SIMDs at 2.4 GHz.
--quick: collab only, S = 64, no brute force (for a rocprofv3 run)."""
import argparse
import ctypes
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'collab': (235868, 1200000, 2), 'ppa': (576289, 10500000, 2), 'citation2': (2927963, 15300000, 3)}
VALU_RATE = 256 * 4 * 2.4e9 / 4  # wave64 VALU instructions per second


def scan_loop_valu():
    """VALU instructions of the scan's inner loop at the default shape, from the ISA hipcc makes of csrc/ss_topk.hip"""
    src = os.path.join(ROOT, 'subgraph-sketching_amd', 'csrc', 'ss_topk.hip')
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'include'),
                               '--save-temps', '-c', src, '-o', os.path.join(tmp, 't.o')], cwd=tmp, stderr=subprocess.DEVNULL)
        asm = open(glob.glob(os.path.join(tmp, '*gfx950*.s'))[0]).read()
    name = '_ZN2ss16topk_scan_kernelILi2EEE'
    body = asm[asm.index(name):]
    body = body[:body.index('.Lfunc_end')].split('\n')
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r'^(\.LBB\d+_\d+):', l)] if m}
    best = None
    for i, l in enumerate(body):  # innermost back edge whose body holds the union's dot products
        m = re.search(r's_cbranch_\w+\s+(\.LBB\d+_\d+)', l)
        if m and labels.get(m.group(1), i) < i:
            seg = body[labels[m.group(1)]:i + 1]
            if any('v_dot2c_f32_bf16' in x for x in seg) and (best is None or len(seg) < len(best)):
                best = seg
    return sum(1 for x in best if x.strip().startswith('v_'))


def make(shape, dev):
    import subgraph_sketching_amd as ssa
    N, e_und, h = SHAPES[shape]
    rng = np.random.RandomState(5)
    e = torch.from_numpy(rng.randint(0, N, size=(2, e_und)).astype(np.int64))
    ei = torch.cat([e, e.flip(0)], 1).to(dev)
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    table, _ = eh.build_hash_tables(N, ei)
    torch.cuda.synchronize()
    return eh, table, ei, N, h


def split(eh, table, src, k, hops, ei):
    """ms of scan / exclude / select over the same block loop as topk_candidates"""
    from subgraph_sketching_amd import _native, engine
    from subgraph_sketching_amd._runtime import _ptr, _stream
    from subgraph_sketching_amd.csr import build_csr
    dev = src.device
    mh, hll, N, P = eh._resolve_tables(table, dev)
    params = eh._params(dev)
    csr = build_csr(ei.flip(0), N, dev, check=False)
    S = src.numel()
    blk = max(1, min(S, engine._TOPK_KEY_BYTES // (8 * N)))
    keys = torch.empty((blk, N), dtype=torch.int64, device=dev)
    lib, st = _native.lib(), _stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t = [0.0, 0.0, 0.0]
    k1, k2 = hops
    for b0 in range(0, S, blk):
        nb = min(blk, S - b0)
        sb = ctypes.c_void_p(src.data_ptr() + 8 * b0)
        ev[0].record()
        _native.check(lib.ss_topk_scan(sb, nb, N, _ptr(mh[k1 - 1]), _ptr(hll[k1 - 1]), _ptr(mh[k2 - 1]), _ptr(hll[k2 - 1]), P,
                                       ctypes.byref(params.struct), _ptr(keys), keys.numel() * 8, None, st), 'scan')
        ev[1].record()
        _native.check(lib.ss_topk_exclude(sb, nb, N, _ptr(csr.rowptr), _ptr(csr.col), _ptr(keys), keys.numel() * 8, st), 'exclude')
        ev[2].record()
        engine._decode_topk_keys(torch.topk(keys[:nb], k, dim=1).values)
        ev[3].record()
        torch.cuda.synchronize()
        for j in range(3):
            t[j] += ev[j].elapsed_time(ev[j + 1])
    return t


def brute(eh, table, src, k, hops, N, chunk_pairs=1 << 24):
    """_get_intersections over every (u, v) + self / exclude masking left out (a lower bound) + torch.topk, in chunks of sources"""
    dev = src.device
    per = max(1, chunk_pairs // N)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ar = torch.arange(N, device=dev)
    for s0 in range(0, src.numel(), per):
        u = src[s0:s0 + per]
        links = torch.stack([u.repeat_interleave(N), ar.repeat(u.numel())], 1)
        sc = eh._get_intersections(links, table)[hops].view(u.numel(), N)
        torch.topk(sc, k, dim=1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='collab,ppa,citation2')
    ap.add_argument('--sources', default='64,1024')
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--no-brute', action='store_true')
    ap.add_argument('--quick', action='store_true')
    a = ap.parse_args()
    shapes, sizes = a.shapes.split(','), [int(x) for x in a.sources.split(',')]
    if a.quick:
        shapes, sizes, a.no_brute = ['collab'], [64], True
    dev = torch.device('cuda:0')
    try:
        n_valu = scan_loop_valu()
        ceil = VALU_RATE * 4 / n_valu
        print(f'scan inner loop (topk_scan_kernel<2>): {n_valu} VALU instructions per wave64 iteration = 4 pairs -> VALU ceiling '
              f'{ceil / 1e9:.1f} G pairs/s (4 cycles / instruction, 256 CUs x 4 SIMDs, 2.4 GHz; estimator and key store not counted)')
    except Exception as exc:  # (the ISA count needs hipcc; the timings do not)
        ceil = None
        print(f'scan inner loop: not counted ({exc})')
    for shape in shapes:
        eh, table, ei, N, h = make(shape, dev)
        hops = (h, h)
        for S in sizes:
            src = torch.from_numpy(np.random.RandomState(S).choice(N, S, replace=False)).to(dev)
            eh.topk_candidates(src, table, a.k, hops=hops, exclude=ei)  # warm-up
            torch.cuda.synchronize()
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                eh.topk_candidates(src, table, a.k, hops=hops, exclude=ei)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            call = statistics.median(times)
            sc, ex, se = split(eh, table, src, a.k, hops, ei)
            pairs = S * N
            line = (f'{shape:9s} N={N:8d} h={h} hops={hops} S={S:5d} k={a.k}: call {call * 1e3:9.2f} ms = {pairs / call / 1e9:6.2f} G pairs/s | '
                    f'scan {sc:8.2f} ms ({pairs / sc / 1e6:6.2f} G pairs/s' + (f', {pairs / sc / 1e6 / (ceil / 1e9):.2f} of the VALU ceiling' if ceil else '')
                    + f') exclude {ex:6.2f} ms select {se:8.2f} ms')
            if not a.no_brute and S <= 64:
                bt = brute(eh, table, src, a.k, hops, N)
                line += f' | brute force {bt * 1e3:9.2f} ms = {pairs / bt / 1e9:5.2f} G pairs/s ({bt / call:.1f}x the call)'
            print(line, flush=True)
        del eh, table, ei
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
