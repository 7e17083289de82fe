"""probe: link_decoder.link_gather / link_hadamard on the bench's graph size (collab, N = 235 868) -> profiles/link_decoder_probe.txt

For batches of L = 2 048, 65 536 and 1 048 576 links with uniform endpoints and with rank^-0.9 ones (the first L edges of
bench.synthetic_graph(kind='powerlaw', alpha=0.9): endpoint 0 by weight, endpoint 1 uniform -- the positives of a hub-heavy graph),
F = 128, 256, 1024: the plan build, forward, backward and forward + backward of both functions against `x[links]` (gathered ONCE;
for the product, its halves multiplied: what the reference's loop and predictor do) under torch autograd in the same process, and
against the byte model (roofline.link_decoder_bytes).  On the rank^-0.9 batches a sweep of hub_entries (256 ... 8192, 10^9 = no hub
tier).  Nothing is gated: the file is a measurement to quote.  It decides link_decoder.DEFAULT_HUB_ENTRIES."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import subgraph_sketching_amd as ssa
from subgraph_sketching_amd import link_decoder, roofline

dev = torch.device('cuda:0')
n = bench.N_NODES
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, window=0.05):
    """ms per call: after a warm-up, one call is timed to size the run, then as many calls as fill `window` seconds (at least 5, at
    most 2000), a host clock around them, ending in a device synchronise"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = int(min(2000, max(5, window / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def torch_hadamard(t, links):
    """the reference's composition: ONE gather (runners/train.py:200), then the product of its halves (models/elph.py:54)"""
    y = t[links]
    return y[:, 0, :] * y[:, 1, :]


def fwd_bwd(f, x, g):
    x.grad = None
    f(x).backward(g)


def bwd_alone(f, x, g):
    """ms per backward of one kept forward (timed on its own, not as a difference of two means)"""
    y = f(x)

    def run():
        x.grad = None
        y.backward(g, retain_graph=True)

    return timed(run)


def pct(model, ms):
    return 100 * model / ms / 1e6 / roofline.HBM_PEAK_GBS


def batch(kind, L):
    if kind == 'uniform':
        return bench.synthetic_links(n, L, seed=3)
    return np.ascontiguousarray(bench.synthetic_graph(n, L, 'powerlaw', 0.9, seed=3)[:, :L].T)


say(f'default in this run: hub_entries = {link_decoder.DEFAULT_HUB_ENTRIES}; N = {n}; times in ms per call, the mean over a 50 ms window (5 to 2000 calls) after a warm-up')
for kind in ('uniform', 'rank^-0.9'):
    for L in (2048, 65536, 1048576):
        links_np = batch(kind, L)
        m = np.bincount(links_np.reshape(-1), minlength=n)
        links = torch.from_numpy(links_np).to(dev)
        t_plan = timed(lambda: ssa.LinkBatch(n, links))
        plan = ssa.LinkBatch(n, links)
        say(f'batch {kind}, L = {L}: {plan.num_touched} touched nodes, most slots on one node {m.max()}; plan build (one stable grouping, node and hub '
            f'lists, one host read) {t_plan:.3f} ms; at hub_entries = {plan.hub_entries}: {plan.n_hubs} hub rows in {plan.n_chunks} chunks')
        for F in (128, 256, 1024):
            x = torch.randn(n, F, device=dev, requires_grad=True)
            for name, ours, theirs, shape, product in (('gather', ssa.link_gather, lambda t: t[links], (L, 2, F), False),
                                                      ('hadamard', ssa.link_hadamard, lambda t: torch_hadamard(t, links), (L, F), True)):
                g = torch.randn(shape, device=dev)
                b_f = roofline.link_decoder_bytes(n, L, F, product=product)['total']
                b_b = roofline.link_decoder_bytes(n, L, F, product=product, backward=True, M=plan.num_touched, hub_chunks=plan.n_chunks)['total']
                with torch.no_grad():
                    t_f = timed(lambda: ours(x, plan))
                    t_tf = timed(lambda: theirs(x))
                t_fb = timed(lambda: fwd_bwd(lambda t: ours(t, plan), x, g))
                t_tfb = timed(lambda: fwd_bwd(theirs, x, g))
                t_b, t_tb = bwd_alone(lambda t: ours(t, plan), x, g), bwd_alone(theirs, x, g)
                t_own = timed(lambda: fwd_bwd(lambda t: ours(t, links), x, g))  # the plan built inside the forward
                say(f'  F = {F:>4} {name:<8}: forward {t_f:.3f} (torch {t_tf:.3f}) = {pct(b_f, t_f):.1f} % of the HBM peak by the byte model ({b_f:,} B); '
                    f'forward + backward {t_fb:.3f} (torch {t_tfb:.3f}), backward alone {t_b:.3f} (torch {t_tb:.3f}) = {pct(b_b, t_b):.1f} % ({b_b:,} B); '
                    f'forward + backward with the plan built in the forward {t_own:.3f}')
                if kind != 'uniform' and name == 'hadamard':
                    parts = []
                    for hub in (256, 512, 1024, 2048, 8192, 10 ** 9):
                        p = ssa.LinkBatch(n, links, hub_entries=hub)
                        t = timed(lambda: fwd_bwd(lambda t: ours(t, p), x, g))
                        parts.append(f'{hub}: {p.n_hubs} hubs / {p.n_chunks} chunks, {t:.3f}')
                        del p
                    say(f'  F = {F:>4} hadamard, forward + backward, hub_entries sweep -- ' + '; '.join(parts))
                del g
            del x
        del plan

text = '\n'.join(lines) + '\n'
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'link_decoder_probe.txt')
with open(path, 'w') as f:
    f.write(text)
