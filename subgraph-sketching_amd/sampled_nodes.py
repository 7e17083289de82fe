"""Per-hop sampled subgraph node lists (ElphHashes.sampled_subgraph_nodes, csrc/ss_sampled_nodes.hip): per link (u, v) the node row of
the reference's k_hop_subgraph with its sample_ratio / max_nodes_per_hop (src/datasets/seal.py:291-348), deterministic in a seed -- one
joint walk from {u, v} that keeps a uniform sample of every hop's fringe and expands only what it kept.  Design: DESIGN 3.19; Python-set
restatement: tests/sampled_subgraph_restatement.py.

Host side only, as exact_nodes.py: argument checks, the CSR (the engine's cache), the slot arena (exact._arena) and the two walks over
the batches: a count pass, ONE host read of the total for the allocation, a fill pass."""
import numbers
from ctypes import byref

import torch

from . import _native, exact, exact_nodes, knobs
from ._runtime import _compute_device, _ptr, _stream, _Span


def sampling_arguments(max_nodes_per_hop, ratio_per_hop, seed):
    """-> (cap for the C ABI: 0 = none, ratio as float, seed as int) after the checks"""
    if max_nodes_per_hop is not None:
        if isinstance(max_nodes_per_hop, bool) or not isinstance(max_nodes_per_hop, numbers.Integral) or max_nodes_per_hop < 1:
            raise ValueError(f'max_nodes_per_hop must be None or an integer >= 1, got {max_nodes_per_hop!r}')
        if max_nodes_per_hop >= (1 << 31):
            max_nodes_per_hop = (1 << 31) - 1  # (no fringe holds 2^31 nodes: the same as no cap)
    if isinstance(ratio_per_hop, bool) or not isinstance(ratio_per_hop, numbers.Real) or not 0.0 < float(ratio_per_hop) <= 1.0:
        raise ValueError(f'ratio_per_hop must be a real number in (0, 1], got {ratio_per_hop!r}')
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < (1 << 63):
        raise ValueError(f'seed must be an integer in [0, 2^63), got {seed!r}')
    return int(max_nodes_per_hop or 0), float(ratio_per_hop), int(seed)


def sampled_subgraph_nodes(eh, links, num_nodes, edge_index, batch_size=11000000, max_nodes_per_hop=None, ratio_per_hop=1.0, seed=0,
                           max_nodes=None, return_info=False, stats=None):
    """see ElphHashes.sampled_subgraph_nodes.  stats (measurement hook, tools/probe_sampled_subgraphs.py): a dict that receives the
    milliseconds of the count pass, of the row pointer with its host read and allocation, and of the fill pass (the call then synchronises)"""
    h = eh.max_hops
    cap_hop, ratio, seed = sampling_arguments(max_nodes_per_hop, ratio_per_hop, seed)
    cap = exact_nodes._cap(max_nodes)
    lk, ei, N, batch_size = exact.check_arguments(h, links, num_nodes, edge_index, batch_size)
    home, L = lk.device, lk.size(0)
    if L == 0:
        out = (torch.zeros((1,), dtype=torch.int64, device=home), torch.empty((0,), dtype=torch.int64, device=home),
               torch.empty((0,), dtype=torch.uint8, device=home))
        info = {'truncated': torch.empty((0,), dtype=torch.int64, device=home), 'lds_links': 0, 'large_links': 0, 'sampled_links': 0}
        return out + (info,) if return_info else out
    device = _compute_device(lk, ei)
    csr = eh._csr_cache.get(ei, N, device)  # (the engine's CSR cache: a repeated edge_index is not rebuilt)
    graph = _native.CsrGraphStruct(rowptr=csr.rowptr.data_ptr(), col=csr.col.data_ptr(), num_nodes=N, n_self_loops=0,
                                   n_self_loops_dev=csr.n_self_dev.data_ptr())
    lk = lk.to(device=device, dtype=torch.int64).contiguous()
    lib = _native.lib()
    starts = list(range(0, L, batch_size))
    # every batch keeps its own workspace (4 counter words, then its overflow list) from the count pass to the fill pass
    ws = torch.empty((4 * len(starts) + L,), dtype=torch.int32, device=device)
    counts = torch.empty((L,), dtype=torch.int32, device=device)
    state = torch.empty((L,), dtype=torch.int32, device=device)
    slots, arena = exact._arena(device, N)
    stream = _stream(device)
    lds_nodes = max(0, int(knobs.EXACT_LDS_MAX_NODES))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if stats is not None else None

    def walk(rowptr, ids, hop):
        for i, s0 in enumerate(starts):
            nb = min(batch_size, L - s0)
            args = (byref(graph), exact._at(lk, 2 * s0), nb, N, h, cap_hop, ratio, seed)
            outs = (exact._at(counts, s0), exact._at(state, s0), exact._at(rowptr, s0), _ptr(ids) if ids is not None else None,
                    _ptr(hop) if hop is not None else None)
            space = (exact._at(ws, 4 * i + s0), 16 + 4 * nb)
            with _Span('sampled_nodes_pairs', device):
                _native.check(lib.ss_sampled_nodes_pairs(*args, lds_nodes, *outs, None, *space, stream), 'ss_sampled_nodes_pairs')
            with _Span('sampled_nodes_large', device):
                _native.check(lib.ss_sampled_nodes_large(*args, *outs, *space, slots, _ptr(arena), arena.numel(), stream),
                              'ss_sampled_nodes_large')

    if ev:
        ev[0].record()
    walk(None, None, None)
    if ev:
        ev[1].record()
    take = counts.to(torch.int64)
    if cap is not None:
        take.masked_fill_(counts > cap, 0)  # a row that is too long lists nothing
    rowptr = torch.zeros((L + 1,), dtype=torch.int64, device=device)
    torch.cumsum(take, 0, out=rowptr[1:])
    total = int(rowptr[-1])  # the one host read: the allocation
    ids = torch.empty((total,), dtype=torch.int64, device=device)
    hop = torch.empty((total,), dtype=torch.uint8, device=device)
    if ev:
        ev[2].record()
    if total:
        walk(rowptr, ids, hop)
    if ev:
        ev[3].record()
        ev[3].synchronize()
        for k, name in enumerate(('count_ms', 'rowptr_ms', 'fill_ms')):
            stats[name] = stats.get(name, 0.0) + ev[k].elapsed_time(ev[k + 1])
        stats['slots'], stats['nodes'] = slots, total
    out = (rowptr, ids, hop)
    if return_info:
        large, sampled = torch.stack([((state >> 1) & 1).sum(), (state & 1).sum()]).tolist()
        gone = torch.nonzero(counts > cap).flatten() if cap is not None else torch.empty((0,), dtype=torch.int64, device=device)
        out += ({'truncated': gone, 'lds_links': L - large, 'large_links': large, 'sampled_links': sampled},)
    if home != device:
        out = tuple(t.to(home) if torch.is_tensor(t) else {k: (x.to(home) if torch.is_tensor(x) else x) for k, x in t.items()} for t in out)
    return out
