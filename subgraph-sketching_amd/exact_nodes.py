"""Exact subgraph node lists (ElphHashes.exact_subgraph_nodes, csrc/ss_exact_nodes.hip): per link (u, v) the nodes of
B_h(u) | B_h(v) with the distance pair (d_u, d_v) on each -- the enclosing subgraph's node set with its distance-encoding labels, what
exact_subgraph_features counts and then discards.  Design: DESIGN 3.17; numpy / scipy restatement: tests/exact_nodes_restatement.py.

Host side only: argument checks (exact.check_arguments), the graph struct (exact.csr_graph), the large tier's slot arena (exact._arena)
and the two walks over the batches that variable-length rows need: a count pass, ONE host read of the total for the allocation, a fill
pass.  That walk, the info dict and the move home are here once, for this call and for sampled_nodes.sampled_subgraph_nodes."""
from ctypes import byref

import torch

from . import _native, exact, knobs
from ._runtime import _compute_device, _ptr, _stream, _Span


def _cap(max_nodes):
    if max_nodes is None:
        return None
    if isinstance(max_nodes, bool) or int(max_nodes) != max_nodes or int(max_nodes) < 1:
        raise ValueError(f'max_nodes must be None or a positive integer, got {max_nodes!r}')
    return int(max_nodes)


def _two_pass_rows(device, L, batch_size, cap, stats, tail, launch):
    """the two walks over the batches: a count pass, the row pointer (rows longer than `cap` list nothing) with the one host read and
    the allocation, a fill pass (skipped when nothing is listed).  launch(s0, nb, counts, rowptr, ids, per_node, space) issues the two
    tier launches of the batch of links [s0, s0 + nb) -- the count pass when rowptr is None -- with space = (address, bytes) of the
    batch's workspace.  tail: as in exact.empty_rows.  stats: the measurement hook of the two calls (then this synchronises).
    -> (rowptr, ids, per_node, counts, ws, starts) on `device`; batch i's workspace begins at word 4 * i + starts[i] of ws"""
    starts = list(range(0, L, batch_size))
    # every batch keeps its own workspace (4 counter words, then its overflow list) from the count pass to the fill pass
    ws = torch.empty((4 * len(starts) + L,), dtype=torch.int32, device=device)
    counts = torch.empty((L,), dtype=torch.int32, device=device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if stats is not None else None

    def walk(rowptr, ids, per_node):
        for i, s0 in enumerate(starts):
            nb = min(batch_size, L - s0)
            launch(s0, nb, counts, rowptr, ids, per_node, (exact._at(ws, 4 * i + s0), 16 + 4 * nb))

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
    per_node = torch.empty((total,) + tail, dtype=torch.uint8, device=device)
    if ev:
        ev[2].record()
    if total:
        walk(rowptr, ids, per_node)
    if ev:
        ev[3].record()
        ev[3].synchronize()
        for k, name in enumerate(('count_ms', 'rowptr_ms', 'fill_ms')):
            stats[name] = stats.get(name, 0.0) + ev[k].elapsed_time(ev[k + 1])
        stats['nodes'] = total
    return rowptr, ids, per_node, counts, ws, starts


def _info(counts, cap, large, **more):
    """the info dict of a call (large: the large tier's links, read from the device by the caller)"""
    gone = torch.nonzero(counts > cap).flatten() if cap is not None else torch.empty((0,), dtype=torch.int64, device=counts.device)
    return {'truncated': gone, 'lds_links': counts.numel() - large, 'large_links': large, **more}


def _home(out, home):
    """a call's tuple (the rows, then the info dict if there is one) where the links live"""
    if home != out[0].device:
        out = tuple(t.to(home) if torch.is_tensor(t) else {k: (x.to(home) if torch.is_tensor(x) else x) for k, x in t.items()} for t in out)
    return out


def exact_subgraph_nodes(eh, links, num_nodes, edge_index, batch_size=11000000, mask_target=False, max_nodes=None, return_info=False,
                         stats=None):
    """see ElphHashes.exact_subgraph_nodes.  stats (measurement hook, tools/probe_exact_nodes.py): a dict that receives the milliseconds
    of the count pass, of the row pointer with its host read and allocation, and of the fill pass (the call then synchronises)"""
    h = eh.max_hops
    exact.check_mask_target(mask_target)
    cap = _cap(max_nodes)
    lk, ei, N, batch_size = exact.check_arguments(h, links, num_nodes, edge_index, batch_size)
    home, L = lk.device, lk.size(0)
    if L == 0:
        return exact.empty_rows(home, (2,), return_info)
    device = _compute_device(lk, ei)
    graph, csr = exact.csr_graph(eh, ei, N, device)
    lk = lk.to(device=device, dtype=torch.int64).contiguous()
    flags = _native.SS_FLAG_MASK_TARGET if mask_target else 0
    lib = _native.lib()
    slots, arena = exact._arena(device, N)
    stream = _stream(device)
    lds_nodes = max(0, int(knobs.EXACT_LDS_MAX_NODES))

    def launch(s0, nb, counts, rowptr, ids, dist, space):
        args = (byref(graph), exact._at(lk, 2 * s0), nb, N, h, flags)
        outs = (exact._at(counts, s0), exact._at(rowptr, s0), _ptr(ids), _ptr(dist))
        with _Span('exact_nodes_pairs', device):
            _native.check(lib.ss_exact_nodes_pairs(*args, lds_nodes, *outs, None, *space, stream), 'ss_exact_nodes_pairs')
        with _Span('exact_nodes_large', device):
            _native.check(lib.ss_exact_nodes_large(*args, *outs, *space, slots, _ptr(arena), arena.numel(), stream),
                          'ss_exact_nodes_large')

    rowptr, ids, dist, counts, ws, starts = _two_pass_rows(device, L, batch_size, cap, stats, (2,), launch)
    if stats is not None:
        stats['slots'] = slots
    out = (rowptr, ids, dist)
    if return_info:
        heads = torch.tensor([4 * i + s0 for i, s0 in enumerate(starts)], dtype=torch.int64, device=device)
        out += (_info(counts, cap, int(ws[heads].sum())),)  # (the overflow counts of the count pass)
    return _home(out, home)
