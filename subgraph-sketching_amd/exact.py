"""Exact subgraph features (ElphHashes.exact_subgraph_features, csrc/ss_exact.hip): the sizes of the intersections of the k-hop balls of
u and v in the graph build_hash_tables propagates over, counted by BFS, and the feature algebra of get_subgraph_features applied to
them -- what the sketch query would return if MinHash and HLL++ were exact (reference hashing.py:139-189, 258-323).

Host side only: argument checks, the CSR (the engine's cache), launch planning per batch (the on-chip tier, then the large tier over
the pairs it left), the large tier's slot arena and the output tensors.  The node-list calls (exact_nodes.py, sampled_nodes.py) and
exact_subgraphs take their checks, the kernels' graph struct, the arena and the node rows of no links from here."""
from ctypes import byref, c_void_p

import torch

from . import _native, knobs
from ._runtime import _compute_device, _ptr, _stream, _Span

# (device, stream) -> (N, slots, zeroed uint8 slot arena of ss_exact_large).  One arena per STREAM: every slot's distance words must
# be zero when a call's large-tier launch starts and are zero again when it ends (the visit lists behind them are scratch, written
# before they are read), which holds for calls ordered on one stream; calls in flight on two streams at once get two arenas.  An
# entry is replaced (the old arena freed into the stream it was used on) when N or the slot count changes.
_ARENA = {}


def _at(t, offset):
    """device address of element `offset` of a contiguous tensor (None: a null pointer)"""
    return c_void_p(t.data_ptr() + offset * t.element_size()) if t is not None else c_void_p(0)


def _is_int_tensor(t):
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _arena(device, N):
    """(slots, arena) for the current stream of `device`: the large tier's persistent workgroups and their memory, all zero between
    calls (every call leaves it so).  At most knobs.EXACT_LARGE_SLOTS slots, and no more than a quarter of the free device memory"""
    slot_bytes = int(_native.lib().ss_exact_slot_bytes(N))
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    entry = _ARENA.get(key)
    want = int(knobs.EXACT_LARGE_SLOTS)
    if entry is not None and entry[0] == N and entry[3] == want:
        return entry[1], entry[2]
    _ARENA.pop(key, None)
    free, _ = torch.cuda.mem_get_info(device)
    slots = max(1, min(want, free // 4 // slot_bytes))
    arena = torch.zeros(slots * slot_bytes, dtype=torch.uint8, device=device)
    _ARENA[key] = (N, slots, arena, want)
    return slots, arena


def check_mask_target(mask_target):
    if not isinstance(mask_target, bool):
        raise ValueError(f'mask_target of the exact query is a bool (the links are masked in the edge_index given), got {type(mask_target).__name__}')


def csr_graph(eh, ei, N, device):
    """-> (the kernels' graph of `ei`, the implicit loops of build_hash_tables included, and the engine's cached CSR it points into: a
    repeated edge_index is not rebuilt; the struct holds addresses only, so the caller keeps the CSR for as long as it launches)"""
    csr = eh._csr_cache.get(ei, N, device)
    return _native.CsrGraphStruct(rowptr=csr.rowptr.data_ptr(), col=csr.col.data_ptr(), num_nodes=N, n_self_loops=0,
                                  n_self_loops_dev=csr.n_self_dev.data_ptr()), csr


def empty_rows(home, tail, return_info, **more):
    """what a node-list call returns for no links.  tail: the shape of what a listed node carries besides its id"""
    out = (torch.zeros((1,), dtype=torch.int64, device=home), torch.empty((0,), dtype=torch.int64, device=home),
           torch.empty((0,) + tail, dtype=torch.uint8, device=home))
    info = {'truncated': torch.empty((0,), dtype=torch.int64, device=home), 'lds_links': 0, 'large_links': 0, **more}
    return out + (info,) if return_info else out


def check_arguments(h, links, num_nodes, edge_index, batch_size):
    """-> (links [L, 2], edge_index [2, E], num_nodes, batch_size) after every check that needs no launch on the compute device"""
    if h not in (1, 2, 3):
        raise NotImplementedError('Only 1, 2 and 3 hop hashes are implemented')
    lk = torch.as_tensor(links)
    if lk.dim() == 1:
        lk = lk.unsqueeze(0)
    if lk.dim() != 2 or lk.size(1) != 2 or not _is_int_tensor(lk):
        raise ValueError(f'links must be an integer [L, 2] (or [2]) tensor, got {lk.dtype} {tuple(lk.shape)}')
    ei = torch.as_tensor(edge_index)
    if ei.dim() != 2 or ei.size(0) != 2 or not _is_int_tensor(ei):
        raise ValueError(f'edge_index must be an integer tensor of shape [2, num_edges], got {ei.dtype} {tuple(ei.shape)}')
    N = int(num_nodes)
    if N < 0 or N >= (1 << 31):
        raise ValueError(f'num_nodes must lie in [0, 2^31), got {N}')
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size must be positive, got {batch_size}')
    # the id ranges in ONE host read per device the inputs live on (a device read synchronises; both on one device: once)
    parts = {}
    for t in (lk, ei):
        if t.numel():
            parts.setdefault(t.device, []).extend(x.to(torch.int64) for x in torch.aminmax(t))
    read = {d: torch.stack(v).tolist() for d, v in parts.items()}
    if lk.numel():
        lo, hi = read[lk.device][0:2]
        if lo < -N or hi >= N:
            raise IndexError(f'links refer to nodes outside [-{N}, {N})')
    if ei.numel():
        lo, hi = read[ei.device][-2:]
        if lo < 0 or hi >= N:
            raise IndexError(f'edge_index refers to nodes outside [0, {N})')  # (what build_csr(check=True) raises)
    return lk, ei, N, batch_size


def exact_subgraph_features(eh, links, num_nodes, edge_index, batch_size=11000000, return_counts=False, stats=None, mask_target=False):
    """see ElphHashes.exact_subgraph_features.  stats (measurement hook, tools/probe_exact.py): a dict that receives the overflow
    count and the milliseconds of each tier, summed over batches (the call then synchronises after every launch)"""
    h = eh.max_hops
    check_mask_target(mask_target)
    lk, ei, N, batch_size = check_arguments(h, links, num_nodes, edge_index, batch_size)
    home, L, nf = lk.device, lk.size(0), h * (h + 2)
    if L == 0:
        feats = torch.empty((0, nf), dtype=torch.float32, device=home)
        if not return_counts:
            return feats
        return (feats, torch.empty((0, h, h), dtype=torch.int32, device=home), torch.empty((0, 2, h), dtype=torch.int32, device=home))
    device = _compute_device(lk, ei)
    graph, csr = csr_graph(eh, ei, N, device)
    lk = lk.to(device=device, dtype=torch.int64).contiguous()
    feats = torch.empty((L, nf), dtype=torch.float32, device=device)
    I = torch.empty((L, h, h), dtype=torch.int32, device=device) if return_counts else None
    balls = torch.empty((L, 2, h), dtype=torch.int32, device=device) if return_counts else None
    flags = (_native.SS_FLAG_USE_ZERO_ONE if eh.use_zero_one else 0) | (_native.SS_FLAG_FLOOR_SF if eh.floor_sf else 0)
    flags |= _native.SS_FLAG_MASK_TARGET if mask_target else 0
    lib = _native.lib()
    bmax = min(batch_size, L)
    ws_bytes = int(lib.ss_exact_workspace_bytes(bmax))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    slots, arena = _arena(device, N)
    stream = _stream(device)
    lds_nodes = max(0, int(knobs.EXACT_LDS_MAX_NODES))
    for s0 in range(0, L, batch_size):
        nb = min(batch_size, L - s0)
        args = (_at(lk, 2 * s0), nb, N, h, flags)
        outs = (_at(I, s0 * h * h), _at(balls, s0 * 2 * h), _at(feats, s0 * nf))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if stats is not None else None
        if ev:
            ev[0].record()
        with _Span('exact_pairs', device):
            _native.check(lib.ss_exact_pairs(byref(graph), *args, lds_nodes, *outs, None, _ptr(ws), ws_bytes, stream), 'ss_exact_pairs')
        if ev:
            ev[1].record()
        with _Span('exact_large', device):
            _native.check(lib.ss_exact_large(byref(graph), *args, *outs, _ptr(ws), ws_bytes, slots, _ptr(arena), arena.numel(), stream),
                          'ss_exact_large')
        if ev:
            ev[2].record()
            ev[2].synchronize()
            stats['overflow'] = stats.get('overflow', 0) + int(ws[:4].view(torch.int32).item())
            stats['lds_ms'] = stats.get('lds_ms', 0.0) + ev[0].elapsed_time(ev[1])
            stats['large_ms'] = stats.get('large_ms', 0.0) + ev[1].elapsed_time(ev[2])
            stats['slots'] = slots
    if home != device:
        feats = feats.to(home)
        I = I.to(home) if I is not None else None
        balls = balls.to(home) if balls is not None else None
    return (feats, I, balls) if return_counts else feats
