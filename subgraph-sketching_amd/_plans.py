"""What the plans of the feature-row products share (gcn.GCNGraph, aggr.AggrGraph, link_decoder.LinkBatch, sign): the checks and the
device copy of an edge list, the hub-row listing, the identity-keyed plan cache of the layers, and the padding of feature rows to whole
float4 pieces.  Everything here is torch on whatever device the tensors live on: nothing calls the library."""
import weakref

import torch


def check_edge_list(num_nodes, edge_index, edge_weight):
    """-> (n, E) for an edge list a plan accepts; ValueError otherwise"""
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
        raise ValueError('edge_index must be an int64 tensor [2, E]')
    n = int(num_nodes)
    if n < 1 or n >= 1 << 31:
        raise ValueError(f'num_nodes must lie in [1, 2^31), got {num_nodes}')
    E = edge_index.size(1)
    if edge_weight is not None:
        if not isinstance(edge_weight, torch.Tensor) or edge_weight.shape != (E,) or not edge_weight.is_floating_point():
            raise ValueError('edge_weight must be a floating-point tensor [E]')
        if edge_weight.requires_grad:
            raise ValueError('edge_weight is not differentiable here: pass edge_weight.detach()')
    return n, E


def device_edge_list(edge_index, edge_weight, device, unit_weights):
    """-> (ei, row, col, w, no_order): the plan's own copy of the edge list on `device` (later edits of the caller's tensors do not
    reach it).  ei: int64 [2, E]; row, col: its two rows; w: float32 [E], for edge_weight None `unit_weights(E)` (ones, or None for
    kernels that never gather unit weights).  E == 0: the kernels never dereference an empty edge list, but the pointers must exist --
    row, col and w (unless None) are size-1 zeros, and no_order is the size-1 int32 stand-in for an empty order array (an empty slice
    has no address); otherwise no_order is None."""
    E = edge_index.size(1)
    ei = edge_index.detach().to(device=device, copy=True).contiguous()
    row, col = ei[0], ei[1]
    w = unit_weights(E) if edge_weight is None else edge_weight.detach().to(device=device, dtype=torch.float32, copy=True)
    no_order = None
    if E == 0:
        w = None if w is None else torch.zeros(1, dtype=torch.float32, device=device)
        row = col = torch.zeros(1, dtype=torch.int64, device=device)
        no_order = torch.zeros(1, dtype=torch.int32, device=device)
    return ei, row, col, w, no_order


def list_hubs(m, hub_entries, chunk, cap, names=None):
    """The device phase of the hub listing, without a host read.  m: int64 [n], the entries of every row; a row of more than
    hub_entries entries is a hub, cut into chunks of `chunk` entries; cap: there are at most this many hubs.  A slot per possible hub,
    the spare one collects the rest.  -> (rows int32 [cap + 1]: the hubs ascending, as row numbers or as names[row] (int32 [n]);
    chunks int64 [cap + 1]: their chunk counts; hub_chunk int64 [cap + 1]: where the chunks of every hub start; the number of hubs and
    of chunks as int64 [1] tensors for the caller's one host read)"""
    device = m.device
    is_hub = m > hub_entries
    slot = torch.where(is_hub, torch.cumsum(is_hub, 0) - 1, torch.full_like(m, cap))
    if names is None:
        names = torch.arange(m.numel(), dtype=torch.int32, device=device)
    rows = torch.zeros(cap + 1, dtype=torch.int32, device=device).scatter_(0, slot, names)
    chunks = torch.zeros(cap + 1, dtype=torch.int64, device=device).scatter_(0, slot, (m + (chunk - 1)) // chunk)
    chunks[cap] = 0
    hub_chunk = torch.zeros(cap + 1, dtype=torch.int64, device=device)
    torch.cumsum(chunks[:cap], 0, out=hub_chunk[1:])
    return rows, chunks, hub_chunk, is_hub.sum().reshape(1), hub_chunk[-1:]


def finish_hubs(rows, chunks, hub_chunk, H, C):
    """The finish phase, once the host knows the H hubs and their C chunks: -> (hub_rows int32 [max(H, 1)], hub_chunk int32 [H + 1],
    chunk_hub int32 [C]: the hub of every chunk; a size-1 stand-in for H == 0)"""
    if C >= 1 << 31:
        raise ValueError('the hub rows have 2^31 chunks or more')
    device = rows.device
    chunk_hub = torch.repeat_interleave(torch.arange(H, dtype=torch.int32, device=device), chunks[:H], output_size=C) if H else \
        torch.zeros(1, dtype=torch.int32, device=device)
    return rows[:max(H, 1)].contiguous(), hub_chunk[:H + 1].to(torch.int32), chunk_hub


def _identity(t):
    # A tensor made under torch.inference_mode() tracks no version (reading t._version raises).  It is still cached, keyed on
    # object, address and shape alone: outside inference mode torch refuses every in-place edit of it, so there the key cannot go
    # stale; an edit INSIDE an inference_mode block goes unseen -- pass a plan, or a fresh tensor, after such an edit.  Not
    # caching it instead would rebuild the plan in every conv of an evaluation loop, which is what the cache exists to avoid.
    if t is None:
        return None
    return (weakref.ref(t), t.data_ptr(), tuple(t.shape), None if t.is_inference() else t._version)


def _same(a, b):
    if a is None or b is None:
        return a is b
    return a[0]() is not None and a[0]() is b[0]() and a[1:] == b[1:]


class _PlanCache(object):
    """The plan of the tensors seen last, shared by the layers of one module: the convs of one forward do one build.  Keyed on plain
    values and on the IDENTITY of tensors -- the same tensor object, storage address, shape and version counter (an in-place edit bumps
    it) -- never on content: a fresh tensor of equal content rebuilds."""

    def __init__(self):
        self._key = self._plan = None

    def get(self, plain, tensors, build):
        """the cached plan if `plain` (a tuple of plain values) and every one of `tensors` (tensors or None) are those of the last
        call, else build()"""
        key = (plain, tuple(_identity(t) for t in tensors))
        old = self._key
        if old is None or old[0] != key[0] or len(old[1]) != len(key[1]) or not all(_same(a, b) for a, b in zip(old[1], key[1])):
            self._key = self._plan = None
            self._plan = build()
            self._key = key
        return self._plan


def padded_rows(run, F, *xs):
    """run(F', *xs') -> [N, F'] on feature rows padded with zero columns to F', the next multiple of 4 (the kernels move float4
    pieces), sliced back to the F columns asked for.  xs: tensors [N, F], or None (passed through)."""
    pad = (-F) % 4
    if pad:
        xs = [x if x is None else torch.nn.functional.pad(x, (0, pad)) for x in xs]
    out = run(F + pad, *xs)
    return out[:, :F] if pad else out
