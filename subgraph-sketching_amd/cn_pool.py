"""Node features pooled over every link's common neighbours, trainable (csrc/ss_cn_rows.hip): the common-neighbour term
of Neural Common Neighbour, `x[u] * x[v]` concatenated with the sum of LEARNED embeddings h[w] over the common neighbours w of (u, v).
  CommonNeighbourBatch(A, links, weighting)   the plan: the list heuristics.common_neighbours returns, kept on the device, with
                                              everything the backward needs
  CommonNeighbourBatch.from_lists(...)        the same plan from a caller's own list
  common_neighbour_pool(x, batch)             float32 [L, F], out[q] = sum over the entries k of link q of coef[k] * x[ids[k]]
A list is (rowptr int64 [L + 1], ids int64 [T], coef float32 [T]); entry k belongs to link owner[k], the q with rowptr[q] <= k <
rowptr[q + 1].  torch writes the product as `coef[:, None] * x[ids]` and an index_add_: a [T, F] tensor, and float atomics in both
directions that serialise on every hub -- the node that is a common neighbour of many links of the batch.  Here both directions are
the chunked row sum ss_aggr.hip and ss_link_decoder.hip are pinned to: a row's entries in chunks of 256, each chunk
summed sequentially from +0, the chunk sums added in chunk order, products and adds rounded separately:
  forward   out[q]    = the chunked sum of fl(coef[k] * x[ids[k]])   over k = rowptr[q] .. rowptr[q + 1] - 1, list order; empty: +0.0
  backward  grad_x[n] = the chunked sum of fl(coef[k] * g[owner[k]]) over the entries with ids[k] == n, ascending k; zeros for rows
            no entry names.  coef and the list are constants: there is no gradient with respect to them.
Forward and backward repeat bit for bit, and a row's bits depend on its own entries and their order alone -- not on the tier (rows of
more than hub_entries entries are cut at chunk boundaries, one lane group per chunk, and a finish launch adds the partials in order),
not on the other rows or the batch, not on whether float4 or scalar pieces ran (F % 4 != 0 or a misaligned base; nothing is padded).
For a link of at most 256 common neighbours the forward row IS heuristics.common_neighbour_features' row, bit for bit: one chunk is
that function's sequential sum, and a sum begun at +0 is never -0.  A link of more than 256 follows the chunk rule and may differ
from it in the last bits.

x is float32 [N, F] on the plan's device: there is no CPU fallback and no silent copy.
"""
import torch

from . import _native, heuristics
from ._plans import finish_hubs, list_hubs
from ._runtime import _compute_device, _error_flag, _ptr, _stream
from .sign import group_ids_stable

CN_ROWS_CHUNK = 256  # the unit's SS_CN_ROWS_CHUNK, which ss_cn_rows_chunk() returns: a plan checks that the two agree
# rows of more than this many entries go through the hub tier: the value the sweeps of aggr (profiles/aggr_probe.txt) and of the link
# decoder (profiles/link_decoder_probe.txt) chose for the same kernels; not swept again here
DEFAULT_HUB_ENTRIES = 256

_LIMIT = 1 << 31


def _check_hub(hub_entries):
    hub = DEFAULT_HUB_ENTRIES if hub_entries is None else hub_entries
    if isinstance(hub, bool) or not isinstance(hub, int) or not 1 <= hub < 1 << 63:
        raise ValueError(f'hub_entries must be a positive integer below 2^63, got {hub_entries!r}')
    return hub


def _check_num_nodes(num_nodes):
    n = int(num_nodes)
    if n < 1 or n >= _LIMIT:
        raise ValueError(f'num_nodes must lie in [1, 2^31), got {num_nodes}')
    return n


def _resolve_device(device, *tensors):
    """where a plan lives: `device` (a bare 'cuda' names the current GPU, so that x.device compares equal), else the first GPU
    tensor's, else the current GPU"""
    if device is None:
        return _compute_device(*tensors)
    device = torch.device(device)
    if device.type != 'cuda':
        raise ValueError(f'a plan lives on a GPU, got device {device}: there is no CPU fallback')
    return device if device.index is not None else torch.device('cuda', torch.cuda.current_device())


class CommonNeighbourBatch(object):
    """The plan of `common_neighbour_pool`: the common neighbours of links (int tensor [L, 2]) in A (a scipy sparse adjacency matrix
    or a heuristics.DeviceAdjacency) as the list `heuristics.common_neighbours(A, links, weighting)` returns -- the same rowptr, ids
    and coef, made by the same two launches -- kept on the device, plus what the two directions need: owner (int64 [T], the link of
    every entry), the stable grouping of the entries by node (nodes: the M distinct named nodes, ascending, int64 [M]; node_rowptr
    int64 [M + 1]; order int32 [T], the entries of every node ascending) and the rows of more than `hub_entries` entries on BOTH
    sides -- links and nodes -- listed on the device with the offsets of their 256-entry chunks.
    weighting: 'CN', 'AA', 'RA' or a 1-D float multiplier of length N, as common_neighbour_features takes it; None is refused.
    links is copied: later edits do not reach a plan.  hub_entries: None takes DEFAULT_HUB_ENTRIES.  device: where the plan lives
    (default: the links' GPU, or the current one for host tensors).  Argument errors are raised before anything touches a device.
    Two host reads: T, which the list itself costs, and one for the flags, M and the four hub totals.  A link id outside [0, N)
    raises IndexError."""
    builds = 0  # plans built so far (tests count them)

    def __init__(self, A, links, weighting='CN', hub_entries=None, device=None):
        links = heuristics._check_links(links)
        weighting = heuristics._check_weighting(A, weighting, allow_none=False)
        hub = _check_hub(hub_entries)
        n = _check_num_nodes(heuristics._num_nodes(A))
        L = links.size(0)
        if L >= _LIMIT:
            raise ValueError('batches of 2^31 links or more are not supported')
        device = _resolve_device(device, links)
        adj = heuristics._adjacency(A, device)
        if adj.device != device:
            raise ValueError(f'the adjacency is on {adj.device}, the plan on {device}')
        lib, stream, err = _native.lib(), _stream(device), _error_flag(device)
        lk = links.detach().to(device=device, dtype=torch.int64, copy=True).contiguous()
        mult, _ = heuristics._multiplier(adj, weighting)
        rowptr = torch.zeros(L + 1, dtype=torch.int64, device=device)
        T = 0
        if L:
            counts = torch.empty(L, dtype=torch.int64, device=device)
            _native.check(lib.ss_common_neighbour_count(_ptr(adj.rowptr), _ptr(adj.col), n, _ptr(lk), L, _ptr(counts), _ptr(err), stream),
                          'ss_common_neighbour_count')
            torch.cumsum(counts, 0, out=rowptr[1:])
            T = int(rowptr[-1].item())  # (the host read the list costs)
        if T >= _LIMIT:
            raise ValueError('lists of 2^31 entries or more are not supported')
        ids = torch.empty(max(T, 1), dtype=torch.int64, device=device)  # (never an empty device buffer behind the C ABI)
        coef = torch.empty(max(T, 1), dtype=torch.float32, device=device)
        if T:
            _native.check(lib.ss_common_neighbour_fill(_ptr(adj.rowptr), _ptr(adj.col), _ptr(adj.val), _ptr(mult), n, _ptr(lk), L, _ptr(rowptr),
                                                       _ptr(ids), _ptr(coef), _ptr(err), stream), 'ss_common_neighbour_fill')
        self.links = lk
        self._plan(n, rowptr, ids[:T], coef[:T], hub, device, links_flag=err)

    @classmethod
    def from_lists(cls, num_nodes, rowptr, ids, coef, hub_entries=None, device=None):
        """The plan of a caller's own list: rowptr int64 [L + 1] (starts at 0, non-decreasing, ends at T), ids int64 [T], coef float32
        [T].  ids need not ascend or be distinct inside a row: list order is the accumulation order.  The three tensors are copied.
        ValueError for a rowptr that is not monotone or does not run from 0 to T; IndexError for an id outside [0, num_nodes),
        negative ones included -- both before anything touches a device when the tensors are on the host, else with the plan's one
        host read."""
        n = _check_num_nodes(num_nodes)
        hub = _check_hub(hub_entries)
        if not isinstance(rowptr, torch.Tensor) or rowptr.dtype != torch.int64 or rowptr.dim() != 1 or rowptr.numel() < 1:
            raise ValueError('rowptr must be an int64 tensor [L + 1]')
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError('ids must be an int64 tensor [T]')
        if not isinstance(coef, torch.Tensor) or coef.dtype != torch.float32 or coef.shape != ids.shape:
            raise ValueError('coef must be a float32 tensor [T], one coefficient per id')
        if coef.requires_grad:
            raise ValueError('coef is not differentiable here: pass coef.detach()')
        L, T = rowptr.numel() - 1, ids.numel()
        if L >= _LIMIT or T >= _LIMIT:
            raise ValueError('lists of 2^31 links or entries, or more, are not supported')
        rowptr_flag = None
        if not rowptr.is_cuda:
            if not _rowptr_ok(rowptr, T):
                raise ValueError(f'rowptr must start at 0, never descend and end at T = {T}')
        if not ids.is_cuda and T and bool(((ids < 0) | (ids >= n)).any()):
            raise IndexError('ids refers to nodes outside [0, num_nodes)')
        device = _resolve_device(device, rowptr, ids, coef)
        if rowptr.is_cuda:
            rowptr_flag = (~_rowptr_ok(rowptr, T, as_tensor=True)).to(torch.int64).reshape(1).to(device)
        self = cls.__new__(cls)
        self.links = None
        to = lambda t: t.detach().to(device=device, copy=True).contiguous()
        self._plan(n, to(rowptr), to(ids), to(coef), hub, device, rowptr_flag=rowptr_flag)
        return self

    def _plan(self, n, rowptr, ids, coef, hub, device, links_flag=None, rowptr_flag=None):
        lib = _native.lib()
        if lib.ss_cn_rows_chunk() != CN_ROWS_CHUNK:
            raise RuntimeError(f'the library sums chunks of {lib.ss_cn_rows_chunk()} entries, this module lists chunks of {CN_ROWS_CHUNK}')
        L, T = rowptr.numel() - 1, ids.numel()
        self.num_nodes, self.num_links, self.num_entries, self.device, self.hub_entries = n, L, T, device, hub
        self.rowptr, self.ids, self.coef = rowptr, ids, coef
        i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=device)
        i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=device)
        word = lambda f: i64(1) if f is None else f.to(torch.int64).reshape(1)
        if T == 0:  # nothing to group; the kernels are never launched, the pointers exist all the same
            self.owner, self.nodes, self.node_rowptr, self.order = i64(0), i64(0), i64(1), i32(0)
            self.link_hubs = self.node_hubs = ((i32(1), i32(1), i32(1)), 0, 0)
            self.num_touched = 0
            if links_flag is not None or rowptr_flag is not None:
                self._raise(*torch.cat([word(links_flag), word(rowptr_flag)]).tolist(), 0, links_flag)
            CommonNeighbourBatch.builds += 1
            return
        counts = rowptr[1:] - rowptr[:-1]
        if rowptr_flag is not None:  # (a rowptr still to be judged: one that fails lists no hub, so the listing stays inside its cap)
            counts = counts * (1 - rowptr_flag)
        # the link of every entry: the last q with rowptr[q] <= k (empty rows repeat a pointer).  A rowptr that fails its check is
        # refused below; until then the clamp keeps every owner a row
        self.owner = (torch.searchsorted(rowptr, torch.arange(T, dtype=torch.int64, device=device), right=True) - 1).clamp_(0, max(L - 1, 0))
        err = i32(1)
        bad = ((ids < 0) | (ids >= n)).any().to(torch.int64).reshape(1)  # negative ids count as out of range: nothing wraps
        full, self.order = group_ids_stable(ids, n, err)
        m = full[1:] - full[:-1]
        # the touched nodes ascending with the starts of their groups, without a host read: a place per possible node, the spare one
        # collects the rest
        touched = m > 0
        pos = torch.cumsum(touched, 0) - 1
        cap_m = min(n, T)
        place = torch.where(touched, pos, torch.full_like(pos, cap_m))
        nodes = i64(cap_m + 1).scatter_(0, place, torch.arange(n, dtype=torch.int64, device=device))
        starts = i64(cap_m + 1).scatter_(0, place, full[:-1])
        # the hub rows of both sides: a row of more than `hub` entries, of which there are at most T // (hub + 1).  Links by their row
        # number, nodes by their position in `nodes`
        cap_h = T // (hub + 1)
        *link_listed, lh, lc = list_hubs(counts, hub, CN_ROWS_CHUNK, cap_h)
        *node_listed, nh, nc = list_hubs(m, hub, CN_ROWS_CHUNK, cap_h, names=pos.to(torch.int32))
        # (the one host read) the flags, M, and the four totals the hub launches are sized by
        flag, bad, bad_links, bad_rowptr, M, LH, LC, NH, NC = torch.cat(
            [err.to(torch.int64), bad, word(links_flag), word(rowptr_flag), touched.sum().reshape(1), lh, lc, nh, nc]).tolist()
        self._raise(bad_links, bad_rowptr, flag or bad, links_flag)
        self.link_hubs = (finish_hubs(*link_listed, LH, LC), LH, LC)
        self.node_hubs = (finish_hubs(*node_listed, NH, NC), NH, NC)
        self.num_touched = M
        self.nodes = nodes[:M].contiguous()
        self.node_rowptr = torch.cat([starts[:M], full[-1:]])
        CommonNeighbourBatch.builds += 1

    def _raise(self, bad_links, bad_rowptr, bad_ids, links_flag):
        if bad_links:
            links_flag.zero_()  # (the device's shared report word: read, so cleared)
            raise IndexError(f'links refers to nodes outside [0, {self.num_nodes})')
        if bad_rowptr:
            raise ValueError(f'rowptr must start at 0, never descend and end at T = {self.num_entries}')
        if bad_ids:
            raise IndexError('ids refers to nodes outside [0, num_nodes)')

    def forward(self, x):
        """out float32 [L, F] of one forward; x contiguous fp32 [N, F] on the plan's device"""
        L, T, n, F = self.num_links, self.num_entries, self.num_nodes, x.size(1)
        if F == 0 or L == 0 or T == 0:
            return torch.zeros((L, F), dtype=torch.float32, device=self.device)
        out = torch.empty((L, F), dtype=torch.float32, device=self.device)  # every row is stored: by the regular tier or by the finish
        lib, stream = _native.lib(), _stream(self.device)
        (hub_rows, hub_chunk, chunk_hub), H, C = self.link_hubs
        _native.check(lib.ss_cn_rows_forward(_ptr(self.rowptr), _ptr(self.ids), _ptr(self.coef), L, T, n, self.hub_entries, _ptr(x), F, _ptr(out),
                                             stream), 'ss_cn_rows_forward')
        if H:
            ws_bytes = lib.ss_cn_rows_workspace_bytes(C, F)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            _native.check(lib.ss_cn_rows_forward_hub_partials(_ptr(self.rowptr), _ptr(self.ids), _ptr(self.coef), L, T, n, _ptr(hub_rows),
                                                              _ptr(hub_chunk), _ptr(chunk_hub), H, C, _ptr(x), F, _ptr(ws), ws_bytes, stream),
                          'ss_cn_rows_forward_hub_partials')
            _native.check(lib.ss_cn_rows_forward_hub_finish(L, _ptr(hub_rows), _ptr(hub_chunk), H, C, _ptr(ws), ws_bytes, F, _ptr(out), stream),
                          'ss_cn_rows_forward_hub_finish')
        return out

    def grad(self, g):
        """grad_x float32 [N, F] of one backward; g contiguous fp32 [L, F].  Only the M named rows are walked: the others are the
        allocation's zeros."""
        L, T, n, M, F = self.num_links, self.num_entries, self.num_nodes, self.num_touched, g.size(1)
        grad_x = torch.zeros((n, F), dtype=torch.float32, device=self.device)
        if F == 0 or M == 0:
            return grad_x
        lib, stream = _native.lib(), _stream(self.device)
        (hub_rows, hub_chunk, chunk_hub), H, C = self.node_hubs
        _native.check(lib.ss_cn_rows_grad(_ptr(self.nodes), _ptr(self.node_rowptr), _ptr(self.order), M, _ptr(self.owner), _ptr(self.coef), T, L, n,
                                          self.hub_entries, _ptr(g), F, _ptr(grad_x), stream), 'ss_cn_rows_grad')
        if H:
            ws_bytes = lib.ss_cn_rows_workspace_bytes(C, F)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            _native.check(lib.ss_cn_rows_grad_hub_partials(_ptr(self.node_rowptr), _ptr(self.order), M, _ptr(self.owner), _ptr(self.coef), T, L, n,
                                                           _ptr(hub_rows), _ptr(hub_chunk), _ptr(chunk_hub), H, C, _ptr(g), F, _ptr(ws), ws_bytes,
                                                           stream), 'ss_cn_rows_grad_hub_partials')
            _native.check(lib.ss_cn_rows_grad_hub_finish(_ptr(self.nodes), M, _ptr(hub_rows), _ptr(hub_chunk), H, C, n, _ptr(ws), ws_bytes, F,
                                                         _ptr(grad_x), stream), 'ss_cn_rows_grad_hub_finish')
        return grad_x


def _rowptr_ok(rowptr, T, as_tensor=False):
    ok = (rowptr[0] == 0) & (rowptr[-1] == T) & (rowptr[1:] >= rowptr[:-1]).all()
    return ok if as_tensor else bool(ok)


class _CommonNeighbourPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, batch):
        ctx.batch = batch  # nothing else is saved: the product is linear in x
        return batch.forward(x.contiguous())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return ctx.batch.grad(g.contiguous()), None


def common_neighbour_pool(x, batch):
    """float32 [L, F], out[q] = the chunked sum (module docstring) of fl(coef[k] * x[ids[k]]) over the entries of link q in list
    order; a link without entries gets +0.0.  x: float32 [N, F] on the plan's device; batch: a CommonNeighbourBatch.  Differentiable
    in x: grad_x[n] = the chunked sum of fl(coef[k] * g[owner[k]]) over the entries with ids[k] == n, ascending k; zeros for the rows
    no entry names.  Nothing but the plan is kept for the backward.  Equal to heuristics.common_neighbour_features bit for bit on
    every link of at most 256 common neighbours; longer rows follow the chunk rule.  ValueError for anything else: another dtype,
    another device, a wrong N."""
    if not isinstance(batch, CommonNeighbourBatch):
        raise ValueError('batch must be a CommonNeighbourBatch')
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError('x must be a float32 tensor [N, F]')
    if x.size(0) != batch.num_nodes:
        raise ValueError(f'x must be a float32 tensor [{batch.num_nodes}, F], it has {x.size(0)} rows')
    if x.size(1) >= _LIMIT:
        raise ValueError('F must be below 2^31')
    if x.device != batch.device:
        raise ValueError(f'x is on {x.device}, the plan on {batch.device}: there is no CPU fallback and no silent copy')
    return _CommonNeighbourPool.apply(x, batch)
