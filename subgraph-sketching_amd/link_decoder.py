"""The link decoder's endpoint gather and Hadamard product in HIP (csrc/ss_link_decoder.hip): the one graph-shaped step
of every training loop of the reference that torch indexing still did here.
  link_gather(x, links)    float32 [L, 2, F], out[l, s] = x[links[l, s]]: what `x[links]` gives (reference runners/train.py:56, :63, :200,
                           :201 -- node_features[curr_links], emb[curr_links], data.x[curr_links])
  link_hadamard(x, links)  float32 [L, F], out[l] = x[links[l, 0]] * x[links[l, 1]]: `x[:, 0, :] * x[:, 1, :]` of
                           LinkPredictor.feature_forward (models/elph.py:54) and `x_i * x_j` (models/gnn.py:212) on the gathered rows, as
                           one fp32 multiply -- torch's bits -- without the [L, 2, F] tensor in between
Both are torch.autograd.Functions, differentiable in x.  torch's backward of `x[links]` is an index_put with float atomics: a node at
the end of several links of the batch receives its gradient rows in whatever order the hardware delivers them.  Here the 2L endpoint
slots q = 2l + s are grouped by node (`LinkBatch`, the plan) and every touched row of grad_x is summed by the accumulation order
ss_aggr.hip is pinned to: the row's slots ascending, in chunks of 256, each summed sequentially from +0, the chunk sums
added in chunk order.  term t_q = g[l, s] for the gather, fl(g[l] * x[links[l, 1 - s]]) for the product; a self link (u, u) is two
slots of u.  Forward and backward repeat bit for bit, and a row's bits depend on its own slots and their order alone -- not on the
tier (rows of more than hub_entries slots are cut at chunk boundaries, one lane group per chunk, and a finish launch adds the
partials in order), not on the other links of the batch.

x is float32 [N, F] on the GPU: there is no CPU fallback and no silent copy.  links is an int64 tensor [L, 2] (the layout
get_subgraph_features takes) or a LinkBatch.  Given a tensor, a plan is built at forward time only when x.requires_grad and grad mode
is on; otherwise nothing is grouped and nothing is read from the device: an id outside [0, N) is then not followed, its output row
(for the product: the link's row) is zeros, and it is reported late, like pooling's deferred errors: by the next call into this module
or by check_errors(), as IndexError.  A caller who gathers several tensors at the same links (node features and embeddings at
curr_links) builds ONE LinkBatch and passes it to every call.
"""
import torch

from . import _native
from ._plans import finish_hubs, list_hubs
from ._runtime import _DeferredErrors, _compute_device, _ptr, _stream
from .sign import group_ids_stable

LINK_CHUNK = 256  # the unit's SS_LINK_CHUNK, which ss_link_chunk() returns: a plan checks that the two agree
# rows of more than this many slots go through the hub tier.  Measured (profiles/link_decoder_probe.txt): on the rank^-0.9
# batch of 1 048 576 links (41 929 slots on one node) link_hadamard forward + backward takes 11.2 / 11.4 / 46.6 ms without the tier and
# 0.64 / 1.17 / 4.81 ms at 256 (F = 128 / 256 / 1024); 256, one chunk, was the fastest of 256 .. 8192 at every width there and at
# 65 536 links (0.14 / 0.24 / 0.92 ms against 0.18 / 0.28 / 1.10 ms at 512), and a batch without such rows never launches the tier.
DEFAULT_HUB_ENTRIES = 256

_ERRORS = _DeferredErrors()


def _raise_if_set(synchronize=False):
    calls = ', '.join(_ERRORS._calls)
    try:
        _ERRORS.raise_if_set(synchronize=synchronize)
    except IndexError:
        raise IndexError(f'an earlier link_gather / link_hadamard without a plan was given link ids outside [0, num_nodes) (reported '
                         f'late); the rows of such links are zeros. Calls since the last clean check: {calls}') from None


def check_errors():
    """waits for the device, then raises IndexError if a forward-only call since the last check met a link id out of range"""
    _raise_if_set(synchronize=True)


def _check_links(links):
    if not isinstance(links, torch.Tensor) or links.dtype != torch.int64 or links.dim() != 2 or links.size(1) != 2:
        raise ValueError('links must be an int64 tensor [L, 2] (or a LinkBatch)')
    if links.size(0) >= 1 << 30:
        raise ValueError('batches of 2^30 links or more are not supported')


class LinkBatch(object):
    """The plan of the backward of `link_gather` / `link_hadamard`: the 2L endpoint slots q = 2l + s of links (int64 [L, 2]) grouped
    by node.  nodes: the M distinct touched nodes, ascending (int64 [M]); rowptr: int64 [M + 1]; order: int32 [2L], the slot ids of
    every node ascending (a STABLE grouping: the order inside a group is the accumulation order).  The rows of more than `hub_entries`
    slots are listed on the device as positions in `nodes` (hub_rows) with the offsets of their 256-slot chunks (hub_chunk, chunk_hub).
    Built with torch ops on the device and ONE host read: the bounds flag, M and the two hub totals.  Ids outside [0, num_nodes) --
    negative ones too -- raise IndexError.  links is copied: later edits do not reach a plan.  hub_entries: None takes
    DEFAULT_HUB_ENTRIES.  device: where the plan lives (default: the links' GPU, or the current one for host tensors)."""
    builds = 0  # plans built so far (tests count them)

    def __init__(self, num_nodes, links, hub_entries=None, device=None):
        _check_links(links)
        n = int(num_nodes)
        if n < 1 or n >= 1 << 31:
            raise ValueError(f'num_nodes must lie in [1, 2^31), got {num_nodes}')
        hub = DEFAULT_HUB_ENTRIES if hub_entries is None else hub_entries
        if isinstance(hub, bool) or not isinstance(hub, int) or not 1 <= hub < 1 << 63:
            raise ValueError(f'hub_entries must be a positive integer below 2^63, got {hub_entries!r}')
        lib = _native.lib()
        if lib.ss_link_chunk() != LINK_CHUNK:
            raise RuntimeError(f'the library sums chunks of {lib.ss_link_chunk()} slots, this module lists chunks of {LINK_CHUNK}')
        device = torch.device(device) if device is not None else _compute_device(links)  # (host tensors: the current GPU)
        L = links.size(0)
        self.links = links.detach().to(device=device, copy=True).contiguous()
        self.num_nodes, self.num_links, self.device, self.hub_entries = n, L, device, hub
        i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=device)
        if L == 0:  # nothing to group, nothing to read; the kernels are never launched, but the pointers exist
            self.links = torch.zeros((1, 2), dtype=torch.int64, device=device)
            self.nodes, self.rowptr = torch.zeros(0, dtype=torch.int64, device=device), torch.zeros(1, dtype=torch.int64, device=device)
            self.order, self.hub_rows, self.hub_chunk, self.chunk_hub = i32(0), i32(1), i32(1), i32(1)
            self.num_touched = self.n_hubs = self.n_chunks = 0
            LinkBatch.builds += 1
            return
        slots = self.links.view(-1)  # slot q = 2l + s is position q of the row-major [L, 2] tensor
        err = i32(1)
        bad = ((slots < 0) | (slots >= n)).any().to(torch.int64).reshape(1)  # negative ids count as out of range: nothing wraps
        full, self.order = group_ids_stable(slots, n, err)
        m = full[1:] - full[:-1]
        ids = torch.arange(n, dtype=torch.int64, device=device)
        # the touched nodes ascending with the starts of their groups, without a host read: a place per possible node, the spare one
        # collects the rest
        touched = m > 0
        pos = torch.cumsum(touched, 0) - 1
        cap_m = min(n, 2 * L)
        place = torch.where(touched, pos, torch.full_like(pos, cap_m))
        nodes = torch.zeros(cap_m + 1, dtype=torch.int64, device=device).scatter_(0, place, ids)
        starts = torch.zeros(cap_m + 1, dtype=torch.int64, device=device).scatter_(0, place, full[:-1])
        # the hub rows likewise, named by their position in `nodes`; a row of more than `hub` slots: there are at most 2L // (hub + 1)
        *listed, n_hubs, n_chunks = list_hubs(m, hub, LINK_CHUNK, 2 * L // (hub + 1), names=pos.to(torch.int32))
        # (the one host read) the grouping's flag and the sign test, M, and the two totals the hub launches are sized by
        flag, bad, M, H, C = torch.cat([err.to(torch.int64), bad, touched.sum().reshape(1), n_hubs, n_chunks]).tolist()
        hub_lists = finish_hubs(*listed, H, C)
        self.num_touched, self.n_hubs, self.n_chunks = M, H, C
        self.nodes = nodes[:M].contiguous()
        self.rowptr = torch.cat([starts[:M], full[-1:]])
        self.hub_rows, self.hub_chunk, self.chunk_hub = hub_lists
        if flag or bad:
            raise IndexError('links refers to nodes outside [0, num_nodes)')
        LinkBatch.builds += 1

    def grad(self, g, x=None):
        """grad_x float32 [N, F] of one backward.  x None: the gather, g contiguous fp32 [L, 2, F]; else the product, g contiguous
        fp32 [L, F] and x the forward's contiguous [N, F].  Only the M touched rows are walked: the others are the allocation's zeros."""
        n, L, F = self.num_nodes, self.num_links, g.size(-1)
        grad_x = torch.zeros((n, F), dtype=torch.float32, device=self.device)
        if F == 0 or self.num_touched == 0:
            return grad_x
        mode = 0 if x is None else 1
        lib, stream, M = _native.lib(), _stream(self.device), self.num_touched
        _native.check(lib.ss_link_grad_rows(_ptr(self.nodes), _ptr(self.rowptr), _ptr(self.order), M, _ptr(self.links), L, n, self.hub_entries, mode,
                                            _ptr(g), _ptr(x), F, _ptr(grad_x), stream), 'ss_link_grad_rows')
        if self.n_hubs:
            ws_bytes = lib.ss_link_workspace_bytes(self.n_chunks, F)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            _native.check(lib.ss_link_grad_hub_partials(_ptr(self.rowptr), _ptr(self.order), M, _ptr(self.links), L, n, _ptr(self.hub_rows),
                                                        _ptr(self.hub_chunk), _ptr(self.chunk_hub), self.n_hubs, self.n_chunks, mode, _ptr(g), _ptr(x), F,
                                                        _ptr(ws), ws_bytes, stream), 'ss_link_grad_hub_partials')
            _native.check(lib.ss_link_grad_hub_finish(_ptr(self.nodes), M, _ptr(self.hub_rows), _ptr(self.hub_chunk), self.n_hubs, self.n_chunks, n,
                                                      _ptr(ws), ws_bytes, F, _ptr(grad_x), stream), 'ss_link_grad_hub_finish')
        return grad_x


class _LinkGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, links, L, batch, err):
        x = x.contiguous()
        N, F = x.shape
        out = torch.empty((L, 2, F), dtype=torch.float32, device=x.device)
        _native.check(_native.lib().ss_link_gather(_ptr(links), L, _ptr(x), N, F, _ptr(out), _ptr(err), _stream(x.device)), 'ss_link_gather')
        ctx.batch, ctx.shape = batch, (N, F)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.batch is None:  # (no link at all: see _prepare)
            return torch.zeros(ctx.shape, dtype=torch.float32, device=g.device), None, None, None, None
        return ctx.batch.grad(g.contiguous()), None, None, None, None


class _LinkHadamard(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, links, L, batch, err):
        x = x.contiguous()
        N, F = x.shape
        out = torch.empty((L, F), dtype=torch.float32, device=x.device)
        _native.check(_native.lib().ss_link_hadamard(_ptr(links), L, _ptr(x), N, F, _ptr(out), _ptr(err), _stream(x.device)), 'ss_link_hadamard')
        ctx.batch, ctx.shape = batch, (N, F)
        if batch is not None:
            ctx.save_for_backward(x)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.batch is None:
            return torch.zeros(ctx.shape, dtype=torch.float32, device=g.device), None, None, None, None
        (x,) = ctx.saved_tensors
        return ctx.batch.grad(g.contiguous(), x), None, None, None, None


def _prepare(x, links, what):
    """-> (links int64 [L, 2] on x.device, L, the plan or None, the report word)"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError('x must be a float32 tensor [N, F]')
    if isinstance(links, LinkBatch):
        if x.size(0) != links.num_nodes:
            raise ValueError(f'x must be a float32 tensor [{links.num_nodes}, F]')
        if x.device != links.device:
            raise ValueError(f'x is on {x.device}, the links on {links.device}: there is no CPU fallback and no silent copy')
        batch, lk, L = links, links.links, links.num_links
    else:
        _check_links(links)
        if not x.is_cuda:
            raise ValueError('x must be on the GPU: there is no CPU fallback and no silent copy')
        if links.device != x.device:
            raise ValueError(f'links is on {links.device}, x on {x.device}: there is no silent copy')
        batch, lk, L = None, links.contiguous(), links.size(0)
        if x.requires_grad and torch.is_grad_enabled() and L:
            if x.size(0) == 0:
                raise IndexError('links refers to nodes outside [0, num_nodes)')
            batch = LinkBatch(x.size(0), lk, device=x.device)
            lk = batch.links  # the copy the backward reads
    _raise_if_set()
    return lk, L, batch, _ERRORS.flag(x.device, f'{what}(x {tuple(x.shape)}, {L} links)')


def link_gather(x, links):
    """float32 [L, 2, F], out[l, s] = x[links[l, s]]: the bits of x[links].  Differentiable in x: grad_x[n] = the chunked sum (module
    docstring) of g[l, s] over the slots (l, s) with links[l, s] == n, ascending in 2l + s; rows no link touches are zeros."""
    return _LinkGather.apply(x, *_prepare(x, links, 'link_gather'))


def link_hadamard(x, links):
    """float32 [L, F], out[l] = x[links[l, 0]] * x[links[l, 1]], one fp32 multiply: the bits of x[links[:, 0]] * x[links[:, 1]], and
    no [L, 2, F] tensor is made.  Differentiable in x: grad_x[n] = the chunked sum (module docstring) of fl(g[l] * x[links[l, 1 - s]])
    over the slots (l, s) with links[l, s] == n, ascending in 2l + s; a self link (n, n) contributes two terms."""
    return _LinkHadamard.apply(x, *_prepare(x, links, 'link_hadamard'))
