"""Graph readouts over a disjoint-union batch of subgraphs (csrc/ss_pool.hip): what every SEAL model of the reference ends its
message passing with (reference models/seal.py: global_sort_pool :245 in SEALDGCNN, global_add_pool / global_mean_pool in SEALMLP,
SEALGCN and SEALGIN, centre pooling x[src] * x[dst] :88-95 in SEALGCN / SEALSAGE).

PyG is absent from this image, so its semantics are RESTATED (as in sign.py and gcn.py; tests/pooling_restatement.py is the numpy form):
  global_add_pool   out[q] = sum of x[t] over the nodes of graph q; here in ascending t by one lane: the sequential fp32 loop bit for bit
  global_mean_pool  that sum, then ONE division by float(max(n, 1)) (PyG: scatter-mean's sum / count.clamp(min=1))
  global_sort_pool  per graph the nodes ordered by the LAST channel, descending, cut or zero-padded to k rows, flattened to [k * F].
                    PyG leaves ties to torch.sort; here the order is total: NaN first (as torch.sort(descending=True) has it), -0.0 ties
                    with +0.0, ties by ascending node position -- an integer key, so the result cannot depend on the algorithm.
  center_pool       x[root_u] * x[root_v] per link.  The reference finds the roots with np.unique(batch.cpu().numpy(), return_index=True)
                    and ASSUMES them at local indices 0 and 1; exact_subgraphs' rows ascend by id, so here they are read from
                    subgraphs.roots on the device.
All four are torch.autograd.Functions, differentiable in x, forward and backward in HIP, without float atomics: two runs give the
same bits.  x is float32 [T, F] on the GPU: there is no CPU fallback and no silent copy.

Graphs are given as `batch` -- an ExactSubgraphs / SampledSubgraphs (its rowptr is used) or PyG's non-decreasing int64 [T] vector --
or as rowptr= int64 [L + 1].  For a vector, rowptr comes from torch.searchsorted on the device; without size= ONE host read gives the
number of graphs together with the monotonicity check (a decreasing batch raises ValueError); with size= nothing is read and the
order is the caller's promise.

A rowptr or roots entry that points outside x is not followed by the kernels; it is reported late, like the engine's deferred
bounds errors: by the next call into this module or by check_errors(), as IndexError.
"""
import math

import torch

from . import _native
from ._runtime import _DeferredErrors, _ptr, _stream
from .subgraphs import ExactSubgraphs

SORT_CAPACITY = 1024  # C = ss_pool_sort_capacity(): the rows the on-chip sort of the select kernel holds; k <= C

_ERRORS = _DeferredErrors()


def _raise_if_set(synchronize=False):
    calls = ', '.join(_ERRORS._calls)
    try:
        _ERRORS.raise_if_set(synchronize=synchronize)
    except IndexError:
        raise IndexError(f'an earlier readout was given a rowptr or roots entry that points outside x (reported late); the places of '
                         f'such a graph were not computed. Calls since the last clean check: {calls}') from None


def check_errors():
    """waits for the device, then raises IndexError if a readout since the last check met a rowptr / perm / roots entry out of range"""
    _raise_if_set(synchronize=True)


def rowptr_from_batch(batch, size=None):
    """int64 [L + 1] offsets of PyG's node-to-graph vector (int64 [T], non-decreasing, ids >= 0), on its device.  size=None: L =
    batch[-1] + 1, read from the device together with the monotonicity flag (ONE host read; ValueError for a decreasing vector).
    size=L: no host read, no check; graphs past the last id are empty."""
    if not isinstance(batch, torch.Tensor) or batch.dtype != torch.int64 or batch.dim() != 1:
        raise ValueError('batch must be an int64 tensor [T] (or an ExactSubgraphs)')
    if size is None:
        L = 0
        if batch.numel():
            decreasing = (batch[1:] < batch[:-1]).any() | (batch[0] < 0)
            last, bad = torch.stack([batch[-1], decreasing.to(torch.int64)]).tolist()  # the one host read
            if bad:
                raise ValueError('batch must be non-decreasing and non-negative (PyG: the nodes of a graph are consecutive)')
            L = last + 1
    else:
        L = int(size)
        if L < 0:
            raise ValueError(f'size must be >= 0, got {size}')
    return torch.searchsorted(batch, torch.arange(L + 1, dtype=torch.int64, device=batch.device))


def _check_x(x):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError('x must be a float32 tensor [T, F]')
    if not x.is_cuda:
        raise ValueError('x must be on the GPU: there is no CPU fallback and no silent copy')


def _graphs(x, batch, rowptr, size):
    """-> rowptr int64 [L + 1] on x.device"""
    if (batch is None) == (rowptr is None):
        raise ValueError('give either batch (an ExactSubgraphs or an int64 [T] vector) or rowptr=, not both and not neither')
    _check_x(x)
    if isinstance(batch, ExactSubgraphs):
        if size is not None and int(size) != batch.num_links:
            raise ValueError(f'size={size} but the batch holds {batch.num_links} subgraphs')
        rowptr = batch.rowptr
    elif batch is not None:
        if not isinstance(batch, torch.Tensor) or batch.shape != (x.size(0),):
            raise ValueError(f'batch must be an int64 tensor [{x.size(0)}] (or an ExactSubgraphs)')
        if batch.device != x.device:
            raise ValueError(f'batch is on {batch.device}, x on {x.device}')
        return rowptr_from_batch(batch, size)
    if not isinstance(rowptr, torch.Tensor) or rowptr.dtype != torch.int64 or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError('rowptr must be an int64 tensor [L + 1]')
    if size is not None and int(size) != rowptr.numel() - 1:
        raise ValueError(f'size={size} but rowptr describes {rowptr.numel() - 1} graphs')
    if rowptr.device != x.device:
        raise ValueError(f'rowptr is on {rowptr.device}, x on {x.device}: there is no silent copy')
    return rowptr.contiguous()


def _flag(x, what):
    _raise_if_set()
    return _ERRORS.flag(x.device, f'{what}(x {tuple(x.shape)})')


class _SegmentPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rowptr, mean, err):
        x = x.contiguous()
        (T, F), L = x.shape, rowptr.numel() - 1
        ctx.rowptr, ctx.mean, ctx.shape = rowptr, mean, (T, F)
        out = torch.zeros((L, F), dtype=torch.float32, device=x.device)  # (small beside x; a refused graph's row stays 0)
        if L:
            _native.check(_native.lib().ss_segment_pool(_ptr(rowptr), L, _ptr(x), T, F, mean, _ptr(out), _ptr(err), _stream(x.device)),
                          'ss_segment_pool')
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        (T, F), L = ctx.shape, ctx.rowptr.numel() - 1
        grad = torch.empty((T, F), dtype=torch.float32, device=g.device)
        _native.check(_native.lib().ss_segment_pool_grad(_ptr(ctx.rowptr), L, _ptr(g), T, F, ctx.mean, _ptr(grad), _stream(g.device)),
                      'ss_segment_pool_grad')
        return grad, None, None, None


class _SortPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rowptr, k, err):
        x = x.contiguous()
        (T, F), L = x.shape, rowptr.numel() - 1
        lib, stream = _native.lib(), _stream(x.device)
        perm = torch.empty((L, k), dtype=torch.int32, device=x.device)
        out = torch.empty((L, k * F), dtype=torch.float32, device=x.device)
        if L:
            keys = x if F else torch.zeros((T, 1), dtype=torch.float32, device=x.device)  # (no channel: every key ties, positions decide)
            _native.check(lib.ss_pool_select(_ptr(rowptr), L, _ptr(keys), T, max(F, 1), k, _ptr(perm), _ptr(err), stream), 'ss_pool_select')
            _native.check(lib.ss_pool_gather(_ptr(rowptr), L, _ptr(perm), k, _ptr(x), T, F, _ptr(out), _ptr(err), stream), 'ss_pool_gather')
        ctx.rowptr, ctx.perm, ctx.k, ctx.shape, ctx.err = rowptr, perm, k, (T, F), err
        ctx.mark_non_differentiable(perm)
        return out, perm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        g = g.contiguous()
        (T, F), L = ctx.shape, ctx.rowptr.numel() - 1
        if L == 0:
            return torch.zeros((T, F), dtype=torch.float32, device=g.device), None, None, None
        grad = torch.empty((T, F), dtype=torch.float32, device=g.device)
        _native.check(_native.lib().ss_pool_scatter(_ptr(ctx.rowptr), L, _ptr(ctx.perm), ctx.k, _ptr(g), T, F, _ptr(grad), _ptr(ctx.err),
                                                    _stream(g.device)), 'ss_pool_scatter')
        return grad, None, None, None


class _CenterPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rowptr, roots, err):
        x = x.contiguous()
        (T, F), L = x.shape, rowptr.numel() - 1
        out = torch.zeros((L, F), dtype=torch.float32, device=x.device)  # (a refused link's row stays 0)
        if L:
            _native.check(_native.lib().ss_center_pool(_ptr(rowptr), L, _ptr(roots), _ptr(x), T, F, _ptr(out), _ptr(err), _stream(x.device)),
                          'ss_center_pool')
        ctx.save_for_backward(x)
        ctx.rowptr, ctx.roots, ctx.err = rowptr, roots, err
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,), g = ctx.saved_tensors, g.contiguous()
        (T, F), L = x.shape, ctx.rowptr.numel() - 1
        if L == 0:
            return torch.zeros_like(x), None, None, None
        grad = torch.empty_like(x)
        _native.check(_native.lib().ss_center_pool_grad(_ptr(ctx.rowptr), L, _ptr(ctx.roots), _ptr(x), _ptr(g), T, F, _ptr(grad), _ptr(ctx.err),
                                                        _stream(g.device)), 'ss_center_pool_grad')
        return grad, None, None, None


def global_add_pool(x, batch=None, *, rowptr=None, size=None):
    """torch_geometric.nn.global_add_pool [PyG semantics restated]: float32 [L, F], out[q] = the fp32 sum of x[t] over graph q in
    ascending t (one lane per element: the sequential loop, bit for bit); an empty graph gives 0.  Backward: grad_x[t] = g[q(t)]."""
    rowptr = _graphs(x, batch, rowptr, size)
    return _SegmentPool.apply(x, rowptr, 0, _flag(x, 'global_add_pool'))


def global_mean_pool(x, batch=None, *, rowptr=None, size=None):
    """torch_geometric.nn.global_mean_pool [PyG semantics restated]: global_add_pool's sum, then ONE division by float(max(n, 1)).
    Backward: grad_x[t] = g[q(t)] / float(max(n, 1))."""
    rowptr = _graphs(x, batch, rowptr, size)
    return _SegmentPool.apply(x, rowptr, 1, _flag(x, 'global_mean_pool'))


def global_sort_pool(x, batch=None, k=None, *, rowptr=None, size=None, return_perm=False):
    """torch_geometric.nn.global_sort_pool [PyG semantics restated]: float32 [L, k * F]; per graph the nodes ordered by the LAST
    channel descending -- NaN first, -0.0 == +0.0, ties by ascending node position -- and the first k of them laid side by side:
    out[q, j * F : (j + 1) * F] = x[rowptr[q] + perm[q, j]]; for j >= n the slot is zero and perm[q, j] = -1.  k in [1, C], C =
    pooling.SORT_CAPACITY.  return_perm: also perm int32 [L, k].  Backward: grad_x[rowptr[q] + perm[q, j]] = g[q, j * F : (j + 1) * F],
    zero elsewhere (a node is selected at most once: no atomics)."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= SORT_CAPACITY:
        raise ValueError(f'k must be an integer in [1, {SORT_CAPACITY}] (the sort capacity C = {SORT_CAPACITY}), got {k!r}')
    rowptr = _graphs(x, batch, rowptr, size)
    out, perm = _SortPool.apply(x, rowptr, k, _flag(x, 'global_sort_pool'))
    return (out, perm) if return_perm else out


def center_pool(x, subgraphs):
    """SEAL's centre pooling (reference models/seal.py:88-95): float32 [L, F], out[q] = x[rowptr[q] + roots[q, 0]] * x[rowptr[q] +
    roots[q, 1]] with the roots of subgraphs.roots read on the device (they are NOT at local indices 0 and 1 here: rows ascend by id);
    a row emptied by max_nodes (roots (-1, -1)) gives zeros.  Backward: grad_x[a] = g * x[b], grad_x[b] = g * x[a], their sum for a
    self link a == b, zero elsewhere."""
    if not isinstance(subgraphs, ExactSubgraphs):
        raise ValueError('subgraphs must be an ExactSubgraphs / SampledSubgraphs (its rowptr and roots are read)')
    _check_x(x)
    rowptr, roots = subgraphs.rowptr, subgraphs.roots
    L = subgraphs.num_links
    if not isinstance(roots, torch.Tensor) or roots.dtype != torch.int32 or roots.shape != (L, 2):
        raise ValueError(f'subgraphs.roots must be an int32 tensor [{L}, 2]')
    if rowptr.device != x.device or roots.device != x.device:
        raise ValueError(f'the subgraphs are on {rowptr.device}, x on {x.device}: there is no silent copy')
    return _CenterPool.apply(x, rowptr.contiguous(), roots.contiguous(), _flag(x, 'center_pool'))


def sort_pool_k(subgraphs_or_rowptr, ratio=0.6, minimum=10):
    """SEALDGCNN's k (reference models/seal.py:186-197): ratio > 1 is k itself; otherwise the ratio-percentile of the graphs' node
    counts, sorted[ceil(ratio * L) - 1], and at least `minimum`; 30 without graphs.  Host arithmetic on one copy of rowptr."""
    if ratio > 1:
        return int(ratio)
    rowptr = subgraphs_or_rowptr.rowptr if isinstance(subgraphs_or_rowptr, ExactSubgraphs) else subgraphs_or_rowptr
    rowptr = torch.as_tensor(rowptr)
    sizes = sorted((rowptr[1:] - rowptr[:-1]).tolist())
    if not sizes:
        return 30
    return int(max(minimum, sizes[int(math.ceil(ratio * len(sizes))) - 1]))
