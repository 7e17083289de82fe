"""Host mirror of the reference's per-link heuristics (src/heuristics.py:10-113: CN, AA, RA, PPR) -- SURVEY 8(f)
row N4: `RA` is the other per-link precompute of HashDataset.__init__ (datasets/elph.py:76-77, negatives at :314).

Same call surface as the reference: `RA(A, edge_index, batch_size)` with A a scipy sparse adjacency matrix and
`edge_index` an int tensor of links [L, 2]; returns `(float32 scores [L], edge_index)`.  The three scores are one kernel
with a different column multiplier; the multiplier itself is computed on the host with the reference's own numpy expression,
so its values are identical.  The kernel follows scipy's arithmetic for the matrix's dtype: fp64 products and sum for int, bool
and float64 matrices (ss_common_neighbour_scores: CN of integer weights is exact, the rest within one float32 ulp), float32
products and numpy's float32 pairwise summation order for float32 matrices (ss_common_neighbour_scores_f32: bit-identical).
No CPU fallback: the kernels need a HIP device.

`common_neighbours(A, edge_index, weighting)` lists the nodes those sums run over, with their coefficients, and
`common_neighbour_features(A, edge_index, x, weighting)` pools the node features x over them, one [F] row per link
(ss_common_neighbour_count / _fill / _pool: csrc/ss_cn_pool.hip).

`PPR(A, edge_index)` keeps the reference's own return convention, which differs from the other three: the scores come in the
order of `torch.sort(edge_index[:, 0])` and the second value is that sorted link list as a [2, L] tensor.  The personalised
PageRank vectors of all distinct sources are computed in batches of S columns (ss_ppr_*: csrc/ss_ppr.hip);
`personalized_pagerank` is the layer underneath, returning the vectors themselves.
"""
import collections
import ctypes
import logging
import weakref

import numpy as np
import torch

from . import _native, knobs
from .hashing import _compute_device, _error_flag, _ptr, _stream, _take_error

logger = logging.getLogger(__name__)


class DeviceAdjacency(object):
    """scipy sparse matrix -> device CSR with sorted, duplicate-free rows (the canonical form scipy itself computes with)
    plus the values widened to fp64 (exact); built once per matrix object and reused by CN / AA / RA.  `dtype` (A's) picks
    the arithmetic of the scores: float32 matrices are scored in float32, as scipy does"""

    def __init__(self, A, device):
        A = A.tocsr()
        if not A.has_canonical_format:
            A = A.copy()
            A.sum_duplicates()  # also sorts the column ids of every row
        if A.shape[0] != A.shape[1]:
            raise ValueError('adjacency matrix must be square')
        self.num_nodes = A.shape[0]
        self.device = device
        self.rowptr = torch.from_numpy(A.indptr.astype(np.int64)).to(device)
        self.col = torch.from_numpy(A.indices.astype(np.int32) if A.nnz else np.zeros(1, dtype=np.int32)).to(device)
        unit = A.nnz == 0 or bool(np.all(A.data == 1))
        self.val = None if unit else torch.from_numpy(A.data.astype(np.float64)).to(device)
        # column sums exactly as the reference forms them (heuristics.py:38,59): np.matrix of the matrix's dtype
        self.colsum = np.asarray(A.sum(axis=0)).ravel()
        # no reference to A itself: _ADJ_CACHE drops this object when the caller's matrix dies (a weakref callback), which a
        # strong reference from here would prevent.  The PageRank operator is derived from the device CSR and A's dtype instead.
        self.nnz, self.dtype = A.nnz, A.data.dtype
        self._ppr = {}

    def multiplier(self, kind):
        if kind == 'CN':
            return None
        with np.errstate(divide='ignore', invalid='ignore'):
            mult = 1 / (np.log(self.colsum) if kind == 'AA' else self.colsum)
        mult = np.asarray(mult, dtype=np.float64)
        mult[np.isinf(mult)] = 0
        return torch.from_numpy(mult).to(self.device)

    def ppr_operator(self, p):
        """the device operator of pagerank_power(A, p) (fast_pagerank, called at heuristics.py:99), built once per p:
        the CSR of W^T's pull form -- row v lists the u with A[u, v] != 0 and r_u != 0, weight (p * A[u, v]) * (1 / r_u) --, z,
        and the rows with more than SS_PPR_SEGMENT entries cut into segments.  Every value comes from the reference's own numpy
        expressions on the matrix's dtype (r = A.sum(axis=1), 1 / r[k], p * A.T, z = ((1 - p)(r != 0) + (r == 0)) / n)."""
        key = float(p)
        if key not in self._ppr:
            self._ppr[key] = _PprOperator(self._host_csr(), key, self.device)
        return self._ppr[key]

    def _host_csr(self):
        """the canonical CSR back from the device, values in A's dtype again (exact: they were widened to fp64)"""
        import scipy.sparse as sp
        data = np.ones(self.nnz) if self.val is None else self.val.cpu().numpy()
        return sp.csr_matrix((data.astype(self.dtype), self.col[:self.nnz].cpu().numpy(), self.rowptr.cpu().numpy()),
                             shape=(self.num_nodes, self.num_nodes))


class _PprOperator(object):
    def __init__(self, A, p, device):
        n = A.shape[0]
        r = np.asarray(A.sum(axis=1)).reshape(-1)
        k = r.nonzero()[0]
        inv_k = 1 / r[k]
        inv = np.zeros(n, dtype=inv_k.dtype)
        inv[k] = inv_k
        self.z = ((1 - p) * (r != 0) + (r == 0)) / n
        AT = A.T.tocsr()  # row v = the in-edges (u, v) of v
        AT.sort_indices()
        u = AT.indices
        keep = r[u] != 0  # rows of A that sum to 0 have no entry in D^-1: their columns of W are empty
        w = ((p * AT.data) * inv[u]).astype(np.float64)
        deg = np.diff(AT.indptr)
        rows = np.repeat(np.arange(n), deg)[keep]
        deg = np.bincount(rows, minlength=n)
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(deg, out=indptr[1:])
        col, w = u[keep].astype(np.int32), w[keep]
        hubs = np.nonzero(deg > _native.PPR_SEGMENT)[0].astype(np.int32)
        nseg = (deg[hubs] + _native.PPR_SEGMENT - 1) // _native.PPR_SEGMENT
        hub_seg = np.zeros(len(hubs) + 1, dtype=np.int32)
        np.cumsum(nseg, out=hub_seg[1:])
        seg_hub = np.repeat(np.arange(len(hubs), dtype=np.int32), nseg)
        self.num_nodes, self.nnz, self.n_hubs, self.n_segments = n, len(col), len(hubs), int(hub_seg[-1])
        self.device = device

        def dev(a, dtype):  # never an empty device buffer: the C ABI gets a valid pointer for every array
            return torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1), dtype=dtype)).to(device)

        self.rowptr, self.col, self.w = dev(indptr, np.int64), dev(col, np.int32), dev(w, np.float64)
        self.zdev = dev(self.z, np.float64)
        self.hub_rows, self.hub_seg, self.seg_hub = dev(hubs, np.int32), dev(hub_seg, np.int32), dev(seg_hub, np.int32)
        self.struct = _native.PprGraphStruct(
            rowptr=self.rowptr.data_ptr(), col=self.col.data_ptr(), w=self.w.data_ptr(), z=self.zdev.data_ptr(), num_nodes=n,
            nnz=self.nnz, hub_rows=self.hub_rows.data_ptr(), hub_seg=self.hub_seg.data_ptr(), seg_hub=self.seg_hub.data_ptr(),
            n_hubs=self.n_hubs, n_segments=self.n_segments)

    def workspace_bytes(self, S):
        return _native.lib().ss_ppr_workspace_bytes(self.num_nodes, S, self.n_hubs, self.n_segments)

    def columns(self, n_sources):
        """S: the knob, capped by the sources there are and by half the free device memory"""
        S = max(1, min(int(knobs.PPR_COLUMNS), n_sources, _native.PPR_MAX_COLUMNS))
        free = torch.cuda.mem_get_info(self.device)[0]
        while S > 1 and self.workspace_bytes(S) > free // 2:
            S //= 2
        return S

    def run(self, sources, S, tol, max_iter, on_batch):
        """personalised PageRank of `sources` (device int64) in batches of S columns; on_batch(lo, count, workspace, nbytes)
        reads each batch's result before the next one overwrites it"""
        lib = _native.lib()
        nbytes = self.workspace_bytes(S)
        if nbytes == 0:
            raise ValueError(f'personalised PageRank does not support N = {self.num_nodes} with {S} columns')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        n_active = torch.zeros(1, dtype=torch.int32, device=self.device)
        g = ctypes.byref(self.struct)
        stream, err = _stream(self.device), _error_flag(self.device)
        every = max(int(knobs.PPR_CHECK_EVERY), 1)
        limit = max(int(max_iter), 1)  # the reference's loop steps once before it tests max_iter
        for lo in range(0, len(sources), S):
            cnt = min(S, len(sources) - lo)
            _native.check(lib.ss_ppr_begin(g, _ptr(sources[lo:lo + cnt]), cnt, float(tol), _ptr(ws), nbytes, _ptr(err), stream),
                          'ss_ppr_begin')
            k = 0
            while k < limit:
                for _ in range(min(every, limit - k)):
                    k += 1
                    _native.check(lib.ss_ppr_iterate(g, cnt, k, int(max_iter), float(tol), _ptr(ws), nbytes, stream), 'ss_ppr_iterate')
                _native.check(lib.ss_ppr_status(g, cnt, _ptr(ws), nbytes, None, _ptr(n_active), stream), 'ss_ppr_status')
                if int(n_active.item()) == 0:
                    break
            on_batch(lo, cnt, ws, nbytes)


_ADJ_CACHE = {}


def _adjacency(A, device):
    if isinstance(A, DeviceAdjacency):
        return A
    key = (id(A), str(device))
    hit = _ADJ_CACHE.get(key)
    if hit is not None and hit[0]() is A and hit[2] == (A.nnz, A.shape):
        return hit[1]
    adj = DeviceAdjacency(A, device)
    try:
        _ADJ_CACHE[key] = (weakref.ref(A, lambda _r, k=key: _ADJ_CACHE.pop(k, None)), adj, (A.nnz, A.shape))
    except TypeError:  # not weak-referenceable: do not cache
        pass
    return adj


class _PairCall(object):
    """The walk the three pair calls share after their own argument checks: the links' home and the compute device (`x` may name it,
    `out` must be on it), the device adjacency, the links there as contiguous int64, the library, the error flag and the stream."""

    def __init__(self, A, links, x=None, out=None):
        self.home = links.device
        self.device = _compute_device(links, x)
        if out is not None and out.device != self.device:
            raise ValueError(f'out must be on the compute device {self.device}, it is on {out.device}')
        self.adj = _adjacency(A, self.device)
        self.lk = links.to(device=self.device, dtype=torch.int64).contiguous()
        self.lib, self.err, self.stream = _native.lib(), _ptr(_error_flag(self.device)), _stream(self.device)

    def csr(self, mult):  # the head of every ss_common_neighbour_* call that takes values
        return _ptr(self.adj.rowptr), _ptr(self.adj.col), _ptr(self.adj.val), _ptr(mult), self.adj.num_nodes

    def launch(self, fn, *args, name=None):  # ... and its tail; `name`: what an error names
        _native.check(getattr(self.lib, fn)(*args, self.err, self.stream), name or fn)

    def batches(self, batch_size):  # the reference's DataLoader chunks (heuristics.py:18,41,62); results do not depend on them
        L, step = self.lk.size(0), max(int(batch_size), 1)
        return [(lo, min(lo + step, L)) for lo in range(0, L, step)]

    def finish(self, *results, stay=False):  # one synchronising read after the launches, then the results on the links' device
        if _take_error(self.device):
            raise IndexError(f'edge_index refers to nodes outside [0, {self.adj.num_nodes})')
        return [t if t is None or stay else t.to(self.home) for t in results]


def _scores(kind, A, edge_index, batch_size):
    links = torch.as_tensor(edge_index)
    if links.dim() != 2 or links.size(1) != 2:
        raise ValueError('edge_index must be a tensor of links with shape [num_links, 2]')
    call = _PairCall(A, links)
    mult = call.adj.multiplier(kind)
    out = torch.empty(call.lk.size(0), dtype=torch.float32, device=call.device)
    fn = 'ss_common_neighbour_scores_f32' if call.adj.dtype == np.float32 else 'ss_common_neighbour_scores'
    for lo, hi in call.batches(batch_size):
        call.launch(fn, *call.csr(mult), _ptr(call.lk[lo:hi]), hi - lo, _ptr(out[lo:hi]), name='ss_common_neighbour_scores')
    return call.finish(out)[0], edge_index


def CN(A, edge_index, batch_size=100000):
    """common neighbours (reference heuristics.py:10-27)"""
    scores, edge_index = _scores('CN', A, edge_index, batch_size)
    logger.info(f'evaluated Common Neighbours for {len(scores)} edges')
    return scores, edge_index


def AA(A, edge_index, batch_size=100000):
    """Adamic Adar (reference heuristics.py:30-48)"""
    scores, edge_index = _scores('AA', A, edge_index, batch_size)
    logger.info(f'evaluated Adamic Adar for {len(scores)} edges')
    return scores, edge_index


def RA(A, edge_index, batch_size=100000):
    """resource allocation (reference heuristics.py:51-70)"""
    scores, edge_index = _scores('RA', A, edge_index, batch_size)
    logger.info(f'evaluated Resource Allocation for {len(scores)} edges')
    return scores, edge_index


CommonNeighbours = collections.namedtuple('CommonNeighbours', 'rowptr ids coef')


def _num_nodes(A):
    return A.num_nodes if isinstance(A, DeviceAdjacency) else A.shape[0]


def _check_links(edge_index):
    links = torch.as_tensor(edge_index)
    if links.dim() != 2 or links.size(1) != 2 or links.dtype.is_floating_point or links.dtype.is_complex or links.dtype == torch.bool:
        raise ValueError('edge_index must be an int tensor of links with shape [num_links, 2]')
    return links


def _check_weighting(A, weighting, allow_none):
    """host-side checks of `weighting`: 'CN' | 'AA' | 'RA', a 1-D float tensor / array of length N, or (lists only) None"""
    if weighting is None:
        if not allow_none:
            raise ValueError("weighting=None is for common_neighbours only: pass 'CN' for unweighted pooling")
        return None
    if isinstance(weighting, str):
        if weighting not in ('CN', 'AA', 'RA'):
            raise ValueError(f"weighting must be 'CN', 'AA', 'RA' or a multiplier of length N, got {weighting!r}")
        return weighting
    w = torch.as_tensor(weighting)
    if w.dim() != 1 or not w.dtype.is_floating_point or w.numel() != _num_nodes(A):
        raise ValueError(f'a custom multiplier must be a 1-D float tensor or array of length N = {_num_nodes(A)}, '
                         f'got {w.dtype} {tuple(w.shape)}')
    return w


def _multiplier(adj, weighting):
    """(mult, with_coef): the device fp64 multiplier (None = 1) of a checked `weighting`"""
    if weighting is None:
        return None, False
    if isinstance(weighting, str):
        return adj.multiplier(weighting), True
    return weighting.detach().to(device=adj.device, dtype=torch.float64).contiguous(), True


def common_neighbours(A, edge_index, weighting=None):
    """The common neighbours of every link as a list: CommonNeighbours(rowptr int64 [L + 1], ids int64 [T], coef float32 [T] or None);
    link q's are ids[rowptr[q]:rowptr[q + 1]], ascending.  They are the columns STORED in both row u and row v of the canonical CSR of
    A (sorted, duplicate-free rows -- what CN / AA / RA sum over; an explicitly stored zero counts, and u or v itself is one when A
    says so).  coef[k] = float32(A[u, w] * (A[v, w] * mult[w])), evaluated in fp64 with this association and rounded once, for every
    matrix dtype (the scipy-float32 emulation of the scores is not repeated here).  `weighting`: None (no coef), 'CN' (mult = 1),
    'AA' / 'RA' (the multiplier of the scores), or a 1-D float tensor / array of length N (the caller's own, used as fp64).
    A, edge_index as CN takes them; CPU links in, CPU tensors out.  A count pass, a cumsum, one host read of T, a fill pass
    (ss_common_neighbour_count / _fill: csrc/ss_cn_pool.hip).  A link id outside [0, N) raises IndexError after the launches."""
    links = _check_links(edge_index)
    weighting = _check_weighting(A, weighting, allow_none=True)
    call = _PairCall(A, links)
    adj, lk, device = call.adj, call.lk, call.device
    mult, with_coef = _multiplier(adj, weighting)
    L = lk.size(0)
    rowptr = torch.zeros(L + 1, dtype=torch.int64, device=device)
    T = 0
    if L:
        counts = torch.empty(L, dtype=torch.int64, device=device)
        call.launch('ss_common_neighbour_count', _ptr(adj.rowptr), _ptr(adj.col), adj.num_nodes, _ptr(lk), L, _ptr(counts))
        torch.cumsum(counts, 0, out=rowptr[1:])
        T = int(rowptr[-1].item())
    ids = torch.empty(max(T, 1), dtype=torch.int64, device=device)  # (never an empty device buffer behind the C ABI)
    coef = torch.empty(max(T, 1), dtype=torch.float32, device=device) if with_coef else None
    if T:
        call.launch('ss_common_neighbour_fill', *call.csr(mult), _ptr(lk), L, _ptr(rowptr), _ptr(ids), _ptr(coef))
    return CommonNeighbours(*call.finish(rowptr, ids[:T], coef[:T] if with_coef else None))


def common_neighbour_features(A, edge_index, x, weighting='CN', batch_size=100000, out=None):
    """Node features pooled over every link's common neighbours: float32 [L, F] with
        out[q, :] = sum over the common neighbours w of link q, ASCENDING w, of c(q, w) * x[w, :]
    where the common neighbours and c(q, w) = float32(A[u, w] * (A[v, w] * mult[w])) are those of `common_neighbours` -- the device
    form of (A[src].multiply(A_[dst])) @ x without the [L, N] matrix, a BUDDY-style precompute for a fixed x (raw or SIGN features)
    stored beside subgraph_features and RA.  The sum is float32 from +0.0, product and sum rounded separately, each element
    accumulated by one lane in that order: a row has ONE value whatever batch_size, the order or repetition of the links, or which of
    the two rows is longer; a link without common neighbours gets +0.0.
    x: float32 [N, F] on the CPU or the device (anything else is a ValueError -- no silent cast; a non-contiguous x is made
    contiguous); any F >= 0.  weighting: 'CN', 'AA', 'RA' or a 1-D float multiplier of length N.  out: optional contiguous float32
    [L, F] on the compute device, filled and returned.  batch_size: links per launch.  Otherwise the result is on the links' device.
    Inference and precompute only: there is NO gradient with respect to x (it would be a float scatter-add), and NaN or Inf in x is
    outside the contract (0 * Inf of a stored zero is NaN).  The trainable form is cn_pool.common_neighbour_pool on a
    CommonNeighbourBatch: the same rows bit for bit up to 256 common neighbours, the chunked sum beyond.  A link id outside [0, N) gives a row of zeros and an IndexError after
    the launches (ss_common_neighbour_pool: csrc/ss_cn_pool.hip)."""
    links = _check_links(edge_index)
    weighting = _check_weighting(A, weighting, allow_none=False)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError('x must be a float32 tensor of shape [N, F]')
    N, F, L = _num_nodes(A), x.size(1), links.size(0)
    if x.size(0) != N:
        raise ValueError(f'x has {x.size(0)} rows, the adjacency matrix has N = {N}')
    if F >= 1 << 31:
        raise ValueError('F must be below 2^31')
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (L, F)
                            or not out.is_contiguous()):
        raise ValueError(f'out must be a contiguous float32 tensor of shape [{L}, {F}]')
    call = _PairCall(A, links, x, out)
    mult, _ = _multiplier(call.adj, weighting)
    xd = x.detach().to(call.device).contiguous()
    res = out if out is not None else torch.empty((L, F), dtype=torch.float32, device=call.device)
    for lo, hi in call.batches(batch_size):
        call.launch('ss_common_neighbour_pool', *call.csr(mult), _ptr(call.lk[lo:hi]), hi - lo, _ptr(xd), F, _ptr(res[lo:hi]))
    return call.finish(res, stay=out is not None)[0]  # (a caller's `out` stays on the compute device)


PprPlan = collections.namedtuple('PprPlan', 'edge_reindex sources link_col batches')


def ppr_plan(edge_index, columns):
    """the reference's link order (heuristics.py:84-86: torch.sort of the sources, default -- not stable -- on the tensor as
    given) and the batches: `sources` = the distinct sources in that order, source i in batch i // columns at column
    i % columns; `link_col` = the column of every sorted link's source; `batches` = (first source, sources, first link, links)"""
    links = torch.as_tensor(edge_index)
    if links.dim() != 2 or links.size(1) != 2:
        raise ValueError('edge_index must be a tensor of links with shape [num_links, 2]')
    src_index, sort_indices = torch.sort(links[:, 0])
    dst_index = links[sort_indices, 1]
    edge_reindex = torch.stack([src_index, dst_index])
    sources, counts = torch.unique_consecutive(src_index, return_counts=True)
    S = max(int(columns), 1)
    col = torch.arange(len(sources), device=links.device) % S
    link_col = torch.repeat_interleave(col, counts).to(torch.int32)
    ends = torch.cumsum(counts, 0).tolist()
    batches = []
    for lo in range(0, len(sources), S):
        hi = min(lo + S, len(sources))
        first = ends[lo - 1] if lo else 0
        batches.append((lo, hi - lo, first, ends[hi - 1] - first))
    return PprPlan(edge_reindex, sources, link_col, batches)


def personalized_pagerank(A, sources, p=0.85, tol=1e-7, max_iter=100):
    """fast_pagerank.pagerank_power(A, p, personalize=e_s, tol, max_iter) for every s in `sources` (the call the reference makes per
    source, heuristics.py:99): returns (fp64 [len(sources), N] normalised vectors, int32 [len(sources)] iterations taken), on the
    device of `sources` (CPU in, CPU out)"""
    src = torch.as_tensor(sources, dtype=torch.int64).reshape(-1)
    home = src.device
    device = _compute_device(src)
    adj = _adjacency(A, device)
    op = adj.ppr_operator(p)
    K = len(src)
    out = torch.empty((K, adj.num_nodes), dtype=torch.float64, device=device)
    iters = torch.zeros(K, dtype=torch.int32, device=device)
    if K == 0:
        return out.to(home), iters.to(home)
    src_dev = src.to(device).contiguous()
    lib = _native.lib()
    g = ctypes.byref(op.struct)

    def take(lo, cnt, ws, nbytes):
        stream = _stream(device)
        _native.check(lib.ss_ppr_vectors(g, cnt, _ptr(ws), nbytes, _ptr(out[lo:lo + cnt]), stream), 'ss_ppr_vectors')
        _native.check(lib.ss_ppr_status(g, cnt, _ptr(ws), nbytes, _ptr(iters[lo:lo + cnt]), None, stream), 'ss_ppr_status')

    op.run(src_dev, op.columns(K), tol, max_iter, take)
    if _take_error(device):
        raise IndexError(f'sources outside [0, {adj.num_nodes})')
    return out.to(home), iters.to(home)


def PPR(A, edge_index, p=0.85, tol=1e-7, max_iter=100):
    """personalised PageRank (reference heuristics.py:74-113) with the reference's call and return convention: returns
    (float32 scores, edge_reindex) where edge_reindex = [2, L] links sorted by source and the scores follow that order"""
    links = torch.as_tensor(edge_index)
    if links.dim() != 2 or links.size(1) != 2:
        raise ValueError('edge_index must be a tensor of links with shape [num_links, 2]')
    home = links.device
    L = links.size(0)
    if L == 0:
        return torch.zeros(0, dtype=torch.float32, device=home), torch.stack([links[:, 0], links[:, 1]])
    device = _compute_device(links)
    adj = _adjacency(A, device)
    op = adj.ppr_operator(p)
    n_sources = len(torch.unique(links[:, 0]))
    S = op.columns(n_sources)
    plan = ppr_plan(links, S)
    srcs = plan.sources.to(device=device, dtype=torch.int64).contiguous()
    dst = plan.edge_reindex[1].to(device=device, dtype=torch.int64).contiguous()
    link_col = plan.link_col.to(device).contiguous()
    out = torch.empty(L, dtype=torch.float32, device=device)
    lib = _native.lib()
    g = ctypes.byref(op.struct)
    batch_links = {lo: (first, count) for lo, _, first, count in plan.batches}

    def score(lo, cnt, ws, nbytes):
        first, count = batch_links[lo]
        _native.check(lib.ss_ppr_scores(g, cnt, _ptr(dst[first:first + count]), _ptr(link_col[first:first + count]), count, _ptr(ws),
                                        nbytes, _ptr(out[first:first + count]), _ptr(_error_flag(device)), _stream(device)),
                      'ss_ppr_scores')

    op.run(srcs, S, tol, max_iter, score)
    if _take_error(device):
        raise IndexError(f'edge_index refers to nodes outside [0, {adj.num_nodes})')
    logger.info(f'evaluated PPR for {L} edges')
    return out.to(home), plan.edge_reindex
