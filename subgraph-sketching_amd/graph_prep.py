"""The edge-list preparation every dataset constructor of the reference begins with, on the device: coalesce, to_undirected,
coalesce_graph and is_undirected.  Kernels: csrc/ss_coalesce.hip; design: DESIGN 3.26; numpy restatement: tests/graph_prep_restatement.py.

The reference calls torch_sparse.coalesce (src/datasets/elph.py:54-66, src/datasets/seal.py:58-60, 111-113) and PyG's
to_undirected(..., reduce='add') (src/datasets/elph.py:54-66 for directed data, src/data.py:137, 174).  Neither package is in this image,
so their semantics are RESTATED here: coalesce sorts the entries by (row, col) and merges equal pairs with `op`; to_undirected
concatenates the list as given with the list reversed, doubles the attributes, and coalesces -- a pair present in both directions gets
the sum on both arcs, a self loop (u, u) meets its own copy (2 w under 'add').

The contract: accumulation order.  A RUN is the entries of one (row, col) pair in the order of the input list (for to_undirected: of the
concatenated list).
  add   the run is cut into chunks of 256 entries from its start; every chunk is summed sequentially in list order starting from its
        first entry, and the chunk sums are added in chunk order.  A run of at most 256 entries is the plain sequential loop.  The rule of
        ss_aggr.hip and ss_link_decoder.hip, for the same reason: a value's bits depend on its own run alone -- not on the tier, on
        long_entries, on the other edges or on the order of other runs -- and a call repeats bit for bit.  int64 sums wrap.
  mean  the add sum divided by the count in the value's dtype; int64: floor division, as PyG's scatter does.
  min / max  the canonical quiet NaN if any entry is NaN, otherwise the extreme; of -0.0 and +0.0 the one listed first wins.
There are no float atomics anywhere, and row and col are never multiplied together (no n^2 key to overflow).

Launches: the positions sorted by (row, col, position) come from two stable groupings of what exists (sign.group_ids_stable: by col, then
by row of the result), then mark / cumsum / fill / reduce / reduce_long of ss_coalesce.hip.  One host read per call: the output size E',
which carries the error flags along.

Conventions, as _plans.check_edge_list: an int64 [2, E] edge_index, 1 <= N < 2^31, E (after doubling) < 2^31.  Ids outside [0, N) raise
IndexError -- negative ids are refused, not wrapped.  CPU tensors are moved to the compute device and the results come back on the
caller's device, as sign.spmm does.  E = 0 works.  No CPU fallback.
"""
import torch

from . import _native
from ._plans import check_edge_list
from ._runtime import CsrProtocolFault, _Span, _compute_device, _ptr, _stream, mark_csr_protocol_faults_reported
from .sign import group_ids_stable

OPS = {'add': 0, 'mean': 1, 'min': 2, 'max': 3}                        # the op codes of ss_coalesce_reduce (include/subgraph_sketch.h)
DTYPES = {torch.int64: 0, torch.float32: 1, torch.float64: 2}          # its dtype codes
_LIMIT = 1 << 31


def _check_list(num_nodes, edge_index, doubled):
    """-> (N, E of the list as given); ValueError for a list the kernels do not take"""
    N, E = check_edge_list(num_nodes, edge_index, None)
    if E * (2 if doubled else 1) >= _LIMIT:
        raise ValueError(f'edge_index holds {E} edges{" (doubled by to_undirected)" if doubled else ""}: positions are 32-bit, fewer than 2^31')
    return N, E


def _check_value(value, E, what):
    """-> (value flattened to [E] or None, its shape); ValueError for a width, dtype or length the kernels do not take"""
    if value is None:
        return None, None
    if not isinstance(value, torch.Tensor) or value.dim() not in (1, 2) or value.size(0) != E or (value.dim() == 2 and value.size(1) != 1):
        raise ValueError(f'{what} must be a tensor [E] or [E, 1] with E = {E} (multi-column attributes are out of scope)')
    if value.dtype not in DTYPES:
        raise ValueError(f'{what} must be int64, float32 or float64, got {value.dtype}')
    if value.requires_grad:
        raise ValueError(f'{what} is not differentiable here: pass {what}.detach()')
    return value.reshape(E), tuple(value.shape)


def _check_op(op, what):
    if op not in OPS:
        raise ValueError(f"{what} must be one of 'add', 'mean', 'min', 'max', got {op!r} ('mul' is out of scope)")
    return OPS[op]


def _check_long_entries(long_entries):
    if not isinstance(long_entries, int) or isinstance(long_entries, bool) or not 1 <= long_entries < _LIMIT:
        raise ValueError(f'long_entries must be an integer in [1, 2^31), got {long_entries!r}')
    return long_entries


def sorted_positions(row, col, N, err):
    """int32 [E]: the positions of the list sorted by (row, col, position) -- two stable groupings, least significant key first.
    err: device int32 word the groupings report into (see ss_csr_group_ids)."""
    _, oc = group_ids_stable(col, N, err)
    _, o2 = group_ids_stable(torch.index_select(row, 0, oc), N, err)
    return torch.index_select(oc, 0, o2)


class _Merged(object):
    """what one merge leaves on the compute device"""

    def __init__(self, N, device, edge_index, value, count, rowptr, info):
        self.N, self.device, self.edge_index, self.value, self.count, self.rowptr, self.info = N, device, edge_index, value, count, rowptr, info


def _merge(N, ei, value, op, long_entries, device):
    """ei: int64 [2, E] contiguous on `device` (the list, doubled already for to_undirected); value: [n_values] on `device` or None,
    n_values == E or E / 2 (list position p reads value[p mod n_values]) -> _Merged"""
    lib = _native.lib()
    E = ei.size(1)
    info = torch.zeros(2, dtype=torch.int32, device=device)  # {long runs, longest run}
    if E == 0:
        return _Merged(N, device, torch.empty((2, 0), dtype=torch.int64, device=device),
                       None if value is None else torch.empty(0, dtype=value.dtype, device=device),
                       torch.empty(0, dtype=torch.int32, device=device), torch.zeros(N + 1, dtype=torch.int64, device=device), info)
    row, col = ei[0], ei[1]
    flags = torch.zeros(2, dtype=torch.int32, device=device)  # {the groupings' word (bit 1: a given-up wait), the mark pass's}
    stream = _stream(device)
    with _Span('coalesce_sort', device):
        perm = sorted_positions(row, col, N, flags[0:1])
    BLOCK = lib.ss_coalesce_block()
    heads = torch.empty((E + BLOCK - 1) // BLOCK, dtype=torch.int32, device=device)
    with _Span('coalesce_merge', device):
        _native.check(lib.ss_coalesce_mark(_ptr(row), _ptr(col), _ptr(perm), E, N, _ptr(heads), _ptr(flags[1:2]), stream), 'ss_coalesce_mark')
        incl = torch.cumsum(heads, 0, dtype=torch.int64)
        n_runs, grouping, marked = torch.cat([incl[-1:], flags.to(torch.int64)]).tolist()  # the one host read of the call
        if grouping & _native.SS_CSR_ERR_PROTOCOL:
            mark_csr_protocol_faults_reported()
            raise CsrProtocolFault('a grouping of this coalesce gave up a cross-workgroup wait after its time bound: nothing is returned')
        if grouping or marked:
            raise IndexError(f'edge_index refers to nodes outside [0, {N}) (negative ids are not wrapped)')
        out = torch.empty((2, n_runs), dtype=torch.int64, device=device)
        run_start = torch.empty(n_runs + 1, dtype=torch.int32, device=device)
        rowptr = torch.empty(N + 1, dtype=torch.int64, device=device)
        _native.check(lib.ss_coalesce_fill(_ptr(row), _ptr(col), _ptr(perm), E, N, _ptr(incl), n_runs, _ptr(out[0]), _ptr(out[1]), _ptr(run_start),
                                           _ptr(rowptr), stream), 'ss_coalesce_fill')
        count = torch.empty(n_runs, dtype=torch.int32, device=device)
        merged = None
        if value is None:
            _native.check(lib.ss_coalesce_reduce(_ptr(perm), _ptr(run_start), n_runs, None, 0, 0, 0, long_entries, None, _ptr(count), None, 0,
                                                 _ptr(info), stream), 'ss_coalesce_reduce')
        else:
            dtype, n_values = DTYPES[value.dtype], value.numel()
            merged = torch.empty(n_runs, dtype=value.dtype, device=device)
            max_long = E // long_entries + 1  # (a listed run has more than long_entries entries)
            long_runs = torch.empty(max_long, dtype=torch.int32, device=device)
            _native.check(lib.ss_coalesce_reduce(_ptr(perm), _ptr(run_start), n_runs, _ptr(value), n_values, dtype, op, long_entries, _ptr(merged),
                                                 _ptr(count), _ptr(long_runs), max_long, _ptr(info), stream), 'ss_coalesce_reduce')
            _native.check(lib.ss_coalesce_reduce_long(_ptr(perm), _ptr(run_start), n_runs, _ptr(value), n_values, dtype, op, _ptr(merged),
                                                      _ptr(long_runs), _ptr(info), max_long, stream), 'ss_coalesce_reduce_long')
    return _Merged(N, device, out, merged, count, rowptr, info)


def _device_list(edge_index, value, device, symmetrize):
    """the list and its values on the compute device; symmetrize: the list followed by the list reversed (the values are NOT doubled:
    the kernels read value[p mod E])"""
    ei = edge_index.detach().to(device)
    ei = torch.cat([ei, ei.flip(0)], dim=1) if symmetrize else ei.contiguous()
    return ei, None if value is None else value.detach().to(device).contiguous()


class CoalescedGraph(object):
    """a merged edge list, as coalesce_graph returns it.

    edge_index   int64 [2, E']: the pairs sorted by (row, col), every pair once
    edge_weight  [E'] in the dtype given (None without weights): `reduce` over every pair's entries, in list order under the chunk rule
    count        int32 [E']: how many entries of the list every pair merged
    rowptr       int64 [N + 1]: where the pairs of every row edge_index[0] start
    num_nodes    N"""

    def __init__(self, merged, home):
        self._merged, self.num_nodes = merged, merged.N
        self.edge_index, self.count, self.rowptr = merged.edge_index.to(home), merged.count.to(home), merged.rowptr.to(home)
        self.edge_weight = None if merged.value is None else merged.value.to(home)
        self.num_edges = int(merged.count.numel())

    def info(self):
        """{'runs': E', 'long_runs': the runs the wavefront tier reduced, 'longest_run': the most entries one pair merged} (a host read)"""
        n_long, longest = self._merged.info.tolist()
        return {'runs': self.num_edges, 'long_runs': n_long, 'longest_run': longest}

    def to_scipy(self):
        """scipy.sparse.csr_matrix [N, N] in canonical format (sorted, duplicate-free: heuristics.DeviceAdjacency takes it as it is);
        the data are edge_weight, without weights the counts"""
        import scipy.sparse as ssp
        data = self.count if self.edge_weight is None else self.edge_weight
        A = ssp.csr_matrix((data.cpu().numpy(), self.edge_index[1].cpu().numpy(), self.rowptr.cpu().numpy()), shape=(self.num_nodes, self.num_nodes))
        A.has_canonical_format = True  # (by construction: no pass over the entries to find out)
        return A

    def is_symmetric(self, weights=True):
        """whether every pair (u, v) has its pair (v, u) -- with weights=True (and weights present) of the same weight, NaN equal to
        NaN.  Computed on the device; one host read."""
        m = self._merged
        if self.num_edges == 0:
            return True
        value = m.value if weights else None
        word = torch.empty(1, dtype=torch.int32, device=m.device)
        with _Span('coalesce_symmetric', m.device):
            _native.check(_native.lib().ss_coalesce_symmetric(_ptr(m.rowptr), _ptr(m.edge_index[0]), _ptr(m.edge_index[1]), self.num_edges, m.N,
                                                              _ptr(value), DTYPES[value.dtype] if value is not None else 0, _ptr(word),
                                                              _stream(m.device)), 'ss_coalesce_symmetric')
        return not int(word.item())


def coalesce_graph(num_nodes, edge_index, edge_weight=None, reduce='add', symmetrize=False, long_entries=256, return_info=False):
    """the merged edge list of a graph: a CoalescedGraph (with return_info: the pair (graph, graph.info())).
    @param num_nodes: N, 1 <= N < 2^31
    @param edge_index: int64 [2, E]; ids outside [0, N) raise IndexError
    @param edge_weight: None, or int64 / float32 / float64 [E] or [E, 1] (returned as [E'])
    @param reduce: 'add', 'mean', 'min' or 'max'
    @param symmetrize: merge the list followed by its reverse (to_undirected)
    @param long_entries: runs of more entries go to the wavefront tier; the results do not depend on it"""
    N, E = _check_list(num_nodes, edge_index, symmetrize)
    value, _ = _check_value(edge_weight, E, 'edge_weight')
    op = _check_op(reduce, 'reduce')
    long_entries = _check_long_entries(long_entries)
    device = _compute_device(edge_index, edge_weight)
    ei, value = _device_list(edge_index, value, device, symmetrize)
    graph = CoalescedGraph(_merge(N, ei, value, op, long_entries, device), edge_index.device)
    return (graph, graph.info()) if return_info else graph


def coalesce(index, value, m, n, op='add'):
    """torch_sparse.coalesce(index, value, m, n, op): (index int64 [2, E'] sorted by (row, col), every pair once; value merged with `op`,
    its dtype and trailing shape kept, None for None).  Square shapes only (the reference passes num_nodes for both)."""
    if m != n:
        raise ValueError(f'square shapes only (the reference passes num_nodes for both), got m = {m}, n = {n}')
    N, E = _check_list(m, index, False)
    flat, shape = _check_value(value, E, 'value')
    code = _check_op(op, 'op')
    device = _compute_device(index, value)
    ei, flat = _device_list(index, flat, device, False)
    merged = _merge(N, ei, flat, code, 256, device)
    out_value = None if value is None else merged.value.reshape((-1,) + shape[1:]).to(value.device)
    return merged.edge_index.to(index.device), out_value


def _nodes_of(edge_index, num_nodes):
    if num_nodes is not None:
        return num_nodes
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2:
        raise ValueError('edge_index must be an int64 tensor [2, E]')
    return int(edge_index.max()) + 1 if edge_index.numel() else 1  # (one host read)


def to_undirected(edge_index, edge_attr=None, num_nodes=None, reduce='add'):
    """torch_geometric.utils.to_undirected(edge_index, edge_attr, num_nodes, reduce) for one attribute column: both directions
    concatenated (the list, then the list reversed), the attributes doubled, the result coalesced.  Returns edge_index alone when
    edge_attr is None, else (edge_index, edge_attr).  num_nodes=None: max + 1 (one more host read)."""
    N, E = _check_list(_nodes_of(edge_index, num_nodes), edge_index, True)
    flat, shape = _check_value(edge_attr, E, 'edge_attr')
    code = _check_op(reduce, 'reduce')
    device = _compute_device(edge_index, edge_attr)
    ei, flat = _device_list(edge_index, flat, device, True)
    merged = _merge(N, ei, flat, code, 256, device)
    out = merged.edge_index.to(edge_index.device)
    if edge_attr is None:
        return out
    return out, merged.value.reshape((-1,) + shape[1:]).to(edge_attr.device)


def is_undirected(edge_index, edge_attr=None, num_nodes=None):
    """whether the merged ('add') graph has, for every pair (u, v), the pair (v, u) with the same attribute:
    coalesce_graph(...).is_symmetric()"""
    return coalesce_graph(_nodes_of(edge_index, num_nodes), edge_index, edge_attr).is_symmetric()
