"""Connected components of an edge_index and the induced subgraph of a node set, on the device: connected_components,
induced_subgraph and largest_component_subgraph.  Kernels: csrc/ss_components.hip; design: DESIGN 3.20; numpy / scipy restatement:
tests/components_restatement.py.

The reference takes the largest connected component of every non-OGB dataset before anything else (data.use_lcc, src/data.py:102-103,
241-260, on src/lcc.py): a Python set walk that scans the whole `row` array once per visited node, then a list comprehension that tests
`i in lcc` against a numpy array for every edge -- O(N E) interpreter work, minutes at PubMed size.  Here the components are one
streaming pass over the edges (a lock-free union-find, no CSR), and the subgraph two count / fill passes.

Semantics.  A component's label is the SMALLEST node id in it, so labels, roots and sizes are a pure function of the graph.  The largest
component is the one with the most nodes and, among equals, the one with the smallest root: what np.argmax over the reference's
discovery order (src/lcc.py:10-15) picks.  Kept edges come out in their original order, renumbered, with their original positions.

Two differences from the reference, both deliberate:
  * The reference numbers the kept nodes in the iteration order of a Python set of numpy integers (src/lcc.py:15, 18-24), which is NOT
    ascending (it was unordered in six of eight graphs tried).  This module numbers them ascending by id; the two subgraphs are equal
    up to that relabelling.  induced_subgraph(nodes=...) numbers by position in the list, as get_node_mapper does, for callers that
    need a given order.
  * On a directed edge_index the reference follows out-edges only (src/lcc.py:41), which gives the set reachable from the start node,
    not a component.  Here an edge counts in both directions: the components are the WEAK components.  The two agree on the symmetric
    graphs the reference feeds it.

Conventions, as negatives.py: an integer [2, E] edge_index, torch-style negative ids wrap, CPU ids outside [-N, N) raise IndexError
at once, device ids outside it are reported through the deferred error word (check_errors(), or the next call on the result) and the
offending edge is ignored.  N < 2^31 and E < 2^31.  Results live on edge_index's device.  No CPU fallback.
"""
import torch

from . import _native
from ._runtime import _DeferredErrors, _Span, _compute_device, _ptr, _stream
from .negatives import _int


def _nodes_count(num_nodes):
    N = _int(num_nodes, 'num_nodes', 1)
    if N >= (1 << 31):
        raise ValueError(f'components need num_nodes < 2^31 (node ids are int32 in the union-find), got {N}')
    return N


def _edge_index(ei, N):
    """an integer [2, E] edge_index with E < 2^31, its CPU ids checked at once (device ids: by the kernels)"""
    ei = torch.as_tensor(ei)
    if ei.dim() != 2 or ei.size(0) != 2 or ei.dtype.is_floating_point or ei.dtype.is_complex or ei.dtype == torch.bool:
        raise ValueError(f'edge_index must be an integer [2, E] tensor, got {ei.dtype} {tuple(ei.shape)}')
    if ei.size(1) >= (1 << 31):
        raise ValueError(f'edge_index holds {ei.size(1)} edges: the compaction passes take fewer than 2^31')
    if not ei.is_cuda and ei.numel() and (int(ei.min()) < -N or int(ei.max()) >= N):
        raise IndexError(f'edge_index refers to nodes outside [-{N}, {N})')
    return ei


def _node_set(N, nodes, mask):
    """what induced_subgraph checks of its node set before a device is touched: (nodes or None, mask or None)"""
    if (nodes is None) == (mask is None):
        raise ValueError('give the node set once: either nodes (a list of distinct ids) or mask (bool [N])')
    if mask is not None:
        mask = torch.as_tensor(mask)
        if mask.dtype != torch.bool or mask.dim() != 1 or mask.size(0) != N:
            raise ValueError(f'mask must be a bool [{N}] tensor, got {mask.dtype} {tuple(mask.shape)}')
        return None, mask
    nodes = torch.as_tensor(nodes)
    if nodes.dim() != 1 or nodes.dtype.is_floating_point or nodes.dtype.is_complex or nodes.dtype == torch.bool:
        raise ValueError(f'nodes must be an integer [n] tensor, got {nodes.dtype} {tuple(nodes.shape)}')
    if nodes.numel() >= (1 << 31):
        raise ValueError(f'nodes lists {nodes.numel()} ids: at most num_nodes < 2^31 distinct ones exist')
    if not nodes.is_cuda and nodes.numel():
        if int(nodes.min()) < -N or int(nodes.max()) >= N:
            raise IndexError(f'nodes refers to ids outside [-{N}, {N})')
        wrapped = torch.where(nodes < 0, nodes + N, nodes)
        if torch.unique(wrapped).numel() != wrapped.numel():
            raise ValueError('nodes lists an id more than once: the new ids are positions in the list')
    return nodes, None


def _on_device(t, device):
    return t.to(device=device, dtype=torch.int64).contiguous()


def _chunks(n):
    return (n + _native.COMPONENTS_CHUNK - 1) // _native.COMPONENTS_CHUNK


def _cumsum(counts):
    """the inclusive cumulative sum the fill passes take, and its last entry (one synchronising read)"""
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    return incl, int(incl[-1].item())


class Components(object):
    """the connected components of a graph, as connected_components returns them.

    labels          int64 [N]: the smallest node id of each node's component
    roots           int64 [C]: the nodes that are their own label, ascending
    sizes           int64 [C]: the number of nodes of the component of roots[i]
    num_components  C
    Ids outside [-N, N) in a DEVICE edge_index are reported late: IndexError from check_errors(), or from the next call of largest() /
    same() / subgraph(); such an edge is ignored."""

    def __init__(self, N, device, home, label32, roots, sizes, best, deferred):
        self.num_nodes, self.device = N, device
        self._home, self._label32, self._best, self._deferred = home, label32, best, deferred
        self.labels = label32.to(device=home, dtype=torch.int64)
        self.roots, self.sizes = roots.to(home), sizes.to(home)
        self.num_components = int(roots.numel())
        self._largest = None

    def check_errors(self):
        """wait for the launches issued so far and raise IndexError if one met a node id outside [-N, N)"""
        self._deferred.raise_if_set(synchronize=True)

    def _select_largest(self):
        """(nodes, mapper) of the largest component on the compute device, computed once"""
        if self._largest is None:
            self._largest = _select(self.num_nodes, self.device, label32=self._label32, best=self._best)
        return self._largest

    def largest(self):
        """int64 [n]: the node ids of the largest component, ascending (among equally large ones: the one with the smallest root)"""
        self._deferred.raise_if_set()
        return self._select_largest()[0].to(self._home)

    def same(self, links):
        """bool [L]: whether the two nodes of each link (int [L, 2], torch-style negative ids allowed) share a component.  CPU ids
        outside [-N, N) raise IndexError at once; device ids are reported late (check_errors) and give False."""
        N, device = self.num_nodes, self.device
        links = torch.as_tensor(links)
        if links.dim() != 2 or links.size(1) != 2 or links.dtype.is_floating_point or links.dtype.is_complex or links.dtype == torch.bool:
            raise ValueError(f'links must be an integer [L, 2] tensor, got {links.dtype} {tuple(links.shape)}')
        if not links.is_cuda and links.numel() and (int(links.min()) < -N or int(links.max()) >= N):
            raise IndexError(f'links refer to nodes outside [-{N}, {N})')
        self._deferred.raise_if_set()
        home, L = links.device, links.size(0)
        links = _on_device(links, device)
        out = torch.empty((L,), dtype=torch.bool, device=device)
        err = self._deferred.flag(device, f'same({L} links, num_nodes={N})')
        with _Span('components_same', device):
            _native.check(_native.lib().ss_components_same(_ptr(self._label32), N, _ptr(links), L, _ptr(out), _ptr(err), _stream(device)),
                          'ss_components_same')
        return out.to(home)

    def subgraph(self, edge_index):
        """the InducedSubgraph of the largest component over edge_index (the graph the components were taken of, or any other edge
        list over the same nodes)"""
        ei = _edge_index(edge_index, self.num_nodes)
        self._deferred.raise_if_set()
        nodes, mapper = self._select_largest()
        return _induce(self.num_nodes, ei, self.device, nodes, mapper, self._deferred)


class InducedSubgraph(object):
    """the subgraph a node set induces, as induced_subgraph returns it.

    nodes       int64 [n]: the kept node ids; new id i is nodes[i]
    mapper      int64 [N]: the new id of every node, -1 outside the set
    edge_index  int64 [2, E']: the edges with both ends kept, renumbered, in their original order
    edge_ids    int64 [E']: the positions of those edges in the input, strictly increasing
    Ids outside [-N, N) in a DEVICE edge_index are reported late: IndexError from check_errors(); such an edge is dropped."""

    def __init__(self, nodes, mapper, edge_index, edge_ids, deferred):
        self.nodes, self.mapper, self.edge_index, self.edge_ids = nodes, mapper, edge_index, edge_ids
        self.num_nodes, self.num_edges = int(nodes.numel()), int(edge_ids.numel())
        self._deferred = deferred

    def check_errors(self):
        """wait for the launches issued so far and raise IndexError if one met a node id outside [-N, N)"""
        self._deferred.raise_if_set(synchronize=True)


def _select(N, device, mask=None, label32=None, best=None):
    """(nodes ascending, mapper) on the device of the set mask, or of the component whose root the key *best names"""
    lib = _native.lib()
    counts = torch.empty((_chunks(N),), dtype=torch.int32, device=device)
    mapper = torch.empty((N,), dtype=torch.int64, device=device)
    with _Span('induced_select', device):
        _native.check(lib.ss_induced_select(_ptr(mask), _ptr(label32), _ptr(best), N, None, _ptr(counts), None, None, _stream(device)),
                      'ss_induced_select')
        incl, n = _cumsum(counts)
        nodes = torch.empty((max(n, 1),), dtype=torch.int64, device=device)  # (an empty set still takes the pass: mapper = -1)
        _native.check(lib.ss_induced_select(_ptr(mask), _ptr(label32), _ptr(best), N, _ptr(incl), None, _ptr(nodes), _ptr(mapper),
                                            _stream(device)), 'ss_induced_select')
    return nodes[:n], mapper


def _induce(N, ei, device, nodes, mapper, deferred):
    """the InducedSubgraph of (nodes, mapper) (on the compute device) over the checked edge_index ei, on ei's device"""
    lib = _native.lib()
    home, E = ei.device, ei.size(1)
    ei = _on_device(ei, device)
    src, dst = ei[0], ei[1]
    n_kept = 0
    if E:
        err = deferred.flag(device, f'induced_subgraph({E} edges, num_nodes={N})')
        counts = torch.empty((_chunks(E),), dtype=torch.int32, device=device)
        with _Span('induced_edges', device):
            _native.check(lib.ss_induced_edges(_ptr(src), _ptr(dst), E, N, _ptr(mapper), None, _ptr(counts), None, None, None, _ptr(err),
                                               _stream(device)), 'ss_induced_edges')
        incl, n_kept = _cumsum(counts)
    out = torch.empty((2, n_kept), dtype=torch.int64, device=device)
    ids = torch.empty((n_kept,), dtype=torch.int64, device=device)
    if n_kept:
        with _Span('induced_edges', device):
            _native.check(lib.ss_induced_edges(_ptr(src), _ptr(dst), E, N, _ptr(mapper), _ptr(incl), None, _ptr(out[0]), _ptr(out[1]), _ptr(ids),
                                               None, _stream(device)), 'ss_induced_edges')
    return InducedSubgraph(nodes.to(home), mapper.to(home), out.to(home), ids.to(home), deferred)


def connected_components(num_nodes, edge_index, device=None):
    """the (weak) connected components of the graph of edge_index over num_nodes nodes: a Components.
    @param num_nodes: N, 1 <= N < 2^31
    @param edge_index: int [2, E], E < 2^31 (torch-style negative ids allowed); CPU ids outside [-N, N) raise IndexError here
    @param device: the HIP device (default: edge_index's, else the current one)"""
    N = _nodes_count(num_nodes)
    ei = _edge_index(edge_index, N)
    device = torch.device(device) if device is not None else _compute_device(ei)
    lib = _native.lib()
    home, E = ei.device, ei.size(1)
    ei = _on_device(ei, device)
    deferred = _DeferredErrors()
    err = deferred.flag(device, f'connected_components({E} edges, num_nodes={N})')
    parent = torch.empty((N,), dtype=torch.int32, device=device)
    label = torch.empty((N,), dtype=torch.int32, device=device)
    with _Span('components_labels', device):
        _native.check(lib.ss_components_labels(_ptr(ei[0]) if E else None, _ptr(ei[1]) if E else None, E, N, _ptr(parent), _ptr(label), _ptr(err),
                                               _stream(device)), 'ss_components_labels')
    size = parent  # (the union-find's scratch is free again)
    counts = torch.empty((_chunks(N),), dtype=torch.int32, device=device)
    best = torch.zeros((1,), dtype=torch.int64, device=device)
    with _Span('components_sizes', device):
        _native.check(lib.ss_components_sizes(_ptr(label), N, _ptr(size), _ptr(counts), _stream(device)), 'ss_components_sizes')
        incl, C = _cumsum(counts)
        roots = torch.empty((C,), dtype=torch.int64, device=device)
        sizes = torch.empty((C,), dtype=torch.int64, device=device)
        _native.check(lib.ss_components_roots(_ptr(label), _ptr(size), N, _ptr(incl), _ptr(roots), _ptr(sizes), _ptr(best), _stream(device)),
                      'ss_components_roots')
    return Components(N, device, home, label, roots, sizes, best, deferred)


def induced_subgraph(num_nodes, edge_index, nodes=None, mask=None, device=None):
    """the subgraph of edge_index that a node set induces: an InducedSubgraph.
    @param nodes: int [n], distinct ids (torch-style negative ids allowed): the new id of nodes[i] is i
    @param mask: bool [N]: the new ids follow ascending id
    Give exactly one of the two.  A repeated id is a ValueError (from a device list: after one synchronising read); CPU ids outside
    [-N, N) raise IndexError at once."""
    N = _nodes_count(num_nodes)
    ei = _edge_index(edge_index, N)
    nodes, mask = _node_set(N, nodes, mask)
    device = torch.device(device) if device is not None else _compute_device(ei, nodes, mask)
    deferred = _DeferredErrors()
    if mask is not None:
        kept, mapper = _select(N, device, mask=mask.to(device).contiguous().view(torch.uint8))
    else:
        n = nodes.numel()
        listed = _on_device(nodes, device)
        mapper = torch.empty((N,), dtype=torch.int64, device=device)
        flags = torch.zeros((2,), dtype=torch.int32, device=device)  # {an id out of range, an id listed twice}
        with _Span('induced_mapper', device):
            _native.check(_native.lib().ss_induced_mapper(_ptr(listed) if n else None, n, N, _ptr(mapper), _ptr(flags[0:]), _ptr(flags[1:]),
                                                          _stream(device)), 'ss_induced_mapper')
        bad, twice = flags.tolist()
        if bad:
            raise IndexError(f'nodes refers to ids outside [-{N}, {N})')
        if twice:
            raise ValueError('nodes lists an id more than once: the new ids are positions in the list')
        kept = torch.where(listed < 0, listed + N, listed)
    return _induce(N, ei, device, kept, mapper, deferred)


def largest_component_subgraph(num_nodes, edge_index, device=None):
    """connected_components and induced_subgraph composed: what data.use_lcc computes (src/data.py:241-249).  The caller indexes its
    node features and labels with .nodes; .edge_index is the new graph."""
    N = _nodes_count(num_nodes)
    ei = _edge_index(edge_index, N)
    device = torch.device(device) if device is not None else _compute_device(ei)
    home, ei = ei.device, _on_device(ei, device)  # (one copy serves both steps)
    sub = connected_components(N, ei, device=device).subgraph(ei)
    if home != device:
        sub = InducedSubgraph(sub.nodes.to(home), sub.mapper.to(home), sub.edge_index.to(home), sub.edge_ids.to(home), sub._deferred)
    return sub
