"""Exact enclosing subgraphs (ElphHashes.exact_subgraphs, csrc/ss_subgraph.hip): per link (u, v) the node row of exact_subgraph_nodes
with the induced adjacency (local indices, arc multiplicities) and the SEAL node labels computed on that adjacency -- what the
reference builds per link in Python (src/datasets/seal.py:291-389, src/labelling_tricks.py) as one disjoint-union batch.
Design: DESIGN 3.18; numpy restatement: tests/subgraph_restatement.py.

With max_nodes_per_hop or ratio_per_hop < 1 the node rows are those of the sampled walk instead (sampled_nodes.sampled_subgraph_nodes,
DESIGN 3.19: the reference's per-hop neighbour caps) and the result is a SampledSubgraphs; the adjacency and the labels are the same calls.

Host side only: argument checks, the node rows (exact_nodes.exact_subgraph_nodes, unchanged), the CSR with sorted rows (a copy of the
engine's cached CSR columns, sorted once per edge_index), the count / fill walk of the adjacency with ONE host read between them (the
number of arcs, together with the workspace nodes of the rows labelled off chip) and the label launch."""
import weakref

import torch

from . import _native, exact, exact_nodes, knobs, sampled_nodes
from ._runtime import _compute_device, _ptr, _stream, _Span

NODE_LABELS = ('drnl', 'de', 'de+', 'hop', 'zo', None)


class ExactSubgraphs(object):
    """the labelled enclosing subgraphs of L links as one disjoint-union batch (every tensor on one device).

    rowptr int64 [L + 1], ids int64 [T], dist uint8 [T, 2]: exactly what exact_subgraph_nodes returns; node t of link q has the local
        index t - rowptr[q], rows ascend by id
    roots  int32 [L, 2]: local indices of u and v in their row, (-1, -1) for a row emptied by max_nodes
    adj_ptr int64 [T + 1], nbr int32 [A], weight int32 [A]: adjacency row of listed node t = nbr[adj_ptr[t] : adj_ptr[t + 1]], the local
        indices (in the same link's row, ascending) of the distinct nodes with an arc into t, and how many copies of that arc
        edge_index holds (the edge_weight SEAL's csr_matrix sums)
    z      the node labels: int64 [T] ('drnl', 'hop', 'zo'), int64 [T, 2] ('de', 'de+') or None
    info   with return_info: the node list's {'truncated', 'lds_links', 'large_links'}"""

    _per_node = 'dist'  # the field that holds what the node walk says of every listed node

    def __init__(self, rowptr, ids, dist, roots, adj_ptr, nbr, weight, z, node_label, info=None):
        self.rowptr, self.ids, self.dist, self.roots = rowptr, ids, dist, roots
        self.adj_ptr, self.nbr, self.weight, self.z = adj_ptr, nbr, weight, z
        self.node_label, self.info = node_label, info

    @property
    def num_links(self):
        return self.rowptr.numel() - 1

    def batch(self):
        """int64 [T]: the link of every listed node"""
        L = self.num_links
        return torch.repeat_interleave(torch.arange(L, dtype=torch.int64, device=self.rowptr.device), self.rowptr[1:] - self.rowptr[:-1])

    def edge_index(self):
        """int64 [2, A] in batch-global node slots: source rowptr[q] + nbr, target t -- the edge_index PyG's collate builds for the
        disjoint union of the subgraphs"""
        T = self.ids.numel()
        target = torch.repeat_interleave(torch.arange(T, dtype=torch.int64, device=self.ids.device), self.adj_ptr[1:] - self.adj_ptr[:-1])
        source = self.rowptr[:-1][self.batch()][target] + self.nbr.to(torch.int64)
        return torch.stack([source, target])

    def link(self, q):
        """the views of link q: dict(ids, dist (SampledSubgraphs: hop), roots, adj_ptr (local offsets, starting at 0), nbr, weight, z)"""
        a, b = int(self.rowptr[q]), int(self.rowptr[q + 1])
        e0, e1 = int(self.adj_ptr[a]), int(self.adj_ptr[b])
        return {'ids': self.ids[a:b], self._per_node: getattr(self, self._per_node)[a:b], 'roots': self.roots[q], 'adj_ptr': self.adj_ptr[a:b + 1] - e0,
                'nbr': self.nbr[e0:e1], 'weight': self.weight[e0:e1], 'z': None if self.z is None else self.z[a:b]}

    def to(self, device):
        move = lambda t: t.to(device) if torch.is_tensor(t) else t
        info = None if self.info is None else {k: move(x) for k, x in self.info.items()}
        return type(self)(*[move(getattr(self, k)) for k in ('rowptr', 'ids', self._per_node, 'roots', 'adj_ptr', 'nbr', 'weight', 'z')],
                          self.node_label, info)


class SampledSubgraphs(ExactSubgraphs):
    """the batch of exact_subgraphs(max_nodes_per_hop=..., ratio_per_hop=...): the node rows of sampled_subgraph_nodes, and on them what
    ExactSubgraphs holds.  hop uint8 [T] (the hop at which the node joined the walk, 0 for the roots: the reference's `dists`) takes the
    place of dist, which is None; link(q) returns 'hop'; info has 'sampled_links' too"""

    _per_node = 'hop'

    def __init__(self, rowptr, ids, hop, roots, adj_ptr, nbr, weight, z, node_label, info=None):
        ExactSubgraphs.__init__(self, rowptr, ids, None, roots, adj_ptr, nbr, weight, z, node_label, info)
        self.hop = hop


class _SortedRowsCache(object):
    """one-entry cache beside the engine's CSR cache: the column array of the cached CSR with every row sorted ascending (a COPY: the
    exact kernels keep reading the cached one), keyed like _CsrCache on the identity and version of the edge_index tensor"""

    def __init__(self):
        self._ref, self._version, self._key, self._col = None, None, None, None

    def get(self, edge_index, num_nodes, device, csr):
        key = (num_nodes, tuple(edge_index.shape), str(device))
        if self._ref is not None and self._ref() is edge_index and self._version == edge_index._version and self._key == key:
            return self._col
        lib = _native.lib()
        E = csr.num_edges
        col = csr.col.clone()
        ws_bytes = lib.ss_csr_sort_workspace_bytes(E)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
        with _Span('subgraph_sort_rows', device):
            _native.check(lib.ss_csr_sort_rows(_ptr(csr.rowptr), _ptr(col), num_nodes, E, None, _ptr(ws), ws_bytes, _stream(device)),
                          'ss_csr_sort_rows')
        self._ref, self._version, self._key, self._col = weakref.ref(edge_index), edge_index._version, key, col
        return col


def _label_arguments(node_label, max_dist):
    if node_label not in NODE_LABELS:
        raise ValueError(f"node_label must be one of 'drnl', 'de', 'de+', 'hop', 'zo' or None, got {node_label!r}")
    if isinstance(max_dist, bool) or not isinstance(max_dist, int) or not 1 <= max_dist <= _native.SUBGRAPH_MAX_DIST:
        raise ValueError(f'max_dist must be an integer in [1, {_native.SUBGRAPH_MAX_DIST}], got {max_dist!r}')
    return node_label, max_dist


def exact_subgraphs(eh, links, num_nodes, edge_index, batch_size=11000000, mask_target=True, max_nodes=None, node_label='drnl',
                    max_dist=1000, return_info=False, stats=None, *, max_nodes_per_hop=None, ratio_per_hop=1.0, seed=0):
    """see ElphHashes.exact_subgraphs.  stats (measurement hook, tools/probe_subgraphs.py): a dict that receives the milliseconds of
    the node list's passes and of the adjacency count, the offsets with the host read, the adjacency fill and the labels"""
    h = eh.max_hops
    exact.check_mask_target(mask_target)
    exact_nodes._cap(max_nodes)
    node_label, max_dist = _label_arguments(node_label, max_dist)
    cap_hop, ratio, seed = sampled_nodes.sampling_arguments(max_nodes_per_hop, ratio_per_hop, seed)
    sampled = cap_hop > 0 or ratio < 1.0
    lk, ei, N, batch_size = exact.check_arguments(h, links, num_nodes, edge_index, batch_size)
    home, L = lk.device, lk.size(0)
    if sampled:  # the node rows of the sampled walk (the target link stays in the walk: removing it belongs to the adjacency)
        make = SampledSubgraphs
        node_rows = lambda lk_, st: sampled_nodes.sampled_subgraph_nodes(eh, lk_, N, ei, batch_size, max_nodes_per_hop, ratio, seed, max_nodes,
                                                                         True, stats=st)
    else:  # the node list's own call (same kernels, same bits)
        make = ExactSubgraphs
        node_rows = lambda lk_, st: exact_nodes.exact_subgraph_nodes(eh, lk_, N, ei, batch_size, mask_target, max_nodes, True, stats=st)
    two = node_label in ('de', 'de+')
    if L == 0:
        rowptr, ids, per_node, info = node_rows(lk, None)
        z = None if node_label is None else torch.empty((0, 2) if two else (0,), dtype=torch.int64, device=home)
        return make(rowptr, ids, per_node, torch.empty((0, 2), dtype=torch.int32, device=home), torch.zeros((1,), dtype=torch.int64, device=home),
                    torch.empty((0,), dtype=torch.int32, device=home), torch.empty((0,), dtype=torch.int32, device=home), z,
                    node_label, info if return_info else None)
    device = _compute_device(lk, ei)
    lk = lk.to(device=device, dtype=torch.int64).contiguous()
    rowptr, ids, per_node, info = node_rows(lk, stats)  # (fills the engine's CSR cache for `ei`)
    out = make(rowptr, ids, per_node, *_adjacency_and_labels(eh, lk, ei, N, device, rowptr, ids, per_node, mask_target, node_label, max_dist, stats),
               node_label, info if return_info else None)
    return out.to(home) if home != device else out


def _adjacency_and_labels(eh, lk, ei, N, device, rowptr, ids, per_node, mask_target, node_label, max_dist, stats):
    """-> (roots, adj_ptr, nbr, weight, z) of node rows on the compute device, whichever walk made them: the induced adjacency (count,
    ONE host read, fill) and the labels.  per_node: dist uint8 [T, 2] or hop uint8 [T], what 'hop' and 'zo' are read from"""
    L = lk.size(0)
    two = node_label in ('de', 'de+')
    csr = eh._csr_cache.get(ei, N, device)
    cache = eh.__dict__.get('_sorted_rows_cache')
    if cache is None:
        cache = eh._sorted_rows_cache = _SortedRowsCache()
    col = cache.get(ei, N, device, csr)
    T = ids.numel()
    lib, stream = _native.lib(), _stream(device)
    flags = _native.SS_FLAG_MASK_TARGET if mask_target else 0
    switch = min(max(0, int(knobs.SUBGRAPH_ADJ_SWITCH)), (1 << 31) - 1)
    lds_nodes = max(0, int(knobs.EXACT_LDS_MAX_NODES))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if stats is not None else None
    adj = lambda counts, adj_ptr, nbr, weight, roots: _native.check(
        lib.ss_subgraph_adj(_ptr(csr.rowptr), _ptr(col), N, _ptr(lk), L, _ptr(rowptr), _ptr(ids), T, flags, switch, _ptr(counts), _ptr(adj_ptr),
                            _ptr(nbr), _ptr(weight), _ptr(roots), stream), 'ss_subgraph_adj')
    if ev:
        ev[0].record()
    counts = torch.empty((T,), dtype=torch.int32, device=device)
    with _Span('subgraph_adj_count', device):
        adj(counts, None, None, None, None)
    if ev:
        ev[1].record()
    adj_ptr = torch.zeros((T + 1,), dtype=torch.int64, device=device)
    torch.cumsum(counts, 0, dtype=torch.int64, out=adj_ptr[1:])
    # rows longer than the label kernel's on-chip limit get a slice of a device workspace: their node counts, summed
    sizes = rowptr[1:] - rowptr[:-1]
    ws_ptr = torch.zeros((L + 1,), dtype=torch.int64, device=device)
    torch.cumsum(torch.where(sizes > min(lds_nodes, 2048), sizes, torch.zeros_like(sizes)), 0, out=ws_ptr[1:])
    A, ws_nodes = torch.stack([adj_ptr[-1], ws_ptr[-1]]).tolist()  # the one host read: two allocations
    nbr = torch.empty((max(A, 1),), dtype=torch.int32, device=device)  # (A = 0: not a null pointer, the fill pass still writes the roots)
    weight = torch.empty((max(A, 1),), dtype=torch.int32, device=device)
    roots = torch.full((L, 2), -1, dtype=torch.int32, device=device)
    if ev:
        ev[2].record()
    with _Span('subgraph_adj_fill', device):
        adj(None, adj_ptr, nbr, weight, roots)
    if ev:
        ev[3].record()
    if node_label in _native.SUBGRAPH_LABELS:
        z = torch.empty((T, 2) if two else (T,), dtype=torch.int64, device=device)
        ws = torch.empty((4 * ws_nodes,), dtype=torch.int32, device=device) if ws_nodes else None
        if T:
            with _Span('subgraph_labels', device):
                _native.check(lib.ss_subgraph_labels(_ptr(rowptr), L, _ptr(roots), _ptr(adj_ptr), _ptr(nbr), _native.SUBGRAPH_LABELS[node_label],
                                                     max_dist, lds_nodes, _ptr(ws_ptr), _ptr(ws), _ptr(z), stream), 'ss_subgraph_labels')
    elif node_label is None:
        z = None
    else:  # the two labels that are functions of the ball distances alone
        z = (per_node.min(dim=1).values if per_node.dim() == 2 else per_node).to(torch.int64)
        if node_label == 'zo':
            z = (z == 0).to(torch.int64)
    nbr, weight = nbr[:A], weight[:A]
    if ev:
        ev[4].record()
        ev[4].synchronize()
        for k, name in enumerate(('adj_count_ms', 'adj_ptr_ms', 'adj_fill_ms', 'labels_ms')):
            stats[name] = stats.get(name, 0.0) + ev[k].elapsed_time(ev[k + 1])
        stats['arcs'] = A
    return roots, adj_ptr, nbr, weight, z
