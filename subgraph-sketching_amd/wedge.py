"""Exact two-hop link candidates: WedgeGraph.candidates -- the nodes that share at least one neighbour with each source, with the
number of walks -- and topk_links restricted to them (ElphHashes.topk_links_wedge).  Kernels: csrc/ss_wedge.hip; design: DESIGN
3.16; numpy restatement: tests/wedge_restatement.py.

The reference has no counterpart: its sample_hard_negatives (src/data.py:262-304: non-edges with a common neighbour) is unfinished.
topk_links scores all N nodes per source, topk_links_lsh the nodes that share a MinHash band with it (approximate, its recall a matter
of rows / bands); this is the exact set in between, from the sorted CSR that NegativeSampler builds.

Semantics.  The graph is the directed pairs u -> v of edge_index exactly as given: no self loops added, duplicates kept, negative ids
wrapped; row u = {v : u -> v}.  A walk of u is u -> w -> v with w in row u and v in row w, every copy of a repeated edge its own walk
(the wedge of sample_negatives); W(u) = sum of deg(w) over w in row u; common[u, v] = the walks of u that end in v -- on a simple
symmetric graph without self loops the number of common neighbours.  v is a candidate of u iff v != u, common[u, v] >= min_common and
u -> v is not in `exclude`.  Neighbours of u are candidates unless excluded (exclude=edge_index: non-edges only).  A source outside
[-N, N), or with W(u) > max_walks or W(u) >= 2^31, lists nothing and is counted as skipped.
"""
import numpy as np
import torch

from . import _native
from ._runtime import _DeferredErrors, _Span, _compute_device, _ptr, _stream
from .candidates import _block_walk, _check_host_ids, _check_scoring, _id_list, _int, _rows, _topk_rows
from .engine import _table_shape
from .negatives import _edge_index, _sorted_rows

# rows depend on none of these (not user knobs)
_WEDGE_BLOCK_BYTES = 1 << 30  # bound on the arrays of one block of sources: 24 bytes per source of the walks launch, then the block's walks
_WEDGE_WALK_BYTES = 64        # per walk of a block: key + count, the sorted keys and the sort's indices, the unique keys, their inverse and sums
_WEDGE_SLICE_WALKS = 1 << 15  # the large tier spreads a block over ceil(largest W / this) workgroups per source (at most _native.WEDGE_MAX_SLICES)
_MAX_WALKS = (1 << 31) - 1
_PAD = (1 << 63) - 1          # kWedgePad of csrc/ss_wedge.hpp


def _arguments(N, sources, exclude, min_common, max_walks, lds_slots):
    """what .candidates and topk_links_wedge check of their own arguments before a device is touched:
    (sources, exclude or None, min_common, the largest W(u) that is listed, lds_slots)"""
    src = _id_list(sources)
    if src.numel() >= (1 << 31):
        raise ValueError(f'sources holds {src.numel()} ids: a call takes fewer than 2^31')
    ex = None if exclude is None else _edge_index(exclude, 'exclude', N)
    _check_host_ids(src, N)
    min_common = _int(min_common, 'min_common', 1)
    cap = _MAX_WALKS if max_walks is None else min(_int(max_walks, 'max_walks', 0), _MAX_WALKS)
    slots = _native.WEDGE_MAX_SLOTS if lds_slots is None else _int(lds_slots, '_lds_slots', 1, _native.WEDGE_MAX_SLOTS)
    if slots & (slots - 1):
        raise ValueError(f'_lds_slots must be a power of two, got {lds_slots!r}')
    return src, ex, min_common, cap, slots


# ---- the three launches (module-level, so that the host walk can be rehearsed without a device) -------------------------------------
def _launch_walks(graph, sources, walks, err):
    with _Span('wedge_walks', graph.device):
        _native.check(_native.lib().ss_wedge_walks(_ptr(graph.rowptr), _ptr(graph.col), graph.num_nodes, _ptr(sources), sources.numel(),
                                                   _ptr(walks), _ptr(err), _stream(graph.device)), 'ss_wedge_walks')


def _launch_fold(graph, sources, take, offsets, slots, keys, counts):
    with _Span('wedge_fold', graph.device):
        _native.check(_native.lib().ss_wedge_fold(_ptr(graph.rowptr), _ptr(graph.col), graph.num_nodes, _ptr(sources), sources.numel(),
                                                  _ptr(take), _ptr(offsets), slots, _ptr(keys), _ptr(counts), _stream(graph.device)),
                      'ss_wedge_fold')


def _launch_emit(graph, sources, take, offsets, slots, slices, keys):
    with _Span('wedge_emit', graph.device):
        _native.check(_native.lib().ss_wedge_emit(_ptr(graph.rowptr), _ptr(graph.col), graph.num_nodes, _ptr(sources), sources.numel(),
                                                  _ptr(take), _ptr(offsets), slots, slices, _ptr(keys), _stream(graph.device)),
                      'ss_wedge_emit')


def _walk(graph, src, ex, min_common, cap, slots, bounds):
    """candidates._block_walk over the walks of the graph, to be called with a consume: blocks of sources bounded by _WEDGE_BLOCK_BYTES, per
    block the walks launch (its W(u): the sizes, and which tier has work); per group both tiers write into one (key, count) array of sum
    W(u) places, the LDS tier's padding is dropped, a sort and a run-length sum fold what the large tier left unfolded; min_common and
    v != u are the filter.  -> (the walk; W(u) int64 [S] on the device, which it fills; the tier counts [lds, large], which it adds to)"""
    device, N = graph.device, graph.num_nodes
    walks = torch.zeros((src.numel(),), dtype=torch.int64, device=device)
    served = [0, 0]

    def count(c0, sources, err):
        mine = walks[c0:c0 + sources.numel()]
        _launch_walks(graph, sources, mine, err)
        w = mine.cpu().numpy()
        w = np.where(w > cap, 0, w)  # (a skipped source lists nothing)
        return np.cumsum(w), (w, mine)

    def expand(block, a, e, _base, total, sb, u):
        keys = torch.empty((total,), dtype=torch.int64, device=device)
        common = torch.ones((total,), dtype=torch.int32, device=device)
        if total:
            wb = block[0][a:e]
            folds, emits = (wb > 0) & (2 * wb <= slots), 2 * wb > slots
            served[0] += int(folds.sum())
            served[1] += int(emits.sum())
            take = block[1][a:e]
            take = take.masked_fill(take > cap, 0)
            offsets = torch.cumsum(take, 0) - take
            if folds.any():
                _launch_fold(graph, sb, take, offsets, slots, keys, common)
            if emits.any():
                slices = min(_native.WEDGE_MAX_SLICES, -(-int(wb[emits].max()) // _WEDGE_SLICE_WALKS))
                _launch_emit(graph, sb, take, offsets, slots, slices, keys)
            with _Span('wedge_unique', device):
                if folds.any():
                    used = keys != _PAD
                    keys, common = keys[used], common[used]
                keys, order = torch.sort(keys)
                common = common[order]
                if emits.any():
                    keys, run = torch.unique_consecutive(keys, return_inverse=True)
                    common = torch.zeros((keys.numel(),), dtype=torch.int32, device=device).index_add_(0, run, common)
        with _Span('wedge_filter', device):
            s = keys // N
            return keys, common, (common >= min_common) & (keys - s * N != u[s])

    block = max(1, _WEDGE_BLOCK_BYTES // 24)
    room = max(1, _WEDGE_BLOCK_BYTES // _WEDGE_WALK_BYTES)
    walk = lambda consume: _block_walk(device, N, src, ex, bounds, 'wedge candidates', 'wedge_filter', block, room, count, expand, consume)
    return walk, walks, served


class WedgeGraph(object):
    """the sorted CSR of a graph, built once and resident on the device; .candidates lists, per source, the nodes two steps away.

    @param num_nodes: N, 1 <= N < 2^31
    @param edge_index: int [2, E] (torch-style negative ids allowed); ids outside [-N, N) raise IndexError here
    @param device: the HIP device (default: edge_index's, else the current one)
    `strict_bounds` says how ids outside [-N, N) in DEVICE sources are reported, as ElphHashes.strict_bounds does: 'deferred' (default)
    = IndexError at the next .candidates, at check_errors() or when a result is copied to a CPU caller; True = from the offending call;
    False = never.  Such a source lists nothing and counts as skipped.  After the graph changes (update_hash_tables): build a new one."""

    def __init__(self, num_nodes, edge_index, device=None):
        N = _int(num_nodes, 'num_nodes', 1)
        if N >= (1 << 31):
            raise ValueError(f'a WedgeGraph needs num_nodes < 2^31 (node ids are int32 in the CSR), got {N}')
        ei = _edge_index(edge_index, 'edge_index', N)
        self.num_nodes = N
        self.device = torch.device(device) if device is not None else _compute_device(ei)
        self.strict_bounds = 'deferred'
        self._deferred = _DeferredErrors()
        csr = _sorted_rows(ei, N, self.device)
        self.rowptr, self.col, self.num_edges = csr.rowptr, csr.col, int(csr.num_edges)

    def __repr__(self):
        return f'WedgeGraph(num_nodes={self.num_nodes}, num_edges={self.num_edges}, device={self.device})'

    def __getstate__(self):  # host copies and names only: no device memory, no pinned report word
        return {'num_nodes': self.num_nodes, 'num_edges': self.num_edges, 'device': str(self.device), 'strict_bounds': self.strict_bounds,
                'rowptr': self.rowptr.cpu(), 'col': self.col.cpu()}

    def __setstate__(self, state):
        self.num_nodes, self.num_edges, self.strict_bounds = state['num_nodes'], state['num_edges'], state['strict_bounds']
        self.device = torch.device(state['device'])
        self._deferred = _DeferredErrors()
        self.rowptr, self.col = state['rowptr'].to(self.device), state['col'].to(self.device)

    def check_errors(self):
        """strict_bounds = 'deferred': wait for the launches issued so far and raise IndexError if one met a source outside [-N, N)"""
        self._deferred.raise_if_set(synchronize=True)

    def _bounds(self, device, what):
        if self.strict_bounds == 'deferred':
            self._deferred.raise_if_set()
            return False, self._deferred.flag(device, what)
        return bool(self.strict_bounds), None

    def candidates(self, sources, exclude=None, min_common=1, max_walks=None, return_info=False, _lds_slots=None):
        """per source the nodes v != u that >= min_common walks u -> w -> v end in, without the pairs u -> v of `exclude`.
        @param sources: int [S] node ids (torch-style negative ids wrapped, duplicates allowed, CPU or device, S = 0 fine)
        @param exclude: optional int [2, E] edge_index read as a set of directed pairs (duplicates, self loops, negative ids fine);
               exclude=edge_index leaves the non-edges
        @param max_walks: a source with more walks W(u) lists nothing and is counted (None: only W(u) >= 2^31 does): the rule
               max_bucket is for build_lsh_index, applied to hubs
        @return: (rowptr int64 [S + 1], ids int64 [T], common int32 [T]) on sources.device: row s is ids[rowptr[s] : rowptr[s + 1]],
                 ascending and unique, common = the walks that end there.  A row depends on its source and the graph only.  With
                 return_info also {'skipped_sources': n, 'walks': W(u) int64 [S], 'lds_sources' / 'large_sources': how many sources
                 each kernel tier served}.  No CPU fallback."""
        N, device = self.num_nodes, self.device
        src, ex, min_common, cap, slots = _arguments(N, sources, exclude, min_common, max_walks, _lds_slots)
        walk, walks, served = _walk(self, src, ex, min_common, cap, slots, self._bounds)
        home, out = src.device, [*_rows(device, src.numel(), N, walk), walks]
        if home != device:
            out = [t.to(home) for t in out]
            if self.strict_bounds == 'deferred':  # a copy has waited for the launches: a deferred report is final behind it
                self._deferred.raise_if_set()
        if not return_info:
            return tuple(out[:3])
        lk = src.to(torch.int64)
        skipped = int(((lk < -N) | (lk >= N) | (out[3] > cap)).sum())
        return out[0], out[1], out[2], {'skipped_sources': skipped, 'walks': out[3], 'lds_sources': served[0], 'large_sources': served[1]}


def topk_links_wedge(eh, sources, hash_table, cards, k, head, graph, degrees, exclude, min_common, max_walks, lds_slots=None):
    _check_scoring(eh, cards, head, degrees)
    if not isinstance(graph, WedgeGraph):
        raise ValueError(f'graph must be a WedgeGraph (WedgeGraph(num_nodes, edge_index)), got {type(graph).__name__}')
    N, P = _table_shape(hash_table, 1)
    if graph.num_nodes != N:
        raise ValueError(f'the graph has {graph.num_nodes} nodes, hash_table holds [{N}, {P}] MinHash tables')
    eh._topk_arguments(sources, hash_table, k, None)
    src, ex, min_common, cap, slots = _arguments(N, sources, exclude, min_common, max_walks, lds_slots)
    walk = _walk(graph, src, ex, min_common, cap, slots, eh._bounds)[0]
    return _topk_rows(eh, src, hash_table, cards, int(k), head, degrees, graph.device, 'wedge_select', walk)
