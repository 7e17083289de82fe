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
from ._runtime import _DeferredErrors, _Span, _compute_device, _ptr, _stream, _take_error
from .engine import _csr_row_keys, _exclude_csr, _table_shape, _table_ptrs
from .lsh import _row_starts, _select_rows
from .negatives import _edge_index, _int, _sorted_rows

# rows depend on none of these (not user knobs)
_WEDGE_BLOCK_BYTES = 1 << 30  # bound on the arrays of one block of sources: 24 bytes per source of the walks launch, then the block's walks
_WEDGE_WALK_BYTES = 64        # per walk of a block: key + count, the sorted keys and the sort's indices, the unique keys, their inverse and sums
_WEDGE_SLICE_WALKS = 1 << 15  # the large tier spreads a block over ceil(largest W / this) workgroups per source (at most _native.WEDGE_MAX_SLICES)
_MAX_WALKS = (1 << 31) - 1
_PAD = (1 << 63) - 1          # kWedgePad of csrc/ss_wedge.hpp


def _arguments(N, sources, exclude, min_common, max_walks, lds_slots):
    """what .candidates and topk_links_wedge check of their own arguments before a device is touched:
    (sources, exclude or None, min_common, the largest W(u) that is listed, lds_slots)"""
    src = torch.as_tensor(sources)
    if src.dim() != 1 or src.dtype.is_floating_point or src.dtype == torch.bool:
        raise ValueError(f'sources must be a 1-D integer tensor, got {src.dtype} {tuple(src.shape)}')
    if src.numel() >= (1 << 31):
        raise ValueError(f'sources holds {src.numel()} ids: a call takes fewer than 2^31')
    ex = None if exclude is None else _edge_index(exclude, 'exclude', N)
    if not src.is_cuda and src.numel() and (int(src.min()) < -N or int(src.max()) >= N):
        raise IndexError(f'sources refer to nodes outside [-{N}, {N})')
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


def _walk(graph, src, ex, min_common, cap, slots, bounds, consume):
    """the walk both queries share: blocks of sources bounded by _WEDGE_BLOCK_BYTES -- the walks launch over a block, ONE host read
    (its W(u): the sizes, and which tier has work), then as many whole sources as fit the budget (one at least): both tiers write into
    one (key, count) array of sum W(u) places, the padding of the LDS tier is dropped, a sort and a run-length sum fold what the large
    tier left unfolded, then min_common and the exclude list, then consume(b0, u, keys, common, err): sources [b0, b0 + len(u)) with
    wrapped ids u, the block's pairs as sorted unique keys s * N + v (s: the source's place in the block) and their walk counts.
    The tier never shows: every source goes through the same sort.  -> (W(u) int64 [S] on the device, tier counts [lds, large])"""
    device, N = graph.device, graph.num_nodes
    S = src.numel()
    lk = src.to(device=device, dtype=torch.int64).contiguous()
    strict, err = bounds(device, f'wedge candidates({S} sources, num_nodes={N})')
    csr, err = _exclude_csr(ex, N, device, strict, err)
    walks = torch.zeros((S,), dtype=torch.int64, device=device)
    served = [0, 0]
    room = max(1, _WEDGE_BLOCK_BYTES // _WEDGE_WALK_BYTES)
    cblk = max(1, min(S, _WEDGE_BLOCK_BYTES // 24))
    for c0 in range(0, S, cblk):
        nc = min(cblk, S - c0)
        _launch_walks(graph, lk[c0:c0 + nc], walks[c0:c0 + nc], err)
        w = walks[c0:c0 + nc].cpu().numpy()
        w = np.where(w > cap, 0, w)  # (a skipped source lists nothing)
        ends = np.cumsum(w)
        a = 0
        while a < nc:  # as many whole sources as fit the budget, one at least
            base = int(ends[a - 1]) if a else 0
            e = min(nc, max(a + 1, int(np.searchsorted(ends, base + room, side='right'))))
            total = int(ends[e - 1]) - base
            sb = lk[c0 + a:c0 + e]
            u = torch.where(sb < 0, sb + N, sb)
            u = u.masked_fill((u < 0) | (u >= N), 0)  # (an id out of range has no walks)
            keys = torch.empty((total,), dtype=torch.int64, device=device)
            common = torch.ones((total,), dtype=torch.int32, device=device)
            if total:
                wb = w[a:e]
                folds, emits = (wb > 0) & (2 * wb <= slots), 2 * wb > slots
                served[0] += int(folds.sum())
                served[1] += int(emits.sum())
                take = walks[c0 + a:c0 + e]
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
                keep = common >= min_common
                s = keys // N
                keep &= keys - s * N != u[s]
                if csr is not None and keys.numel():
                    gone = _csr_row_keys(csr, u, N)
                    if gone is not None:
                        keep &= gone[torch.searchsorted(gone, keys).clamp_(max=gone.numel() - 1)] != keys
                keys, common = keys[keep], common[keep]
            consume(c0 + a, u, keys, common, err)
            a = e
    if strict and S and _take_error(device):
        raise IndexError(f'sources refer to nodes outside [-{N}, {N})')
    return walks, served


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
        home, S = src.device, src.numel()
        sizes = torch.zeros((S,), dtype=torch.int64, device=device)
        ids, common = [torch.empty((0,), dtype=torch.int64, device=device)], [torch.empty((0,), dtype=torch.int32, device=device)]

        def consume(b0, u, keys, counts, _err):
            sizes[b0:b0 + u.numel()] = torch.diff(_row_starts(keys, u.numel(), N))
            ids.append(keys % N)
            common.append(counts)

        walks, served = _walk(self, src, ex, min_common, cap, slots, self._bounds, consume)
        rowptr = torch.zeros((S + 1,), dtype=torch.int64, device=device)
        torch.cumsum(sizes, 0, out=rowptr[1:])
        out = [rowptr, torch.cat(ids), torch.cat(common), walks]
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
    eh._check_head(head, degrees)
    if cards is None:
        raise ValueError('cards must be given: the feature row needs the neighbourhood sizes build_hash_tables returns')
    if not isinstance(graph, WedgeGraph):
        raise ValueError(f'graph must be a WedgeGraph (WedgeGraph(num_nodes, edge_index)), got {type(graph).__name__}')
    N, P = _table_shape(hash_table, 1)
    if graph.num_nodes != N:
        raise ValueError(f'the graph has {graph.num_nodes} nodes, hash_table holds [{N}, {P}] MinHash tables')
    eh._topk_arguments(sources, hash_table, k, None)
    src, ex, min_common, cap, slots = _arguments(N, sources, exclude, min_common, max_walks, lds_slots)
    k = int(k)
    home, S = src.device, src.numel()
    device = graph.device
    mh, hll, N, P = eh._resolve_tables(hash_table, device)
    params = eh._params(device)
    cd, dg, hd = eh._device_cards(cards, N, device), eh._device_degrees(degrees, N, device), head._device(device)
    mh_ptrs, hll_ptrs = _table_ptrs(mh, hll)
    ids = torch.empty((S, k), dtype=torch.int64, device=device)
    scores = torch.empty((S, k), dtype=torch.float32, device=device)

    def consume(b0, u, keys, _common, err):
        score = eh._pair_scores(device, N, P, mh_ptrs, hll_ptrs, cd, params, dg, hd, err)
        n = u.numel()
        s = keys // N
        sc = score(torch.stack([u[s], keys - s * N], dim=1).contiguous(), torch.empty((keys.numel(),), dtype=torch.float32, device=device))
        with _Span('wedge_select', device):
            ids[b0:b0 + n], scores[b0:b0 + n] = _select_rows(keys, sc, n, N, k)

    _walk(graph, src, ex, min_common, cap, slots, eh._bounds, consume)
    return eh._send_home(home, ids, scores)
