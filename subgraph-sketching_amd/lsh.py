"""LSH by banding over one hop's MinHash table: the index (ElphHashes.build_lsh_index), the candidate query behind it (lsh_candidates)
and topk_links restricted to the candidates (topk_links_lsh).  Kernels: csrc/ss_lsh.hip; design and measurements: DESIGN 3.14.

The reference has no counterpart: its sample_hard_negatives (src/data.py:262-304) is unfinished; topk_candidates / topk_links answer it
by scanning all N nodes per source, which is the tool for evaluation and too much for a pass over every source of a graph.

Semantics (tests/lsh_restatement.py restates them in numpy).  With M_k[v] the stored hop-k MinHash row of v, band j of v is the slice
M_k[v][j r : (j + 1) r]; the bucket of (j, v) is the set of nodes whose band-j slice equals v's, value for value; a bucket with more
than max_bucket members is skipped; v is a candidate of u iff v != u, (u -> v) is not excluded and u, v share a non-skipped bucket in
at least min_bands bands.  The 64-bit key the bands are sorted by only finds the range to verify: with all 64 bits two different
slices meet in one range with probability about 2^-64 per pair, and the one way such a meeting could show is a range of more than
max_bucket entries made of several smaller buckets, which is dropped like a large bucket.
"""
from ctypes import c_void_p

import numpy as np
import torch

from . import _native
from ._runtime import _Span, _check_sizes, _compute_device, _ptr, _stream, _take_error
from .containers import HopSketch, _packed_minhash_of
from .engine import TOPK_SENTINEL, _csr_row_keys, _decode_topk_keys, _encode_topk_keys, _exclude_csr, _table_ptrs, _table_shape

# rows depend on neither constant (not user knobs)
_LSH_BLOCK_BYTES = 1 << 30  # bound on the arrays of one block of sources: counts + offsets per (source, band), then the block's entries
_LSH_ENTRY_BYTES = 48       # per listed (source, band, node) entry: the entry, its sorted copy and the sort's indices, unique keys + counts
_LSH_SORT_BYTES = 1 << 28   # bands sorted per torch.sort call when the index is built: their keys fit this


class LshIndex(object):
    """what build_lsh_index returns: per band the sorted 64-bit keys of all nodes and the nodes in that order, resident on the compute
    device, plus a VIEW of the hop's packed MinHash table (every candidate's slice is compared with the source's: the keys only find
    the range).  Stale once the table changes (update_hash_tables): rebuild it.  No file format, one hop per index."""

    def __init__(self, hop, rows, bands, max_bucket, mh_u32, keys, perm, skipped_buckets, key_bits=64):
        self.hop, self.rows, self.bands, self.max_bucket, self.key_bits = int(hop), int(rows), int(bands), int(max_bucket), int(key_bits)
        self.mh_u32 = mh_u32                    # [N, P] int32 holding uint32 bit patterns: the table's own tensor
        self.keys, self.perm = keys, perm       # [bands, N] int64 sorted per band / int32 node ids in that order
        self.skipped_buckets = skipped_buckets  # int64 [bands]: buckets of more than max_bucket members

    @property
    def num_nodes(self):
        return int(self.mh_u32.shape[0])

    @property
    def num_perm(self):
        return int(self.mh_u32.shape[1])

    @property
    def nbytes(self):
        """device bytes the index owns (12 per node and band; the table it views is the caller's)"""
        return sum(t.numel() * t.element_size() for t in (self.keys, self.perm, self.skipped_buckets))

    def __repr__(self):
        return (f'LshIndex(hop={self.hop}, rows={self.rows}, bands={self.bands}, num_nodes={self.num_nodes}, num_perm={self.num_perm}, '
                f'max_bucket={self.max_bucket}, nbytes={self.nbytes})')


def _int(value, name, lo, hi=None):
    try:
        v = int(value)
    except (TypeError, ValueError):
        raise ValueError(f'{name} must be an integer, got {value!r}')
    if v != value or v < lo or (hi is not None and v > hi):
        raise ValueError(f'{name} must lie in [{lo}, {hi if hi is not None else "..."}], got {value!r}')
    return v


def build_lsh_index(eh, hash_table, hop, rows, bands, max_bucket, key_bits):
    hop = _int(hop, 'hop', 1, eh.max_hops)
    N, P = _table_shape(hash_table, hop)
    _check_sizes(P, eh.p)
    rows = _int(rows, 'rows', 1, P)
    bands = P // rows if bands is None else _int(bands, 'bands', 1)
    if rows * bands > P:
        raise ValueError(f'rows * bands = {rows} * {bands} bands need more than the {P} MinHash values of a row')
    max_bucket = min(_int(max_bucket, 'max_bucket', 1), (1 << 31) - 2)
    key_bits = _int(key_bits, '_key_bits', 1, 64)
    if not 1 <= N < (1 << 31):
        raise ValueError(f'an LSH index needs 1 <= num_nodes < 2^31, got {N}')
    entry = hash_table[hop]
    if isinstance(entry, HopSketch):
        device = _compute_device(entry.mh_u32)
        mh = entry.packed(device)[0] if entry.mh_u32.device == device else entry.mh_u32.to(device)
    else:
        device = _compute_device(entry['minhash'])
        mh = _packed_minhash_of(entry['minhash'], device)
    mh = mh.contiguous()
    lib = _native.lib()
    keys = torch.empty((bands, N), dtype=torch.int64, device=device)
    with _Span('lsh_band_keys', device):
        _native.check(lib.ss_lsh_band_keys(_ptr(mh), N, P, rows, bands, key_bits, _ptr(keys), _stream(device)), 'ss_lsh_band_keys')
    perm = torch.empty((bands, N), dtype=torch.int32, device=device)
    skipped = torch.zeros((bands,), dtype=torch.int64, device=device)
    step = max(1, _LSH_SORT_BYTES // (8 * N))
    with _Span('lsh_sort', device):
        for j0 in range(0, bands, step):
            sk, order = torch.sort(keys[j0:j0 + step], dim=1)
            keys[j0:j0 + step] = sk
            perm[j0:j0 + step] = order
            # runs of equal keys never cross a band: every band's first entry starts one
            start = torch.ones(sk.shape, dtype=torch.bool, device=device)
            start[:, 1:] = sk[:, 1:] != sk[:, :-1]
            at = torch.nonzero(start.reshape(-1)).reshape(-1)
            length = torch.diff(at, append=at.new_tensor([sk.numel()]))
            skipped[j0:j0 + step] = torch.bincount(at[length > max_bucket] // N, minlength=sk.size(0))
    return LshIndex(hop, rows, bands, max_bucket, mh, keys, perm, skipped, key_bits)


def _arguments(eh, sources, index, exclude, min_bands):
    """what lsh_candidates and topk_links_lsh check of their own arguments before a device is touched"""
    if not isinstance(index, LshIndex):
        raise ValueError(f'index must be an LshIndex (ElphHashes.build_lsh_index), got {type(index).__name__}')
    min_bands = _int(min_bands, 'min_bands', 1)
    src, ex, N, _ = eh._topk_arguments(sources, {1: {'minhash': index.mh_u32}}, 1, exclude)
    return src, ex, min_bands


def _walk(eh, what, src, ex, index, min_bands, consume):
    """the walk both queries share: blocks of sources bounded by _LSH_BLOCK_BYTES -- the entries of a block cannot be known before
    its counts are -- , per block the count and fill launches, sort + unique (the pairs, in how many bands each), min_bands, the
    exclude list, then consume(b0, u, keys, bands, err): sources [b0, b0 + len(u)) with wrapped ids u; the block's pairs as sorted
    unique keys s * N + v (s: the source's place in the block) and their band counts; err: the word the launches report into.
    Host reads: one per block of counts (the sizes), one per block with an exclude list (the size of its rows)."""
    device = index.mh_u32.device
    N, P, b = index.num_nodes, index.num_perm, index.bands
    S = src.numel()
    lk = src.to(device=device, dtype=torch.int64).contiguous()
    strict, err = eh._bounds(device, f'{what}({S} sources, num_nodes={N})')
    csr, err = _exclude_csr(ex, N, device, strict, err)
    lib = _native.lib()
    shape = (_ptr(index.mh_u32), P, index.rows, b, index.key_bits, _ptr(index.keys), _ptr(index.perm), index.max_bucket)
    cap = max(1, _LSH_BLOCK_BYTES // _LSH_ENTRY_BYTES)
    cblk = max(1, min(S, _LSH_BLOCK_BYTES // (12 * b), ((1 << 31) - 1) // b))
    for c0 in range(0, S, cblk):
        nc = min(cblk, S - c0)
        counts = torch.empty((nc * b,), dtype=torch.int32, device=device)
        with _Span('lsh_count', device):
            _native.check(lib.ss_lsh_count(c_void_p(lk.data_ptr() + 8 * c0), nc, N, *shape, _ptr(counts), _ptr(err), _stream(device)),
                          'ss_lsh_count')
        offsets = torch.zeros((nc * b + 1,), dtype=torch.int64, device=device)
        torch.cumsum(counts, 0, out=offsets[1:])
        ends = offsets[b::b].cpu().numpy()  # entries up to and including each source
        a = 0
        while a < nc:  # as many whole sources as fit the budget, one at least
            base = int(ends[a - 1]) if a else 0
            e = min(nc, max(a + 1, int(np.searchsorted(ends, base + cap, side='right'))))
            total = int(ends[e - 1]) - base
            sb = lk[c0 + a:c0 + e]
            u = torch.where(sb < 0, sb + N, sb)
            u = u.masked_fill((u < 0) | (u >= N), 0)  # (an id out of range has no entries)
            raw = torch.empty((total,), dtype=torch.int64, device=device)
            if total:
                at = offsets[a * b:e * b] - base
                with _Span('lsh_fill', device):
                    _native.check(lib.ss_lsh_fill(_ptr(sb), e - a, N, *shape, _ptr(at), _ptr(raw), _stream(device)), 'ss_lsh_fill')
            with _Span('lsh_unique', device):
                keys, bands = torch.unique(raw, return_counts=True)
                keep = bands >= min_bands
                if csr is not None and keys.numel():
                    gone = _csr_row_keys(csr, u, N)
                    if gone is not None:
                        keep &= gone[torch.searchsorted(gone, keys).clamp_(max=gone.numel() - 1)] != keys
                if min_bands > 1 or csr is not None:
                    keys, bands = keys[keep], bands[keep]
            consume(c0 + a, u, keys, bands, err)
            a = e
    if strict and S and _take_error(device):
        raise IndexError(f'sources refer to nodes outside [-{N}, {N})')


def _row_starts(keys, n, N):
    """where each of a block's n sources starts in its sorted keys s * N + v: int64 [n + 1]"""
    return torch.searchsorted(keys, torch.arange(n + 1, dtype=torch.int64, device=keys.device) * N)


def _select_rows(keys, sc, n, N, k):
    """the k best pairs of each of a block's n sources: keys = the block's sorted unique s * N + v, sc their float32 scores ->
    (ids int64 [n, k], scores float32 [n, k]) by (score desc, id asc), tails -1 / -inf (topk_links_lsh and topk_links_wedge)"""
    device = keys.device
    s = keys // N
    rank = _encode_topk_keys(sc, keys - s * N)
    by_key = torch.argsort(rank, descending=True)                  # unique inside a source: (score desc, id asc)
    order = by_key[torch.sort(s[by_key], stable=True).indices]     # ... grouped by source again
    s_o = s[order]
    place = torch.arange(keys.numel(), dtype=torch.int64, device=device) - _row_starts(keys, n, N)[s_o]
    take = place < k
    top = torch.full((n, k), TOPK_SENTINEL, dtype=torch.int64, device=device)
    top[s_o[take], place[take]] = rank[order][take]
    return _decode_topk_keys(top)


def lsh_candidates(eh, sources, index, exclude, min_bands):
    src, ex, min_bands = _arguments(eh, sources, index, exclude, min_bands)
    home, S, N = src.device, src.numel(), index.num_nodes
    device = index.mh_u32.device
    sizes = torch.zeros((S,), dtype=torch.int64, device=device)
    ids, bands = [torch.empty((0,), dtype=torch.int64, device=device)], [torch.empty((0,), dtype=torch.int32, device=device)]

    def consume(b0, u, keys, n_bands, _err):
        sizes[b0:b0 + u.numel()] = torch.diff(_row_starts(keys, u.numel(), N))
        ids.append(keys % N)
        bands.append(n_bands.to(torch.int32))

    _walk(eh, 'lsh_candidates', src, ex, index, min_bands, consume)
    rowptr = torch.zeros((S + 1,), dtype=torch.int64, device=device)
    torch.cumsum(sizes, 0, out=rowptr[1:])
    return eh._send_home(home, rowptr, torch.cat(ids), torch.cat(bands))


def topk_links_lsh(eh, sources, hash_table, cards, k, head, index, degrees, exclude, min_bands):
    eh._check_head(head, degrees)
    if cards is None:
        raise ValueError('cards must be given: the feature row needs the neighbourhood sizes build_hash_tables returns')
    src, ex, min_bands = _arguments(eh, sources, index, exclude, min_bands)
    _, _, N, P = eh._topk_arguments(src, hash_table, k, None)
    if (index.num_nodes, index.num_perm) != (N, P):
        raise ValueError(f'the index was built over a [{index.num_nodes}, {index.num_perm}] MinHash table, hash_table holds [{N}, {P}] ones')
    k = int(k)
    home, S = src.device, src.numel()
    device = index.mh_u32.device
    mh, hll, N, P = eh._resolve_tables(hash_table, device)
    params = eh._params(device)
    cd, dg, hd = eh._device_cards(cards, N, device), eh._device_degrees(degrees, N, device), head._device(device)
    mh_ptrs, hll_ptrs = _table_ptrs(mh, hll)
    ids = torch.empty((S, k), dtype=torch.int64, device=device)
    scores = torch.empty((S, k), dtype=torch.float32, device=device)

    def consume(b0, u, keys, _bands, err):
        score = eh._pair_scores(device, N, P, mh_ptrs, hll_ptrs, cd, params, dg, hd, err)
        n = u.numel()
        s = keys // N
        v = keys - s * N
        sc = score(torch.stack([u[s], v], dim=1).contiguous(), torch.empty((keys.numel(),), dtype=torch.float32, device=device))
        with _Span('lsh_select', device):
            ids[b0:b0 + n], scores[b0:b0 + n] = _select_rows(keys, sc, n, N, k)

    _walk(eh, 'topk_links_lsh', src, ex, index, min_bands, consume)
    return eh._send_home(home, ids, scores)
