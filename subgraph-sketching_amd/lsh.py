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
import torch

from . import _native
from ._runtime import _Span, _check_sizes, _compute_device, _ptr, _stream
from .candidates import _block_walk, _check_scoring, _int, _rows, _topk_rows
from .containers import HopSketch, _packed_minhash_of
from .engine import _table_shape

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


def _leading(index, sources):  # (the two launches are module-level, so that the host walk can be rehearsed without a device)
    return (_ptr(sources), sources.numel(), index.num_nodes, _ptr(index.mh_u32), index.num_perm, index.rows, index.bands, index.key_bits,
            _ptr(index.keys), _ptr(index.perm), index.max_bucket)


def _launch_count(index, sources, counts, err):
    with _Span('lsh_count', index.mh_u32.device):
        _native.check(_native.lib().ss_lsh_count(*_leading(index, sources), _ptr(counts), _ptr(err), _stream(index.mh_u32.device)), 'ss_lsh_count')


def _launch_fill(index, sources, offsets, entries):
    with _Span('lsh_fill', index.mh_u32.device):
        _native.check(_native.lib().ss_lsh_fill(*_leading(index, sources), _ptr(offsets), _ptr(entries), _stream(index.mh_u32.device)), 'ss_lsh_fill')


def _walk(eh, what, src, ex, index, min_bands):
    """candidates._block_walk over the buckets of the index, to be called with a consume: blocks of sources bounded by _LSH_BLOCK_BYTES,
    per block the count launch (a size per source and band), per group the fill launch, then sort + unique: the pairs, and in how many
    bands each; min_bands is the filter"""
    device, b = index.mh_u32.device, index.bands

    def count(_c0, sources, err):
        counts = torch.empty((sources.numel() * b,), dtype=torch.int32, device=device)
        _launch_count(index, sources, counts, err)
        offsets = torch.zeros((counts.numel() + 1,), dtype=torch.int64, device=device)
        torch.cumsum(counts, 0, out=offsets[1:])
        return offsets[b::b].cpu().numpy(), offsets

    def expand(offsets, a, e, base, total, sb, _u):
        raw = torch.empty((total,), dtype=torch.int64, device=device)
        if total:
            _launch_fill(index, sb, offsets[a * b:e * b] - base, raw)
        with _Span('lsh_unique', device):
            keys, bands = torch.unique(raw, return_counts=True)
            return keys, bands, (bands >= min_bands if min_bands > 1 else None)

    block = max(1, min(_LSH_BLOCK_BYTES // (12 * b), ((1 << 31) - 1) // b))
    room = max(1, _LSH_BLOCK_BYTES // _LSH_ENTRY_BYTES)
    return lambda consume: _block_walk(device, index.num_nodes, src, ex, eh._bounds, what, 'lsh_unique', block, room, count, expand, consume)


def lsh_candidates(eh, sources, index, exclude, min_bands):
    src, ex, min_bands = _arguments(eh, sources, index, exclude, min_bands)
    return eh._send_home(src.device, *_rows(index.mh_u32.device, src.numel(), index.num_nodes, _walk(eh, 'lsh_candidates', src, ex, index, min_bands)))


def topk_links_lsh(eh, sources, hash_table, cards, k, head, index, degrees, exclude, min_bands):
    _check_scoring(eh, cards, head, degrees)
    src, ex, min_bands = _arguments(eh, sources, index, exclude, min_bands)
    _, _, N, P = eh._topk_arguments(src, hash_table, k, None)
    if (index.num_nodes, index.num_perm) != (N, P):
        raise ValueError(f'the index was built over a [{index.num_nodes}, {index.num_perm}] MinHash table, hash_table holds [{N}, {P}] ones')
    walk = _walk(eh, 'topk_links_lsh', src, ex, index, min_bands)
    return _topk_rows(eh, src, hash_table, cards, int(k), head, degrees, index.mh_u32.device, 'lsh_select', walk)
