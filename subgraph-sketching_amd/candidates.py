"""What the candidate queries (lsh.py: LSH buckets; wedge.py: two-hop walks) share on the host: the walk over blocks of sources with
the exclude list, its two consumers -- rows, and the k best per source by the structure head -- and argument checks.  A candidate
source supplies the generator that _block_walk describes, nothing else.  Design: DESIGN 3.14, "host walk"."""
import numpy as np
import torch

from ._runtime import _Span, _take_error
from .engine import TOPK_SENTINEL, _csr_row_keys, _decode_topk_keys, _encode_topk_keys, _exclude_csr, _table_ptrs


def _int(value, name, lo, hi=None):
    try:
        v = int(value)
    except (TypeError, ValueError):
        raise ValueError(f'{name} must be an integer, got {value!r}')
    if v != value or v < lo or (hi is not None and v > hi):
        raise ValueError(f'{name} must lie in [{lo}, {hi if hi is not None else "..."}], got {value!r}')
    return v


def _id_list(sources, what='sources'):
    src = torch.as_tensor(sources)
    if src.dim() != 1 or src.dtype.is_floating_point or src.dtype == torch.bool:
        raise ValueError(f'{what} must be a 1-D integer tensor, got {src.dtype} {tuple(src.shape)}')
    return src


def _check_host_ids(src, N, what='sources'):
    """CPU ids are checked before a device is touched; device ids are reported late (strict_bounds)"""
    if not src.is_cuda and src.numel() and (int(src.min()) < -N or int(src.max()) >= N):
        raise IndexError(f'{what} refer to nodes outside [-{N}, {N})')


def _block_walk(device, N, src, ex, bounds, what, span, block, room, count, expand, consume):
    """the walk every candidate query shares.  Sources go in blocks of at most `block`; count(c0, sources, err) -> (ends, state) is a
    block's size launch and its ONE host read: ends = numpy int64, the entries up to and including each source.  As many whole sources
    as fit `room` entries (one at least) form a group; expand(state, a, e, base, total, sb, u) -> (keys, counts, keep) lists sources
    [a, e) of the block (sb as given; u wrapped, an id out of range 0: it has no entries), `total` entries from `base` on, as sorted
    unique keys s * N + v (s: the source's place in the group) with a count each; keep = the generator's own filter as a mask, or None.
    The exclude list leaves the mask (under `span`); consume(b0, u, keys, counts, err) takes sources [b0, b0 + len(u)), err = the word
    the launches report into.  Host reads: that per block, one per group with an exclude list (its rows' size), the strict check."""
    S = src.numel()
    lk = src.to(device=device, dtype=torch.int64).contiguous()
    strict, err = bounds(device, f'{what}({S} sources, num_nodes={N})')
    csr, err = _exclude_csr(ex, N, device, strict, err)
    for c0 in range(0, S, block):
        ends, state = count(c0, lk[c0:c0 + block], err)
        a, nc = 0, len(ends)
        while a < nc:  # as many whole sources as fit the budget, one at least
            base = int(ends[a - 1]) if a else 0
            e = min(nc, max(a + 1, int(np.searchsorted(ends, base + room, side='right'))))
            sb = lk[c0 + a:c0 + e]
            u = torch.where(sb < 0, sb + N, sb)
            u = u.masked_fill((u < 0) | (u >= N), 0)
            keys, counts, keep = expand(state, a, e, base, int(ends[e - 1]) - base, sb, u)
            with _Span(span, device):
                if csr is not None and keys.numel():
                    gone = _csr_row_keys(csr, u, N)
                    if gone is not None:
                        free = gone[torch.searchsorted(gone, keys).clamp_(max=gone.numel() - 1)] != keys
                        keep = free if keep is None else keep & free
                if keep is not None:
                    keys, counts = keys[keep], counts[keep]
            consume(c0 + a, u, keys, counts, err)
            a = e
    if strict and S and _take_error(device):
        raise IndexError(f'sources refer to nodes outside [-{N}, {N})')


def _row_starts(keys, n, N):
    """where each of a group's n sources starts in its sorted keys s * N + v: int64 [n + 1]"""
    return torch.searchsorted(keys, torch.arange(n + 1, dtype=torch.int64, device=keys.device) * N)


def _select_rows(keys, sc, n, N, k):
    """the k best pairs of each of a group's n sources: keys = the group's sorted unique s * N + v, sc their float32 scores ->
    (ids int64 [n, k], scores float32 [n, k]) by (score desc, id asc), tails -1 / -inf"""
    s = keys // N
    rank = _encode_topk_keys(sc, keys - s * N)
    by_key = torch.argsort(rank, descending=True)                  # unique inside a source: (score desc, id asc)
    order = by_key[torch.sort(s[by_key], stable=True).indices]     # ... grouped by source again
    s_o = s[order]
    place = torch.arange(keys.numel(), dtype=torch.int64, device=keys.device) - _row_starts(keys, n, N)[s_o]
    take = place < k
    top = torch.full((n, k), TOPK_SENTINEL, dtype=torch.int64, device=keys.device)
    top[s_o[take], place[take]] = rank[order][take]
    return _decode_topk_keys(top)


def _rows(device, S, N, walk):
    """what walk(consume) lists, as (rowptr int64 [S + 1], ids int64 [T], counts int32 [T]) on the compute device"""
    sizes = torch.zeros((S,), dtype=torch.int64, device=device)
    ids, counts = [torch.empty((0,), dtype=torch.int64, device=device)], [torch.empty((0,), dtype=torch.int32, device=device)]

    def consume(b0, u, keys, n, _err):
        sizes[b0:b0 + u.numel()] = torch.diff(_row_starts(keys, u.numel(), N))
        ids.append(keys % N)
        counts.append(n.to(torch.int32))

    walk(consume)
    rowptr = torch.zeros((S + 1,), dtype=torch.int64, device=device)
    torch.cumsum(sizes, 0, out=rowptr[1:])
    return rowptr, torch.cat(ids), torch.cat(counts)


def _check_scoring(eh, cards, head, degrees):
    eh._check_head(head, degrees)
    if cards is None:
        raise ValueError('cards must be given: the feature row needs the neighbourhood sizes build_hash_tables returns')


def _topk_rows(eh, src, hash_table, cards, k, head, degrees, device, span, walk):
    """what walk(consume) lists, scored by the head, the k best per source: (ids int64 [S, k], scores float32 [S, k]) on src.device, tails -1 / -inf"""
    mh, hll, N, P = eh._resolve_tables(hash_table, device)
    params = eh._params(device)
    cd, dg, hd = eh._device_cards(cards, N, device), eh._device_degrees(degrees, N, device), head._device(device)
    mh_ptrs, hll_ptrs = _table_ptrs(mh, hll)
    ids = torch.empty((src.numel(), k), dtype=torch.int64, device=device)
    scores = torch.empty((src.numel(), k), dtype=torch.float32, device=device)

    def consume(b0, u, keys, _counts, err):
        score = eh._pair_scores(device, N, P, mh_ptrs, hll_ptrs, cd, params, dg, hd, err)
        n = u.numel()
        s = keys // N
        sc = score(torch.stack([u[s], keys - s * N], dim=1).contiguous(), torch.empty((keys.numel(),), dtype=torch.float32, device=device))
        with _Span(span, device):
            ids[b0:b0 + n], scores[b0:b0 + n] = _select_rows(keys, sc, n, N, k)

    walk(consume)
    return eh._send_home(src.device, ids, scores)
