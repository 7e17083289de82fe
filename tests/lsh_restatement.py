"""The semantics of ElphHashes.build_lsh_index / lsh_candidates restated in numpy, from the reference-shaped int64 rows
table[hop]['minhash'] alone.  Shares no code with the engine: no sort key, no binary search -- the nodes of a band are grouped by
exact equality of their slices (value by value, np.unique over exact integer pairs).

    band j of v          minhash[v][j * rows : (j + 1) * rows]
    bucket of (j, v)     all nodes whose band-j slice equals v's; one of more than max_bucket members is skipped: it yields nothing
    candidates of u      every v != u with (u -> v) not in `exclude` that shares a non-skipped bucket with u in >= min_bands bands
    bands[u, v]          the number of such bands
"""
import numpy as np


def band_groups(minhash, rows, bands=None):
    """per band: (group id of every node int64 [N], size of every group int64 [G])"""
    mh = np.asarray(minhash)
    N, P = mh.shape
    b = P // rows if bands is None else bands
    assert rows >= 1 and b >= 1 and rows * b <= P
    out = []
    assert mh.min() >= 0 and mh.max() < (1 << 32) and N < (1 << 31)
    for j in range(b):
        # exact grouping, one value of the slice at a time: (group so far, next value) is one int64 without loss
        group = np.zeros(N, dtype=np.int64)
        for c in range(j * rows, (j + 1) * rows):
            _, group = np.unique((group << 32) | mh[:, c].astype(np.int64), return_inverse=True)
            group = group.reshape(-1).astype(np.int64)
        out.append((group, np.bincount(group).astype(np.int64)))
    return out


def skipped_buckets(minhash, rows, bands=None, max_bucket=1024):
    """int64 [bands]: the buckets of more than max_bucket members"""
    return np.array([int((sizes > max_bucket).sum()) for _, sizes in band_groups(minhash, rows, bands)], dtype=np.int64)


def shared_bands(minhash, sources, rows, bands=None, max_bucket=1024):
    """int32 [S, N]: in how many bands node v shares a non-skipped bucket with sources[s] (negative ids wrapped; the source's own
    column is left as counted)"""
    N = np.asarray(minhash).shape[0]
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    src = np.where(src < 0, src + N, src)
    distinct, place = np.unique(src, return_inverse=True)
    shared = np.zeros((len(distinct), N), dtype=np.int32)
    for group, sizes in band_groups(minhash, rows, bands):
        mine = group[distinct]
        kept = sizes[mine] <= max_bucket
        shared += (group[None, :] == mine[:, None]) & kept[:, None]
    return shared[place.reshape(-1)]


def lsh_candidates(minhash, sources, rows, bands=None, max_bucket=1024, exclude=None, min_bands=1):
    """(rowptr int64 [S + 1], ids int64 [T], bands int32 [T]): row s = the candidates of sources[s], ascending"""
    N = np.asarray(minhash).shape[0]
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    src = np.where(src < 0, src + N, src)
    shared = shared_bands(minhash, src, rows, bands, max_bucket) if len(src) else np.zeros((0, N), dtype=np.int32)
    ok = shared >= min_bands
    ok[np.arange(len(src)), src] = False
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64).reshape(2, -1)
        ex = np.where(ex < 0, ex + N, ex)
        for s, u in enumerate(src):
            ok[s, ex[1][ex[0] == u]] = False
    rowptr = np.zeros(len(src) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(ok.sum(axis=1))
    s_of, ids = np.nonzero(ok)
    return rowptr, ids.astype(np.int64), shared[s_of, ids].astype(np.int32)


def trailing_graph(n_ring=20, m=10):
    """(N, edge_index, m): a ring with chords over nodes 0 .. n_ring - 1 and m trailing nodes at and above max(edge_index) + 1: no edge
    and no self loop, so they share ONE row in every hop table"""
    a = np.arange(n_ring, dtype=np.int64)
    e = np.concatenate([np.stack([a, (a + 1) % n_ring]), np.stack([a[::3], (a[::3] + 7) % n_ring])], axis=1)
    return n_ring + m, np.concatenate([e, e[::-1]], axis=1), m
