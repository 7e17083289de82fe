"""numpy restatement of graph_prep (coalesce / to_undirected / coalesce_graph / is_symmetric): the sorted order by np.lexsort with the
position as last key, the accumulation order as explicit loops in the value's own dtype under the chunk rule, the NaN and zero rules
of min / max.  Nothing here calls the library."""
import numpy as np

CHUNK = 256
OPS = ('add', 'mean', 'min', 'max')


def sorted_positions(row, col):
    """the positions of the list sorted by (row, col, position)"""
    return np.lexsort((np.arange(len(row)), col, row))  # (lexsort: the LAST key is the primary one)


def sorted_positions_two_groupings(row, col):
    """the same order as the library composes it: two stable groupings, least significant key first"""
    oc = np.argsort(col, kind='stable')
    o2 = np.argsort(row[oc], kind='stable')
    return oc[o2]


def run_starts(row, col, perm):
    """int64 [E' + 1]: the sorted positions at which a new (row, col) pair starts, then E"""
    E = len(perm)
    if E == 0:
        return np.zeros(1, dtype=np.int64)
    r, c = row[perm], col[perm]
    head = np.ones(E, dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    return np.concatenate([np.flatnonzero(head), [E]]).astype(np.int64)


def _nan(dtype):
    return np.array(np.nan, dtype=dtype)[()]


def _step(acc, x, op):
    """one step of a fold in the dtype of acc (a NaN never wins a comparison: _finish looks for them)"""
    if op in ('add', 'mean'):
        with np.errstate(over='ignore'):
            return acc + x
    if op == 'min':
        return x if x < acc else acc  # strict: of equal values (-0.0, +0.0) the one listed first stays
    return x if x > acc else acc


def fold_sequential(values, op):
    """the plain loop over a run in list order, WITHOUT the chunk rule"""
    acc = values[0]
    for x in values[1:]:
        acc = _step(acc, x, op)
    return acc


def fold_loop(values, op, chunk=CHUNK):
    """THE DEFINITION: the run cut into chunks of `chunk` entries from its start, every chunk folded sequentially from its first entry,
    the chunk results folded in chunk order; then mean's division / the NaN rule.  values: 1-d array of the run in list order."""
    values = np.asarray(values)
    dtype, n = values.dtype, len(values)
    total = None
    for c0 in range(0, n, chunk):
        part = fold_sequential(values[c0:c0 + chunk], op)
        total = part if total is None else _step(total, part, op)
    return _finish(total, values, op, dtype, n)


def _finish(total, values, op, dtype, n):
    if op == 'mean':
        if dtype == np.int64:
            return np.int64(int(total) // n)  # floor division, as PyG's scatter does
        return (total / dtype.type(n)).astype(dtype)
    if op in ('min', 'max') and dtype != np.int64 and np.isnan(values).any():
        return _nan(dtype)
    return dtype.type(total)


def fold(values, op, chunk=CHUNK):
    """fold_loop without the interpreter loop: np.add.accumulate adds strictly left to right in the array's dtype, np.argmin / argmax
    return the FIRST extreme (test_graph_prep_host checks the two against each other)"""
    values = np.asarray(values)
    dtype, n = values.dtype, len(values)
    if op in ('min', 'max'):
        if dtype != np.int64 and np.isnan(values).any():
            return _nan(dtype)
        return values[np.argmin(values) if op == 'min' else np.argmax(values)]
    with np.errstate(over='ignore'):
        parts = np.array([np.add.accumulate(values[c0:c0 + chunk], dtype=dtype)[-1] for c0 in range(0, n, chunk)], dtype=dtype)
        total = np.add.accumulate(parts, dtype=dtype)[-1]
    return _finish(total, values, op, dtype, n)


def coalesce(row, col, value, N, op='add', chunk=CHUNK, fold_fn=fold):
    """-> dict(row, col int64 [E'], value [E'] or None, count int32 [E'], rowptr int64 [N + 1], perm, starts)"""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    if len(row) and (min(row.min(), col.min()) < 0 or max(row.max(), col.max()) >= N):
        raise IndexError('ids outside [0, N)')
    perm = sorted_positions(row, col)
    starts = run_starts(row, col, perm)
    heads = perm[starts[:-1]]
    out_row, out_col = row[heads], col[heads]
    count = np.diff(starts).astype(np.int32)
    out_value = None
    if value is not None:
        value = np.asarray(value)
        ordered = value[perm]
        out_value = np.array([fold_fn(ordered[a:b], op, chunk) for a, b in zip(starts[:-1], starts[1:])], dtype=value.dtype)
    rowptr = np.searchsorted(out_row, np.arange(N + 1), side='left').astype(np.int64)
    return dict(row=out_row, col=out_col, value=out_value, count=count, rowptr=rowptr, perm=perm, starts=starts)


def to_undirected(row, col, value, N, op='add'):
    """the list followed by the list reversed, the values doubled, coalesced"""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    return coalesce(np.concatenate([row, col]), np.concatenate([col, row]), None if value is None else np.concatenate([value, value]), N, op)


def is_symmetric(out, weights=True):
    """whether every pair (u, v) of a coalesce() result has its pair (v, u), with weights=True of the same value (NaN equal to NaN)"""
    pairs = {(int(u), int(v)): k for k, (u, v) in enumerate(zip(out['row'], out['col']))}
    for (u, v), k in pairs.items():
        j = pairs.get((v, u))
        if j is None:
            return False
        if weights and out['value'] is not None:
            a, b = out['value'][k], out['value'][j]
            if not (a == b or (a != a and b != b)):
                return False
    return True
