"""What cn_pool.common_neighbour_pool computes, restated in numpy, and the planted list its tests share.

A list is (rowptr int64 [L + 1], ids int64 [T], coef float32 [T]); entry k belongs to link owner[k], the q with rowptr[q] <= k <
rowptr[q + 1].  Both directions are the chunked sum of float32 terms given in order, chunks of C = 256:
    p_c = the sequential fp32 sum from +0 of the terms of chunk c          s = ((0 + p_0) + p_1) + ...          no terms: +0
    forward   out[q]    over k = rowptr[q] .. rowptr[q + 1] - 1, list order,          t_k = fl(coef[k] * x[ids[k]])
    backward  grad_x[n] over the entries with ids[k] == n, ascending k,               t_k = fl(coef[k] * g[owner[k]])
The product is rounded to float32 before the add.  `sequential=True` is the variant that is NOT the contract beyond one chunk: one
running sum over the whole row (what heuristics.common_neighbour_features does).  `use` (bool [T], optional) marks the entries that are
followed: one that is not keeps its place in its chunk and adds nothing.
"""
import numpy as np

C = 256


def chunked_sum(terms, sequential=False):
    """the sum of float32 terms [m, F] given in order: chunks of C summed sequentially from +0, then added in chunk order"""
    terms = np.asarray(terms, dtype=np.float32)
    s = np.zeros(terms.shape[1], dtype=np.float32)
    if sequential:
        for t in terms:
            s = s + t
        return s
    for a in range(0, len(terms), C):
        p = np.zeros(terms.shape[1], dtype=np.float32)
        for t in terms[a:a + C]:
            p = p + t  # (float32 add)
        s = s + p
    return s


def owners(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def _terms(coef, rows, use):
    t = coef[:, None] * rows  # (float32 multiply, rounded before any add)
    if use is not None:
        t[~use] = 0.0  # (+0 added to a sum begun at +0 changes no bit: the place is kept, nothing is added)
    return t


def forward_rows(rowptr, ids, coef, x_rows, links, sequential=False, use=None):
    """rows `links` of the forward, x given as a function of node ids -> float32 rows"""
    rowptr, ids, coef = np.asarray(rowptr, dtype=np.int64), np.asarray(ids, dtype=np.int64), np.asarray(coef, dtype=np.float32)
    out = []
    for q in links:
        k = np.arange(rowptr[q], rowptr[q + 1])
        safe = ids[k] if use is None else np.where(use[k], ids[k], 0)
        out.append(chunked_sum(_terms(coef[k], np.asarray(x_rows(safe), dtype=np.float32), None if use is None else use[k]), sequential))
    return np.stack(out)


def forward(rowptr, ids, coef, x, sequential=False, use=None):
    """out float32 [L, F]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    L = len(rowptr) - 1
    if L == 0:
        return np.zeros((0, x.shape[1]), dtype=np.float32)
    return forward_rows(rowptr, ids, coef, lambda i: x[i].reshape(len(i), x.shape[1]), range(L), sequential, use)


def grad_rows(rowptr, ids, coef, g_rows, nodes, F, sequential=False, use=None):
    """rows `nodes` of the backward, g given as a function of link ids -> float32 rows"""
    ids, coef, own = np.asarray(ids, dtype=np.int64), np.asarray(coef, dtype=np.float32), owners(rowptr)
    out = []
    for n in nodes:
        k = np.nonzero(ids == n)[0]  # ascending
        safe = own[k] if use is None else np.where(use[k], own[k], 0)
        rows = np.asarray(g_rows(safe), dtype=np.float32).reshape(len(k), F)
        out.append(chunked_sum(_terms(coef[k], rows, None if use is None else use[k]), sequential))
    return np.stack(out) if out else np.zeros((0, F), dtype=np.float32)


def grad(rowptr, ids, coef, g, N, sequential=False, use=None):
    """grad_x float32 [N, F] of <forward(x), g>; rows no entry names are zeros"""
    g = np.ascontiguousarray(g, dtype=np.float32)
    F = g.shape[1]
    out = np.zeros((N, F), dtype=np.float32)
    named = np.unique(np.asarray(ids, dtype=np.int64))
    named = named[(named >= 0) & (named < N)]
    if len(named):
        out[named] = grad_rows(rowptr, ids, coef, lambda i: g[i], named, F, sequential, use)
    return out


def dense(rowptr, ids, coef, N):
    """S float64 [L, N] with S[q, n] = the sum of the coefficients of link q's entries that name n: forward = S @ x, backward = S^T @ g"""
    S = np.zeros((len(rowptr) - 1, N))
    np.add.at(S, (owners(rowptr), np.asarray(ids, dtype=np.int64)), np.asarray(coef, dtype=np.float64))
    return S


def grouping(ids, N):
    """(nodes int64 [M], rowptr int64 [M + 1], order int64 [T]): the entries of every named node, nodes ascending, entries ascending
    inside a node"""
    ids = np.asarray(ids, dtype=np.int64)
    order = np.argsort(ids, kind='stable')
    m = np.bincount(ids, minlength=N)
    nodes = np.nonzero(m)[0]
    return nodes.astype(np.int64), np.concatenate([[0], np.cumsum(m[nodes])]).astype(np.int64), order.astype(np.int64)


# ---- the planted list -------------------------------------------------------------------------------------------------------------
# N nodes.  Three kinds of links:
#   row links     one per entry of ROW_COUNTS, with that many entries, all naming pool nodes (nodes that are no target): the link rows
#                 on both sides of the four-ahead request group (4), of the lane-stretch steps (16, 64), of the chunk (256, with 258:
#                 a second chunk of two entries) and of two and four chunks
#   spread links  SPREAD of them; spread link j names every target node NODES[k] with COUNTS[k] > j, so that NODES[k] is named by
#                 exactly COUNTS[k] entries of COUNTS[k] DIFFERENT links (1 025 for the last one): the node groups of the backward
#   the repeat link   one link of REPEAT entries that all name REPEAT_NODE: ids repeat inside a row
# Row order: the 1 025-entry row first, the 512-entry row last, the 513-entry row between two empty rows; L is odd.
N = 3000
COUNTS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 258, 512, 513, 1025)
ROW_COUNTS = COUNTS
NODES = tuple([7] + [1 + 150 * k for k in range(1, 18)] + [N - 1])  # (7: the target no entry names; N - 1: the last id)
SPREAD, REPEAT, REPEAT_NODE = 1025, 300, 2950
UNNAMED = 0  # node 0 is named by nothing: what a stand-in load reads must not matter


def planted(seed=13, coefficients='random'):
    """(rowptr int64 [L + 1], ids int64 [T], coef float32 [T]).  coefficients: 'random' (uniform in [0.25, 2), every 97th one 0 and
    every 89th one negative) or 'unit'"""
    rng = np.random.RandomState(seed)
    pool = np.setdiff1d(np.arange(1, N), list(NODES) + [REPEAT_NODE])
    row_links = {m: pool[(31 * m + 7 * np.arange(m)) % len(pool)] for m in ROW_COUNTS}
    spread = []
    for j in range(SPREAD):
        named = np.array([v for v, c in zip(NODES, COUNTS) if c > j], dtype=np.int64)
        spread.append(named[rng.permutation(len(named))])  # (list order inside a row is free: ids need not ascend)
    middle = [row_links[m] for m in ROW_COUNTS if m not in (0, 1025, 513, 512)] + spread + [np.full(REPEAT, REPEAT_NODE, dtype=np.int64)]
    middle = [middle[i] for i in rng.permutation(len(middle))]
    empty = np.zeros(0, dtype=np.int64)
    rows = [row_links[1025], empty, row_links[513], empty] + middle[:400] + [empty] + middle[400:] + [row_links[512]]
    assert len(rows) % 2 == 1
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int64)
    if coefficients == 'unit':
        coef = np.ones(len(ids), dtype=np.float32)
    else:
        coef = rng.uniform(0.25, 2.0, size=len(ids)).astype(np.float32)
        coef[::97] = 0.0
        coef[5::89] *= -1.0
    return rowptr, ids, coef


def features(n, F, seed=3):
    return np.random.RandomState(seed).standard_normal((n, F)).astype(np.float32)
