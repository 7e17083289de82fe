"""What aggr.aggregate computes, restated in numpy, and the planted directed graph the aggregation tests share.

Output row i of a product takes the edges e grouped at i (flow='target': col_e == i, the value comes from row_e; flow='source': the
other way round), ascending, in chunks of C = 256:
    p_c = the sequential fp32 sum from +0 of the terms of chunk c          s = ((0 + p_0) + p_1) + ...          no entries: +0
    term t_e = fl(w_e * v_e) (unit weights: v_e * 1, the same bits),  v_e = x[src_e]
    mean:  out_i = fl(s / den_i), den_i the same chunked sum over w_e alone (1 where the row has no entries)
    root:  out_i += fl(r * x_i)
A row of at most 256 entries is the plain sequential sum: those rows are oracle.spmm's (the sequential fp32 scatter-add in edge order,
product and add rounded separately); longer rows are an explicit float32 loop.  The gradient with respect to x of a product is the
other flow's SUM product of g (mean: of g' = fl(g / den), den the forward's) with the same root term applied to g.
"""
import numpy as np

from oracle import oracle

import gcn_restatement as gr

C = 256
OTHER = {'target': 'source', 'source': 'target'}


def _ends(edge_index, flow):
    """(dst, src): where every edge's term arrives and where its value comes from"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    return (ei[1], ei[0]) if flow == 'target' else (ei[0], ei[1])


def chunked_sum(terms):
    """the contract's sum of float32 terms [m, F] given in order: chunks of C summed sequentially from +0, then added in chunk order"""
    s = np.zeros(terms.shape[1], dtype=np.float32)
    for a in range(0, len(terms), C):
        p = np.zeros(terms.shape[1], dtype=np.float32)
        for t in terms[a:a + C]:
            p = p + t  # (float32 add)
        s = s + p
    return s


def sum_product(edge_index, w, n, x, flow):
    """the SUM product, float32 [n, F]: rows of at most C entries through oracle.spmm, the others through chunked_sum.
    w None: unit weights (a multiplication by 1 leaves the bits alone, so oracle.spmm with ones is the same product)"""
    dst, src = _ends(edge_index, flow)
    x = np.ascontiguousarray(x, dtype=np.float32)
    wv = np.ones(len(dst), dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    m = np.bincount(dst, minlength=n)
    small = m[dst] <= C
    out = oracle.spmm(np.stack([dst[small], src[small]]), wv[small], n, x)
    for i in np.nonzero(m > C)[0]:
        e = np.nonzero(dst == i)[0]  # ascending edge indices
        out[i] = chunked_sum(x[src[e]] * wv[e][:, None])
    return out


def den(edge_index, w, n, flow):
    """float32 [n]: the chunked sum of the weights arriving at every node (unit weights: the count), 1 for a node without entries"""
    dst, _ = _ends(edge_index, flow)
    d = sum_product(edge_index, w, n, np.ones((n, 1), dtype=np.float32), flow)[:, 0]
    d[np.bincount(dst, minlength=n) == 0] = 1
    return d


def aggregate(edge_index, w, n, x, flow, aggr='sum', root=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = sum_product(edge_index, w, n, x, flow)
    if aggr == 'mean':
        out = out / den(edge_index, w, n, flow)[:, None]  # (float32 division, correctly rounded)
    if root is not None:
        out = out + np.float32(root) * x
    return out


def aggregate_grad(edge_index, w, n, g, flow, aggr='sum', root=None):
    """the gradient with respect to x of <aggregate(x, flow, aggr, root), g>, in the arithmetic of the backward"""
    g = np.ascontiguousarray(g, dtype=np.float32)
    gd = g / den(edge_index, w, n, flow)[:, None] if aggr == 'mean' else g
    out = sum_product(edge_index, w, n, gd, OTHER[flow])
    if root is not None:
        out = out + np.float32(root) * g
    return out


def propagate_rows(edge_index, w, n, x_rows, rows, flow, aggr='sum', root=None):
    """rows `rows` of aggregate(...) for an x given as a function node ids -> float32 [len, F] (the large-offset test: x itself is
    never held on the host): the same chunked sum, evaluated for the sampled rows only"""
    dst, src = _ends(edge_index, flow)
    order = np.argsort(dst, kind='stable')
    starts = np.searchsorted(dst[order], rows, side='left')
    ends = np.searchsorted(dst[order], rows, side='right')
    out = []
    for i, a, b in zip(rows, starts, ends):
        e = order[a:b]
        xs = x_rows(src[e])
        wv = np.ones(len(e), dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)[e]
        s = chunked_sum(xs * wv[:, None]) if len(e) else np.zeros(x_rows(np.array([i])).shape[1], dtype=np.float32)
        if aggr == 'mean':
            d = chunked_sum(wv[:, None])[0] if len(e) else np.float32(1)
            s = s / d
        if root is not None:
            s = s + np.float32(root) * x_rows(np.array([i]))[0]
        out.append(s.astype(np.float32))
    return np.stack(out)


def dense(edge_index, w, n):
    """float64 [n, n] A with A[row_e, col_e] += w_e (flow='source' is A @ x, 'target' A.T @ x), |A| accumulated the same way, and
    the entries per row of A and of A.T"""
    ei = np.asarray(edge_index, dtype=np.int64)
    wv = np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    A = np.zeros((n, n), dtype=np.float64)
    M = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (ei[0], ei[1]), wv)
    np.add.at(M, (ei[0], ei[1]), np.abs(wv))
    return A, M, np.bincount(ei[0], minlength=n), np.bincount(ei[1], minlength=n)


# ---- the planted graph ------------------------------------------------------------------------------------------------------------
# gcn_restatement.planted (601 nodes: rows of 0 .. 300 entries, duplicates, the node with two self loops -- which COUNT here, like
# every self loop) extended to N nodes with rows of exactly BIG[k] entries at node HUBS[k], in BOTH directions: in-entries from and
# out-entries to the pool POOL0 .. POOL0 + POOL - 1 (2305 > POOL: the longest row repeats sources, duplicates count once per copy).
N = 3001  # not a multiple of any rows-per-wave (1, 2, 4, ... 64)
BIG = (257, 255, 256, 511, 512, 513, 767, 769, 1024, 2305, 1025)
HUBS = (0, 700, 701, 710, 720, 730, 740, 750, 760, 770, N - 1)  # the first and the last node id; 700 and 701 side by side
POOL0, POOL = 1000, 1999


def planted(weights, seed=11):
    """(edge_index int64 [2, E], w float32 [E]) on N nodes, the edges in a seeded random order.  weights: 'unit' or 'random'
    (uniform in [0.25, 2); the planted loop weights of gcn_restatement.planted are kept, except the self loop of weight 0 at an
    otherwise isolated node, which gets 0.75: a den of 0 makes the mean 0 / 0, whose NaN has no agreed bits)"""
    ei0, w0 = gr.planted(weights)
    if weights != 'unit':
        w0[(ei0[0] == gr.ZERO_LOOP) & (ei0[1] == gr.ZERO_LOOP)] = 0.75
    rng = np.random.RandomState(seed)
    have_in, have_out = np.bincount(ei0[1], minlength=N), np.bincount(ei0[0], minlength=N)
    src, dst = [], []
    for node, d in zip(HUBS, BIG):
        k = d - have_in[node]
        src += list(POOL0 + (7 * node + np.arange(k)) % POOL)
        dst += [node] * k
        k = d - have_out[node]
        src += [node] * k
        dst += list(POOL0 + (5 * node + 3 + np.arange(k)) % POOL)
    extra = np.array([src, dst], dtype=np.int64)
    we = np.ones(extra.shape[1], dtype=np.float32) if weights == 'unit' else rng.uniform(0.25, 2.0, size=extra.shape[1]).astype(np.float32)
    ei, w = np.concatenate([ei0, extra], axis=1), np.concatenate([w0, we])
    perm = rng.permutation(ei.shape[1])
    return np.ascontiguousarray(ei[:, perm]), np.ascontiguousarray(w[perm])


def features(n, F, seed=3):
    return np.random.RandomState(seed).standard_normal((n, F)).astype(np.float32)
