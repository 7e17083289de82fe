"""What gcn.gcn_propagate computes, restated with the oracle's two functions, and the planted directed graph the GCN tests share.

  flow='source' (torch_sparse.spmm, sign.py):  oracle.spmm(ei2, wn, n, x)          out[row_e] += wn_e * x[col_e]
  flow='target' (GCNConv's default flow):      oracle.spmm(ei2[[1, 0]], wn, n, x)  out[col_e] += wn_e * x[row_e]
with (ei2, wn) = oracle.gcn_norm(edge_index, w, n): existing self loops removed, one loop per node appended BEHIND all other edges,
wn = dinv[row] * w * dinv[col] left to right in fp32.  oracle.spmm is the sequential fp32 scatter-add in edge order, product and add
rounded separately -- exactly the kernels' contract (one lane per output element, ascending edge order, the loop last), so the GPU
comparisons are bit for bit.  Each flow is the other's gradient with respect to x.
"""
import numpy as np

from oracle import oracle

N = 601  # not a multiple of any rows-per-wave (1, 2, 4, ... 64)
PROFILE = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129, 300)  # entries per row: around the 4-ahead batches and the 16 / 64-lane stretches
IN_NODES = tuple(range(10, 10 + len(PROFILE)))   # node 10 + k has in-degree PROFILE[k] and no out-edges
OUT_NODES = tuple(range(40, 40 + len(PROFILE)))  # node 40 + k has out-degree PROFILE[k] and no in-edges
TWO_LOOPS, ZERO_LOOP = 560, 570


def norm(edge_index, w, n):
    return oracle.gcn_norm(edge_index, np.asarray(w, dtype=np.float32), n)


def propagate(edge_index, w, n, x, flow):
    ei2, wn = norm(edge_index, w, n)
    index = ei2 if flow == 'source' else ei2[[1, 0]]
    return oracle.spmm(index, wn, n, np.ascontiguousarray(x, dtype=np.float32))


def propagate_rows(edge_index, w, n, x_rows, rows, flow):
    """rows `rows` of propagate(...) for an x given as a function node ids -> float32 [len, F] (the large-offset test: x itself is
    never held on the host).  The same sequential sum, evaluated for the sampled rows only."""
    ei2, wn = norm(edge_index, w, n)
    dst, src = (ei2[0], ei2[1]) if flow == 'source' else (ei2[1], ei2[0])
    order = np.argsort(dst, kind='stable')
    starts = np.searchsorted(dst[order], rows, side='left')
    ends = np.searchsorted(dst[order], rows, side='right')
    out = []
    for a, b in zip(starts, ends):
        e = order[a:b]
        xs = x_rows(src[e])
        acc = np.zeros(xs.shape[1], dtype=np.float32)
        for k in range(len(e)):
            acc = acc + xs[k] * wn[e[k]]  # (float32 product, float32 add: rounded separately)
        out.append(acc)
    return np.stack(out)


def dense(edge_index, w, n):
    """float64 [n, n] A with A[row_e, col_e] += wn_e, the fp32 norms taken as exact numbers (flow='source' is A @ x, 'target' A.T @ x),
    |A| accumulated the same way, and the entries per row of A (out-degree + 1) and of A.T (in-degree + 1)"""
    ei2, wn = norm(edge_index, w, n)
    A = np.zeros((n, n), dtype=np.float64)
    M = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (ei2[0], ei2[1]), wn.astype(np.float64))
    np.add.at(M, (ei2[0], ei2[1]), np.abs(wn.astype(np.float64)))
    return A, M, np.bincount(ei2[0], minlength=n), np.bincount(ei2[1], minlength=n)


def planted(weights, seed=7):
    """(edge_index int64 [2, E], w float32 [E]) on N nodes: in- and out-degrees PROFILE at IN_NODES / OUT_NODES, duplicate edges, a node
    with two explicit self loops (weights 2.0 then 0.5: the last one wins), an otherwise isolated node with a self loop of weight 0
    (degree 0: dinv inf -> 0), directed (A != A.T), the edges in a seeded random order.  weights: 'unit' (every weight 1, the planted
    loop weights too: the kernels' fast path) or 'random' (uniform in [0.25, 2))."""
    rng = np.random.RandomState(seed)
    src, dst = [], []
    for node, d in zip(IN_NODES, PROFILE):
        src += list(100 + np.arange(d))  # distinct sources 100 .. 399
        dst += [node] * d
    for node, d in zip(OUT_NODES, PROFILE):
        src += [node] * d
        dst += list(200 + np.arange(d))  # distinct targets 200 .. 499
    src += [500, 500, 500, 501, 502, 502]  # duplicates
    dst += [501, 501, 501, 500, 503, 503]
    src += [TWO_LOOPS, TWO_LOOPS, TWO_LOOPS, 562, ZERO_LOOP]
    dst += [TWO_LOOPS, TWO_LOOPS, 561, TWO_LOOPS, ZERO_LOOP]
    src += [N - 1, 0, N - 1, 599]  # the first and the last row take part
    dst += [0, N - 1, 599, N - 1]
    ei = np.array([src, dst], dtype=np.int64)[:, rng.permutation(len(src))]
    E = ei.shape[1]
    if weights == 'unit':
        w = np.ones(E, dtype=np.float32)
    else:
        assert weights == 'random'
        w = rng.uniform(0.25, 2.0, size=E).astype(np.float32)
        two = np.nonzero((ei[0] == TWO_LOOPS) & (ei[1] == TWO_LOOPS))[0]
        w[two] = (2.0, 0.5)  # in edge order
        w[(ei[0] == ZERO_LOOP) & (ei[1] == ZERO_LOOP)] = 0.0
    return ei, w


def features(n, F, seed=3):
    return np.random.RandomState(seed).standard_normal((n, F)).astype(np.float32)
