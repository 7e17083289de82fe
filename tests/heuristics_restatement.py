"""The reference's CN / AA / RA (src/heuristics.py:10-70) restated in scipy, for the heuristics tests: the same expressions on the
matrix's own dtype, all links in one batch (the reference's DataLoader chunks do not change any row's sum).

    multiplier = 1 / log(A.sum(axis=0))  (AA)  |  1 / A.sum(axis=0)  (RA);   multiplier[isinf] = 0;   A_ = A.multiply(multiplier)
    scores = float32( sum over axis 1 of  A[src].multiply(A_[dst]) )          (CN: A_ = A)

On a float32 matrix scipy keeps every step in float32 and the row sum adds a row's terms in numpy's pairwise order;
`pairwise_sum_f32` states that order on its own so a test can pin it.  Also the matrices the tests feed: graphs whose pairs share
a chosen number of neighbours, and the weightings that reach the multiplier's edge cases.
"""
import numpy as np
import scipy.sparse as sp


def multiplier(A, kind):
    """np.matrix [1, N] in the dtype numpy gives (float32 for a float32 matrix, float64 for int and bool)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        m = 1 / (np.log(A.sum(axis=0)) if kind == 'AA' else A.sum(axis=0))
    m[np.isinf(m)] = 0
    return m


def scores(A, links, kind):
    """kind in {'CN', 'AA', 'RA'}; A scipy sparse; links int [L, 2] -> float32 [L] (torch.FloatTensor's cast)"""
    A = sp.csr_matrix(A)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    A_ = A if kind == 'CN' else A.multiply(multiplier(A, kind)).tocsr()
    s = np.array(np.sum(A[links[:, 0]].multiply(A_[links[:, 1]]), 1)).flatten()
    return s.astype(np.float32)


def pairwise_sum_f32(a):
    """numpy's float32 pairwise sum of a 1-d array: fewer than 8 terms in order from -0.0; up to 128 in 8 strided accumulators
    combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest in order; above 128 split at n/2 rounded down to a multiple of 8"""
    f = np.float32
    n = len(a)
    if n < 8:
        res = f(-0.0)
        for x in a:
            res = f(res + x)
        return res
    if n <= 128:
        r = [f(x) for x in a[:8]]
        i = 8
        while i < n - n % 8:
            r = [f(r[j] + a[i + j]) for j in range(8)]
            i += 8
        res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
        for x in a[i:]:
            res = f(res + x)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return f(pairwise_sum_f32(a[:n2]) + pairwise_sum_f32(a[n2:]))


def row_sum_f32(t):
    """scipy's CSR row sum of one float32 row (np.add.reduceat): the first term, plus the pairwise sum of the rest"""
    t = np.asarray(t, dtype=np.float32)
    return np.float32(0) if len(t) == 0 else np.float32(t[0] + pairwise_sum_f32(t[1:]))


# ------------------------------------------------------------------------------------------------------------------- matrices
COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 1000, 3001, 5000)


def shared_count_graph(counts=COUNTS, pool=6000, extra=40, seed=0):
    """(src, dst, links, n): pair i = (2i, 2i+1) shares exactly counts[i] neighbours drawn from a pool of `pool` column nodes
    (so its sum has counts[i] terms); both rows also hold up to `extra` columns of their own; the pool nodes link among
    themselves at random; the last two nodes are isolated.  links: every pair both ways, self pairs, pool pairs, isolated pairs"""
    rng = np.random.RandomState(seed)
    k = len(counts)
    base = 2 * k
    n = base + pool + 2
    src, dst = [], []
    for i, m in enumerate(counts):
        cols = base + rng.choice(pool, size=m + 2 * extra, replace=False)
        shared, own_u, own_v = cols[:m], cols[m:m + extra], cols[m + extra:]
        for node, c in ((2 * i, np.concatenate([shared, own_u[:rng.randint(extra + 1)]])),
                        (2 * i + 1, np.concatenate([shared, own_v[:rng.randint(extra + 1)]]))):
            src.append(np.full(len(c), node))
            dst.append(c)
    e = 20 * pool
    src.append(base + rng.randint(0, pool, size=e))
    dst.append(base + rng.randint(0, pool, size=e))
    src, dst = np.concatenate(src), np.concatenate(dst)
    pairs = np.stack([np.arange(0, base, 2), np.arange(1, base, 2)], axis=1)
    iso = np.array([[n - 2, n - 1], [n - 1, n - 1], [0, n - 2], [n - 1, 2 * (k - 1)]])
    links = np.concatenate([pairs, pairs[:, ::-1], np.repeat(np.arange(0, base, 5), 2).reshape(-1, 2), iso,
                            base + rng.randint(0, pool, size=(3000, 2)), rng.randint(0, base, size=(200, 2))])
    return src.astype(np.int64), dst.astype(np.int64), links.astype(np.int64), n


def powerlaw_graph(n, e, seed):
    """undirected power-law multigraph: node i is picked with weight (i + 1)^-0.9, so the first nodes hold thousands of entries"""
    rng = np.random.RandomState(seed)
    w = np.arange(1, n + 1, dtype=np.float64) ** -0.9
    cdf = np.cumsum(w / w.sum())
    a = np.minimum(np.searchsorted(cdf, rng.random_sample(e)), n - 1)
    b = rng.randint(0, n, size=e)
    return np.concatenate([a, b]).astype(np.int64), np.concatenate([b, a]).astype(np.int64)


def weights(kind, src, dst, n, seed):
    """float32 weights of the edges (src, dst) (duplicates are summed by csr_matrix):
    unit: all 1; random: log-uniform over 1e-3 .. 1e3; small: every column sums into (0, 1), AA multipliers negative;
    colsum_one: weights 1 / column count, so every column sums to 1 -- exactly where the count is a power of two, and there the
    AA multiplier is 1 / log(1) = inf -> 0; zeros: random, with every tenth stored entry an explicit zero"""
    rng = np.random.RandomState(seed)
    E = len(src)
    if kind == 'unit':
        return np.ones(E, dtype=np.float32)
    if kind in ('random', 'zeros'):
        return (10.0 ** rng.uniform(-3, 3, size=E)).astype(np.float32)
    cnt = np.bincount(dst, minlength=n).astype(np.float64)
    if kind == 'small':
        return (rng.uniform(0.05, 0.95, size=E) / cnt[dst]).astype(np.float32)
    if kind == 'colsum_one':
        return (1 / cnt[dst]).astype(np.float32)
    raise ValueError(kind)


def matrix(src, dst, w, n, kind=None):
    A = sp.csr_matrix((w, (src, dst)), shape=(n, n))
    if kind == 'zeros':  # stored zeros stay stored: scipy's products drop them
        A.data[::10] = 0
    return A
