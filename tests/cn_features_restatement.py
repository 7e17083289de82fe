"""heuristics.common_neighbours / common_neighbour_features restated in numpy, for the tests of csrc/ss_cn_pool.hip.

    members(u, v) = np.intersect1d of the column ids of rows u and v of the canonical CSR (sorted, duplicate-free; stored zeros stay)
    c(u, v, w)    = float32( A[u, w] * (A[v, w] * mult[w]) )   in fp64 with this association, one rounding
    pooled(u, v)  = the loop  acc = acc + c[k] * x[w_k]  in float32 over ascending w, from +0.0 (numpy rounds product and sum apart)

The multiplier is the one DeviceAdjacency.multiplier forms: the reference's numpy expression on the matrix's dtype, widened to fp64.
The planted graphs are those of tests/heuristics_restatement.py.  No test lives here.
"""
import numpy as np
import scipy.sparse as sp


def canonical(A):
    A = sp.csr_matrix(A)
    if not A.has_canonical_format:
        A = A.copy()
        A.sum_duplicates()
    return A


def multiplier(A, weighting):
    """fp64 [N] or None: None / 'CN' -> None; 'AA' / 'RA' -> 1 / log(colsum) | 1 / colsum with inf -> 0; an array -> itself as fp64"""
    if weighting is None or (isinstance(weighting, str) and weighting == 'CN'):
        return None
    if isinstance(weighting, str):
        colsum = np.asarray(canonical(A).sum(axis=0)).ravel()
        with np.errstate(divide='ignore', invalid='ignore'):
            mult = 1 / (np.log(colsum) if weighting == 'AA' else colsum)
        mult = np.asarray(mult, dtype=np.float64)
        mult[np.isinf(mult)] = 0
        return mult
    return np.asarray(weighting, dtype=np.float64)


def lists(A, links, weighting=None):
    """(rowptr int64 [L + 1], ids int64 [T], coef float32 [T] or None when weighting is None)"""
    A = canonical(A)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    mult = multiplier(A, weighting)
    indptr, indices, data = A.indptr, A.indices, A.data.astype(np.float64)
    rowptr = np.zeros(len(links) + 1, dtype=np.int64)
    ids, coef = [], []
    for q, (u, v) in enumerate(links):
        cu, cv = indices[indptr[u]:indptr[u + 1]], indices[indptr[v]:indptr[v + 1]]
        w, iu, iv = np.intersect1d(cu, cv, assume_unique=True, return_indices=True)
        rowptr[q + 1] = rowptr[q] + len(w)
        ids.append(w.astype(np.int64))
        a_u, a_v = data[indptr[u] + iu], data[indptr[v] + iv]
        c = a_u * (a_v * mult[w]) if mult is not None else a_u * a_v
        coef.append(c.astype(np.float32))
    ids = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
    coef = np.concatenate(coef) if coef else np.zeros(0, dtype=np.float32)
    return rowptr, ids, (None if weighting is None else coef)


def pool_lists(rowptr, ids, coef, x):
    """the float32 loop acc = acc + c[k] * x[w_k] of every link at once: step k adds the k-th member of every link that has one"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and coef.dtype == np.float32
    L = len(rowptr) - 1
    counts = np.diff(rowptr)
    acc = np.zeros((L, x.shape[1]), dtype=np.float32)
    order = np.argsort(-counts, kind='stable')  # links by falling count: step k touches a prefix of them
    sorted_counts = counts[order]
    for k in range(int(counts.max()) if L else 0):
        sel = order[:np.searchsorted(-sorted_counts, -k, side='left')]  # the links with count > k
        at = rowptr[sel] + k
        prod = coef[at][:, None] * x[ids[at]]
        acc[sel] = acc[sel] + prod
    return acc


def pooled(A, links, x, weighting='CN'):
    """float32 [L, F]"""
    rowptr, ids, coef = lists(A, links, weighting)
    return pool_lists(rowptr, ids, coef, x)


def scipy_pooled_f64(A, links, x, weighting='CN'):
    """(S @ x, |S| @ |x|, members per link) in float64 with S = A[src].multiply(A_[dst]), A_ = A.multiply(mult)"""
    mult = multiplier(A, weighting)  # on the matrix's own dtype, as the restatement and the engine form it
    A = canonical(A).astype(np.float64)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    A_ = A if mult is None else sp.csr_matrix(A.multiply(mult[None, :]))
    S = sp.csr_matrix(A[links[:, 0]].multiply(A_[links[:, 1]]))
    x64 = np.asarray(x, dtype=np.float64)
    return S @ x64, abs(S) @ np.abs(x64), S
