"""fp64 restatement of fast_pagerank.pagerank_power (the third-party call behind the reference's PPR, heuristics.py:99; the
package is not a dependency here), for the PPR tests.  Several personalisation vectors run side by side as the columns of one
dense matrix; every column keeps its own stop rule, exactly as separate calls would:

    r = A.sum(axis=1); D^-1 = diag(1 / r_k) on rows with r_k != 0; s = n e_src; z = ((1-p)[r != 0] + [r == 0]) / n
    W = p * A.T @ D^-1; x = s; oldx = 0
    while ||x - oldx|| > tol: oldx = x; x = W x + s (z^T x); it += 1; if it >= max_iter: break
    return x / sum(x)
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def operator(A, p):
    A = sp.csr_matrix(A)
    n = A.shape[0]
    r = np.asarray(A.sum(axis=1)).reshape(-1)
    k = r.nonzero()[0]
    D_1 = sp.csr_matrix((1 / r[k], (k, k)), shape=(n, n))
    z = ((1 - p) * (r != 0) + (r == 0)) / n
    W = p * A.T @ D_1
    return W.tocsr(), z


def pagerank_power(A, sources, p=0.85, tol=1e-7, max_iter=100):
    """returns (vectors [K, n] normalised, iterations [K], residuals): residuals[j][k] = ||x_k - x_(k-1)|| of column j, the
    value the stop rule compared with tol after step k (k = 0: the initial ||s - 0|| = n)"""
    W, z = operator(A, p)
    n = W.shape[0]
    K = len(sources)
    s = np.zeros((n, K))
    s[np.asarray(sources), np.arange(K)] = n
    x = s.copy()
    oldx = np.zeros((n, K))
    active = np.ones(K, dtype=bool)
    iters = np.zeros(K, dtype=np.int64)
    residuals = [[] for _ in range(K)]
    while True:
        res = np.sqrt(((x - oldx) ** 2).sum(axis=0))
        for j in np.nonzero(active)[0]:
            residuals[j].append(res[j])
        active &= res > tol
        if not active.any():
            break
        cols = np.nonzero(active)[0]
        oldx[:, cols] = x[:, cols]
        xa = x[:, cols]
        x[:, cols] = W @ xa + s[:, cols] * (z @ xa)[None, :]
        iters[cols] += 1
        active &= ~(iters >= max_iter)  # the reference breaks after the step that reaches max_iter
        for j in cols[~active[cols]]:
            residuals[j].append(np.sqrt(((x[:, j] - oldx[:, j]) ** 2).sum()))
    return (x / x.sum(axis=0)).T, iters, residuals


def ppr_solve(A, src, p=0.85):
    """the converged vector without the loop: x is proportional to (I - W)^-1 e_src"""
    W, _ = operator(A, p)
    n = W.shape[0]
    e = np.zeros(n)
    e[src] = 1.0
    y = spla.spsolve((sp.identity(n, format='csc') - W).tocsc(), e)
    return y / y.sum()
