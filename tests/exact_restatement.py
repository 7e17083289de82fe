"""The exact subgraph features restated in scipy, for the exact-feature tests (ElphHashes.exact_subgraph_features).

G' is the graph build_hash_tables propagates over (reference hashing.py:139-165): every edge j -> i of edge_index (flow source ->
target) plus a self loop at every node below n_self = max(edge_index) + 1 (add_self_loops without num_nodes, hashing.py:148).  With
A'[x, j] = 1 for every (j -> x) in G', the k-hop balls B_0(x) = {x}, B_k(x) = U_{(j -> x)} B_{k-1}(j) are the rows of the boolean
powers B_k = A'^k.  For a pair (u, v): I[k1][k2] = |B_k1(u) & B_k2(v)|, balls = |B_k(u)|, |B_k(v)|, and the features are the feature
algebra of hashing.py:276-320 on float(I) and float(balls), in the kernel's fp32 operation order (csrc/ss_feature_algebra.hpp).
Only the rows of the nodes a test asks about are formed: M_k = E_X A'^k for the selector E_X of those nodes.
"""
import numpy as np
import scipy.sparse as sp


def adjacency(num_nodes, edge_index):
    """A' as a 0/1 float32 csr [N, N] (row x = the in-neighbours of x in G'; float32 keeps the products small and every count below
    2^24 exact)"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    n_self = int(ei.max()) + 1 if ei.size else 0
    loops = np.arange(n_self, dtype=np.int64)
    rows = np.concatenate([ei[1], loops])
    cols = np.concatenate([ei[0], loops])
    A = sp.csr_matrix((np.ones(rows.size, dtype=np.float32), (rows, cols)), shape=(num_nodes, num_nodes))
    A.sum_duplicates()
    A.data[:] = 1
    return A


def ball_rows(A, nodes, h):
    """[M_1 .. M_h]: csr [len(nodes), N] 0/1, row i = B_k(nodes[i])"""
    N = A.shape[0]
    nodes = np.asarray(nodes, dtype=np.int64)
    M = sp.csr_matrix((np.ones(nodes.size, dtype=np.float32), (np.arange(nodes.size), nodes)), shape=(nodes.size, N))
    out = []
    for _ in range(h):
        M = (M @ A).tocsr()
        M.data[:] = 1
        M.eliminate_zeros()
        out.append(M)
    return out


def counts(num_nodes, edge_index, links, h):
    """(I int64 [L, h, h], balls int64 [L, 2, h]) of the pairs `links` (int [L, 2], negative ids wrapped)"""
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    links = np.where(links < 0, links + num_nodes, links)
    A = adjacency(num_nodes, edge_index)
    nodes, inv = np.unique(links.reshape(-1), return_inverse=True)
    inv = inv.reshape(-1, 2)
    M = ball_rows(A, nodes, h)
    L = links.shape[0]
    I = np.zeros((L, h, h), dtype=np.int64)
    balls = np.zeros((L, 2, h), dtype=np.int64)
    for k in range(h):
        sizes = np.asarray(M[k].sum(axis=1)).ravel()
        sizes = np.rint(sizes).astype(np.int64)
        balls[:, 0, k] = sizes[inv[:, 0]]
        balls[:, 1, k] = sizes[inv[:, 1]]
    for k1 in range(h):
        Mu = M[k1][inv[:, 0]]
        for k2 in range(h):
            I[:, k1, k2] = np.rint(np.asarray(Mu.multiply(M[k2][inv[:, 1]]).sum(axis=1)).ravel()).astype(np.int64)
    return I, balls


def features(I, balls, use_zero_one, floor_sf):
    """fp32 [L, h(h+2)]: assemble_features<h> of csrc/ss_feature_algebra.hpp, operation for operation, on float32 arrays"""
    f32 = np.float32
    I = np.asarray(I).astype(f32)
    c1 = np.asarray(balls)[:, 0, :].astype(f32)
    c2 = np.asarray(balls)[:, 1, :].astype(f32)
    h = I.shape[1]
    f = [None] * (h * (h + 2))
    f[0] = I[:, 0, 0]
    if h == 1:
        f[1] = c2[:, 0] - f[0]
        f[2] = c1[:, 0] - f[0]
    elif h == 2:
        f[1] = I[:, 1, 0] - f[0]
        f[2] = I[:, 0, 1] - f[0]
        f[3] = I[:, 1, 1] - f[0] - f[1] - f[2]
        f[4] = c2[:, 0] - (f[0] + f[1])
        f[5] = c1[:, 0] - f[0] - f[2]
        f[6] = c2[:, 1] - ((((f[0] + f[4]) + f[1]) + f[2]) + f[3])
        f[7] = c1[:, 1] - f[0] - (((f[0] + f[1]) + f[2]) + f[3]) - f[5]
    else:
        f[1] = I[:, 1, 0] - f[0]
        f[2] = I[:, 0, 1] - f[0]
        f[3] = I[:, 1, 1] - f[0] - f[1] - f[2]
        f[4] = I[:, 2, 0] - f[0] - f[1]
        f[5] = I[:, 0, 2] - f[0] - f[2]
        s04 = ((f[0] + f[1]) + f[2]) + f[3]
        f[6] = I[:, 2, 1] - s04 - f[4]
        f[7] = I[:, 1, 2] - s04 - f[5]
        f[8] = I[:, 2, 2] - (((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7])
        f[9] = c2[:, 0] - f[0] - f[1] - f[4]
        f[10] = c1[:, 0] - f[0] - f[2] - f[5]
        s05 = (((f[0] + f[4]) + f[1]) + f[2]) + f[3]
        f[11] = c2[:, 1] - s05 - f[6] - f[9]
        f[12] = c1[:, 1] - s05 - f[7] - f[10]
        s09 = (((((((f[8] + f[0]) + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]
        f[13] = c2[:, 2] - s09 - f[9] - f[11]
        f[14] = c1[:, 2] - s09 - f[10] - f[12]
    out = np.stack(f, axis=1).astype(f32)
    if not use_zero_one:
        zero = {1: [], 2: [4, 5], 3: [4, 5, 11, 12]}[h]
        out[:, zero] = 0
    if floor_sf:
        out = np.where(out < 0, f32(0), out)
    return out


def restate(num_nodes, edge_index, links, h, use_zero_one=True, floor_sf=False):
    """(features fp32 [L, h(h+2)], I, balls)"""
    I, balls = counts(num_nodes, edge_index, links, h)
    return features(I, balls, use_zero_one, floor_sf), I, balls
