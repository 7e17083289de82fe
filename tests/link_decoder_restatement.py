"""What link_decoder.link_gather / link_hadamard compute, restated in numpy, and the planted batch of links their tests share.

Forward:  gather[l, s] = x[links[l, s]];  hadamard[l] = x[links[l, 0]] * x[links[l, 1]] (one float32 multiply).
Backward: the 2L endpoint slots q = 2l + s are grouped by node, ascending inside every group (a stable grouping, written out below as a
counting loop).  Row n of grad_x takes its slots q_0 < q_1 < ... in chunks of C = 256:
    p_c = the sequential fp32 sum from +0 of the terms of chunk c          s = ((0 + p_0) + p_1) + ...          no slots: +0
    term t_q = g[l, s] (gather),  fl(g[l] * x[links[l, 1 - s]]) (product),  l = q >> 1, s = q & 1;  a self link (u, u) is two slots of u
`mutation` names one deliberate mistake each (the host test shows that every one of them changes bits on the planted batch).
"""
import numpy as np

C = 256
MUTATIONS = ('wrong partner', 's swapped', 'descending', 'one running sum')


def gather(x, links):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)[np.asarray(links, dtype=np.int64)])


def hadamard(x, links):
    x, links = np.asarray(x, dtype=np.float32), np.asarray(links, dtype=np.int64)
    return x[links[:, 0]] * x[links[:, 1]]  # (float32 multiply)


def grouping(links, n):
    """(nodes int64 [M], rowptr int64 [M + 1], order int64 [2L]): the slots of every touched node, nodes ascending, slots ascending
    inside a node -- a counting sort written as loops"""
    flat = np.asarray(links, dtype=np.int64).reshape(-1)
    counts = [0] * n
    for v in flat:
        counts[v] += 1
    nodes = [v for v in range(n) if counts[v]]
    rowptr, start = [0], {}
    for v in nodes:
        start[v] = rowptr[-1]
        rowptr.append(rowptr[-1] + counts[v])
    order = [0] * len(flat)
    for q, v in enumerate(flat):  # ascending q: every group fills in ascending slot order
        order[start[v]] = q
        start[v] += 1
    return np.array(nodes, dtype=np.int64), np.array(rowptr, dtype=np.int64), np.array(order, dtype=np.int64)


def chunked_sum(terms, one_running_sum=False):
    """the contract's sum of float32 terms [m, F] given in order: chunks of C summed sequentially from +0, then added in chunk order"""
    s = np.zeros(terms.shape[1], dtype=np.float32)
    if one_running_sum:
        for t in terms:
            s = s + t
        return s
    for a in range(0, len(terms), C):
        p = np.zeros(terms.shape[1], dtype=np.float32)
        for t in terms[a:a + C]:
            p = p + t  # (float32 add)
        s = s + p
    return s


def slot_terms(links, qs, g_rows, x_rows=None, mutation=None):
    """float32 [len(qs), F]: the terms of the slots qs.  g_rows: (row indices of g as a [rows, F] matrix) -> float32 rows -- for the
    gather g is [L, 2, F] seen as [2L, F]; x_rows None: the gather; else node ids -> float32 rows of x: the product"""
    links = np.asarray(links, dtype=np.int64)
    qs = np.asarray(qs, dtype=np.int64)
    l, s = qs >> 1, qs & 1
    if x_rows is None:
        return g_rows(2 * l + (1 - s if mutation == 's swapped' else s))
    partner = links[l, s if mutation == 'wrong partner' else 1 - s]
    return g_rows(l) * x_rows(partner)  # (float32 multiply, rounded before any add)


def row_grad(links, qs, g_rows, x_rows=None, mutation=None):
    qs = np.asarray(qs, dtype=np.int64)
    if mutation == 'descending':
        qs = qs[::-1]
    return chunked_sum(slot_terms(links, qs, g_rows, x_rows, mutation), one_running_sum=mutation == 'one running sum')


def grad(links, n, g, x=None, mutation=None):
    """grad_x float32 [n, F] of <gather(x, links), g> (x None, g [L, 2, F]) or of <hadamard(x, links), g> (g [L, F]), in the
    arithmetic of the backward"""
    g = np.ascontiguousarray(g, dtype=np.float32)
    F = g.shape[-1]
    g2 = g.reshape(-1, F)
    out = np.zeros((n, F), dtype=np.float32)
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.float32)
    nodes, rowptr, order = grouping(links, n)
    for r, node in enumerate(nodes):
        out[node] = row_grad(links, order[rowptr[r]:rowptr[r + 1]], lambda i: g2[i], None if x is None else (lambda i: x[i]), mutation)
    return out


def grad_rows(links, rows, g_rows, F, x_rows=None):
    """rows `rows` of grad(...) with g and x given as functions of row indices (the large case: neither is held on the host)"""
    flat = np.asarray(links, dtype=np.int64).reshape(-1)
    out = []
    for node in rows:
        qs = np.nonzero(flat == node)[0]  # ascending
        out.append(row_grad(links, qs, g_rows, x_rows) if len(qs) else np.zeros(F, dtype=np.float32))
    return np.stack(out)


def grad64(links, n, g, x=None):
    """(the float64 gradient, the sum of the terms' magnitudes) -- what the rounding bound is measured against"""
    links = np.asarray(links, dtype=np.int64)
    g = np.asarray(g, dtype=np.float64)
    F = g.shape[-1]
    out, mag = np.zeros((n, F)), np.zeros((n, F))
    for s in (0, 1):
        t = g[:, s] if x is None else g * np.asarray(x, dtype=np.float64)[links[:, 1 - s]]
        np.add.at(out, links[:, s], t)
        np.add.at(mag, links[:, s], np.abs(t))
    return out, mag


# ---- the planted batch ------------------------------------------------------------------------------------------------------------
# N nodes; node NODES[k] has exactly COUNTS[k] slots: rows on both sides of the lane-stretch steps (16, 64), of the chunk (256) and of
# two chunks (512), and one of five chunks with a last chunk of one slot.  The other endpoints come from the pool (every node that is
# not planted), so a pool node's count is whatever the generator gives it -- slot_counts() says what.
N = 701  # not a multiple of any rows-per-wave (1, 2, 4, ... 64)
COUNTS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
NODES = (5, 0, 40, 41, 80, 120, 160, 200, 240, 280, 320, 360, 400, 440, 480, 520, N - 1)  # the first and the last id; 40 and 41 side by side
ZERO, SELF_ONLY, TRIPLE, STRADDLE = NODES[0], NODES[2], NODES[3], NODES[12]
# SELF_ONLY: its two slots are one self link.  TRIPLE: its three slots are one link, three times.  STRADDLE (257 slots): 255 slots,
# then the two slots of a self link -- positions 255 and 256 of its group, either side of the chunk boundary.


def planted(seed=13):
    """links int64 [L, 2] in a seeded random order (the self link of STRADDLE moved behind the node's other links).  A planted node is
    endpoint 0 of its even links and endpoint 1 of its odd ones."""
    pool = np.setdiff1d(np.arange(N), NODES)
    links = []
    for node, m in zip(NODES, COUNTS):
        if node == SELF_ONLY:
            links.append((node, node))
        elif node == TRIPLE:
            links += [(node, pool[7])] * 3
        else:
            k = m - 2 if node == STRADDLE else m
            partners = pool[(7 * node + 3 * np.arange(k)) % len(pool)]  # (1025 > the pool: partners repeat)
            links += [(node, p) if i % 2 == 0 else (p, node) for i, p in enumerate(partners)]
            if node == STRADDLE:
                links.append((node, node))
    links = np.array(links, dtype=np.int64)
    links = links[np.random.RandomState(seed).permutation(len(links))]
    mine = np.nonzero((links == STRADDLE).any(axis=1))[0]
    loop = mine[(links[mine, 0] == STRADDLE) & (links[mine, 1] == STRADDLE)][0]
    links[[loop, mine[-1]]] = links[[mine[-1], loop]]
    return np.ascontiguousarray(links)


def slot_counts(links, n=N):
    return np.bincount(np.asarray(links).reshape(-1), minlength=n)


def features(n, F, seed=3):
    return np.random.RandomState(seed).standard_normal((n, F)).astype(np.float32)
