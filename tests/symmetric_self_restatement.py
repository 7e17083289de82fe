"""numpy restatement of what the self-row skip of the table hops rests on (no GPU, no library):

  * sketch hops over a CSR-by-destination, with the implicit self row of every i < n_self or -- `skip` -- without it for the rows
    that have an in-edge (csrc/ss_common.hpp table_hop_total);
  * the two symmetry sums of the CSR build's level-0 pass (csrc/ss_csr.hip tile_sort_kernel: sym_mix0 / sym_mix1).

The lemma (include/subgraph_sketch.h, SS_GRAPH_HOP_TABLES): on a graph whose edge multiset is symmetric, with a self loop at
every node that occurs in an edge, a hop k >= 2 gives the same rows with and without the own row of every row that has an in-edge.
"""
import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def splitmix_finaliser(x):
    """hash_u64 of csrc/ss_common.hpp"""
    x = _u64(x).copy()
    with np.errstate(over='ignore'):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def sym_mix0(x):
    with np.errstate(over='ignore'):
        return splitmix_finaliser(_u64(x) + np.uint64(0x9E3779B97F4A7C15))


def sym_mix1(x):
    x = _u64(x) ^ np.uint64(0xD6E8FEB86659FD93)
    with np.errstate(over='ignore'):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def symmetry_sums(edge_index):
    """(S_0, S_1) as Python ints mod 2^64: an edge s -> d with s < d adds mix(s << 32 | d), with s > d takes mix(d << 32 | s) away,
    a self edge adds nothing"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    s, d = ei[0], ei[1]
    lo, hi = np.minimum(s, d).astype(np.uint64), np.maximum(s, d).astype(np.uint64)
    x = (lo << np.uint64(32)) | hi
    sums = []
    for mix in (sym_mix0, sym_mix1):
        f = mix(x)
        up = int(f[s < d].astype(object).sum()) if (s < d).any() else 0
        down = int(f[s > d].astype(object).sum()) if (s > d).any() else 0
        sums.append((up - down) % (1 << 64))
    return tuple(sums)


def is_symmetric_multiset(edge_index):
    """exact: as many copies of j -> i as of i -> j, for every pair"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    fwd = np.sort(ei[0] * (1 << 32) + ei[1])
    bwd = np.sort(ei[1] * (1 << 32) + ei[0])
    return bool(np.array_equal(fwd, bwd))


def csr_by_destination(edge_index, num_nodes):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    order = np.argsort(ei[1], kind='stable')
    rowptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.add.at(rowptr, ei[1] + 1, 1)
    return np.cumsum(rowptr), ei[0][order]


def hop0_minhash(n, num_perm=16):
    """rows that are functions of the node id alone (values in [0, 2^32), like the hop-0 MinHash table)"""
    ids = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(num_perm) + np.arange(num_perm, dtype=np.uint64)[None, :]
    return (splitmix_finaliser(ids + np.uint64(1)) >> np.uint64(32)).astype(np.uint32)


def hop0_hll(n, p=6):
    """one non-zero register per row (like the hop-0 HLL table)"""
    hv = splitmix_finaliser(np.arange(n, dtype=np.uint64) + np.uint64(1))
    m = 1 << p
    out = np.zeros((n, m), dtype=np.uint8)
    bits = hv >> np.uint64(p)
    bl = np.array([int(b).bit_length() for b in bits])
    out[np.arange(n), (hv & np.uint64(m - 1)).astype(np.int64)] = (64 - p) - bl + 1
    return out


def hop(x, rowptr, col, n_self, agg, skip=False):
    """one table hop: out[i] = agg over the in-neighbours of i and -- i < n_self, unless `skip` and i has an in-edge -- x[i];
    rows that fold nothing are zero.  agg: np.minimum (MinHash) or np.maximum (HLL)"""
    out = np.zeros_like(x)
    for i in range(len(rowptr) - 1):
        nb = col[rowptr[i]:rowptr[i + 1]]
        rows = [x[j] for j in nb]
        if i < n_self and not (skip and len(nb) > 0):
            rows.append(x[i])
        if rows:
            out[i] = agg.reduce(np.stack(rows), axis=0)
    return out


def build(edge_index, num_nodes, hops, skip, num_perm=16, p=6):
    """tables of hops 1 .. hops, [(minhash, hll)]; the inferred self loops (i < max(edge_index) + 1); hop 1 always keeps the self row,
    `skip` applies to the hops k >= 2 (their inputs are hop-(k-1) tables of the same graph)"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    n_self = int(ei.max()) + 1 if ei.size else 0
    rowptr, col = csr_by_destination(ei, num_nodes)
    mh, hl = hop0_minhash(num_nodes, num_perm), hop0_hll(num_nodes, p)
    out = []
    for k in range(1, hops + 1):
        mh = hop(mh, rowptr, col, n_self, np.minimum, skip and k >= 2)
        hl = hop(hl, rowptr, col, n_self, np.maximum, skip and k >= 2)
        out.append((mh, hl))
    return out


def symmetric_graph(rng, n_active, e_und, n_isolated_low=0, self_edges=0, duplicates=0, leaves=0):
    """[2, E] int64: e_und random undirected edges over ids [n_isolated_low .. ) stored in both directions, `duplicates` of them stored
    twice in both directions, `self_edges` explicit self edges, `leaves` extra nodes with one neighbour each; the first `n_isolated_low`
    ids occur in no edge (isolated ids BELOW n_self).  Returns (edge_index, num_nodes)"""
    lo = n_isolated_low
    e = rng.randint(lo, lo + n_active, size=(2, e_und)).astype(np.int64)
    parts = [e, e[::-1]]
    if duplicates:
        d = e[:, rng.choice(e_und, size=duplicates, replace=False)]
        parts += [d, d[::-1]]
    if self_edges:
        s = rng.randint(lo, lo + n_active, size=self_edges).astype(np.int64)
        parts.append(np.stack([s, s]))
    n = lo + n_active
    if leaves:
        leaf = np.arange(n, n + leaves, dtype=np.int64)
        hub = rng.randint(lo, lo + n_active, size=leaves).astype(np.int64)
        parts += [np.stack([leaf, hub]), np.stack([hub, leaf])]
        n += leaves
    ei = np.concatenate(parts, axis=1)
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])]), n


# the two asymmetric graphs on which leaving out the self row WOULD change a row (asserted on the CPU by test_symmetric_self_host, run
# on the GPU by test_symmetric_self_gpu: the word must be 0 and the tables the oracle's)
ONE_DIRECTED_EDGE = (np.array([[0], [1]], dtype=np.int64), 2)                   # 0 -> 1 alone: row 1 at hop 2 needs its own row
PATH_MINUS_ONE_REVERSE = (np.array([[0, 1, 1], [1, 0, 2]], dtype=np.int64), 3)  # path 0 - 1 - 2 without 2 -> 1: row 2 needs its own
