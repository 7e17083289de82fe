"""The per-hop sampled enclosing subgraphs restated in Python sets, for the sampled-subgraph tests (ElphHashes.sampled_subgraph_nodes and
exact_subgraphs(max_nodes_per_hop=..., ratio_per_hop=...)).

The walk is the reference's k_hop_subgraph (src/datasets/seal.py:291-348) with its two random.sample calls replaced by one bottom-m
selection by a key -- uniform samples of uniform samples are uniform, and so is a bottom-m selection by an independent key:

    visited = kept = {u, v};  for hop = 1 .. h:
        fringe = in-neighbours(kept) - visited;  visited |= fringe      (the WHOLE fringe: a rejected node never comes back)
        F = len(fringe);  m = F if ratio == 1.0 else int(ratio * F);  cap given: m = min(m, cap)
        kept = the m fringe nodes with the smallest (key, id);  stop when m == 0
    key(x) = H(H(K + GOLDEN * hop) ^ (x + 1)),  K = H(seed ^ H(((u << 32) | v) + 1)),  H = the splitmix64 finaliser, 64-bit wrapping

The target link stays in the walk.  The row lists the kept nodes ascending by id, each with the hop it joined at.  The induced
adjacency, the roots and the labels on those rows: subgraph_restatement's bfs / link_labels / drnl (they take adjacency rows); its
restate() makes its own node rows, so the adjacency is restated here with scipy, A[ids][:, ids].
"""
import numpy as np
import scipy.sparse as sp

import subgraph_restatement as sr

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def hash_u64(x):
    """the splitmix64 finaliser on numpy uint64 (scalars or arrays), wrapping"""
    with np.errstate(over='ignore'):
        x = np.asarray(x, dtype=np.uint64)
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def link_key(seed, u, v):
    with np.errstate(over='ignore'):
        return hash_u64(np.uint64(seed) ^ hash_u64(((np.uint64(u) << np.uint64(32)) | np.uint64(v)) + np.uint64(1)))


def keys(seed, u, v, hop, nodes):
    """uint64 keys of the int64 array `nodes` at `hop` of link (u, v)"""
    with np.errstate(over='ignore'):
        hop_key = hash_u64(link_key(seed, u, v) + GOLDEN * np.uint64(hop))
        return hash_u64(hop_key ^ (np.asarray(nodes, dtype=np.int64).astype(np.uint64) + np.uint64(1)))


def in_neighbours(num_nodes, edge_index):
    """[set of the sources of the arcs into x] per node"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    nb = [set() for _ in range(int(num_nodes))]
    for j, x in zip(ei[0].tolist(), ei[1].tolist()):
        nb[x].add(j)
    return nb


def walk(nb, u, v, h, cap=None, ratio=1.0, seed=0, fringes=None):
    """{node: hop} of one link (u, v wrapped already).  fringes (optional list) receives (F, m) of every hop walked"""
    hop_of = {u: 0, v: 0}
    visited, kept = {u, v}, {u, v}
    for hop in range(1, h + 1):
        fringe = set()
        for y in kept:
            fringe |= nb[y]
        fringe -= visited
        visited |= fringe
        F = len(fringe)
        m = F if ratio == 1.0 else int(ratio * F)
        if cap is not None:
            m = min(m, cap)
        if fringes is not None:
            fringes.append((F, m))
        if m == 0:
            break
        nodes = np.array(sorted(fringe), dtype=np.int64)
        order = np.lexsort((nodes, keys(seed, u, v, hop, nodes)))  # by key, then by id
        kept = set(nodes[order[:m]].tolist())
        for x in kept:
            hop_of[x] = hop
    return hop_of


def restate_nodes(num_nodes, edge_index, links, h, cap=None, ratio=1.0, seed=0, max_nodes=None, return_info=False, nb=None):
    """(rowptr int64 [L + 1], ids int64 [T], hop uint8 [T]) of `links` (int [L, 2], negative ids wrapped); with return_info also
    {'truncated': indices of the rows emptied by max_nodes, 'sampled_links': links where some hop dropped a node}.  nb: the caller's own
    node -> set of in-neighbours in place of in_neighbours(num_nodes, edge_index) (a sparse mapping where a list of N sets is too much)"""
    n = int(num_nodes)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    links = np.where(links < 0, links + n, links)
    nb = in_neighbours(n, edge_index) if nb is None else nb
    rowptr, ids, hops, gone, sampled = [0], [], [], [], 0
    for q, (u, v) in enumerate(links.tolist()):
        fr = []
        hop_of = walk(nb, u, v, h, cap, ratio, seed, fr)
        sampled += any(m < F for F, m in fr)
        row = sorted(hop_of)
        if max_nodes is not None and len(row) > max_nodes:
            gone.append(q)
            row = []
        ids.append(np.array(row, dtype=np.int64))
        hops.append(np.array([hop_of[x] for x in row], dtype=np.uint8))
        rowptr.append(rowptr[-1] + len(row))
    out = (np.asarray(rowptr, dtype=np.int64), np.concatenate(ids + [np.zeros((0,), dtype=np.int64)]),
           np.concatenate(hops + [np.zeros((0,), dtype=np.uint8)]))
    return out + ({'truncated': np.array(gone, dtype=np.int64), 'sampled_links': sampled},) if return_info else out


def rows(rowptr, ids, hop):
    """[(ids, hop)] per link"""
    return [(ids[a:b], hop[a:b]) for a, b in zip(rowptr[:-1], rowptr[1:])]


def restate(num_nodes, edge_index, links, h, mask_target=True, cap=None, ratio=1.0, seed=0, max_nodes=None):
    """a subgraph_restatement.Restated with `hop` in place of `dist`: the node rows above and on them roots, adj_ptr, nbr, weight -- the
    in-arc multiplicity matrix M[x, j] = copies of j -> x restricted to the row, M[ids][:, ids], without its diagonal and, mask_target
    and u != v, without (u, v) and (v, u)"""
    n = int(num_nodes)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    links = np.where(links < 0, links + n, links)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    rowptr, ids, hop = restate_nodes(n, ei, links, h, cap, ratio, seed, max_nodes)
    M = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.int64), (ei[1], ei[0])), shape=(n, n))
    M.sum_duplicates()
    roots = np.full((len(links), 2), -1, dtype=np.int32)
    counts, nbr, weight = [], [], []
    for q, (u, v) in enumerate(links.tolist()):
        row = ids[rowptr[q]:rowptr[q + 1]]
        if row.size == 0:
            continue
        ru, rv = int(np.searchsorted(row, u)), int(np.searchsorted(row, v))
        assert row[ru] == u and row[rv] == v
        roots[q] = [ru, rv]
        sub = M[row][:, row].tolil()
        sub.setdiag(0)
        if mask_target and u != v:
            sub[ru, rv] = 0
            sub[rv, ru] = 0
        sub = sub.tocsr()
        sub.eliminate_zeros()
        sub.sort_indices()
        counts.extend(np.diff(sub.indptr).tolist())
        nbr.append(sub.indices.astype(np.int64))
        weight.append(sub.data.astype(np.int64))
    adj_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda parts: np.concatenate(parts + [np.zeros((0,), dtype=np.int64)]).astype(np.int32)
    return sr.Restated(rowptr=rowptr, ids=ids, hop=hop, roots=roots, adj_ptr=adj_ptr, nbr=cat(nbr), weight=cat(weight), links=links)


def labels(sub, node_label, max_dist=1000):
    """z of a restate() result for one label mode (None for None): 'hop' / 'zo' from hop, the rest by subgraph_restatement.link_labels"""
    if node_label is None:
        return None
    if node_label in ('hop', 'zo'):
        hop = sub.hop.astype(np.int64)
        return hop if node_label == 'hop' else (hop == 0).astype(np.int64)
    out = [np.zeros((0, 2) if node_label != 'drnl' else (0,), dtype=np.int64)]
    for q in range(len(sub.rowptr) - 1):
        if sub.rowptr[q + 1] > sub.rowptr[q]:
            _, ptr, nbr, _ = sub.row(q)
            out.append(sr.link_labels(ptr, nbr, int(sub.roots[q, 0]), int(sub.roots[q, 1]), node_label, max_dist))
    return np.concatenate(out).astype(np.int64)
