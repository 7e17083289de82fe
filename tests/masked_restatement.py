"""The rule of target-link masking (ElphHashes.get_subgraph_features(mask_target=...)) restated in numpy (no code shared with
the engine), and the leave-one-out reference it is checked against: the oracle run over the edge list minus the link.

G is what build_hash_tables(num_nodes, edge_index) propagates over: the edges, flow source -> target, plus a self loop at every node
below n_self = max(edge_index) + 1.  G_uv is G without every copy of u -> v and of v -> u (n_self and the self loops stay).  With N'(x)
the in-neighbours of x without the partner when x is u or v, T_k the stored hop-k tables and fold = min (MinHash) / max (HLL):
  R1(x) = fold of hop 0 over N'(x), and x itself if x < n_self                       x in {u, v}
  H1(y) = R1(y) for y in {u, v}, else T_1(y)
  R2(x) = fold of H1(w) over w in N'(x), and R1(x) if x < n_self
  R3(x) = R2(x) if x < n_self, folded with H1(w) (w < n_self) and H1(y), y in N'(w), for every w in N'(x)
A fold over nothing is the all-zero row (the scatter default of the propagation)."""
import numpy as np

from oracle import oracle


def n_self_of(edge_index):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    return int(ei.max()) + 1 if ei.size else 0


def in_neighbours(num_nodes, edge_index):
    """list of int arrays: row x = the sources of the edges into x, duplicates kept"""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    order = np.argsort(ei[1], kind='stable')
    counts = np.bincount(ei[1], minlength=num_nodes)
    return np.split(ei[0][order], np.cumsum(counts)[:-1])


def is_edge(nbrs, u, v):
    return u != v and (bool((nbrs[u] == v).any()) or bool((nbrs[v] == u).any()))


def _fold(rows, kind, width, dtype):
    if not rows:
        return np.zeros(width, dtype=dtype)
    stack = np.stack(rows)
    return stack.min(axis=0) if kind == 'minhash' else stack.max(axis=0)


def masked_rows(u, v, nbrs, n_self, tables, h):
    """-> {kind: uint array [2, h, W]}: hop 1 .. h rows of u (index 0) and v (index 1) in G_uv, by the rule above"""
    out = {}
    for kind in ('minhash', 'hll'):
        T0, T1 = tables[0][kind], tables[1][kind]
        width, dtype = T0.shape[1], T0.dtype

        def nprime(x):
            nb = nbrs[x]
            if x == u:
                nb = nb[nb != v]
            elif x == v:
                nb = nb[nb != u]
            return nb

        R1 = {}
        for x in (u, v):
            R1[x] = _fold([T0[j] for j in nprime(x)] + ([T0[x]] if x < n_self else []), kind, width, dtype)

        def H1(y):
            return R1[y] if y in R1 else T1[y]

        rows = np.zeros((2, h, width), dtype=dtype)
        for side, x in enumerate((u, v)):
            rows[side, 0] = R1[x]
            if h >= 2:
                R2 = _fold([H1(w) for w in nprime(x)] + ([R1[x]] if x < n_self else []), kind, width, dtype)
                rows[side, 1] = R2
            if h >= 3:
                parts = [R2] if x < n_self else []
                for w in nprime(x):
                    if w < n_self:
                        parts.append(H1(w))
                    parts.extend(H1(y) for y in nprime(w))
                rows[side, 2] = _fold(parts, kind, width, dtype)
        out[kind] = rows
    return out


def masked_query(links, num_nodes, edge_index, tables, cards, h, params, use_zero_one=True, floor_sf=False):
    """the masked call restated: -> (features [L, h(h+2)], {'match', 'zeros', 'row_zeros', 'masked', 'rows'}).  tables / cards: the
    oracle's for the FULL graph (hops 0 .. h).  The pair arithmetic is the oracle's own, run on a two-row table per link"""
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    L = links.shape[0]
    nbrs = in_neighbours(num_nodes, edge_index)
    n_self = n_self_of(edge_index)
    P, M = tables[1]['minhash'].shape[1], tables[1]['hll'].shape[1]
    mh = np.zeros((2 * L, h, P), dtype=np.uint32)
    hl = np.zeros((2 * L, h, M), dtype=np.uint8)
    cd = np.zeros((2 * L, h), dtype=np.float32)
    masked = np.zeros(L, dtype=bool)
    for q, (u, v) in enumerate(links.tolist()):
        u, v = (u + num_nodes if u < 0 else u), (v + num_nodes if v < 0 else v)
        if is_edge(nbrs, u, v):
            masked[q] = True
            rows = masked_rows(u, v, nbrs, n_self, tables, h)
            mh[2 * q:2 * q + 2] = rows['minhash']
            hl[2 * q:2 * q + 2] = rows['hll']
            for side in range(2):
                cd[2 * q + side] = oracle.hll_count(rows['hll'][side], params)
        else:
            for side, x in enumerate((u, v)):
                for k in range(h):
                    mh[2 * q + side, k] = tables[k + 1]['minhash'][x]
                    hl[2 * q + side, k] = tables[k + 1]['hll'][x]
                cd[2 * q + side] = cards[x, :h]
    two = {k + 1: {'minhash': np.ascontiguousarray(mh[:, k]), 'hll': np.ascontiguousarray(hl[:, k])} for k in range(h)}
    pairs = np.arange(2 * L, dtype=np.int64).reshape(L, 2)
    feats, dbg = oracle.pair_features(pairs, two, cd, h, params, use_zero_one=use_zero_one, floor_sf=floor_sf, debug=True)
    row_zeros = (hl == 0).sum(axis=2).astype(np.int32).reshape(L, 2, h)
    return feats, {'match': dbg['match'], 'zeros': dbg['zeros'], 'row_zeros': row_zeros, 'masked': masked,
                   'rows': {'minhash': mh.reshape(L, 2, h, P), 'hll': hl.reshape(L, 2, h, M)}, 'cards': cd.reshape(L, 2, h),
                   'branch': dbg['branch']}


def without_link(edge_index, u, v):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    hit = ((ei[0] == u) & (ei[1] == v)) | ((ei[0] == v) & (ei[1] == u))
    return ei[:, ~hit] if u != v else ei


def leave_one_out(u, v, num_nodes, edge_index, h, num_perm, params, use_zero_one=True, floor_sf=False):
    """the reference of the contract: the oracle's propagation over add_self_loops(edge_index minus the link, num_nodes = n_self of the
    FULL list), then its pair arithmetic.  -> (features [h(h+2)], debug of the one pair, {kind: rows [2, h, W]}, cards [2, h])"""
    ei = oracle.add_self_loops(without_link(edge_index, u, v), num_nodes=n_self_of(edge_index))
    tables = {0: {'minhash': oracle.minhash_init(num_nodes, num_perm), 'hll': oracle.hll_init(num_nodes, params.p)}}
    cards = np.zeros((num_nodes, h), dtype=np.float32)
    for k in range(1, h + 1):
        m, l = oracle.propagate(num_nodes, ei, tables[k - 1]['minhash'], tables[k - 1]['hll'])
        tables[k] = {'minhash': m, 'hll': l}
        cards[:, k - 1] = oracle.hll_count(l, params)
    feats, dbg = oracle.pair_features(np.array([[u, v]]), tables, cards, h, params, use_zero_one=use_zero_one, floor_sf=floor_sf, debug=True)
    rows = {kind: np.stack([np.stack([tables[k][kind][x] for k in range(1, h + 1)]) for x in (u, v)]) for kind in ('minhash', 'hll')}
    return feats[0], {k: a[0] for k, a in dbg.items()}, rows, cards[[u, v]]


def assert_features_bar(got, want, cards, what=''):
    """rtol 1e-5, atol 1e-5 * 4 * max|cards|"""
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * 4 * float(np.abs(cards).max() if np.size(cards) else 0.0), err_msg=what)


def exact_on_g_uv(links, num_nodes, edge_index, h, exact_fn):
    """exact counts link by link on G_uv with n_self pinned: exact_fn(link [1, 2], edge_index', n_self) -> (feats, I, balls)"""
    n_self = n_self_of(edge_index)
    outs = [exact_fn(np.array([[u, v]], dtype=np.int64), without_link(edge_index, u, v), n_self) for u, v in np.asarray(links).tolist()]
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3))
