"""The planted inputs of tests/subgraph_planted.py without a GPU: every property a case claims is asserted here from the arrays the
kernels will read (positions of the runs against multiples of 16, finds per step, deg against switch * n, frontier sizes per level of the
restated BFS, the kind sequence of `many`, T of `sweep`), subgraph_restatement.adjacency_of_rows is pinned to scipy's M[ids][:, ids]
without the diagonal and the masked pair on every adjacency case, and subgraph_restatement.bfs to scipy.sparse.csgraph on every label case."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import subgraph_planted as planted
import subgraph_restatement as sr

G = planted.GROUP


@pytest.fixture(scope='module')
def adj_cases():
    made = {}
    return lambda name: made.setdefault(name, (planted.ADJ_CASES[name] if name != 'switch_probe' else planted.adj_switch_probe)())


@pytest.fixture(scope='module')
def label_cases():
    made = {}
    return lambda name: made.setdefault(name, planted.LABEL_CASES[name]())


def scipy_adjacency(case, mask):
    """(roots, adj_ptr, nbr, weight) of a case's rows by matrix slicing: M[x, j] = copies of the arc j -> x, per link M[ids][:, ids]
    without the diagonal and, masked and u != v, without (u, v) and (v, u) -- as sampled_subgraph_restatement.restate does"""
    M = sp.csr_matrix((np.ones(case.ei.shape[1], dtype=np.int64), (case.ei[1], case.ei[0])), shape=(case.N, case.N))
    M.sum_duplicates()
    roots = np.full((len(case.links), 2), -1, dtype=np.int32)
    counts, nbr, weight = [np.zeros((0,), dtype=np.int64)], [np.zeros((0,), dtype=np.int64)], [np.zeros((0,), dtype=np.int64)]
    for q, (u, v) in enumerate(case.links.tolist()):
        row = case.ids[case.rowptr[q]:case.rowptr[q + 1]]
        if row.size == 0:
            continue
        ru, rv = int(np.searchsorted(row, u)), int(np.searchsorted(row, v))
        assert row[ru] == u and row[rv] == v
        roots[q] = [ru, rv]
        sub = M[row][:, row].tocoo()
        keep = (sub.row != sub.col) & (sub.data != 0)
        if mask and u != v:
            keep &= ~(((sub.row == ru) & (sub.col == rv)) | ((sub.row == rv) & (sub.col == ru)))
        order = np.lexsort((sub.col[keep], sub.row[keep]))
        counts.append(np.bincount(sub.row[keep], minlength=row.size))
        nbr.append(sub.col[keep][order])
        weight.append(sub.data[keep][order])
    adj_ptr = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    return roots, adj_ptr, np.concatenate(nbr).astype(np.int32), np.concatenate(weight).astype(np.int32)


# ---- the contracts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(planted.ADJ_CASES) + ['switch_probe'])
def test_adjacency_cases_keep_the_kernel_contract(adj_cases, name):
    c = adj_cases(name)
    assert c.rowptr[0] == 0 and c.rowptr[-1] == c.T and (np.diff(c.rowptr) >= 0).all() and c.rowptr.size == len(c.links) + 1
    assert c.ids.size == 0 or (0 <= c.ids.min() and c.ids.max() < c.N)
    assert 0 <= c.links.min() and c.links.max() < c.N and 0 <= c.ei.min() and c.ei.max() < c.N
    for q, (u, v) in enumerate(c.links):
        row = c.ids[c.rowptr[q]:c.rowptr[q + 1]]
        assert row.size == 0 or ((np.diff(row) > 0).all() and u in row and v in row)
    rowptr, col = c.csr()
    assert rowptr[-1] == col.size == c.ei.shape[1] and col.dtype == np.int32 and rowptr.dtype == np.int64
    for x in np.unique(c.ids):
        assert (np.diff(c.in_row(x)) >= 0).all()


@pytest.mark.parametrize('name', list(planted.LABEL_CASES))
def test_label_cases_keep_the_kernel_contract(label_cases, name):
    c = label_cases(name)
    assert c.rowptr[0] == 0 and c.adj_ptr[0] == 0 and c.adj_ptr.size == c.T + 1 and c.adj_ptr[-1] == c.nbr.size
    assert c.roots.shape == (c.B, 2) and c.roots.dtype == c.nbr.dtype == np.int32
    sizes = np.diff(c.rowptr)
    owner = np.repeat(np.repeat(sizes, sizes), np.diff(c.adj_ptr))  # the row length that bounds every nbr entry
    assert (c.nbr >= 0).all() and (c.nbr < owner).all()
    full = sizes > 0
    assert (c.roots[full] >= 0).all() and (c.roots[full] < sizes[full, None]).all() and (c.roots[~full] == planted.PRESET_ROOT).all()


# ---- adjacency claims ------------------------------------------------------------------------------------------------------------------------
def test_runs_sit_where_the_steps_end(adj_cases):
    c = adj_cases('runs')
    x, v, layout = c.claims['x'], c.claims['v'], c.claims['layout']
    col, row = c.in_row(x), c.ids[:c.rowptr[1]]
    assert col.size == c.claims['deg'] == 95 and col.size % G != 0
    for s, (first, copies, listed) in layout.items():
        at = np.flatnonzero(col == s)
        assert at.tolist() == list(range(first, first + copies)) and listed == (s in row and s != x)
    first, copies, _ = layout[30]  # starts on lane 15 and goes on into the next step
    assert first % G == G - 1 and copies == 4 and (first + copies - 1) // G == first // G + 1
    first, copies, _ = layout[80]  # a whole step inside one run, which starts on lane 0
    assert copies == 40 and first % G == 0 and first + G <= 64 and 80 <= first + copies
    first, copies, _ = layout[x]  # self loops across a step's end
    assert (first, copies) == (31, 3) and first // G != (first + copies - 1) // G
    assert layout[v][1] == 3 and layout[v][2]
    first, copies, listed = layout[100]  # the last run is listed and ends at deg
    assert first + copies == col.size and listed and row[-1] == 100
    unlisted = [s for s, (_, _, listed) in layout.items() if not listed and s != x]
    assert min(unlisted) < row[0] and any(row[0] < s < row[-1] for s in unlisted)
    assert c.in_row(v).max() > row[-1] and (c.in_row(v) == x).sum() == 3  # loc == n, and the partner of x = v
    assert c.links.tolist() == [[x, v], [v, x], [x, x]]


def test_steps_find_what_they_claim(adj_cases):
    c = adj_cases('steps')
    row = c.ids
    degs = []
    for x, (deg, pattern, _) in c.claims['targets'].items():
        col = c.in_row(x)
        degs.append(deg)
        assert col.size == deg and (np.diff(col) > 0).all() and x in row
        found = np.isin(col, row) & (col != x)
        assert [int(found[s:s + G].sum()) for s in range(0, deg, G)] == pattern
    assert set(degs) == {0, 1, 15, 16, 17, 31, 32, 33, 48}
    patterns = [p for _, p, _ in c.claims['targets'].values()]
    whole = {f for deg, p, _ in c.claims['targets'].values() for s, f in enumerate(p) if deg - G * s >= G}
    assert whole == {0, 1, 16}  # what a step of 16 positions contributes
    assert [16, 1] in patterns and [1, 16] in patterns and [16, 16, 1] in patterns  # a later step placed after totals of 16, 1 and 32
    every = np.concatenate([c.in_row(x) for x in c.claims['targets']])
    assert every.min() < row[0] and every.max() > row[-1]
    assert row.size * planted.DEFAULT_SWITCH > max(degs)  # the default ratio walks the arcs everywhere


@pytest.mark.parametrize('name', ['switch', 'switch_probe'])
def test_switch_nodes_sit_on_the_boundary(adj_cases, name):
    c = adj_cases(name)
    blocks = c.claims['blocks']
    want = {(s, n) for s in planted.SWITCH_RATIOS for n in planted.SWITCH_ROWS if n >= 2 or name == 'switch'}
    assert {(b['ratio'], b['n']) for b in blocks if not b['by_ids']} == {(b['ratio'], b['n']) for b in blocks if b['by_ids']} == want
    weights = set()
    for b in blocks:
        q, x = b['link'], b['x']
        row = c.ids[c.rowptr[q]:c.rowptr[q + 1]]
        col = c.in_row(x)
        assert row.size == b['n'] and x in row and col.size == b['deg']
        assert b['deg'] == b['ratio'] * b['n'] + (1 if b['by_ids'] else 0) and b['by_ids'] == (b['deg'] > b['ratio'] * b['n'])
        j, w = np.unique(col[np.isin(col, row)], return_counts=True)
        weights |= set(w.tolist())
        if b['outer']:
            assert row[0] < row[1] < col.min() and col.max() < row[-2] < row[-1] and j.size >= 2
        if name == 'switch_probe':
            assert b['deg'] >= 2 and (np.diff(col) > 0).all() and j.size >= 1
            a = planted.descending_csr(c)[1][c.csr()[0][x]:c.csr()[0][x + 1]]
            assert (np.diff(a) < 0).all() and sorted(a.tolist()) == col.tolist()
    assert weights == ({1} if name == 'switch_probe' else {2, 5})


def test_empty_rows_and_sweep_shapes(adj_cases):
    c = adj_cases('empty_rows')
    sizes = np.diff(c.rowptr)
    assert len(c.links) == 9 and np.flatnonzero(sizes == 0).tolist() == c.claims['empty'] == [0, 3, 4, 8]
    assert c.T == c.claims['T'] and c.T % G != 0
    for q in c.claims['single']:
        assert sizes[q] == 1 and c.links[q, 0] == c.links[q, 1]
    assert c.in_row(59).size == 0 and 7 in c.in_row(7)
    c = adj_cases('sweep')
    sizes = np.diff(c.rowptr)
    assert c.T == c.claims['T'] and c.T - planted.ADJ_SWEEP == 21 and c.T % G == 5
    assert (sizes[:66] > 1000).all() and abs(int(np.median(sizes[:66])) - 2000) < 50 and sizes[66:].tolist() == [0, 0]
    assert 3000 <= c.N <= 5000


# ---- adjacency_of_rows against scipy ---------------------------------------------------------------------------------------------------------
# (sweep: 131 093 listed nodes through the per-node loop once, masked)
@pytest.mark.parametrize('name,mask', [(n, m) for n in list(planted.ADJ_CASES) + ['switch_probe'] for m in (False, True) if m or n != 'sweep'])
def test_adjacency_of_rows_is_the_sliced_matrix(adj_cases, name, mask):
    c = adj_cases(name)
    got = sr.adjacency_of_rows(c.N, c.ei, c.links, c.rowptr, c.ids, mask)
    for g, w, what in zip(got, scipy_adjacency(c, mask), ('roots', 'adj_ptr', 'nbr', 'weight')):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w, err_msg=what)
    if name == 'runs':  # what the planted runs come to: the weights of x's row in the first link
        x, v, layout = c.claims['x'], c.claims['v'], c.claims['layout']
        t = int(np.searchsorted(c.ids[:c.rowptr[1]], x))
        want = [copies for s, (_, copies, listed) in layout.items() if listed and not (mask and s == v)]
        assert got[3][got[1][t]:got[1][t + 1]].tolist() == want
    if name == 'switch':
        assert set(got[3].tolist()) == {2, 5}


# ---- bfs against scipy -----------------------------------------------------------------------------------------------------------------------
def _scipy_depths(ptr, nbr, root, removed=-1):
    n = len(ptr) - 1
    tgt = np.repeat(np.arange(n), np.diff(ptr))
    keep = (nbr != removed) & (tgt != removed)
    A = sp.csr_matrix((np.ones(int(keep.sum())), (tgt[keep], nbr[keep])), shape=(n, n))  # the walk goes from y to nbr[y]
    d = csgraph.shortest_path(A, method='D', unweighted=True, indices=root)
    out = np.where(np.isinf(d), 0, d).astype(np.int64)
    out[np.isinf(d)] = sr.INF
    return out


def _rows_to_check(c):
    if c.name != 'many':
        return range(c.B)
    k = planted.many_kinds()
    return [q for q in range(0, c.B, 97) if k[q] != 2] + list(range(c.B - 7, c.B))


@pytest.mark.parametrize('name', list(planted.LABEL_CASES))
def test_bfs_is_scipy_shortest_path(label_cases, name):
    c = label_cases(name)
    for q in _rows_to_check(c):
        ptr, nbr, ru, rv = c.row(q)
        if len(ptr) == 1:
            continue
        for root, other in ((ru, rv), (rv, ru)):
            np.testing.assert_array_equal(sr.bfs(ptr, nbr, root), _scipy_depths(ptr, nbr, root), err_msg=f'{name} row {q}')
            if other != root and len(ptr) - 1 <= 300:
                want = _scipy_depths(ptr, nbr, root, other)
                want[other] = sr.INF
                np.testing.assert_array_equal(sr.bfs(ptr, nbr, root, other), want, err_msg=f'{name} row {q} without {other}')


# ---- label claims ----------------------------------------------------------------------------------------------------------------------------
def _levels(ptr, nbr, root, removed=-1):
    d = sr.bfs(ptr, nbr, root, removed)
    return np.bincount(d[d != sr.INF]).tolist()


def test_path_depths_pass_the_clip_and_fill_the_queue(label_cases):
    c = label_cases('path')
    assert c.claims['sizes'] == (2048, 2049, 5000) == tuple(np.diff(c.rowptr)[::2]) and planted.LDS_NODES == 2048
    for k, n in enumerate(c.claims['sizes']):
        ptr, nbr, ru, rv = c.row(2 * k)
        assert (ru, rv) == (0, n - 1) and _levels(ptr, nbr, ru) == [1] * n  # n - 1 levels, the queue's entry n - 1 written
        assert n - 1 == c.claims['depth'][k] > 1000 and n - 1 < planted.MAX_DIST_TOP
        ptr, nbr, ru, rv = c.row(2 * k + 1)
        assert rv == ru + 1 == n // 2 and int(nbr[ptr[ru]:ptr[ru + 1]].max()) == rv
        assert len(_levels(ptr, nbr, ru, rv)) == n // 2 and len(_levels(ptr, nbr, ru)) == n - n // 2 + 1 > 1000
    assert set(c.max_dists) == {1, 3, 1000, planted.MAX_DIST_TOP}


def test_wide_frontiers(label_cases):
    c = label_cases('wide')
    stars = c.claims['stars']
    assert stars == (15, 16, 17, 255, 256, 257)
    for r, k in enumerate(stars):
        ptr, nbr, ru, rv = c.row(r)
        assert ru == rv and _levels(ptr, nbr, ru) == [1, k]
        ptr, nbr, ru, rv = c.row(len(stars) + r)
        assert ru != rv and _levels(ptr, nbr, ru) == [1, k] and _levels(ptr, nbr, rv) == [1, 1, k - 1] and _levels(ptr, nbr, ru, rv) == [1, k - 1]
    q, side0, side1 = c.claims['two_trees']
    ptr, nbr, ru, rv = c.row(q)
    assert _levels(ptr, nbr, ru) == side0 == [1, 5, 16] and _levels(ptr, nbr, rv) == side1 == [1, 30, 1]
    assert side0[1] < G < side0[1] + side1[1] and side0[2] == G  # the sides change inside a pass of 16, then exactly at one
    q, side0 = c.claims['bipartite']
    ptr, nbr, ru, rv = c.row(q)
    assert _levels(ptr, nbr, ru) == side0 == [1, 64, 64]
    low = np.arange(65, 129)
    assert all(np.diff(ptr)[j] == 64 for j in low) and rv == 128  # each of the 64 is reached from all 64 frontier nodes


def test_cut_directed_one_root_far(label_cases):
    c = label_cases('cut')
    ptr, nbr, ru, rv = c.row(0)
    far = c.claims['far']
    assert sr.bfs(ptr, nbr, ru)[far].tolist() == c.claims['de'] and (sr.bfs(ptr, nbr, ru, rv)[far] == sr.INF).all()
    assert (sr.link_labels(ptr, nbr, ru, rv, 'de+', 1000)[far, 0] == 1000).all()
    assert sr.link_labels(ptr, nbr, ru, rv, 'de', 1000)[far, 0].tolist() == [3, 4, 5]
    assert c.row(1)[2:] == (rv, ru)
    c = label_cases('directed')
    for q in range(c.B):
        ptr, nbr, ru, rv = c.row(q)
        A = sp.csr_matrix((np.ones(nbr.size), (np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), nbr)), shape=(len(ptr) - 1,) * 2)
        assert (A != A.T).nnz > 0
    ptr, nbr, ru, rv = c.row(0)
    assert sr.bfs(ptr, nbr, ru)[rv] != sr.bfs(ptr, nbr, rv)[ru]
    c = label_cases('one_root')
    assert (c.roots[:, 0] == c.roots[:, 1]).all() and 1 in np.diff(c.rowptr)
    c = label_cases('far')
    assert c.T == 3 and c.nbr.size == 0 and c.roots.tolist() == [[0, 1]] and c.max_dists == (1, planted.MAX_DIST_TOP)
    z = sr.link_labels(*c.row(0), 'drnl', planted.MAX_DIST_TOP)
    assert z.dtype == np.int64 and z.tolist() == [1, 1, c.claims['drnl_top']] and c.claims['drnl_top'] == 2 ** 40 + 1 > 2 ** 32
    assert sr.link_labels(*c.row(0), 'drnl', 1).tolist() == [1, 1, 2]


def test_limits_rows_sit_on_the_tier_edge(label_cases):
    c = label_cases('limits')
    sizes = np.diff(c.rowptr)
    assert tuple(sizes) == c.claims['sizes'] == (17, 18, 2048, 2049) and c.lds == (17, 2048, 4096)
    for lds in c.lds:
        limit = min(lds, planted.LDS_NODES)
        assert limit in sizes and limit + 1 in sizes
        ws = planted.ws_ptr(c.rowptr, lds)
        assert sizes[np.diff(ws) > 0].tolist() == c.claims['workspace'][lds] and ws[-1] == sum(c.claims['workspace'][lds])
    np.testing.assert_array_equal(planted.ws_ptr(c.rowptr, 4096), planted.ws_ptr(c.rowptr, 2048))


def test_many_kinds_follow_each_other(label_cases):
    c = label_cases('many')
    grid = planted.LABEL_GRID
    assert c.B == c.claims['B'] == 2 * 1536 + 7 and grid == 1536 and c.lds == (planted.MANY_LDS,) == (24,)
    k = planted.kinds(c, planted.MANY_LDS)
    np.testing.assert_array_equal(k, planted.many_kinds())  # the rows are of the kinds they were made as
    assert np.diff(c.rowptr).max() <= 60
    follows = set()
    for w in range(grid):
        seq = k[w::grid].tolist()
        assert len(seq) == (3 if w < 7 else 2) and len(set(seq)) == len(seq)
        follows |= set(zip(seq[:-1], seq[1:]))
    assert follows == {(a, b) for a in range(4) for b in range(4) if a != b}
    ws = planted.ws_ptr(c.rowptr, planted.MANY_LDS)
    assert ws[-1] == np.diff(c.rowptr)[k == 1].sum() > 0 and np.diff(c.rowptr)[k != 1].max() <= planted.MANY_LDS
    # max_dist 3 clips strictly inside the reachable depths of some row
    deep = [q for q in range(0, c.B, 50) if k[q] == 1 and _levels(*c.row(q)[:3])[4:]]
    assert deep and 3 in c.max_dists
