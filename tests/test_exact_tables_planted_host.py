"""CPU tests of what tests/test_exact_tables_planted_gpu.py trusts (tests/exact_tables_planted.py): the module's constants against the
text of csrc/ss_exact_bfs.hpp, so a changed hash or tier constant cannot quietly turn the planted collisions into ordinary ids; every
planted piece against its claim, by the probe model and a numpy CSR; and the expected rows -- the restatements on the components the
links touch -- against the restatements on the whole graph, against one another and against closed forms."""
import os
import re

import numpy as np
import pytest

import exact_nodes_restatement as nr
import exact_restatement as er
import exact_tables_planted as planted
import subgraph_restatement as sr
from conftest import REPO

HEADER = os.path.join(REPO, 'subgraph-sketching_amd', 'csrc', 'ss_exact_bfs.hpp')


@pytest.fixture(scope='module')
def g():
    return planted.graph()


def _union(g, row, h=1):
    """the ids of B_h(u) | B_h(v) of planted link `row`"""
    rowptr, ids, _ = planted.expected_nodes(g, h, False)
    return ids[rowptr[row]:rowptr[row + 1]]


def _first(g, case, u, v):
    return int(np.nonzero((g.case == case) & (g.links[:, 0] == u) & (g.links[:, 1] == v))[0][0])


# ---- the constants ---------------------------------------------------------------------------------------------------------------------
def test_constants_equal_the_header():
    src = open(HEADER).read()
    const = lambda name: re.search(r'constexpr int %s = ([^;]+);' % name, src).group(1).strip()
    mult, shift = re.search(r'lds_hash\(uint32_t x\) \{ return \(x \* (\d+)u\) >> \(([^)]+)\); \}', src).groups()
    assert int(mult) == planted.HASH_MULTIPLIER and shift == '32 - kExactSlotsLog'
    assert int(const('kExactSlotsLog')) == planted.SLOT_BITS == 12 and planted.HASH_SHIFT == 32 - planted.SLOT_BITS
    assert const('kExactSlots') == '1 << kExactSlotsLog' and planted.SLOTS == 4096
    assert const('kExactMaxNodes') == 'kExactSlots / 2' and planted.NODE_LIMIT == 2048
    assert int(const('kBigDegree')) == planted.BIG_DEGREE and int(const('kBigList')) == planted.BIG_LIST
    assert int(const('kScanWords')) == planted.SCAN_WORDS and int(const('kExactThreads')) == planted.THREADS
    assert const('kExactGrid') == '256 * 4' and planted.LDS_GRID == 1024
    assert planted.SCAN_STEP == planted.SCAN_WORDS * planted.THREADS * planted.NODES_PER_WORD == 4096
    # the probe wraps with & (kExactSlots - 1), one level byte per node and four to a word, > kBigDegree goes on the big list
    assert src.count('i = (i + 1) & (kExactSlots - 1);') == 2
    assert 'return (N + 3) / 4; }' in src and 'const int sh = 8 * (x & 3);' in src
    assert src.count('if (e1 - e0 > kBigDegree) {') == 1 and 'w0 += kScanWords * kExactThreads' in src
    assert planted.GROUP_LANES == 16 and re.search(r'constexpr int kRow = 16;', open(os.path.join(os.path.dirname(HEADER), 'ss_common.hpp')).read())


def test_hash_twin_known_answers():
    """lds_hash by hand: 32-bit wrapping multiply, top 12 bits"""
    assert int(planted.home(0)) == 0 and int(planted.home(1)) == 2654435761 >> 20 == 2531
    assert int(planted.home(2)) == ((2 * 2654435761) % (1 << 32)) >> 20 == 966
    x = np.arange(planted.N)
    np.testing.assert_array_equal(planted.home(x), [((int(i) * 2654435761) % (1 << 32)) >> 20 for i in x[:2000]] + list(planted.home(x[2000:])))
    per_home = np.bincount(planted.home(x), minlength=planted.SLOTS)
    assert per_home.min() >= 23 and per_home.max() <= 26 and per_home[planted.ONE_HOME] == 26


def test_probe_model_occupied_set_is_order_free():
    rng = np.random.RandomState(3)
    ids = np.concatenate([np.nonzero(planted.home(np.arange(planted.N)) >= planted.WRAP_FROM)[0], rng.choice(50000, 900, replace=False) + 50000])
    ids = np.unique(ids)
    occ, slot_of, moved = planted.probe(ids)
    assert len(occ) == len(ids) and sorted(slot_of.values()) == occ.tolist()
    assert all((int(planted.home(x)) + d) % planted.SLOTS == slot_of[x] for x, d in moved.items())
    for _ in range(3):
        occ2, slot2, _ = planted.probe(ids, order=rng.permutation(ids))
        np.testing.assert_array_equal(occ, occ2)
    assert slot2 != slot_of  # (the places do move)


# ---- the planted claims ----------------------------------------------------------------------------------------------------------------
def test_graph_shape(g):
    assert g.n == planted.N and int(g.ei.max()) == g.n - 1 and int(g.ei.min()) == 0  # n_self = N: every root has its self loop
    pairs = set(zip(g.ei[0].tolist(), g.ei[1].tolist()))
    assert all((b, a) in pairs for a, b in pairs) and not any(a == b for a, b in pairs)  # undirected, no loops listed
    np.testing.assert_array_equal(g.degree, np.bincount(g.ei[1], minlength=g.n))
    assert len(g.links) >= 50 and set(g.case) == {'scan_edges', 'scan_edges_top', 'one_home', 'wrap', 'window', 'window_two_hubs',
                                                  'window_2048', 'window_2049', 'halves', 'raced_key', 'big_boundary'}
    both = {(u, v) for u, v in g.links.tolist()}
    for c in ('one_home', 'wrap', 'window', 'window_two_hubs', 'window_2048', 'window_2049', 'raced_key', 'big_boundary', 'scan_edges'):
        assert all((v, u) in both for u, v in g.links[g.rows_of(c)].tolist()), c
    # the pieces share no node: every component holds one piece
    planted.restrict(g, g.links)  # (labels the components)
    comp_of = g._component
    hubs = [g.names[k]['hub'] for k in ('scan_edges', 'one_home', 'wrap', 'raced_key')] + g.names['window']['hubs'].tolist()
    hubs += [g.names['big_boundary']['t'], g.names['big_boundary']['q']]
    assert len({int(comp_of[x]) for x in hubs}) == len(hubs)
    for k in ('scan_edges', 'one_home', 'wrap', 'raced_key', 'window', 'big_boundary'):
        assert g.degree[g.names[k]['iso']] == 0


def test_one_home_chain(g):
    m = g.names['one_home']
    assert len(m['leaves']) >= 24 and (planted.home(m['leaves']) == planted.ONE_HOME).all()
    row = _first(g, 'one_home', m['hub'], m['iso'])
    ids = _union(g, row)
    assert ids.size == len(m['leaves']) + 2
    occ, _, moved = planted.probe(ids)
    assert set(range(planted.ONE_HOME, planted.ONE_HOME + 24)) <= set(occ.tolist())
    assert max(moved.values()) >= len(m['leaves']) - 1  # the last of the chain, whichever key it is
    leaf = _union(g, _first(g, 'one_home', m['leaves'][0], m['leaves'][-1]), h=2)  # leaf to leaf: the whole star from h = 2 on
    assert set(m['leaves'].tolist()) <= set(leaf.tolist())


def test_wrap_cluster(g):
    m = g.names['wrap']
    assert (planted.home(m['leaves']) >= planted.WRAP_FROM).all() and len(m['leaves']) >= 190
    ids = _union(g, _first(g, 'wrap', m['hub'], m['iso']))
    rng = np.random.RandomState(5)
    for order in (ids, ids[::-1], rng.permutation(ids)):
        occ, slot_of, _ = planted.probe(ids, order=order)
        assert {planted.SLOTS - 1, 0} <= set(occ.tolist())
        below = sum(slot_of[int(x)] < int(planted.home(x)) for x in ids)
        assert below == len(m['leaves']) - 8 >= 100  # eight slots before the end; every other leaf sits below its home


def test_window_unions(g):
    m = g.names['window']
    a, b, c, d, e = m['hubs'].tolist()
    la = m['leaves'][0]
    assert (planted.home(la) >= planted.WINDOW[0]).all() and (planted.home(la) < planted.WINDOW[1]).all() and len(la) > 1500
    one = _union(g, _first(g, 'window', a, m['iso']))
    assert one.size == len(la) + 2 < planted.NODE_LIMIT
    _, _, moved = planted.probe(one)
    assert np.mean([moved[int(x)] for x in la]) > 500  # one cluster ~1 560 long over 64 homes
    sizes = planted.union_sizes(g, 1, False)
    assert sizes[_first(g, 'window_two_hubs', a, b)] == len(la) + len(m['leaves'][1]) + 2 > planted.NODE_LIMIT
    for h in (1, 2, 3):
        for mask in (False, True):
            s = planted.union_sizes(g, h, mask)
            assert s[_first(g, 'window_2048', c, d)] == s[_first(g, 'window_2048', d, c)] == planted.NODE_LIMIT
            assert s[_first(g, 'window_2049', c, e)] == s[_first(g, 'window_2049', e, c)] == planted.NODE_LIMIT + 1


def test_halves_share_a_word_alone(g):
    rows = g.rows_of('halves')
    pairs, quads = g.names['halves']['pairs'], g.names['halves']['quads']
    assert len(rows) == len(pairs) + len(quads)
    rowptr, ids, dist = planted.expected_nodes(g, 3, False)
    rng = np.random.RandomState(7)
    for row, (u, v, x, y, lx, ly) in zip(rows, pairs):
        assert g.links[row].tolist() == [u, v] and lx != ly
        k = int(planted.home(x))
        assert k % 2 == 0 and int(planted.home(y)) == k + 1
        mine = ids[rowptr[row]:rowptr[row + 1]]
        for order in (mine, rng.permutation(mine)):
            occ, slot_of, _ = planted.probe(mine, order=order)
            assert slot_of[x] == k and slot_of[y] == k + 1
            assert not {k - 1, k + 2} & set(occ.tolist())  # nothing is displaced into the word, nothing sits beside it
        d = dict(zip(mine.tolist(), dist[rowptr[row]:rowptr[row + 1]].tolist()))
        assert d[x] == [lx, 4] and d[y] == [4, ly]  # x by u alone, y by v alone, at different levels
    for row, (u, v, q0) in zip(rows[len(pairs):], quads):
        assert g.links[row].tolist() == [u, v] and q0 % planted.NODES_PER_WORD == 0
        d = dict(zip(ids[rowptr[row]:rowptr[row + 1]].tolist(), dist[rowptr[row]:rowptr[row + 1]].tolist()))
        assert [d[q0 + i] for i in range(4)] == [[1, 4], [4, 2], [2, 4], [4, 1]]


def test_raced_key_arcs_come_16_in_a_row(g):
    m = g.names['raced_key']
    assert len(m['leaves']) == planted.RACED_LEAVES and set(planted.home(m['leaves']).tolist()) == set(planted.RACED_HOMES)
    at = np.nonzero(g.ei[1] == m['hub'])[0]
    assert at.size == planted.RACED_LEAVES * planted.GROUP_LANES <= planted.BIG_DEGREE
    src = g.ei[0][at].reshape(-1, planted.GROUP_LANES)
    assert (src == src[:, :1]).all() and np.unique(src[:, 0]).size == planted.RACED_LEAVES
    assert (np.diff(at.reshape(-1, planted.GROUP_LANES), axis=1) == 1).all()  # in a row in edge_index too
    tails = m['tails']
    assert len(tails) == planted.RACED_TAILS and set(planted.home(tails).tolist()) == {planted.RACED_HOMES[0]}
    assert set(planted.home(m['leaves'][:len(tails)]).tolist()) == {planted.RACED_HOMES[0]}
    assert (g.degree[m['leaves'][len(tails):]] == planted.GROUP_LANES).all() and (g.degree[m['leaves'][:len(tails)]] == 2 * planted.GROUP_LANES).all()
    for x, y in zip(m['leaves'], tails):  # a tail's row is ONE source 16 times, whatever order the CSR keeps: 16 lanes, one new key
        assert g.ei[0][g.ei[1] == y].tolist() == [x] * planted.GROUP_LANES
    ids = _union(g, _first(g, 'raced_key', m['hub'], m['iso']))
    assert ids.size == planted.RACED_LEAVES + 2
    _, _, moved = planted.probe(ids)
    assert max(moved.values()) >= planted.RACED_LEAVES // 2 - 1  # a colliding chain
    assert set(_union(g, _first(g, 'raced_key', tails[0], m['iso']), h=3).tolist()) >= set(m['leaves'].tolist()) | {m['hub']}
    # the race happens INSIDE a chain: the kernels insert a side's root before its level 1, so a tail holds the home slot when its
    # leaf arrives in 16 lanes at once, and the second tail's leaf finds three slots taken
    x = [int(v) for v in m['leaves'][:3]]
    t = [int(v) for v in tails[:3]]
    _, _, moved = planted.probe([t[0], x[0], m['iso']])  # (tails[0], isolated) at h = 1: u, level 1 of u, v
    assert moved[t[0]] == 0 and moved[x[0]] == 1
    assert _union(g, _first(g, 'raced_key', t[1], t[2])).tolist() == sorted([t[1], x[1], t[2], x[2]])
    _, _, moved = planted.probe([t[1], x[1], t[2], x[2]])
    assert (moved[x[1]], moved[t[2]], moved[x[2]]) == (1, 2, 3)


def test_big_boundary_degrees(g):
    m = g.names['big_boundary']
    assert g.degree[m['t_kids']].tolist() == [planted.BIG_DEGREE, planted.BIG_DEGREE + 1]
    deg = g.degree[m['q_kids']]
    assert int((deg > planted.BIG_DEGREE).sum()) == planted.BIG_LEVEL >= planted.BIG_LIST + 1 and int((deg == planted.BIG_DEGREE).sum()) == 3
    # all of them form level 1 of hub Q, and each guards two leaves that only its own walk reaches
    rowptr, ids, dist = planted.expected_nodes(g, 2, False)
    row = _first(g, 'big_boundary', m['q'], m['iso'])
    d = dict(zip(ids[rowptr[row]:rowptr[row + 1]].tolist(), dist[rowptr[row]:rowptr[row + 1], 0].tolist()))
    assert all(d[int(k)] == 1 for k in m['q_kids']) and sum(v == 2 for v in d.values()) == 2 * len(m['q_kids'])


@pytest.mark.parametrize('n', [planted.N, planted.ODD_N])
def test_scan_edge_ids(n):
    g = planted.graph(n)
    assert g.n == n and int(g.ei.max()) == n - 1
    leaves = g.names['scan_edges']['leaves']
    assert {0, 4095, 4096, 4097, 8191, 8192, n - 1} <= set(leaves.tolist())
    busy = np.nonzero(g.degree)[0]
    for x in leaves:  # the rest of each level word is never visited
        word = np.arange(4 * (x // 4), min(4 * (x // 4) + 4, n))
        assert set(np.intersect1d(word, busy).tolist()) <= set(leaves.tolist())
    rows = g.rows_of('scan_edges')
    got = set(np.concatenate([_union(g, r, h=2) for r in rows]).tolist())
    assert set(leaves.tolist()) <= got
    if n == planted.ODD_N:
        full = planted.graph(planted.N)
        assert n % 4 != 0 and g.ei.shape[1] == full.ei.shape[1] - 2 and len(g.links) == len(full.links) - 3


def test_reuse_list(g):
    links, of, swapped = planted.reuse_links(g)
    L, grid = len(g.links), planted.LDS_GRID
    assert len(links) >= 3 * grid + 100 and set(of.tolist()) == set(range(L))
    assert (links[~swapped] == g.links[of[~swapped]]).all() and (links[swapped] == g.links[of[swapped]][:, ::-1]).all()
    for w in range(grid):  # a workgroup's rows: link, the same link swapped, the link REUSE_STEP places on, that one swapped, ...
        mine, which = links[w::grid], of[w::grid]
        assert len(mine) >= 6 and len(set(which[:6].tolist())) == 3
        for k in (0, 2, 4):
            assert which[k] == which[k + 1] == (w + planted.REUSE_STEP * (k // 2)) % L and (mine[k + 1] == mine[k][::-1]).all()
    # at the limit of the GPU test, most workgroups serve links of BOTH tiers, and hundreds serve an on-chip link straight after one
    # they abandoned -- by the unions (features, node lists) and by the visited sets of the sampled walk
    uniq, inv = np.unique(links, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    sizes = planted.union_sizes(g, 2, False, uniq)[inv]
    limit = planted.reuse_limit(sizes)
    visited = planted.expected_sampled(g, 2, *planted.REUSE_SAMPLING, uniq)[1][inv]
    assert len(sizes) // 4 < int((sizes > limit).sum()) < (2 * len(sizes)) // 5  # about a third, by the unions
    for size in (sizes, visited):
        assert planted.workgroups_serving_after_an_overflow(size, limit) >= 300


# ---- the expected rows -----------------------------------------------------------------------------------------------------------------
def test_restriction_equals_the_whole_graph(g):
    """the restatements on the touched components give what they give on all of g (a sample of links: every case, both window tiers)"""
    rows = np.concatenate([g.rows_of(c)[:2] for c in sorted(set(g.case))])
    lk = g.links[rows]
    for h, mask in ((1, False), (2, True), (3, False)):
        f, I, balls = planted.expected_features(g, h, mask)
        wf, wI, wb = er.restate(g.n, g.ei, lk, h)
        if not mask:  # (masked: restated per link below, on the node lists)
            np.testing.assert_array_equal(I[rows], wI)
            np.testing.assert_array_equal(balls[rows], wb)
            np.testing.assert_array_equal(f[rows].view(np.int32), wf.view(np.int32))
        want = nr.restate(g.n, g.ei, lk, h, mask_target=mask, directed=True)
        for a, b in zip(planted.take_rows(*planted.expected_nodes(g, h, mask), rows), want):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('mask', [False, True])
def test_restatements_agree(g, h, mask):
    """four implementations, one answer: the ball sizes and intersections of exact_restatement (sparse products) are the counts of the
    (d_u, d_v) rows of exact_nodes_restatement (shortest paths); subgraph_restatement lists the same rows; the sampled walk without
    sampling lists the union with hop = min(d_u, d_v)"""
    _, I, balls = planted.expected_features(g, h, mask)
    rowptr, ids, dist = planted.expected_nodes(g, h, mask)
    for q in range(len(g.links)):
        d = dist[rowptr[q]:rowptr[q + 1]].astype(np.int64)
        for k1 in range(h):
            assert balls[q, 0, k1] == (d[:, 0] <= k1 + 1).sum() and balls[q, 1, k1] == (d[:, 1] <= k1 + 1).sum()
            for k2 in range(h):
                assert I[q, k1, k2] == ((d[:, 0] <= k1 + 1) & (d[:, 1] <= k2 + 1)).sum()
    small = np.nonzero(np.diff(rowptr) < 300)[0]  # (subgraph_restatement walks every listed node's arcs in Python)
    sub = sr.restate(g.n, g.ei, g.links[small], h, mask_target=mask)
    for a, b in zip((sub.rowptr, sub.ids, sub.dist), planted.take_rows(rowptr, ids, dist, small)):
        np.testing.assert_array_equal(a, b)
    if not mask:  # (the sampled walk keeps the target link)
        (sp_ptr, sp_ids, sp_hop), visited, sampled = planted.expected_sampled(g, h, None, 1.0)
        assert sampled == 0
        np.testing.assert_array_equal(sp_ptr, rowptr)
        np.testing.assert_array_equal(sp_ids, ids)
        np.testing.assert_array_equal(sp_hop, dist.min(axis=1))
        np.testing.assert_array_equal(visited, np.diff(rowptr))


def test_closed_forms(g):
    """a star link (hub, isolated): |B_1(hub)| = leaves + 1, |B_k(isolated)| = 1, I = 0, at every h; leaf to leaf: I[0][0] = 1 (the hub),
    I[1][1] = the whole star; hub to leaf with the link masked: the leaf's ball is itself"""
    for name in ('one_home', 'wrap', 'raced_key', 'scan_edges'):
        m = g.names[name]
        L = len(m['leaves'])
        for h in (1, 2, 3):
            _, I, balls = planted.expected_features(g, h, False)
            row = _first(g, name, m['hub'], m['iso'])
            tails = len(m.get('tails', ()))  # (the raced star: a second level behind four of its leaves)
            assert balls[row, 0].tolist() == [L + 1] + [L + 1 + tails] * (h - 1) and (balls[row, 1] == 1).all() and not I[row].any()
            assert not I[_first(g, name, m['iso'], m['hub'])].any()
    for name in ('one_home', 'wrap'):
        m = g.names[name]
        L = len(m['leaves'])
        leaves = g.links[g.rows_of(name)[2]]
        row = _first(g, name, *leaves)
        _, I, balls = planted.expected_features(g, 2, False)
        assert I[row].tolist() == [[1, 2], [2, L + 1]] and balls[row].tolist() == [[2, L + 1], [2, L + 1]]
        hub_leaf = g.links[g.rows_of(name)[4]]
        assert hub_leaf[0] == m['hub']
        _, I, balls = planted.expected_features(g, 3, True)
        row = _first(g, name, *hub_leaf)
        assert balls[row].tolist() == [[L, L, L], [1, 1, 1]] and not I[row].any()
    f, _, _ = planted.expected_features(g, 1, False)
    m = g.names['one_home']
    assert f[_first(g, 'one_home', m['hub'], m['iso'])].tolist() == [0.0, 1.0, len(m['leaves']) + 1.0]


def test_sampled_fringes_run_over_the_chains(g):
    """the settings of the GPU test: a cap of F - 1 drops exactly one node of the hub's fringe, a ratio of 0.5 half of it"""
    for name in ('one_home', 'wrap', 'window'):
        m = g.names[name]
        hub = m['hub'] if name != 'window' else int(m['hubs'][0])
        F = len(m['leaves']) if name != 'window' else len(m['leaves'][0])
        for cap, ratio, kept in ((F - 1, 1.0, F - 1), (None, 0.5, F // 2)):
            (rowptr, ids, hop), visited, sampled = planted.expected_sampled(g, 2, cap, ratio, [[hub, m['iso']]])
            assert rowptr[1] == kept + 2 and visited[0] == F + 2 and (hop == 1).sum() == kept and sampled == 1
