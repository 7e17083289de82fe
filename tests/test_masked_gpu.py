"""ElphHashes.get_subgraph_features(mask_target=edge_index) and exact_subgraph_features(mask_target=True) on the GPU (masked.py,
csrc/ss_masked.hip, csrc/ss_exact.hip).  References: the numpy restatement of the rule (tests/masked_restatement.py, pinned on one oracle
rebuild per link by tests/test_masked_host.py), the oracle's leave-one-out rebuild itself, the engine's own other route
(update_hash_tables(removed=...) + the plain query) and the scipy restatement of the exact features on the graph minus the link.
Integers (MinHash match counts, HLL union zero counts, zero counts of the masked rows, which links were masked) bit-exact; features
within DESIGN 4's bar (rtol 1e-5, atol 1e-5 * 4 * max|cards|); rows of links that are not edges torch.equal to the plain query."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import exact_restatement as er
import masked_restatement as mr
import update_restatement as ur
from conftest import load_golden, oracle_params
from oracle import oracle

pytestmark = pytest.mark.gpu

COLLAB_N, COLLAB_E_UND = 235868, 1179052
SHAPES = [(128, 8), (64, 6), (256, 10), (8, 4)]


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, h=2, num_perm=128, p=8, **kw):
    args = dict(max_hash_hops=h, hll_p=p, minhash_num_perm=num_perm, floor_sf=False, use_zero_one=True)
    args.update(kw)
    return ssa.ElphHashes(Namespace(**args))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bar(got, want, cards, what=''):
    mr.assert_features_bar(got, want, cards, what)


def check_engine(ssa, dev, n, ei, links, h, num_perm=128, p=8, expect_masked=None, **flags):
    """the masked call against the restatement on the oracle's full-graph tables -> (engine features, debug)"""
    eh = _eh(ssa, h, num_perm, p, **flags)
    prm = oracle_params(eh.hll_tables)
    ei_t = _t(ei, dev)
    table, cards = eh.build_hash_tables(n, ei_t)
    feats, dbg = eh.get_subgraph_features(_t(links, dev), table, cards, mask_target=ei_t, return_debug=True)
    otab, ocards = oracle.build_hash_tables(n, ei, h, num_perm, prm)
    want, wdbg = mr.masked_query(links, n, ei, otab, ocards, h, prm, use_zero_one=eh.use_zero_one, floor_sf=eh.floor_sf)
    assert dbg['masked'].dtype == torch.bool and dbg['match'].dtype == torch.int32
    assert np.array_equal(dbg['masked'].cpu().numpy(), wdbg['masked'])
    for key in ('match', 'zeros', 'row_zeros'):
        got = dbg[key].cpu().numpy()
        bad = np.flatnonzero((got != wdbg[key]).reshape(len(got), -1).any(axis=1))
        assert not len(bad), f'{key}: {len(bad)} links differ, first {np.asarray(links)[bad[:5]].tolist()}: {got[bad[:2]].tolist()} != {wdbg[key][bad[:2]].tolist()}'
    got = feats.cpu().numpy()
    print(f'N={n} h={h} shape=({num_perm},{p}) links={len(got)} masked={int(wdbg["masked"].sum())} max|feature diff|={float(np.abs(got - want).max()):.3g}')
    _bar(got, want, ocards)
    if expect_masked is not None:
        assert wdbg['masked'].tolist() == list(expect_masked)
    eh.check_errors()
    return eh, table, cards, feats, dbg


def _ba40():
    g = load_golden('g3_g4_ba40.npz')
    return int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)


def _uniform3000():
    n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
    e = np.random.RandomState(seed).randint(0, n, size=(2, e_und)).astype(np.int64)
    return n, np.concatenate([e, e[::-1]], axis=1)


def _non_edges(n, ei, count, seed):
    """`count` random pairs with u != v and neither direction in ei"""
    keys = np.unique(ei[0] * n + ei[1])
    rng = np.random.RandomState(seed)
    out = np.zeros((0, 2), dtype=np.int64)
    while len(out) < count:
        c = rng.randint(0, n, size=(2 * count, 2)).astype(np.int64)
        ok = (c[:, 0] != c[:, 1]) & ~np.isin(c[:, 0] * n + c[:, 1], keys) & ~np.isin(c[:, 1] * n + c[:, 0], keys)
        out = np.concatenate([out, c[ok]])
    return out[:count]


def _edge_links(ei, count, seed):
    pick = np.random.RandomState(seed).choice(ei.shape[1], size=count, replace=False)
    links = ei[:, pick].T
    return np.ascontiguousarray(links[links[:, 0] != links[:, 1]])


# ---- against the restatement / oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('num_perm,p', SHAPES)
def test_ba40_every_edge_and_40_non_edges(ssa, dev, num_perm, p, h):
    n, ei = _ba40()
    links = np.concatenate([ei.T, _non_edges(n, ei, 40, 5)])
    check_engine(ssa, dev, n, ei, links, h, num_perm, p, expect_masked=[True] * ei.shape[1] + [False] * 40)


@pytest.mark.parametrize('num_perm,p', SHAPES)
def test_uniform3000_256_edge_links(ssa, dev, num_perm, p):
    n, ei = _uniform3000()
    links = _edge_links(ei, 256, 3)
    assert len(links) >= 250
    check_engine(ssa, dev, n, ei, links, 3, num_perm, p, expect_masked=[True] * len(links))


@pytest.mark.parametrize('h', [1, 2, 3])
def test_directed_graph_where_only_one_direction_exists(ssa, dev, h):
    rng = np.random.RandomState(17)
    n = 80
    ei = rng.randint(0, n, size=(2, 200)).astype(np.int64)
    have = set(map(tuple, ei.T.tolist()))
    one_way = [(u, v) for u, v in ei.T.tolist() if u != v and (v, u) not in have][:30]
    links = np.array(one_way + [(v, u) for u, v in one_way[:10]], dtype=np.int64)
    check_engine(ssa, dev, n, ei, links, h, expect_masked=[True] * 40)


@pytest.mark.parametrize('h', [2, 3])
@pytest.mark.parametrize('flags', [{}, {'use_zero_one': False, 'floor_sf': True}])
def test_duplicated_edges_self_edges_and_u_equals_v(ssa, dev, h, flags):
    rng = np.random.RandomState(23)
    n = 60
    e = rng.randint(0, n, size=(2, 90)).astype(np.int64)
    ei = np.concatenate([e, e[::-1], e[:, :30], e[::-1][:, :10]], axis=1)
    x = rng.randint(0, n, size=6)
    ei = np.concatenate([ei, np.stack([x, x])], axis=1)
    dup = e[:, :30].T
    dup = dup[dup[:, 0] != dup[:, 1]]
    links = np.concatenate([dup, [[int(x[0]), int(x[0])], [7, 7], [-1, -2]]]).astype(np.int64)  # (negative ids wrap, as in the plain query)
    check_engine(ssa, dev, n, ei, links, h, **flags)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_trailing_isolated_nodes(ssa, dev, h):
    g = load_golden('g7_edge_cases.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    edges = np.array([e for e in ei.T.tolist() if e[0] != e[1]], dtype=np.int64)
    links = np.concatenate([edges, [[10, 3], [11, 9], [2, 11]]]).astype(np.int64)
    check_engine(ssa, dev, n, ei, links, h, expect_masked=[True] * len(edges) + [False] * 3)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_n_self_stays_that_of_the_full_edge_list(ssa, dev, h):
    rng = np.random.RandomState(29)
    e = rng.randint(0, 30, size=(2, 50)).astype(np.int64)
    ei = np.concatenate([e, e[::-1], [[4, 37], [37, 4]]], axis=1)
    check_engine(ssa, dev, 40, ei, np.array([[4, 37], [37, 4], [36, 4]]), h, expect_masked=[True, True, False])


@pytest.mark.parametrize('h', [1, 2])
def test_links_at_the_largest_hub_against_the_oracle(ssa, dev, h):
    """node 0 of the power-law graph collects ~7 000 in-edges (a mega row of the build): links incident to it and to its neighbours,
    each against one oracle rebuild without the link"""
    n = 50000
    ei = ur.power_law_graph(n, 250000, 7)
    deg = np.bincount(ei[1], minlength=n)
    assert int(np.argmax(deg)) == 0 and deg[0] > 2048
    nb0 = np.unique(ei[0][ei[1] == 0])
    nb0 = nb0[nb0 != 0]
    at_hub = [(0, int(nb0[0])), (int(nb0[1]), 0), (0, int(nb0[-1]))]
    near = []
    for w in nb0[2:40].tolist():  # a neighbour of the hub and one of ITS other neighbours
        other = ei[0][(ei[1] == w) & (ei[0] != 0) & (ei[0] != w)]
        if len(other):
            near.append((w, int(other[0])))
        if len(near) == 3:
            break
    assert len(near) == 3
    links = np.array(at_hub + near, dtype=np.int64)
    eh = _eh(ssa, h)
    prm = oracle_params(eh.hll_tables)
    ei_t = _t(ei, dev)
    table, cards = eh.build_hash_tables(n, ei_t)
    feats, dbg = eh.get_subgraph_features(_t(links, dev), table, cards, mask_target=ei_t, return_debug=True)
    assert bool(dbg['masked'].all())
    cmax = float(cards.abs().max())
    for q, (u, v) in enumerate(links.tolist()):
        want_f, want_dbg, want_rows, _ = mr.leave_one_out(u, v, n, ei, h, 128, prm)
        assert np.array_equal(dbg['match'][q].cpu().numpy(), want_dbg['match']), (q, u, v)
        assert np.array_equal(dbg['zeros'][q].cpu().numpy(), want_dbg['zeros']), (q, u, v)
        assert np.array_equal(dbg['row_zeros'][q].cpu().numpy(), (want_rows['hll'] == 0).sum(axis=2)), (q, u, v)
        np.testing.assert_allclose(feats[q].cpu().numpy(), want_f, rtol=1e-5, atol=1e-5 * 4 * cmax, err_msg=f'link ({u}, {v})')


# ---- links that are not edges keep the plain query's bits -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def collab(ssa, dev):
    n = COLLAB_N
    ei = ur.uniform_graph(n, COLLAB_E_UND, 51)
    assert mr.n_self_of(ei) > n - 50
    out = {}
    for h in (2, 3):
        eh = _eh(ssa, h)
        ei_t = _t(ei, dev)
        out[h] = (eh, ei_t) + tuple(eh.build_hash_tables(n, ei_t))
    return n, ei, out


@pytest.mark.parametrize('h', [2, 3])
def test_65536_non_edges_at_collab_size_are_the_plain_query(ssa, dev, collab, h):
    n, ei, built = collab
    eh, ei_t, table, cards = built[h]
    links = _t(_non_edges(n, ei, 65536, 61), dev)
    plain = eh.get_subgraph_features(links, table, cards)
    got, dbg = eh.get_subgraph_features(links, table, cards, mask_target=ei_t, return_debug=True)
    assert not bool(dbg['masked'].any())
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
    assert torch.equal(eh.get_subgraph_features(links, table, cards, mask_target=ei_t).view(torch.int32), plain.view(torch.int32))


def test_mixed_batch_cpu_call_and_small_batches(ssa, dev, collab):
    n, ei, built = collab
    eh, ei_t, table, cards = built[2]
    edges, non = _edge_links(ei, 3000, 62), _non_edges(n, ei, 3000, 63)
    perm = np.random.RandomState(64).permutation(len(edges) + len(non))
    mixed = np.concatenate([edges, non])[perm]
    f_e = eh.get_subgraph_features(_t(edges, dev), table, cards, mask_target=ei_t)
    f_n = eh.get_subgraph_features(_t(non, dev), table, cards, mask_target=ei_t)
    want = torch.cat([f_e, f_n])[torch.from_numpy(perm).to(dev)]
    got, dbg = eh.get_subgraph_features(_t(mixed, dev), table, cards, mask_target=ei_t, return_debug=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(dbg['masked'].cpu().numpy(), (perm < len(edges)))
    assert not torch.equal(f_e, eh.get_subgraph_features(_t(edges, dev), table, cards))  # masking an edge changes its row
    # links and edge_index on the CPU: same rows, on the CPU, in the caller's order
    got_cpu, dbg_cpu = eh.get_subgraph_features(torch.from_numpy(mixed), table, cards, mask_target=torch.from_numpy(ei), return_debug=True)
    assert got_cpu.device.type == 'cpu' and dbg_cpu['masked'].device.type == 'cpu'
    assert torch.equal(got_cpu.view(torch.int32), want.cpu().view(torch.int32))
    # batch_size smaller than L (and not a divisor of it); a 1-D link
    got_b, dbg_b = eh.get_subgraph_features(_t(mixed, dev), table, cards, mask_target=ei_t, batch_size=1777, return_debug=True)
    assert torch.equal(got_b.view(torch.int32), want.view(torch.int32))
    for key in dbg:
        assert torch.equal(dbg_b[key], dbg[key]), key
    one = eh.get_subgraph_features(_t(edges[5], dev), table, cards, mask_target=ei_t)
    assert one.shape == (1, 8) and torch.equal(one[0].view(torch.int32), f_e[5].view(torch.int32))
    assert eh.get_subgraph_features(torch.zeros((0, 2), dtype=torch.int64), table, cards, mask_target=ei_t).shape == (0, 8)


@pytest.mark.parametrize('h', [2, 3])
def test_agrees_with_update_hash_tables_then_the_plain_query(ssa, dev, collab, h):
    """the engine's own other route, one link at a time: remove both directions with update_hash_tables(copy=True), query plainly"""
    n, ei, built = collab
    eh, ei_t, table, cards = built[h]
    links = _edge_links(ei, 6, 65 + h)
    got, dbg = eh.get_subgraph_features(_t(links, dev), table, cards, mask_target=ei_t, return_debug=True)
    assert bool(dbg['masked'].all())
    cmax = float(cards.abs().max())
    for q, (u, v) in enumerate(links.tolist()):
        new = mr.without_link(ei, u, v)
        assert mr.n_self_of(new) == mr.n_self_of(ei)  # a uniform graph keeps max(edge_index) in place: the two routes see the same self loops
        removed = np.array([[u, v], [v, u]], dtype=np.int64)
        t2, c2 = eh.update_hash_tables(table, cards, n, _t(new, dev), removed=_t(removed, dev), copy=True)
        f2, d2 = eh._pair_kernel(_t(links[q:q + 1], dev), t2, c2, want_debug=True)
        assert torch.equal(d2['match'][0], dbg['match'][q]) and torch.equal(d2['zeros'][0], dbg['zeros'][q]), (u, v)
        np.testing.assert_allclose(got[q].cpu().numpy(), f2[0].cpu().numpy(), rtol=1e-5, atol=1e-5 * 4 * cmax, err_msg=f'link ({u}, {v})')


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def test_out_of_range_ids_give_nan_rows_and_index_errors(ssa, dev):
    n, ei = _ba40()
    ei_t = _t(ei, dev)
    links = _t(np.array([[int(ei[0, 0]), int(ei[1, 0])], [3, n + 4], [-n - 1, 2]], dtype=np.int64), dev)
    eh = _eh(ssa, 2)
    table, cards = eh.build_hash_tables(n, ei_t)
    eh.strict_bounds = False
    got, dbg = eh.get_subgraph_features(links, table, cards, mask_target=ei_t, return_debug=True)
    assert bool(torch.isnan(got[1:]).all()) and not bool(torch.isnan(got[0]).any())
    assert dbg['masked'].tolist() == [True, False, False]
    eh.strict_bounds = True
    with pytest.raises(IndexError):
        eh.get_subgraph_features(links, table, cards, mask_target=ei_t)
    eh.strict_bounds = 'deferred'
    eh.get_subgraph_features(links, table, cards, mask_target=ei_t)
    with pytest.raises(IndexError):
        eh.check_errors()


def test_reference_format_tables_are_accepted(ssa, dev):
    n, ei = _ba40()
    ei_t = _t(ei, dev)
    eh = _eh(ssa, 2)
    table, cards = eh.build_hash_tables(n, ei_t)
    links = _t(ei.T[:20], dev)
    want = eh.get_subgraph_features(links, table, cards, mask_target=ei_t)
    plain = {k: {'minhash': table[k]['minhash'].cpu(), 'hll': table[k]['hll'].cpu()} for k in range(3)}
    got = eh.get_subgraph_features(links, plain, cards.cpu(), mask_target=ei_t)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- the exact companion --------------------------------------------------------------------------------------------------------------
def _scipy_on_g_uv(n, ei, links, h):
    """the scipy restatement link by link on the graph minus the link, n_self pinned by listing the full graph's self loops"""
    n_self = mr.n_self_of(ei)
    loops = np.arange(n_self, dtype=np.int64)
    outs = []
    for u, v in links.tolist():
        e2 = np.concatenate([mr.without_link(ei, u, v), np.stack([loops, loops])], axis=1)
        outs.append(er.restate(n, e2, np.array([[u, v]]), h))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3))


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('graph', ['ba40', 'uniform3000'])
def test_exact_companion_against_scipy_on_the_graph_minus_the_link(ssa, dev, graph, h):
    n, ei = _ba40() if graph == 'ba40' else _uniform3000()
    edges = ei.T if graph == 'ba40' else _edge_links(ei, 200, 71)
    links = np.concatenate([edges, _non_edges(n, ei, 20, 72), [[3, 3]]]).astype(np.int64)
    eh = _eh(ssa, h)
    ei_t = _t(ei, dev)
    feats, I, balls = eh.exact_subgraph_features(_t(links, dev), n, ei_t, return_counts=True, mask_target=True)
    wf, wI, wb = _scipy_on_g_uv(n, ei, links, h)
    assert np.array_equal(I.cpu().numpy(), wI) and np.array_equal(balls.cpu().numpy(), wb)
    assert np.array_equal(feats.cpu().numpy().view(np.int32), wf.view(np.int32))
    # mask_target=False is today's call, byte for byte -- and differs from the masked one on an edge
    today = eh.exact_subgraph_features(_t(links, dev), n, ei_t, return_counts=True)
    off = eh.exact_subgraph_features(_t(links, dev), n, ei_t, return_counts=True, mask_target=False)
    for a, b in zip(today, off):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    rf, rI, rb = er.restate(n, ei, links, h)
    assert np.array_equal(today[1].cpu().numpy(), rI) and np.array_equal(today[2].cpu().numpy(), rb)
    assert not torch.equal(today[1][:len(edges)], I[:len(edges)])


def test_exact_companion_large_tier(ssa, dev, monkeypatch):
    """the large tier reads the same flag: every pair forced off the on-chip tier"""
    monkeypatch.setattr(ssa.knobs, 'EXACT_LDS_MAX_NODES', 0)
    n, ei = _uniform3000()
    links = _edge_links(ei, 60, 73)
    eh = _eh(ssa, 3)
    feats, I, balls = eh.exact_subgraph_features(_t(links, dev), n, _t(ei, dev), return_counts=True, mask_target=True)
    wf, wI, wb = _scipy_on_g_uv(n, ei, links, 3)
    assert np.array_equal(I.cpu().numpy(), wI) and np.array_equal(balls.cpu().numpy(), wb)
    assert np.array_equal(feats.cpu().numpy().view(np.int32), wf.view(np.int32))
