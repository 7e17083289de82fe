"""ElphHashes.update_hash_tables on the GPU (update.py, csrc/ss_update.hip).  Reference in every case: build_hash_tables of the SAME
engine on the new edge list (itself pinned on goldens and oracle by the rest of the suite).  Per case: hop tables torch.equal to the
rebuild; cards within DESIGN 4's bar (rtol 1e-5, atol 1e-5 * 4 * max|cards|); cards outside dirty_k bit-identical to their OLD values
(never written); and, from return_info='masks', the marker's own record equal to the numpy restatement (tests/update_restatement.py) AS
SETS: the byte map of hop k == dirty_k, the row list and the hub list together == dirty_k with each row once, the hub list == the dirty
rows above the CSR's hub threshold, the counters == the lengths -- which a rebuild in disguise cannot meet, because every case first
asserts |dirty_h| < N on the restatement alone.  (A MinHash or HLL row rarely changes when one in-neighbour does: "equal to the
rebuild" alone passes for most rows a marker wrongly skips, and a count passes for a marker that swaps one row for another.)"""
from argparse import Namespace

import numpy as np
import pytest
import torch

import update_restatement as ur
from conftest import load_golden

pytestmark = pytest.mark.gpu

COLLAB_N, COLLAB_E_UND = 235868, 1179052


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, h=2, num_perm=128, p=8):
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=num_perm, floor_sf=False, use_zero_one=True))


def expected_dirty(n, old_ei, new_ei, added, removed, h):
    """the restatement alone: a row had its self loop iff it lies below max(old edge_index) + 1 (what cards_old[:, 0] > 0 says)"""
    had_loop = (np.arange(n) < ur.n_self_of(old_ei)).astype(np.float32)[:, None]
    dirty = ur.dirty_sets(n, new_ei, had_loop, added, removed, h)
    assert dirty[h].sum() < n, f'the case is no restriction: dirty_{h} covers all {n} rows'
    return dirty


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None


def _snapshot(table, cards, h):
    return {k: (table[k].mh_u32.clone(), table[k].hll_u8.clone()) for k in range(1, h + 1)}, cards.clone()


def _assert_cards_bar(got, want):
    want = want.cpu().numpy()
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5 * 4 * float(np.abs(want).max() if want.size else 0.0))


def hub_threshold_of(ssa, new_ei):
    """the threshold build_csr gives the CSR of the update: the knob, or the default for that many edges"""
    forced = ssa.knobs.HUB_THRESHOLD
    return forced if forced is not None else ssa.hashing.default_hub_threshold(np.asarray(new_ei).shape[1])


def assert_marks(ssa, dev, n, new_ei, info, dirty, h):
    """the marker's maps, lists and counters against the restatement, as sets"""
    deg = np.bincount(np.asarray(new_ei, dtype=np.int64)[1], minlength=n)
    above = deg > hub_threshold_of(ssa, new_ei)
    assert info['seed_rows'] == int(dirty[1].sum())
    for k in range(1, h + 1):
        mask = info['dirty_mask'][k]
        assert mask.dtype == torch.bool and mask.device.type == 'cuda' and tuple(mask.shape) == (n,)
        assert torch.equal(mask, torch.from_numpy(dirty[k]).to(dev)), \
            f'hop {k}: the map differs from dirty_{k} at rows {np.flatnonzero(mask.cpu().numpy() != dirty[k])[:8]}'
        assert info['rows'][k].dtype == torch.int32 and info['hubs'][k].dtype == torch.int32
        rows, hubs = info['rows'][k].cpu().numpy(), info['hubs'][k].cpu().numpy()
        listed = np.concatenate([rows, hubs])
        assert np.array_equal(np.sort(listed), np.flatnonzero(dirty[k])), f'hop {k}: the lists are not dirty_{k}, each row once'
        assert np.array_equal(np.sort(hubs), np.flatnonzero(dirty[k] & above)), f'hop {k}: the hub list is not the dirty rows above the threshold'
        assert (info['dirty_rows'][k], info['row_list'][k], info['hub_list'][k]) == (listed.size, rows.size, hubs.size), (k, info['dirty_rows'])


def check_update(ssa, dev, n, old_ei, new_ei, added, removed, h=2, num_perm=128, p=8, copy=False, hubs_at=None):
    """-> (eh, updated table, updated cards, rebuilt table, rebuilt cards, dirty)
    hubs_at: {k: bool}, whether hop k must have listed hub rows (a case that is meant to reach the hub kernels says so)"""
    dirty = expected_dirty(n, old_ei, new_ei, added, removed, h)
    eh = _eh(ssa, h, num_perm, p)
    t_old, c_old = eh.build_hash_tables(n, _t(old_ei, dev))
    snap_t, snap_c = _snapshot(t_old, c_old, h)
    t_ref, c_ref = eh.build_hash_tables(n, _t(new_ei, dev))
    t_up, c_up, info = eh.update_hash_tables(t_old, c_old, n, _t(new_ei, dev), added=_t(added, dev), removed=_t(removed, dev), copy=copy,
                                             return_info='masks')
    if copy:
        assert t_up is not t_old and c_up is not c_old
        for k in range(1, h + 1):  # the inputs are bit-identical to what they were
            assert torch.equal(t_old[k].mh_u32, snap_t[k][0]) and torch.equal(t_old[k].hll_u8, snap_t[k][1])
            assert t_up[k].mh_u32.data_ptr() != t_old[k].mh_u32.data_ptr()
        assert torch.equal(c_old.view(torch.int32), snap_c.view(torch.int32))
    else:
        assert t_up is t_old and c_up is c_old
    assert getattr(c_up, '_ss_tables', None) == eh.tables_id
    assert t_up[0] is t_old[0]  # hop 0 never changes
    print(f'N={n} h={h} shape=({num_perm},{p}) info={ {key: info[key] for key in ("seed_rows", "dirty_rows", "row_list", "hub_list")} }')
    assert_marks(ssa, dev, n, new_ei, info, dirty, h)
    for k, want in (hubs_at or {}).items():
        assert (info['hub_list'][k] > 0) == want, f'hop {k} lists {info["hub_list"][k]} hub rows'
    for k in range(1, h + 1):
        assert torch.equal(t_up[k].mh_u32, t_ref[k].mh_u32), f'MinHash hop {k}'
        assert torch.equal(t_up[k].hll_u8, t_ref[k].hll_u8), f'HLL hop {k}'
        clean = torch.from_numpy(~dirty[k]).to(dev)
        assert torch.equal(c_up[clean, k - 1].view(torch.int32), snap_c[clean, k - 1].view(torch.int32)), f'cards outside dirty_{k} moved'
        d = torch.from_numpy(dirty[k]).to(dev)
        differ = int((c_up[d, k - 1].view(torch.int32) != c_ref[d, k - 1].view(torch.int32)).sum())
        print(f'  hop {k}: |dirty| = {int(dirty[k].sum())}, dirty cards not bit-identical to the rebuild: {differ}')
    _assert_cards_bar(c_up, c_ref)
    eh.check_errors()
    return eh, t_up, c_up, t_ref, c_ref, dirty


# ---- the inputs (their |dirty_h| < N is asserted by expected_dirty before the GPU is touched) ----------------------------------------------
def ba40_case(kind):
    g = load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    deg = np.bincount(ei[1], minlength=n)
    if kind == 'add':  # an edge between the two nodes of smallest degree that are not yet adjacent
        order = np.argsort(deg, kind='stable')
        have = set(map(tuple, ei.T.tolist()))
        u, v = next((int(a), int(b)) for i, a in enumerate(order) for b in order[i + 1:] if (int(a), int(b)) not in have)
        add = ur.undirected(np.array([[u], [v]]))
        return n, ei, np.concatenate([ei, add], axis=1), add, None
    # remove: the edge whose endpoints have the smallest degree sum (every copy of both directions)
    e = int(np.argmin(deg[ei[0]] + deg[ei[1]]))
    u, v = int(ei[0, e]), int(ei[1, e])
    hit = ((ei[0] == u) & (ei[1] == v)) | ((ei[0] == v) & (ei[1] == u))
    return n, ei, ei[:, ~hit], None, ei[:, hit]


def mixed_change(n, ei, seed, n_remove, n_add, kind='mixed'):
    rng = np.random.RandomState(seed)
    half = ei.shape[1] // 2
    new, added, removed = ei, None, None
    if kind in ('mixed', 'remove'):
        new, removed = ur.remove_edges(ei, rng.choice(half, size=n_remove, replace=False))
    if kind in ('mixed', 'add'):
        new, added = ur.add_edges(new, rng.randint(0, n, size=(2, n_add)))
    return new, added, removed


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('kind', ['add', 'remove'])
def test_ba40_single_edge(ssa, dev, kind, h):
    n, old, new, added, removed = ba40_case(kind)
    check_update(ssa, dev, n, old, new, added, removed, h=h)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_trailing_nodes_edge_raises_max_edge_index(ssa, dev, h):
    """G7: nodes 9 .. 11 of 12 are trailing (no self loop); the added edge (10, 6) gives rows 9 and 10 their loop -- 9 appears in no
    changed edge -- and row 11 stays all-zero"""
    g = load_golden('g7_edge_cases.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    add = np.array([[10], [6]], dtype=np.int64)
    new = np.concatenate([ei, add], axis=1)
    _, t_up, c_up, _, _, dirty = check_update(ssa, dev, n, ei, new, add, None, h=h)
    assert dirty[1][9] and dirty[1][10] and dirty[1][6] and not dirty[1][11]
    assert float(c_up[9, 0]) > 0 and float(c_up[11, 0]) == 0.0 and int(t_up[1].hll_u8[11].sum()) == 0
    # ... and back: the loops of 9 and 10 go away again
    check_update(ssa, dev, n, new, ei, None, add, h=h)


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('num_perm,p', [(128, 8), (64, 6), (256, 10), (8, 4)])
def test_sketch_shapes_and_hop_counts(ssa, dev, num_perm, p, h):
    n = 6000
    ei = ur.uniform_graph(5900, 9000, 41)  # (nodes 5 900 .. 5 999 trail: all-zero rows that must stay untouched)
    new, added, removed = mixed_change(5900, ei, 42, 3, 3)
    check_update(ssa, dev, n, ei, new, added, removed, h=h, num_perm=num_perm, p=p)


@pytest.mark.parametrize('kind', ['add', 'remove', 'mixed'])
def test_additions_removals_mixed(ssa, dev, kind):
    n = 20000
    ei = ur.uniform_graph(n, 60000, 43)
    new, added, removed = mixed_change(n, ei, 44, 40, 40, kind)
    check_update(ssa, dev, n, ei, new, added, removed, h=2)


def test_remove_then_readd_returns_the_original_tables(ssa, dev):
    n, h = 20000, 2
    ei = ur.uniform_graph(n, 60000, 45)
    new, removed = ur.remove_edges(ei, np.random.RandomState(46).choice(ei.shape[1] // 2, size=64, replace=False))
    expected_dirty(n, ei, new, None, removed, h)
    eh = _eh(ssa, h)
    t0, c0 = eh.build_hash_tables(n, _t(ei, dev))
    snap_t, snap_c = _snapshot(t0, c0, h)
    t1, c1 = eh.update_hash_tables(t0, c0, n, _t(new, dev), removed=_t(removed, dev), copy=True)
    assert not torch.equal(t1[2].mh_u32, t0[2].mh_u32)
    t2, c2 = eh.update_hash_tables(t1, c1, n, _t(ei, dev), added=_t(removed, dev))
    assert t2 is t1
    for k in range(1, h + 1):
        assert torch.equal(t2[k].mh_u32, snap_t[k][0]) and torch.equal(t2[k].hll_u8, snap_t[k][1])
        assert torch.equal(t0[k].mh_u32, snap_t[k][0]) and torch.equal(t0[k].hll_u8, snap_t[k][1])  # the originals were never touched
    assert torch.equal(c2.view(torch.int32), snap_c.view(torch.int32)) and torch.equal(c0.view(torch.int32), snap_c.view(torch.int32))


def _hub_graph():
    n = 50000
    return n, ur.power_law_graph(n, 250000, 7)  # node 0 collects ~7 000 in-edges (a mega row), a few dozen nodes more than the hub threshold


@pytest.mark.parametrize('h', [1, 2])
def test_changed_edge_touches_the_largest_hub(ssa, dev, h):
    n, ei = _hub_graph()
    deg = np.bincount(ei[1], minlength=n)
    hub = int(np.argmax(deg))
    assert deg[hub] > 2048
    leaf = int(np.flatnonzero(deg == 0)[0]) if (deg == 0).any() else int(np.argmin(deg))
    new, added = ur.add_edges(ei, np.array([[leaf], [hub]]))
    _, _, _, _, _, dirty = check_update(ssa, dev, n, ei, new, added, None, h=h)
    assert dirty[1][hub]
    if h == 2:
        assert dirty[2].sum() > deg[hub] // 2  # the hub dirties its whole neighbourhood, other hub rows among it
        assert (dirty[2] & (deg > 1024)).sum() >= 1


def test_hubs_that_are_not_dirty_are_not_recomputed(ssa, dev):
    n, ei = _hub_graph()
    h = 2
    deg = np.bincount(ei[1], minlength=n)
    hubs = np.flatnonzero(deg > 128)  # every row at or above the smallest threshold the engine can choose
    assert hubs.size > 10
    # an edge between two low-degree nodes no hub is within two hops of
    A_rows = [set() for _ in range(n)]
    for s, d in ei.T.tolist():
        A_rows[d].add(s)
    near = set(hubs.tolist())
    for x in hubs.tolist():
        near |= A_rows[x]
    far = [x for x in range(n) if x not in near and 0 < deg[x] < 4 and not (A_rows[x] & near)]
    assert len(far) >= 2
    u, v = far[0], far[1]
    new, added = ur.add_edges(ei, np.array([[u], [v]]))
    dirty = expected_dirty(n, ei, new, added, None, h)
    assert not dirty[h][hubs].any()
    eh = _eh(ssa, h)
    t, c = eh.build_hash_tables(n, _t(ei, dev))
    snap_t, snap_c = _snapshot(t, c, h)
    idx = torch.from_numpy(hubs).to(dev)
    _, _, info = eh.update_hash_tables(t, c, n, _t(new, dev), added=_t(added, dev), return_info=True)
    assert info['hub_list'] == {1: 0, 2: 0} and info['dirty_rows'] == {k: int(dirty[k].sum()) for k in (1, 2)}
    for k in (1, 2):
        assert torch.equal(t[k].mh_u32[idx], snap_t[k][0][idx]) and torch.equal(t[k].hll_u8[idx], snap_t[k][1][idx])
    t_ref, c_ref = eh.build_hash_tables(n, _t(new, dev))
    for k in (1, 2):
        assert torch.equal(t[k].mh_u32, t_ref[k].mh_u32) and torch.equal(t[k].hll_u8, t_ref[k].hll_u8)
    _assert_cards_bar(c, c_ref)


@pytest.mark.parametrize('changed', [2048, 60000])
def test_collab_size(ssa, dev, changed):
    n, h = COLLAB_N, 2
    ei = ur.uniform_graph(n, COLLAB_E_UND, 51)
    new, added, removed = mixed_change(n, ei, 52, changed // 2, changed // 2)
    eh, t_up, c_up, t_ref, c_ref, dirty = check_update(ssa, dev, n, ei, new, added, removed, h=h)
    if changed == 2048:
        assert dirty[2].sum() < 0.3 * n
        # the query on the updated tables equals the query on the rebuilt ones within the same bar
        links = _t(np.random.RandomState(53).randint(0, n, size=(50000, 2)).astype(np.int64), dev)
        f_up = eh.get_subgraph_features(links, t_up, c_up)
        f_ref = eh.get_subgraph_features(links, t_ref, c_ref)
        _assert_cards_bar(f_up, f_ref)


def test_materialised_leaves_read_the_new_values(ssa, dev):
    n, h = 20000, 2
    ei = ur.uniform_graph(n, 60000, 47)
    new, added, removed = mixed_change(n, ei, 48, 20, 20)
    expected_dirty(n, ei, new, added, removed, h)
    eh = _eh(ssa, h)
    t, c = eh.build_hash_tables(n, _t(ei, dev))
    leaf_mh, leaf_hll = t[2]['minhash'], t[2]['hll']  # materialised BEFORE the update
    assert leaf_mh.dtype == torch.int64 and leaf_hll.dtype == torch.int8
    eh.update_hash_tables(t, c, n, _t(new, dev), added=_t(added, dev), removed=_t(removed, dev))
    t_ref, _ = eh.build_hash_tables(n, _t(new, dev))
    assert t[2]['minhash'] is leaf_mh and torch.equal(leaf_mh, t_ref[2]['minhash'])
    assert torch.equal(t[2]['hll'], t_ref[2]['hll']) and torch.equal(leaf_hll, t_ref[2]['hll'])
    # the refreshed leaf does not read as "edited by the caller": the packed table stays the one the kernels wrote
    packed = t[2].mh_u32
    assert t[2].packed(dev)[0] is packed


def test_out_of_range_targets_are_reported(ssa, dev):
    n, h = 2000, 2
    ei = ur.uniform_graph(n, 6000, 49)
    eh = _eh(ssa, h)
    eh.strict_bounds = True
    t, c = eh.build_hash_tables(n, _t(ei, dev))
    with pytest.raises(IndexError):
        eh.update_hash_tables(t, c, n, _t(ei, dev), added=_t(np.array([[1], [n + 5]], dtype=np.int64), dev))
    eh.strict_bounds = 'deferred'
    eh.update_hash_tables(t, c, n, _t(ei, dev), added=_t(np.array([[1], [n + 5]], dtype=np.int64), dev))
    with pytest.raises(IndexError):
        eh.check_errors()


# ---- hub rows at every sketch shape, and many of them ----------------------------------------------------------------------------------
def _leaf_to_hub_case():
    n = 20000
    ei = ur.power_law_graph(n, 100000, 65)
    deg = np.bincount(ei[1], minlength=n)
    hub, leaf = int(np.argmax(deg)), int(np.flatnonzero(deg == 0)[0])
    assert deg[hub] > 2048 and (deg > 40).sum() > 100  # a row only the whole workgroup (or, unlisted, one wavefront) walks
    new, added = ur.add_edges(ei, np.array([[leaf], [hub]]))
    return n, ei, new, added


@pytest.mark.parametrize('threshold', [40, 10 ** 9])
@pytest.mark.parametrize('num_perm,p,h', [(128, 8, 2), (64, 6, 2), (192, 8, 2), (256, 10, 2), (8, 4, 2), (128, 8, 3), (8, 4, 3)])
def test_hub_kernels_at_every_shape(ssa, dev, monkeypatch, num_perm, p, h, threshold):
    """update_hub_first_kernel<PPL> at PPL 1 .. 4 and update_hub_table_kernel at M = 16 / 64 / 256 / 1 024 and P = 8 (threshold 40: the
    changed hub and the hubs among its neighbours are listed at every hop); with everything regular (threshold 10^9) one wavefront of
    the row kernels walks the 3 700-edge row"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    n, ei, new, added = _leaf_to_hub_case()
    check_update(ssa, dev, n, ei, new, added, None, h=h, num_perm=num_perm, p=p, hubs_at={k: threshold == 40 for k in range(1, h + 1)})


@pytest.mark.parametrize('num_perm,p', [(128, 8), (8, 4)])
def test_more_listed_hubs_than_hub_workgroups(ssa, dev, monkeypatch, num_perm, p):
    """threshold 8 on a graph of mean degree 20: nearly every dirty row is a hub row, more than the 256 workgroups of a hub launch --
    the `q += gridDim.x` stride of update_hub_first_kernel (128, 8) and of update_hub_table_kernel (hop 2; at (8, 4) hop 1 as well)"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', 8)
    n = 20000
    ei = ur.uniform_graph(n, 200000, 61)
    new, added = ur.add_edges(ei, np.random.RandomState(62).randint(0, n, size=(2, 150)))
    _, _, _, _, _, dirty = check_update(ssa, dev, n, ei, new, added, None, h=2, num_perm=num_perm, p=p, hubs_at={1: True, 2: True})
    deg = np.bincount(new[1], minlength=n)
    assert (dirty[1] & (deg > 8)).sum() > 256 and (dirty[2] & (deg > 8)).sum() > 2048


@pytest.mark.parametrize('num_perm,p', [(128, 8), (8, 4)])
def test_fewer_nodes_than_hub_workgroups(ssa, dev, monkeypatch, num_perm, p):
    """N = 100: hub_grid = N, one 256-row block, every launch smaller than its cap"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', 8)
    n = 100
    ei = ur.uniform_graph(n, 1500, 63)
    new, added = ur.add_directed(ei, np.array([[5], [17]]))
    check_update(ssa, dev, n, ei, new, added, None, h=2, num_perm=num_perm, p=p, hubs_at={1: True, 2: True})


# ---- directed and multigraph changes ---------------------------------------------------------------------------------------------------
def _directed_graph():
    n = 6000
    return n, ur.directed_graph(n, 18000, 64)


def directed_change(n, ei, kind):
    """3 directed additions (at least one of their sources is no target of any change), 4 directed removals, or both"""
    rng = np.random.RandomState(70)
    new, added, removed = ei, None, None
    if kind in ('remove', 'mixed'):
        new, removed = ur.remove_directed(ei, rng.choice(ei.shape[1], size=4, replace=False))
    if kind in ('add', 'mixed'):
        new, added = ur.add_directed(new, rng.randint(0, n, size=(2, 3)))
    return new, added, removed


@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('kind', ['add', 'remove', 'mixed'])
def test_directed_changes_on_a_directed_graph(ssa, dev, kind, h):
    """only edge[1] of a changed edge is a seed, and dirt travels along the edges' direction (CSR by destination): on undirected lists
    both endpoints are targets, and a marker that read the wrong row of `added`, or pushed along out-edges, would pass"""
    n, ei = _directed_graph()
    new, added, removed = directed_change(n, ei, kind)
    changes = np.concatenate([c for c in (added, removed) if c is not None], axis=1)
    sources_only = np.setdiff1d(changes[0], changes[1])
    assert sources_only.size >= 1 and ur.n_self_of(ei) == ur.n_self_of(new)
    _, _, _, _, _, dirty = check_update(ssa, dev, n, ei, new, added, removed, h=h)
    # (check_update compared the engine's hop-1 map with this one exactly)
    assert not dirty[1][sources_only].any() and dirty[1].sum() == np.unique(changes[1]).size


def _old_tables(ssa, dev, n, ei, h):
    t, _ = _eh(ssa, h).build_hash_tables(n, _t(ei, dev))
    return t


@pytest.mark.parametrize('form', ['copy-added', 'copy-removed', 'self-loop', 'empty-added', 'int32-added'])
def test_multigraph_changes_and_input_forms(ssa, dev, form):
    n, ei = _directed_graph()
    h = 2
    edge = ei[:, 100:101]
    assert edge[0, 0] != edge[1, 0]
    if form == 'copy-added':      # a second copy of an existing edge: no table changes, the target is dirty all the same
        new, added = ur.add_directed(ei, edge)
        _, t_up, _, _, _, dirty = check_update(ssa, dev, n, ei, new, added, None, h=h)
        assert dirty[1].sum() == 1 and dirty[1][edge[1, 0]]
        t_old = _old_tables(ssa, dev, n, ei, h)
        for k in range(1, h + 1):
            assert torch.equal(t_up[k].mh_u32, t_old[k].mh_u32) and torch.equal(t_up[k].hll_u8, t_old[k].hll_u8)
    elif form == 'copy-removed':  # one of two copies goes
        old, removed = ur.add_directed(ei, edge)
        check_update(ssa, dev, n, old, ei, None, removed, h=h)
    elif form == 'self-loop':     # an explicit (u, u) beside the implicit one
        u = int(edge[0, 0])
        new, added = ur.add_directed(ei, np.array([[u], [u]]))
        _, _, _, _, _, dirty = check_update(ssa, dev, n, ei, new, added, None, h=h)
        assert np.flatnonzero(dirty[1]).tolist() == [u]
    elif form == 'empty-added':   # `added` of shape [2, 0] beside a non-empty `removed`
        new, removed = ur.remove_directed(ei, np.array([7, 4000]))
        check_update(ssa, dev, n, ei, new, np.zeros((2, 0), dtype=np.int64), removed, h=h)
    else:                         # int32 ids
        new, added = ur.add_directed(ei, np.array([[11, 5000], [4999, 12]]))
        check_update(ssa, dev, n, ei, new, added.astype(np.int32), None, h=h)


# ---- the update writes exactly its rows ------------------------------------------------------------------------------------------------
SENTINEL_BYTE, SENTINEL_CARD = 0xA5, -7.0


@pytest.fixture(scope='module')
def uniform_20k():
    n = 20000
    ei = ur.uniform_graph(n, 200000, 61)
    assert ur.n_self_of(ei) == n
    return n, ei


@pytest.mark.parametrize('num_perm,p', [(128, 8), (8, 4)])
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_update_writes_exactly_its_rows(ssa, dev, uniform_20k, k, h, num_perm, p):
    """k directed additions with distinct non-hub targets: the hop-1 row list is k long -- around the 4 rows a workgroup of the
    wave-per-row kernels takes and the 16 of the 16-lane ones, whose `q >= n` groups must store nothing.  Before the update every row
    of the LAST hop's packed tables and cards column outside dirty_h is filled with a sentinel (bytes 0xA5, card -7.0): a clean row
    that is recomputed gets its own bits back, so only a sentinel shows a stray store.  Only the last hop can be poisoned -- later
    hops read the earlier ones -- and at h = 1 its cards column is also the marker's self-loop memory (cards_old > 0), so there the
    sentinel card is +7.0: every row keeps saying "had its loop", and must still hold +7.0 bit for bit.
    The packed tensors are edited directly: a HopSketch watches its materialised leaves for caller edits, not its packed twins, and
    no leaf is materialised here."""
    n, ei = uniform_20k
    rng = np.random.RandomState(1000 * h + k)
    targets = rng.choice(n, size=k, replace=False)
    new, added = ur.add_directed(ei, np.stack([rng.randint(0, n, size=k), targets]))
    deg = np.bincount(new[1], minlength=n)
    assert (deg[targets] <= hub_threshold_of(ssa, new)).all()
    dirty = expected_dirty(n, ei, new, added, None, h)
    assert dirty[1].sum() == k
    eh = _eh(ssa, h, num_perm, p)
    t, c = eh.build_hash_tables(n, _t(ei, dev))
    t_ref, c_ref = eh.build_hash_tables(n, _t(new, dev))
    clean = torch.from_numpy(~dirty[h]).to(dev)
    d = ~clean
    card = torch.tensor([SENTINEL_CARD if h > 1 else -SENTINEL_CARD], dtype=torch.float32, device=dev)
    t[h].mh_u32.view(torch.uint8)[clean] = SENTINEL_BYTE
    t[h].hll_u8[clean] = SENTINEL_BYTE
    c[clean, h - 1] = card[0]
    t_up, c_up, info = eh.update_hash_tables(t, c, n, _t(new, dev), added=_t(added, dev), return_info='masks')
    assert t_up is t and c_up is c
    assert_marks(ssa, dev, n, new, info, dirty, h)
    assert info['row_list'][1] == k and info['hub_list'][1] == 0
    for j in range(1, h):  # the hops below the last one: equal to the rebuild everywhere
        assert torch.equal(t[j].mh_u32, t_ref[j].mh_u32) and torch.equal(t[j].hll_u8, t_ref[j].hll_u8), f'hop {j}'
    _assert_cards_bar(c[:, :h - 1], c_ref[:, :h - 1])
    mh, hll = t[h].mh_u32.view(torch.uint8), t[h].hll_u8
    stray_mh = (mh[clean] != SENTINEL_BYTE).any(dim=1)
    stray_hll = (hll[clean] != SENTINEL_BYTE).any(dim=1)
    stray_card = c[clean, h - 1].view(torch.int32) != card.view(torch.int32)
    rows = torch.nonzero(clean).flatten()
    assert not bool(stray_mh.any()), f'MinHash rows outside dirty_{h} were written: {rows[stray_mh][:8].tolist()}'
    assert not bool(stray_hll.any()), f'HLL rows outside dirty_{h} were written: {rows[stray_hll][:8].tolist()}'
    assert not bool(stray_card.any()), f'cards outside dirty_{h} were written: {rows[stray_card][:8].tolist()}'
    assert torch.equal(t[h].mh_u32[d], t_ref[h].mh_u32[d]) and torch.equal(hll[d], t_ref[h].hll_u8[d]), f'rows of dirty_{h}'
    _assert_cards_bar(c[d, h - 1], c_ref[d, h - 1])
    eh.check_errors()


# ---- a chain of in-place updates -------------------------------------------------------------------------------------------------------
def test_chain_of_in_place_updates(ssa, dev):
    """eight successive in-place updates of one table set, directed additions and removals in turn, one of which moves
    max(edge_index) up and a later one down again: after each step the tables are the rebuild's, and the marker's maps are the
    restatement's with "had its self loop" read from the PREVIOUS graph -- the cards column of the updated tables is the loop memory of
    the next update"""
    n, h = 6000, 2
    ei = ur.directed_graph(5900, 18000, 71)
    top = ur.n_self_of(ei)
    assert top <= 5900
    rng = np.random.RandomState(72)
    up_edge = np.array([[5950], [7]])
    eh = _eh(ssa, h)
    t, c = eh.build_hash_tables(n, _t(ei, dev))
    for step in range(8):
        added = removed = None
        if step == 2:    # rows top .. 5 950 gain their implicit self loop
            new, added = ur.add_directed(ei, up_edge)
        elif step == 5:  # ... and lose it again
            pos = np.flatnonzero((ei[0] == 5950) & (ei[1] == 7))
            assert pos.size == 1
            new, removed = ur.remove_directed(ei, pos)
        elif step % 2 == 0:
            new, added = ur.add_directed(ei, rng.randint(0, 5900, size=(2, 3)))
        else:
            candidates = np.flatnonzero(ei[0] != 5950)
            new, removed = ur.remove_directed(ei, rng.choice(candidates, size=3, replace=False))
        dirty = expected_dirty(n, ei, new, added, removed, h)
        if step in (2, 5):
            assert ur.n_self_of(new) != ur.n_self_of(ei) and dirty[1][top:5951].all() and not dirty[1][5951:].any()
        t2, c2, info = eh.update_hash_tables(t, c, n, _t(new, dev), added=_t(added, dev), removed=_t(removed, dev), return_info='masks')
        assert t2 is t and c2 is c
        assert_marks(ssa, dev, n, new, info, dirty, h)
        t_ref, c_ref = eh.build_hash_tables(n, _t(new, dev))
        for k in range(1, h + 1):
            assert torch.equal(t[k].mh_u32, t_ref[k].mh_u32) and torch.equal(t[k].hll_u8, t_ref[k].hll_u8), f'step {step}, hop {k}'
        _assert_cards_bar(c, c_ref)
        assert torch.equal(c[:, 0] > 0, torch.from_numpy(np.arange(n) < ur.n_self_of(new)).to(dev)), f'step {step}: the loop memory'
        ei = new
    eh.check_errors()
