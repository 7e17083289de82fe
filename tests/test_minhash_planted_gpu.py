"""The two-phase MinHash first hop (csrc/ss_walks.hpp first_hop_minhash_fast, MinhashRows::row) on the planted permutation parameters
of tests/minhash_planted.py: (a_q, b_q) solved so that chosen entries of chosen rows sit exactly where the walk's rules decide -- two
keys in one bucket, in adjacent buckets with the value order reversed, two buckets apart (the fast path, just outside the rule), a
wrapped low word, bucket 0, the all-ones middle word with r = M - 1, M, M + 1, M + 7 (the `r >= M` branch of mod_mersenne61), one-entry
rows against the 0xFFFFFFFF start of the second-smallest key, identical keys in two batches of one wavefront, a winner carried from an
earlier batch -- through every kernel that reaches the walk: ss_first_hop (8 rows per wavefront), the fused stage and its records
form (4 rows per wavefront), the hub units (16 wavefronts per row), update_hash_tables (plain batches of 64), the engine's
build_hash_tables, the masked query, and the hop-0 kernels on planted node hashes.

Every comparison is exact equality of whole MinHash rows with minhash_planted.want_row / want_tables (Python integers); hop-2 rows with
the min-fold of the wanted hop-1 rows.  test_minhash_planted_host.py proves on the CPU that the discriminating cases make the shortcut
wrong when a rule is missing."""
import functools
from argparse import Namespace
from ctypes import byref

import numpy as np
import pytest
import torch

import minhash_planted as mp

pytestmark = pytest.mark.gpu

M = 256
SHORT_P = (64, 128, 192, 256)


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in ('SS_FUSED_STAGE', 'SS_FUSED_POSTS', 'SS_SELF_SKIP', 'SS_HUB_HINTS'):
        monkeypatch.delenv(name, raising=False)


def _param_set(name, P):
    s = mp.short_params() if name == 'short' else mp.long_params(name)
    return s.a[:P], s.b[:P]


@functools.lru_cache(maxsize=None)
def _want(name, P, edges='new'):
    """(hop-1, hop-2) uint32 [n, P] in Python integers, once per parameter set and graph"""
    g = mp.graph()
    ei = g.edge_index if edges == 'new' else _edit(name)[0]
    a, b = _param_set(name, P)
    return mp.want_tables(g.n, ei, a, b)


def _ab(name, P, dev):
    a, b = _param_set(name, P)
    return torch.from_numpy(np.stack([mp.as_u64(a), mp.as_u64(b)]).view(np.int64)).to(dev)


def _eh(ssa, dev, name, P, **kw):
    """a fresh engine whose permutation parameters are the planted ones: on the instance, never on the class or the module"""
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True), **kw)
    a, b = _param_set(name, P)
    eh._init_permutations = lambda num_perm, ab=np.stack([mp.as_u64(a), mp.as_u64(b)]): ab[:, :num_perm].copy()
    assert not eh._dev_perms
    got = eh._perms(dev).cpu().numpy().view(np.uint64)
    assert got[0].tolist() == list(a) and got[1].tolist() == list(b)
    return eh


def _edge_order(csr, ei):
    """The CSR build leaves the order of a row's sources unspecified; the planted slots (equal slots in two batches, the batch of A and
    of B) need the order of edge_index.  After checking that the build lists every row's sources, rewrite them in that order: the
    walks under test read `col`, they do not care who sorted it."""
    ei = np.asarray(ei)
    n, E = csr.num_nodes, ei.shape[1]
    rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()[:E]
    assert np.array_equal(np.diff(rowptr), np.bincount(ei[1], minlength=n))
    want = ei[0][np.argsort(ei[1], kind='stable')].astype(np.int32)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) << 32
    assert np.array_equal(np.sort(rows + col), np.sort(rows + want)), 'the CSR build lists other sources than edge_index'
    csr.col[:E].copy_(torch.from_numpy(want).to(csr.col.device))
    return csr


def _csr(ssa, dev, ei, hub_threshold=None):
    """the strict build (it reads the hub counters back, so the plan can be asserted; hub_threshold None: knobs.HUB_THRESHOLD) with
    every row in edge order"""
    g = mp.graph()
    csr = ssa.hashing.build_csr(torch.from_numpy(ei).to(dev), g.n, dev, check=True, hub_threshold=hub_threshold)
    csr.use_inferred_self_loops = True
    return _edge_order(csr, ei)


def _edge_ordered_builds(ssa, monkeypatch):
    """build_hash_tables and update_hash_tables build their CSR themselves: the same rewrite behind their build_csr"""
    import importlib
    real = ssa.hashing.build_csr

    def build_csr(edge_index, num_nodes, device, **kw):
        return _edge_order(real(edge_index, num_nodes, device, **kw), edge_index.cpu().numpy())

    for name in ('engine', 'update'):
        monkeypatch.setattr(importlib.import_module(f'{ssa.__name__}.{name}'), 'build_csr', build_csr)


def _hub_plan(csr):
    """(rows handed to the hub units, rows handed to the mega slices)"""
    hubs = csr.hub_rows[:int(csr.hub_count[0])].cpu().tolist()
    mega = csr.mega_rows[:int(csr.mega_count[0]), 0].cpu().tolist()
    return set(hubs), set(mega)


def _assert_rows(got, want, what):
    got = got.cpu().numpy().view(np.uint32) if isinstance(got, torch.Tensor) else got
    if not np.array_equal(got, want):
        rows, perms = np.nonzero(got != want)
        i, q = int(rows[0]), int(perms[0])
        raise AssertionError(f'{what}: {len(set(rows.tolist()))} rows differ, first row {i} permutation {q}: got {int(got[i, q]):#x}, '
                             f'want {int(want[i, q]):#x}')


def _first_hop(ssa, dev, csr, ab, P):
    from subgraph_sketching_amd._runtime import _ptr, _stream
    n = csr.num_nodes
    mh = torch.full((n, P), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    prm = _plain_engine(ssa, P)._params(dev)
    graph = csr.struct()
    rc = ssa._native.lib().ss_first_hop(byref(graph), _ptr(ab[0]), _ptr(ab[1]), P, _ptr(mh), 8, None, None, 2, byref(prm.struct), _stream(dev))
    assert rc == 0, f'ss_first_hop returned {rc}'
    return mh


def _plain_engine(ssa, P):
    return ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True))


def _fused(ssa, dev, csr, ab, P, records):
    """ss_fused_hop_stage, or ss_fused_hop_stage_records with its workspace -> (hop-1 MinHash, hop-2 MinHash or None)"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    n = csr.num_nodes
    mh = [torch.full((n, P), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(2)]
    hll = [torch.full((n, M), 255, dtype=torch.uint8, device=dev) for _ in range(2)]
    cards = torch.full((n, 2), -1.0, dtype=torch.float32, device=dev)
    prm = _plain_engine(ssa, P)._params(dev)
    graph = csr.struct()
    lib = ssa._native.lib()
    mh2 = _ptr(mh[1]) if P == 128 else None
    if records:
        rec = torch.empty((n, 16), dtype=torch.int32, device=dev)
        rc = lib.ss_fused_hop_stage_records(byref(graph), _ptr(ab[0]), _ptr(ab[1]), P, _ptr(mh[0]), mh2, 8, _ptr(hll[0]), _ptr(cards),
                                            _ptr(hll[1]), _ptr(cards[:, 1]), 2, byref(prm.struct), _ptr(rec), int(csr.num_edges), _stream(dev))
    else:
        rc = lib.ss_fused_hop_stage(byref(graph), _ptr(ab[0]), _ptr(ab[1]), P, _ptr(mh[0]), mh2, 8, _ptr(hll[0]), _ptr(cards), _ptr(hll[1]),
                                    _ptr(cards[:, 1]), 2, byref(prm.struct), _stream(dev))
    assert rc == 0, f'the fused stage returned {rc}'
    return mh[0], (mh[1] if P == 128 else None)


def _mh(table, k):
    return table[k].mh_u32


# ---- the graph as the kernels see it ---------------------------------------------------------------------------------------------------
def test_csr_holds_the_planted_rows_in_edge_order(ssa, dev, monkeypatch):
    """the slots of the restatement: every row's sources as minhash_planted.graph lists them, every node with its self loop"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', 200)
    g = mp.graph()
    csr = _csr(ssa, dev, g.edge_index)
    rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()
    assert int(csr.n_self_dev[0]) == g.n
    for i in range(g.n):
        assert col[rowptr[i]:rowptr[i + 1]].tolist() == g.col.get(i, []), i


# ---- short rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threshold', [8, None])
@pytest.mark.parametrize('P', SHORT_P)
def test_short_rows_through_the_first_hop_and_the_fused_stage(ssa, dev, monkeypatch, P, threshold):
    """every scenario S1 .. S10 on a row of its own: ss_first_hop (R = 8), ss_fused_hop_stage (R = 4) and, at P = 128, its records form"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    g = mp.graph()
    csr = _csr(ssa, dev, g.edge_index)
    hubs, mega = _hub_plan(csr)
    deg = np.bincount(g.edge_index[1], minlength=g.n)
    limit = 8 if threshold == 8 else ssa.hashing.default_hub_threshold(g.edge_index.shape[1])
    assert csr.hub_threshold == limit and hubs | mega == set(np.flatnonzero(deg > limit).tolist()) and csr.has_hub_rows
    assert set(g.long.values()) >= hubs | mega and (threshold != 8 or hubs | mega == set(g.long.values()))
    assert not any(s in hubs | mega for _, s, _ in g.short), 'the two-entry and the one-entry rows stay regular'
    ab = _ab('short', P, dev)
    want1, want2 = _want('short', P)
    _assert_rows(_first_hop(ssa, dev, csr, ab, P), want1, f'ss_first_hop P={P} threshold={threshold}')
    # (the stage takes its records form only for a graph that lists no hub rows: a third CSR, every row regular)
    for records in ((False, True) if P == 128 else (False,)):
        if records:
            csr = _csr(ssa, dev, g.edge_index, hub_threshold=10 ** 9)
            assert not csr.has_hub_rows
        mh1, mh2 = _fused(ssa, dev, csr, ab, P, records)
        _assert_rows(mh1, want1, f'fused stage P={P} threshold={threshold} records={records}: hop 1')
        if mh2 is not None:
            _assert_rows(mh2, want2, f'fused stage P={P} threshold={threshold} records={records}: hop 2')


@pytest.mark.parametrize('threshold', [8, None])
@pytest.mark.parametrize('P', SHORT_P)
def test_short_rows_through_the_engine(ssa, dev, monkeypatch, P, threshold):
    """build_hash_tables with the fused stage on and off, twice each (the second build runs with the hub hint of the first); a second
    engine with OTHER parameters on the same graph gets its own rows, and no build reads a sketch cache from disk"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    _edge_ordered_builds(ssa, monkeypatch)
    monkeypatch.setattr(torch, 'load', lambda *a, **k: pytest.fail('build_hash_tables must not read a cache'))
    g = mp.graph()
    ei = torch.from_numpy(g.edge_index).to(dev)
    want1, want2 = _want('short', P)
    for fuse in (True, False):
        eh = _eh(ssa, dev, 'short', P, fuse_hop_stage=fuse)
        for rep in range(2):
            table, _ = eh.build_hash_tables(g.n, ei)
            _assert_rows(_mh(table, 1), want1, f'engine P={P} threshold={threshold} fuse={fuse} build {rep}: hop 1')
            _assert_rows(_mh(table, 2), want2, f'engine P={P} threshold={threshold} fuse={fuse} build {rep}: hop 2')
    if P == 128:
        other = _eh(ssa, dev, 'adjacent', P)
        table, _ = other.build_hash_tables(g.n, ei)
        _assert_rows(_mh(table, 1), _want('adjacent', P)[0], 'a second engine with other parameters')
        assert not np.array_equal(_want('adjacent', P)[0], want1)


@functools.lru_cache(maxsize=None)
def _edit(name):
    """(old edge_index, added, removed): the planted graph is the graph AFTER the edit.  Short set: every second two-entry row gains its
    one neighbour, the others and the one-entry rows lose an extra neighbour; long sets: every long row gains its first entry"""
    g = mp.graph()
    ei = g.edge_index
    if name == 'short':
        gain = {s for q, (_, s, t) in enumerate(g.short) if t is not None and q % 2 == 0}
        lose = [s for q, (_, s, t) in enumerate(g.short) if not (t is not None and q % 2 == 0)]
        keep = np.array([int(i) not in gain for i in ei[1]])
        removed = np.array([[g.n - 3 - (k % 2) for k in range(len(lose))], lose], dtype=np.int64)
    else:
        first = {row: g.col[row][0] for row in g.long.values()}
        keep = np.array([not (int(i) in first and first[int(i)] == int(u)) for u, i in zip(ei[0], ei[1])])
        removed = np.zeros((2, 0), dtype=np.int64)
    added = ei[:, ~keep]
    old = np.concatenate([ei[:, keep], removed], axis=1)
    assert int(old.max()) == g.n - 1 and added.shape[1] > 0
    return old, added, removed


@pytest.mark.parametrize('threshold', [8, None])
@pytest.mark.parametrize('P', SHORT_P)
def test_short_rows_through_update_hash_tables(ssa, dev, monkeypatch, P, threshold):
    """an edit that dirties every planted row: half of the two-entry rows gain their neighbour, the other rows lose an extra one, and
    the updated tables must be the planted graph's (plain batches of 64 by one wavefront: first_hop_minhash_fast)"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    _edge_ordered_builds(ssa, monkeypatch)
    g = mp.graph()
    old, added, removed = _edit('short')
    eh = _eh(ssa, dev, 'short', P)
    table, cards = eh.build_hash_tables(g.n, torch.from_numpy(old).to(dev))
    before1, _ = _want('short', P, 'old')
    _assert_rows(_mh(table, 1), before1, 'the build on the graph before the edit')
    table, cards, info = eh.update_hash_tables(table, cards, g.n, torch.from_numpy(g.edge_index).to(dev), added=torch.from_numpy(added).to(dev),
                                               removed=torch.from_numpy(removed).to(dev), copy=True, return_info='masks')
    dirty = info['dirty_mask'][1].cpu().numpy()
    assert all(dirty[s] for _, s, _ in g.short) and info['hub_list'][1] == 0
    want1, want2 = _want('short', P)
    changed = np.flatnonzero((before1 != want1).any(axis=1))
    assert len(changed) >= 250, 'the edit changes the planted rows'
    _assert_rows(_mh(table, 1), want1, f'update P={P} threshold={threshold}: hop 1')
    _assert_rows(_mh(table, 2), want2, f'update P={P} threshold={threshold}: hop 2')


# ---- long rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threshold', [200, 10 ** 9])
@pytest.mark.parametrize('rule', mp.RULES)
def test_long_rows_through_every_kernel(ssa, dev, monkeypatch, rule, threshold):
    """rows of 61, 130, 210 and 1 100 entries with A and B planted per permutation: both in one batch, in two batches of one wavefront
    with equal slots, the winner in the first batch and in a later one, A or B the row's own id, a row that lists itself.  Threshold
    200: the rows of 210 and 1 100 entries go to the hub units (16 wavefronts, each judged on its share); 10^9: one wavefront walks all"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    P = 128
    g = mp.graph()
    csr = _csr(ssa, dev, g.edge_index)
    hubs, mega = _hub_plan(csr)
    assert hubs | mega == ({g.long['L210'], g.long['L1100']} if threshold == 200 else set())
    ab = _ab(rule, P, dev)
    want1, want2 = _want(rule, P)
    _assert_rows(_first_hop(ssa, dev, csr, ab, P), want1, f'ss_first_hop {rule} threshold={threshold}')
    for records in (False, True):
        mh1, mh2 = _fused(ssa, dev, csr, ab, P, records)
        _assert_rows(mh1, want1, f'fused stage {rule} threshold={threshold} records={records}: hop 1')
        _assert_rows(mh2, want2, f'fused stage {rule} threshold={threshold} records={records}: hop 2')
    _edge_ordered_builds(ssa, monkeypatch)
    old, added, _ = _edit(rule)
    eh = _eh(ssa, dev, rule, P)
    table, cards = eh.build_hash_tables(g.n, torch.from_numpy(old).to(dev))
    _assert_rows(_mh(table, 1), _want(rule, P, 'old')[0], 'the build on the graph before the edit')
    table, cards, info = eh.update_hash_tables(table, cards, g.n, torch.from_numpy(g.edge_index).to(dev), added=torch.from_numpy(added).to(dev),
                                               copy=True, return_info='masks')
    dirty = info['dirty_mask'][1].cpu().numpy()
    assert all(dirty[row] for row in g.long.values()) and info['hub_list'][1] == (2 if threshold == 200 else 0)
    _assert_rows(_mh(table, 1), want1, f'update {rule} threshold={threshold}: hop 1')
    _assert_rows(_mh(table, 2), want2, f'update {rule} threshold={threshold}: hop 2')


# ---- the masked query ------------------------------------------------------------------------------------------------------------------
def test_masked_query_at_planted_rows(ssa, dev, monkeypatch):
    """links at the rows that hold the - M value (S8, r = M: value 0) in the permutation that plants it.  A link that is no edge of the
    graph is masked by nothing: the masked query must return the plain query's rows bit for bit.  A link that IS the row's one edge is
    recomputed from node ids by the masked kernel's own exact walk (masked_first_hop, permuted_hash): its match counts must be those of
    the plain query on tables built without that edge"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', None)
    P = 128
    g, sp = mp.graph(), mp.short_params()
    s8 = [inf for inf in sp.info[:P] if inf.name == 'S8m']
    assert {inf.planted for inf in s8} == {0, 1}
    ei = torch.from_numpy(g.edge_index).to(dev)
    eh = _eh(ssa, dev, 'short', P)
    table, cards = eh.build_hash_tables(g.n, ei)
    want1, _ = _want('short', P)
    for inf in s8:
        assert want1[inf.row, inf.q] == 0 and int(_mh(table, 1)[inf.row, inf.q]) == 0
    non_edges = torch.tensor([[inf.row, s8[0].neighbour + 1] for inf in s8] + [[s8[0].row, s8[1].row]], dtype=torch.int64, device=dev)
    edges = set(map(tuple, g.edge_index.T.tolist()))
    assert not any((u, v) in edges or (v, u) in edges for u, v in non_edges.tolist())
    plain = eh.get_subgraph_features(non_edges, table, cards)
    got, dbg = eh.get_subgraph_features(non_edges, table, cards, mask_target=ei, return_debug=True)
    assert not bool(dbg['masked'].any()) and torch.equal(got, plain)
    for inf in s8:
        link = torch.tensor([[inf.neighbour, inf.row], [inf.row, inf.neighbour]], dtype=torch.int64, device=dev)
        got, dbg = eh.get_subgraph_features(link, table, cards, mask_target=ei, return_debug=True)
        assert bool(dbg['masked'].all())
        keep = ~((g.edge_index[0] == inf.neighbour) & (g.edge_index[1] == inf.row))
        less = torch.from_numpy(g.edge_index[:, keep]).to(dev)
        eh2 = _eh(ssa, dev, 'short', P)
        table2, cards2 = eh2.build_hash_tables(g.n, less)
        a, b = _param_set('short', P)
        _assert_rows(_mh(table2, 1), mp.want_tables(g.n, g.edge_index[:, keep], a, b, hops=1)[0], 'the build without the link')
        _, pdbg = eh2._pair_kernel(link, table2, cards2, want_debug=True)
        assert torch.equal(dbg['match'], pdbg['match']) and torch.equal(dbg['zeros'], pdbg['zeros'])


# ---- hop 0 on planted hashes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [4, 8, 16])
def test_hll_init_on_planted_hashes(ssa, dev, p):
    from subgraph_sketching_amd._runtime import _ptr, _stream
    lib = ssa._native.lib()
    for name, hv in mp.hll_hashes(p).items():
        pre = mp.inverse_splitmix64(hv)
        out = torch.full((3, 1 << p), 77, dtype=torch.uint8, device=dev)
        assert lib.ss_hll_init(_ptr(out), pre - 1, 3, p, _stream(dev)) == 0
        got = out.cpu().numpy()
        for k in range(3):
            assert got[k].tolist() == mp.hll_row(mp.splitmix64(pre + k), p), (name, k)


@pytest.mark.parametrize('P', [8, 2048])
def test_minhash_init_on_planted_hashes(ssa, dev, P):
    """ss_minhash_init, the generic path's hop 0, on a node whose permuted hashes are r = M - 1, M, M + 1, M + 7, x = 0 and
    x = 2^64 - 1 in turn"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    hv, a, b, names = mp.minhash_init_params(P)
    pre = mp.inverse_splitmix64(hv)
    ab = torch.from_numpy(np.stack([mp.as_u64(a), mp.as_u64(b)]).view(np.int64)).to(dev)
    out = torch.full((2, P), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    assert ssa._native.lib().ss_minhash_init(_ptr(out), pre - 1, 2, _ptr(ab[0]), _ptr(ab[1]), P, _stream(dev)) == 0
    got = out.cpu().numpy().view(np.uint32)
    assert got[0].tolist() == [mp.S8_VALUES[name] for name in names]
    assert got[1].tolist() == [mp.value_of_x(mp.x_of(aq, bq, mp.splitmix64(pre + 1))) for aq, bq in zip(a, b)]
