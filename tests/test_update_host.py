"""ElphHashes.update_hash_tables without a GPU: (1) the rule that says WHICH rows an edge change can reach (tests/update_restatement.py)
is sufficient, checked against the CPU oracle -- not the code under test --: every row of every hop that differs between the oracle's
tables of the old and the new graph lies in the restatement's dirty_k, and cards outside dirty_k are bit-equal; (2) the new C-ABI
symbols are declared and exported; (3) the method exists with its signature and rejects bad arguments before touching a device."""
import ctypes
import inspect
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import update_planted as up
import update_restatement as ur
from conftest import REPO, oracle_params

H, P = 3, 32


@pytest.fixture(scope='module')
def prm(regenerated_tables):
    return oracle_params(regenerated_tables[8])


def _assert_rule_is_sufficient(n, old_ei, new_ei, added, removed, prm):
    from oracle import oracle
    ot, oc = oracle.build_hash_tables(n, old_ei, H, P, prm)
    nt, nc = oracle.build_hash_tables(n, new_ei, H, P, prm)
    dirty = ur.dirty_sets(n, new_ei, oc, added, removed, H)
    changed_total = 0
    for k in range(1, H + 1):
        ch = ur.changed_rows(ot[k]['minhash'], nt[k]['minhash']) | ur.changed_rows(ot[k]['hll'], nt[k]['hll'])
        changed_total += int(ch.sum())
        outside = ch & ~dirty[k]
        assert not outside.any(), f'hop {k}: rows {np.flatnonzero(outside)[:8]} changed outside dirty_{k}'
        clean = ~dirty[k]
        assert np.array_equal(ur.bits(oc[clean, k - 1]), ur.bits(nc[clean, k - 1])), f'hop {k}: cards moved outside dirty_{k}'
    return dirty, changed_total


def _graphs():
    return [('uniform', 3000, ur.uniform_graph(3000, 9000, 11)), ('uniform-sparse', 2000, ur.uniform_graph(2000, 2500, 12)),
            ('power-law', 3000, ur.power_law_graph(3000, 9000, 13)), ('power-law-steep', 2500, ur.power_law_graph(2500, 6000, 14, exponent=5.0)),
            # directed lists (the engine is specified on them: CSR by destination, only edge[1] of a change is a seed)
            ('directed', 3000, ur.directed_graph(3000, 9000, 64)), ('directed-sparse', 2000, ur.directed_graph(2000, 3000, 15))]


def _changers(directed):
    """(remove(ei, positions), add(ei, edges), number of removable positions of ei)"""
    if directed:
        return ur.remove_directed, ur.add_directed, lambda ei: ei.shape[1]
    return ur.remove_edges, ur.add_edges, lambda ei: ei.shape[1] // 2


@pytest.mark.parametrize('name,n,ei', _graphs(), ids=[g[0] for g in _graphs()])
def test_rule_covers_additions_removals_and_both(name, n, ei, prm):
    rng = np.random.RandomState(len(name))
    remove, add, positions = _changers(name.startswith('directed'))
    half = positions(ei)
    new_add, added = add(ei, rng.randint(0, n, size=(2, 5)))
    _, changed = _assert_rule_is_sufficient(n, ei, new_add, added, None, prm)
    assert changed > 0
    new_rem, removed = remove(ei, rng.choice(half, size=5, replace=False))
    _assert_rule_is_sufficient(n, ei, new_rem, None, removed, prm)
    mid, removed = remove(ei, rng.choice(half, size=4, replace=False))
    new_both, added = add(mid, rng.randint(0, n, size=(2, 4)))
    dirty, _ = _assert_rule_is_sufficient(n, ei, new_both, added, removed, prm)
    assert dirty[1].sum() <= 16 and dirty[1].sum() < dirty[2].sum() <= dirty[3].sum()


def test_rule_when_max_edge_index_moves(prm):
    """trailing nodes: with an old max id of 2 499, an added edge (2 519, 3) gives rows 2 500 .. 2 519 a self loop although only 3 and
    2 519 appear in `added`; removing it again takes the loops away"""
    n = 2600
    ei = ur.uniform_graph(2500, 7000, 21)
    assert ur.n_self_of(ei) <= 2500
    top = ur.n_self_of(ei)
    up, added = ur.add_edges(ei, np.array([[2519], [3]]))
    dirty, _ = _assert_rule_is_sufficient(n, ei, up, added, None, prm)
    assert dirty[1][top:2520].all() and not dirty[1][2520:].any() and dirty[1].sum() == 2520 - top + 1
    # ... and down again (the new graph is the old one: the rows 2 500 .. 2 519 lose their loop, 2 519 empties)
    down, removed = up[:, :ei.shape[1]], added
    dirty, _ = _assert_rule_is_sufficient(n, up, down, None, removed, prm)
    assert dirty[1][top:2520].all() and dirty[1].sum() == 2520 - top + 1


def test_rule_on_emptied_rows_duplicates_and_empty_graphs(prm):
    n = 1500
    ei = ur.uniform_graph(n, 4000, 31)
    half = ei.shape[1] // 2
    # every edge of one node goes: its row keeps nothing but the self loop
    node = int(ei[1, 0])
    pos = np.flatnonzero((ei[0, :half] == node) | (ei[1, :half] == node))
    new, removed = ur.remove_edges(ei, pos)
    _assert_rule_is_sufficient(n, ei, new, None, removed, prm)
    # duplicate edges: adding a copy of an existing edge changes nothing; removing one of two copies neither
    dup, added = ur.add_edges(ei, ei[:, :3])
    _, changed = _assert_rule_is_sufficient(n, ei, dup, added, None, prm)
    assert changed == 0
    _assert_rule_is_sufficient(n, dup, ei, None, added, prm)
    # E == 0 after (everything removed) and before (everything added)
    small = ur.uniform_graph(200, 300, 32)
    empty = np.zeros((2, 0), dtype=np.int64)
    _assert_rule_is_sufficient(220, small, empty, None, small, prm)
    dirty, _ = _assert_rule_is_sufficient(220, empty, small, small, None, prm)
    assert dirty[1][:ur.n_self_of(small)].all() and not dirty[1][ur.n_self_of(small):].any()


@pytest.mark.parametrize('seed', range(6))
def test_rule_on_random_mixed_changes(seed, prm):
    rng = np.random.RandomState(100 + seed)
    n = int(rng.randint(40, 400))
    used = int(rng.randint(n // 2, n + 1))
    ei = ur.uniform_graph(used, int(rng.randint(used, 3 * used)), 200 + seed) if seed % 2 else ur.power_law_graph(used, 2 * used, 200 + seed)
    half = ei.shape[1] // 2
    mid, removed = ur.remove_edges(ei, rng.choice(half, size=min(6, half), replace=False))
    new, added = ur.add_edges(mid, rng.randint(0, n, size=(2, 5)))
    _assert_rule_is_sufficient(n, ei, new, added, removed, prm)


@pytest.mark.parametrize('seed', range(6))
def test_rule_on_random_mixed_directed_changes(seed, prm):
    """the same on directed graphs with directed change lists: only the TARGET of a changed edge is a seed, and dirt travels along
    the edges' direction only"""
    rng = np.random.RandomState(300 + seed)
    n = int(rng.randint(40, 400))
    used = int(rng.randint(n // 2, n + 1))
    ei = ur.directed_graph(used, int(rng.randint(used, 4 * used)), 400 + seed)
    mid, removed = ur.remove_directed(ei, rng.choice(ei.shape[1], size=6, replace=False))
    new, added = ur.add_directed(mid, rng.randint(0, n, size=(2, 5)))
    dirty, _ = _assert_rule_is_sufficient(n, ei, new, added, removed, prm)
    loops_moved = ur.n_self_of(ei) != ur.n_self_of(new)
    sources_only = np.setdiff1d(np.concatenate([added[0], removed[0]]), np.concatenate([added[1], removed[1]]))
    if not loops_moved:
        assert not dirty[1][sources_only].any()  # a source that is no target is no seed


def test_rule_on_the_checked_directed_case(prm):
    """RandomState(64).randint(0, 3000, (2, 9000)), 4 directed additions, then 4 directed removals, h = 3"""
    n = 3000
    ei = ur.directed_graph(n, 9000, 64)
    rng = np.random.RandomState(65)
    new, added = ur.add_directed(ei, rng.randint(0, n, size=(2, 4)))
    dirty, _ = _assert_rule_is_sufficient(n, ei, new, added, None, prm)
    assert dirty[1].sum() == np.unique(added[1]).size <= 4 and dirty[1].sum() < dirty[2].sum() < dirty[3].sum() < n
    back, removed = ur.remove_directed(new, rng.choice(new.shape[1], size=4, replace=False))
    dirty, _ = _assert_rule_is_sufficient(n, new, back, None, removed, prm)
    assert dirty[1].sum() == np.unique(removed[1]).size <= 4 and dirty[3].sum() < n


# ---- the planted graph of tests/test_update_planted_gpu.py -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planted():
    return up.plan()


def test_planted_graph_has_every_tier_and_step_boundary(planted):
    pl = planted
    assert pl['n'] == pl['n_self'] + up.TRAILING and pl['edge_index'].shape[1] == sum(up.DEGREES) == 40356
    assert pl['edge_index'][0].max() < up.D <= pl['edge_index'][1].min()  # sources have no in-edge, rows no out-edge
    tiers = [up.tier(d) for d in up.DEGREES]
    assert tiers.count('solo') == 5 and tiers.count('wave') == 9 and tiers.count('workgroup') == 11
    for edge in (32, 64, 128, 2048, 2304, 3072, 4096):  # tier ends and step boundaries: below, at, above
        assert {edge - 1, edge, edge + 1} <= set(up.DEGREES)
    big = sorted(pl['rows'][d] for d in up.DEGREES if up.tier(d) == 'workgroup')
    in_a = [r for r in big if r // 256 == up.BLOCK_A]
    assert len(in_a) >= 3 and in_a[0] % 256 == 0 and in_a[-1] % 256 == 255 and all(r // 256 == up.BLOCK_A + 1 for r in big[len(in_a):])


@pytest.mark.parametrize('s', [0, 1, 31, 32, 33, 63, 64, 2047, 2048, 2049, 4096, 5120, 5121, up.D - 1])
def test_planted_single_seed_closed_form_is_the_restatement(planted, s):
    pl = planted
    cards = up.had_loop_cards(pl['n'], pl['n_self'])
    want = ur.dirty_sets(pl['n'], pl['edge_index'], cards, np.array([[0], [s]]), None, 3)
    closed = up.single_seed_dirty(pl, s)
    assert np.array_equal(want[1], closed[1]) and np.array_equal(want[2], closed[2])
    assert np.array_equal(want[3], closed[2])  # rows have no out-edge: hop 3 reaches nothing new
    assert int(closed[2].sum()) == 1 + sum(d > s for d in up.DEGREES)


def test_planted_self_loop_seeds_follow_column_zero_only(planted):
    pl = planted
    n, n_self = pl['n'], pl['n_self']
    cards = up.had_loop_cards(n, n_self, stride=5)
    cards[[3, up.D + 7], 0] = 0.0          # rows below n_self without a loop before: seeds
    cards[[n_self, n - 1], 0] = 2.5        # trailing rows that had one: seeds
    want = ur.dirty_sets(n, pl['edge_index'], cards, None, None, 3)
    assert np.flatnonzero(want[1]).tolist() == [3, up.D + 7, n_self, n - 1]
    assert np.array_equal(want[2], want[1] | (pl['deg'] > 3)) and np.array_equal(want[3], want[2])
    assert want[3][n_self:].sum() == 2     # a trailing row is dirty only as a seed


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('ss_update_workspace_bytes', 'ss_update_mark', 'ss_update_hop')


def test_update_symbols_are_declared_and_exported():
    import subgraph_sketching_amd as ssa
    text = open(os.path.join(REPO, 'include', 'subgraph_sketch.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(ss_[a-z0-9_]+)\s*\(', text))
    handle = ctypes.CDLL(ssa._native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f'{name} is not declared in include/subgraph_sketch.h'
        assert hasattr(handle, name), f'{name} is not exported by the built library'
        assert name in ssa._native.SIGNATURES
    lib = ssa._native.lib()
    assert lib.ss_update_workspace_bytes(1000, 2) >= 2 * 5 * 1000
    assert lib.ss_update_workspace_bytes(1000, 0) == 0 and lib.ss_update_workspace_bytes(1000, 4) == 0 and lib.ss_update_workspace_bytes(-1, 2) == 0
    # argument errors are found on the host, before any launch
    assert lib.ss_update_mark(None, None, 0, None, 0, None, 1, 2, None, None, 0, None) == -1       # no graph
    assert lib.ss_update_mark(None, None, 0, None, 0, None, 1, 4, None, None, 0, None) == -4       # h = 4
    g = ssa._native.CsrGraphStruct(rowptr=8, col=8, num_nodes=4, n_self_loops=0, n_self_loops_dev=None, hub_threshold=512, reserved=0,
                                   hub_rows=None, hub_count=None, mega_rows=None, mega_count=None, mega_scratch=None, row_begin=0, row_end=0)
    fake = ctypes.c_void_p(8)  # never dereferenced
    assert lib.ss_update_mark(ctypes.byref(g), None, 3, None, 0, fake, 2, 2, None, fake, 1 << 20, None) == -1   # targets missing
    assert lib.ss_update_mark(ctypes.byref(g), fake, 3, None, 0, fake, 2, 2, None, fake, 16, None) == -3        # workspace too small
    assert lib.ss_update_hop(ctypes.byref(g), 3, 2, fake, fake, fake, fake, 128, fake, fake, 8, fake, 2, None, fake, 1 << 20, None) == -1  # hop > h
    assert lib.ss_update_hop(ctypes.byref(g), 2, 2, fake, fake, None, fake, 128, fake, fake, 8, fake, 2, None, fake, 1 << 20, None) == -4  # ids beyond hop 1
    assert lib.ss_update_hop(ctypes.byref(g), 1, 2, fake, fake, fake, fake, 128, None, fake, 6, fake, 2, None, fake, 1 << 20, None) == -4  # HLL from ids: p = 8


def test_workspace_carving_matches_the_documented_layout():
    """update.carve_workspace (what return_info='masks' and the planted marker tests read) on a host buffer: header of 64 int32
    counters, h byte maps pad(N) apart, h int32 lists of pad(N) entries, all inside ss_update_workspace_bytes(N, h), none overlapping"""
    import subgraph_sketching_amd as ssa
    from subgraph_sketching_amd.update import carve_workspace, workspace_info
    lib = ssa._native.lib()
    for n, h in ((1, 1), (255, 2), (256, 3), (257, 3), (6188, 2)):
        pad = (n + 255) & ~255
        nbytes = int(lib.ss_update_workspace_bytes(n, h))
        assert nbytes == 256 + 5 * h * pad
        ws = torch.zeros(nbytes, dtype=torch.uint8)
        counters, maps, lists = carve_workspace(ws, n, h)
        assert counters.dtype == torch.int32 and counters.numel() == 64 and len(maps) == len(lists) == h
        base = ws.data_ptr()
        spans = [(counters.data_ptr() - base, 256)]
        for k in range(h):
            assert maps[k].dtype == torch.uint8 and maps[k].numel() == n and maps[k].data_ptr() - base == 256 + k * pad
            assert lists[k].dtype == torch.int32 and lists[k].numel() == pad and lists[k].data_ptr() - base == 256 + h * pad + 4 * k * pad
            spans += [(maps[k].data_ptr() - base, pad), (lists[k].data_ptr() - base, 4 * pad)]
        spans.sort()
        assert spans[0][0] == 0 and all(a + la == b for (a, la), (b, _) in zip(spans, spans[1:])) and sum(spans[-1]) == nbytes
        # a hand-filled workspace reads back as the info it stands for: rows from the front, hubs from index n - 1 downwards
        last = h - 1
        counters[0], counters[4 * h], counters[4 * h + 1], counters[4 * h + 2] = 7, 3, 2, 1
        maps[last][0] = 1
        lists[last][0], lists[last][1], lists[last][n - 1] = 5, 9, 0
        if n >= 3:
            info = workspace_info(ws, n, h, masks=True)
            assert info['seed_rows'] == 7 and (info['dirty_rows'][h], info['row_list'][h], info['hub_list'][h]) == (3, 2, 1)
            assert info['dirty_mask'][h].dtype == torch.bool and info['dirty_mask'][h].nonzero().flatten().tolist() == [0]
            assert info['rows'][h].tolist() == [5, 9] and info['hubs'][h].tolist() == [0]
            assert set(workspace_info(ws, n, h)) == {'seed_rows', 'dirty_rows', 'row_list', 'hub_list'}


# ---- the method -----------------------------------------------------------------------------------------------------------------------
def _eh(h=2, num_perm=128, p=8):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=num_perm, floor_sf=False, use_zero_one=True))


def _cpu_tables(n, h, num_perm=128, m=256):
    import subgraph_sketching_amd as ssa
    table = ssa.SketchTable()
    for k in range(h + 1):
        table[k] = ssa.HopSketch(torch.zeros((n, num_perm), dtype=torch.int32), torch.zeros((n, m), dtype=torch.uint8), torch.device('cpu'))
    return table, torch.zeros((n, h), dtype=torch.float32)


def test_update_hash_tables_signature():
    import subgraph_sketching_amd as ssa
    sig = inspect.signature(ssa.ElphHashes.update_hash_tables)
    assert list(sig.parameters) == ['self', 'hash_table', 'cards', 'num_nodes', 'edge_index', 'added', 'removed', 'copy', 'return_info']
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {'added': None, 'removed': None, 'copy': False, 'return_info': False}


def test_update_hash_tables_rejects_bad_arguments():
    eh = _eh(h=2)
    n = 10
    table, cards = _cpu_tables(n, 2)
    ei = torch.tensor([[0, 1], [1, 0]])
    one = torch.tensor([[0], [1]])
    with pytest.raises(ValueError, match='added'):
        eh.update_hash_tables(table, cards, n, ei)                                # neither added nor removed
    with pytest.raises(ValueError, match='added'):
        eh.update_hash_tables(table, cards, n, ei, added=torch.tensor([0, 1]))     # not [2, A]
    with pytest.raises(ValueError, match='removed'):
        eh.update_hash_tables(table, cards, n, ei, removed=torch.zeros((3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match='added'):
        eh.update_hash_tables(table, cards, n, ei, added=torch.zeros((2, 2)))      # floating point ids
    with pytest.raises(ValueError, match='edge_index'):
        eh.update_hash_tables(table, cards, n, torch.tensor([0, 1]), added=one)
    with pytest.raises(ValueError, match='cards'):
        eh.update_hash_tables(table, torch.zeros((n, 3)), n, ei, added=one)        # cards of another hop count
    with pytest.raises(ValueError, match='cards'):
        eh.update_hash_tables(table, cards.double(), n, ei, added=one)
    with pytest.raises(ValueError, match='hop 2 is missing'):
        eh.update_hash_tables({0: table[0], 1: table[1]}, cards, n, ei, added=one)
    bad, _ = _cpu_tables(n, 2)
    bad[2] = _cpu_tables(n + 1, 2)[0][2]
    with pytest.raises(ValueError, match='same shape'):
        eh.update_hash_tables(bad, cards, n, ei, added=one)                        # mismatched hop shapes
    bad[2] = _cpu_tables(n, 2, num_perm=64)[0][2]
    with pytest.raises(ValueError, match='same shape'):
        eh.update_hash_tables(bad, cards, n, ei, added=one)
    with pytest.raises(ValueError, match='HopSketch'):
        eh.update_hash_tables({0: table[0], 1: table[1], 2: {'minhash': torch.zeros((n, 128), dtype=torch.int64),
                                                             'hll': torch.zeros((n, 256), dtype=torch.int8)}}, cards, n, ei, added=one)
    other = cards.clone()
    other._ss_tables = 'some-other-table'
    with pytest.raises(ValueError, match='HLL\\+\\+ tables'):
        eh.update_hash_tables(table, other, n, ei, added=one)
    with pytest.raises(ValueError, match='return_info'):
        eh.update_hash_tables(table, cards, n, ei, added=one, return_info='mask')  # True, False or 'masks'
    with pytest.raises(ValueError, match='compute device'):
        eh.update_hash_tables(table, cards, n, ei, added=one)                      # CPU tables: there is no CPU path
