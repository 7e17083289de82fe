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
            ('power-law', 3000, ur.power_law_graph(3000, 9000, 13)), ('power-law-steep', 2500, ur.power_law_graph(2500, 6000, 14, exponent=5.0))]


@pytest.mark.parametrize('name,n,ei', _graphs(), ids=[g[0] for g in _graphs()])
def test_rule_covers_additions_removals_and_both(name, n, ei, prm):
    rng = np.random.RandomState(len(name))
    half = ei.shape[1] // 2
    new_add, added = ur.add_edges(ei, rng.randint(0, n, size=(2, 5)))
    _, changed = _assert_rule_is_sufficient(n, ei, new_add, added, None, prm)
    assert changed > 0
    new_rem, removed = ur.remove_edges(ei, rng.choice(half, size=5, replace=False))
    _assert_rule_is_sufficient(n, ei, new_rem, None, removed, prm)
    mid, removed = ur.remove_edges(ei, rng.choice(half, size=4, replace=False))
    new_both, added = ur.add_edges(mid, rng.randint(0, n, size=(2, 4)))
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
    with pytest.raises(ValueError, match='compute device'):
        eh.update_hash_tables(table, cards, n, ei, added=one)                      # CPU tables: there is no CPU path
