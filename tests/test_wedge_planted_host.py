"""The planted graphs of the two-hop kernels (wedge_planted.py) without a GPU: every plan against scipy's A[sources] @ A (the
formulation test_wedge_host.py already trusts), the builds that wedge_restatement.py can afford against it, the Python twin of
csrc/ss_wedge.hpp against its literal known answers and against the tier counts of the rehearsed host walk, and the planted graphs
through that rehearsal with a group boundary on, just below and just above a cumulative sum of walks."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import REPO
from test_wedge_host import _rehearse
import wedge_planted as planted
import wedge_restatement as restated


def _max_slots():
    import subgraph_sketching_amd as ssa
    return ssa._native.WEDGE_MAX_SLOTS


FULL = {'table_sizes': lambda: planted.table_sizes(_max_slots()), 'wide_fold': lambda: planted.wide_fold(_max_slots()),
        'collisions': lambda: planted.collisions(_max_slots()), 'emit_shapes': lambda: planted.emit_shapes(_max_slots()),
        'mixed': lambda: planted.mixed(_max_slots()),
        'walks_46341_squared': lambda: planted.too_many_walks(*planted.GIANTS[0]), 'walks_2_to_31': lambda: planted.too_many_walks(*planted.GIANTS[1])}
# the same builders at sizes where a Python list per node is affordable (N <= 5 000)
SMALL = {'table_sizes': lambda: planted.table_sizes(512), 'wide_fold': lambda: planted.wide_fold(1024, T=64),
         'emit_shapes': lambda: planted.emit_shapes(256, T=32, big=600),
         'collisions': lambda: planted.collisions(256, N=5000),  # (tables of 64 and 256 slots: the chains that wrap from m - 1 to 0)
         'walks_46341_squared': FULL['walks_46341_squared'], 'walks_2_to_31': FULL['walks_2_to_31']}


@pytest.mark.parametrize('name', sorted(FULL))
def test_the_plan_equals_the_sparse_product(name):
    N, ei, src, expect, _ = FULL[name]()
    assert N <= 70000 and ei.shape[1] < 400000 and (src == np.arange(len(src))).all()
    A = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.int64), (ei[0], ei[1])), shape=(N, N))  # (duplicates are summed)
    two = (A[src] @ A).tocsr()
    two.sum_duplicates()
    assert two.dtype == np.int64
    np.testing.assert_array_equal(np.asarray(two.sum(axis=1)).reshape(-1), expect['walks'])
    for s, u in enumerate(src.tolist()):
        row = two.getrow(s)
        ends = {int(v): int(c) for v, c in zip(row.indices, row.data) if c}
        assert ends == expect['ends'][s], (name, u)
        assert {v: c for v, c in ends.items() if v != u} == expect['rows'][s], (name, u)  # the v != u filter
    # ... and the arrays that the GPU tests compare with, under each filter
    listed = expect['walks'] <= planted.MAX_WALKS
    for kw in (dict(), dict(min_common=2), dict(exclude_edges=True)):
        rowptr, ids, common, skipped = planted.want(N, ei, src, expect, **kw)
        assert skipped == int((~listed).sum())
        for s, u in enumerate(src.tolist()):
            row = two.getrow(s)
            keep = (row.indices != u) & (row.data >= kw.get('min_common', 1)) & bool(listed[s])
            if kw.get('exclude_edges'):
                keep &= ~np.isin(row.indices, A.getrow(u).indices)
            order = np.argsort(row.indices[keep])
            np.testing.assert_array_equal(ids[rowptr[s]:rowptr[s + 1]], row.indices[keep][order])
            np.testing.assert_array_equal(common[rowptr[s]:rowptr[s + 1]], row.data[keep][order])
        assert rowptr[-1] == ids.size == common.size and common.dtype == np.int32 and ids.dtype == np.int64


@pytest.mark.parametrize('name', sorted(SMALL))
def test_the_small_builds_equal_the_restatement(name):
    N, ei, src, expect, _ = SMALL[name]()
    assert N <= 5000
    np.testing.assert_array_equal(restated.walks(N, ei, src), expect['walks'])
    for kw, rkw in ((dict(), dict()), (dict(min_common=2), dict(min_common=2)), (dict(exclude_edges=True), dict(exclude=ei)),
                    (dict(max_walks=5), dict(max_walks=5))):
        got, want = planted.want(N, ei, src, expect, **kw), restated.candidates(N, ei, src, **rkw)
        for a, b in zip(got[:3], want[:3]):
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a, b)
        assert got[3] == want[3]


def test_the_twin_reproduces_its_known_answers():
    ks = [k for _, k, _ in planted.KNOWN_SLOTS]
    assert len(planted.KNOWN_SLOTS) >= 16 and {1, 6, 8, 12} <= set(ks) and max(v for v, _, _ in planted.KNOWN_SLOTS) == (1 << 31) - 1
    for v, k, h in planted.KNOWN_SLOTS:
        assert planted.slot(v, k) == h and int(planted.slots_of([v], k)[0]) == h and 0 <= h < (1 << k)
    for W, slots, m in ((1, 4096, 2), (2, 4096, 4), (3, 4096, 8), (32, 4096, 64), (33, 4096, 128), (2048, 4096, 4096), (31, 64, 64), (4, 8, 8)):
        assert planted.table_slots(W, slots) == m and planted.folds(W, slots) and not planted.emits(W, slots)
    assert planted.emits(2049, 4096) and not planted.folds(2049, 4096) and not planted.folds(0, 64) and not planted.emits(0, 1)
    assert planted.emits(1, 1) and planted.tiers([0, 1, 32, 33, 1 << 31], 64) == (2, 1)
    # 3, 4 095 and 65 535 start at slot 54 of 64: a chain; from the last slot it goes on at slot 0
    assert planted.probe_places([3, 4095, 3, 65535], 64) == {3: (54, 54), 4095: (54, 55), 65535: (54, 56)}
    assert planted.probe_places([1, 3], 2) == {1: (1, 1), 3: (1, 0)}


def test_the_host_check_holds_the_same_known_answers():
    """tools/wedge_host_check.hip checks wedge_slot of csrc/ss_wedge.hpp against a literal table: the same numbers as KNOWN_SLOTS"""
    text = open(os.path.join(REPO, 'tools', 'wedge_host_check.hip')).read()
    body = text[text.index('known[] = {'):text.index('for (const auto &a : known)')]
    triples = tuple(tuple(int(x) for x in t) for t in re.findall(r'\{(\d+), (\d+), (\d+)\}', body))
    assert triples == planted.KNOWN_SLOTS and 'CHECK(wedge_slot(a.v, a.k) == a.slot)' in text


def test_the_twin_agrees_with_the_rehearsal_on_the_boundary_graph(monkeypatch):
    N, ei = restated.boundary_graph()
    wedge, g, _ = _rehearse(monkeypatch, N, ei)
    info = g.candidates(torch.arange(8), return_info=True, _lds_slots=64)[3]
    W = info['walks'].tolist()
    assert W == [31, 32, 33, 32, 32, 32, 0, 0]
    assert (info['lds_sources'], info['large_sources']) == planted.tiers(W, 64) == (5, 1)
    assert [planted.table_slots(w, 64) for w in W[:6] if planted.folds(w, 64)] == [64] * 5
    default = g.candidates(torch.arange(8), return_info=True)[3]
    assert (default['lds_sources'], default['large_sources']) == planted.tiers(W, _max_slots()) == (6, 0)


@pytest.mark.parametrize('name', sorted(SMALL))
def test_the_planted_graphs_through_the_rehearsed_host_walk(monkeypatch, name):
    """a group holds the sources whose cumulative walks fit the budget: the budget is put exactly on the sum up to a source that a
    source without walks follows, one below it and one above it; the first source has no walks either"""
    N, ei, src, expect, _ = SMALL[name]()
    wedge, g, launches = _rehearse(monkeypatch, N, ei)
    W = np.where(expect['walks'] > planted.MAX_WALKS, 0, expect['walks'])
    ends = np.cumsum(W)
    ok = [j for j in range(1, len(W) - 1) if W[j] > 0 and W[j + 1] == 0 and ends[j] < ends[-1]]
    j = ok[len(ok) // 2]
    assert W[0] == 0 and W[-1] == 0 and ends[j] > 2
    want = planted.want(N, ei, src, expect)
    sd = torch.from_numpy(src)
    for slots in (None, 64, 1):
        whole = g.candidates(sd, return_info=True, _lds_slots=slots)
        for got, w in zip(whole[:3], want[:3]):
            np.testing.assert_array_equal(got.numpy(), w)
        np.testing.assert_array_equal(whole[3]['walks'].numpy(), expect['walks'])
        assert (whole[3]['lds_sources'], whole[3]['large_sources']) == planted.tiers(expect['walks'], slots or _max_slots())
        assert whole[3]['skipped_sources'] == want[3]
        for room in (int(ends[j]), int(ends[j]) - 1, int(ends[j]) + 1):
            monkeypatch.setattr(wedge, '_WEDGE_BLOCK_BYTES', room * wedge._WEDGE_WALK_BYTES)
            before = launches['fold'] + launches['emit']
            split = g.candidates(sd, return_info=True, _lds_slots=slots)
            monkeypatch.setattr(wedge, '_WEDGE_BLOCK_BYTES', 1 << 30)
            assert launches['fold'] + launches['emit'] - before >= 2, 'the budget splits the sources into groups'
            assert all(torch.equal(a, b) for a, b in zip(split[:3], whole[:3]))
            assert (split[3]['lds_sources'], split[3]['large_sources']) == (whole[3]['lds_sources'], whole[3]['large_sources'])
