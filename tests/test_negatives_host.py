"""Negative sampling (NegativeSampler / sample_negatives, csrc/ss_negatives.hip) without a GPU: known answers of the draw,
the Python restatement of the semantics (negatives_restatement.py) against a set-based checker written here, the proposal law of the
wedge mode, the cap on unsampled slots, the argument checks that run before a device is touched, and the new entry point in the
header, the bindings and the library."""
import collections
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import negatives_restatement as restated

N, EI = restated.negatives_graph()
EDGES = set(zip(*EI.tolist()))
OUT = collections.defaultdict(set)  # OUT[u] = {v : u -> v}
for _u, _v in EDGES:
    OUT[_u].add(_v)
ALL_NODES = np.stack([np.arange(N), (np.arange(N) * 7 + 1) % N], axis=1).astype(np.int64)
HELD_OUT = np.array([[0, 0, 3, 388, 17, -1], [1, 2, 4, 389, -5, 6]], dtype=np.int64)  # an exclude list (negative ids included)


# computed from the formula with numpy uint64 arithmetic, independently of negatives_restatement.py
DRAWS = [((0, 0, 0, 0), 0x4181b152fb77616f), ((0, 0, 0, 1), 0x169c646d52269d62), ((0, 1, 0, 0), 0x657e0be0e89a4916),
         ((1, 0, 0, 0), 0x275f2ae791fef8a1), ((7, 770, 15, 1), 0xf4637262054cf81e),
         (((1 << 64) - 1, (1 << 40) + 3, 63, 1), 0xb2cafcafc29b1240), ((12345, 1 << 31, 5, 0), 0x8b52c24ecc150940)]


def test_known_answers_of_the_draw():
    for args, want in DRAWS:
        assert restated.draw(*args) == want
    assert restated.pick((1 << 64) - 1, 400) == 399 and restated.pick(0, 400) == 0 and restated.pick(1 << 63, 401) == 200


def _sets(n, ei):
    """(N, the set of arcs, {u: {v : u -> v}}) of a graph"""
    edges = set(zip(*np.asarray(ei).tolist()))
    out = collections.defaultdict(set)
    for u, v in edges:
        out[u].add(v)
    return n, edges, out


def _candidates(u, mode, gone=frozenset(), graph=None):
    """every v a slot of source u may return, from sets alone (graph: _sets of another graph than the module's)"""
    n, edges, out = graph or (N, EDGES, OUT)
    reach = {v for w in out[u] for v in out[w]} if mode == 'wedge' else set(range(n))
    return {v for v in reach if v != u and (u, v) not in edges and (u, v) not in gone}


def _check(out, unsampled, mode, positives, num_neg, gone=frozenset(), graph=None):
    n, edges, arcs = graph or (N, EDGES, OUT)
    assert out.dtype == np.int64 and out.shape == (len(positives) * num_neg, 2)
    assert unsampled == int((out[:, 1] < 0).sum())
    for q, (u, v) in enumerate(out.tolist()):
        assert u == int(positives[q // num_neg][0]) % n
        if not _candidates(u, mode, gone, graph):
            assert v == -1, f'source {u} has no candidate in mode {mode}'
        if v >= 0:
            assert v != u and (u, v) not in edges and (u, v) not in gone
            if mode == 'wedge':
                assert arcs[u] & {w for w in range(n) if v in arcs[w]}, f'no w with {u} -> w -> {v}'


@pytest.mark.parametrize('mode', restated.MODES)
@pytest.mark.parametrize('num_neg,seed', [(1, 0), (3, 1)])
def test_restatement_against_the_set_based_checker(mode, num_neg, seed):
    positives = np.concatenate([ALL_NODES, EI.T[:257], ALL_NODES[[398, 383, 399, 360]] - N])  # (negative ids wrap)
    out, unsampled = restated.sample(N, EI, positives, num_neg=num_neg, mode=mode, seed=seed)
    _check(out, unsampled, mode, positives, num_neg)
    if mode == 'wedge':  # the star centre, the K5 members, the isolated nodes: never sampled
        for u in (398, 383, 384, 385, 386, 387, 399, 360, 381):
            assert not _candidates(u, 'wedge')
        assert (out[:, 1] >= 0).mean() > 0.8
    else:
        assert unsampled == 0


@pytest.mark.parametrize('mode', restated.MODES)
def test_restatement_with_an_exclude_list(mode):
    gone = {(int(u) % N, int(v) % N) for u, v in HELD_OUT.T}
    assert not gone & EDGES, 'held-out pairs are not edges of the graph'
    positives = np.repeat(np.array([[0, 9], [3, 9], [388, 9], [17, 9], [N - 1, 9]], dtype=np.int64), 40, axis=0)
    out, unsampled = restated.sample(N, EI, positives, num_neg=5, mode=mode, seed=3, exclude=HELD_OUT)
    _check(out, unsampled, mode, positives, 5, gone)
    free, _ = restated.sample(N, EI, positives, num_neg=5, mode=mode, seed=3)
    if mode == 'wedge':  # 388 -> 398 -> 389 is a wedge: without the list it comes back, with it never
        assert (388, 389) in set(map(tuple, free.tolist())) and (388, 389) not in set(map(tuple, out.tolist()))


@pytest.mark.parametrize('mode', restated.MODES)
@pytest.mark.parametrize('num_neg,max_tries', [(1, 1), (3, 4), (7, 16)])
def test_restatement_on_the_directed_graph(mode, num_neg, max_tries):
    n, ei = restated.directed_graph()
    graph = _sets(n, ei)
    assert not {(1, 0), (10, 1), (6, 5), (31, 30), (40, 41)} & graph[1], 'a directed graph'
    positives = np.stack([np.arange(n), np.arange(n)[::-1]], axis=1).astype(np.int64)
    out, unsampled = restated.sample(n, ei, positives, num_neg=num_neg, mode=mode, seed=2, max_tries=max_tries)
    _check(out, unsampled, mode, positives, num_neg, graph=graph)
    src = restated.DIRECTED_SOURCES
    if mode == 'wedge':
        for name in ('all_sinks', 'rejected', 'no_out_arc'):
            assert not _candidates(src[name], 'wedge', graph=graph)
        assert _candidates(src['mixed'], 'wedge', graph=graph) == {10, 11, 12}  # (not 0 itself, reached through 2)
        assert _candidates(src['repeated'], 'wedge', graph=graph) == {33, 34, 35}


def test_the_directed_plan_is_not_trivial():
    """the all-sinks source is unsampled in every slot (each attempt stops at a w without an out-arc), the mixed source is sampled in
    some slot and stopped at a sink in some attempt, and the repeated arc 30 -> 31 is picked three times out of four"""
    n, ei = restated.directed_graph()
    rows = restated.rows_of(n, ei)
    src = restated.DIRECTED_SOURCES
    assert all(not rows[w] for w in rows[src['all_sinks']]) and len(rows[src['all_sinks']]) == 3
    assert [bool(rows[w]) for w in rows[src['mixed']]] == [True, True, False, False]
    assert rows[src['repeated']] == [31, 31, 31, 32] and not rows[src['no_out_arc']]
    for num_neg, max_tries in ((1, 1), (3, 4), (7, 16)):
        positives = np.array([[src['all_sinks'], 0], [src['mixed'], 0], [src['repeated'], 0]], dtype=np.int64)
        out, unsampled = restated.sample(n, ei, positives, num_neg=num_neg, mode='wedge', seed=0, max_tries=max_tries)
        by = out[:, 1].reshape(3, num_neg)
        assert (by[0] == -1).all() and (out[:num_neg, 0] == src['all_sinks']).all()
        assert unsampled >= num_neg
        if max_tries > 1:
            assert (by[1] >= 0).any() and (by[2] >= 0).all()
    # at one try per slot, a slot of the mixed source whose w is a sink stays unsampled: the `continue` is taken, not only passed by
    first_w = [rows[0][restated.pick(restated.draw(0, q, 0, 0), 4)] for q in range(64)]
    out, _ = restated.sample(n, ei, np.array([[0, 0]]), num_neg=64, mode='wedge', seed=0, max_tries=1)
    assert {3, 4} & set(first_w) and {1, 2} & set(first_w)
    assert all(v == -1 for w, v in zip(first_w, out[:, 1].tolist()) if w in (3, 4))
    many, _ = restated.sample(n, ei, np.array([[30, 0]]), num_neg=400, mode='wedge', seed=1, max_tries=1)
    assert 250 < int(np.isin(many[:, 1], [33, 34]).sum()) < 350  # 3 / 4 of 400, within 5 sigma (43)


def test_any_source_uniform():
    out, unsampled = restated.sample(N, EI, None, mode='uniform', seed=5, num_samples=1000)
    assert out.shape == (1000, 2) and unsampled == 0
    for u, v in out.tolist():
        assert 0 <= u < N and 0 <= v < N and u != v and (u, v) not in EDGES
    assert len(set(out[:, 0].tolist())) > 300  # the sources are drawn, not fixed


@pytest.mark.parametrize('mode', restated.MODES)
def test_restatement_does_not_depend_on_the_split(mode):
    positives = ALL_NODES[::3]
    whole, unsampled = restated.sample(N, EI, positives, num_neg=3, mode=mode, seed=2)
    n = len(whole)
    parts = [restated.sample(N, EI, positives, num_neg=3, mode=mode, seed=2, slots=range(a, min(a + 64, n))) for a in range(0, n, 64)]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), whole)
    assert sum(p[1] for p in parts) == unsampled
    # ... nor on the positives around it: positive i alone, at its own slots
    one, _ = restated.sample(N, EI, positives[:8], num_neg=3, mode=mode, seed=2, slots=range(21, 24))
    np.testing.assert_array_equal(one, whole[21:24])


def test_the_wedge_law_is_proportional_to_ra():
    """20 000 slots of one source: the count of every eligible v within 5 sigma (+ 1) of n p, p = pi(v) / sum of pi over the
    eligible, pi(v) = sum_w mult(u, w) mult(w, v) / (deg u deg w) -- the resource-allocation score of (u, v) over deg u.  Node 3 has
    the doubled edge (3, 5) and the hub 382 among its neighbours."""
    u, n = 3, 20000
    mult = collections.Counter(zip(*EI.tolist()))
    deg = collections.Counter(EI[0].tolist())
    pi = collections.defaultdict(float)
    for (a, w), m_uw in mult.items():
        if a == u:
            for (b, v), m_wv in mult.items():
                if b == w:
                    pi[v] += m_uw * m_wv / (deg[u] * deg[w])
    assert abs(sum(pi.values()) - 1.0) < 1e-12 and mult[(3, 5)] == 2 and (3, 382) in mult
    ok = _candidates(u, 'wedge')
    assert ok == {v for v in pi if v != u and (u, v) not in EDGES} and len(ok) > 100
    total = sum(pi[v] for v in ok)
    out, unsampled = restated.sample(N, EI, np.array([[u, 0]]), num_neg=n, mode='wedge', seed=0, max_tries=64)
    assert unsampled == 0 and set(out[:, 1].tolist()) <= ok
    counts = collections.Counter(out[:, 1].tolist())
    for v in sorted(ok):
        p = pi[v] / total
        assert abs(counts[v] - n * p) <= 5 * math.sqrt(n * p * (1 - p)) + 1, (v, counts[v], n * p)


@pytest.mark.parametrize('mode', restated.MODES)
def test_at_most_one_percent_of_the_eligible_slots_stay_unsampled(mode):
    has = np.array([bool(_candidates(u, mode)) for u in range(N)])
    assert has.sum() == (370 if mode == 'wedge' else N)
    for seed in (0, 1, 2):
        out, _ = restated.sample(N, EI, ALL_NODES, num_neg=8, mode=mode, seed=seed, max_tries=16)
        missed = int(((out[:, 1] < 0) & np.repeat(has, 8)).sum())
        assert missed <= 0.01 * 8 * has.sum(), (mode, seed, missed)


# ---- the package, without a device --------------------------------------------------------------------------------------------------
GRAPH = torch.from_numpy(EI.copy())
OK = torch.tensor([[0, 1], [2, 3]])


@pytest.mark.parametrize('kw', [dict(mode='hard'), dict(mode=None), dict(num_neg=0), dict(num_neg=1.5), dict(max_tries=0), dict(max_tries=65),
                                dict(positives=torch.tensor([0, 1])), dict(positives=torch.tensor([[0.0, 1.0]])),
                                dict(positives=torch.tensor([[0, 1, 2]])), dict(positives=None, mode='same_source', num_samples=4),
                                dict(positives=None, mode='wedge', num_samples=4), dict(positives=None, mode='uniform'),
                                dict(num_samples=4), dict(seed=-1), dict(seed=1 << 64), dict(batch_size=0)])
def test_arguments_are_checked_before_a_device_is_touched(kw):
    import subgraph_sketching_amd as ssa
    kw = dict(dict(positives=OK), **kw)
    with pytest.raises(ValueError):
        ssa.sample_negatives(N, GRAPH, **kw)


def test_graph_arguments_are_checked_before_a_device_is_touched():
    import subgraph_sketching_amd as ssa
    for n in (1 << 31, 0, -1, 2.5):
        with pytest.raises(ValueError):
            ssa.sample_negatives(n, GRAPH, OK)
        with pytest.raises(ValueError):
            ssa.NegativeSampler(n, GRAPH)
    for bad in (torch.tensor([0, 1, 2]), torch.zeros((3, 2), dtype=torch.int64), torch.zeros((2, 3))):
        with pytest.raises(ValueError):
            ssa.NegativeSampler(N, bad)
        with pytest.raises(ValueError):
            ssa.NegativeSampler(N, GRAPH, exclude=bad)
    # CPU ids are checked at once, as the link queries check them
    for bad in ([[0], [N]], [[-N - 1], [0]]):
        with pytest.raises(IndexError):
            ssa.NegativeSampler(N, torch.tensor(bad))
        with pytest.raises(IndexError):
            ssa.sample_negatives(N, GRAPH, OK, exclude=torch.tensor(bad))
    for bad in ([[N, 0]], [[-N - 1, 0]]):
        with pytest.raises(IndexError):
            ssa.sample_negatives(N, GRAPH, torch.tensor(bad))
    assert ssa.negatives.NegativeSampler is ssa.NegativeSampler and ssa.negatives.sample_negatives is ssa.sample_negatives


def test_the_entry_point_is_declared_bound_and_exported():
    import subgraph_sketching_amd as ssa
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'subgraph_sketch.h')).read(), flags=re.S)
    assert os.path.exists(ssa._native.LIB_PATH), 'run `python __graft_entry__.py` first (build())'
    handle = ctypes.CDLL(ssa._native.LIB_PATH)
    assert re.search(r'\bint\s+ss_sample_negatives\s*\(', text)
    restype, argtypes = ssa._native.SIGNATURES['ss_sample_negatives']
    assert restype is ctypes.c_int32 and len(argtypes) == 17 and hasattr(handle, 'ss_sample_negatives')
    for name, value in (('SS_NEG_UNIFORM', 0), ('SS_NEG_SAME_SOURCE', 1), ('SS_NEG_WEDGE', 2)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, value), text)
    assert ssa._native.NEG_MODES == {'uniform': 0, 'same_source': 1, 'wedge': 2}
    assert re.search(r'#define\s+SS_NEG_MAX_TRIES\s+%d\b' % ssa._native.NEG_MAX_TRIES, text)
    assert handle.ss_version() == 129


def test_argument_errors_of_the_library_are_reported_without_a_gpu():
    from ctypes import c_void_p
    import subgraph_sketching_amd as ssa
    fn = ssa._native.lib().ss_sample_negatives
    fake = c_void_p(16)  # never dereferenced

    def call(rowptr=fake, col=fake, xr=None, xc=None, n=400, src=fake, stride=2, slots=10, num_neg=1, mode=2, seed=0, tries=16, first=0,
             out=fake, unsampled=None, err=None):
        return fn(rowptr, col, xr, xc, n, src, stride, slots, num_neg, mode, seed, tries, first, out, unsampled, err, None)

    assert call(n=1 << 31) == -1       # col is int32
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(num_neg=0) == -1 and call(tries=0) == -1 and call(tries=65) == -1
    assert call(slots=-1) == -1 and call(first=-1) == -1
    assert call(src=None, mode=1) == -1 and call(src=None, mode=2) == -1  # only uniform samples any source
    assert call(stride=0) == -1
    assert call(xr=fake) == -1 and call(xc=fake) == -1  # half an exclude CSR
    assert call(rowptr=None) == -1 and call(col=None) == -1 and call(out=None) == -1
    assert call(out=c_void_p(8)) == -1  # a pair leaves as one 16-byte store
    assert call(n=0, src=None, mode=0) == -1
    assert call(slots=0) == 0 and call(slots=0, rowptr=None, col=None, out=None, src=None, mode=0) == 0  # nothing to do
