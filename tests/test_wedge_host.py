"""Exact two-hop candidates (WedgeGraph.candidates / ElphHashes.topk_links_wedge, csrc/ss_wedge.hip) without a GPU: the
numpy restatement of the semantics (wedge_restatement.py) against a brute force over every walk written here, against scipy's sparse
product and against the CN heuristic; the argument checks that run before a device is touched; the host block walk rehearsed with
numpy stand-ins for the three launches; the new entry points in the header, the bindings and the library."""
from argparse import Namespace
import collections
import ctypes
import os
import pickle
import re
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import REPO, load_golden
from score_restatement import raw_head
import heuristics_restatement
import wedge_restatement as restated


def _ba40():
    g = load_golden('g3_g4_ba40.npz')
    return int(g['num_nodes']), g['edge_index'].astype(np.int64)


def _uniform200():
    n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
    return 200, restated.induced(restated.uniform_graph(n, e_und, seed), 200)


GRAPHS = {'ba40': _ba40, 'uniform200': _uniform200, 'star': restated.star, 'clique': restated.clique, 'path': restated.path,
          'odd': restated.odd_graph, 'boundary': restated.boundary_graph}
SIMPLE_SYMMETRIC = ('ba40', 'star', 'clique', 'path')


def _sources(N):
    return np.array(list(range(0, N, max(1, N // 40))) + [N - 1, -1, -N, 0, 0, 5 - N], dtype=np.int64)


def _brute_force(N, ei, sources, exclude=None, min_common=1, max_walks=None):
    """Python dicts over every walk: out[u] = the list of v per copy of u -> v"""
    wrap = lambda x: x + N if x < 0 else x
    out = collections.defaultdict(list)
    for u, v in zip(*np.asarray(ei).tolist()):
        out[wrap(u)].append(wrap(v))
    gone = set() if exclude is None else {(wrap(u), wrap(v)) for u, v in zip(*np.asarray(exclude).tolist())}
    rowptr, ids, common, skipped, n_walks = [0], [], [], 0, []
    for u in np.asarray(sources).tolist():
        u = wrap(u)
        count = collections.Counter()
        total = 0
        if 0 <= u < N:
            for w in out[u]:
                for v in out[w]:
                    count[v] += 1
                    total += 1
        n_walks.append(total)
        if not 0 <= u < N or (max_walks is not None and total > max_walks):
            skipped += 1
        else:
            for v in sorted(count):
                if v != u and count[v] >= min_common and (u, v) not in gone:
                    ids.append(v)
                    common.append(count[v])
        rowptr.append(len(ids))
    return (np.array(rowptr, dtype=np.int64), np.array(ids, dtype=np.int64), np.array(common, dtype=np.int32), skipped), np.array(n_walks, dtype=np.int64)


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w)
        else:
            assert g == w


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_restatement_against_the_brute_force(name):
    N, ei = GRAPHS[name]()
    assert N <= 200 or name == 'boundary'
    src = _sources(N)
    want, n_walks = _brute_force(N, ei, src)
    assert want[1].size and np.diff(want[0]).min() < N - 1, 'a trivial case checks nothing'
    _assert_same(restated.candidates(N, ei, src), want)
    np.testing.assert_array_equal(restated.walks(N, ei, src), n_walks)
    _assert_same(restated.candidates(N, ei, src, min_common=2), _brute_force(N, ei, src, min_common=2)[0])
    exclude = np.concatenate([ei[:, ::2], ei[:, :5], np.array([[0, -1, 5], [0, 3, 5 - N]])], axis=1)  # duplicates, self loops, negative ids
    _assert_same(restated.candidates(N, ei, src, exclude=exclude), _brute_force(N, ei, src, exclude=exclude)[0])
    cap = int(n_walks.max()) - 1
    capped = restated.candidates(N, ei, src, max_walks=cap)
    _assert_same(capped, _brute_force(N, ei, src, max_walks=cap)[0])
    assert capped[3] == int((n_walks > cap).sum()) > 0
    _assert_same(restated.candidates(N, ei, src[:0]), (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), 0))


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_restatement_against_the_sparse_product(name):
    N, ei = GRAPHS[name]()
    wrapped = np.where(ei < 0, ei + N, ei)
    A = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.int64), (wrapped[0], wrapped[1])), shape=(N, N))  # (duplicates are summed)
    src = np.arange(N, dtype=np.int64)
    two = (A[src] @ A).toarray()
    np.testing.assert_array_equal(restated.walks(N, ei, src), two.sum(axis=1))
    np.fill_diagonal(two, 0)
    rowptr, ids, common, skipped = restated.candidates(N, ei, src)
    s_of, v = np.nonzero(two)
    assert skipped == 0
    np.testing.assert_array_equal(rowptr, np.concatenate([[0], np.cumsum(np.bincount(s_of, minlength=N))]))
    np.testing.assert_array_equal(ids, v)
    np.testing.assert_array_equal(common, two[s_of, v])


@pytest.mark.parametrize('name', SIMPLE_SYMMETRIC)
def test_common_is_cn_on_simple_symmetric_graphs(name):
    N, ei = GRAPHS[name]()
    assert len(set(zip(*ei.tolist()))) == ei.shape[1] and not (ei[0] == ei[1]).any()
    A = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.float32), (ei[0], ei[1])), shape=(N, N))
    src = np.arange(N, dtype=np.int64)
    rowptr, ids, common, _ = restated.candidates(N, ei, src)
    links = np.stack([np.repeat(src, np.diff(rowptr)), ids], axis=1)
    np.testing.assert_array_equal(heuristics_restatement.scores(A, links, 'CN'), common.astype(np.float32))


def test_the_special_sources():
    N, ei = restated.star()
    rowptr, ids, common, _ = restated.candidates(N, ei, [0, 1, N - 1])
    assert rowptr.tolist() == [0, 0, N - 3, N - 3]  # the centre's walks all return to it; a leaf sees the other leaves; isolated: none
    assert (common == 1).all() and 1 not in ids
    assert restated.walks(N, ei, [0, 1, N - 1]).tolist() == [N - 2, N - 2, 0]
    N, ei = restated.odd_graph()
    rowptr, ids, common, _ = restated.candidates(N, ei, [0, 7, 5, 3, 9, -1])
    rows = [dict(zip(ids[a:b].tolist(), common[a:b].tolist())) for a, b in zip(rowptr[:-1], rowptr[1:])]
    assert rows[0] == {2: 6}      # 0 -> 1 three times, 1 -> 2 twice; the three walks back to 0 are no candidates
    assert rows[1] == {}          # 7 -> 8 -> 7 only
    assert rows[2] == {}          # 5 -> 6, and 6 has no out-edge
    assert rows[3] == {4: 1}      # 3 -> 3 -> 4; (3 -> 3 -> 3 and 3 -> 4 -> 3 end in 3 itself)
    assert rows[4] == {11: 1} and rows[5] == {}
    N, ei = restated.boundary_graph()
    assert restated.walks(N, ei, np.arange(7)).tolist() == [31, 32, 33, 32, 32, 32, 0]
    rowptr, ids, common, _ = restated.candidates(N, ei, [4, 5])
    assert np.diff(rowptr).tolist() == [1, 32] and common[0] == 32 and (common[1:] == 1).all()


# ---- the package, without a device --------------------------------------------------------------------------------------------------
def _eh(h=2, P=128, p=8):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))


def _table(N=30, P=128, p=8, h=2):
    return {k: {'minhash': torch.zeros((N, P), dtype=torch.int64), 'hll': torch.zeros((N, 1 << p), dtype=torch.int8)} for k in range(h + 1)}


def _head(h=2):
    import subgraph_sketching_amd as ssa
    return ssa.StructureHead(**raw_head(h * (h + 2), 1))


def _host_graph(N, ei):
    """a WedgeGraph over CPU tensors: enough for every check that comes before a device is touched, and for the rehearsal"""
    import subgraph_sketching_amd as ssa
    rows = restated.rows_of(N, ei)
    g = object.__new__(ssa.WedgeGraph)
    g.num_nodes, g.num_edges, g.device, g.strict_bounds = N, int(np.asarray(ei).shape[1]), torch.device('cpu'), False
    g.rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64))
    g.col = torch.from_numpy(np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int32))
    return g


def test_graph_arguments_are_checked_before_a_device_is_touched():
    import subgraph_sketching_amd as ssa
    ok = torch.tensor([[0, 1], [1, 2]])
    for n in (1 << 31, 0, -1, 2.5):
        with pytest.raises(ValueError):
            ssa.WedgeGraph(n, ok)
    for bad in (torch.tensor([0, 1, 2]), torch.zeros((3, 2), dtype=torch.int64), torch.zeros((2, 3))):
        with pytest.raises(ValueError):
            ssa.WedgeGraph(30, bad)
    for bad in ([[0], [30]], [[-31], [0]]):  # CPU ids are checked at once
        with pytest.raises(IndexError):
            ssa.WedgeGraph(30, torch.tensor(bad))
    assert ssa.wedge.WedgeGraph is ssa.WedgeGraph and callable(ssa.ElphHashes.topk_links_wedge) and callable(ssa.roofline.wedge_bytes)


def test_query_arguments_are_checked_before_a_device_is_touched():
    N, ei = restated.path(30)
    g = _host_graph(N, ei)
    eh, ok = _eh(), torch.tensor([0, 1])
    calls = [lambda **kw: g.candidates(ok, **kw), lambda **kw: eh.topk_links_wedge(ok, _table(), torch.zeros((30, 2)), 5, _head(), g, **kw)]
    for call in calls:
        for kw in (dict(min_common=0), dict(min_common=1.5), dict(max_walks=-1), dict(max_walks='many'), dict(_lds_slots=0), dict(_lds_slots=48),
                   dict(_lds_slots=8192), dict(exclude=torch.tensor([0, 1, 2])), dict(exclude=torch.zeros((2, 3)))):
            with pytest.raises(ValueError):
                call(**kw)
        with pytest.raises(IndexError):
            call(exclude=torch.tensor([[0], [30]]))
    for bad in (torch.tensor([[0, 1]]), torch.tensor([0.5]), torch.tensor([True])):
        with pytest.raises(ValueError):
            g.candidates(bad)
    for bad in ([0, 30], [-31]):
        with pytest.raises(IndexError):
            g.candidates(torch.tensor(bad))
        with pytest.raises(IndexError):
            eh.topk_links_wedge(torch.tensor(bad), _table(), torch.zeros((30, 2)), 5, _head(), g)


def test_topk_arguments():
    N, ei = restated.path(30)
    g, eh, ok, cards = _host_graph(N, ei), _eh(), torch.tensor([0, 1]), torch.zeros((30, 2))
    with pytest.raises(ValueError, match='WedgeGraph'):
        eh.topk_links_wedge(ok, _table(), cards, 5, _head(), _table())
    with pytest.raises(ValueError, match='31 nodes'):
        eh.topk_links_wedge(ok, _table(), cards, 5, _head(), _host_graph(*restated.path(31)))
    for k in (0, -1, 31):
        with pytest.raises(ValueError, match='k must lie'):
            eh.topk_links_wedge(ok, _table(), cards, k, _head(), g)
    with pytest.raises(ValueError, match='max_hash_hops'):
        eh.topk_links_wedge(ok, _table(), cards, 5, _head(h=3), g)
    with pytest.raises(ValueError, match='degrees'):
        eh.topk_links_wedge(ok, _table(), cards, 5, _head(), g, degrees=torch.ones(30))
    with pytest.raises(ValueError, match='cards'):
        eh.topk_links_wedge(ok, _table(), None, 5, _head(), g)


def test_pickled_state_holds_host_tensors_only():
    N, ei = restated.odd_graph()
    g = _host_graph(N, ei)
    state = g.__getstate__()
    assert set(state) == {'num_nodes', 'num_edges', 'device', 'strict_bounds', 'rowptr', 'col'}
    assert all(not t.is_cuda for t in state.values() if isinstance(t, torch.Tensor)) and isinstance(state['device'], str)
    back = pickle.loads(pickle.dumps(g))
    assert back.num_nodes == N and torch.equal(back.rowptr, g.rowptr) and torch.equal(back.col, g.col) and back.num_edges == ei.shape[1]


def test_byte_model():
    import subgraph_sketching_amd as ssa
    assert ssa.roofline.wedge_bytes(1, 0, 0, 0) == 32
    assert ssa.roofline.wedge_bytes(2, 10, 100, 7) == 64 + 400 + 400 + 84


# ---- the host walk, rehearsed: the three launches replaced by numpy stand-ins that call the restatement ------------------------------
def _rehearse(monkeypatch, N, ei):
    import subgraph_sketching_amd as ssa
    wedge = ssa.wedge
    rows = restated.rows_of(N, ei)
    rng = np.random.RandomState(0)
    launches = collections.Counter()

    def ends_of(u):
        return np.concatenate([rows[w] for w in rows[u]]) if len(rows[u]) else np.zeros(0, dtype=np.int64)

    def wrapped(sources):
        return [int(u) + N if int(u) < 0 else int(u) for u in sources.tolist()]

    def walks(graph, sources, out, err):
        launches['walks'] += 1
        out.copy_(torch.from_numpy(restated.walks(N, ei, sources.numpy())))

    def fold(graph, sources, take, offsets, slots, keys, counts):
        launches['fold'] += 1
        for s, (u, W, o) in enumerate(zip(wrapped(sources), take.tolist(), offsets.tolist())):
            if W > 0 and 2 * W <= slots:
                v, c = np.unique(ends_of(u), return_counts=True)
                assert c.sum() == W
                order = rng.permutation(len(v))  # (in no particular order)
                keys[o:o + len(v)] = torch.from_numpy(s * N + v[order])
                counts[o:o + len(v)] = torch.from_numpy(c[order].astype(np.int32))
                keys[o + len(v):o + W] = wedge._PAD
                counts[o + len(v):o + W] = 0

    def emit(graph, sources, take, offsets, slots, slices, keys):
        launches['emit'] += 1
        assert 1 <= slices <= 64
        for s, (u, W, o) in enumerate(zip(wrapped(sources), take.tolist(), offsets.tolist())):
            if 2 * W > slots:
                keys[o:o + W] = torch.from_numpy(s * N + ends_of(u))

    def exclude_csr(ex, n, device, strict, err):
        if ex is None:
            return None, err
        gone = restated.rows_of(n, ex.numpy())
        return SimpleNamespace(rowptr=torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in gone])]).astype(np.int64)),
                               col=torch.from_numpy(np.concatenate(gone).astype(np.int32))), err

    for name, fn in (('_launch_walks', walks), ('_launch_fold', fold), ('_launch_emit', emit)):
        monkeypatch.setattr(wedge, name, fn)
    monkeypatch.setattr(ssa.candidates, '_exclude_csr', exclude_csr)  # (where the shared walk looks it up)
    return wedge, _host_graph(N, ei), launches


def _got(result):
    return tuple(t.numpy() for t in result[:3])


@pytest.mark.parametrize('name', ['uniform200', 'odd', 'boundary', 'star'])
def test_the_host_walk_rehearsed_with_stand_ins(monkeypatch, name):
    N, ei = GRAPHS[name]()
    wedge, g, launches = _rehearse(monkeypatch, N, ei)
    src = _sources(N)
    exclude = np.concatenate([ei[:, ::2], np.array([[0, -1], [0, 3]])], axis=1)
    n_walks = restated.walks(N, ei, src)
    cap = int(n_walks.max())  # at a source's W(u) it is listed, just below it is skipped
    for kw in (dict(), dict(min_common=2), dict(exclude=exclude), dict(max_walks=cap), dict(max_walks=cap - 1)):
        want = restated.candidates(N, ei, src, **kw)
        tkw = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
        whole = {}
        for slots in (None, 64, 1):  # the default boundary, a low one, everything through the large tier
            rowptr, ids, common, info = g.candidates(torch.from_numpy(src), return_info=True, _lds_slots=slots, **tkw)
            _assert_same((rowptr.numpy(), ids.numpy(), common.numpy(), info['skipped_sources']), want)
            np.testing.assert_array_equal(info['walks'].numpy(), n_walks)
            assert info['lds_sources'] + info['large_sources'] == int(((n_walks > 0) & (n_walks <= kw.get('max_walks', 1 << 40))).sum())
            assert info['lds_sources'] == 0 if slots == 1 else info['large_sources'] == int((2 * n_walks[n_walks <= kw.get('max_walks', 1 << 40)] > (slots or 4096)).sum())
            whole[slots] = (rowptr, ids, common)
        # a few hundred bytes: a block boundary falls inside the source list, and one source alone exceeds the budget
        monkeypatch.setattr(wedge, '_WEDGE_BLOCK_BYTES', 24 * 7)
        assert n_walks.max() * wedge._WEDGE_WALK_BYTES > 24 * 7 and len(src) > 7
        before = launches['walks']
        for slots in (None, 64, 1):
            split = g.candidates(torch.from_numpy(src), _lds_slots=slots, **tkw)
            assert all(torch.equal(a, b) for a, b in zip(split, whole[slots]))
        assert launches['walks'] - before == 3 * -(-len(src) // 7)
        monkeypatch.setattr(wedge, '_WEDGE_BLOCK_BYTES', 1 << 30)
    none = g.candidates(torch.from_numpy(src[:0]), return_info=True)
    assert none[0].tolist() == [0] and none[1].shape == (0,) and none[2].dtype == torch.int32 and none[3]['skipped_sources'] == 0


def test_the_tier_boundary_rehearsed(monkeypatch):
    N, ei = restated.boundary_graph()
    wedge, g, launches = _rehearse(monkeypatch, N, ei)
    src = torch.arange(8)
    rowptr, ids, common, info = g.candidates(src, return_info=True, _lds_slots=64)
    assert info['walks'].tolist() == [31, 32, 33, 32, 32, 32, 0, 0]
    assert (info['lds_sources'], info['large_sources']) == (5, 1)  # 2 W <= 64 folds: only W = 33 is emitted
    _assert_same(_got((rowptr, ids, common)), restated.candidates(N, ei, src.numpy())[:3])


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_and_exported():
    import subgraph_sketching_amd as ssa
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'subgraph_sketch.h')).read(), flags=re.S)
    assert os.path.exists(ssa._native.LIB_PATH), 'run `python __graft_entry__.py` first (build())'
    handle = ctypes.CDLL(ssa._native.LIB_PATH)
    for name, n_args in (('ss_wedge_walks', 8), ('ss_wedge_fold', 11), ('ss_wedge_emit', 11)):
        assert re.search(r'\bint\s+%s\s*\(' % name, text)
        restype, argtypes = ssa._native.SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == n_args and hasattr(handle, name)
    assert re.search(r'#define\s+SS_WEDGE_MAX_SLOTS\s+%d\b' % ssa._native.WEDGE_MAX_SLOTS, text)


def test_argument_errors_of_the_library_are_reported_without_a_gpu():
    from ctypes import c_void_p
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(16)  # never dereferenced
    assert lib.ss_wedge_walks(fake, fake, 1 << 31, fake, 4, fake, None, None) == -1  # col is int32
    assert lib.ss_wedge_walks(fake, fake, 30, fake, -1, fake, None, None) == -1
    assert lib.ss_wedge_walks(fake, fake, 30, fake, 1 << 31, fake, None, None) == -1
    assert lib.ss_wedge_walks(None, fake, 30, fake, 4, fake, None, None) == -1
    assert lib.ss_wedge_walks(fake, fake, 30, fake, 4, None, None, None) == -1
    assert lib.ss_wedge_walks(fake, fake, 0, fake, 4, fake, None, None) == -1       # sources of an empty graph
    assert lib.ss_wedge_walks(None, None, 30, None, 0, None, None, None) == 0       # no sources: nothing to do

    def fold(rowptr=fake, col=fake, n=30, src=fake, s=4, walks=fake, offsets=fake, slots=64, keys=fake, counts=fake):
        return lib.ss_wedge_fold(rowptr, col, n, src, s, walks, offsets, slots, keys, counts, None)

    def emit(rowptr=fake, col=fake, n=30, src=fake, s=4, walks=fake, offsets=fake, slots=64, slices=1, keys=fake):
        return lib.ss_wedge_emit(rowptr, col, n, src, s, walks, offsets, slots, slices, keys, None)

    for call in (fold, emit):
        assert call(slots=0) == -1 and call(slots=48) == -1 and call(slots=8192) == -1 and call(slots=-64) == -1
        assert call(walks=None) == -1 and call(offsets=None) == -1 and call(keys=None) == -1 and call(col=None) == -1
        assert call(n=1 << 31) == -1 and call(s=-1) == -1
        assert call(s=0, rowptr=None, col=None, src=None, walks=None, offsets=None, keys=None) == 0
    assert fold(counts=None) == -1
    assert emit(slices=0) == -1 and emit(slices=65) == -1
