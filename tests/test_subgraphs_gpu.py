"""ElphHashes.exact_subgraphs (subgraphs.py, csrc/ss_subgraph.hip) on the GPU: every field must EQUAL the numpy restatement
(tests/subgraph_restatement.py), rowptr / ids / dist must equal exact_subgraph_nodes on the same arguments, and on BA-40 the labels must
equal what the reference's own labelling functions gave (tests/golden/g17_seal_labels.npz) -- under batching and shuffling, through
either tier of the node list and of the label kernel, through either direction of the adjacency intersection, on multigraphs, self
loops, masked links, u == v, unreachable roots, max_nodes and the edge cases (no links, no edges, CPU inputs, a directed edge_index).
The two kernels on hand-made rows, where their branches are planted: tests/subgraph_planted.py, tests/test_subgraph_planted_{host,gpu}.py."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import subgraph_restatement as sr
from conftest import load_golden
from test_exact_nodes_gpu import _arena_is_zero, _stars
from test_exact_nodes_host import _ba40, _uniform300
from test_subgraphs_host import GOLDEN_LABELS, _multigraph, _path, _two_components

pytestmark = pytest.mark.gpu
LABELS = ('drnl', 'de', 'de+', 'hop', 'zo', None)
FIELDS = ('rowptr', 'ids', 'dist', 'roots', 'adj_ptr', 'nbr', 'weight')


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture
def lds_limit(ssa):
    """sets knobs.EXACT_LDS_MAX_NODES (the node list's and the label kernel's on-chip limit) for one test and restores it"""
    old = ssa.knobs.EXACT_LDS_MAX_NODES
    yield lambda value: setattr(ssa.knobs, 'EXACT_LDS_MAX_NODES', value)
    ssa.knobs.EXACT_LDS_MAX_NODES = old


@pytest.fixture
def adj_switch(ssa):
    """sets knobs.SUBGRAPH_ADJ_SWITCH for one test and restores it"""
    old = ssa.knobs.SUBGRAPH_ADJ_SWITCH
    yield lambda value: setattr(ssa.knobs, 'SUBGRAPH_ADJ_SWITCH', value)
    ssa.knobs.SUBGRAPH_ADJ_SWITCH = old


def _eh(ssa, h=2):
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))


def _run(eh, n, ei, links, dev, check_nodes=True, **kw):
    """one call with everything on the device -> the ExactSubgraphs' fields as numpy (+ z, info)"""
    ld, ed = torch.from_numpy(np.asarray(links, dtype=np.int64)).to(dev), torch.from_numpy(ei).to(dev)
    sg = eh.exact_subgraphs(ld, n, ed, **kw)
    assert all(getattr(sg, k).device == dev for k in FIELDS) and (sg.z is None or sg.z.device == dev)
    assert sg.rowptr.dtype == sg.ids.dtype == sg.adj_ptr.dtype == torch.int64 and sg.dist.dtype == torch.uint8
    assert sg.roots.dtype == sg.nbr.dtype == sg.weight.dtype == torch.int32 and (sg.z is None or sg.z.dtype == torch.int64)
    got = {k: getattr(sg, k).cpu().numpy() for k in FIELDS}
    got['z'], got['info'], got['sg'] = None if sg.z is None else sg.z.cpu().numpy(), sg.info, sg
    if check_nodes:  # the node rows are the node list's, bit for bit
        nodes_kw = {k: v for k, v in kw.items() if k in ('batch_size', 'max_nodes')}
        want = eh.exact_subgraph_nodes(ld, n, ed, mask_target=kw.get('mask_target', True), **nodes_kw)
        for k, w in zip(('rowptr', 'ids', 'dist'), want):
            np.testing.assert_array_equal(got[k], w.cpu().numpy(), err_msg=f'{k} against exact_subgraph_nodes')
    return got


def _same(got, sub, label='drnl', max_dist=1000):
    """every field equals the restatement `sub` (a Restated, or a dict of fields from another run)"""
    want = sub if isinstance(sub, dict) else dict({k: getattr(sub, k) for k in FIELDS}, z=sr.labels(sub, label, max_dist))
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if want['z'] is None:
        assert got['z'] is None
    else:
        assert got['z'].shape == want['z'].shape
        np.testing.assert_array_equal(got['z'], want['z'], err_msg=f'z ({label}, max_dist {max_dist})')


# ---- BA-40 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ba40_restated():
    n, ei, links = _ba40()  # an edge, a non-edge, u == v, isolated nodes, negative ids
    return {(h, mask): sr.restate(n, ei, links, h, mask_target=mask) for h in (1, 2, 3) for mask in (False, True)}


@pytest.mark.parametrize('label', LABELS)
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_ba40(ssa, dev, ba40_restated, h, mask, label):
    n, ei, links = _ba40()
    eh = _eh(ssa, h)
    for md in (1000, 3):
        _same(_run(eh, n, ei, links, dev, mask_target=mask, node_label=label, max_dist=md), ba40_restated[h, mask], label, md)


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_ba40_labels_equal_the_reference(ssa, dev, h, mask):
    g17 = load_golden('g17_seal_labels.npz')
    n, ei, _ = _ba40()
    links, key = g17[f'links_m{int(mask)}'], f'h{h}_m{int(mask)}'
    eh = _eh(ssa, h)
    for md in g17['max_dists']:
        for label, name in GOLDEN_LABELS.items():
            got = _run(eh, n, ei, links, dev, check_nodes=False, mask_target=mask, node_label=label, max_dist=int(md))
            np.testing.assert_array_equal(got['rowptr'], g17[key + '_rowptr'])
            np.testing.assert_array_equal(got['ids'], g17[key + '_ids'])
            np.testing.assert_array_equal(got['z'], g17[f'{key}_d{int(md)}_{name}'], err_msg=f'{label} max_dist {md}')


def test_ids_do_not_depend_on_mask_target(ssa, dev):
    n, ei, _ = _ba40()
    links = ei[:, :60].T
    for h in (1, 2, 3):
        eh = _eh(ssa, h)
        plain, masked = (_run(eh, n, ei, links, dev, mask_target=m, node_label=None) for m in (False, True))
        np.testing.assert_array_equal(plain['rowptr'], masked['rowptr'])
        np.testing.assert_array_equal(plain['ids'], masked['ids'])
        assert (plain['dist'] != masked['dist']).any() and plain['nbr'].size == masked['nbr'].size + 2 * len(links)


# ---- invariance: 3 000 uniform nodes, 512 random links + 64 edges -------------------------------------------------------------------
@pytest.fixture(scope='module')
def uniform3000():
    n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
    e = np.random.RandomState(seed).randint(0, n, size=(2, e_und)).astype(np.int64)
    ei = np.concatenate([e, e[::-1]], axis=1)
    rng = np.random.RandomState(31)
    links = np.concatenate([rng.randint(0, n, size=(512, 2)), ei[:, rng.randint(0, ei.shape[1], size=64)].T]).astype(np.int64)
    sub = sr.restate(n, ei, links, 2, mask_target=True)
    want = dict({k: getattr(sub, k) for k in FIELDS}, z=sr.labels(sub, 'drnl', 1000))
    return n, ei, links, sub, want


def _row_fields(got, q):
    a, b = got['rowptr'][q], got['rowptr'][q + 1]
    e0, e1 = got['adj_ptr'][a], got['adj_ptr'][b]
    return (got['ids'][a:b], got['dist'][a:b], got['roots'][q], got['adj_ptr'][a:b + 1] - e0, got['nbr'][e0:e1], got['weight'][e0:e1],
            got['z'][a:b])


def test_rows_do_not_depend_on_batching_or_order(ssa, dev, uniform3000):
    n, ei, links, _, want = uniform3000
    eh = _eh(ssa, 2)
    whole = _run(eh, n, ei, links, dev, batch_size=11000000)
    _same(whole, want)
    _same(_run(eh, n, ei, links, dev, batch_size=37), want)
    perm = np.random.RandomState(5).permutation(len(links))
    shuffled = _run(eh, n, ei, links[perm], dev, batch_size=100)
    for place, q in enumerate(perm):
        for g, w in zip(_row_fields(shuffled, place), _row_fields(whole, q)):
            np.testing.assert_array_equal(g, w)


# ---- both tiers (of the node list and of the label kernel) ----------------------------------------------------------------------------
@pytest.mark.parametrize('label', ['drnl', 'de'])
def test_both_tiers_give_the_same_rows(ssa, dev, lds_limit, label):
    n, ei, links = _stars()  # unions of 2 502 - 4 003 nodes (large tier, labels in the device workspace) and of 1 501 (on chip)
    sub = sr.restate(n, ei, links, 2, mask_target=True)
    sizes = np.diff(sub.rowptr)
    assert sizes.max() > 2048 and ((sizes > 1) & (sizes <= 2048)).any()
    eh = _eh(ssa, 2)
    first = _run(eh, n, ei, links, dev, node_label=label, return_info=True)  # the default on-chip capacity
    assert first['info']['lds_links'] > 0 and first['info']['large_links'] > 0 and _arena_is_zero(ssa)
    _same(first, sub, label)
    lds_limit(1)                                                             # everything in the large tier / the workspace
    second = _run(eh, n, ei, links, dev, node_label=label, return_info=True)
    assert second['info']['lds_links'] == 0 and _arena_is_zero(ssa)
    _same(second, sub, label)
    lds_limit(1501)                                                          # the limit equal to a union: still on chip
    third = _run(eh, n, ei, links, dev, node_label=label, return_info=True)
    assert third['info']['lds_links'] > 0 and _arena_is_zero(ssa)
    _same(third, sub, label)


@pytest.mark.parametrize('limit', [0, 17, 100])
def test_small_on_chip_limits(ssa, dev, lds_limit, uniform3000, limit):
    n, ei, links, _, want = uniform3000
    lds_limit(limit)
    got = _run(_eh(ssa, 2), n, ei, links, dev, return_info=True)
    _same(got, want)
    assert got['info']['large_links'] == int((np.diff(want['rowptr']) > limit).sum()) > 0 and _arena_is_zero(ssa)


# ---- both intersection directions --------------------------------------------------------------------------------------------------------
def _hub():
    """centre 0 with leaves 1 .. 3000; 3001 hangs on the centre and on 3003, 3002 on 3004, so the h = 1 union of (3001, 3002) has five
    nodes and reaches the centre (3 001 in-arcs) at its last level; (0, 5) is the centre's own link (3 002 nodes, leaves of degree 1)"""
    a = np.arange(1, 3001)
    src = np.concatenate([np.zeros_like(a), [0, 3001, 3002]])
    dst = np.concatenate([a, [3001, 3003, 3004]])
    ei = np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]).astype(np.int64)
    return 3006, ei, np.array([[3001, 3002], [0, 5], [3001, 0], [3005, 3001], [7, 9]], dtype=np.int64)


@pytest.fixture(scope='module')
def hub_restated():
    n, ei, links = _hub()
    subs = {h: sr.restate(n, ei, links, h, mask_target=True) for h in (1, 2)}
    np.testing.assert_array_equal(subs[1].row(0)[0], [0, 3001, 3002, 3003, 3004])
    return subs, {(h, label): sr.labels(subs[h], label, 1000) for h in (1, 2) for label in ('drnl', 'de+')}


@pytest.mark.parametrize('switch', [None, 0, (1 << 31) - 1])
def test_both_intersection_directions(ssa, dev, adj_switch, hub_restated, switch):
    n, ei, links = _hub()
    subs, z = hub_restated
    if switch is not None:
        adj_switch(switch)  # 0: every node walks the id row; 2^31 - 1: every node walks its arcs
    for (h, label), want in z.items():
        _same(_run(_eh(ssa, h), n, ei, links, dev, node_label=label), dict({k: getattr(subs[h], k) for k in FIELDS}, z=want), label)
    n, ei, links = _multigraph()  # (runs of equal arcs through both directions)
    _same(_run(_eh(ssa, 2), n, ei, links, dev, mask_target=False), sr.restate(n, ei, links, 2, mask_target=False))


# ---- multigraph, self loops, masking, u == v ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_multigraph_self_loops_and_masking(ssa, dev, h, mask):
    n, ei, links = _multigraph()  # arcs repeated 1, 2, 3 and 5 times, self loops on a root and inside, edge / non-edge / repeated-edge links, u == v
    sub = sr.restate(n, ei, links, h, mask_target=mask)
    assert {1, 2, 5} <= set(sub.weight.tolist())
    eh = _eh(ssa, h)
    for label in ('drnl', 'de', 'de+'):
        _same(_run(eh, n, ei, links, dev, mask_target=mask, node_label=label), sub, label)


# ---- reachability ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_dist', [1, 3, 1000])
def test_unreachable_roots_and_the_path_example(ssa, dev, max_dist):
    for (n, ei, links), h in ((_two_components(), 2), (_path(), 1)):
        sub = sr.restate(n, ei, links, h, mask_target=True)
        for label in ('drnl', 'de', 'de+'):
            _same(_run(_eh(ssa, h), n, ei, links, dev, node_label=label, max_dist=max_dist), sub, label, max_dist)
    n, ei, links = _two_components()
    got = _run(_eh(ssa, 2), n, ei, links, dev, node_label='de', max_dist=max_dist)
    np.testing.assert_array_equal(got['z'][:6], np.minimum([[0, 1000], [1, 1000], [1, 1000], [1000, 0], [1000, 1], [1000, 1]], max_dist))
    if max_dist == 1000:
        n, ei, links = _path()
        eh = _eh(ssa, 1)
        assert _run(eh, n, ei, links, dev, node_label='de')['z'][3].tolist() == [3, 1]
        assert _run(eh, n, ei, links, dev, node_label='de+')['z'][3].tolist() == [1000, 1]
        assert _run(eh, n, ei, links, dev, node_label='drnl')['z'][3] == 250002


# ---- max_nodes ----------------------------------------------------------------------------------------------------------------------------
def test_max_nodes(ssa, dev, uniform3000):
    n, ei, links, full, _ = uniform3000
    sizes = np.diff(full.rowptr)
    eh = _eh(ssa, 2)
    for cap in (int(np.median(sizes)), int(sizes.max()), 1):
        got = _run(eh, n, ei, links, dev, max_nodes=cap, return_info=True)
        over = sizes > cap
        np.testing.assert_array_equal(got['info']['truncated'].cpu().numpy(), np.nonzero(over)[0])
        assert (np.diff(got['rowptr'])[over] == 0).all() and (got['roots'][over] == -1).all() and (got['roots'][~over] >= 0).all()
        assert got['ids'].size == sizes[~over].sum() == got['z'].size and got['adj_ptr'].size == got['ids'].size + 1
        want = {k: getattr(full, k) for k in FIELDS}
        want['z'] = sr.labels(full, 'drnl', 1000)
        for q in np.nonzero(~over)[0]:
            for g, w in zip(_row_fields(got, q), _row_fields(want, q)):
                np.testing.assert_array_equal(g, w)
        assert got['nbr'].size == got['adj_ptr'][-1] == sum(_row_fields(want, q)[4].size for q in np.nonzero(~over)[0])


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------
def test_no_links(ssa, dev):
    n, ei, _ = _uniform300()
    got = _run(_eh(ssa, 2), n, ei, np.zeros((0, 2), dtype=np.int64), dev, node_label='de')
    assert got['rowptr'].tolist() == [0] and got['adj_ptr'].tolist() == [0] and got['z'].shape == (0, 2) and got['roots'].shape == (0, 2)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_no_edges(ssa, dev, h):
    links = np.array([[0, 1], [4, 4], [-1, 2], [3, 0]], dtype=np.int64)
    got = _run(_eh(ssa, h), 5, np.zeros((2, 0), dtype=np.int64), links, dev, node_label='de', max_dist=9)
    np.testing.assert_array_equal(got['ids'], [0, 1, 4, 2, 4, 0, 3])
    np.testing.assert_array_equal(got['roots'], [[0, 1], [0, 0], [1, 0], [1, 0]])
    assert got['nbr'].size == 0 and not got['adj_ptr'].any()
    np.testing.assert_array_equal(got['z'], [[0, 9], [9, 0], [0, 0], [9, 0], [0, 9], [9, 0], [0, 9]])


def test_cpu_inputs_give_cpu_outputs(ssa, dev):
    n, ei, links = _uniform300()
    eh = _eh(ssa, 2)
    sg = eh.exact_subgraphs(torch.from_numpy(links), n, torch.from_numpy(ei), max_nodes=40, node_label='de+', return_info=True)
    assert all(getattr(sg, k).device.type == 'cpu' for k in FIELDS + ('z',)) and sg.info['truncated'].device.type == 'cpu'
    want = _run(eh, n, ei, links, dev, max_nodes=40, node_label='de+')
    for k in FIELDS + ('z',):
        np.testing.assert_array_equal(getattr(sg, k).numpy(), want[k], err_msg=k)
    one = eh.exact_subgraphs(torch.tensor([3, 9]), n, torch.from_numpy(ei).to(dev))  # a [2] link; links decide where results go
    assert one.rowptr.device.type == 'cpu' and one.rowptr.shape == (2,) and one.z.device.type == 'cpu'


@pytest.mark.parametrize('mask', [False, True])
def test_directed_edge_index_follows_in_arcs(ssa, dev, mask):
    n, ei, links = _uniform300(directed=True)
    for h in (1, 2, 3):
        sub = sr.restate(n, ei, links, h, mask_target=mask)
        for label in ('drnl', 'de'):
            _same(_run(_eh(ssa, h), n, ei, links, dev, mask_target=mask, node_label=label), sub, label)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def test_helpers(ssa, dev):
    n, ei, links = _multigraph()
    got = _run(_eh(ssa, 2), n, ei, links, dev, node_label='de')
    sg = got['sg']
    owner = np.repeat(np.arange(len(links)), np.diff(got['rowptr']))
    np.testing.assert_array_equal(sg.batch().cpu().numpy(), owner)
    target = np.repeat(np.arange(got['ids'].size), np.diff(got['adj_ptr']))
    source = got['rowptr'][owner[target]] + got['nbr']
    edge_index = sg.edge_index()
    assert edge_index.dtype == torch.int64 and edge_index.device == dev
    np.testing.assert_array_equal(edge_index.cpu().numpy(), np.stack([source, target]))
    arcs = set(zip(ei[0].tolist(), ei[1].tolist()))  # every listed arc is an arc of the graph between two nodes of one link
    assert all((got['ids'][s], got['ids'][t]) in arcs and owner[s] == owner[t] for s, t in zip(source.tolist(), target.tolist()))
    for q in (0, 5, len(links) - 1):
        view = sg.link(q)
        for g, w in zip((view['ids'], view['dist'], view['roots'], view['adj_ptr'], view['nbr'], view['weight'], view['z']), _row_fields(got, q)):
            np.testing.assert_array_equal(g.cpu().numpy(), w)
