"""Connected components and induced subgraphs on the GPU (csrc/ss_components.hip, components.py) against the numpy / scipy
restatement (components_restatement.py) and, for the fixture graphs, against the reference's own largest component
(tests/golden/g19_lcc.npz).  "Equal" is exact integer equality of whole arrays: labels, roots, sizes, largest(), and the nodes, mapper,
edge_index and edge_ids of largest_component_subgraph.  The shapes are the smallest at which the kernels can still go wrong: deep chains
(a path of 4 096 nodes in four listings), one contended root (a star), all-distinct and all-equal labels inside a wavefront (matchings, a
giant component), several workgroups of the count / fill passes (N = 50 000 against chunks of 2 048), ties for the largest size.
Six graphs come from components_planted.py (tests/test_components_planted_host.py pins what they reach): `late giant`, whose largest
root lies behind 3 chunks + 191 isolated nodes at lane 63; `tie across workgroups` and `tie in one wavefront`, two paths of 777 nodes
whose roots sit in chunks 5 and 17, or at lanes 62 and 63 of one wavefront, the path with the larger ids listed first; `stride random`,
`stride random shuffled` and `stride path`, 1 100 000 nodes with 1 400 000 and 1 099 999 arcs: more than the 4 096 x 256 items one trip
of the grid-stride launches (init, hook, flatten) covers -- the shuffled arcs past the cap carry edges the first trip has not seen, the
path is a deep chain that crosses every stride boundary."""
import functools
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import components_planted as planted
import components_restatement as restated

pytestmark = pytest.mark.gpu

G19 = load_golden('g19_lcc.npz')
FIXTURE = [(int(G19[f'g{k}_num_nodes']), G19[f'g{k}_edge_index'], G19[f'g{k}_lcc']) for k in range(int(G19['num_graphs']))]


def _clique(nodes):
    a, b = np.meshgrid(nodes, nodes)
    return np.stack([a[a != b], b[a != b]])


def _path(order, n=4096):
    """the path 0 - 1 - ... - n-1 with its n - 1 edges listed in `order`"""
    rng = np.random.default_rng(41)
    lo = np.arange(n - 1, dtype=np.int64)
    if order == 'descending':
        lo = lo[::-1].copy()
    elif order in ('shuffled', 'relabelled'):
        lo = lo[rng.permutation(n - 1)]
    e = np.stack([lo, lo + 1])
    if order == 'relabelled':  # the node ids themselves permuted: the chain jumps all over the id range
        e = rng.permutation(n)[e]
    return n, e


def _star(centre, n=3000):
    leaves = np.array([x for x in range(n) if x != centre], dtype=np.int64)
    return n, np.stack([leaves, np.full(n - 1, centre, dtype=np.int64)])


def _cliques(count, size=9, n=64):
    """`count` disjoint cliques of one size; the clique that holds the smallest id comes LAST in edge order"""
    starts = [40, 22, 5][3 - count:]
    return n, np.concatenate([_clique(np.arange(s, s + size, dtype=np.int64)) for s in starts], axis=1)


GRAPHS = {
    'one node': lambda: (1, np.zeros((2, 0), dtype=np.int64)),
    'five nodes, no edge': lambda: (5, np.zeros((2, 0), dtype=np.int64)),
    'only self-loops': lambda: (7, np.array([[3, 3, 6, 0], [3, 3, 6, 0]], dtype=np.int64)),
    'one edge 1000 times': lambda: (10, np.tile(np.array([[7], [2]], dtype=np.int64), (1, 1000))),
    'one direction only': lambda: (9, np.array([[8, 7, 6, 2], [7, 6, 5, 1]], dtype=np.int64)),  # 8 -> 7 -> 6 -> 5 and 2 -> 1: weak components
    'negative ids': lambda: (12, np.array([[-1, 3, -12, 5], [3, -8, 11, 5]], dtype=np.int64)),
    'path ascending': lambda: _path('ascending'),
    'path descending': lambda: _path('descending'),
    'path shuffled': lambda: _path('shuffled'),
    'path relabelled': lambda: _path('relabelled'),
    'star centre 0': lambda: _star(0),
    'star centre 2999': lambda: _star(2999),
    'matching far': lambda: (100000, np.stack([np.arange(50000, dtype=np.int64), np.arange(50000, dtype=np.int64) + 50000])),
    'matching adjacent': lambda: (100000, np.stack([np.arange(0, 100000, 2, dtype=np.int64), np.arange(0, 100000, 2, dtype=np.int64) + 1])),
    'sparse 50000': lambda: (50000, restated.symmetric_random_graph(50000, 30000, 7)),
    'giant 50000': lambda: (50000, restated.symmetric_random_graph(50000, 200000, 8)),
    'two cliques': lambda: _cliques(2),
    'three cliques': lambda: _cliques(3),
}
GRAPHS.update({f'fixture {k}': (lambda k=k: FIXTURE[k][:2]) for k in range(len(FIXTURE))})
GRAPHS.update(planted.API_GRAPHS)


@functools.lru_cache(maxsize=None)
def graph(name):
    n, ei = GRAPHS[name]()
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    ei.setflags(write=False)
    return n, ei


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement's answers for a graph, computed once and shared (read only)"""
    n, ei = graph(name)
    lab = restated.labels(n, ei)
    roots, sizes = restated.roots_and_sizes(lab)
    out = dict(labels=lab, roots=roots, sizes=sizes, largest=restated.largest(lab))
    out['nodes'], out['mapper'], out['edge_index'], out['edge_ids'] = restated.largest_component_subgraph(n, ei)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _same(got, expected, where, what):
    assert got.dtype == torch.int64 and got.device == where, what
    assert tuple(got.shape) == expected.shape, (what, tuple(got.shape), expected.shape)
    np.testing.assert_array_equal(got.cpu().numpy(), expected, err_msg=what)


def _check_components(cc, w, where):
    for field in ('labels', 'roots', 'sizes'):
        _same(getattr(cc, field), w[field], where, field)
    assert cc.num_components == len(w['roots'])
    _same(cc.largest(), w['largest'], where, 'largest()')


def _check_subgraph(sub, w, where):
    for field in ('nodes', 'mapper', 'edge_index', 'edge_ids'):
        _same(getattr(sub, field), w[field], where, field)
    assert sub.num_nodes == len(w['nodes']) and sub.num_edges == len(w['edge_ids'])


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_components_and_largest_subgraph_equal_the_restatement(ssa, dev, name):
    n, ei = graph(name)
    w = want(name)
    t = torch.from_numpy(ei.copy()).to(dev)
    cc = ssa.connected_components(n, t)
    _check_components(cc, w, t.device)
    _check_subgraph(ssa.largest_component_subgraph(n, t), w, t.device)
    _check_subgraph(cc.subgraph(t), w, t.device)
    cc.check_errors()


@pytest.mark.parametrize('k', range(len(FIXTURE)))
def test_the_largest_component_is_the_reference_s(ssa, dev, k):
    n, ei, best = FIXTURE[k]
    t = torch.from_numpy(ei.copy()).to(dev)
    _same(ssa.connected_components(n, t).largest(), best, t.device, 'largest()')
    sub = ssa.largest_component_subgraph(n, t)
    _same(sub.nodes, best, t.device, 'nodes')
    inside = np.isin(ei[0], best) & np.isin(ei[1], best)  # the filter of use_lcc
    _same(sub.edge_ids, np.flatnonzero(inside), t.device, 'edge_ids')
    _same(sub.nodes[sub.edge_index], ei[:, inside], t.device, 'the kept edges in old ids')


def test_the_tie_rule_is_tested_by_the_clique_graphs():
    for name, count in (('two cliques', 2), ('three cliques', 3)):
        n, ei = graph(name)
        w = want(name)
        assert restated.tied(w['labels']) == count and w['largest'][0] == 5 and ei[0, 0] != 5  # smallest root, not first in edge order


def test_results_live_on_the_edge_index_s_device(ssa, dev):
    n, ei = graph('fixture 5')
    w = want('fixture 5')
    cpu = torch.device('cpu')
    cc = ssa.connected_components(n, torch.from_numpy(ei.copy()))  # a CPU edge_index: computed on the device, returned on the CPU
    _check_components(cc, w, cpu)
    _check_subgraph(ssa.largest_component_subgraph(n, torch.from_numpy(ei.copy())), w, cpu)
    _check_subgraph(ssa.largest_component_subgraph(n, torch.from_numpy(ei.astype(np.int32)).to(dev)), w, dev)  # any integer dtype


def test_labels_do_not_depend_on_order_direction_or_the_run(ssa, dev):
    n, ei = graph('sparse 50000')
    w = want('sparse 50000')
    rng = np.random.default_rng(5)
    flip = rng.random(ei.shape[1]) < 0.5
    variants = [ei, ei[:, rng.permutation(ei.shape[1])], np.where(flip, ei[::-1], ei)]
    for v in variants:
        t = torch.from_numpy(np.array(v)).to(dev)
        for _ in range(3):
            _same(ssa.connected_components(n, t).labels, w['labels'], dev, 'labels')


def _check_induced(sub, n, ei, where, nodes=None, mask=None):
    expected = dict(zip(('nodes', 'mapper', 'edge_index', 'edge_ids'), restated.induced(n, ei, nodes=nodes, mask=mask)))
    _check_subgraph(sub, expected, where)
    ids, mapper = sub.edge_ids.cpu().numpy(), sub.mapper.cpu().numpy()
    assert np.all(np.diff(ids) > 0)
    np.testing.assert_array_equal(sub.edge_index.cpu().numpy(), mapper[restated.wrapped(n, ei)[:, ids]])


@pytest.mark.parametrize('name', ['fixture 5', 'giant 50000'])
def test_induced_subgraph(ssa, dev, name):
    n, ei = graph(name)
    t = torch.from_numpy(ei.copy()).to(dev)
    rng = np.random.default_rng(9)
    masks = {'nothing': np.zeros(n, dtype=bool), 'everything': np.ones(n, dtype=bool), 'half': rng.random(n) < 0.5,
             'one chunk': (np.arange(n) >= n // 3) & (np.arange(n) < n // 3 + 1500)}
    for what, mask in masks.items():
        _check_induced(ssa.induced_subgraph(n, t, mask=torch.from_numpy(mask).to(dev)), n, ei, dev, mask=mask)
    if name == 'giant 50000':  # the kept edges cross several workgroups of the fill pass
        assert ssa.induced_subgraph(n, t, mask=torch.from_numpy(masks['half']).to(dev)).num_edges > 20 * ssa._native.COMPONENTS_CHUNK
    some = rng.permutation(n)[:(2 * n) // 3].astype(np.int64)
    lists = {'descending': np.sort(some)[::-1].copy(), 'random': some, 'negative ids': some - n * (np.arange(len(some)) % 2),
             'empty': np.zeros(0, dtype=np.int64)}
    for what, nodes in lists.items():
        _check_induced(ssa.induced_subgraph(n, t, nodes=torch.from_numpy(nodes).to(dev)), n, ei, dev, nodes=nodes)
    _check_induced(ssa.induced_subgraph(n, torch.from_numpy(ei.copy()), nodes=lists['random'].tolist()), n, ei, torch.device('cpu'), nodes=lists['random'])


def test_a_device_node_list_is_checked_on_the_device(ssa, dev):
    n, ei = graph('fixture 5')
    t = torch.from_numpy(ei.copy()).to(dev)
    with pytest.raises(ValueError):
        ssa.induced_subgraph(n, t, nodes=torch.tensor([4, 9, 4 - n], device=dev))  # 4 twice, once as a negative id
    with pytest.raises(IndexError):
        ssa.induced_subgraph(n, t, nodes=torch.tensor([4, n], device=dev))


def test_same_equals_the_label_comparison(ssa, dev):
    n, ei = graph('sparse 50000')
    lab = want('sparse 50000')['labels']
    rng = np.random.default_rng(2)
    links = np.concatenate([rng.integers(-n, n, size=(3000, 2)), ei.T[:1000], np.stack([np.arange(50), np.arange(50)], axis=1)])
    cc = ssa.connected_components(n, torch.from_numpy(ei.copy()).to(dev))
    expected = lab[links[:, 0] % n] == lab[links[:, 1] % n]
    assert expected[:3000].any() and not expected[:3000].all() and expected[3000:].all()  # links inside and across components
    for where in (dev, torch.device('cpu')):
        got = cc.same(torch.from_numpy(links).to(where))
        assert got.dtype == torch.bool and got.device == where
        np.testing.assert_array_equal(got.cpu().numpy(), expected)
    assert cc.same(torch.zeros((0, 2), dtype=torch.int64, device=dev)).shape == (0,)
    with pytest.raises(IndexError):
        cc.same(torch.tensor([[0, n]]))
    cc.check_errors()


def test_a_device_id_out_of_range_is_reported_late_and_its_edge_ignored(ssa, dev):
    n, ei = graph('fixture 4')
    bad = np.concatenate([ei[:, :50], np.array([[3], [n]], dtype=np.int64), ei[:, 50:]], axis=1)  # one id >= N among good ones
    w = want('fixture 4')
    t = torch.from_numpy(bad).to(dev)
    cc = ssa.connected_components(n, t)
    _same(cc.labels, w['labels'], dev, 'labels without the bad edge')
    _same(cc.roots, w['roots'], dev, 'roots')
    _same(cc.sizes, w['sizes'], dev, 'sizes')
    with pytest.raises(IndexError):
        cc.check_errors()
    cc.check_errors()  # reported once
    again = ssa.connected_components(n, t)
    with pytest.raises(IndexError):  # ... or by the next call on the result
        again.largest()
    _same(again.largest(), w['largest'], dev, 'largest()')
    sub = ssa.induced_subgraph(n, t, mask=torch.ones(n, dtype=torch.bool, device=dev))
    _same(sub.edge_ids, np.delete(np.arange(bad.shape[1]), 50), dev, 'edge_ids without the bad edge')
    with pytest.raises(IndexError):
        sub.check_errors()


def test_the_integration_shim_on_a_duck_typed_dataset(ssa, dev):
    spec = importlib.util.spec_from_file_location('ssa_integration_lcc', os.path.join(REPO, 'integration', 'src', 'lcc.py'))
    lcc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lcc)
    for n, ei, best in FIXTURE[:2] + FIXTURE[5:]:
        ds = types.SimpleNamespace(data=types.SimpleNamespace(x=torch.zeros((n, 3)), edge_index=torch.from_numpy(ei.copy())))
        got = lcc.get_largest_connected_component(ds)
        assert isinstance(got, np.ndarray) and np.array_equal(got, best)
        assert lcc.get_component(ds, int(best[-1])) == set(best.tolist())
        inside = np.isin(ei[0], best) & np.isin(ei[1], best)
        row, col = lcc.remap_edges([[i, j] for i, j in ei[:, inside].T.tolist()], lcc.get_node_mapper(got))
        sub = ssa.largest_component_subgraph(n, ds.data.edge_index)
        assert [row, col] == sub.edge_index.tolist()
