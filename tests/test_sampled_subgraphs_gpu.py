"""ElphHashes.sampled_subgraph_nodes (sampled_nodes.py, csrc/ss_sampled_nodes.hip) and exact_subgraphs(max_nodes_per_hop=, ratio_per_hop=,
seed=) on the GPU: rowptr, ids and hop -- and through exact_subgraphs every field -- must EQUAL the Python-set restatement
(tests/sampled_subgraph_restatement.py): on BA-40 over hops, caps, ratios, seeds, labels and masking; on a 3 000-node uniform graph under
batching, shuffling and duplicated links; on two stars through either kernel tier (fringes of thousands for a cap of 100, the arena all
zero afterwards); batches, max_nodes and both tiers in one call; at the selection boundaries; on the star of the sampling law; on K_8 with tails; under max_nodes; and on the edge cases
(no links, no edges, CPU inputs, a directed edge_index).  With the default keywords exact_subgraphs is what it was."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import sampled_subgraph_restatement as ssr
import subgraph_restatement as sr
from conftest import load_golden
from test_exact_nodes_gpu import _arena_is_zero, _hub60
from test_exact_nodes_host import _ba40, _uniform300
from test_sampled_subgraphs_host import STAR_SEED, k8_with_tails, star

pytestmark = pytest.mark.gpu
LABELS = ('drnl', 'de', 'de+', 'hop', 'zo', None)
FIELDS = ('rowptr', 'ids', 'hop', 'roots', 'adj_ptr', 'nbr', 'weight')


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
    """sets knobs.EXACT_LDS_MAX_NODES for one test and restores it"""
    old = ssa.knobs.EXACT_LDS_MAX_NODES
    yield lambda value: setattr(ssa.knobs, 'EXACT_LDS_MAX_NODES', value)
    ssa.knobs.EXACT_LDS_MAX_NODES = old


def _eh(ssa, h=2):
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))


def _nodes(eh, n, ei, links, dev, **kw):
    """one sampled_subgraph_nodes call with everything on the device -> numpy (rowptr, ids, hop[, info])"""
    out = eh.sampled_subgraph_nodes(torch.from_numpy(np.asarray(links, dtype=np.int64)).to(dev), n, torch.from_numpy(ei).to(dev), **kw)
    rowptr, ids, hop = out[:3]
    assert rowptr.device == ids.device == hop.device == dev
    assert rowptr.dtype == ids.dtype == torch.int64 and hop.dtype == torch.uint8 and hop.shape == ids.shape and rowptr.shape == (len(links) + 1,)
    return tuple(t.cpu().numpy() for t in out[:3]) + tuple(out[3:])


def _same_nodes(got, want):
    for g, w, name in zip(got, want, ('rowptr', 'ids', 'hop')):
        np.testing.assert_array_equal(g, w, err_msg=name)


def _subgraphs(ssa, eh, n, ei, links, dev, **kw):
    """one exact_subgraphs call with sampling on -> the SampledSubgraphs' fields as numpy (+ z, sg)"""
    sg = eh.exact_subgraphs(torch.from_numpy(np.asarray(links, dtype=np.int64)).to(dev), n, torch.from_numpy(ei).to(dev), **kw)
    assert type(sg) is ssa.subgraphs.SampledSubgraphs and sg.dist is None
    assert all(getattr(sg, k).device == dev for k in FIELDS) and (sg.z is None or sg.z.device == dev)
    assert sg.rowptr.dtype == sg.ids.dtype == sg.adj_ptr.dtype == torch.int64 and sg.hop.dtype == torch.uint8
    assert sg.roots.dtype == sg.nbr.dtype == sg.weight.dtype == torch.int32 and (sg.z is None or sg.z.dtype == torch.int64)
    got = {k: getattr(sg, k).cpu().numpy() for k in FIELDS}
    got['z'], got['sg'] = None if sg.z is None else sg.z.cpu().numpy(), sg
    return got


def _same(got, sub, label='drnl', max_dist=1000):
    """every field equals the restatement `sub`"""
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], getattr(sub, k), err_msg=k)
    z = ssr.labels(sub, label, max_dist)
    if z is None:
        assert got['z'] is None
    else:
        assert got['z'].shape == z.shape
        np.testing.assert_array_equal(got['z'], z, err_msg=f'z ({label}, max_dist {max_dist})')


# ---- BA-40 ------------------------------------------------------------------------------------------------------------------------------
CAPS, RATIOS, SEEDS = (1, 2, 3, 5, 1000), (1.0, 0.5, 0.34), (0, 77)
_BA40 = {}


def _ba40_restated(h, mask, cap, ratio, seed):
    """computed once per combination and shared by the label cases"""
    key = (h, mask, cap, ratio, seed)
    if key not in _BA40:
        n, ei, links = _ba40()  # an edge, a non-edge, u == v, isolated nodes, negative ids
        _BA40[key] = ssr.restate(n, ei, links, h, mask_target=mask, cap=cap, ratio=ratio, seed=seed)
    return _BA40[key]


@pytest.mark.parametrize('label', LABELS)
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_ba40(ssa, dev, h, mask, label):
    n, ei, links = _ba40()
    eh = _eh(ssa, h)
    for cap in CAPS:
        for ratio in RATIOS:
            for seed in SEEDS:
                got = _subgraphs(ssa, eh, n, ei, links, dev, mask_target=mask, node_label=label, max_nodes_per_hop=cap, ratio_per_hop=ratio, seed=seed)
                _same(got, _ba40_restated(h, mask, cap, ratio, seed), label)


def test_ba40_nodes_method_and_a_ratio_alone(ssa, dev):
    n, ei, links = _ba40()
    for h in (1, 2, 3):
        eh = _eh(ssa, h)
        for kw in (dict(cap=None, ratio=0.5, seed=3), dict(cap=2, ratio=1.0, seed=3), dict(cap=None, ratio=1.0, seed=0)):
            got = _nodes(eh, n, ei, links, dev, max_nodes_per_hop=kw['cap'], ratio_per_hop=kw['ratio'], seed=kw['seed'], return_info=True)
            want = ssr.restate_nodes(n, ei, links, h, return_info=True, **kw)
            _same_nodes(got, want)
            assert got[3]['sampled_links'] == want[3]['sampled_links'] and got[3]['lds_links'] + got[3]['large_links'] == len(links)
        sub = ssr.restate(n, ei, links, h, mask_target=True, ratio=0.5, seed=3)  # exact_subgraphs with a ratio and no cap
        _same(_subgraphs(ssa, eh, n, ei, links, dev, ratio_per_hop=0.5, seed=3, max_dist=3), sub, 'drnl', 3)


def test_unsampled_walk_equals_the_reference(ssa, dev):
    g18, g = load_golden('g18_seal_khop.npz'), load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    for h in (1, 2, 3):
        got = _nodes(_eh(ssa, h), n, ei, g18['links'], dev)
        _same_nodes(got, (g18[f'h{h}_rowptr'], g18[f'h{h}_ids'], g18[f'h{h}_hop']))


# ---- invariance: 3 000 uniform nodes, 512 random links + 64 edges -------------------------------------------------------------------
U_KW = dict(cap=10, ratio=0.5, seed=4)


@pytest.fixture(scope='module')
def uniform3000():
    n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
    e = np.random.RandomState(seed).randint(0, n, size=(2, e_und)).astype(np.int64)
    ei = np.concatenate([e, e[::-1]], axis=1)
    rng = np.random.RandomState(31)
    links = np.concatenate([rng.randint(0, n, size=(512, 2)), ei[:, rng.randint(0, ei.shape[1], size=64)].T]).astype(np.int64)
    return n, ei, links, ssr.restate(n, ei, links, 2, mask_target=True, **U_KW)


def _device_kw(kw):
    return dict(max_nodes_per_hop=kw['cap'], ratio_per_hop=kw['ratio'], seed=kw['seed'])


def _rows_of(rowptr, ids, hop, order):
    """the rows of a run, picked in `order` -> (rowptr, ids, hop)"""
    rows = ssr.rows(rowptr, ids, hop)
    rows = [rows[q] for q in order]
    return (np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64),
            np.concatenate([r[0] for r in rows] + [np.zeros((0,), np.int64)]), np.concatenate([r[1] for r in rows] + [np.zeros((0,), np.uint8)]))


def test_rows_do_not_depend_on_batching_order_or_duplicates(ssa, dev, uniform3000):
    n, ei, links, sub = uniform3000
    eh = _eh(ssa, 2)
    want = (sub.rowptr, sub.ids, sub.hop)
    whole = _nodes(eh, n, ei, links, dev, batch_size=11000000, return_info=True, **_device_kw(U_KW))
    _same_nodes(whole, want)
    assert whole[3]['sampled_links'] > 0 and whole[3]['lds_links'] == len(links)
    _same_nodes(_nodes(eh, n, ei, links, dev, batch_size=37, **_device_kw(U_KW)), want)
    perm = np.random.RandomState(5).permutation(len(links))
    _same_nodes(_nodes(eh, n, ei, links[perm], dev, batch_size=100, **_device_kw(U_KW)), _rows_of(*want, perm))
    twice = np.concatenate([np.arange(40), np.arange(40)[::-1], [7, 7, 7]])  # a link that appears twice gets the same row twice
    _same_nodes(_nodes(eh, n, ei, links[twice], dev, batch_size=50, **_device_kw(U_KW)), _rows_of(*want, twice))


def test_uniform3000_every_field(ssa, dev, uniform3000):
    n, ei, links, sub = uniform3000
    eh = _eh(ssa, 2)
    _same(_subgraphs(ssa, eh, n, ei, links, dev, **_device_kw(U_KW)), sub, 'drnl')
    got = _subgraphs(ssa, eh, n, ei, links, dev, batch_size=37, node_label='de+', **_device_kw(U_KW))
    _same(got, sub, 'de+')
    sg = got['sg']  # the helpers on a SampledSubgraphs
    q = 100
    view = sg.link(q)
    a, b = sub.rowptr[q], sub.rowptr[q + 1]
    assert set(view) == {'ids', 'hop', 'roots', 'adj_ptr', 'nbr', 'weight', 'z'}
    np.testing.assert_array_equal(view['hop'].cpu().numpy(), sub.hop[a:b])
    np.testing.assert_array_equal(view['adj_ptr'].cpu().numpy(), sub.adj_ptr[a:b + 1] - sub.adj_ptr[a])
    np.testing.assert_array_equal(sg.batch().cpu().numpy(), np.repeat(np.arange(len(links)), np.diff(sub.rowptr)))
    assert sg.edge_index().shape == (2, sub.nbr.size)
    cpu = sg.to('cpu')
    assert type(cpu) is ssa.subgraphs.SampledSubgraphs and cpu.hop.device.type == 'cpu' and cpu.dist is None


# ---- tiers: fringes far larger than what is kept -----------------------------------------------------------------------------------------
def _stars():
    """hub 0 with leaves 1 .. 2500 and a path 0 - 2501 - ... - 2508 (what a link at the hub visits passes the on-chip table's 2048 nodes,
    and the hub is walked by the whole workgroup); hub 2600 with leaves 2601 .. 4100 (a fringe of 1 500: selected on chip); 4101 isolated"""
    a = np.arange(1, 2501)
    path = np.arange(2501, 2509)
    b = np.arange(2601, 4101)
    src = np.concatenate([np.zeros_like(a), [0], path[:-1], np.full_like(b, 2600)])
    dst = np.concatenate([a, path[:1], path[1:], b])
    ei = np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]).astype(np.int64)
    return 4102, ei


STAR_CASES = {'hub_leaf_h1': (1, np.array([[0, 9], [2600, 2601], [9, 0], [0, 4101], [2600, 4101], [4101, 4101]])),
              'leaf_leaf_h2': (2, np.array([[3, 2077], [2700, 4000], [3, 4000], [2508, 1234], [2507, 2507], [2501, 2500]]))}


@pytest.fixture(scope='module')
def stars_restated():
    n, ei = _stars()
    return {name: ssr.restate_nodes(n, ei, links, h, cap=100, seed=6, return_info=True) for name, (h, links) in STAR_CASES.items()}


@pytest.mark.parametrize('limit', [None, 1, 0, 17, 100])
@pytest.mark.parametrize('case', sorted(STAR_CASES))
def test_stars_through_either_tier(ssa, dev, lds_limit, stars_restated, case, limit):
    n, ei = _stars()
    h, links = STAR_CASES[case]
    if limit is not None:
        lds_limit(limit)
    got = _nodes(_eh(ssa, h), n, ei, links, dev, max_nodes_per_hop=100, seed=6, return_info=True)
    assert _arena_is_zero(ssa)
    _same_nodes(got, stars_restated[case])
    info = got[3]
    assert info['sampled_links'] == stars_restated[case][3]['sampled_links'] > 0
    assert info['lds_links'] + info['large_links'] == len(links)
    if limit is None:
        assert info['lds_links'] > 0 and info['large_links'] > 0   # the default table: hub 0's links overflow it, hub 2600's do not
    elif limit <= 1:
        assert info['large_links'] >= len(links) - 1               # (only a lone root fits a table of one node)
    assert (np.diff(got[0]) <= 2 + h * 100).all()


def test_stars_every_field_in_the_slot_tier(ssa, dev, lds_limit):
    n, ei = _stars()
    h, links = STAR_CASES['leaf_leaf_h2']
    sub = ssr.restate(n, ei, links, h, mask_target=True, cap=100, seed=6)
    eh = _eh(ssa, h)
    _same(_subgraphs(ssa, eh, n, ei, links, dev, max_nodes_per_hop=100, seed=6), sub, 'drnl')
    lds_limit(1)
    _same(_subgraphs(ssa, eh, n, ei, links, dev, max_nodes_per_hop=100, seed=6, node_label='de'), sub, 'de')
    assert _arena_is_zero(ssa)


@pytest.mark.parametrize('h', [2, 3])
def test_batches_cap_and_both_tiers_in_one_call(ssa, dev, lds_limit, h):
    """every batch keeps its own workspace (counters and overflow list) from the count pass to the fill pass: 7 links in batches of 3, an
    on-chip limit of 16 (the four links that visit the hub's leaves pass it), 4 nodes per hop, and max_nodes at the median row length,
    which empties rows of either tier"""
    n, ei, links = _hub60()
    sizes = np.diff(ssr.restate_nodes(n, ei, links, h, cap=4)[0])
    cut = int(np.median(sizes))
    want = ssr.restate_nodes(n, ei, links, h, cap=4, max_nodes=cut, return_info=True)
    nb, visited = ssr.in_neighbours(n, ei), []
    for u, v in np.where(links < 0, links + n, links).tolist():  # what each link visits: its roots and every hop's whole fringe
        fringes = []
        ssr.walk(nb, u, v, h, cap=4, fringes=fringes)
        visited.append(2 - (u == v) + sum(F for F, _ in fringes))
    slot = np.array(visited) > 16
    gone = np.zeros(len(links), dtype=bool)
    gone[want[3]['truncated']] = True
    assert (gone & slot).any() and (gone & ~slot).any() and (~gone & slot).any() and (~gone & ~slot).any()
    lds_limit(16)
    got = _nodes(_eh(ssa, h), n, ei, links, dev, batch_size=3, max_nodes_per_hop=4, max_nodes=cut, return_info=True)
    _same_nodes(got, want)
    np.testing.assert_array_equal(got[3]['truncated'].cpu().numpy(), want[3]['truncated'])
    assert got[3]['sampled_links'] == want[3]['sampled_links'] > 0 and (got[3]['lds_links'], got[3]['large_links']) == ((~slot).sum(), slot.sum())
    assert _arena_is_zero(ssa)


@pytest.mark.parametrize('limit', [None, 1])
def test_selection_boundaries(ssa, dev, lds_limit, limit):
    """caps of F - 1, F, F + 1 and 1 on fringes of F = 1 500 (on chip by default) and F = 2 501 (the slot tier)"""
    n, ei = _stars()
    links = np.array([[2600, 4101], [0, 4101]])
    nb = ssr.in_neighbours(n, ei)
    assert len(nb[2600]) == 1500 and len(nb[0]) == 2501
    if limit is not None:
        lds_limit(limit)
    eh = _eh(ssa, 1)
    for cap in (1, 1499, 1500, 1501, 2500, 2501, 2502):
        got = _nodes(eh, n, ei, links, dev, max_nodes_per_hop=cap, seed=13, return_info=True)
        want = ssr.restate_nodes(n, ei, links, 1, cap=cap, seed=13, return_info=True)
        _same_nodes(got, want)
        assert np.diff(got[0]).tolist() == [2 + min(cap, 1500), 2 + min(cap, 2501)]
        assert got[3]['sampled_links'] == want[3]['sampled_links'] == (cap < 1500) + (cap < 2501)
    for ratio in (0.999, 0.5, 1 / 1500, 1 / 2501, 0.0003):  # floor(ratio * F), down to m == 0
        got = _nodes(eh, n, ei, links, dev, ratio_per_hop=ratio, seed=13)
        _same_nodes(got, ssr.restate_nodes(n, ei, links, 1, ratio=ratio, seed=13))
        assert np.diff(got[0]).tolist() == [2 + int(ratio * 1500), 2 + int(ratio * 2501)]
    assert _arena_is_zero(ssa)


# ---- the sampling law, K_8 with tails -------------------------------------------------------------------------------------------------------
def test_star_of_the_sampling_law(ssa, dev):
    n, ei, links = star()
    eh = _eh(ssa, 1)
    _same_nodes(_nodes(eh, n, ei, links, dev, max_nodes_per_hop=8, seed=STAR_SEED), ssr.restate_nodes(n, ei, links, 1, cap=8, seed=STAR_SEED))
    _same_nodes(_nodes(eh, n, ei, links, dev, ratio_per_hop=0.25, seed=STAR_SEED), ssr.restate_nodes(n, ei, links, 1, ratio=0.25, seed=STAR_SEED))


@pytest.mark.parametrize('h', [2, 3])
def test_k8_with_tails(ssa, dev, h):
    n, ei = k8_with_tails()
    links = np.array([[0, 1], [2, 7], [3, 3], [0, 8]])
    eh = _eh(ssa, h)
    for seed in range(4):
        _same_nodes(_nodes(eh, n, ei, links, dev, max_nodes_per_hop=2, seed=seed), ssr.restate_nodes(n, ei, links, h, cap=2, seed=seed))
    _same(_subgraphs(ssa, eh, n, ei, links, dev, max_nodes_per_hop=2, seed=1, node_label='de+'), ssr.restate(n, ei, links, h, cap=2, seed=1), 'de+')


# ---- max_nodes ------------------------------------------------------------------------------------------------------------------------
def test_max_nodes(ssa, dev, uniform3000):
    n, ei, links, sub = uniform3000
    eh = _eh(ssa, 2)
    sizes = np.diff(sub.rowptr)
    assert sizes.max() <= 2 + 2 * U_KW['cap']
    got = _nodes(eh, n, ei, links, dev, max_nodes=2 + 2 * U_KW['cap'], return_info=True, **_device_kw(U_KW))  # the longest a row can be
    assert got[3]['truncated'].numel() == 0 and got[3]['truncated'].device == dev and got[3]['truncated'].dtype == torch.int64
    _same_nodes(got, (sub.rowptr, sub.ids, sub.hop))
    got = _nodes(eh, n, ei, links, dev, max_nodes=1, return_info=True, **_device_kw(U_KW))  # only a lone root fits
    want = ssr.restate_nodes(n, ei, links, 2, max_nodes=1, return_info=True, **U_KW)
    _same_nodes(got, want)
    np.testing.assert_array_equal(got[3]['truncated'].cpu().numpy(), want[3]['truncated'])
    assert 0 < want[3]['truncated'].size == (sizes > 1).sum()
    cut = int(np.median(sizes))
    full = _subgraphs(ssa, eh, n, ei, links, dev, max_nodes=cut, return_info=True, **_device_kw(U_KW))
    _same(full, ssr.restate(n, ei, links, 2, max_nodes=cut, **U_KW), 'drnl')
    np.testing.assert_array_equal(full['sg'].info['truncated'].cpu().numpy(), np.nonzero(sizes > cut)[0])
    assert (full['roots'][sizes > cut] == -1).all()


# ---- edge cases -------------------------------------------------------------------------------------------------------------------------
def test_no_links(ssa, dev):
    n, ei, _ = _uniform300()
    rowptr, ids, hop = _nodes(_eh(ssa, 2), n, ei, np.zeros((0, 2), dtype=np.int64), dev, max_nodes_per_hop=3)
    assert rowptr.tolist() == [0] and ids.size == 0 and hop.shape == (0,)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_no_edges(ssa, dev, h):
    links = np.array([[0, 1], [4, 4], [-1, 2], [3, 0]], dtype=np.int64)
    rowptr, ids, hop, info = _nodes(_eh(ssa, h), 5, np.zeros((2, 0), dtype=np.int64), links, dev, max_nodes_per_hop=1, ratio_per_hop=0.5,
                                    return_info=True)
    np.testing.assert_array_equal(rowptr, [0, 2, 3, 5, 7])
    np.testing.assert_array_equal(ids, [0, 1, 4, 2, 4, 0, 3])
    assert not hop.any() and info['sampled_links'] == 0


def test_cpu_inputs_give_cpu_outputs(ssa, dev):
    n, ei, links = _uniform300()
    eh = _eh(ssa, 2)
    kw = dict(max_nodes_per_hop=4, ratio_per_hop=0.8, seed=2, max_nodes=9, return_info=True)
    out = eh.sampled_subgraph_nodes(torch.from_numpy(links), n, torch.from_numpy(ei), **kw)
    assert all(t.device.type == 'cpu' for t in out[:3]) and out[3]['truncated'].device.type == 'cpu'
    want = ssr.restate_nodes(n, ei, links, 2, cap=4, ratio=0.8, seed=2, max_nodes=9, return_info=True)
    _same_nodes(tuple(t.numpy() for t in out[:3]), want)
    np.testing.assert_array_equal(out[3]['truncated'].numpy(), want[3]['truncated'])
    _same_nodes(_nodes(eh, n, ei, links, dev, **kw), want)
    one = eh.sampled_subgraph_nodes(torch.tensor([3, 9]), n, torch.from_numpy(ei).to(dev), max_nodes_per_hop=2)  # a [2] link
    assert one[0].device.type == 'cpu' and one[0].shape == (2,)
    sg = eh.exact_subgraphs(torch.from_numpy(links), n, torch.from_numpy(ei), max_nodes_per_hop=4, ratio_per_hop=0.8, seed=2)
    assert type(sg) is ssa.subgraphs.SampledSubgraphs and sg.hop.device.type == sg.z.device.type == 'cpu'
    sub = ssr.restate(n, ei, links, 2, cap=4, ratio=0.8, seed=2)
    _same(dict({k: getattr(sg, k).numpy() for k in FIELDS}, z=sg.z.numpy()), sub, 'drnl')


def test_directed_edge_index_follows_in_edges(ssa, dev):
    n, ei, links = _uniform300(directed=True)  # (with duplicate arcs, self loops, u == v and negative ids)
    for h in (1, 2, 3):
        eh = _eh(ssa, h)
        _same_nodes(_nodes(eh, n, ei, links, dev, max_nodes_per_hop=3, ratio_per_hop=0.9, seed=8),
                    ssr.restate_nodes(n, ei, links, h, cap=3, ratio=0.9, seed=8))
        for mask in (False, True):
            sub = ssr.restate(n, ei, links, h, mask_target=mask, cap=3, ratio=0.9, seed=8)
            _same(_subgraphs(ssa, eh, n, ei, links, dev, mask_target=mask, max_nodes_per_hop=3, ratio_per_hop=0.9, seed=8, node_label='de'), sub, 'de')


# ---- the seed -----------------------------------------------------------------------------------------------------------------------------
def test_the_seed_decides_the_rows(ssa, dev):
    n, ei = _stars()
    links = np.array([[0, 9], [2600, 2601]])
    eh = _eh(ssa, 1)
    first = _nodes(eh, n, ei, links, dev, max_nodes_per_hop=100, seed=1)
    _same_nodes(_nodes(eh, n, ei, links, dev, max_nodes_per_hop=100, seed=1), first)
    other = _nodes(eh, n, ei, links, dev, max_nodes_per_hop=100, seed=2)
    np.testing.assert_array_equal(other[0], first[0])
    for (a, _), (b, _) in zip(ssr.rows(*first), ssr.rows(*other)):
        assert not np.array_equal(a, b)


# ---- the default keywords: exact_subgraphs as it was ----------------------------------------------------------------------------------
@pytest.mark.parametrize('label', ['drnl', 'hop'])
def test_default_keywords_change_nothing(ssa, dev, label):
    n, ei, links = _ba40()
    ld, ed = torch.from_numpy(links).to(dev), torch.from_numpy(ei).to(dev)
    for h in (1, 2, 3):
        eh = _eh(ssa, h)
        for sg in (eh.exact_subgraphs(ld, n, ed, node_label=label, return_info=True),
                   eh.exact_subgraphs(ld, n, ed, node_label=label, return_info=True, max_nodes_per_hop=None, ratio_per_hop=1.0, seed=5)):
            assert type(sg) is ssa.subgraphs.ExactSubgraphs and not hasattr(sg, 'hop') and set(sg.info) == {'truncated', 'lds_links', 'large_links'}
            want = sr.restate(n, ei, links, h, mask_target=True)
            for k in ('rowptr', 'ids', 'dist', 'roots', 'adj_ptr', 'nbr', 'weight'):
                np.testing.assert_array_equal(getattr(sg, k).cpu().numpy(), getattr(want, k), err_msg=k)
            np.testing.assert_array_equal(sg.z.cpu().numpy(), sr.labels(want, label))
            nodes = eh.exact_subgraph_nodes(ld, n, ed, mask_target=True)
            assert all(torch.equal(getattr(sg, k), w) for k, w in zip(('rowptr', 'ids', 'dist'), nodes))
            assert set(sg.link(0)) == {'ids', 'dist', 'roots', 'adj_ptr', 'nbr', 'weight', 'z'}
