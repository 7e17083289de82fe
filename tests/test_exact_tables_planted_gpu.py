"""The node tables of the exact kernels (csrc/ss_exact_bfs.hpp: the on-chip hash table and the large tier's level words, shared by
ss_exact.hip, ss_exact_nodes.hip and ss_sampled_nodes.hip) on PLANTED ids (tests/exact_tables_planted.py): a 26-key chain of one home
slot, a cluster that wraps from slot 4 095 to slot 0, clusters displaced by hundreds of slots, unions of exactly 2 048 and 2 049 nodes,
neighbours alone in one value word and in one level word, 16 lanes racing for one new key, frontier nodes of 512 and 513 in-arcs, a
level of 70 nodes for a 64-entry big list, the step edges of the ordered scan on N = 100 000 and N = 99 999 -- and 6 244 links through
workgroups that serve link after link, of both tiers, from one table.  Everything is integer or bit-exact: counts and node rows EQUAL the restatements,
features match bit for bit, the tier of every link (stats['overflow'], lds_links / large_links) equals the prediction from the union
sizes, and the arena's level words are zero after every large-tier call.  The planted claims themselves are pinned by
tests/test_exact_tables_planted_host.py.  What ran on an MI355X: profiles/exact_tables_planted_tests.txt."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import exact_tables_planted as planted
import sampled_subgraph_restatement as ssr
import subgraph_restatement as sr
from large_exact_helpers import arena_dist_words_are_zero

pytestmark = pytest.mark.gpu

SLOTS = 8  # knobs.EXACT_LARGE_SLOTS of this module: the arena stays at 7 MB
NODE_NAMES = ('rowptr', 'ids', 'dist')
SUBGRAPH_FIELDS = ('rowptr', 'ids', 'roots', 'adj_ptr', 'nbr', 'weight')


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
def knobs(ssa):
    """every test starts from the default on-chip limit and this module's slot count, and leaves both knobs as it found them"""
    old = ssa.knobs.EXACT_LDS_MAX_NODES, ssa.knobs.EXACT_LARGE_SLOTS
    ssa.knobs.EXACT_LDS_MAX_NODES, ssa.knobs.EXACT_LARGE_SLOTS = planted.NODE_LIMIT, SLOTS
    yield ssa.knobs
    ssa.knobs.EXACT_LDS_MAX_NODES, ssa.knobs.EXACT_LARGE_SLOTS = old


class Device(object):
    """a planted graph on the device: g, ei (one tensor, so the engine's CSR is built once), eh (max_hops is read at call time)"""


@pytest.fixture(scope='module')
def on_device(ssa, dev):
    made = {}

    def get(n=planted.N):
        if n not in made:
            d = Device()
            d.g = planted.graph(n)
            d.ei = torch.from_numpy(d.g.ei.copy()).to(dev)
            d.eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
            made[n] = d
        return made[n]

    yield get
    ssa.exact._ARENA.clear()  # (this module's 8-slot arenas)


def _dev_links(links, dev):
    return torch.from_numpy(np.array(links, dtype=np.int64)).to(dev)  # (a copy: the planted arrays are read-only)


def _features(ssa, d, dev, links, h, mask):
    """-> ((features, I, balls) as numpy, overflow: the links the on-chip tier handed to the large tier)"""
    d.eh.max_hops = h
    st = {}
    out = ssa.exact.exact_subgraph_features(d.eh, _dev_links(links, dev), d.g.n, d.ei, return_counts=True, stats=st, mask_target=mask)
    assert st['slots'] <= SLOTS
    return tuple(t.cpu().numpy() for t in out), st['overflow']


def _same_features(got, want, rows=None):
    f, I, balls = want if rows is None else [x[rows] for x in want]
    np.testing.assert_array_equal(got[1], I, err_msg='I')
    np.testing.assert_array_equal(got[2], balls, err_msg='balls')
    np.testing.assert_array_equal(got[0].view(np.int32), f.view(np.int32), err_msg='features')


def _nodes(d, dev, links, h, mask):
    """-> ((rowptr, ids, dist) as numpy, info)"""
    d.eh.max_hops = h
    out = d.eh.exact_subgraph_nodes(_dev_links(links, dev), d.g.n, d.ei, mask_target=mask, return_info=True)
    assert out[2].dtype == torch.uint8 and out[3]['truncated'].numel() == 0
    return tuple(t.cpu().numpy() for t in out[:3]), out[3]


def _sampled(d, dev, links, h, cap, ratio):
    d.eh.max_hops = h
    out = d.eh.sampled_subgraph_nodes(_dev_links(links, dev), d.g.n, d.ei, max_nodes_per_hop=cap, ratio_per_hop=ratio, seed=planted.SAMPLED_SEED,
                                      return_info=True)
    return tuple(t.cpu().numpy() for t in out[:3]), out[3]


def _same_rows(got, want, names=NODE_NAMES):
    for a, b, name in zip(got, want, names):
        np.testing.assert_array_equal(a, b, err_msg=name)


def _tiers(info, sizes, limit):
    """the node-list call's tiers against the prediction: a union (the sampled walk: a visited set) of at most `limit` stays on chip"""
    large = int((sizes > limit).sum())
    assert (info['lds_links'], info['large_links']) == (len(sizes) - large, large)


def test_engine_csr_keeps_the_planted_in_arcs(ssa, dev, on_device):
    """the row lengths of the engine's CSR are the planted in-arc counts, copies included: 512 and 513 at the boundary children, 16
    copies of every arc of the raced star, a tail's row one source 16 times"""
    d = on_device()
    csr = d.eh._csr_cache.get(d.ei, d.g.n, dev)
    rowptr = csr.rowptr.cpu().numpy()
    np.testing.assert_array_equal(np.diff(rowptr[:d.g.n + 1]), d.g.degree)
    m = d.g.names['big_boundary']
    assert np.diff(rowptr)[m['t_kids']].tolist() == [planted.BIG_DEGREE, planted.BIG_DEGREE + 1]
    m = d.g.names['raced_key']
    col = csr.col.cpu().numpy()
    hub_row = col[rowptr[m['hub']]:rowptr[m['hub'] + 1]]  # (the order inside a row is the CSR's own)
    np.testing.assert_array_equal(np.sort(hub_row), np.repeat(np.sort(m['leaves']), planted.RACED_COPIES))
    for x, y in zip(m['leaves'], m['tails']):  # 16 equal sources, one per lane of the group that walks the tail
        assert col[rowptr[y]:rowptr[y + 1]].tolist() == [x] * planted.GROUP_LANES


# ---- every planted link, every hop count, both tiers -------------------------------------------------------------------------------------
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_features_of_every_planted_link(ssa, dev, on_device, knobs, h, mask):
    d = on_device()
    g = d.g
    want, sizes = planted.expected_features(g, h, mask), planted.union_sizes(g, h, mask)
    chip, overflow = _features(ssa, d, dev, g.links, h, mask)
    _same_features(chip, want)
    assert overflow == int((sizes > planted.NODE_LIMIT).sum()) >= 4  # (A, B) and the 2 049 unions, both orders; 2 048 stays on chip
    knobs.EXACT_LDS_MAX_NODES = 0
    slot, overflow = _features(ssa, d, dev, g.links, h, mask)
    assert overflow == len(g.links)
    _same_features(slot, want)
    assert arena_dist_words_are_zero(ssa, dev)


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_nodes_of_every_planted_link(ssa, dev, on_device, knobs, h, mask):
    """on chip the rows come out of lds_ordered_emit, one lds_find per listed node through the planted chains; in the large tier out of
    the ordered scan, whose step edges the scan_edges star sits on"""
    d = on_device()
    g = d.g
    want, sizes = planted.expected_nodes(g, h, mask), planted.union_sizes(g, h, mask)
    chip, info = _nodes(d, dev, g.links, h, mask)
    _same_rows(chip, want)
    _tiers(info, sizes, planted.NODE_LIMIT)
    knobs.EXACT_LDS_MAX_NODES = 0
    slot, info = _nodes(d, dev, g.links, h, mask)
    _same_rows(slot, want)
    _tiers(info, sizes, 0)
    assert arena_dist_words_are_zero(ssa, dev)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_sampled_walk_without_sampling_of_every_planted_link(ssa, dev, on_device, knobs, h):
    """the joint walk's own visit and keep through the same tables: with nothing dropped its rows are the unions, hop = min(d_u, d_v)"""
    d = on_device()
    g = d.g
    want, visited, sampled = planted.expected_sampled(g, h, None, 1.0)
    np.testing.assert_array_equal(want[2], planted.expected_nodes(g, h, False)[2].min(axis=1))
    for limit in (planted.NODE_LIMIT, 0):
        knobs.EXACT_LDS_MAX_NODES = limit
        got, info = _sampled(d, dev, g.links, h, None, 1.0)
        _same_rows(got, want, ('rowptr', 'ids', 'hop'))
        _tiers(info, visited, limit)
        assert info['sampled_links'] == sampled == 0
    assert arena_dist_words_are_zero(ssa, dev)


def test_scan_edges_with_a_partial_last_word(ssa, dev, on_device, knobs):
    """N = 99 999: the last level word of a slot holds three nodes, and id N - 1 = 99 998 is listed"""
    d = on_device(planted.ODD_N)
    g = d.g
    assert g.n % planted.NODES_PER_WORD == 3
    for h in (1, 2, 3):
        want = planted.expected_nodes(g, h, False)
        assert h == 1 or g.n - 1 in want[1]
        for limit in (planted.NODE_LIMIT, 0):
            knobs.EXACT_LDS_MAX_NODES = limit
            got, info = _nodes(d, dev, g.links, h, False)
            _same_rows(got, want)
            _tiers(info, np.diff(want[0]), limit)
            got, _ = _features(ssa, d, dev, g.links, h, True)
            _same_features(got, planted.expected_features(g, h, True))
            got, _ = _sampled(d, dev, g.links, h, None, 1.0)
            _same_rows(got, planted.expected_sampled(g, h, None, 1.0)[0], ('rowptr', 'ids', 'hop'))
        assert arena_dist_words_are_zero(ssa, dev)


# ---- the tier boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('case', ['one_home', 'wrap'])
def test_limit_at_the_union_and_one_below(ssa, dev, on_device, knobs, case, h):
    """limit = |union| of the (hub, isolated) link: the table takes its last key exactly at the limit and the link stays on chip; one
    less and the same link overflows while the chain is being built, leaves the table to lds_clear and goes to the large tier"""
    d = on_device()
    g = d.g
    rows = g.rows_of(case)
    links = g.links[rows]
    for mask in (False, True):
        sizes = planted.union_sizes(g, h, mask)[rows]
        union = int(sizes[0])
        assert union == len(g.names[case]['leaves']) + 2 == sizes.max()
        for limit in (union, union - 1):
            knobs.EXACT_LDS_MAX_NODES = limit
            one, overflow = _features(ssa, d, dev, links[:1], h, mask)
            assert overflow == (limit < union)
            _same_features(one, planted.expected_features(g, h, mask), rows[:1])
            got, overflow = _features(ssa, d, dev, links, h, mask)
            assert overflow == int((sizes > limit).sum())
            _same_features(got, planted.expected_features(g, h, mask), rows)
            one, info = _nodes(d, dev, links[:1], h, mask)
            _tiers(info, sizes[:1], limit)
            got, info = _nodes(d, dev, links, h, mask)
            _tiers(info, sizes, limit)
            _same_rows(got, planted.take_rows(*planted.expected_nodes(g, h, mask), rows))
            _same_rows(one, planted.take_rows(*planted.expected_nodes(g, h, mask), rows[:1]))
            # and every planted link at this limit: the smaller unions on chip, the rest -- the case's own link at union - 1 -- not
            every = planted.union_sizes(g, h, mask)
            got, overflow = _features(ssa, d, dev, g.links, h, mask)
            assert overflow == int((every > limit).sum())
            _same_features(got, planted.expected_features(g, h, mask))
            got, info = _nodes(d, dev, g.links, h, mask)
            _tiers(info, every, limit)
            _same_rows(got, planted.expected_nodes(g, h, mask))
    assert arena_dist_words_are_zero(ssa, dev)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_unions_of_2048_and_2049_at_the_default_limit(ssa, dev, on_device, h):
    d = on_device()
    g = d.g
    for case, union in (('window_2048', planted.NODE_LIMIT), ('window_2049', planted.NODE_LIMIT + 1)):
        rows = g.rows_of(case)
        for mask in (False, True):
            assert (planted.union_sizes(g, h, mask)[rows] == union).all() and len(rows) == 2
            got, overflow = _features(ssa, d, dev, g.links[rows], h, mask)
            assert overflow == (2 if union > planted.NODE_LIMIT else 0)
            _same_features(got, planted.expected_features(g, h, mask), rows)
            got, info = _nodes(d, dev, g.links[rows], h, mask)
            assert (info['lds_links'], info['large_links']) == ((0, 2) if union > planted.NODE_LIMIT else (2, 0))
            _same_rows(got, planted.take_rows(*planted.expected_nodes(g, h, mask), rows))
            got, info = _sampled(d, dev, g.links[rows], h, None, 1.0)
            assert info['large_links'] == (2 if union > planted.NODE_LIMIT else 0)
            assert np.diff(got[0]).tolist() == [union, union]
    assert arena_dist_words_are_zero(ssa, dev)


# ---- the sampled select over a colliding fringe ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('limit', [planted.NODE_LIMIT, 0])
@pytest.mark.parametrize('case', ['one_home', 'wrap', 'window'])
def test_sampled_select_over_a_colliding_fringe(ssa, dev, on_device, knobs, case, limit):
    """a cap of F - 1 (the select drops ONE node of the hub's fringe) and a ratio of 0.5, on the links of the chain, the wrapped
    cluster and the window: sampled_subgraph_nodes on all of the case's links, exact_subgraphs on the hub's"""
    d = on_device()
    g = d.g
    knobs.EXACT_LDS_MAX_NODES = limit
    m = g.names[case]
    F = len(m['leaves'] if case != 'window' else m['leaves'][0])
    links = g.links[g.rows_of(case)]
    for cap, ratio in ((F - 1, 1.0), (None, 0.5)):
        for h in (1, 2, 3):
            want, visited, sampled = planted.expected_sampled(g, h, cap, ratio, links)
            got, info = _sampled(d, dev, links, h, cap, ratio)
            _same_rows(got, want, ('rowptr', 'ids', 'hop'))
            _tiers(info, visited, limit)
            assert info['sampled_links'] == sampled >= 2
        d.eh.max_hops = 2
        hub_links = links[[0, 1, 4]]  # (hub, isolated), (isolated, hub), (hub, leaf)
        sg = d.eh.exact_subgraphs(_dev_links(hub_links, dev), g.n, d.ei, mask_target=True, node_label='drnl', max_nodes_per_hop=cap,
                                  ratio_per_hop=ratio, seed=planted.SAMPLED_SEED)
        assert type(sg) is ssa.subgraphs.SampledSubgraphs
        sub = ssr.restate(g.n, g.ei, hub_links, 2, mask_target=True, cap=cap, ratio=ratio, seed=planted.SAMPLED_SEED)
        for k in SUBGRAPH_FIELDS + ('hop',):
            np.testing.assert_array_equal(getattr(sg, k).cpu().numpy(), getattr(sub, k), err_msg=k)
        np.testing.assert_array_equal(sg.z.cpu().numpy(), ssr.labels(sub, 'drnl'))
    assert arena_dist_words_are_zero(ssa, dev)


# ---- big_boundary and raced_key ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('limit', [planted.NODE_LIMIT, 0])
def test_big_boundary_and_raced_key(ssa, dev, on_device, knobs, limit):
    """the 512 / 513 children, the level of 70 big nodes (each guards two leaves only its own walk reaches) and the star whose arcs come
    16 in a row, through the features, node-list, subgraph and sampled calls in either tier"""
    d = on_device()
    g = d.g
    knobs.EXACT_LDS_MAX_NODES = limit
    rows = g.rows_of('big_boundary', 'raced_key')
    links = g.links[rows]
    for h in (1, 2, 3):
        for mask in (False, True):
            got, overflow = _features(ssa, d, dev, links, h, mask)
            assert overflow == (len(rows) if limit == 0 else 0)
            _same_features(got, planted.expected_features(g, h, mask), rows)
            got, info = _nodes(d, dev, links, h, mask)
            _same_rows(got, planted.take_rows(*planted.expected_nodes(g, h, mask), rows))
            assert info['large_links'] == (len(rows) if limit == 0 else 0)
        want, visited, sampled = planted.expected_sampled(g, h, 40, 0.75, links)
        got, info = _sampled(d, dev, links, h, 40, 0.75)
        _same_rows(got, want, ('rowptr', 'ids', 'hop'))
        assert info['sampled_links'] == sampled > 0
    d.eh.max_hops = 2
    sg = d.eh.exact_subgraphs(_dev_links(links, dev), g.n, d.ei, mask_target=True, node_label='de')
    sub = sr.restate(g.n, g.ei, links, 2, mask_target=True)
    for k in SUBGRAPH_FIELDS + ('dist',):
        np.testing.assert_array_equal(getattr(sg, k).cpu().numpy(), getattr(sub, k), err_msg=k)
    np.testing.assert_array_equal(sg.z.cpu().numpy(), sr.labels(sub, 'de'))
    assert int(sub.weight.max()) == planted.BIG_DEGREE + 1 and planted.RACED_COPIES in sub.weight  # the copies are counted
    assert arena_dist_words_are_zero(ssa, dev)


# ---- workgroups that serve link after link -------------------------------------------------------------------------------------------------
def _reuse_expected(g, h, links):
    uniq, inv = np.unique(links, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return uniq, inv, planted.union_sizes(g, h, False, uniq)[inv]


def _run_reuse(ssa, d, dev, h, limit):
    """the tiled list through the three calls, one launch per tier and pass each: every row equals its link's row computed alone"""
    g = d.g
    links, of, swapped = planted.reuse_links(g)
    uniq, inv, sizes = _reuse_expected(g, h, links)
    for mask in (False, True):
        got, overflow = _features(ssa, d, dev, links, h, mask)
        assert overflow == int((planted.union_sizes(g, h, mask, uniq)[inv] > limit).sum())
        _same_features(got, planted.expected_features(g, h, mask, uniq), inv)
    got, info = _nodes(d, dev, links, h, False)
    _tiers(info, sizes, limit)
    _same_rows(got, planted.take_rows(*planted.expected_nodes(g, h, False, uniq), inv))
    want, visited, sampled = planted.expected_sampled(g, h, *planted.REUSE_SAMPLING, uniq)
    got, info = _sampled(d, dev, links, h, *planted.REUSE_SAMPLING)
    _same_rows(got, planted.take_rows(*want, inv), ('rowptr', 'ids', 'hop'))
    _tiers(info, visited[inv], limit)
    assert arena_dist_words_are_zero(ssa, dev)
    return sizes, visited[inv]


def test_reuse_default_tiers(ssa, dev, on_device):
    """6 244 rows over 1 024 workgroups: each serves a planted link, the same link with its ends swapped, then the link 17 places on
    and so on, from one table that only lds_release empties -- a key left behind is one node too many in the next union, a value
    half left behind moves the swapped link's counts"""
    _run_reuse(ssa, on_device(), dev, 2, planted.NODE_LIMIT)


def test_reuse_a_third_in_the_large_tier_two_slots(ssa, dev, on_device, knobs):
    """a limit that sends about a third of the rows to the large tier, and two slots for them: every slot serves hundreds of links in a
    row (slot_clear / the scan's own clearing between them), and hundreds of on-chip workgroups serve a link from the table that
    lds_clear rebuilt after the link they abandoned just before -- in the features launch, the node lists' count pass and the
    sampled walk's (whose tier goes by its visited set)"""
    d = on_device()
    links, _, _ = planted.reuse_links(d.g)
    _, _, sizes = _reuse_expected(d.g, 2, links)
    limit = planted.reuse_limit(sizes)
    large = int((sizes > limit).sum())
    assert len(sizes) // 4 < large < (2 * len(sizes)) // 5 and limit < planted.NODE_LIMIT
    knobs.EXACT_LDS_MAX_NODES, knobs.EXACT_LARGE_SLOTS = limit, 2
    sizes, visited = _run_reuse(ssa, d, dev, 2, limit)
    assert planted.workgroups_serving_after_an_overflow(sizes, limit) >= 300
    assert planted.workgroups_serving_after_an_overflow(visited, limit) >= 300
    assert ssa.exact._arena(dev, d.g.n)[0] == 2
