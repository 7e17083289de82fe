"""ElphHashes.exact_subgraph_nodes (exact_nodes.py, csrc/ss_exact_nodes.hip) on the GPU: rowptr, ids and dist must EQUAL the scipy
restatement (tests/exact_nodes_restatement.py) -- on the BA-40 golden graph (every hop count, masked or not), a 3 000-node uniform
graph under batching and shuffling, two stars through either kernel tier (and the arena all zero afterwards), batches, max_nodes and
both tiers in one call, against the histograms
the shipped exact_subgraph_features counts, under max_nodes, and on the edge cases (no links, no edges, duplicate and self-loop edges,
CPU inputs, a directed edge_index)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import exact_nodes_restatement as nr
from conftest import load_golden
from test_exact_nodes_host import _ba40, _uniform300

pytestmark = pytest.mark.gpu


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


def _run(eh, n, ei, links, dev, **kw):
    """one call with everything on the device -> numpy (rowptr, ids, dist[, info])"""
    out = eh.exact_subgraph_nodes(torch.from_numpy(np.asarray(links, dtype=np.int64)).to(dev), n, torch.from_numpy(ei).to(dev), **kw)
    rowptr, ids, dist = out[:3]
    assert rowptr.device == ids.device == dist.device == dev
    assert rowptr.dtype == torch.int64 and ids.dtype == torch.int64 and dist.dtype == torch.uint8 and dist.shape == (ids.numel(), 2)
    return tuple(t.cpu().numpy() for t in out[:3]) + tuple(out[3:])


def _same(got, want):
    for g, w, name in zip(got, want, ('rowptr', 'ids', 'dist')):
        np.testing.assert_array_equal(g, w, err_msg=name)


def _arena_is_zero(ssa):
    """every distance byte of every slot of every arena is zero: what the next call's BFS relies on (the int32 visit lists behind a
    slot's bytes are scratch -- written before they are read, by the exact counts too -- and are not part of it)"""
    torch.cuda.synchronize()
    assert ssa.exact._ARENA, 'no large-tier arena was made'
    for n, slots, arena, _ in ssa.exact._ARENA.values():
        words = arena.view(torch.int32).view(slots, -1)
        assert words.size(1) == ssa._native.lib().ss_exact_slot_bytes(n) // 4
        if bool(words[:, :(n + 3) // 4].any()):
            return False
    return True


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_ba40(ssa, dev, h, mask):
    n, ei, links = _ba40()  # an edge, a non-edge, u == v, isolated nodes, negative ids
    _same(_run(_eh(ssa, h), n, ei, links, dev, mask_target=mask), nr.restate(n, ei, links, h, mask_target=mask))


# ---- invariance: 3 000 uniform nodes, 512 random links + 64 edges -------------------------------------------------------------------
@pytest.fixture(scope='module')
def uniform3000():
    n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
    e = np.random.RandomState(seed).randint(0, n, size=(2, e_und)).astype(np.int64)
    ei = np.concatenate([e, e[::-1]], axis=1)
    rng = np.random.RandomState(31)
    links = np.concatenate([rng.randint(0, n, size=(512, 2)), ei[:, rng.randint(0, ei.shape[1], size=64)].T]).astype(np.int64)
    return n, ei, links, {mask: nr.restate(n, ei, links, 2, mask_target=mask) for mask in (False, True)}


def _unshuffle(rowptr, ids, dist, perm):
    """the rows of a run over links[perm], back in the order of links"""
    rows = nr.rows(rowptr, ids, dist)
    back = [None] * len(perm)
    for place, q in enumerate(perm):
        back[q] = rows[place]
    sizes = [len(r[0]) for r in back]
    return (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.concatenate([r[0] for r in back]),
            np.concatenate([r[1] for r in back]).reshape(-1, 2))


@pytest.mark.parametrize('mask', [False, True])
def test_rows_do_not_depend_on_batching_or_order(ssa, dev, uniform3000, mask):
    n, ei, links, want = uniform3000
    eh = _eh(ssa, 2)
    whole = _run(eh, n, ei, links, dev, batch_size=11000000, mask_target=mask)
    _same(whole, want[mask])
    _same(_run(eh, n, ei, links, dev, batch_size=37, mask_target=mask), whole)
    perm = np.random.RandomState(5).permutation(len(links))
    _same(_unshuffle(*_run(eh, n, ei, links[perm], dev, batch_size=100, mask_target=mask), perm), whole)


# ---- tier boundary --------------------------------------------------------------------------------------------------------------------
def _stars():
    """hub 0 with leaves 1 .. 2500 and a path 0 - 2501 - ... - 2508 (unions with a leaf pass the on-chip table's 2048 nodes); hub 2600
    with leaves 2601 .. 4100 (unions of 1 501 nodes: the largest the on-chip tier sorts, no power of two); 4101 isolated"""
    a = np.arange(1, 2501)
    path = np.arange(2501, 2509)
    b = np.arange(2601, 4101)
    src = np.concatenate([np.zeros_like(a), [0], path[:-1], np.full_like(b, 2600)])
    dst = np.concatenate([a, path[:1], path[1:], b])
    ei = np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]).astype(np.int64)
    links = np.array([[3, 2077], [0, 9], [2508, 1234], [2501, 2500], [2508, 2506], [2507, 2507], [2700, 4000], [2600, 2601], [4100, 2601],
                      [4101, 2602], [3, 4000], [2508, 4101]], dtype=np.int64)
    return 4102, ei, links


@pytest.mark.parametrize('mask', [False, True])
def test_both_tiers_give_the_same_rows(ssa, dev, lds_limit, mask):
    n, ei, links = _stars()
    want = nr.restate(n, ei, links, 2, mask_target=mask)
    eh = _eh(ssa, 2)
    first = _run(eh, n, ei, links, dev, mask_target=mask, return_info=True)   # the default on-chip capacity
    assert first[3]['lds_links'] > 0 and first[3]['large_links'] > 0 and first[3]['lds_links'] + first[3]['large_links'] == len(links)
    assert _arena_is_zero(ssa)
    _same(first, want)
    lds_limit(1)                                                              # every link overflows (no union has one node: u != v ...
    second = _run(eh, n, ei, links, dev, mask_target=mask, return_info=True)  # ... or it has neighbours)
    assert second[3]['lds_links'] == 0 and second[3]['large_links'] == len(links)
    assert _arena_is_zero(ssa)
    _same(second, want)
    _same(second, first)
    lds_limit(1501)                                                           # the limit equal to a union: still on chip
    third = _run(eh, n, ei, links, dev, mask_target=mask, return_info=True)
    assert third[3]['lds_links'] > 0 and _arena_is_zero(ssa)
    _same(third, want)


@pytest.mark.parametrize('limit', [0, 17, 100, 141])
def test_small_on_chip_limits(ssa, dev, lds_limit, uniform3000, limit):
    """the node limit only moves links between the tiers (h = 2 unions here hold 52 to 246 nodes: the last two limits split them)"""
    n, ei, links, want = uniform3000
    lds_limit(limit)
    got = _run(_eh(ssa, 2), n, ei, links, dev, return_info=True)
    _same(got, want[False])
    large = int((np.diff(want[False][0]) > limit).sum())
    assert 0 < large == got[3]['large_links'] and got[3]['lds_links'] == len(links) - large and _arena_is_zero(ssa)


# ---- batches, the cap and both tiers in one call ----------------------------------------------------------------------------------------
def _hub60():
    """hub 0 with leaves 1 .. 40 and a path 0 - 41 - 42 - ... - 59; 7 links: unions at the hub hold 42 to 49 nodes, unions on the path 5 to
    9, and with batches of 3 every batch but the last holds both kinds"""
    leaves, path = np.arange(1, 41), np.arange(41, 60)
    src = np.concatenate([np.zeros_like(leaves), [0], path[:-1]])
    dst = np.concatenate([leaves, path[:1], path[1:]])
    ei = np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]).astype(np.int64)
    return 60, ei, np.array([[1, 2], [0, 45], [50, 52], [59, 57], [44, 44], [0, 0], [-1, 3]], dtype=np.int64)


@pytest.mark.parametrize('h', [2, 3])
def test_batches_cap_and_both_tiers_in_one_call(ssa, dev, lds_limit, h):
    """every batch keeps its own workspace (counters and overflow list) from the count pass to the fill pass: batches of 3, an on-chip
    limit of 16 that sends the unions at the hub to the large tier, and max_nodes at the median row length, which empties three of the
    large tier's rows and keeps one"""
    n, ei, links = _hub60()
    rowptr, ids, dist = nr.restate(n, ei, links, h)
    sizes = np.diff(rowptr)
    cap = int(np.median(sizes))
    keep = sizes <= cap
    assert (sizes[keep] > 16).any() and (sizes[keep] <= 16).any() and not keep.all()
    full = nr.rows(rowptr, ids, dist)
    want = (np.concatenate([[0], np.cumsum(np.where(keep, sizes, 0))]), np.concatenate([full[q][0] for q in np.nonzero(keep)[0]]),
            np.concatenate([full[q][1] for q in np.nonzero(keep)[0]]))
    lds_limit(16)
    got = _run(_eh(ssa, h), n, ei, links, dev, batch_size=3, max_nodes=cap, return_info=True)
    _same(got, want)
    np.testing.assert_array_equal(got[3]['truncated'].cpu().numpy(), np.nonzero(~keep)[0])
    assert got[3]['large_links'] == (sizes > 16).sum() and got[3]['lds_links'] == (sizes <= 16).sum() and _arena_is_zero(ssa)


# ---- against the shipped counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('h', [1, 2, 3])
def test_histograms_equal_exact_subgraph_features(ssa, dev, uniform3000, h, mask):
    n, ei, links, _ = uniform3000
    assert links.max() < ei.max() + 1  # (every root has its self loop: the two queries agree on the balls)
    eh = _eh(ssa, h)
    ld, ed = torch.from_numpy(links).to(dev), torch.from_numpy(ei).to(dev)
    rowptr, ids, dist = eh.exact_subgraph_nodes(ld, n, ed, mask_target=mask)
    _, I, balls = eh.exact_subgraph_features(ld, n, ed, return_counts=True, mask_target=mask)
    rowptr, dist, I, balls = rowptr.cpu().numpy(), dist.cpu().numpy(), I.cpu().numpy(), balls.cpu().numpy()
    L = len(links)
    owner = np.repeat(np.arange(L), np.diff(rowptr))
    count = lambda keep: np.bincount(owner[keep], minlength=L)
    for k1 in range(1, h + 1):
        np.testing.assert_array_equal(count(dist[:, 0] <= k1), balls[:, 0, k1 - 1])
        np.testing.assert_array_equal(count(dist[:, 1] <= k1), balls[:, 1, k1 - 1])
        for k2 in range(1, h + 1):
            np.testing.assert_array_equal(count((dist[:, 0] <= k1) & (dist[:, 1] <= k2)), I[:, k1 - 1, k2 - 1])
    np.testing.assert_array_equal(np.diff(rowptr), balls[:, 0, h - 1] + balls[:, 1, h - 1] - I[:, h - 1, h - 1])


# ---- max_nodes --------------------------------------------------------------------------------------------------------------------------
def test_max_nodes(ssa, dev, uniform3000):
    n, ei, links, want = uniform3000
    sizes = np.diff(want[False][0])
    cap = int(np.median(sizes))
    over = np.nonzero(sizes > cap)[0]
    assert 0 < over.size < len(links)
    eh = _eh(ssa, 2)
    rowptr, ids, dist, info = _run(eh, n, ei, links, dev, max_nodes=cap, return_info=True)
    assert info['truncated'].device == dev and info['truncated'].dtype == torch.int64
    np.testing.assert_array_equal(info['truncated'].cpu().numpy(), over)
    got, full = nr.rows(rowptr, ids, dist), nr.rows(*want[False])
    for q in range(len(links)):
        if sizes[q] > cap:
            assert got[q][0].size == 0
        else:
            np.testing.assert_array_equal(got[q][0], full[q][0])
            np.testing.assert_array_equal(got[q][1], full[q][1])
    assert rowptr[-1] == sizes[sizes <= cap].sum() == ids.size
    out = _run(eh, n, ei, links, dev, max_nodes=int(sizes.max()), return_info=True, batch_size=200)
    assert out[3]['truncated'].numel() == 0
    _same(out, want[False])
    rowptr, ids, dist, info = _run(eh, n, ei, links, dev, max_nodes=1, return_info=True)  # (all but single-node unions capped)
    np.testing.assert_array_equal(info['truncated'].cpu().numpy(), np.nonzero(sizes > 1)[0])
    assert ids.size == rowptr[-1] == (sizes == 1).sum()


# ---- edge cases -------------------------------------------------------------------------------------------------------------------------
def test_no_links(ssa, dev):
    n, ei, _ = _uniform300()
    rowptr, ids, dist = _run(_eh(ssa, 2), n, ei, np.zeros((0, 2), dtype=np.int64), dev)
    assert rowptr.tolist() == [0] and ids.size == 0 and dist.shape == (0, 2)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_no_edges(ssa, dev, h):
    links = np.array([[0, 1], [4, 4], [-1, 2], [3, 0]], dtype=np.int64)
    rowptr, ids, dist = _run(_eh(ssa, h), 5, np.zeros((2, 0), dtype=np.int64), links, dev)
    np.testing.assert_array_equal(rowptr, [0, 2, 3, 5, 7])
    np.testing.assert_array_equal(ids, [0, 1, 4, 2, 4, 0, 3])
    np.testing.assert_array_equal(dist, [[0, h + 1], [h + 1, 0], [0, 0], [h + 1, 0], [0, h + 1], [h + 1, 0], [0, h + 1]])


@pytest.mark.parametrize('mask', [False, True])
def test_duplicate_edges_and_self_loops_change_nothing(ssa, dev, mask):
    n, ei, links = _uniform300()  # (holds duplicates and self-loop edges)
    clean = ei[:, ei[0] != ei[1]]
    clean = np.unique(clean[0] * n + clean[1])
    clean = np.stack([clean // n, clean % n])
    assert clean.shape[1] < ei.shape[1]
    for h in (1, 2, 3):
        eh = _eh(ssa, h)
        got = _run(eh, n, ei, links, dev, mask_target=mask)
        _same(got, nr.restate(n, ei, links, h, mask_target=mask))
        _same(_run(eh, n, clean, links, dev, mask_target=mask), got)


def test_cpu_inputs_give_cpu_outputs(ssa, dev):
    n, ei, links = _uniform300()
    eh = _eh(ssa, 2)
    out = eh.exact_subgraph_nodes(torch.from_numpy(links), n, torch.from_numpy(ei), max_nodes=40, return_info=True)
    assert all(t.device.type == 'cpu' for t in out[:3]) and out[3]['truncated'].device.type == 'cpu'
    want = _run(eh, n, ei, links, dev, max_nodes=40, return_info=True)
    _same(tuple(t.numpy() for t in out[:3]), want)
    np.testing.assert_array_equal(out[3]['truncated'].numpy(), want[3]['truncated'].cpu().numpy())
    one = eh.exact_subgraph_nodes(torch.tensor([3, 9]), n, torch.from_numpy(ei).to(dev))  # a [2] link; links decide where results go
    assert one[0].device.type == 'cpu' and one[0].shape == (2,)


@pytest.mark.parametrize('mask', [False, True])
def test_directed_edge_index_follows_in_edges(ssa, dev, mask):
    n, ei, links = _uniform300(directed=True)
    for h in (1, 2, 3):
        _same(_run(_eh(ssa, h), n, ei, links, dev, mask_target=mask), nr.restate(n, ei, links, h, mask_target=mask, directed=True))
