"""ElphHashes.exact_subgraph_features (exact.py, csrc/ss_exact.hip) on the GPU: I and the ball sizes must equal the set / scipy
counts exactly and the features the restatement (tests/exact_restatement.py) bit for bit -- on the BA-40 golden graph (every pair,
every hop count and flag setting), the trailing-isolated-node and empty graphs, a directed graph, a star whose balls are the whole
graph, a 50k-node power-law graph through either tier, and collab size; plus invariance under batching, order and input placement,
a cross-check of I[0][0] against the CN heuristic, and the error paths."""
from argparse import Namespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import exact_restatement as er
from conftest import load_golden

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


def _eh(ssa, h=2, use_zero_one=True, floor_sf=False):
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=floor_sf, use_zero_one=use_zero_one))


def _power_law_graph(n=50000, e_und=250000, seed=7):  # (the generator of test_topk_gpu.py)
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, size=e_und)
    dst = np.minimum((n * rng.random_sample(e_und) ** 3).astype(np.int64), n - 1)
    e = np.stack([src, dst]).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _uniform_graph(n, e_und, seed):
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _pairs(rng, n, ei, count):
    """count // 2 random pairs and count // 2 edge pairs"""
    rnd = rng.randint(0, n, size=(count // 2, 2))
    edges = ei[:, rng.randint(0, ei.shape[1], size=count - count // 2)].T
    return np.concatenate([rnd, edges]).astype(np.int64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(eh, n, ei, links, dev, ei_dev=True):
    """run on the device and compare with the restatement: counts exactly, features bit for bit"""
    e = torch.from_numpy(ei)
    feats, I, balls = eh.exact_subgraph_features(torch.from_numpy(links).to(dev), n, e.to(dev) if ei_dev else e, return_counts=True)
    assert feats.device == dev and feats.dtype == torch.float32 and I.dtype == torch.int32 and balls.dtype == torch.int32
    wf, wI, wb = er.restate(n, ei, links, eh.max_hops, eh.use_zero_one, eh.floor_sf)
    np.testing.assert_array_equal(I.cpu().numpy(), wI)
    np.testing.assert_array_equal(balls.cpu().numpy(), wb)
    np.testing.assert_array_equal(_bits(feats.cpu().numpy()), _bits(wf))
    return feats, I, balls


@pytest.mark.parametrize('h', [1, 2, 3])
def test_ba40_all_pairs(ssa, dev, h):
    g = load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), g['edge_index']
    nbrs = [set() for _ in range(n)]
    for s, d in ei.T.tolist():
        nbrs[d].add(s)  # in-neighbours
    links = np.array([(u, v) for u in range(n) for v in range(n)], dtype=np.int64)
    def ball(x, k):
        b = {x}
        for _ in range(k):
            b = b.union(*[nbrs[y] for y in b])
        return b
    for zo in (True, False):
        for fl in (False, True):
            eh = _eh(ssa, h, zo, fl)
            feats, I, balls = _check(eh, n, ei, links, dev)
    I, balls = I.cpu().numpy(), balls.cpu().numpy()
    for i, (u, v) in enumerate(links[::7]):
        for k1 in range(h):
            assert balls[7 * i, 0, k1] == len(ball(u, k1 + 1)) and balls[7 * i, 1, k1] == len(ball(v, k1 + 1))
            for k2 in range(h):
                assert I[7 * i, k1, k2] == len(ball(u, k1 + 1) & ball(v, k2 + 1))


def test_max_hops_read_at_call_time(ssa, dev):
    g = load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), g['edge_index']
    eh = _eh(ssa, 2)
    eh.max_hops = 3
    eh.use_zero_one, eh.floor_sf = False, True
    _check(eh, n, ei, np.array([[0, 1], [5, 39], [-1, 3]]), dev)
    one = eh.exact_subgraph_features(torch.tensor([0, 1]), n, torch.from_numpy(ei))
    assert one.shape == (1, 15) and one.device.type == 'cpu'


def test_trailing_isolated_nodes_and_empty_graph(ssa, dev):
    g = load_golden('g7_edge_cases.npz')
    n, ei = int(g['num_nodes']), g['edge_index']
    links = np.array([[u, v] for u in range(n) for v in range(n)], dtype=np.int64)
    for h in (1, 2, 3):
        feats, I, balls = _check(_eh(ssa, h), n, ei, links, dev)
        tail = links >= int(ei.max()) + 1
        b = balls.cpu().numpy()
        assert not b[:, 0][tail[:, 0]].any() and not b[:, 1][tail[:, 1]].any()
        assert not feats.cpu().numpy()[tail.all(axis=1)].any()
    feats, I, balls = _eh(ssa, 2).exact_subgraph_features(torch.tensor([[0, 1], [4, 4], [-1, 2]], device=dev), 5,
                                                          torch.zeros((2, 0), dtype=torch.long, device=dev), return_counts=True)
    assert not feats.any() and not I.any() and not balls.any()


def test_directed_graph_follows_in_edges(ssa, dev):
    # a path 0 -> 1 -> 2 -> 3 plus 4 -> 3: B_k(3) grows with k, B_k(0) = {0}
    ei = np.array([[0, 1, 2, 4], [1, 2, 3, 3]], dtype=np.int64)
    feats, I, balls = _check(_eh(ssa, 3), 6, ei, np.array([[3, 0], [0, 3], [3, 3], [2, 4], [5, 3]]), dev)
    b = balls.cpu().numpy()
    np.testing.assert_array_equal(b[0, 0], [3, 4, 5])   # B_1(3) = {3, 2, 4}, B_2 adds 1, B_3 adds 0
    np.testing.assert_array_equal(b[0, 1], [1, 1, 1])   # B_k(0) = {0}: no in-edges
    np.testing.assert_array_equal(b[4, 0], [0, 0, 0])   # node 5 >= max(edge_index) + 1: no self loop
    rng = np.random.RandomState(4)
    ei = rng.randint(0, 300, size=(2, 900)).astype(np.int64)
    _check(_eh(ssa, 3), 300, ei, rng.randint(0, 300, size=(500, 2)), dev)


@pytest.mark.parametrize('h', [2, 3])
def test_star_balls_cover_the_graph(ssa, dev, h):
    n = 100_001
    leaves = np.arange(1, n, dtype=np.int64)
    ei = np.concatenate([np.stack([np.zeros_like(leaves), leaves]), np.stack([leaves, np.zeros_like(leaves)])], axis=1)
    links = np.array([[1, 2], [0, 5], [7, 0], [0, 0], [n - 1, 3], [9, 9]] * 8, dtype=np.int64)
    feats, I, balls = _check(_eh(ssa, h), n, ei, links, dev)
    b = balls.cpu().numpy()
    assert (b[:, :, h - 1] == n).all() and (b[:, :, 1] == n).all()


@pytest.fixture(scope='module')
def powerlaw():
    n = 50000
    ei = _power_law_graph()
    return n, ei, _pairs(np.random.RandomState(1), n, ei, 10000)


@pytest.mark.parametrize('h', [2, 3])
def test_powerlaw_50k_both_tiers(ssa, dev, powerlaw, h):
    """5 000 random + 5 000 edge pairs through the default tiers and through the large tier alone: identical.  The restatement checks
    all of them at h = 2 and 1 000 at h = 3 (its h = 3 balls hold most of the graph: 10 000 such rows do not fit a test's memory)"""
    n, ei, links = powerlaw
    eh = _eh(ssa, h)
    ld = torch.from_numpy(links).to(dev)
    feats, I, balls = eh.exact_subgraph_features(ld, n, torch.from_numpy(ei).to(dev), return_counts=True)
    sub = np.arange(len(links)) if h == 2 else np.r_[0:500, 5000:5500]
    wf, wI, wb = er.restate(n, ei, links[sub], h)
    np.testing.assert_array_equal(I.cpu().numpy()[sub], wI)
    np.testing.assert_array_equal(balls.cpu().numpy()[sub], wb)
    np.testing.assert_array_equal(_bits(feats.cpu().numpy()[sub]), _bits(wf))
    ssa.knobs.EXACT_LDS_MAX_NODES, old = 0, ssa.knobs.EXACT_LDS_MAX_NODES
    try:
        f2, I2, b2 = eh.exact_subgraph_features(ld, n, torch.from_numpy(ei).to(dev), return_counts=True)
    finally:
        ssa.knobs.EXACT_LDS_MAX_NODES = old
    assert torch.equal(I, I2) and torch.equal(balls, b2)
    np.testing.assert_array_equal(_bits(feats.cpu().numpy()), _bits(f2.cpu().numpy()))


@pytest.mark.parametrize('kind', ['uniform', 'powerlaw'])
def test_collab_size(ssa, dev, kind):
    n, e_und = 235_868, 1_179_052
    if kind == 'uniform':
        ei = _uniform_graph(n, e_und, 3)
    else:
        ei = _power_law_graph(n, e_und, 3)
    rng = np.random.RandomState(5)
    links = _pairs(rng, n, ei, 65536)
    eh = _eh(ssa, 2)
    ei_dev = torch.from_numpy(ei).to(dev)
    feats, I, balls = eh.exact_subgraph_features(torch.from_numpy(links).to(dev), n, ei_dev, return_counts=True)
    sample = rng.choice(len(links), size=2000, replace=False)
    wf, wI, wb = er.restate(n, ei, links[sample], 2)
    np.testing.assert_array_equal(I.cpu().numpy()[sample], wI)
    np.testing.assert_array_equal(balls.cpu().numpy()[sample], wb)
    np.testing.assert_array_equal(_bits(feats.cpu().numpy()[sample]), _bits(wf))
    # batch size, link order and input placement change nothing
    f_b = eh.exact_subgraph_features(torch.from_numpy(links).to(dev), n, ei_dev, batch_size=7777)
    assert torch.equal(f_b, feats)
    perm = rng.permutation(len(links))
    f_p = eh.exact_subgraph_features(torch.from_numpy(links[perm]).to(dev), n, ei_dev)
    assert torch.equal(f_p.cpu(), feats.cpu()[perm])
    f_c, I_c, b_c = eh.exact_subgraph_features(torch.from_numpy(links), n, torch.from_numpy(ei), return_counts=True)
    assert f_c.device.type == 'cpu' and I_c.device.type == 'cpu'
    assert torch.equal(f_c, feats.cpu()) and torch.equal(I_c, I.cpu()) and torch.equal(b_c, balls.cpu())


def test_csr_cache_reused(ssa, dev):
    g = load_golden('g3_g4_ba40.npz')
    n = int(g['num_nodes'])
    ei = torch.from_numpy(g['edge_index']).to(dev)
    eh = _eh(ssa, 2)
    links = torch.tensor([[0, 1], [2, 3]], device=dev)
    a = eh.exact_subgraph_features(links, n, ei)
    csr = eh._csr_cache._csr
    b = eh.exact_subgraph_features(links, n, ei)
    assert eh._csr_cache._csr is csr and torch.equal(a, b)


def test_first_cell_equals_common_neighbours_plus_edge(ssa, dev):
    """symmetric 0/1 adjacency without self loops: B_1(x) = N(x) + x, so |B_1(u) & B_1(v)| = CN(u, v) + 2 A[u, v] for u != v"""
    rng = np.random.RandomState(8)
    n = 3000
    e = rng.randint(0, n, size=(2, 12000))
    e = e[:, e[0] != e[1]]
    A = sp.coo_matrix((np.ones(e.shape[1]), (e[0], e[1])), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float32).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    ei = np.stack(A.nonzero()).astype(np.int64)
    n_self = int(ei.max()) + 1
    links = rng.randint(0, n_self, size=(4000, 2))
    links = links[links[:, 0] != links[:, 1]]
    links = np.concatenate([links, ei[:, :500].T]).astype(np.int64)
    cn, _ = ssa.heuristics.CN(A, torch.from_numpy(links))
    _, I, _ = _eh(ssa, 1).exact_subgraph_features(torch.from_numpy(links).to(dev), n, torch.from_numpy(ei).to(dev), return_counts=True)
    adj = np.asarray(A[links[:, 0], links[:, 1]]).ravel()
    np.testing.assert_array_equal(I.cpu().numpy()[:, 0, 0], cn.numpy().astype(np.int64) + 2 * adj.astype(np.int64))


def test_error_paths(ssa, dev):
    g = load_golden('g3_g4_ba40.npz')
    n = int(g['num_nodes'])
    ei = torch.from_numpy(g['edge_index']).to(dev)
    eh = _eh(ssa, 2)
    with pytest.raises(IndexError):
        eh.exact_subgraph_features(torch.tensor([[0, n]], device=dev), n, ei)
    with pytest.raises(IndexError):
        eh.exact_subgraph_features(torch.tensor([[-n - 1, 0]], device=dev), n, ei)
    with pytest.raises(IndexError, match='edge_index refers to nodes outside'):
        eh.exact_subgraph_features(torch.tensor([[0, 1]], device=dev), n - 1, ei)
    with pytest.raises(ValueError):
        eh.exact_subgraph_features(torch.tensor([[0, 1, 2]], device=dev), n, ei)
    eh.max_hops = 4
    with pytest.raises(NotImplementedError):
        eh.exact_subgraph_features(torch.tensor([[0, 1]], device=dev), n, ei)
    eh.max_hops = 2
    # negative ids wrap, as in the sketch query
    a = eh.exact_subgraph_features(torch.tensor([[-1, -40]], device=dev), n, ei)
    b = eh.exact_subgraph_features(torch.tensor([[39, 0]], device=dev), n, ei)
    assert torch.equal(a, b)


@pytest.fixture
def lds_limit(ssa):
    """sets knobs.EXACT_LDS_MAX_NODES for one test and restores it"""
    old = ssa.knobs.EXACT_LDS_MAX_NODES
    yield lambda value: setattr(ssa.knobs, 'EXACT_LDS_MAX_NODES', value)
    ssa.knobs.EXACT_LDS_MAX_NODES = old


@pytest.mark.parametrize('limit', [1, 2, 3, 5, 8, 40, 2048])
def test_every_lds_limit_gives_the_same_counts(ssa, dev, lds_limit, limit):
    """the on-chip node limit only moves pairs between the tiers.  Small limits overflow while a root is inserted: limit 1 with a u
    whose ball is {u} fills the table exactly on side 0 and overflows on v's root"""
    lds_limit(limit)
    rng = np.random.RandomState(12)
    n = 300
    ei = rng.randint(0, n, size=(2, 900)).astype(np.int64)
    sinks = np.setdiff1d(np.arange(n), ei[1])  # no in-edges: B_k(u) = {u}
    assert sinks.size
    links = np.concatenate([rng.randint(0, n, size=(400, 2)), np.stack([sinks, rng.randint(0, n, size=sinks.size)], 1),
                            np.stack([sinks, sinks], 1)]).astype(np.int64)
    for h in (1, 2, 3):
        _check(_eh(ssa, h), n, ei, links, dev)


def test_lds_limit_equal_to_the_first_ball(ssa, dev, lds_limit):
    """limit = |B_h(u)|: side 0 fills the table to the limit exactly; v's side then overflows unless it adds no node"""
    rng = np.random.RandomState(13)
    n = 400
    ei = _uniform_graph(n, 500, 6)
    for h in (2, 3):
        us = rng.choice(n, size=6, replace=False)
        _, _, balls = er.restate(n, ei, np.stack([us, us], 1), h)
        for u, b in zip(us, balls[:, 0, h - 1]):
            lds_limit(int(b))
            links = np.stack([np.full(n, u), np.arange(n)], 1).astype(np.int64)
            _check(_eh(ssa, h), n, ei, links, dev)


def test_two_streams_in_flight(ssa, dev, lds_limit):
    """calls in flight on two streams at once use two large-tier arenas (every pair through the large tier)"""
    lds_limit(0)
    n, ei, links = 50000, _power_law_graph(), _pairs(np.random.RandomState(3), 50000, _power_law_graph(), 4000)
    ei_dev = torch.from_numpy(ei).to(dev)
    la, lb = torch.from_numpy(links[:2000]).to(dev), torch.from_numpy(links[2000:]).to(dev)
    eh = _eh(ssa, 2)
    eh.exact_subgraph_features(la[:1], n, ei_dev)  # (the CSR is built once, outside the race)
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        fa = eh.exact_subgraph_features(la, n, ei_dev)
    with torch.cuda.stream(sb):
        fb = eh.exact_subgraph_features(lb, n, ei_dev)
    torch.cuda.synchronize()
    wf, _, _ = er.restate(n, ei, links, 2)
    np.testing.assert_array_equal(_bits(torch.cat([fa, fb]).cpu().numpy()), _bits(wf))
