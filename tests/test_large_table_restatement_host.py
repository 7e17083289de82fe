"""tests/large_table_restatement.py without a GPU: the blocked torch restatement of one sketch hop reproduces the C oracle bit for
bit on small graphs (this is what makes it the reference of tests/test_large_tables_gpu.py and not a second opinion), it reports
exactly the row a wrapped offset would corrupt, and the graph generator of the large-table tests keeps its promises at a scale a
host can check."""
import numpy as np
import pytest
import torch

from conftest import oracle_params
import large_table_restatement as R

P, HLL_P, H = 128, 8, 2


def _uniform(n, e_und, seed, isolated):
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n - isolated, size=(2, e_und)).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)[:, :-5]          # slightly asymmetric: the direction of the flow matters


def _powerlaw(n, e_und, seed, isolated):
    rng = np.random.RandomState(seed)
    w = np.arange(1, n - isolated + 1, dtype=np.float64) ** -0.9
    cdf = np.cumsum(w / w.sum())
    e = np.stack([np.minimum(np.searchsorted(cdf, rng.random_sample(e_und)), n - isolated - 1),
                  rng.randint(0, n - isolated, size=e_und)]).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _as_torch(otab):
    return {k: (torch.from_numpy(v['minhash'].view(np.int32)), torch.from_numpy(v['hll'])) for k, v in otab.items()}


@pytest.fixture(scope='module')
def prm(regenerated_tables):
    return oracle_params(regenerated_tables[HLL_P])


@pytest.mark.parametrize('kind,n,e_und,isolated', [('uniform', 3000, 9000, 11), ('powerlaw', 4000, 30000, 7)])
def test_restatement_reproduces_the_oracle(prm, kind, n, e_und, isolated):
    """every row of hops 1 and 2 (trailing isolated nodes, which get no self loop, and a power-law hub row longer than a block
    included), with a block size that forces many blocks; hop 0 against the oracle's windows"""
    from oracle import oracle
    ei = (_uniform if kind == 'uniform' else _powerlaw)(n, e_und, 5, isolated)
    otab, _ = oracle.build_hash_tables(n, ei, H, P, prm)
    t = _as_torch(otab)
    blocks = R.EdgeBlocks(torch.from_numpy(ei), n, max_edges=997, max_rows=300)
    assert len(blocks.blocks) > 10 and blocks.blocks[0][0] == 0 and blocks.blocks[-1][1] == n
    assert all(a[1] == b[0] and a[3] == b[2] for a, b in zip(blocks.blocks, blocks.blocks[1:]))
    if kind == 'powerlaw':
        assert int(blocks.degree.max()) > 997, 'one row longer than a block'
    assert int(blocks.degree[n - isolated:].sum()) == 0
    for k in (1, 2):
        bad_mh, bad_hll = R.hop_mismatches(blocks, t[k - 1][0], t[k - 1][1], t[k][0], t[k][1])
        assert len(bad_mh) == 0 and len(bad_hll) == 0, k
        # the restated rows themselves, not only the verdict
        mh, hll = R.restate_block(blocks, blocks.blocks[3], t[k - 1][0], t[k - 1][1])
        r0, r1 = blocks.blocks[3][:2]
        assert np.array_equal(mh.numpy().astype(np.uint32), otab[k]['minhash'][r0:r1]) and np.array_equal(hll.numpy(), otab[k]['hll'][r0:r1])
    assert R.hop0_mismatches(oracle, t[0][0], t[0][1], n, [1024, 2048], HLL_P, width=256) == []


def test_restatement_reports_exactly_the_aliased_row(prm):
    """what a wrapped offset produces: row r - W stored over row r (r mod 2^k aliasing).  The helper names that row and no other,
    in either sketch, and says on which side of which boundary it lies"""
    from oracle import oracle
    n, W = 3000, 1024
    ei = _uniform(n, 9000, 9, 11)
    otab, _ = oracle.build_hash_tables(n, ei, H, P, prm)
    blocks = R.EdgeBlocks(torch.from_numpy(ei), n, max_edges=997, max_rows=300)
    for r in (W, 2 * W + 3, n - 12):
        for k in (1, 2):
            t = _as_torch(otab)
            mh, hll = t[k][0].clone(), t[k][1].clone()
            assert not torch.equal(mh[r], mh[r - W]) and not torch.equal(hll[r], hll[r - W])
            mh[r] = mh[r - W]
            bad_mh, bad_hll = R.hop_mismatches(blocks, t[k - 1][0], t[k - 1][1], mh, hll)
            assert bad_mh.tolist() == [r] and bad_hll.tolist() == []
            hll[r] = hll[r - W]
            mh[r] = t[k][0][r]
            bad_mh, bad_hll = R.hop_mismatches(blocks, t[k - 1][0], t[k - 1][1], mh, hll)
            assert bad_mh.tolist() == [] and bad_hll.tolist() == [r]
    # one element of one row, the smallest corruption there is
    t = _as_torch(otab)
    mh = t[2][0].clone()
    mh[777, 127] ^= 1
    assert R.hop_mismatches(blocks, t[1][0], t[1][1], mh, t[2][1])[0].tolist() == [777]
    # hop 0: a row shifted by W
    mh0, hll0 = t[0][0].clone(), t[0][1].clone()
    mh0[W + 5] = mh0[5]
    assert R.hop0_mismatches(oracle, mh0, hll0, n, [W, 2 * W], HLL_P, width=256) == [W + 5]
    assert R.describe_row(W + 5, [W, 2 * W]) == f'row {W + 5}: below row 2048 = 2^11 (-1019)'
    assert R.describe_row(2 * W, [W, 2 * W]) == 'row 2048: at or above row 2048 = 2^11 (+0)'
    assert 'first row 1029' in R.report([W + 5, 2 * W], [W, 2 * W], 'MinHash hop 1')
    assert R.report([], [W], 'x') == ''


def test_windows():
    assert R.windows(10000, [4096], width=512) == [(0, 512), (3840, 4352), (9488, 10000)]
    assert R.windows(300, [256], width=512) == [(0, 300)]


def test_boundary_graph_keeps_its_promises(prm):
    """the generator of the large-table tests at host scale: window rows have neighbours on both sides of their boundary, the hubs
    sit above the highest boundary with the in-degrees asked for, the last 7 nodes but one are isolated, N - 1 is the mega hub's
    neighbour; and the restatement agrees with the oracle on it"""
    from oracle import oracle
    n, bounds, w = 6000, [1024, 2048], 64
    g = R.boundary_graph(n, bounds, torch.device('cpu'), seed=3, window=w, hub_degree=150, mega_degree=1100)
    assert torch.equal(g.edge_index, R.boundary_graph(n, bounds, torch.device('cpu'), seed=3, window=w, hub_degree=150,
                                                      mega_degree=1100).edge_index), 'seeded'
    ei = g.edge_index.numpy()
    deg = np.bincount(ei[1], minlength=n)
    for b in bounds:
        for v in (b - 1, b, b + 1, b - w, b + w - 1):
            nb = ei[0][ei[1] == v]
            assert (nb < b).sum() >= 10 and (nb >= b).sum() >= 10, (b, v)
    assert all(h > max(bounds) + w and deg[h] >= 150 for h in g.hubs) and len(g.hubs) == 3
    assert deg[g.mega] >= 1100 and g.mega > max(bounds)
    assert (ei[0][ei[1] == g.mega] >= max(bounds)).sum() >= 1100 and not deg[n - 8:n - 1].any()   # (+ a few background edges)
    assert deg[n - 1] >= 1 and set(ei[0][ei[1] == n - 1]) == {g.mega}
    only = R.boundary_graph(n, bounds, torch.device('cpu'), seed=3, window=w, background=0)
    deg_only = np.bincount(only.edge_index[1].numpy(), minlength=n)
    inside = np.zeros(n, dtype=bool)
    for b in bounds:
        inside[b - w:b + w] = True
    assert not deg_only[~inside].any() and deg_only[inside].min() >= 20
    otab, _ = oracle.build_hash_tables(n, ei, H, P, prm)
    t = _as_torch(otab)
    blocks = R.EdgeBlocks(g.edge_index, n, max_edges=2000, max_rows=500)
    for k in (1, 2):
        bad_mh, bad_hll = R.hop_mismatches(blocks, t[k - 1][0], t[k - 1][1], t[k][0], t[k][1])
        assert len(bad_mh) == 0 and len(bad_hll) == 0, k
