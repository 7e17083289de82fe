"""The self-row skip of the table hops, on the CPU (numpy restatement, tests/symmetric_self_restatement.py): the lemma holds row for
row on symmetric graphs, fails on the two asymmetric counter-examples the GPU test runs, and the symmetry sums of the CSR build are
zero exactly for symmetric multisets (any edge order) and non-zero for every single-edge perturbation."""
import numpy as np
import pytest

import symmetric_self_restatement as R


@pytest.mark.parametrize('hops', [2, 3])
@pytest.mark.parametrize('seed,kw', [
    (0, dict(n_active=40, e_und=60)),
    (1, dict(n_active=40, e_und=50, n_isolated_low=7)),                       # isolated ids below n_self
    (2, dict(n_active=30, e_und=40, leaves=12)),                              # leaves
    (3, dict(n_active=30, e_und=40, self_edges=9)),                           # explicit self edges (some on otherwise isolated nodes)
    (4, dict(n_active=30, e_und=40, duplicates=15)),                          # duplicates present in both directions
    (5, dict(n_active=60, e_und=45, n_isolated_low=3, self_edges=8, duplicates=10, leaves=6)),
])
def test_lemma_row_for_row(seed, kw, hops):
    rng = np.random.RandomState(100 + seed)
    ei, n = R.symmetric_graph(rng, **kw)
    n += 4  # ids above n_self: no self loop, no edge -- all-zero rows either way
    assert R.is_symmetric_multiset(ei) and R.symmetry_sums(ei) == (0, 0)
    keep, skip = R.build(ei, n, hops, skip=False), R.build(ei, n, hops, skip=True)
    for k in range(hops):
        for a, b in zip(keep[k], skip[k]):
            assert np.array_equal(a, b), f'hop {k + 1}'


def test_a_node_whose_only_in_edge_is_its_own_self_edge():
    ei = np.array([[0, 1, 3, 3], [1, 0, 3, 3]], dtype=np.int64)  # node 3: explicit self edge (twice) and nothing else; node 2 isolated
    keep, skip = R.build(ei, 5, 3, skip=False), R.build(ei, 5, 3, skip=True)
    for k in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(keep[k], skip[k]))


@pytest.mark.parametrize('graph', [R.ONE_DIRECTED_EDGE, R.PATH_MINUS_ONE_REVERSE], ids=['one_directed_edge', 'path_minus_one_reverse'])
def test_counter_examples_need_the_self_row(graph):
    """on these graphs skipping WOULD change a row -- so the GPU test that finds their tables equal to the oracle's shows that the
    symmetry word, not luck, kept the self row"""
    ei, n = graph
    assert not R.is_symmetric_multiset(ei)
    s0, s1 = R.symmetry_sums(ei)
    assert s0 != 0 and s1 != 0
    keep, skip = R.build(ei, n, 2, skip=False), R.build(ei, n, 2, skip=True)
    assert np.array_equal(keep[0][0], skip[0][0]) and np.array_equal(keep[0][1], skip[0][1])  # hop 1 never skips
    assert not np.array_equal(keep[1][0], skip[1][0]), 'MinHash hop 2 would not change'
    assert not np.array_equal(keep[1][1], skip[1][1]), 'HLL hop 2 would not change'


def test_hop_one_needs_the_self_row_even_on_symmetric_graphs():
    """hop-0 rows are functions of the id alone: the lemma does not start at hop 1"""
    ei, n = R.symmetric_graph(np.random.RandomState(7), n_active=20, e_und=30)
    rowptr, col = R.csr_by_destination(ei, n)
    x = R.hop0_minhash(n)
    assert not np.array_equal(R.hop(x, rowptr, col, n, np.minimum), R.hop(x, rowptr, col, n, np.minimum, skip=True))


def test_sums_are_zero_for_symmetric_multisets_in_any_order():
    rng = np.random.RandomState(11)
    ei, _ = R.symmetric_graph(rng, n_active=500, e_und=900, self_edges=40, duplicates=100, leaves=30)
    for _ in range(5):
        assert R.symmetry_sums(ei[:, rng.permutation(ei.shape[1])]) == (0, 0)
    assert R.symmetry_sums(np.zeros((2, 0), dtype=np.int64)) == (0, 0)
    assert R.symmetry_sums(np.array([[5, 5, 9], [5, 5, 9]])) == (0, 0)  # self edges alone
    big = np.array([[0, (1 << 31) - 1], [(1 << 31) - 1, 0]], dtype=np.int64)  # the largest id the builder takes
    assert R.symmetry_sums(big) == (0, 0) and R.symmetry_sums(big[:, :1]) != (0, 0)


def test_sums_are_nonzero_for_200_single_edge_perturbations():
    rng = np.random.RandomState(12)
    und = rng.randint(0, 300, size=(2, 1000)).astype(np.int64)
    ei = np.concatenate([und, und[::-1]], axis=1)  # 2 000 edges
    assert R.symmetry_sums(ei) == (0, 0)
    done = 0
    while done < 200:
        kind, e = ('drop', 'redirect', 'duplicate')[done % 3], rng.randint(ei.shape[1])
        if kind == 'drop':
            pert = np.delete(ei, e, axis=1)
        elif kind == 'redirect':
            pert = ei.copy()
            pert[rng.randint(2), e] = rng.randint(0, 300)
        else:
            pert = np.concatenate([ei, ei[:, e:e + 1]], axis=1)
        if R.is_symmetric_multiset(pert):  # (a self edge dropped or duplicated, an endpoint redirected to itself: still symmetric)
            assert R.symmetry_sums(pert) == (0, 0)
            continue
        s0, s1 = R.symmetry_sums(pert)
        assert s0 != 0 and s1 != 0, (kind, e)
        done += 1


def test_byte_model_without_the_self_rows():
    """roofline: symmetric=True removes exactly the N self-row gathers from the three table-hop entries, the defaults stay"""
    import subgraph_sketching_amd as ssa
    N, E, B = 235868, 2358104, 65536
    old, new = ssa.roofline.kernel_bytes(N, E, B=B), ssa.roofline.kernel_bytes(N, E, B=B, symmetric=True)
    assert old == ssa.roofline.kernel_bytes(N, E, B=B, symmetric=False)
    assert old['minhash_hop'] - new['minhash_hop'] == N * 128 * 4
    assert old['hll_hop'] - new['hll_hop'] == N * 256
    assert old['fused_first_hop_hll_hop'] - new['fused_first_hop_hll_hop'] == N * 256
    for key in old:
        if key not in ('minhash_hop', 'hll_hop', 'fused_first_hop_hll_hop'):
            assert old[key] == new[key], key
    hubs = dict(hub_edges=100000, hub_rows=40)  # hub units keep their self row: only the regular rows' gathers go
    assert (ssa.roofline.kernel_bytes(N, E, B=B, **hubs)['minhash_hop']
            - ssa.roofline.kernel_bytes(N, E, B=B, symmetric=True, **hubs)['minhash_hop']) == (N - 40) * 128 * 4
    rb = ssa.roofline.minhash_rows_bytes
    assert rb(N, E, 1000) == rb(N, E, 1000, symmetric=False) and rb(N, E, 1000) - rb(N, E, 1000, symmetric=True) == 1000 * 128 * 4
