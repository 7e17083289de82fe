"""heuristics.CN / AA / RA (csrc/ss_heuristics.hip) on the GPU against the reference's own expressions restated in scipy
(tests/heuristics_restatement.py) and against the CPU oracle.  Float32 matrices -- what HashDataset builds from a float
edge_weight -- must match bit for bit: scipy keeps them in float32 and sums each pair's terms in numpy's pairwise order.  Int
and bool matrices keep CN exact, and every fp64-summed score stays within one float32 ulp of the oracle."""
import numpy as np
import pytest
import torch

import heuristics_restatement as hr

pytestmark = pytest.mark.gpu

KINDS = ('CN', 'AA', 'RA')


@pytest.fixture(scope='module')
def hz():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m.heuristics


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _ulp_close(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool(np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))))


def _assert_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, f'{what}: {len(bad)} of {len(got)} differ, first {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}'


@pytest.fixture(scope='module')
def shared():
    return hr.shared_count_graph()


@pytest.fixture(scope='module')
def powerlaw():
    """50 000 nodes, rows above 3 000 entries, links among the 200 largest rows (hub-hub pairs with thousands of terms)"""
    n = 50000
    src, dst = hr.powerlaw_graph(n, 300000, 31)
    rng = np.random.RandomState(32)
    links = np.concatenate([rng.randint(0, n, size=(60000, 2)), rng.randint(0, 200, size=(6000, 2)),
                            np.repeat(rng.randint(0, n, size=200), 2).reshape(-1, 2)]).astype(np.int64)
    return src, dst, links, n


@pytest.mark.parametrize('weighting', ['unit', 'random', 'small', 'colsum_one', 'zeros'])
def test_float32_is_bit_exact_on_chosen_term_counts(hz, dev, shared, weighting):
    """pairs of 1, 7, 8, 9, 127-130, 255-257, 1000, 3001 and 5000 terms both ways round, self pairs, isolated nodes"""
    src, dst, links, n = shared
    A = hr.matrix(src, dst, hr.weights(weighting, src, dst, n, 11), n, weighting)
    assert A.dtype == np.float32
    adj = hz.DeviceAdjacency(A, dev)
    for kind in KINDS:
        want = hr.scores(A, links, kind)
        got = getattr(hz, kind)(adj, torch.from_numpy(links).to(dev))[0].cpu().numpy()
        _assert_bits(got, want, f'{weighting} {kind}')
        # the same through the caller's matrix, CPU links and a batch size that cuts through every pair group
        again = getattr(hz, kind)(A, torch.from_numpy(links), batch_size=97)[0].numpy()
        _assert_bits(again, want, f'{weighting} {kind} batched')


@pytest.mark.parametrize('weighting', ['unit', 'random'])
def test_float32_is_bit_exact_on_a_power_law_graph(hz, dev, powerlaw, weighting):
    src, dst, links, n = powerlaw
    A = hr.matrix(src, dst, hr.weights(weighting, src, dst, n, 12), n)
    assert np.diff(A.indptr).max() > 3000
    adj = hz.DeviceAdjacency(A, dev)
    for kind in KINDS:
        want = hr.scores(A, links, kind)
        assert (want > 0).sum() > 5000
        got = getattr(hz, kind)(adj, torch.from_numpy(links).to(dev), batch_size=100000)[0].cpu().numpy()
        _assert_bits(got, want, f'powerlaw {weighting} {kind}')


def test_other_dtypes_against_the_oracle(hz, dev, shared):
    """int32 and bool: CN exact; int32 / bool / float64: AA and RA within one float32 ulp of the oracle, and of the restatement"""
    from oracle import oracle
    src, dst, links, n = shared
    rng = np.random.RandomState(13)
    mats = {'int32': hr.matrix(src, dst, rng.randint(1, 5, size=len(src)).astype(np.int32), n),
            'bool': hr.matrix(src, dst, np.ones(len(src), dtype=bool), n),
            'float64': hr.matrix(src, dst, 10.0 ** rng.uniform(-3, 3, size=len(src)), n)}
    for name, A in mats.items():
        adj = hz.DeviceAdjacency(A, dev)
        for kind in KINDS:
            got = getattr(hz, kind)(adj, torch.from_numpy(links).to(dev))[0].cpu().numpy()
            want = oracle.common_neighbour_scores(A, links, kind)
            if kind == 'CN' and name != 'float64':
                assert np.array_equal(got, want), (name, kind)
                assert np.array_equal(got, hr.scores(A, links, kind)), (name, kind)
            else:
                assert _ulp_close(got, want), (name, kind)
                assert _ulp_close(got, hr.scores(A, links, kind)), (name, kind)


def test_int_matrix_of_the_power_law_graph_against_the_oracle(hz, dev, powerlaw):
    from oracle import oracle
    src, dst, links, n = powerlaw
    w = np.random.RandomState(14).randint(1, 5, size=len(src)).astype(np.int64)
    A = hr.matrix(src, dst, w, n)
    for kind in KINDS:
        got = getattr(hz, kind)(A, torch.from_numpy(links).to(dev))[0].cpu().numpy()
        want = oracle.common_neighbour_scores(A, links, kind)
        if kind == 'CN':
            assert np.array_equal(got, want)
        else:
            assert _ulp_close(got, want), kind
            assert (got == want).mean() > 0.9999, kind


def test_float32_kernel_matches_the_oracle_float32_mode(hz, dev, powerlaw):
    """the oracle's float32 mode is the same arithmetic (pinned to scipy by tests/test_heuristics_host.py)"""
    from oracle import oracle
    src, dst, links, n = powerlaw
    A = hr.matrix(src, dst, hr.weights('small', src, dst, n, 15), n)
    for kind in KINDS:
        got = getattr(hz, kind)(A, torch.from_numpy(links).to(dev))[0].cpu().numpy()
        _assert_bits(got, oracle.common_neighbour_scores(A, links, kind), kind)
