"""Negative sampling on the GPU (csrc/ss_negatives.hip, negatives.py): NegativeSampler.sample / sample_negatives against
the Python restatement of their semantics (negatives_restatement.py).  "Equal" means the whole int64 [n_slots, 2] tensor and the
unsampled count, exactly.  The graph (400 nodes: a random part, a hub, a K5, a star, isolated nodes, a doubled edge) is the one
test_negatives_host.py checks the restatement on.  The wedge mode runs on a small DIRECTED graph as well (directed_graph: neighbours
without an out-arc, which a symmetric graph does not have).

Run on an MI355X: profiles/wedge_planted_tests.txt."""
from argparse import Namespace
import functools

import numpy as np
import pytest
import torch

import negatives_restatement as restated

pytestmark = pytest.mark.gpu

N, EI = restated.negatives_graph()
NODES = np.stack([np.arange(N), (np.arange(N) * 7 + 1) % N], axis=1).astype(np.int64)  # every node, an arbitrary second column
POSITIVES = {'nodes': NODES, 'edges': np.ascontiguousarray(EI.T[:257]), 'both': np.concatenate([NODES, EI.T[:257]])}
HELD_OUT = np.array([[0, 0, 3, 388, 17, -1], [1, 2, 4, 389, -5, 6]], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def want(which, num_neg, mode, seed, exclude=False, max_tries=16):
    """the restatement's (rows, unsampled) for a case, computed once and shared (read only)"""
    rows, unsampled = restated.sample(N, EI, POSITIVES[which], num_neg=num_neg, mode=mode, seed=seed, max_tries=max_tries,
                                      exclude=HELD_OUT if exclude else None)
    rows.setflags(write=False)
    return rows, unsampled


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sampler(ssa, dev):
    return ssa.NegativeSampler(N, torch.from_numpy(EI.copy()).to(dev))


@pytest.fixture(scope='module')
def filtered(ssa, dev):
    return ssa.NegativeSampler(N, torch.from_numpy(EI.copy()).to(dev), exclude=torch.from_numpy(HELD_OUT).to(dev))


def _equal(got, expected, where):
    out, info = got
    rows, unsampled = expected
    assert out.dtype == torch.int64 and out.shape == rows.shape and out.device == where
    np.testing.assert_array_equal(out.cpu().numpy(), rows)
    assert info == {'unsampled': unsampled}


def test_the_rows_are_sorted_with_their_duplicates(sampler):
    rowptr, col = sampler.graph.rowptr.cpu().numpy(), sampler.graph.col.cpu().numpy()
    rows = restated.rows_of(N, EI)
    assert rowptr.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
    assert col[:rowptr[-1]].tolist() == [v for r in rows for v in r]
    assert rows[3].count(5) == 2 and len(rows[382]) >= 150


@pytest.mark.parametrize('which', ['nodes', 'edges', 'both'])
@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('num_neg', [1, 3])
@pytest.mark.parametrize('mode', restated.MODES)
def test_samples_equal_the_restatement(sampler, dev, mode, num_neg, seed, which):
    pos = torch.from_numpy(POSITIVES[which]).to(dev)
    expected = want(which, num_neg, mode, seed)
    if which == 'edges' and num_neg == 3:
        assert expected[0].shape[0] == 771  # crosses a workgroup boundary
    assert (expected[0][:, 1] >= 0).mean() > 0.5, 'a trivial expectation checks nothing'
    _equal(sampler.sample(pos, num_neg=num_neg, mode=mode, seed=seed, return_info=True), expected, dev)


def test_any_source_uniform(sampler, dev):
    rows, unsampled = restated.sample(N, EI, None, mode='uniform', seed=4, num_samples=1000)
    assert len(set(rows[:, 0].tolist())) > 300
    _equal(sampler.sample(mode='uniform', seed=4, num_samples=1000, return_info=True), (rows, unsampled), dev)
    split = sampler.sample(mode='uniform', seed=4, num_samples=1000, batch_size=300)
    np.testing.assert_array_equal(split.cpu().numpy(), rows)


@pytest.mark.parametrize('mode', restated.MODES)
def test_an_exclude_list_is_never_returned(filtered, sampler, dev, mode):
    pos = torch.from_numpy(POSITIVES['nodes']).to(dev)
    expected = want('nodes', 3, mode, 1, exclude=True)
    got = filtered.sample(pos, num_neg=3, mode=mode, seed=1, return_info=True)
    _equal(got, expected, dev)
    gone = {(int(u) % N, int(v) % N) for u, v in HELD_OUT.T}
    assert not gone & set(map(tuple, got[0].cpu().tolist()))
    if mode == 'wedge':  # the list changes something: without it a held-out wedge comes back
        free = sampler.sample(pos, num_neg=3, mode=mode, seed=1)
        assert gone & set(map(tuple, free.cpu().tolist()))


@pytest.mark.parametrize('mode', restated.MODES)
def test_negative_ids_batches_seeds_and_devices(ssa, sampler, dev, mode):
    pos_np = POSITIVES['both']
    pos = torch.from_numpy(pos_np).to(dev)
    expected = want('both', 3, mode, 0)
    first = sampler.sample(pos, num_neg=3, mode=mode, seed=0, return_info=True)
    _equal(first, expected, dev)
    # negative ids give what the wrapped ids give
    shifted = pos.clone()
    shifted[::2] -= N
    _equal(sampler.sample(shifted, num_neg=3, mode=mode, seed=0, return_info=True), expected, dev)
    # a split call (64 and 300 are no multiples of num_neg: launches start inside a positive)
    for batch_size in (64, 300):
        _equal(sampler.sample(pos, num_neg=3, mode=mode, seed=0, batch_size=batch_size, return_info=True), expected, dev)
    # one seed, one result; another seed, another
    assert torch.equal(sampler.sample(pos, num_neg=3, mode=mode, seed=0), first[0])
    other = sampler.sample(pos, num_neg=3, mode=mode, seed=1)
    np.testing.assert_array_equal(other.cpu().numpy(), want('both', 3, mode, 1)[0])
    assert not torch.equal(other, first[0])
    # a view with other strides (the transposed [2, L] layout of an edge_index) is read in place
    assert torch.equal(sampler.sample(pos.t().contiguous().t(), num_neg=3, mode=mode, seed=0), first[0])
    # CPU positives: the result comes back on the CPU
    on_cpu = sampler.sample(torch.from_numpy(pos_np), num_neg=3, mode=mode, seed=0, return_info=True)
    _equal(on_cpu, expected, torch.device('cpu'))
    # no positives: an empty result
    none = sampler.sample(pos[:0], num_neg=3, mode=mode, seed=0, return_info=True)
    assert none[0].shape == (0, 2) and none[0].dtype == torch.int64 and none[1] == {'unsampled': 0}
    # the one-shot function is the reused sampler
    _equal(ssa.sample_negatives(N, torch.from_numpy(EI.copy()).to(dev), pos, num_neg=3, mode=mode, seed=0, return_info=True), expected, dev)
    _equal(ssa.sample_negatives(N, torch.from_numpy(EI.copy()), torch.from_numpy(pos_np), num_neg=3, mode=mode, seed=0, return_info=True),
           expected, torch.device('cpu'))


def test_max_tries_reaches_the_kernel(sampler, dev):
    """one attempt per slot: many more slots stay unsampled, and they are the restatement's"""
    pos = torch.from_numpy(POSITIVES['nodes']).to(dev)
    expected = want('nodes', 3, 'wedge', 0, max_tries=1)
    assert expected[1] > want('nodes', 3, 'wedge', 0)[1]
    _equal(sampler.sample(pos, num_neg=3, mode='wedge', seed=0, max_tries=1, return_info=True), expected, dev)


# ---- a directed graph: neighbours without an out-arc ---------------------------------------------------------------------------------
DN, DEI = restated.directed_graph()
DPOS = np.stack([np.arange(DN), np.arange(DN)[::-1]], axis=1).astype(np.int64)  # every node as a source: the planted ones among them


@pytest.fixture(scope='module')
def directed(ssa, dev):
    return ssa.NegativeSampler(DN, torch.from_numpy(DEI.copy()).to(dev))


@pytest.mark.parametrize('max_tries', [1, 4, 16])
@pytest.mark.parametrize('num_neg', [1, 3, 7])
def test_wedge_on_a_directed_graph(directed, dev, num_neg, max_tries):
    """a neighbour w without an out-arc ends the attempt, not the slot: the source of sinks alone is unsampled in every slot"""
    expected = restated.sample(DN, DEI, DPOS, num_neg=num_neg, mode='wedge', seed=2, max_tries=max_tries)
    src = restated.DIRECTED_SOURCES
    by_source = expected[0][:, 1].reshape(DN, num_neg)
    assert (by_source[[src['all_sinks'], src['rejected'], src['no_out_arc']]] == -1).all() and (by_source[src['repeated']] >= 0).any()
    assert max_tries == 1 or (by_source[src['mixed']] >= 0).any()
    _equal(directed.sample(torch.from_numpy(DPOS).to(dev), num_neg=num_neg, mode='wedge', seed=2, max_tries=max_tries, return_info=True),
           expected, dev)
    if (num_neg, max_tries) == (7, 4):  # launches that start inside a positive
        _equal(directed.sample(torch.from_numpy(DPOS).to(dev), num_neg=7, mode='wedge', seed=2, max_tries=4, batch_size=5, return_info=True),
               expected, dev)


@pytest.mark.parametrize('mode', ['uniform', 'same_source'])
def test_the_other_modes_on_a_directed_graph(directed, dev, mode):
    expected = restated.sample(DN, DEI, DPOS, num_neg=3, mode=mode, seed=2)
    assert (expected[0][:, 1] >= 0).all()
    _equal(directed.sample(torch.from_numpy(DPOS).to(dev), num_neg=3, mode=mode, seed=2, return_info=True), expected, dev)


def test_ids_out_of_range(ssa, dev):
    sampler = ssa.NegativeSampler(N, torch.from_numpy(EI.copy()).to(dev))
    good = sampler.sample(torch.tensor([[0, 1], [5, 1]], device=dev), num_neg=2, seed=3)
    # device ids: reported late, as the link queries report them; the bad slots are (the id as given, -1), the others untouched
    got, info = sampler.sample(torch.tensor([[0, 1], [N, 1], [5, 1]], device=dev), num_neg=2, seed=3, batch_size=3, return_info=True)
    with pytest.raises(IndexError):
        sampler.check_errors()
    sampler.check_errors()  # (reported once)
    assert got[2:4].tolist() == [[N, -1], [N, -1]] and info['unsampled'] >= 2
    assert torch.equal(got[:2], good[:2])
    sampler.sample(torch.tensor([[-N - 1, 1]], device=dev))
    torch.cuda.synchronize()
    with pytest.raises(IndexError):  # ... at the next call, once the launch has finished
        sampler.sample(torch.tensor([[0, 1]], device=dev))
    with pytest.raises(IndexError):  # CPU ids: at once
        sampler.sample(torch.tensor([[N, 0]]))
    sampler.strict_bounds = True
    with pytest.raises(IndexError):
        sampler.sample(torch.tensor([[N, 0]], device=dev))
    sampler.strict_bounds = False
    assert torch.equal(sampler.sample(torch.tensor([[0, 1], [N, 1], [5, 1]], device=dev), num_neg=2, seed=3), got)
    with pytest.raises(IndexError):  # the one-shot form has no later call to report at
        ssa.sample_negatives(N, torch.from_numpy(EI.copy()).to(dev), torch.tensor([[N, 0]], device=dev))
    with pytest.raises(IndexError):  # a graph with an id out of range, on the device
        ssa.NegativeSampler(N, torch.tensor([[0, 1], [1, N]], device=dev))


def test_sampled_negatives_feed_the_feature_query(ssa, sampler, dev):
    """dtype and layout match what get_subgraph_features takes: the wedge negatives of the graph through the query on tables built
    from the same edge_index"""
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    ei = torch.from_numpy(EI.copy()).to(dev)
    table, cards = eh.build_hash_tables(N, ei)
    neg = sampler.sample(ei.t()[:500], num_neg=2, mode='wedge', seed=9)
    neg = neg[neg[:, 1] >= 0]
    assert neg.shape[0] > 500 and neg.is_contiguous()
    feats = eh.get_subgraph_features(neg, table, cards)
    eh.check_errors()
    assert feats.shape == (neg.shape[0], 8) and bool(torch.isfinite(feats).all())
    # a wedge negative has a common neighbour: the (1, 1) intersection estimate of most of them is positive
    assert float((feats[:, 0] > 0).float().mean()) > 0.5
