"""The self-row skip of the table hops on the GPU: the symmetry word of the CSR build, bit-identity of every table with the skip on
and off (SS_SELF_SKIP=0) and against the oracle on symmetric graphs, asymmetric graphs left alone, and the permission bit.

Float comparisons against the oracle use the project's end-to-end tolerances (__graft_entry__.smoke: cards rtol 1e-5 / atol 1e-4,
features rtol 1e-5 / atol 2e-2 -- the oracle's own float error); everything between the two paths of the library is torch.equal."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import oracle_params
import symmetric_self_restatement as R

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


def _eh(ssa, h=2, P=128):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    eh.hll_tables = ssa.hll_tables.load(8, prefer='regenerated')
    return eh


def _sym(n, e_und, seed):
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    return np.concatenate([e, e[::-1]], axis=1)


def _word(ssa, dev, ei, n, **kw):
    csr = ssa.hashing.build_csr(torch.from_numpy(np.ascontiguousarray(ei)).to(dev), n, dev, check=False, **kw)
    return int(csr.symmetric.item()), csr


# ---- the word -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,e_und', [(5000, 20000), (300000, 600000)], ids=['one_level', 'two_levels'])
def test_symmetry_word(ssa, dev, n, e_und):
    rng = np.random.RandomState(3)
    ei = _sym(n, e_und, 31)
    assert ssa._native.lib().ss_csr_workspace_bytes(n, ei.shape[1]) > 0
    assert _word(ssa, dev, ei, n)[0] == 1
    assert _word(ssa, dev, ei[:, rng.permutation(ei.shape[1])], n)[0] == 1                       # shuffled
    dup = ei[:, rng.choice(e_und, size=e_und // 10, replace=False)]
    assert _word(ssa, dev, np.concatenate([ei, dup, dup[::-1]], axis=1), n)[0] == 1              # balanced duplicates
    k = int(np.flatnonzero(ei[0] != ei[1])[17])
    assert _word(ssa, dev, np.delete(ei, k, axis=1), n)[0] == 0                                  # one reverse edge missing
    assert _word(ssa, dev, np.concatenate([ei, ei[:, k:k + 1]], axis=1), n)[0] == 0              # one direction once more than the other
    loops = rng.randint(0, n, size=1000).astype(np.int64)
    assert _word(ssa, dev, np.stack([loops, loops]), n)[0] == 1                                  # only self edges
    # no edge: no row has a neighbour that could stand in for its self row -- the build says 0, "nothing to skip" (ss_csr_build_symmetric)
    assert _word(ssa, dev, np.zeros((2, 0), dtype=np.int64), n)[0] == 0
    bad = ei.copy()
    bad[:, 5] = (n + 3, 7)
    bad[:, 5 + e_und] = (7, n + 3)                                                               # symmetric, but an id out of range
    assert _word(ssa, dev, bad, n)[0] == 0


def test_symmetry_word_survives_a_reused_build_and_follows_an_edit(ssa, dev):
    n = 6000
    ei = torch.from_numpy(_sym(n, 25000, 32)).to(dev)
    csr = ssa.hashing.build_csr(ei, n, dev, check=False, fingerprint=True)
    skipped = lambda: int(csr.fingerprint.view(torch.int32)[5].item())  # FingerprintWords.skip of the last build
    assert int(csr.symmetric.item()) == 1 and skipped() == 0
    again = ssa.hashing.build_csr(ei.clone(), n, dev, check=False, reuse=csr, fingerprint=True)
    assert again is csr and skipped() == 1 and int(csr.symmetric.item()) == 1      # content unchanged: the word of the kept build
    k = int(torch.nonzero(ei[0] != ei[1])[5])
    ei[:, k] = ei[0, k]                                                             # the edge becomes a self edge: its reverse stands alone
    again = ssa.hashing.build_csr(ei, n, dev, check=False, reuse=csr, fingerprint=True)
    assert again is csr and skipped() == 0 and int(csr.symmetric.item()) == 0


# ---- bit-identity on symmetric graphs -----------------------------------------------------------------------------------------------
def _star_graph():
    """5 000 random nodes + a centre above the default hub threshold (300 leaves) and one above 4 096 neighbours (4 200 leaves: a
    mega row); hub units keep the self row, the regular rows of the same launch skip it"""
    base = _sym(5000, 20000, 41)
    a, b, first = 10, 20, 5000
    la, lb = np.arange(first, first + 300), np.arange(first + 300, first + 4500)
    und = np.concatenate([np.stack([np.full(300, a), la]), np.stack([np.full(4200, b), lb])], axis=1).astype(np.int64)
    return np.concatenate([base, und, und[::-1]], axis=1), first + 4500


def _isolated_middle():
    ei = _sym(5000, 20000, 42)
    ei = ei[:, ((ei[0] < 2400) | (ei[0] >= 2600)) & ((ei[1] < 2400) | (ei[1] >= 2600))]  # 200 ids in the middle occur in no edge
    return ei, 5000


def _only_self_edge():
    ei = _sym(1000, 3000, 43)
    ei = ei[:, (ei[0] != 77) & (ei[1] != 77) & (ei[0] != 500) & (ei[1] != 500)]
    return np.concatenate([ei, np.array([[77, 500, 500], [77, 500, 500]])], axis=1), 1000  # nodes 77 / 500: their self edge (twice) alone


def _tiny(n):
    ei = _sym(n, max(1, 3 * n), 50 + n)
    return ei, n


CASES = {
    'n1': lambda: _tiny(1) + (2, 128), 'n2': lambda: _tiny(2) + (2, 128), 'n63': lambda: _tiny(63) + (2, 128),
    'n64': lambda: _tiny(64) + (3, 128), 'n65': lambda: _tiny(65) + (2, 128),
    'n5000_h2': lambda: (_sym(5000, 20000, 44), 5000, 2, 128), 'n5000_h3': lambda: (_sym(5000, 20000, 44), 5000, 3, 128),
    'P64': lambda: (_sym(5000, 20000, 45), 5000, 3, 64), 'P256': lambda: (_sym(5000, 20000, 46), 5000, 2, 256),
    'isolated_middle': lambda: _isolated_middle() + (3, 128), 'hub_and_mega': lambda: _star_graph() + (3, 128),
    'only_self_edge': lambda: _only_self_edge() + (3, 128),
}


def _build(ssa, dev, ei, n, h, P, links):
    eh = _eh(ssa, h=h, P=P)
    table, cards = eh.build_hash_tables(n, torch.from_numpy(ei).to(dev))
    feats = eh.get_subgraph_features(links, table, cards)
    torch.cuda.synchronize()
    return [(table[k].mh_u32.clone(), table[k].hll_u8.clone()) for k in range(1, h + 1)], cards.clone(), feats.clone()


def _check_against_oracle(ssa, regenerated_tables, ei, n, h, P, links, got):
    from oracle import oracle
    prm = oracle_params(regenerated_tables[8])
    otab, ocards = oracle.build_hash_tables(n, ei, h, P, prm)
    tables, cards, feats = got
    for k in range(1, h + 1):
        assert np.array_equal(tables[k - 1][0].cpu().numpy().view(np.uint32), otab[k]['minhash']), f'minhash hop {k}'
        assert np.array_equal(tables[k - 1][1].cpu().numpy(), otab[k]['hll']), f'hll hop {k}'
    np.testing.assert_allclose(cards.cpu().numpy(), ocards, rtol=1e-5, atol=1e-4)
    ofeat = oracle.pair_features(links.cpu().numpy(), otab, ocards, h, prm)
    np.testing.assert_allclose(feats.cpu().numpy(), ofeat, rtol=1e-5, atol=2e-2)


@pytest.mark.parametrize('case', sorted(CASES))
def test_skip_is_bit_identical_on_symmetric_graphs(ssa, dev, regenerated_tables, monkeypatch, case):
    ei, n, h, P = CASES[case]()
    assert R.is_symmetric_multiset(ei)
    assert _word(ssa, dev, ei, n)[0] == 1
    links = torch.from_numpy(np.random.RandomState(9).randint(0, n, size=(4096, 2)).astype(np.int64)).to(dev)
    monkeypatch.delenv('SS_SELF_SKIP', raising=False)
    on = _build(ssa, dev, ei, n, h, P, links)
    monkeypatch.setenv('SS_SELF_SKIP', '0')
    off = _build(ssa, dev, ei, n, h, P, links)
    monkeypatch.delenv('SS_SELF_SKIP')
    for k in range(h):
        assert torch.equal(on[0][k][0], off[0][k][0]), f'minhash hop {k + 1}'
        assert torch.equal(on[0][k][1], off[0][k][1]), f'hll hop {k + 1}'
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    _check_against_oracle(ssa, regenerated_tables, ei, n, h, P, links, on)


# ---- asymmetric graphs are left alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['one_directed_edge', 'path_minus_one_reverse', 'random_directed'])
def test_asymmetric_graphs_keep_the_self_row(ssa, dev, regenerated_tables, monkeypatch, case):
    """the first two are the graphs test_symmetric_self_host shows a skip WOULD change"""
    monkeypatch.delenv('SS_SELF_SKIP', raising=False)
    if case == 'random_directed':
        ei, n = np.random.RandomState(61).randint(0, 5000, size=(2, 20000)).astype(np.int64), 5000
    else:
        ei, n = R.ONE_DIRECTED_EDGE if case == 'one_directed_edge' else R.PATH_MINUS_ONE_REVERSE
    assert not R.is_symmetric_multiset(ei)
    assert _word(ssa, dev, ei, n)[0] == 0
    links = torch.from_numpy(np.random.RandomState(9).randint(0, n, size=(4096, 2)).astype(np.int64)).to(dev)
    for h in (2, 3):
        _check_against_oracle(ssa, regenerated_tables, ei, n, h, 128, links, _build(ssa, dev, ei, n, h, 128, links))


# ---- the permission bit is required ---------------------------------------------------------------------------------------------------
def test_nothing_is_skipped_without_the_permission_bit(ssa, dev, monkeypatch):
    """hop-0 rows and arbitrary tensors do not satisfy the lemma: the drop-in propagation modules and a table hop without
    SS_GRAPH_HOP_TABLES give the with-self result on a symmetric graph; WITH the bit the same call on a random tensor differs (the
    switch is live, this test is not vacuous)"""
    from oracle import oracle
    monkeypatch.delenv('SS_SELF_SKIP', raising=False)
    H = ssa.hashing
    n = 3000
    ei = _sym(n, 9000, 71)
    ei_loops = oracle.add_self_loops(ei)
    eh = _eh(ssa, h=2)
    rng = np.random.RandomState(72)
    mh_rand = rng.randint(0, 1 << 32, size=(n, 128), dtype=np.int64)
    hll_rand = rng.randint(0, 50, size=(n, 256)).astype(np.int8)
    mh0, hll0 = eh.initialise_minhash(n).to(dev), eh.initialise_hll(n).to(dev)
    t_loops = torch.from_numpy(ei_loops).to(dev)
    for mh_x, hll_x in ((mh0, hll0), (torch.from_numpy(mh_rand).to(dev), torch.from_numpy(hll_rand).to(dev))):
        want_mh, want_hll = oracle.propagate(n, ei_loops, mh_x.cpu().numpy().astype(np.uint32), hll_x.cpu().numpy().view(np.uint8))
        got_mh = H._packed_minhash_of(H.MinhashPropagation()(mh_x, t_loops), dev)
        got_hll = H.HllPropagation()(hll_x, t_loops)
        assert np.array_equal(got_mh.cpu().numpy().view(np.uint32), want_mh)
        assert np.array_equal(got_hll.cpu().numpy().view(np.uint8), want_hll)
    # the C ABI with the word and the inferred self loops in place, on random tensors: without the bit the self row is gathered
    word, csr = _word(ssa, dev, ei, n)
    assert word == 1
    csr.use_inferred_self_loops = True
    mh_in = torch.from_numpy(mh_rand.astype(np.uint32).view(np.int32)).to(dev)
    hll_in = torch.from_numpy(hll_rand.view(np.uint8)).to(dev)
    want_mh, want_hll = oracle.propagate(n, ei_loops, mh_rand.astype(np.uint32), hll_rand.view(np.uint8))
    for P_cols in (128, 64):  # the fast kernels and the generic one
        got_mh, got_hll = H._propagate(csr, mh_in[:, :P_cols].contiguous(), hll_in, dev)
        assert np.array_equal(got_mh.cpu().numpy().view(np.uint32), want_mh[:, :P_cols]) and np.array_equal(got_hll.cpu().numpy(), want_hll)
        skip_mh, skip_hll = H._propagate(csr, mh_in[:, :P_cols].contiguous(), hll_in, dev, hop_tables=True)
        assert not torch.equal(skip_mh, got_mh) and not torch.equal(skip_hll, got_hll)
        monkeypatch.setenv('SS_SELF_SKIP', '0')  # ... and the library-side switch overrides the bit
        off_mh, off_hll = H._propagate(csr, mh_in[:, :P_cols].contiguous(), hll_in, dev, hop_tables=True)
        monkeypatch.delenv('SS_SELF_SKIP')
        assert torch.equal(off_mh, got_mh) and torch.equal(off_hll, got_hll)
