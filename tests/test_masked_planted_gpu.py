"""ElphHashes.get_subgraph_features(mask_target=edge_index) on the planted inputs of tests/masked_planted.py (csrc/ss_masked.hip:
masked_classify_kernel, masked_row_zeros_kernel, masked_pairs_kernel).  References: the numpy restatement of the rule
(tests/masked_restatement.py, pinned on one oracle rebuild per link on these very graphs by tests/test_masked_planted_host.py) over the
oracle's full-graph tables, and the engine's own answer to the same link in a call where every workgroup serves one link.  Which links
were masked, match, zeros and row_zeros: exact.  Features: DESIGN 4's bar against the restatement, bit for bit between calls."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import masked_planted as mp
import masked_restatement as mr
from conftest import oracle_params
from oracle import oracle

pytestmark = pytest.mark.gpu

KEYS = ('match', 'zeros', 'row_zeros')


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.view(torch.int32)


_BUILT = {}


def built(ssa, dev, name, graph, h, num_perm, p):
    """the engine's tables and the oracle's of one planted graph at one shape, built once per module run"""
    key = (name, h, num_perm, p)
    if key not in _BUILT:
        n, ei = graph[0], graph[1]
        eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=num_perm, floor_sf=False, use_zero_one=True))
        prm = oracle_params(eh.hll_tables)
        ei_t = _t(ei, dev)
        table, cards = eh.build_hash_tables(n, ei_t)
        otab, ocards = oracle.build_hash_tables(n, ei, h, num_perm, prm)
        _BUILT[key] = Namespace(eh=eh, n=n, ei=ei, ei_t=ei_t, table=table, cards=cards, otab=otab, ocards=ocards, prm=prm, h=h,
                                num_perm=num_perm, p=p, M=1 << p, dev=dev, own={})
    return _BUILT[key]


def query(b, links, **kw):
    return b.eh.get_subgraph_features(_t(links, b.dev), b.table, b.cards, mask_target=b.ei_t, **kw)


def plain(b, links):
    return b.eh.get_subgraph_features(_t(links, b.dev), b.table, b.cards)


def check(b, links, expect_masked=None):
    """one masked call against the restatement on the oracle's full-graph tables -> (features, debug, the restatement's features)"""
    feats, dbg = query(b, links, return_debug=True)
    want, wdbg = mr.masked_query(links, b.n, b.ei, b.otab, b.ocards, b.h, b.prm)
    assert dbg['masked'].dtype == torch.bool and dbg['match'].dtype == torch.int32
    assert np.array_equal(dbg['masked'].cpu().numpy(), wdbg['masked'])
    if expect_masked is not None:
        assert wdbg['masked'].tolist() == list(expect_masked)
    for key in KEYS:
        got = dbg[key].cpu().numpy()
        bad = np.flatnonzero((got != wdbg[key]).reshape(len(got), -1).any(axis=1))
        assert not len(bad), (f'{key}: {len(bad)} of {len(got)} links differ, first {np.asarray(links)[bad[:5]].tolist()}: '
                              f'{got[bad[:2]].tolist()} != {wdbg[key][bad[:2]].tolist()}')
    got = feats.cpu().numpy()
    print(f'N={b.n} h={b.h} shape=({b.num_perm},{b.p}) links={len(got)} masked={int(wdbg["masked"].sum())} '
          f'max|feature diff|={float(np.abs(got - want).max()):.3g}')
    mr.assert_features_bar(got, want, b.ocards)
    b.eh.check_errors()
    return feats, dbg, want


# ---- 1. the families where the masked edge is the only path ------------------------------------------------------------------------------
@pytest.mark.parametrize('h', mp.HOPS)
@pytest.mark.parametrize('num_perm,p', mp.SHAPES)
def test_k2_bridges_and_cycles(ssa, dev, num_perm, p, h):
    n, ei, links, where, first = mp.small_forest()
    b = built(ssa, dev, 'small_forest', (n, ei), h, num_perm, p)
    feats, dbg, want = check(b, links, expect_masked=[True] * len(links))
    match, row_zeros = dbg['match'].cpu().numpy(), dbg['row_zeros'].cpu().numpy()
    for name, s in where.items():
        if mp.is_bridge(name):  # the two sides share nothing once the bridge is gone
            assert not match[s].any(), (name, match[s].tolist())
    assert (row_zeros[where['K2']] == b.M - 1).all() and (row_zeros[where['bridge(0,0)']] == b.M - 1).all()  # the own self loop, no more
    # a masked row is not the plain row: asserted on the engine's two answers wherever the two references lie further apart than
    # rounding can bring them (ten times the bar) -- which they do on every link here but the few where one id less moves no register
    ofeat = oracle.pair_features(links, b.otab, b.ocards, h, b.prm)
    apart = np.abs(want - ofeat).max(axis=1) > 10 * 1e-5 * (4 * float(np.abs(b.ocards).max()) + float(np.abs(ofeat).max()))
    differ = (_bits(feats) != _bits(plain(b, links))).any(dim=1).cpu().numpy()
    assert differ[apart].all() and apart[where['K2']].all() and apart.sum() >= len(links) - 4, (int(apart.sum()), len(links))


# ---- 2. the partner at every position of a scanned row ---------------------------------------------------------------------------------
@pytest.mark.parametrize('num_perm,p', [(128, 8), (8, 4)])
@pytest.mark.parametrize('variant', mp.POSITION_VARIANTS)
@pytest.mark.parametrize('L', mp.POSITION_L)
def test_every_position(ssa, dev, L, variant, num_perm, p):
    n, ei, links = mp.every_position(L, variant)
    b = built(ssa, dev, f'every_position({L},{variant})', (n, ei), 3, num_perm, p)
    feats, dbg, _ = check(b, links, expect_masked=[True] * (2 * L))
    assert bool(dbg['masked'].all())


# ---- 3. the hop-3 walk over rows of every planted length --------------------------------------------------------------------------------
@pytest.mark.parametrize('num_perm,p', mp.SHAPES)
def test_comb_at_three_hops(ssa, dev, num_perm, p):
    n, ei, links = mp.comb()
    b = built(ssa, dev, 'comb', (n, ei), 3, num_perm, p)
    check(b, links, expect_masked=[True] * len(links))


# ---- 4 .. 6. batch patterns ---------------------------------------------------------------------------------------------------------------
def batch(ssa, dev, h, num_perm=128, p=8):
    """the batch forest at one shape with the answers the distinct links and the non-edges get in small calls -- every workgroup of
    masked_pairs_kernel serves one link there, every scan takes one trip -- checked against the restatement"""
    n, ei, distinct, non = mp.batch_forest()
    b = built(ssa, dev, 'batch_forest', (n, ei), h, num_perm, p)
    if 'edges' not in b.own:
        feats, dbg, _ = check(b, distinct, expect_masked=[True] * len(distinct))
        b.own['edges'] = (feats, dbg)
        feats, dbg, _ = check(b, non, expect_masked=[False] * len(non))
        assert torch.equal(_bits(feats), _bits(plain(b, non)))
        b.own['non'] = (feats, dbg)
    return b, distinct, non


def expected(b, is_edge, which):
    """rows and debug integers of a batch, gathered from the small calls"""
    e, w = _t(is_edge, b.dev), _t(which, b.dev)
    (fe, de), (fn, dn) = b.own['edges'], b.own['non']
    we, wn = w.clamp(max=len(fe) - 1), w.clamp(max=len(fn) - 1)
    feats = torch.where(e[:, None], fe[we], fn[wn])
    dbg = {key: torch.where(e.view(-1, 1, 1), de[key][we], dn[key][wn]) for key in KEYS}
    dbg['masked'] = e
    return feats, dbg


def assert_same(got, dbg, want, wdbg, what=''):
    bad = (_bits(got) != _bits(want)).any(dim=1).nonzero().flatten()
    assert not len(bad), f'{what}: {len(bad)} of {len(got)} feature rows differ, first at {bad[:8].tolist()}'
    if dbg is not None:
        for key in wdbg:
            assert torch.equal(dbg[key], wdbg[key]), f'{what}: {key} differs at {(dbg[key] != wdbg[key]).nonzero()[:8].tolist()}'


@pytest.mark.parametrize('length', mp.WAVE_LENGTHS)
def test_wave_patterns(ssa, dev, length):
    b, distinct, non = batch(ssa, dev, 3)
    links, is_edge, which = mp.wave_patterns(length)
    got, dbg = query(b, links, return_debug=True)
    assert np.array_equal(dbg['masked'].cpu().numpy(), is_edge)
    keep = _t(~is_edge, dev)
    assert torch.equal(_bits(got)[keep], _bits(plain(b, links))[keep])  # a link that is not an edge keeps the plain query's bits
    for q in np.flatnonzero(is_edge).tolist():                           # an edge: the row of a call of its own
        i = int(which[q])
        if i not in b.own:
            b.own[i] = query(b, distinct[i:i + 1])
        assert torch.equal(_bits(got[q]), _bits(b.own[i][0])), (q, links[q].tolist())
    assert_same(got, dbg, *expected(b, is_edge, which), what=f'wave_patterns({length})')


@pytest.mark.parametrize('h', [2, 3])
@pytest.mark.parametrize('num_perm,p', [(128, 8), (8, 4), (512, 11)])
def test_many_edges_in_one_call(ssa, dev, num_perm, p, h):
    """3 x 4096 + 7 edge links: every workgroup of masked_pairs_kernel serves three or four links in turn, in the order the compaction
    left them in (a K2 link after a hub link, a hub link after a K2 link)"""
    b, distinct, non = batch(ssa, dev, h, num_perm, p)
    links, which = mp.many_edges()
    want, wdbg = expected(b, np.ones(len(links), dtype=bool), which)
    got, dbg = query(b, links, return_debug=True)
    assert_same(got, dbg, want, wdbg, 'one call')
    assert_same(query(b, links), None, want, None, 'one call, no debug outputs')
    # batches of 4100: the workspace and its counter serve calls of 4100, 4100 and 4095 edge links ...
    got, dbg = query(b, links, batch_size=4100, return_debug=True)
    assert_same(got, dbg, want, wdbg, 'batch_size=4100')
    # ... and, behind 3000 links that are not edges, of 1100, 4100, 4100 and 2995
    front = np.arange(3000) % len(non)
    mixed = np.concatenate([non[front], links])
    is_edge = np.arange(len(mixed)) >= 3000
    got, dbg = query(b, mixed, batch_size=4100, return_debug=True)
    assert_same(got, dbg, *expected(b, is_edge, np.concatenate([front, which])), what='3000 non-edges in front, batch_size=4100')


def test_long_batch(ssa, dev):
    """131072 + 83 links in one call: the 16-lane scans of masked_classify_kernel and masked_row_zeros_kernel take a second trip"""
    b, distinct, non = batch(ssa, dev, 3)
    links, is_edge, which = mp.long_batch()
    want, wdbg = expected(b, is_edge, which)
    got, dbg = query(b, links, return_debug=True)
    assert np.array_equal(dbg['masked'].cpu().numpy(), is_edge)
    assert_same(got, dbg, want, wdbg, 'return_debug=True')
    assert_same(query(b, links), None, want, None, 'return_debug=False')
    keep = _t(~is_edge, dev)
    assert torch.equal(_bits(got)[keep], _bits(plain(b, links))[keep])
