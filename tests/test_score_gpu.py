"""ElphHashes.score_links on the GPU: the structure-feature head inside the pair kernel (csrc/ss_head.hpp) against
the reference's own feature rows, against the engine's own rows for every link, unit by unit, across batch sizes and walks, on
every sketch shape the query dispatches on, against a torch module in eval mode, and its errors.

Tolerance (derived, nothing tuned; score_restatement.e_fp):  |score - ref64| <= (2 dim + 6) u A(q),  u = 2^-24,
A(q) = |b2| + sum_j |w2_j| (|t'_j| + sum_i |W'_ji| |x_qi|)."""
from argparse import Namespace
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

from conftest import load_golden
from score_restatement import e_fp, feature_slack, raw_head, unfolded64

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-4  # what tests/test_gpu_parity.py grants a feature row against the golden vectors


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()  # fail loudly if the HIP library is not built
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, h=2, p=8, P=128, floor_sf=False, use_zero_one=True, regenerated=False):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=floor_sf, use_zero_one=use_zero_one))
    if regenerated:  # the golden vectors are defined for the regenerated tables
        eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    return eh


def _sub(table, cards, h):
    return {k: table[k] for k in range(h + 1)}, cards[:, :h]


def _head(ssa, h, normalised, seed, **kw):
    nf = h * (h + 2)
    return ssa.StructureHead(normalised=normalised, **raw_head(2 * nf if normalised else nf, seed, **kw))


def _check(scores, ref64, bar, what):
    got = scores.double().cpu().numpy()
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - ref64)
    worst = int(np.argmax(err - bar))
    assert np.all(err <= bar), f'{what}: link {worst}: |score - ref| = {err[worst]:.3e}, bar {bar[worst]:.3e}'


def _links(n, B, seed, hub=0, isolated=()):
    """B links with duplicates, u == v, negative ids, the top hub on both sides and isolated nodes"""
    rng = np.random.RandomState(seed)
    lk = rng.randint(0, n, size=(B, 2)).astype(np.int64)
    lk[10:20] = lk[0:10]            # duplicates
    lk[20:40, 1] = lk[20:40, 0]     # u == v
    lk[40:140, 0] = hub             # the top hub as u, as v, and with itself
    lk[140:240, 1] = hub
    lk[240] = (hub, hub)
    for t, node in enumerate(isolated):
        lk[250 + 3 * t] = (node, rng.randint(0, n))
        lk[251 + 3 * t] = (rng.randint(0, n), node)
        lk[252 + 3 * t] = (node, node)
    lk[5::97] -= n                  # torch-style negative ids
    return lk


def _graphs():
    """{name: (n, edge_index [2, E] numpy, isolated nodes, top hub)}: N = 3 000, 9 000 undirected edges; the last five nodes isolated"""
    n, e_und, live = 3000, 9000, 2995
    rng = np.random.RandomState(21)
    e = rng.randint(0, live, size=(2, e_und)).astype(np.int64)
    out = {'uniform': np.concatenate([e, e[::-1]], axis=1)}
    rng = np.random.RandomState(22)
    w = np.arange(1, live + 1, dtype=np.float64) ** -0.9
    cdf = np.cumsum(w / w.sum())
    e = np.stack([np.minimum(np.searchsorted(cdf, rng.random_sample(e_und)), live - 1), rng.randint(0, live, size=e_und)]).astype(np.int64)
    out['rank^-0.9'] = np.concatenate([e, e[::-1]], axis=1)
    res = {}
    for name, ei in out.items():
        deg = np.bincount(ei[0], minlength=n)
        assert np.all(deg[live:] == 0)
        res[name] = (n, ei, tuple(range(live, n)), int(np.argmax(deg)))
    return res


@pytest.fixture(scope='module')
def world(ssa, dev):
    """3-hop tables of both graphs, their degrees and B = 20 000 links each, built once; every test reads them only"""
    res = {}
    for t, (name, (n, ei, isolated, hub)) in enumerate(_graphs().items()):
        table, cards = _eh(ssa, h=3).build_hash_tables(n, torch.from_numpy(ei).to(dev))
        deg = torch.from_numpy(np.bincount(ei[0], minlength=n).astype(np.float32)).to(dev)
        links = torch.from_numpy(_links(n, 20000, 31 + t, hub=hub, isolated=isolated)).to(dev)
        res[name] = (n, table, cards, deg, links)
    return res


@pytest.fixture(scope='module')
def ba40(ssa, dev):
    g = load_golden('g3_g4_ba40.npz')
    table, cards = _eh(ssa, h=3, regenerated=True).build_hash_tables(int(g['num_nodes']), torch.from_numpy(g['edge_index']).to(dev))
    return g, table, cards


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [1, 2, 3])
def test_scores_against_the_reference_rows(ssa, dev, ba40, h):
    """the unfolded head in float64 on the reference's own feature rows (G4), every flag combination, three heads each; the
    degree-normalised case on G9 (two zero-degree nodes).  Bar: E_fp + what the feature tolerance RTOL / ATOL can move a score by."""
    g, table, cards = ba40
    sub, c = _sub(table, cards, h)
    links = torch.from_numpy(g['links']).to(dev)
    for zo in (0, 1):
        for fl in (0, 1):
            eh = _eh(ssa, h=h, floor_sf=bool(fl), use_zero_one=bool(zo), regenerated=True)
            rows = g[f'feat_h{h}_zo{zo}_fl{fl}']
            assert np.all(np.isfinite(rows))
            for seed in (101, 202, 303):
                raw = raw_head(h * (h + 2), seed + 10 * h + 2 * zo + fl)
                head = ssa.StructureHead(**raw)
                scores = eh.score_links(links, sub, c, head)
                assert scores.dtype == torch.float32 and scores.shape == (len(rows),) and scores.device == links.device
                _check(scores, unfolded64(raw, rows), e_fp(head, rows) + feature_slack(head, rows, RTOL, ATOL), f'h={h} zo={zo} fl={fl} seed={seed}')
    g9 = load_golden('g9_degree_normalised.npz')
    eh = _eh(ssa, h=h, regenerated=True)
    rows = g9[f'normed_h{h}']
    assert np.all(np.isfinite(rows)) and int((g9['degrees'] == 0).sum()) == 2
    for seed in (404, 505, 606):
        raw = raw_head(2 * h * (h + 2), seed + h)
        head = ssa.StructureHead(normalised=True, **raw)
        scores = eh.score_links(torch.from_numpy(g9['links']).to(dev), sub, c, head, degrees=torch.from_numpy(g9['degrees']))
        _check(scores, unfolded64(raw, rows), e_fp(head, rows) + feature_slack(head, rows, RTOL, ATOL), f'h={h} normalised seed={seed}')


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [1, 2, 3])
@pytest.mark.parametrize('graph', ['uniform', 'rank^-0.9'])
def test_scores_against_the_engine_rows_every_link(ssa, dev, world, graph, h):
    """the float64 head on the rows get_subgraph_features returns for the same 20 000 links, E_fp alone, with and without degrees"""
    n, table, cards, deg, links = world[graph]
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    for normalised in (False, True):
        dg = deg if normalised else None
        rows = eh.get_subgraph_features(links, sub, c, degrees=dg).double().cpu().numpy()
        assert np.all(np.isfinite(rows))
        head = _head(ssa, h, normalised, 7 * h + int(normalised))
        scores = eh.score_links(links, sub, c, head, degrees=dg)
        assert scores.shape == (len(links),)
        _check(scores, head.reference(rows), e_fp(head, rows), f'{graph} h={h} normalised={normalised}')


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [3, 6, 8, 15, 16, 30])
def test_every_hidden_unit_is_owned_by_its_lane(ssa, dev, ba40, dim):
    """w2 one-hot at unit j: the score is that unit alone -- fewer than, exactly, and more than 16 units per 16-lane row"""
    g, table, cards = ba40
    h, normalised = {3: (1, False), 6: (1, True), 8: (2, False), 16: (2, True), 15: (3, False), 30: (3, True)}[dim]
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h, regenerated=True)
    links = torch.from_numpy(g['links']).to(dev)
    dg = torch.from_numpy(load_golden('g9_degree_normalised.npz')['degrees']).to(dev) if normalised else None
    rows = eh.get_subgraph_features(links, sub, c, degrees=dg).double().cpu().numpy()
    raw = raw_head(dim, 900 + dim)
    raw['bias'] = raw['bias'] + 3.0  # most units positive before the ReLU: a unit that is clipped to 0 shows nothing
    live = 0
    for j in range(dim):
        one_hot = torch.zeros(dim)
        one_hot[j] = 1.5
        head = ssa.StructureHead(normalised=normalised, **dict(raw, out_weight=one_hot, out_bias=None))
        ref = head.reference(rows)
        live += int(np.any(ref != 0))
        _check(eh.score_links(links, sub, c, head, degrees=dg), ref, e_fp(head, rows), f'dim={dim} unit {j}')
    assert live >= dim - 2, 'the one-hot heads must not all be clipped by the ReLU'


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_relu_and_bias(ssa, dev, world):
    n, table, cards, deg, links = world['rank^-0.9']
    sub, c = _sub(table, cards, 2)
    eh = _eh(ssa, h=2)
    raw = raw_head(8, 5)
    ident = dict(bn_weight=torch.ones(8), bn_bias=torch.zeros(8), bn_mean=torch.zeros(8), bn_var=torch.ones(8), bn_eps=0.0)
    raw.update(ident, bias=torch.full((8,), -1e30))
    head = ssa.StructureHead(**raw)
    assert np.all(head.shift == np.float32(-1e30))
    scores = eh.score_links(links[:4000], sub, c, head)
    want = torch.full((4000,), float(raw['out_bias'][0]), dtype=torch.float32)
    assert torch.equal(scores.cpu().view(torch.int32), want.view(torch.int32))        # bit-equal float32(out_bias)
    scores = eh.score_links(links[:4000], sub, c, ssa.StructureHead(**dict(raw, out_bias=None)))
    assert bool((scores == 0).all())


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalised', [False, True])
def test_one_link_one_score(ssa, dev, world, monkeypatch, normalised):
    """a link's score does not depend on the batch, the grid, `out`, or the walk (grouped, gathered / scattered)"""
    n, table, cards, deg, links = world['rank^-0.9']
    h = 3
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, normalised, 77)
    dg = deg if normalised else None
    full = eh.score_links(links, sub, c, head, degrees=dg)
    assert bool(torch.isfinite(full).all())
    for B in (1, 15, 16, 17, 16384, 16385):  # a lane-group block; one against two pairs per group in the grid rule
        assert torch.equal(eh.score_links(links[:B], sub, c, head, degrees=dg), full[:B]), B
    assert torch.equal(eh.score_links(links[3], sub, c, head, degrees=dg), full[3:4])           # a 1-D link
    for bs in (7, 4096):
        assert torch.equal(eh.score_links(links, sub, c, head, degrees=dg, batch_size=bs), full), bs
    big = torch.full((len(links) + 20,), 7.0, device=dev)
    for bs in (11_000_000, 4096):
        back = eh.score_links(links, sub, c, head, degrees=dg, batch_size=bs, out=big[10:-10])
        assert back.data_ptr() == big[10:].data_ptr() and torch.equal(back, full)
        assert bool((big[:10] == 7).all()) and bool((big[-10:] == 7).all())
    assert torch.equal(eh.score_links(links.cpu(), sub, c.cpu(), head, degrees=dg).to(dev), full)  # host-resident callers get a host tensor
    monkeypatch.setattr(ssa.knobs, 'GROUP_LINKS_MIN', 1000)
    for mode in (True, False, 'auto'):
        eh.group_links = mode
        for gather_min in (1 << 40, 0):  # the order walked by the kernel itself / chunks gathered before and scattered after it
            monkeypatch.setattr(ssa.knobs, 'GROUP_GATHER_MIN', gather_min)
            for bs in (11_000_000, 6001):
                assert torch.equal(eh.score_links(links, sub, c, head, degrees=dg, batch_size=bs), full), (mode, gather_min, bs)
            big.fill_(7.0)
            eh.score_links(links, sub, c, head, degrees=dg, batch_size=6001, out=big[10:-10])
            assert torch.equal(big[10:-10], full) and bool((big[:10] == 7).all()) and bool((big[-10:] == 7).all())


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,p', [(64, 8), (192, 8), (256, 8), (8, 4), (128, 16)])
def test_other_sketch_shapes(ssa, dev, P, p):
    """the fast paths (P in {64, 192, 256} at p = 8) and the run-time-size path, as test 2 at h = 2 and B = 2 000"""
    n, e_und, h = 600, 1800, 2
    rng = np.random.RandomState(41)
    e = rng.randint(0, n - 3, size=(2, e_und)).astype(np.int64)
    ei = np.concatenate([e, e[::-1]], axis=1)
    eh = _eh(ssa, h=h, p=p, P=P)
    table, cards = eh.build_hash_tables(n, torch.from_numpy(ei).to(dev))
    deg = torch.from_numpy(np.bincount(ei[0], minlength=n).astype(np.float32)).to(dev)
    links = torch.from_numpy(_links(n, 2000, 43, hub=int(np.argmax(np.bincount(ei[0]))), isolated=(n - 3, n - 2, n - 1))).to(dev)
    for normalised in (False, True):
        dg = deg if normalised else None
        rows = eh.get_subgraph_features(links, table, cards, degrees=dg).double().cpu().numpy()
        assert np.all(np.isfinite(rows))
        head = _head(ssa, h, normalised, P + p + int(normalised))
        _check(eh.score_links(links, table, cards, head, degrees=dg), head.reference(rows), e_fp(head, rows), f'P={P} p={p} normalised={normalised}')


# 7 ---------------------------------------------------------------------------------------------------------------------------------
class _Model(torch.nn.Module):
    """a stand-in with the attribute names of both reference models and nothing but the label branch behind `lin`"""

    def __init__(self, dim, append_normalised):
        super().__init__()
        self.dim, self.append_normalised = dim, append_normalised
        self.label_lin_layer = torch.nn.Linear(dim, dim)
        self.bn_labels = torch.nn.BatchNorm1d(dim)
        self.lin = torch.nn.Linear(dim, 1)

    def forward(self, sf):
        return self.lin(torch.relu(self.bn_labels(self.label_lin_layer(sf)))).squeeze(-1)


@pytest.mark.parametrize('normalised', [False, True])
def test_a_torch_module_in_eval_mode(ssa, dev, world, normalised):
    n, table, cards, deg, links = world['uniform']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    dg = deg if normalised else None
    rows = eh.get_subgraph_features(links, sub, c, degrees=dg)
    torch.manual_seed(1234)
    model = _Model(rows.size(1), normalised).to(dev)
    with torch.no_grad():
        model.bn_labels.weight.uniform_(0.5, 1.5)
        model.bn_labels.bias.normal_()
        for s in range(4):  # running statistics from a few training-mode passes over seeded batches of real rows
            model(rows[torch.randint(0, len(rows), (512,), generator=torch.Generator().manual_seed(s)).to(dev)])
    with pytest.raises(ValueError):
        ssa.StructureHead.from_module(model)          # still in training mode
    model.eval()
    assert float(model.bn_labels.running_mean.abs().max()) > 0 and float((model.bn_labels.running_var - 1).abs().max()) > 1e-3
    head = ssa.StructureHead.from_module(model)
    assert head.normalised == normalised and head.hops == h
    with torch.no_grad():
        want = model(rows)
    scores = eh.score_links(links, sub, c, head, degrees=dg)
    _check(scores, want.double().cpu().numpy(), 2 * e_fp(head, rows.double().cpu().numpy()), f'module, normalised={normalised}')


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_bounds(ssa, dev, world):
    n, table, cards, deg, links = world['uniform']
    h = 2
    sub, c = _sub(table, cards, h)
    eh = _eh(ssa, h=h)
    head = _head(ssa, h, False, 9)
    good = eh.score_links(links[:300], sub, c, head)
    bad = links[:300].clone()
    bad[7, 0] = n + 3
    bad[200, 1] = -n - 1
    eh.strict_bounds = True
    with pytest.raises(IndexError):
        eh.score_links(bad, sub, c, head)
    with pytest.raises(IndexError):
        eh.get_subgraph_features(bad, sub, c)        # (the same report as the feature query's)
    eh.strict_bounds = False
    got = eh.score_links(bad, sub, c, head)
    nan = torch.isnan(got)
    assert nan.nonzero().flatten().tolist() == [7, 200]
    assert torch.equal(got[~nan], good[~nan])
    eh.strict_bounds = 'deferred'
    got = eh.score_links(bad, sub, c, head)
    assert torch.isnan(got).nonzero().flatten().tolist() == [7, 200]
    with pytest.raises(IndexError):
        eh.check_errors()
    eh.check_errors()                                 # reported once
    with pytest.raises(ValueError):
        eh.score_links(links, sub, c, _head(ssa, 3, False, 1))                    # a 3-hop head
    with pytest.raises(ValueError):
        eh.score_links(links, sub, c, _head(ssa, h, True, 1))                     # normalised without degrees
    with pytest.raises(ValueError):
        eh.score_links(links, sub, c, head, degrees=deg)                          # degrees without normalised
    L = len(links)
    for wrong in (torch.empty((L + 1,), device=dev), torch.empty((L, 1), device=dev), torch.empty((L,), device=dev, dtype=torch.float64),
                  torch.empty((L,)), torch.empty((2 * L,), device=dev)[::2]):
        with pytest.raises(ValueError):
            eh.score_links(links, sub, c, head, out=wrong)
        with pytest.raises(ValueError):
            eh.score_links(links, sub, c, head, out=wrong, batch_size=4096)
    # the C entry point on raw device pointers: the same bits
    lib = ssa._native.lib()
    prm, hd = eh._params(dev), head._device(dev)
    mh = [table[k].mh_u32 for k in range(1, h + 1)]
    hl = [table[k].hll_u8 for k in range(1, h + 1)]
    mh_ptrs = (c_void_p * h)(*[t.data_ptr() for t in mh])
    hl_ptrs = (c_void_p * h)(*[t.data_ptr() for t in hl])
    cc = c.contiguous() if c.stride(1) != 1 else c
    out = torch.full((L,), 7.0, device=dev)
    flags = ssa._native.SS_FLAG_USE_ZERO_ONE
    rc = lib.ss_pair_scores(c_void_p(links.data_ptr()), None, L, n, h, mh_ptrs, 128, hl_ptrs, c_void_p(cc.data_ptr()), cc.stride(0),
                            byref(prm.struct), flags, None, byref(hd.struct), c_void_p(out.data_ptr()), None,
                            c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    assert torch.equal(out, eh.score_links(links, sub, c, head))
    order = torch.randperm(L, generator=torch.Generator().manual_seed(2)).to(dev).to(torch.int32)
    out2 = torch.full((L,), 7.0, device=dev)
    rc = lib.ss_pair_scores(c_void_p(links.data_ptr()), c_void_p(order.data_ptr()), L, n, h, mh_ptrs, 128, hl_ptrs, c_void_p(cc.data_ptr()),
                            cc.stride(0), byref(prm.struct), flags, None, byref(hd.struct), c_void_p(out2.data_ptr()), None,
                            c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0 and torch.equal(out2, out)         # out[q] is pair q whatever the order (and the register budget that goes with it)
