"""update_hash_tables, mask_target, score_links, topk_links, rank_links and PPR across the 2 GiB and 4 GiB offset boundaries.  Needs a
real MI355X: `-m gpu`.  The companion of tests/test_large_tables_gpu.py, which pins build_hash_tables and the plain pair query at these
sizes; those two are the trusted references here, with compacted copies of the touched rows (every offset below 2^31).

Shapes, h = 2, the smallest that cross each boundary (row r of an [N, row] table starts at byte r * row_bytes):
  S1  P = 128, p = 8, N = 2^23 + 2^18, bounds [2^22, 2^23] (fixture A's graph).  MinHash row 512 B: row 2^22 starts at byte 2^31, row
      2^23 at byte 2^32.  HLL row 256 B: row 2^23 starts at byte 2^31.  2 hops: 2 * 8 650 752 * 768 B = 13.3 GB.
  S2  P = 256, p = 8, same N and bounds.  MinHash row 1 024 B: bytes 2^32 / 2^33 at the bounds, and the uint32 ELEMENT index r * 256
      reaches 2^31 at row 2^23 (a signed 32-bit element index does not show at S1).  HLL as S1.
  S3  P = 64, p = 10 (M = 1 024, the run-time-size path), N = 2^22 + 2^18, bounds [2^21, 2^22].  HLL row 1 024 B: row 2^21 starts at
      byte 2^31, row 2^22 at byte 2^32.  MinHash row 256 B: row 2^22 starts at byte 2^30 (no crossing).
The hop tables of S2 and S3 are not pinned row by row at this size; the query tests do not need that (their references read the same
stored rows), so S2 and S3 serve the query entry points only and update_hash_tables / mask_target, which need CORRECT tables, run at S1.

The fixtures' free-memory requirements: NEEDS below (profiles/large_tables_tests.txt)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import oracle_params
import large_table_restatement as R
import masked_restatement as mr
import rank_restatement as rr
import update_restatement as ur
from large_table_helpers import LIVE, Big, boundary_links, compacted_oracle, feature_tol, release_all, require_free_memory, wrap
from ppr_restatement import pagerank_power
from score_restatement import e_fp, raw_head

pytestmark = pytest.mark.gpu

H = 2
SHAPES = {'S1': (128, 8, (1 << 23) + (1 << 18), [1 << 22, 1 << 23]),
          'S2': (256, 8, (1 << 23) + (1 << 18), [1 << 22, 1 << 23]),
          'S3': (64, 10, (1 << 22) + (1 << 18), [1 << 21, 1 << 22])}
# free device memory a fixture asks for.  NOT YET MEASURED (profiles/large_tables_tests.txt says why): until the peaks of a run are
# recorded there, this is the arithmetic of the resident hop tables alone, 2 hops * N * (4 P + M) bytes -- three builds at S1 (the
# fixture's, update_hash_tables' private one and the rebuild it is compared with), one at S2 and S3 -- and so a lower bound
_TABLES = {name: 2 * n * (4 * P + (1 << p)) for name, (P, p, n, _) in SHAPES.items()}
NEEDS = {'S1': 3 * _TABLES['S1'], 'S2': _TABLES['S2'], 'S3': _TABLES['S3']}
LOW_HUB_THRESHOLD = 16   # below the ~40 in-edges of a window row, far above the background's (Poisson, mean 2)
STEP = 4000000           # links per brute-force score_links call: 64 MB of links, 16 MB of scores
K = 50


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, P, p):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=H, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    return eh


def _near_head(ssa):
    """a normalised head that ranks by neighbourhood overlap: the intersection columns (d_u, d_v >= 1: 0-3, and 8-11 of the normalised
    copy) keep positive weights, every other column is scaled by 1e-3, the output weights are positive.  s(u, .) then peaks on the
    two-hop neighbourhood of u -- for a source in a boundary window that lies on BOTH sides of the boundary row -- and still differs
    from row to row elsewhere (the cardinality columns keep a small weight), so counts over all N rows mean something"""
    raw = raw_head(16, 77)
    w = raw['weight'].clone()
    inter = [0, 1, 2, 3, 8, 9, 10, 11]
    other = [4, 5, 6, 7, 12, 13, 14, 15]
    w[:, inter] = w[:, inter].abs()
    w[:, other] *= 1e-3
    return ssa.StructureHead(normalised=True, **dict(raw, weight=w, out_weight=raw['out_weight'].abs() + 0.1))


def _make(ssa, dev, name):
    release_all(dev)
    P, p, n, bounds = SHAPES[name]
    require_free_memory(dev, NEEDS[name], f'fixture {name}')
    torch.cuda.reset_peak_memory_stats(dev)
    big = Big()
    big.name, big.n, big.bounds, big.P, big.M = name, n, bounds, P, 1 << p
    big.graph = g = R.boundary_graph(n, bounds, dev, seed=20 + len(bounds))     # (S1, S2: the graph of fixture A)
    deg = torch.bincount(R.self_looped_edges(g.edge_index)[1], minlength=n)    # in-degree over the self-looped list
    for b in bounds:  # the boundary rows, their predecessors and successors carry work (>= 1 edge besides the self loop)
        assert int(deg[b - 1:b + 2].min()) >= 2, f'boundary row {b} of fixture {name} has no edge'
    assert int(deg[n - 8:n - 1].max()) == 1 and int(deg[n - 1]) == 2, 'the last 7 nodes but one are isolated, N - 1 is a neighbour'
    assert int(deg[g.mega]) > ssa._native.MEGA_SLICE and min(g.hubs) > max(bounds)
    assert n * P * 4 > (1 << 31) or n * big.M > (1 << 31), 'the shape crosses no boundary'
    big.eh = _eh(ssa, P, p)
    big.table, big.cards = big.eh.build_hash_tables(n, g.edge_index)
    big.prm = oracle_params(big.eh.hll_tables)
    big.degrees = torch.bincount(g.edge_index[0], minlength=n).to(torch.float32)
    big.degrees[:1000:7] = 0          # (division by zero -> 0 in the normalised copy), the boundary rows among them
    for b in bounds:
        big.degrees[b] = big.degrees[b + 3] = 0
    big.near = _near_head(ssa)
    big.cache = {}                    # {u: float32 [N] brute-force scores s(u, .) under big.near}, shared by the topk and rank tests
    LIVE.append(big)
    return big


@pytest.fixture(scope='module')
def s1(ssa, dev):
    big = _make(ssa, dev, 'S1')
    yield big
    big.release()


@pytest.fixture(scope='module')
def s2(ssa, dev):
    big = _make(ssa, dev, 'S2')   # (releases S1 first)
    yield big
    big.release()


@pytest.fixture(scope='module')
def s3(ssa, dev):
    big = _make(ssa, dev, 'S3')   # (releases S2 first)
    yield big
    big.release()


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _where(big, rows):
    return ', '.join(R.describe_row(r, big.bounds) for r in list(rows)[:4])


def _alias_distances(big):
    """row distances at which an offset wrapped at 2^31 or 2^32 (bytes, or uint32 elements of a MinHash row) reads another row"""
    d = set()
    for unit in (big.P * 4, big.M, big.P):
        d |= {(1 << 31) // unit, (1 << 32) // unit}
    return sorted(x for x in d if x < big.n)


def _touches_every_bound(big, links):
    """the condition on the inputs alone: rows at or above every boundary row, and below the lowest, are read"""
    ids = wrap(links.to(torch.int64), big.n)
    assert int(ids.min()) < min(big.bounds)
    for b in big.bounds:
        assert bool((ids == b).any()) and int((ids > b).sum()) >= 50, f'no link reads rows at or above row {b}'


def _compact(big, links, degrees, dev):
    """the distinct rows `links` touch, index_select-ed into small tables -> (renumbered links, table, cards, degrees)"""
    from subgraph_sketching_amd.containers import HopSketch
    ids = wrap(links.to(torch.int64), big.n)
    uniq, inv = torch.unique(ids.flatten(), return_inverse=True)
    assert uniq.numel() * max(big.P * 4, big.M) < (1 << 30), 'the compacted tables must stay far below 2^31 bytes'
    table = {k: HopSketch(big.table[k].mh_u32.index_select(0, uniq), big.table[k].hll_u8.index_select(0, uniq), dev) for k in (1, 2)}
    return (inv.reshape(-1, 2).contiguous(), table, big.cards.index_select(0, uniq).contiguous(),
            None if degrees is None else degrees.index_select(0, uniq))


def _bits(a):
    a = np.asarray(a, dtype=np.float32)
    return np.where(a == 0, np.float32(0), a).view(np.int32)  # +-0 compare equal, every other value bit for bit


def _score_row(big, dev, u):
    """s(u, v) for ALL v by score_links, STEP links at a time (the brute force topk_links and rank_links replace): float32 [N]"""
    row = big.cache.get(u)
    if row is None:
        row = np.empty(big.n, dtype=np.float32)
        for s in range(0, big.n, STEP):
            v = torch.arange(s, min(s + STEP, big.n), device=dev)
            row[s:s + STEP] = big.eh.score_links(torch.stack([torch.full_like(v, u), v], 1), big.table, big.cards, big.near,
                                                 degrees=big.degrees).cpu().numpy()
        assert np.all(np.isfinite(row))
        big.cache[u] = row
    return row


# ---------------------------------------------------------------------------------------------------
# the checks, one per entry point
# ---------------------------------------------------------------------------------------------------
def _check_anchor(big, dev):
    links = boundary_links(big, dev, 2048, seed=1)
    _touches_every_bound(big, links)
    ofeat, odbg = compacted_oracle(big, links, debug=True)
    feats, dbg = big.eh._pair_kernel(links, big.table, big.cards, want_debug=True)
    ids = wrap(links, big.n).cpu().numpy()
    for key, what in (('match', 'MinHash match counts'), ('zeros', 'HLL zero counts')):
        bad = np.flatnonzero((dbg[key].cpu().numpy() != odbg[key]).reshape(len(ids), -1).any(axis=1))
        assert not len(bad), f'{what}: {len(bad)} links differ, first {ids[bad[0]].tolist()}: {_where(big, ids[bad[0]])}'
    np.testing.assert_allclose(feats.cpu().numpy(), ofeat, **feature_tol(ofeat))
    assert torch.equal(big.eh.get_subgraph_features(links, big.table, big.cards), feats)


def _check_scores(ssa, big, dev):
    small = boundary_links(big, dev, 2048, seed=4)
    _touches_every_bound(big, small)
    top = max(big.bounds)
    gen = torch.Generator(device=dev).manual_seed(5)
    high = torch.randint(top, big.n, (65536 + 4099, 2), device=dev, generator=gen)      # every row at or above the top boundary row
    high[::9] -= big.n
    for normalised in (False, True):
        dg = big.degrees if normalised else None
        head = ssa.StructureHead(normalised=normalised, **raw_head(16 if normalised else 8, 300 + int(normalised)))
        for links in (small, high):
            got = big.eh.score_links(links, big.table, big.cards, head, degrees=dg)
            assert got.dtype == torch.float32 and got.shape == (len(links),)
            assert len(torch.unique(got)) > 256, 'the scores must tell the links apart'
            lk, table, cards, cdg = _compact(big, links, dg, dev)
            want = big.eh.score_links(lk, table, cards, head, degrees=cdg)
            bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero().flatten()
            assert not len(bad), (f'normalised={normalised}, B={len(links)}: {len(bad)} scores differ from the compacted tables, first link '
                                  f'{wrap(links[bad[0]], big.n).tolist()}: {_where(big, wrap(links[bad[0]], big.n).tolist())}')
        if normalised:
            z = wrap(small, big.n)
            assert int((big.degrees[z[:, 0]] == 0).sum()) > 0 and int((big.degrees[z[:, 1]] == 0).sum()) > 0, 'degree 0 on both sides'
        # the float64 head on the feature rows of the plain query (pinned at S1 by test_large_tables_gpu.py, at S2 / S3 by the anchor)
        rows = big.eh.get_subgraph_features(small, big.table, big.cards, degrees=dg).double().cpu().numpy()
        assert np.all(np.isfinite(rows))
        err = np.abs(big.eh.score_links(small, big.table, big.cards, head, degrees=dg).double().cpu().numpy() - head.reference(rows))
        bar = e_fp(head, rows)
        worst = int(np.argmax(err - bar))
        assert np.all(err <= bar), f'{big.name} normalised={normalised}: link {worst}: |score - ref| = {err[worst]:.3e}, bar {bar[worst]:.3e}'


def _topk_sources(big):
    lo, b = big.bounds[0], big.bounds[-1]
    return [b - 3, b, b + 700, -(big.n - lo)]       # inside the dense window of the top bound; the lower bound as a negative id


def _check_topk(big, dev):
    n, eh, b = big.n, big.eh, big.bounds[-1]
    sources = _topk_sources(big)
    ei = big.graph.edge_index
    nb = torch.unique(ei[0][ei[1] == b - 3])
    below, above = nb[nb < b][:3], nb[nb >= b][:3]
    assert len(below) == 3 and len(above) == 3, 'the exclude list holds neighbours of row b - 3 on both sides of b'
    ex_v = torch.cat([below, above, torch.tensor([b + 1], device=dev)])
    exclude = torch.stack([torch.tensor([b - 3] * 6 + [b], device=dev), ex_v])
    ex = exclude.cpu().numpy()
    want = []
    for u in sources:
        u = u + n if u < 0 else u
        sc = _score_row(big, dev, u)
        elig = np.ones(n, dtype=bool)
        elig[u] = False
        elig[ex[1][ex[0] == u]] = False
        cand = np.nonzero(elig)[0]
        order = np.lexsort((cand, -sc[cand]))[:K + 1]
        ids = cand[order]
        # on the reference alone: candidates on both sides of the boundary row, and no two of them a wrapped offset apart
        if u >= b - big.graph.window:
            assert (ids[:K] > b).any() and (ids[:K] < b).any(), f'source {u}: the reference must rank candidates on both sides of row {b}'
        gaps = np.abs(ids[:, None] - ids[None, :])
        assert not np.isin(gaps, _alias_distances(big)).any(), f'source {u}: two of the top {K + 1} rows alias under a wrapped offset'
        want.append((ids[:K], sc[ids[:K]]))
    ids, scores = eh.topk_links(torch.tensor(sources, device=dev), big.table, big.cards, K, big.near, degrees=big.degrees, exclude=exclude)
    for r, u in enumerate(sources):
        got = ids[r].cpu().numpy()
        diff = np.flatnonzero(got != want[r][0])
        assert not len(diff), f'source {u}: ids differ from place {diff[0]}: got {_where(big, got[diff])}; want {_where(big, want[r][0][diff])}'
        np.testing.assert_array_equal(_bits(scores[r].cpu().numpy()), _bits(want[r][1]), err_msg=f'source {u}')
    assert not np.isin(ids[0].cpu().numpy(), ex_v.cpu().numpy()[:6]).any()


def _rank_links(big):
    n, (lo, b), g = big.n, big.bounds, big.graph
    far = [(lo // 3 + 11, b + 4321), (b + g.window + 9000, lo + 77), (lo + g.window + 5000, n - 3), (12345, 2 * lo // 3)]
    return np.array([(b - 3, b + 5), (b - 3, b - 7), (b - 3, 12345), (b - 3, lo),                  # a repeated source (one of topk's)
                     (b, b), (b, lo - 1), (b + 700, b), (b + 700, lo),                              # target == a boundary row, u == t
                     (-(n - lo), b), (-(n - lo), lo + 1),                                           # the lower bound as a negative id
                     (lo - 1, lo + 1), (lo + 1, lo - 1), (b - 1, b + 1), (b + 1, b - 1),            # straddling each bound
                     (5, b), (5, lo), (5, n - 1), (n - 1, b - 1), (n - 1, -n),                      # low -> high, high -> low
                     (g.mega, b + 9), (g.mega, 77), (g.hubs[0], lo)] + far, dtype=np.int64)         # from the mega row, from a hub


def _check_rank(ssa, big, dev, monkeypatch):
    n, eh, b = big.n, big.eh, big.bounds[-1]
    links = _rank_links(big)
    w = rr.wrap(links, n)
    for bound in big.bounds:
        for col in (0, 1):
            assert (w[:, col] < bound).any() and (w[:, col] >= bound).any() and (w[:, 1] == bound).any()
    ei = big.graph.edge_index
    ex_ref = ei[:, torch.isin(ei[0], torch.from_numpy(np.unique(w[:, 0])).to(dev))].cpu().numpy()   # a set: only these columns count
    row = lambda q, u: _score_row(big, dev, u)
    lk = torch.from_numpy(links).to(dev)
    for exclude, ref in ((None, None), (ei, ex_ref)):
        want = rr.rank_counts(row, links, n, ref)
        # on the reference alone: the rows at or above the top boundary row add to `greater` for at least half of the links
        high = 0
        for q, (u, t) in enumerate(w):
            s, c = row(q, int(u)), rr.candidates(int(u), int(t), n, ref)
            high += int(np.count_nonzero(s[b:][c[b:]] > s[t]) > 0)
        assert 2 * high >= len(links), f'only {high} of {len(links)} links count a row at or above row {b}'
        call = lambda: eh.rank_links(lk, big.table, big.cards, big.near, degrees=big.degrees, exclude=exclude)
        runs = [call()]
        monkeypatch.setattr(ssa.engine, '_RANK_LAUNCH_LINKS', 5)       # the links split into launches,
        monkeypatch.setattr(ssa.engine, '_RANK_EXCLUDE_PAIRS', 512)    # the excluded pairs into chunks
        runs.append(call())
        monkeypatch.undo()
        for greater, equal in runs:
            gr, eq = greater.cpu().numpy(), equal.cpu().numpy()
            bad = np.flatnonzero((gr != want[0]) | (eq != want[1]))
            assert not len(bad), (f'exclude={exclude is not None}: {len(bad)} links differ, first {w[bad[0]].tolist()} ({_where(big, w[bad[0]])}): '
                                  f'got ({gr[bad[0]]}, {eq[bad[0]]}), want ({want[0][bad[0]]}, {want[1][bad[0]]})')


# ---------------------------------------------------------------------------------------------------
# S1: P = 128, p = 8 (the shipped fast path), the pinned build
# ---------------------------------------------------------------------------------------------------
def test_score_links_s1(ssa, s1, dev):
    """(2) crosses: MinHash bytes 2^31 / 2^32 (rows 2^22 / 2^23), HLL byte 2^31 (row 2^23), cards and degrees at those rows.
    Reference: score_links on the COMPACTED tables (torch.equal on the bits: 2 048 boundary links and 69 635 links of high rows only,
    both register budgets; plain and normalised head, degrees with zeros) and the float64 head on the plain query's rows, bound
    (2 dim + 6) 2^-24 A(q).  On the inputs alone: the links read rows on both sides of every bound and the bound rows themselves,
    the compacted tables stay below 2^30 bytes, and the scores take more than 256 distinct values (a row read elsewhere shows)"""
    _check_scores(ssa, s1, dev)


def test_topk_links_s1(s1, dev):
    """(3) crosses: `v * row` of the one-vs-all scan over all N rows, the staged source rows at and above row 2^23.  Reference: brute
    force, score_links over (s, v) for ALL v in chunks of 4 M, eligibility, lexsort by (score desc, id asc); ids exact, scores bit
    for bit.  On the reference alone: every source of the top window ranks candidates on both sides of row 2^23, and no two of a
    source's top k + 1 rows lie a wrapped offset apart, so aliased reads cannot reproduce the list"""
    _check_topk(s1, dev)


def test_rank_links_s1(ssa, s1, dev, monkeypatch):
    """(4) crosses: the LDS-staged 64-bit link ids and `v * row` of ss_rank.hip, the exclusion correction's pair scores.  Reference:
    rank_restatement.rank_counts over the brute-force score_links rows (shared with the topk test), exclude=None and the edge list;
    greater / equal exact, also with the launches and exclusion chunks split small.  On the reference alone: rows at or above row 2^23
    add to `greater` for at least half of the links, so a scan that dropped or wrapped the high rows counts differently"""
    _check_rank(ssa, s1, dev, monkeypatch)


def _update_case(big, dev, kind):
    """-> (new edge_index, added, removed) on the device: changed edges with targets at rows b - 1, b, b + 1 of both bounds, N - 1 (added
    only: its one edge keeps max(edge_index) in place), a hub above the bounds and a handful of far rows"""
    n, g = big.n, big.graph
    ei = g.edge_index
    gen = torch.Generator(device=dev).manual_seed(90)
    targets = [b + d for b in big.bounds for d in (-1, 0, 1)] + [g.hubs[1]] + torch.randint(0, n - 8, (5,), device=dev, generator=gen).tolist()
    new, added, removed = ei, None, None
    if kind in ('removed', 'mixed'):
        half = ei.size(1) // 2
        pos = []
        for t in targets:   # one undirected edge at each target: both stored directions go
            hit = ((ei[1, :half] == t) & (ei[0, :half] != t)).nonzero().flatten()
            hit = hit if len(hit) else ((ei[1, half:] == t) & (ei[0, half:] != t)).nonzero().flatten()
            if len(hit):   # (a far row may have no edge; the boundary rows have: the fixture asserts it)
                pos.append(int(hit[0]))
        pos = torch.tensor(sorted(set(pos)), device=dev)
        keep = torch.ones(ei.size(1), dtype=torch.bool, device=dev)
        keep[pos] = False
        keep[pos + half] = False
        new, removed = ei[:, keep], torch.cat([ei[:, pos], ei[:, pos + half]], 1)
    if kind in ('added', 'mixed'):
        t = torch.tensor(targets + [n - 1], device=dev)
        und = torch.stack([torch.randint(0, n - 8, (len(t),), device=dev, generator=gen), t])
        added = torch.cat([und, und.flip(0)], 1)
        new = torch.cat([new, added], 1)
    assert int(new.max()) == int(ei.max()) == n - 1, 'n_self must not move'
    return new, added, removed


def _check_update(ssa, big, dev, kind, want_hubs=False):
    n, eh = big.n, big.eh
    old = big.graph.edge_index
    new, added, removed = _update_case(big, dev, kind)
    host = lambda a: None if a is None else a.cpu().numpy()
    had_loop = (np.arange(n) < ur.n_self_of(host(old))).astype(np.float32)[:, None]
    dirty = ur.dirty_sets(n, host(new), had_loop, host(added), host(removed), H)
    assert 0 < dirty[2].sum() < n / 100, 'the case must be a restriction: a rebuild in disguise recomputes every row'
    for b in big.bounds:
        assert dirty[1][b - 1:b + 2].all()
    table, cards = eh.build_hash_tables(n, old)                     # a private build: updated in place
    old_cards = cards.clone()
    t_up, c_up, info = eh.update_hash_tables(table, cards, n, new, added=added, removed=removed, return_info=True)
    assert t_up is table and c_up is cards
    t_ref, c_ref = eh.build_hash_tables(n, new)                     # pinned at this size by test_large_tables_gpu.py
    assert info['seed_rows'] == int(dirty[1].sum())
    for k in (1, 2):
        assert info['dirty_rows'][k] == int(dirty[k].sum()), (k, info)
        for what, got, want in (('MinHash', t_up[k].mh_u32, t_ref[k].mh_u32), ('HLL', t_up[k].hll_u8, t_ref[k].hll_u8)):
            if not torch.equal(got, want):
                bad = (got != want).any(dim=1).nonzero().flatten().cpu().numpy()
                raise AssertionError(R.report(bad, big.bounds, f'{kind}: {what} hop {k}'))
        clean = torch.from_numpy(~dirty[k]).to(dev)
        assert torch.equal(c_up[clean, k - 1].view(torch.int32), old_cards[clean, k - 1].view(torch.int32)), f'cards outside dirty_{k} moved'
        if want_hubs:
            assert info['hub_list'][k] > 0, 'the boundary-window rows take the cooperative hub path'
    mr.assert_features_bar(c_up.cpu().numpy(), c_ref.cpu().numpy(), c_ref.cpu().numpy(), 'cards')   # (== test_update_gpu._assert_cards_bar)
    eh.check_errors()


@pytest.mark.parametrize('kind', ['added', 'removed', 'mixed'])
def test_update_hash_tables_s1(ssa, s1, dev, kind):
    """(5) crosses: rows read from the int32 dirty list (`mh_out + i * P`, `cards_out[i * cards_stride]`) at rows 2^22 +- 1 and
    2^23 +- 1, N - 1, a hub and far rows.  Reference: build_hash_tables on the new edge list (pinned at this size): torch.equal on both
    tables of both hops, cards within rtol 1e-5 / atol 1e-5 * 4 max|cards|, cards outside dirty_k bit-identical to the old ones,
    info == update_restatement.dirty_sets.  On the restatement alone, before the update runs: the boundary rows are dirty and
    |dirty_2| < N / 100, so neither a rebuild in disguise nor an update that skipped the high rows can pass"""
    _check_update(ssa, s1, dev, kind)


def test_update_hash_tables_hub_path_s1(ssa, s1, dev, monkeypatch):
    """(5) the mixed case with HUB_THRESHOLD = 16: the boundary-window rows (~40 in-edges) take the update's cooperative hub path;
    same reference and conditions, plus info['hub_list'][k] > 0"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', LOW_HUB_THRESHOLD)
    _check_update(ssa, s1, dev, 'mixed', want_hubs=True)


def test_mask_target_s1(ssa, s1, dev):
    """(6) crosses: `y * P` / `y * M` of ss_masked.hip for links whose endpoints (and whose neighbours' rows, re-merged without the
    link) lie on both sides of rows 2^22 and 2^23.  Links that are edges: rows b - 1 and b + 1 of each bound with a neighbour on the other
    side of b, both directions; both ends above the top bound; a hub above the bounds.  Reference for each: the engine's other route,
    update_hash_tables(copy=True, removed=both directions) (test 5) then the plain query; match and zero counts bit-exact, features
    within rtol 1e-5 / atol 1e-5 * 4 max|cards|.  Non-edges at the same rows: torch.equal to the plain query.  On the inputs alone:
    dbg['masked'] is 1 for exactly the edge links, and every edge link's masked row differs from its plain row"""
    big = s1
    n, eh, g = big.n, big.eh, big.graph
    ei = g.edge_index
    nbrs = lambda u: torch.unique(ei[0][(ei[1] == u) & (ei[0] != u)])
    edges = []
    for b in big.bounds:
        up, down = nbrs(b - 1), nbrs(b + 1)
        hi, lo = int(up[up >= b][0]), int(down[down < b][0])
        edges += [(b - 1, hi), (hi, b - 1), (b + 1, lo), (lo, b + 1)]
    top = big.bounds[-1]
    above = nbrs(top + 2)
    edges += [(top + 2, int(above[above > top + 2][0])), (int(above[above > top + 2][-1]), top + 2)]
    hub_nb = nbrs(g.hubs[0])
    edges += [(g.hubs[0], int(hub_nb[0])), (int(hub_nb[-1]), g.hubs[0])]
    keys = ei[0] * n + ei[1]
    is_edge = lambda u, v: bool((keys == u * n + v).any()) or bool((keys == v * n + u).any())
    non = [(u, edges[(q + 3) % len(edges)][1]) for q, (u, _) in enumerate(edges)]
    non = [(u, v) for u, v in non if u != v and not is_edge(u, v)]
    assert len(edges) == 12 and len(non) >= 8 and all(is_edge(u, v) for u, v in edges)
    links = torch.tensor(edges + non, device=dev)
    got, dbg = eh.get_subgraph_features(links, big.table, big.cards, mask_target=ei, return_debug=True)
    assert dbg['masked'].tolist() == [True] * len(edges) + [False] * len(non)
    plain = eh.get_subgraph_features(links, big.table, big.cards)
    assert torch.equal(got[len(edges):].view(torch.int32), plain[len(edges):].view(torch.int32)), 'non-edges are the plain query'
    cards = big.cards.cpu().numpy()
    for q, (u, v) in enumerate(edges):
        assert not torch.equal(got[q], plain[q]), f'masking edge ({u}, {v}) must change its row'
        hit = ((ei[0] == u) & (ei[1] == v)) | ((ei[0] == v) & (ei[1] == u))
        new = ei[:, ~hit]
        assert int(new.max()) == n - 1
        t2, c2 = eh.update_hash_tables(big.table, big.cards, n, new, removed=torch.tensor([[u, v], [v, u]], device=dev), copy=True)
        f2, d2 = eh._pair_kernel(links[q:q + 1], t2, c2, want_debug=True)
        where = f'link ({u}, {v}): {_where(big, (u, v))}'
        assert torch.equal(d2['match'][0], dbg['match'][q]) and torch.equal(d2['zeros'][0], dbg['zeros'][q]), where
        mr.assert_features_bar(got[q].cpu().numpy(), f2[0].cpu().numpy(), cards, where)
        del t2, c2


def test_ppr_iterate_above_4_gib_s1(ssa, s1, dev, monkeypatch):
    """(7) crosses: the fp64 iterate [N, 64] of 64 sources (512-byte rows: 4.43 GB, bytes 2^31 at row 2^22 and 2^32 at row 2^23).
    Reference: the same call with PPR_COLUMNS = 8 (64-byte rows, 0.55 GB, no crossing): torch.equal on vectors and iteration counts,
    default tol and max_iter; and tests/ppr_restatement.py (scipy, fp64) for two source columns, rtol 1e-10 as test_ppr_gpu.py, with
    tol = 0 and max_iter = 6 for BOTH sides -- the restatement takes about a second per step at 8.6 M nodes on the CPU.  On the inputs
    alone: a 64-column iterate is larger than 2^32 bytes, an 8-column one smaller than 2^31, and the compared columns are non-zero on both sides of row 2^23"""
    import scipy.sparse as sp
    from subgraph_sketching_amd.heuristics import DeviceAdjacency, personalized_pagerank
    big = s1
    n, g = big.n, big.graph
    lo, b = big.bounds
    ei = g.edge_index.cpu().numpy()
    A = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
    rng = np.random.RandomState(12)
    src = [lo - 1, lo, lo + 1, b - 1, b, b + 1, n - 1, n - 2, g.mega, g.hubs[0], 0, b + 700]
    src += rng.randint(0, n - 8, size=64 - len(src)).tolist()
    sources = torch.tensor(src, device=dev)
    adj = DeviceAdjacency(A.tocoo(), dev)
    assert n * 64 * 8 > (1 << 32) and n * 8 * 8 < (1 << 31) and adj.ppr_operator(0.85).workspace_bytes(64) > (1 << 32)
    runs = {}
    for S in (64, 8):
        monkeypatch.setattr(ssa.knobs, 'PPR_COLUMNS', S)
        runs[S] = personalized_pagerank(adj, sources)
        fixed = personalized_pagerank(adj, sources, tol=0.0, max_iter=6)
        if S == 64:
            short = fixed
        else:
            assert torch.equal(fixed[0], short[0]) and torch.equal(fixed[1], short[1]), 'fixed step count'
        del fixed
    monkeypatch.undo()
    wide, narrow = runs[64], runs[8]
    assert torch.equal(wide[1], narrow[1]), 'iteration counts'
    if not torch.equal(wide[0], narrow[0]):
        bad = (wide[0] != narrow[0]).any(dim=0).nonzero().flatten().cpu().numpy()
        raise AssertionError(R.report(bad, big.bounds, 'PPR vectors, 64 columns against 8'))
    assert int(wide[1].max()) > 6 and int(wide[1][7]) == 1           # (N - 2 is isolated: one step)
    cols = [4, 2]                                                      # sources 2^23 and 2^22 + 1
    ref, ref_iters, _ = pagerank_power(A, [src[j] for j in cols], tol=0.0, max_iter=6)
    for j, want in zip(cols, ref):
        vec = short[0][j].cpu().numpy()
        assert int(short[1][j]) == 6 and (want[b:] > 0).any() and (want[:b] > 0).any()
        np.testing.assert_allclose(vec, want, rtol=1e-10, atol=1e-300)


# ---------------------------------------------------------------------------------------------------
# S2: P = 256, p = 8 (S1 is released when it is built)
# ---------------------------------------------------------------------------------------------------
def test_plain_query_anchor_s2(s2, dev):
    """(1) crosses: the MinHash uint32 ELEMENT index r * 256 = 2^31 at row 2^23, MinHash bytes 2^32 / 2^33, HLL byte 2^31.  Reference:
    the C oracle on the compacted table; match and zero counts bit-exact, features within the plain query's tolerance.  On the inputs
    alone: the links read rows on both sides of every bound and the bound rows.  This lets the tests below trust the plain query at S2"""
    _check_anchor(s2, dev)


def test_score_links_s2(ssa, s2, dev):
    """(2) at P = 256: as test_score_links_s1, with the element index r * 256 crossing 2^31 at row 2^23"""
    _check_scores(ssa, s2, dev)


def test_topk_links_s2(s2, dev):
    """(3) at P = 256: as test_topk_links_s1 (`ur * P` / `v * P` as element indices reach 2^31 at row 2^23)"""
    _check_topk(s2, dev)


def test_rank_links_s2(ssa, s2, dev, monkeypatch):
    """(4) at P = 256: as test_rank_links_s1"""
    _check_rank(ssa, s2, dev, monkeypatch)


# ---------------------------------------------------------------------------------------------------
# S3: P = 64, p = 10, the run-time-size path (S2 is released when it is built)
# ---------------------------------------------------------------------------------------------------
def test_plain_query_anchor_s3(s3, dev):
    """(1) crosses: HLL rows of 1 024 bytes, byte 2^31 at row 2^21 and 2^32 at row 2^22 (`v * M` of the run-time-size path).
    Reference and conditions as test_plain_query_anchor_s2"""
    _check_anchor(s3, dev)


def test_score_links_s3(ssa, s3, dev):
    """(2) on the run-time-size path: as test_score_links_s1, HLL bytes 2^31 / 2^32 at rows 2^21 / 2^22"""
    _check_scores(ssa, s3, dev)


def test_topk_links_s3(s3, dev):
    """(3) on the run-time-size path: as test_topk_links_s1 around row 2^22"""
    _check_topk(s3, dev)


def test_rank_links_s3(ssa, s3, dev, monkeypatch):
    """(4) on the run-time-size path: as test_rank_links_s1 around rows 2^21 and 2^22"""
    _check_rank(ssa, s3, dev, monkeypatch)
