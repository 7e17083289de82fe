"""The fused stage (ss_fused_hop_stage) against the unfused sequence (ss_first_hop + ss_propagate, what SS_FUSED_STAGE=0 runs) on graphs
planted where the per-row work of the stage branches: the harmonic sum that is digested only for wavefronts holding a row off linear
counting, the "row lists itself" test, the path of rows that lie inside the current batch of 60 col entries and the loop of rows that
do not.  Built as tests/test_fused_posts_gpu.py: both MinHash tables, both HLL tables and both cardinality columns bit for bit, P = 64
and 128, buffer and flat posts (SS_FUSED_POSTS); at P = 128 the tables are also held to the CPU oracle, which shares no code with
either sequence (the two sequences share MinhashRows, at 4 and at 8 rows per wavefront: batches of 60 and of 56 entries).

Graph 1, `lc_graph`: hop-2 rows with exactly 147 and 148 non-zero registers (lc_min_zeros = 109 at p = 8: the last row of linear
counting and the first one off it).  A node's hop-0 row is one register, so a row is planted by choosing WHO feeds it (hll_planted
does the same): destination w has one in-neighbour, a collector t of its own, whose in-neighbours are one node per wanted register.
The row off linear counting sits at each of the four positions of a chunk of four rows; one chunk has none, one has four; a saturated
row (256 registers) and a row without entries (one register, its own) sit between such rows, and the last chunk ends in the row of a
node that no edge names (no self loop either: the all-zero row).  The same rows go through the HLL-only hop
(hll_propagate_row16_kernel, the ELPH call sequence) and their cardinalities are compared with the numpy restatement of the estimator.
This graph has 2 700 nodes, not a few hundred: every node owns ONE register, and the ids 0 .. n - 1 cover all 256 registers only
from n = 2 639 on (asserted below) -- there is no saturated row on fewer nodes.

Graph 2, `rows_graph` (400 nodes): chunks whose col entries total 59, 60, 61, 120 and 121; rows that start exactly at entry 60 and 120
of their chunk; a row of 130 entries over three batches (hub threshold 200); rows without entries in between; a hub row (210 entries)
skipped in the middle of a chunk; rows that list themselves once and twice -- alone in their row (first AND last entry whatever
order the CSR gives a row's sources), as the lowest and as the highest id of the row, in rows that straddle entry 60 on either side of
it, in the three-batch row; two rows of one chunk that list each other and not themselves; chunks with one such row and none."""
import functools
from argparse import Namespace
from ctypes import byref

import numpy as np
import pytest
import torch

import hll_planted as hp
from hll_planted import F32

gpu = pytest.mark.gpu

BATCH = 60  # col entries per batch of the fused stage: 64 lanes - 4 rows
M = 256


# ---- graph 1: the linear-counting boundary --------------------------------------------------------------------------------------------
LC_N = 2700
LC_HUB_THRESHOLD = 1024  # every row regular (the collectors have 146 .. 255 entries)
LONE, EMPTY, FULL = 1, 0, 256


@functools.lru_cache(maxsize=None)
def _lc_counts():
    prm = hp.params(hp.tables(8))
    on = M - prm.lc_min_zeros  # 147 registers: zeros == lc_min_zeros, the last linear-counting row
    return prm, on, on + 1


def lc_chunks():
    """first row of a chunk of four -> the number of non-zero registers planted in each of its hop-2 rows"""
    _, on, off = _lc_counts()
    return {2000: [off, on, on, on], 2004: [on, off, on, on], 2008: [on, on, off, on], 2012: [on, on, on, off],  # each position
            2016: [on] * 4, 2020: [off] * 4,                                                                       # none, all four
            2024: [FULL, off, LONE, on],                     # a saturated row and a row without entries next to such rows
            LC_N - 4: [off, FULL, on, EMPTY]}                # ... and the all-zero row of the last node


@functools.lru_cache(maxsize=None)
def lc_graph():
    """-> (edge_index int64 [2, E], want {row: registers})"""
    from oracle import oracle
    n = LC_N
    hop0 = oracle.hll_init(n, 8)
    assert ((hop0 != 0).sum(axis=1) == 1).all()
    reg = np.argmax(hop0, axis=1)
    want = {first + k: c for first, counts in lc_chunks().items() for k, c in enumerate(counts)}
    collectors = {w: 1900 + j for j, w in enumerate(sorted(want))}
    taken = set(want) | set(collectors.values())
    by_reg = {}
    for i in range(n - 4):
        if i not in taken:
            by_reg.setdefault(int(reg[i]), []).append(i)
    assert len(by_reg) == M, 'the feeding nodes must cover every register (ids below 2 639 do not)'
    assert len(set(reg[:2638].tolist())) < M
    rng = np.random.RandomState(3)
    src, dst = [], []
    for w, count in sorted(want.items()):
        if count in (LONE, EMPTY):
            continue
        t = collectors[w]
        fixed = {int(reg[w]), int(reg[t])}  # (row 2 of w folds rows 1 of t and of w itself: the registers t collects, t's and w's)
        others = [int(r) for r in rng.permutation(M) if r not in fixed][:count - len(fixed)]
        for j, r in enumerate(others):
            for u in by_reg[r][:2 if j < 12 else 1]:  # (a second feeder on the same register for a dozen of them: a max is taken)
                src.append(u)
                dst.append(t)
        src.append(t)
        dst.append(w)
    ei = np.array([src, dst], dtype=np.int64)
    assert int(ei.max()) == n - 2 and not (ei == n - 1).any()  # (inferred self loops for every node but the last)
    return ei, want


def hll_hops(n, ei, hops=2):
    """HLL rows of hops 1 .. `hops` in numpy: max over the in-neighbours and -- nodes below max(edge_index) + 1 -- the row itself"""
    from oracle import oracle
    x = oracle.hll_init(n, 8)
    n_self = int(ei.max()) + 1
    out = []
    for _ in range(hops):
        y = np.zeros_like(x)
        y[:n_self] = x[:n_self]
        np.maximum.at(y, ei[1], x[ei[0]])
        out.append(y)
        x = y
    return out


# ---- graph 2: self edges and batch boundaries ------------------------------------------------------------------------------------------
ROWS_N = 400
ROWS_HUB_THRESHOLD = 200
FIRST = 200  # planted rows 200 .. 231; sources below 200 (`lo`) or from 300 (`hi`): a row's own id is its lowest or its highest source
# per row: (sources below the row, sources above it, times it lists itself, other rows it lists)
ROWS_CHUNKS = [
    [(19, 0, 1, ()), (0, 19, 0, ()), (0, 0, 0, ()), (0, 18, 2, ())],          # 59: once as the highest id, twice as the lowest, an empty row
    [(15, 0, 0, ()), (15, 0, 0, ()), (0, 14, 0, (207,)), (14, 0, 0, (206,))],  # 60: rows 206 and 207 list each other, nobody itself
    [(20, 0, 0, ()), (0, 20, 0, ()), (20, 0, 0, ()), (0, 0, 1, ())],          # 61: row 211 is its self edge alone, at entry 60
    [(60, 0, 0, ()), (0, 0, 0, ()), (0, 30, 0, ()), (30, 0, 0, ())],          # 120: row 214 starts at entry 60, behind an empty row
    [(50, 0, 0, ()), (0, 28, 2, ()), (39, 0, 1, ()), (0, 1, 0, ())],          # 121: row 217 straddles entry 60, row 219 starts at 120
    [(55, 0, 0, ()), (9, 0, 1, ()), (0, 3, 0, ()), (2, 0, 0, ())],            # row 221 straddles entry 60, itself as the highest id
    [(10, 0, 0, ()), (65, 64, 1, ()), (0, 5, 0, ()), (3, 0, 0, ())],          # row 225: 130 entries, batches 0, 1 and 2
    [(25, 0, 0, ()), (120, 90, 0, ()), (0, 25, 0, ()), (30, 0, 0, ())],       # row 229: 210 entries, a hub row skipped mid-chunk
]
ROWS_TOTALS = [59, 60, 61, 120, 121, 70, 148, 290]


@functools.lru_cache(maxsize=None)
def rows_graph():
    src, dst = [], []
    for c, chunk in enumerate(ROWS_CHUNKS):
        for k, (n_lo, n_hi, n_own, others) in enumerate(chunk):
            i = FIRST + 4 * c + k
            row = [(11 * i + 7 * j) % 200 for j in range(n_lo)] + [300 + (13 * i + 3 * j) % 100 for j in range(n_hi)]
            row = list(others) + row[:len(row) // 2] + [i] * n_own + row[len(row) // 2:]
            src += row
            dst += [i] * len(row)
    src.append(ROWS_N - 1)  # (the inferred self loops reach every node)
    dst.append(0)
    return np.array([src, dst], dtype=np.int64)


def test_the_graphs_plant_what_they_claim():
    # graph 1
    prm, on, off = _lc_counts()
    assert (on, off, prm.lc_min_zeros) == (147, 148, 109)
    ei, want = lc_graph()
    h1, h2 = hll_hops(LC_N, ei)
    got = (h2 != 0).sum(axis=1)
    for w, count in want.items():
        assert got[w] == count, (w, int(got[w]), count)
    V, S, _ = hp.stats(h2[sorted(want)])
    for w, v, s in zip(sorted(want), V, S):
        if want[w] != EMPTY:
            assert hp.estimate32(prm, int(v), float(s))[1] == (hp.BRANCH_LC if want[w] <= on else hp.BRANCH_BIAS), w
    chunks = lc_chunks()
    assert all(first % 4 == 0 for first in chunks)
    where_off = [tuple(k for k, c in enumerate(counts) if c == off) for counts in chunks.values()]
    assert {(0,), (1,), (2,), (3,), (), (0, 1, 2, 3)} <= set(where_off)
    assert not h2[LC_N - 1].any() and (h2[2026] != 0).sum() == 1 and (h2[2024] != 0).all() and (h2[LC_N - 3] != 0).all()
    deg = np.bincount(ei[1], minlength=LC_N)
    assert deg.max() <= LC_HUB_THRESHOLD and all(deg[w] == (0 if c in (LONE, EMPTY) else 1) for w, c in want.items())
    # graph 2
    ei = rows_graph()
    assert int(ei.max()) == ROWS_N - 1
    deg = np.bincount(ei[1], minlength=ROWS_N)
    deg[0] -= 1
    planted = deg[FIRST:FIRST + 4 * len(ROWS_CHUNKS)].reshape(-1, 4)
    assert planted.sum(axis=1).tolist() == ROWS_TOTALS and {59, 60, 61, 120, 121} <= set(ROWS_TOTALS)
    assert not deg[:FIRST].any() and not deg[FIRST + 4 * len(ROWS_CHUNKS):].any()
    start = np.concatenate([np.zeros((len(planted), 1), np.int64), np.cumsum(planted, axis=1)[:, :3]], axis=1)  # first entry, chunk-relative
    own = np.zeros(ROWS_N, np.int64)
    np.add.at(own, ei[1][ei[0] == ei[1]], 1)
    rows = {i: (int(start[(i - FIRST) // 4, (i - FIRST) % 4]), int(deg[i]), int(own[i])) for i in range(FIRST, FIRST + planted.size)}
    assert rows[211] == (BATCH, 1, 1) and rows[214][0] == BATCH and rows[219][0] == 2 * BATCH and rows[213][1] == 0 and rows[202][1] == 0
    assert rows[200][2] == 1 and rows[203][2] == 2 and sorted(own[FIRST:FIRST + 4].tolist()) == [0, 0, 1, 2]
    for i in (217, 221):  # rows with self edges across entry 60
        s, d, o = rows[i]
        assert s < BATCH < s + d and o >= 1
    lists = lambda i: set(ei[0][ei[1] == i].tolist())
    assert min(lists(217)) == 217 and max(lists(221)) == 221 and min(lists(203)) == 203 and max(lists(200)) == 200
    s, d, o = rows[225]
    assert s // BATCH == 0 and (s + d - 1) // BATCH == 2 and o == 1 and d <= ROWS_HUB_THRESHOLD
    assert rows[229][1] > ROWS_HUB_THRESHOLD and max(d for i, (s, d, o) in rows.items() if i != 229) <= ROWS_HUB_THRESHOLD
    assert rows[230][0] // BATCH != (rows[230][0] + rows[230][1] - 1) // BATCH  # (the row behind the hub row straddles a batch too)
    assert 207 in lists(206) and 206 in lists(207) and own[206] == own[207] == 0
    assert own[208:212].tolist() == [0, 0, 0, 1] and not own[204:208].any()
    for i in rows:  # no duplicate among a row's sources but its own id
        col = ei[0][ei[1] == i]
        assert len(set(col.tolist())) == len(col) - max(rows[i][2] - 1, 0), i


# ---- the two sequences -----------------------------------------------------------------------------------------------------------------
GRAPHS = {'lc': (LC_N, LC_HUB_THRESHOLD, lambda: lc_graph()[0]), 'rows': (ROWS_N, ROWS_HUB_THRESHOLD, rows_graph)}


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, P, **kw):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True), **kw)
    eh.hll_tables = hp.tables(8)
    return eh


_unfused = {}


def unfused(ssa, dev, name, P):
    """ss_first_hop + ss_propagate, once per graph and P"""
    if (name, P) not in _unfused:
        n, _, edges = GRAPHS[name]
        table, cards = _eh(ssa, P, fuse_hop_stage=False).build_hash_tables(n, torch.from_numpy(edges()).to(dev))
        torch.cuda.synchronize()
        _unfused[(name, P)] = (table[1].mh_u32.clone(), table[1].hll_u8.clone(), table[2].mh_u32.clone(), table[2].hll_u8.clone(), cards.clone())
    return _unfused[(name, P)]


def fused(ssa, dev, name, P):
    """ss_fused_hop_stage on the same graph; hop-2 MinHash is part of the stage at P = 128 only"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    n, _, edges = GRAPHS[name]
    eh = _eh(ssa, P)
    csr = ssa.hashing.build_csr(torch.from_numpy(edges()).to(dev), n, dev, check=False)
    csr.use_inferred_self_loops = True
    graph = csr.struct()
    ab, params = eh._perms(dev), eh._params(dev)
    mh = [torch.full((n, P), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    hll = [torch.full((n, M), 255, dtype=torch.uint8, device=dev) for _ in range(2)]
    cards = torch.full((n, 2), -1.0, dtype=torch.float32, device=dev)
    rc = ssa._native.lib().ss_fused_hop_stage(byref(graph), _ptr(ab[0]), _ptr(ab[1]), P, _ptr(mh[0]), _ptr(mh[1]) if P == 128 else None, 8,
                                              _ptr(hll[0]), _ptr(cards), _ptr(hll[1]), _ptr(cards[:, 1]), 2, byref(params.struct),
                                              _stream(dev))
    assert rc == 0, f'ss_fused_hop_stage returned {rc}'
    torch.cuda.synchronize()
    return mh[0], hll[0], mh[1], hll[1], cards


@functools.lru_cache(maxsize=None)
def _oracle_tables(name):
    from oracle import oracle
    n, _, edges = GRAPHS[name]
    return oracle.build_hash_tables(n, edges(), 2, 128, hp.oracle_params(hp.tables(8)))


def _check_cards(got, regs, what):
    """cardinalities of register rows against the numpy restatement: bit for bit where fp32 adds the harmonic sum exactly in any order,
    at the project's RTOL elsewhere (the bar of tests/test_hll_planted_gpu.py) -> the branch of every row"""
    prm = _lc_counts()[0]
    V, S, exact = hp.stats(regs)
    want, branch = np.zeros(len(regs), F32), np.zeros(len(regs), np.int32)
    for i in range(len(regs)):
        want[i], branch[i] = hp.estimate32(prm, int(V[i]), float(S[i]))
    got = np.asarray(got, dtype=F32)
    exact = np.asarray(exact)
    assert np.array_equal(got[exact].view(np.int32), want[exact].view(np.int32)), what
    np.testing.assert_allclose(got[~exact], want[~exact], rtol=hp.RTOL, atol=0, err_msg=what)
    return branch


@gpu
@pytest.mark.parametrize('posts', ['buffer', 'flat'])
@pytest.mark.parametrize('P', [64, 128])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_fused_stage_equals_the_unfused_sequence(ssa, dev, monkeypatch, name, P, posts):
    n, threshold, edges = GRAPHS[name]
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    monkeypatch.delenv('SS_FUSED_POSTS', raising=False)
    monkeypatch.delenv('SS_SELF_SKIP', raising=False)
    want = unfused(ssa, dev, name, P)
    monkeypatch.setenv('SS_FUSED_POSTS', posts)
    got = fused(ssa, dev, name, P)
    assert torch.equal(got[0], want[0]), 'hop-1 MinHash'
    assert torch.equal(got[1], want[1]), 'hop-1 HLL'
    assert torch.equal(got[3], want[3]), 'hop-2 HLL'
    assert torch.equal(got[4].view(torch.int32), want[4].view(torch.int32)), 'cards of hops 1 and 2'
    if P == 128:
        assert torch.equal(got[2], want[2]), 'hop-2 MinHash'
        otab, ocards = _oracle_tables(name)
        for k, (mh, hll) in enumerate(((got[0], got[1]), (got[2], got[3])), start=1):
            assert np.array_equal(mh.cpu().numpy().view(np.uint32), otab[k]['minhash']), f'hop-{k} MinHash against the oracle'
            assert np.array_equal(hll.cpu().numpy(), otab[k]['hll']), f'hop-{k} HLL against the oracle'
        np.testing.assert_allclose(got[4].cpu().numpy(), ocards, rtol=hp.RTOL, atol=1e-4)
    regs, cards = got[3].cpu().numpy(), got[4].cpu().numpy()
    branch = _check_cards(cards[:, 1], regs, 'hop-2 cards against the numpy estimator')
    _check_cards(cards[:, 0], got[1].cpu().numpy(), 'hop-1 cards against the numpy estimator')
    if name == 'lc':
        _, on, off = _lc_counts()
        for w, count in lc_graph()[1].items():
            assert int((regs[w] != 0).sum()) == count, w
            assert branch[w] == (hp.BRANCH_LC if count <= on else hp.BRANCH_BIAS), w
        assert not regs[LC_N - 1].any() and not got[0][LC_N - 1].any() and cards[LC_N - 1, 1] == 0.0, 'the all-zero row of the last node'


@gpu
def test_hll_only_hop_on_the_linear_counting_boundary(ssa, dev, monkeypatch):
    """the rows of graph 1 through hll_propagate_row16_kernel (hll_prop, the ELPH call sequence: explicit self loops for every node
    but the last): tables and carried cardinalities equal to the unfused build's bit for bit, and to the numpy estimator"""
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', LC_HUB_THRESHOLD)
    monkeypatch.delenv('SS_SELF_SKIP', raising=False)
    want = unfused(ssa, dev, 'lc', 128)
    eh = _eh(ssa, 128)
    ei = torch.from_numpy(lc_graph()[0]).to(dev)
    hei = torch.cat([ei, torch.arange(LC_N - 1, device=dev).repeat(2, 1)], dim=1)
    x = eh.initialise_hll(LC_N)
    for k in (1, 2):
        x = eh.hll_prop(x, hei)
        regs = x.cpu().numpy().view(np.uint8)
        assert np.array_equal(regs, want[2 * k - 1].cpu().numpy()), f'hop-{k} HLL'
        assert x._ss_count is not None, 'hll_prop carries the cardinalities its kernel computed'
        cards = eh.hll_count(x).cpu().numpy()
        assert np.array_equal(cards.view(np.int32), want[4][:, k - 1].cpu().numpy().view(np.int32)), f'hop-{k} cards'
        _check_cards(cards, regs, f'hll_prop hop {k} against the numpy estimator')
