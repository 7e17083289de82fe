"""csrc/ss_ppr.hip on the planted graph of tests/ppr_planted.py, against the fp64 restatement (tests/ppr_restatement.py): every
in-degree at which ppr_gather takes another trip, the hub rule at 256 / 257 kept entries, last segments of 1, 2, 255 and 256 edges,
1 / 4 / 5 / 9 hubs, every boundary width, columns that stop inside a pair and inside a slice, the C ABI into guarded and poisoned
workspaces, and iterate offsets past 2^31 elements.  Vectors at rtol = 1e-10 (every kept weight is positive: asserted in
tests/test_ppr_planted_host.py), iteration counts for equality (no restated residual lies within 1e-6 tol of tol: asserted there
too), everything said to be the same bits with torch.equal on integer views."""
import ctypes
import time

import numpy as np
import pytest
import torch

import ppr_planted as pp
from large_table_helpers import require_free_memory
from ppr_restatement import pagerank_power

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 63, 64, 65, 128, 129)
GUARD = 64 << 10
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as ssa
    return ssa


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda', torch.cuda.current_device())


def _bits(t):
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _compare(got, iters, ref, ref_iters, desc, what):
    """vectors within 1e-10 relative of the restatement, iteration counts equal; a failure names the planted rows"""
    assert np.array_equal(iters, ref_iters), (what, np.nonzero(iters != ref_iters)[0], iters, ref_iters)
    worst = pp.worst_relative(got, ref)
    print(f'\n[ppr planted] {what}: {got.shape[0]} sources, worst relative error against the restatement {worst:.3e}')
    try:
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-300)
    except AssertionError as e:
        raise AssertionError(f'{what}: {e}\n{pp.worst_by_row(got, ref, desc)}') from None


def _links_of(srcs, desc, seed):
    """three links per source: to a hub row, to itself, to a random node"""
    rng = np.random.RandomState(seed)
    hubs = np.array(desc['hubs'])
    s = np.asarray(srcs, dtype=np.int64)
    dst = np.concatenate([hubs[np.arange(len(s)) % len(hubs)], s, rng.randint(0, pp.N, size=len(s))])
    return torch.from_numpy(np.stack([np.tile(s, 3), dst], 1))


# ---- a. every planted row, every variant -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(pp.VARIANTS))
def test_every_planted_row(name, ssa, dev):
    A, desc = pp.variant(name)
    srcs, ref, ref_iters, _ = pp.restated(name, 'rows', 'rows')
    vec, iters = ssa.heuristics.personalized_pagerank(A, torch.tensor(srcs), **pp.ROWS_CFG)
    op = ssa.heuristics._adjacency(A, dev).ppr_operator(pp.ROWS_CFG['p'])
    assert (op.n_hubs, op.n_segments) == pp.COUNTS[name]
    vec, iters = vec.numpy(), iters.numpy()
    for j, s in enumerate(srcs):
        if s in pp.QUICK:
            assert iters[j] == 1 and np.array_equal(vec[j], np.eye(1, pp.N, s)[0]), s
        else:
            assert iters[j] == pp.ROWS_CFG['max_iter'], (s, iters[j])
    _compare(vec, iters, ref, ref_iters, desc, f'rows of `{name}`')


# ---- b. widths ---------------------------------------------------------------------------------------------------------------------
def test_boundary_widths_give_the_same_bits(ssa, dev):
    from subgraph_sketching_amd.heuristics import PPR, personalized_pagerank
    A, desc = pp.variant('nine')
    srcs, ref, ref_iters, _ = pp.restated('nine', 'widths', 'rows')
    assert len(srcs) == 129 and set(desc['hubs']) | set(pp.QUICK) <= set(srcs)
    sources = torch.tensor(srcs)
    perm = torch.from_numpy(np.random.RandomState(2).permutation(len(srcs)))
    links = _links_of(srcs, desc, seed=3)
    assert (links[:, 0] == links[:, 1]).sum() >= 129 and np.isin(links[:, 1].numpy(), desc['hubs']).sum() >= 129
    vec, iters = personalized_pagerank(A, sources, **pp.ROWS_CFG)
    scores, order = PPR(A, links, **pp.ROWS_CFG)
    _compare(vec.numpy(), iters.numpy(), ref, ref_iters, desc, 'widths of `nine`')
    col = {s: j for j, s in enumerate(srcs)}
    rows = torch.tensor([col[int(s)] for s in order[0]])
    assert _same(scores, vec[rows, order[1]].to(torch.float32))          # one fp32 rounding of the fp64 vector
    saved = ssa.knobs.PPR_COLUMNS
    try:
        for S in WIDTHS:                                                       # tail batches: 64 + 64 + 1, 65 + 64, 128 + 1
            ssa.knobs.PPR_COLUMNS = S
            v, it = personalized_pagerank(A, sources, **pp.ROWS_CFG)
            assert _same(v, vec) and _same(it, iters), S
            vp, ip = personalized_pagerank(A, sources[perm], **pp.ROWS_CFG)
            assert _same(vp, vec[perm]) and _same(ip, iters[perm]), S
            sc, od = PPR(A, links, **pp.ROWS_CFG)
            assert torch.equal(od, order) and _same(sc, scores), S
    finally:
        ssa.knobs.PPR_COLUMNS = saved


# ---- c. stops inside a pair and inside a slice -------------------------------------------------------------------------------------
def test_stops_inside_a_pair_and_inside_a_slice(ssa, dev):
    from subgraph_sketching_amd.heuristics import personalized_pagerank
    A, desc = pp.variant('five')
    srcs, ref, ref_iters, _ = pp.restated('five', 'stops', 'stops')
    order, pairs = pp.stop_order(srcs, ref_iters)
    at = {s: j for j, s in enumerate(srcs)}
    alone_of = list(dict.fromkeys(order))
    saved = ssa.knobs.PPR_COLUMNS
    try:
        ssa.knobs.PPR_COLUMNS = 1
        alone_vec, alone_it = personalized_pagerank(A, torch.tensor(alone_of), **pp.STOPS_CFG)
        ssa.knobs.PPR_COLUMNS = 128
        for what, lst in (('quick slice last', order), ('quick slice first', order[::-1])):
            vec, iters = personalized_pagerank(A, torch.tensor(lst), **pp.STOPS_CFG)
            idx = [at[s] for s in lst]
            _compare(vec.numpy(), iters.numpy(), ref[idx], ref_iters[idx], desc, f'stops, {what}')
            k = iters.tolist()
            if lst is order:                                                   # the pattern ran as planned
                assert 1 < k[0] < k[1] and k[2] > k[3] > 1 and k[4] == 1 < k[5] and k[6] > 1 == k[7]
                assert min(k[:4] + k[8:64]) > 1 and set(k[64:]) == {1}
            else:
                assert set(k[:64]) == {1} and k[126] > k[127] > 1 and 1 < k[124] < k[125]
            single = torch.tensor([alone_of.index(s) for s in lst])
            assert _same(vec, alone_vec[single]) and _same(iters, alone_it[single]), what
    finally:
        ssa.knobs.PPR_COLUMNS = saved


# ---- d. straight through the C ABI -------------------------------------------------------------------------------------------------
class _Direct(object):
    """one batch through ss_ppr_begin / iterate x max_iter / status / vectors / scores, into a workspace at a given address"""

    def __init__(self, ssa, dev, A, cfg):
        self.lib, self.dev, self.cfg = ssa._native.lib(), dev, cfg
        self.op = ssa.heuristics._adjacency(A, dev).ppr_operator(cfg['p'])
        self.g = ctypes.byref(self.op.struct)
        self.N = self.op.num_nodes
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def need(self, S):
        return self.op.workspace_bytes(S)

    def run(self, addr, nbytes, srcs, dst, link_col):
        lib, g, dev, S = self.lib, self.g, self.dev, len(srcs)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        ws = ctypes.c_void_p(addr)
        src_d = torch.tensor(srcs, dtype=torch.int64, device=dev)
        dst_d = torch.tensor(dst, dtype=torch.int64, device=dev)
        col_d = torch.tensor(link_col, dtype=torch.int32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)                  # [0] ss_ppr_begin's, [1] ss_ppr_scores'
        iters = torch.full((S,), -7, dtype=torch.int32, device=dev)
        n_active = torch.full((1,), -7, dtype=torch.int32, device=dev)
        vec = torch.full((S, self.N), float('nan'), dtype=torch.float64, device=dev)
        out = torch.full((len(dst),), float('nan'), dtype=torch.float32, device=dev)
        tol, max_iter = float(self.cfg['tol']), int(self.cfg['max_iter'])
        assert lib.ss_ppr_begin(g, p(src_d), S, tol, ws, nbytes, p(flags), self.stream) == 0
        for k in range(1, max_iter + 1):
            assert lib.ss_ppr_iterate(g, S, k, max_iter, tol, ws, nbytes, self.stream) == 0
        assert lib.ss_ppr_status(g, S, ws, nbytes, p(iters), p(n_active), self.stream) == 0
        assert lib.ss_ppr_vectors(g, S, ws, nbytes, p(vec), self.stream) == 0
        assert lib.ss_ppr_scores(g, S, p(dst_d), p(col_d), len(dst), ws, nbytes, p(out), ctypes.c_void_p(flags.data_ptr() + 4),
                                 self.stream) == 0
        torch.cuda.synchronize(dev)
        assert int(n_active.item()) == 0
        return vec.cpu(), iters.cpu(), out.cpu(), flags.cpu().tolist()


def _direct_case(S, desc):
    """(S distinct sources with hubs and quick ones among them, dst and link_col of 257 links: one past a workgroup of the scores kernel)"""
    rows = pp.sources(desc, 'rows')
    top = max(desc['hubs'], key=lambda h: desc['in_rows'][h])
    srcs = rows[:S] if S > 3 else [top, pp.SINK, rows[-1]]
    rng = np.random.RandomState(40 + S)
    link_col = rng.randint(0, S, size=257)
    dst = rng.randint(0, pp.N, size=257)
    dst[:S] = np.asarray(srcs)[link_col[:S]]                                   # dst == src
    dst[S:S + 5] = desc['hubs']
    link_col[-1], dst[-1] = S - 1, pp.N - 1                                    # the last column, the last row, the lone last thread
    return srcs, dst.tolist(), link_col.tolist()


@pytest.fixture(scope='module')
def direct(ssa, dev):
    A, desc = pp.variant('five')
    return _Direct(ssa, dev, A, pp.ROWS_CFG), A, desc


@pytest.fixture(scope='module', params=[65, 3])
def guarded(request, direct, ssa, dev):
    """the module path's bits and a direct run into the middle of a sentinel-filled buffer"""
    from subgraph_sketching_amd.heuristics import PPR, personalized_pagerank
    d, A, desc = direct
    S = request.param
    srcs, dst, link_col = _direct_case(S, desc)
    vec, iters = personalized_pagerank(A, torch.tensor(srcs), **pp.ROWS_CFG)
    links = torch.tensor([[srcs[c], v] for c, v in zip(link_col, dst)])
    scores, order = PPR(A, links, **pp.ROWS_CFG)
    by_link = {(int(s), int(v)): x for s, v, x in zip(order[0], order[1], scores)}
    scores = torch.stack([by_link[(srcs[c], v)] for c, v in zip(link_col, dst)])
    need = d.need(S)
    buf = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    addr = buf.data_ptr() + GUARD
    assert need > 0 and need % 256 == 0 and addr % 256 == 0
    got = d.run(addr, need, srcs, dst, link_col)
    return dict(S=S, srcs=srcs, dst=dst, link_col=link_col, module=(vec, iters, scores), got=got, buf=buf, addr=addr, need=need)


def test_direct_launch_into_a_guarded_workspace(guarded, direct):
    vec, iters, scores = guarded['module']
    gvec, giters, gscores, flags = guarded['got']
    buf, need = guarded['buf'], guarded['need']
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + need:] == SENTINEL).all())
    assert flags == [0, 0]
    assert _same(gvec, vec) and _same(giters, iters) and _same(gscores, scores)
    quick = [j for j, s in enumerate(guarded['srcs']) if s in pp.QUICK]
    assert quick and all(int(giters[j]) == 1 for j in quick) and int(giters.max()) == pp.ROWS_CFG['max_iter']
    want = vec[torch.tensor(guarded['link_col']), torch.tensor(guarded['dst'])].to(torch.float32)
    assert _same(gscores, want) and int((want != 0).sum()) > 128              # out[l] == np.float32(vectors[col, dst])


def test_poisoned_and_leftover_workspace(guarded, direct, dev):
    """every byte of the workspace NaN patterns, then the leftovers of a batch carved with another Sp: the pad column of x[1], segp
    and part, and everything ss_ppr_begin does not clear, never reach a result"""
    d, A, desc = direct
    S, other = guarded['S'], {65: 64, 3: 4}[guarded['S']]
    nbytes = max(d.need(S), d.need(other))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    base = guarded['got']
    first = d.run(ws.data_ptr(), nbytes, guarded['srcs'], guarded['dst'], guarded['link_col'])
    o_srcs, o_dst, o_col = _direct_case(other, desc) if other > 3 else ([pp.B, 0, 63, 64], [0] * 257, [1] * 257)
    d.run(ws.data_ptr(), nbytes, o_srcs[::-1], o_dst, o_col)
    second = d.run(ws.data_ptr(), nbytes, guarded['srcs'], guarded['dst'], guarded['link_col'])
    for got in (first, second):
        assert _same(got[0], base[0]) and _same(got[1], base[1]) and _same(got[2], base[2]) and got[3] == [0, 0]


def test_bad_links_score_zero_and_leave_their_neighbours(guarded, direct):
    d = direct[0]
    S, base = guarded['S'], guarded['got']
    dst, link_col = list(guarded['dst']), list(guarded['link_col'])
    bad = {17: (pp.N, None), 100: (-1, None), 200: (None, S), 255: (None, -1)}
    for l, (v, c) in bad.items():
        if v is not None:
            dst[l] = v
        if c is not None:
            link_col[l] = c
    vec, iters, scores, flags = d.run(guarded['addr'], guarded['need'], guarded['srcs'], dst, link_col)
    assert flags == [0, 1]
    good = torch.ones(257, dtype=torch.bool)
    good[list(bad)] = False
    assert _same(scores[good], base[2][good]) and _same(scores[~good], torch.zeros(4))
    assert _same(vec, base[0]) and _same(iters, base[1])


def test_a_bad_source_in_an_odd_batch(guarded, direct):
    d = direct[0]
    S, base = guarded['S'], guarded['got']
    for swaps in ([(S // 2 - 1, pp.N), (S // 2, -1)] if S > 3 else [(1, pp.N)], [(S // 2, -1)]):
        srcs = list(guarded['srcs'])
        for j, s in swaps:
            srcs[j] = s
        vec, iters, scores, flags = d.run(guarded['addr'], guarded['need'], srcs, guarded['dst'], guarded['link_col'])
        assert flags == [1, 0]
        bad = torch.zeros(S, dtype=torch.bool)
        bad[[j for j, _ in swaps]] = True
        assert _same(vec[bad], torch.zeros((int(bad.sum()), pp.N), dtype=torch.float64)) and not bool(iters[bad].any())
        assert _same(vec[~bad], base[0][~bad]) and _same(iters[~bad], base[1][~bad])
        on_good = ~bad[torch.tensor(guarded['link_col'])]
        assert _same(scores[on_good], base[2][on_good]) and _same(scores[~on_good], torch.zeros(int((~on_good).sum())))
    buf, need = guarded['buf'], guarded['need']
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + need:] == SENTINEL).all())


def test_return_codes_launch_nothing(direct, ssa, dev):
    d, A, desc = direct
    lib, g, S = d.lib, d.g, 65
    OK, INVALID, WORKSPACE = (ssa._native.DEFINES[k] for k in ('SS_OK', 'SS_ERR_INVALID_ARG', 'SS_ERR_WORKSPACE'))
    assert (OK, INVALID, WORKSPACE) == (0, -1, -3)
    nh, ns = d.op.n_hubs, d.op.n_segments
    assert lib.ss_ppr_workspace_bytes(pp.N, 0, nh, ns) == 0 and lib.ss_ppr_workspace_bytes(pp.N, 4097, nh, ns) == 0
    assert lib.ss_ppr_workspace_bytes(1 << 31, 1, 0, 0) == 0 and lib.ss_ppr_workspace_bytes(pp.N, 4096, nh, ns) > 0
    need = d.need(S)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.full((need,), SENTINEL, dtype=torch.uint8, device=dev)
    srcs = torch.zeros(S, dtype=torch.int64, device=dev)
    dst = torch.zeros(4, dtype=torch.int64, device=dev)
    col = torch.zeros(4, dtype=torch.int32, device=dev)
    flag = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    iters = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    vec = torch.full((S, pp.N), 3.0, dtype=torch.float64, device=dev)
    out = torch.full((4,), 3.0, dtype=torch.float32, device=dev)
    w, st = p(ws), d.stream
    assert lib.ss_ppr_begin(g, p(srcs), S, 1e-6, w, need - 1, p(flag), st) == WORKSPACE
    assert lib.ss_ppr_iterate(g, S, 1, 12, 1e-6, w, need - 1, st) == WORKSPACE
    assert lib.ss_ppr_status(g, S, w, need - 1, p(iters), p(flag), st) == WORKSPACE
    assert lib.ss_ppr_vectors(g, S, w, need - 1, p(vec), st) == WORKSPACE
    assert lib.ss_ppr_scores(g, S, p(dst), p(col), 4, w, need - 1, p(out), p(flag), st) == WORKSPACE
    assert lib.ss_ppr_iterate(g, S, 0, 12, 1e-6, w, need, st) == INVALID
    assert lib.ss_ppr_scores(g, S, p(dst), p(col), 0, w, need, p(out), p(flag), st) == OK
    torch.cuda.synchronize(dev)
    assert bool((ws == SENTINEL).all()) and int(flag.item()) == SENTINEL and bool((iters == SENTINEL).all())
    assert bool((vec == 3.0).all()) and bool((out == 3.0).all())


# ---- e. offsets past 2^31 elements -------------------------------------------------------------------------------------------------
def test_iterate_offsets_past_2_31_elements(ssa, dev):
    """N = 1 100 000 rows of 2 048 columns: v * Sp + c passes 2^31 at row 2^20.  Scores of sources and destinations on both sides of
    that row against the restatement of 24 of the columns (columns are independent), after three steps"""
    from subgraph_sketching_amd.heuristics import PPR
    n, S, line_row = 1100000, 2048, 1 << 20
    t0 = time.perf_counter()
    A, last, line = pp.ring_graph(n)
    planted = np.concatenate([last, line, [0]])
    fill = np.setdiff1d(np.linspace(1, line_row - 2, S).astype(np.int64), planted)[:S - len(planted)]
    srcs = np.sort(np.concatenate([planted, fill]))
    assert len(np.unique(srcs)) == S and srcs[0] == 0 and srcs[-1] == n - 1 and np.isin(line, srcs).all()
    parts = [np.stack([srcs, (srcs + k) % n], 1) for k in range(4)]
    parts += [np.stack([np.repeat(last, 3), np.tile(line, 64)], 1), np.stack([np.tile(line, 64), np.repeat(last, 3)], 1)]
    links = torch.from_numpy(np.concatenate(parts))
    op = ssa.heuristics._adjacency(A, dev).ppr_operator(0.85)
    nbytes = op.workspace_bytes(S)
    assert nbytes > 2 * n * S * 8 and S * n > 1 << 31
    require_free_memory(dev, 2 * nbytes + (1 << 30), f'personalised PageRank at N = {n}, S = {S}')
    saved = ssa.knobs.PPR_COLUMNS
    try:
        ssa.knobs.PPR_COLUMNS = S
        assert op.columns(S) == S                                              # the width is not halved for lack of memory
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        scores, order = PPR(A, links, max_iter=3, tol=0)
        t2 = time.perf_counter()
    finally:
        ssa.knobs.PPR_COLUMNS = saved
        torch.cuda.empty_cache()
    subset = np.unique(np.concatenate([last[::7], line, [0], fill[::len(fill) // 10][:10]]))
    assert len(subset) == 24 and n - 1 in subset
    ref, ref_iters, _ = pagerank_power(A, subset.tolist(), p=0.85, tol=0, max_iter=3)
    assert (ref_iters == 3).all()
    row = {int(s): j for j, s in enumerate(subset)}
    src, dst = order[0].numpy(), order[1].numpy()
    take = np.isin(src, subset)
    expect = np.array([ref[row[int(s)], int(v)] for s, v in zip(src[take], dst[take])], dtype=np.float32)
    got = scores.numpy()[take]
    assert len(np.unique(src[take][src[take] >= line_row])) >= 8 and len(np.unique(dst[take][dst[take] >= line_row])) >= 8
    assert np.count_nonzero(expect) > len(expect) // 2
    worst = pp.worst_relative(got.astype(np.float64), expect.astype(np.float64))
    print(f'\n[ppr planted] offsets past 2^31: workspace {nbytes} bytes, {len(subset)} columns and {take.sum()} scores compared, worst '
          f'relative error {worst:.3e}; graph and links {t1 - t0:.2f} s, PPR {t2 - t1:.2f} s, restatement {time.perf_counter() - t2:.2f} s')
    np.testing.assert_allclose(got, expect, rtol=1e-6, atol=1e-30)
