"""Every table kernel across the 2 GiB and 4 GiB offset boundaries.  Needs a real MI355X: `-m gpu`.

Every kernel addresses rows of an [N, row] table by base + row * row_bytes.  With the default sketch shape a MinHash row is 512
bytes and an HLL row 256: MinHash row 2^22 starts at byte 2^31, row 2^23 at byte 2^32 (where the HLL row starts at byte 2^31), and
at row 2^24 the MinHash uint32 ELEMENT index reaches 2^31 and the HLL byte offset 2^32.  A row offset computed in 32 bits passes
every other test of the suite (largest single table there: 1.5 GB) and corrupts the first graph of more than 4.2 M nodes.

  fixture A: N = 2^23 + 2^18 (MinHash 4.43 GB, HLL 2.21 GB per hop), fixture B: N = 2^24 + 2^18 (8.72 GB / 4.36 GB per hop).

References: tests/large_table_restatement.py (one hop in blocked stock torch operators, pinned on the C oracle by
tests/test_large_table_restatement_host.py) for whole tables; the C oracle on a COMPACTED table (the distinct rows a query touches,
gathered to the host and renumbered) for queries.  Supported limits these tests establish: DESIGN.md section 4.

update_hash_tables, mask_target, score_links, topk_links, rank_links and PPR at these sizes: tests/test_large_tables_links_gpu.py.

Measured peaks (`torch.cuda.max_memory_allocated()`, profiles/large_tables_tests.txt) set the fixtures' free-memory requirements."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import oracle_params
import large_table_restatement as R
from large_table_helpers import ATOL, GB, LIVE as _LIVE, NEEDS_ONE_TABLE, Big as _Big, boundary_links as _boundary_links, \
    compacted_oracle as _compacted_oracle, feature_tol as _feature_tol, release_all as _release_all, require_free_memory as _require_free_memory

pytestmark = pytest.mark.gpu

RTOL = 1e-5
LC_RTOL = 3e-7
SHAPES = {'A': ((1 << 23) + (1 << 18), [1 << 22, 1 << 23]), 'B': ((1 << 24) + (1 << 18), [1 << 22, 1 << 23, 1 << 24])}
# free device memory a fixture asks for: the measured peak of its tests + 10 % (profiles/large_tables_tests.txt)
NEEDS = {'A': int(1.1 * 52526602240), 'B': int(1.1 * 83686005760), 'spmm': NEEDS_ONE_TABLE}
LOW_HUB_THRESHOLD = 16   # below the ~40 in-edges of a window row, far above the background's (Poisson, mean 2)


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, **kw):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True), **kw)
    eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    return eh


def _make(ssa, dev, name):
    _release_all(dev)
    n, bounds = SHAPES[name]
    _require_free_memory(dev, NEEDS[name], f'fixture {name}')
    torch.cuda.reset_peak_memory_stats(dev)
    big = _Big()
    big.name, big.n, big.bounds = name, n, bounds
    big.graph = R.boundary_graph(n, bounds, dev, seed=20 + len(bounds))
    big.blocks = R.EdgeBlocks(big.graph.edge_index, n)
    deg = big.blocks.degree
    for b in bounds:  # the boundary rows, their predecessors and successors carry work (>= 1 edge besides the self loop)
        assert int(deg[b - 1:b + 2].min()) >= 2, f'boundary row {b} of fixture {name} has no edge'
    assert int(deg[n - 8:n - 1].max()) == 1 and int(deg[n - 1]) == 2, 'the last 7 nodes but one are isolated, N - 1 is a neighbour'
    thr = ssa.hashing.default_hub_threshold(big.graph.edge_index.size(1))   # the adaptive threshold of this build
    assert all(int(deg[h]) > thr for h in big.graph.hubs) and int(deg[big.graph.mega]) > ssa._native.MEGA_SLICE
    assert min(big.graph.hubs) > max(bounds)
    big.eh = _eh(ssa)
    big.table, big.cards = big.eh.build_hash_tables(n, big.graph.edge_index)
    big.prm = oracle_params(big.eh.hll_tables)
    _LIVE.append(big)
    return big


@pytest.fixture(scope='module')
def big_a(ssa, dev):
    big = _make(ssa, dev, 'A')
    yield big
    big.release()


@pytest.fixture(scope='module')
def big_b(ssa, dev):
    big = _make(ssa, dev, 'B')   # (releases fixture A first)
    yield big
    big.release()


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
def _assert_tables(table, big, what):
    """hops 0-2 of `table`, every row: hop 0 on the oracle's windows, hop k from hop k - 1 by the restatement"""
    from oracle import oracle
    assert table[1].mh_u32.shape == (big.n, 128) and table[1].hll_u8.shape == (big.n, 256)
    bad0 = R.hop0_mismatches(oracle, table[0].mh_u32, table[0].hll_u8, big.n, big.bounds, 8)
    assert not bad0, R.report(bad0, big.bounds, f'{what}: hop 0')
    for k in (1, 2):
        bad_mh, bad_hll = R.hop_mismatches(big.blocks, table[k - 1].mh_u32, table[k - 1].hll_u8, table[k].mh_u32, table[k].hll_u8)
        assert not len(bad_mh), R.report(bad_mh, big.bounds, f'{what}: MinHash hop {k}')
        assert not len(bad_hll), R.report(bad_hll, big.bounds, f'{what}: HLL hop {k}')


def _build_variant(ssa, big, variant, monkeypatch):
    if variant == 'default':
        return big.table, big.cards
    if variant == 'three_call':  # ss_first_hop, ss_propagate (MinHash table hop, hll_propagate_row16): no fused stage, nothing deferred
        monkeypatch.setattr(ssa.knobs, 'DEFER_FIRST_HOP', False)
        monkeypatch.setattr(ssa.knobs, 'DEFER_TABLE_HOP', False)
        return _eh(ssa, fuse_hop_stage=False, defer_first_hop=False, defer_table_hop=False).build_hash_tables(big.n, big.graph.edge_index)
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', LOW_HUB_THRESHOLD)
    csr = ssa.build_csr(big.graph.edge_index, big.n, big.graph.edge_index.device)
    hubs = csr.hub_rows[:int(csr.hub_count.item())].long()
    for b in big.bounds:  # the boundary rows themselves are on the cooperative path now
        assert bool((hubs == b).any()) and bool((hubs == b - 1).any()) and bool((hubs == b + 1).any())
    del csr
    return _eh(ssa).build_hash_tables(big.n, big.graph.edge_index)


def _check_build(ssa, big, variant, monkeypatch):
    table, cards = _build_variant(ssa, big, variant, monkeypatch)
    _assert_tables(table, big, f'fixture {big.name}, {variant}')
    if variant != 'default':  # (the default build's cards: test 3)
        assert torch.equal(cards, big.cards)


# ---------------------------------------------------------------------------------------------------
# fixture A
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['default', 'three_call', 'low_hub_threshold'])
def test_build_every_row_of_every_hop_a(ssa, big_a, variant, monkeypatch):
    """(1) build_hash_tables against the restatement, bit-exact, all N rows, hops 0-2: the shipped schedule (fused stage), the
    three-call sequence, and a hub threshold so low that the boundary-window rows take the cooperative path"""
    _check_build(ssa, big_a, variant, monkeypatch)


def _check_cards(big, dev):
    from oracle import oracle
    for k in (0, 1):
        assert torch.equal(big.cards[:, k], big.eh.hll_count(big.table[k + 1].hll_u8.view(torch.int8))), f'cards hop {k + 1}'
        for lo, hi in R.windows(big.n, big.bounds):
            want, branch = oracle.hll_count(big.table[k + 1].hll_u8[lo:hi].cpu().numpy(), big.prm, return_branch=True)
            got = big.cards[lo:hi, k].cpu().numpy()
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=f'hop {k + 1}, rows [{lo}, {hi})')
            lc = branch == 0
            np.testing.assert_allclose(got[lc], want[lc], rtol=LC_RTOL, atol=0, err_msg=f'linear counting, hop {k + 1}, rows [{lo}, {hi})')


def test_cardinalities_a(big_a, dev):
    """(3) cards[:, k] == hll_count of the returned registers on every row; == the oracle on the 4 096-row windows"""
    _check_cards(big_a, dev)


def _check_pair_query(ssa, big, dev, monkeypatch):
    eh = big.eh
    small = _boundary_links(big, dev, 2048, seed=1)
    large = _boundary_links(big, dev, 65536 + 4099, seed=2)
    for links in (small, large):
        ofeat, odbg = _compacted_oracle(big, links, debug=True)
        feats, dbg = eh._pair_kernel(links, big.table, big.cards, want_debug=True)
        assert np.array_equal(dbg['match'].cpu().numpy(), odbg['match']), 'MinHash match counts'
        assert np.array_equal(dbg['zeros'].cpu().numpy(), odbg['zeros']), 'HLL zero counts'
        np.testing.assert_allclose(feats.cpu().numpy(), ofeat, **_feature_tol(ofeat))
        as_listed = eh.get_subgraph_features(links, big.table, big.cards)           # (below GROUP_LINKS_MIN: ss_pair_features)
        assert torch.equal(as_listed, feats)
        monkeypatch.setattr(ssa.knobs, 'GROUP_LINKS_MIN', 1)                       # the grouped kernel walking an order
        monkeypatch.setattr(ssa.knobs, 'GROUP_GATHER_MIN', 1 << 40)
        eh.group_links = True
        try:
            assert torch.equal(eh.get_subgraph_features(links, big.table, big.cards), feats), 'grouped kernel'
            monkeypatch.setattr(ssa.knobs, 'GROUP_GATHER_MIN', 0)                  # gather / grouped query / scatter
            assert torch.equal(eh.get_subgraph_features(links, big.table, big.cards, batch_size=30011), feats), 'gather / scatter form'
        finally:
            eh.group_links = 'auto'
        monkeypatch.undo()
    # the two register budgets of the as-listed kernel agree on the same links
    assert torch.equal(eh.get_subgraph_features(large[:2048], big.table, big.cards), eh.get_subgraph_features(large, big.table, big.cards)[:2048])


def test_pair_query_above_the_boundaries_a(ssa, big_a, dev, monkeypatch):
    """(4) the as-listed kernel at B = 2 048 and above 65 536 (its two register budgets), the grouped kernel and the gather /
    scatter form: bit-identical to each other; match and zero counts bit-exact and features within tolerance against the oracle on
    the compacted table.  `GROUP_LINKS_MIN = 0` DISABLES grouping in this engine (knobs.py), so the grouped forms are forced with
    the lowest thresholds that enable them (GROUP_LINKS_MIN = 1, GROUP_GATHER_MIN = 0) and group_links = True"""
    _check_pair_query(ssa, big_a, dev, monkeypatch)


def test_elph_call_sequence_a(ssa, big_a, dev):
    """(2) initialise_*, hll_prop / minhash_prop / hll_count per hop as ELPH.forward calls them (explicit self loops), then ONE batch
    through the deferred table hop (ss_minhash_hop_rows) with links in the boundary windows and the hub region: the rows served
    equal the full table's rows (features bit-identical to the fixture's), and so does the table once it is completed"""
    H = ssa.hashing
    big = big_a
    n = big.n
    src, dst = R.self_looped_edges(big.graph.edge_index)
    hash_edge_index = torch.stack([src, dst])
    del src, dst
    eh = _eh(ssa)
    mh, hll = eh.initialise_minhash(n), eh.initialise_hll(n)
    cards = torch.zeros((n, 2))
    table = {0: {'minhash': mh, 'hll': hll}}
    for k in (1, 2):
        hll = eh.hll_prop(hll, hash_edge_index)
        mh = eh.minhash_prop(mh, hash_edge_index)
        cards[:, k - 1] = eh.hll_count(hll)
        table[k] = {'minhash': mh, 'hll': hll}
        assert torch.equal(H._packed_hll_of(hll, dev), big.table[k].hll_u8), f'hll_prop hop {k}'
    del table[0]
    assert torch.equal(cards.to(dev), big.cards)
    last = table[2]['minhash']
    assert isinstance(last, H.LazyMinhash) and last._pending is not None, 'the last table hop is owed'
    links = _boundary_links(big, dev, 2048, seed=3)
    feats = eh.get_subgraph_features(links, table, cards)
    assert last._pending is not None and last._partial_rows == links.numel(), 'served through ss_minhash_hop_rows, table still owed'
    assert torch.equal(feats, big.eh.get_subgraph_features(links, big.table, big.cards))
    assert torch.equal(H._packed_minhash_of(table[1]['minhash'], dev), big.table[1].mh_u32), 'hop-1 MinHash (deferred first hop)'
    assert torch.equal(H._packed_minhash_of(last, dev), big.table[2].mh_u32), 'the whole hop-2 table, once someone asks for it'


def test_query_whose_own_arrays_cross_4_gib_a(ssa, big_a, dev):
    """(5) B = 2^26 + 12 345 links with degrees= (64-byte rows: 4.29 GB of rows, 1.07 GB of links), every source repeated (the BUDDY
    pattern), default knobs: ss_group_links_by_source, ss_gather_links, the grouped kernel and ss_scatter_feature_rows as shipped.
    torch.equal, slice by slice, to the same call in chunks of 4 999 999 links with grouping off; the last 3 000 rows and 3 000
    rows around output bytes 2^31 and 2^32 also against the compacted oracle"""
    big = big_a
    n, eh = big.n, big.eh
    B = (1 << 26) + 12345
    assert B >= ssa.knobs.GROUP_GATHER_MIN >= ssa.knobs.GROUP_LINKS_MIN > 0 and eh.group_links == 'auto'
    gen = torch.Generator(device=dev).manual_seed(55)
    top = max(big.bounds)
    pool = torch.cat([torch.randint(0, n, (1 << 19,), device=dev, generator=gen),
                      torch.arange(top - 512, top + 512, device=dev), torch.tensor([n - 1, big.graph.mega, 1 << 22], device=dev)])
    links = torch.stack([pool[torch.randint(0, pool.numel(), (B,), device=dev, generator=gen)],
                         torch.randint(0, n, (B,), device=dev, generator=gen)], 1)
    links[-1] = torch.tensor([n - 1, top], device=dev)
    links[::11] -= n
    degrees = big.blocks.degree.to(torch.float32)
    degrees[:1000:7] = 0          # (division by zero -> 0 in the normalised copy)
    got = eh.get_subgraph_features(links, big.table, big.cards, degrees=degrees)
    assert got.shape == (B, 16) and got.numel() * 4 > (1 << 32) and links.numel() * 8 > (1 << 30)
    eh.group_links = False
    try:
        step = 4999999
        for s in range(0, B, step):
            want = eh._pair_kernel(links[s:s + step], big.table, big.cards, degrees=degrees)[0]
            assert torch.equal(got[s:s + step], want), f'links [{s}, {s + step}): output bytes [{64 * s}, {64 * (s + step)})'
            del want
    finally:
        eh.group_links = 'auto'
    for lo in (B - 3000, (1 << 31) // 64 - 1500, (1 << 32) // 64 - 1500):
        ofeat, _ = _compacted_oracle(big, links[lo:lo + 3000], degrees=degrees)
        np.testing.assert_allclose(got[lo:lo + 3000].cpu().numpy(), ofeat, err_msg=f'rows from {lo}', **_feature_tol(ofeat))


def test_one_vs_all_scan_a(ssa, big_a, dev):
    """(6) topk_candidates for sources below and above the boundary, with an exclude list, against the brute-force composition
    (_get_intersections over (s, v) for ALL v, in chunks): ids exact, scores bit for bit, and every source has a candidate above 2^23
    -- checked on the brute-force result first"""
    big = big_a
    n, eh, k = big.n, big.eh, 50
    b = 1 << 23
    sources = [b - 3, b, b + 700, -(n - (1 << 22))]        # inside the dense windows; the last one is row 2^22 as a negative id
    ex_src = torch.tensor([b - 3] * 4 + [b], device=dev)
    ei = big.graph.edge_index
    first_nb = ei[0][ei[1] == b - 3][:4]
    exclude = torch.stack([ex_src, torch.cat([first_nb, torch.tensor([b + 1], device=dev)])])
    ids, scores = eh.topk_candidates(torch.tensor(sources, device=dev), big.table, k, hops=(1, 1), exclude=exclude)
    ex = exclude.cpu().numpy()
    step = 4000000
    for r, u in enumerate(sources):
        u = u + n if u < 0 else u
        sc = np.empty(n, dtype=np.float32)
        for s in range(0, n, step):
            v = torch.arange(s, min(s + step, n), device=dev)
            sc[s:s + step] = eh._get_intersections(torch.stack([torch.full_like(v, u), v], 1), big.table)[(1, 1)].cpu().numpy()
        elig = np.ones(n, dtype=bool)
        elig[u] = False
        elig[ex[1][ex[0] == u]] = False
        cand = np.nonzero(elig)[0]
        order = np.lexsort((cand, -sc[cand]))[:k]
        want_ids, want_sc = cand[order], sc[cand[order]]
        if u >= (1 << 22) + big.graph.window:
            assert (want_ids > b).any(), f'source {u}: the reference itself must rank a candidate above 2^23'
        np.testing.assert_array_equal(ids[r].cpu().numpy(), want_ids, err_msg=f'source {u}')
        bits = lambda a: np.where(a == 0, np.float32(0), a).view(np.int32)
        np.testing.assert_array_equal(bits(scores[r].cpu().numpy()), bits(want_sc), err_msg=f'source {u}')
    assert not np.isin(ids[0].cpu().numpy(), first_nb.cpu().numpy()).any()


def test_digest_a(ssa, big_a, dev):
    """(7) ss_table_digest of the 4.43 GB hop-2 MinHash table against the numpy restatement of the same sum / xor, fed 64 MB at a
    time; it changes when one byte in the last row is flipped and comes back when the byte is restored"""
    t = big_a.table[2].mh_u32
    nbytes = t.numel() * 4
    assert nbytes > (1 << 32)

    def mix(x):
        K = np.uint64(0xD6E8FEB86659FD93)
        x = x ^ (x >> np.uint64(32)); x = x * K
        x = x ^ (x >> np.uint64(32)); x = x * K
        return x ^ (x >> np.uint64(32))

    flat = t.view(-1)
    total, xor = np.uint64(0), np.uint64(0)
    step = (64 << 20) // 4
    with np.errstate(over='ignore'):
        for s in range(0, flat.numel(), step):
            w = flat[s:s + step].cpu().numpy().view(np.uint64).reshape(-1, 2)
            i = np.arange(s // 4, s // 4 + len(w), dtype=np.uint64)
            h = mix(w[:, 0] ^ (i * np.uint64(0x9E3779B97F4A7C15))) + mix(w[:, 1] + i)
            total = total + h.sum(dtype=np.uint64)
            xor = xor ^ np.bitwise_xor.reduce(h)
    got = ssa.dist.table_digests([t])[0].cpu().numpy().view(np.uint64)
    assert (int(got[0]), int(got[1])) == (int(total), int(xor))
    last = t[-1].view(torch.uint8)
    last[509] ^= 4
    flipped = ssa.dist.table_digests([t])[0].cpu().numpy().view(np.uint64)
    last[509] ^= 4
    assert (int(flipped[0]), int(flipped[1])) != (int(total), int(xor))
    assert np.array_equal(ssa.dist.table_digests([t])[0].cpu().numpy().view(np.uint64), got)


def test_mirrored_row_stores_straddle_row_2_23_a(ssa, big_a, dev):
    """(8) the row-range / mirror form through the C ABI, one mirror, row range straddling 2^23: the mirror equals the primary on
    every row of the range and is untouched outside it (first hop from ids, table hops, cardinalities)"""
    H = ssa.hashing
    big = big_a
    n, h, eh = big.n, 2, big.eh
    csr = H.build_csr(big.graph.edge_index, n, dev, check=False)
    csr.use_inferred_self_loops = True
    params = eh._params(dev)
    lo, hi = (1 << 23) - 3000, (1 << 23) + 5000
    blank = lambda shape, dtype: [torch.full(shape, 7, dtype=dtype, device=dev) for _ in range(2)]
    none = [0]
    ptrs = lambda ts: [ts[1].data_ptr()]

    def check(pair, want, what):
        for j, t in enumerate(pair):
            assert torch.equal(t[lo:hi], want[lo:hi]), (what, 'primary' if j == 0 else 'mirror')
            assert bool((t[:lo] == 7).all()) and bool((t[hi:] == 7).all()), (what, j, 'rows outside the range')

    cd = blank((n, h), torch.float32)
    mh = blank((n, 128), torch.int32)
    eh._first_hop(csr, dev, mh[0], None, None, params, rows=(lo, hi), mirrors=(ptrs(mh), none, none))
    check(mh, big.table[1].mh_u32, 'MinHash hop 1')
    H._propagate(csr, big.table[1].mh_u32, None, dev, mh_out=mh[0], rows=(lo, hi), mirrors=(ptrs(mh), none, none))
    check(mh, big.table[2].mh_u32, 'MinHash hop 2')
    del mh
    hl = blank((n, 256), torch.uint8)
    eh._first_hop(csr, dev, None, hl[0], cd[0], params, rows=(lo, hi), mirrors=(none, ptrs(hl), ptrs(cd)))
    check(hl, big.table[1].hll_u8, 'HLL hop 1')
    H._propagate(csr, None, big.table[1].hll_u8, dev, cards_out=cd[0][:, 1], cards_stride=h, params=params, hll_out=hl[0], rows=(lo, hi),
                 mirrors=(none, ptrs(hl), [cd[1].data_ptr() + 4]))
    check(hl, big.table[2].hll_u8, 'HLL hop 2')
    check(cd, big.cards, 'cards')


# ---------------------------------------------------------------------------------------------------
# fixture B (fixture A is released when it is built)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['default', 'three_call', 'low_hub_threshold'])
def test_build_every_row_of_every_hop_b(ssa, big_b, variant, monkeypatch):
    """(1) on fixture B: the MinHash element index crosses 2^31 and the HLL byte offset 2^32 at row 2^24"""
    _check_build(ssa, big_b, variant, monkeypatch)


def test_cardinalities_b(big_b, dev):
    _check_cards(big_b, dev)


def test_pair_query_above_the_boundaries_b(ssa, big_b, dev, monkeypatch):
    _check_pair_query(ssa, big_b, dev, monkeypatch)


# ---------------------------------------------------------------------------------------------------
# wide node tables that are not sketches (both fixtures released first)
# ---------------------------------------------------------------------------------------------------
def test_spmm_operand_above_4_gib(ssa, dev):
    """(9) ss_spmm_csr with F = 128 fp32 at fixture A's N (4.43 GB operand and result) against the oracle's edge-order fp32
    scatter-add on the rows of the boundary windows, their sources gathered and compacted; bit-exact"""
    from oracle import oracle
    from subgraph_sketching_amd import sign
    _release_all(dev)
    n, bounds = SHAPES['A']
    _require_free_memory(dev, NEEDS['spmm'], 'the spmm operand and result')
    torch.cuda.reset_peak_memory_stats(dev)
    g = R.boundary_graph(n, bounds, dev, seed=31)
    ei = g.edge_index
    gen = torch.Generator(device=dev).manual_seed(32)
    val = torch.rand(ei.size(1), device=dev, generator=gen)
    x = torch.randn((n, 128), device=dev, generator=gen)
    got = sign.spmm(ei, val, n, n, x)
    assert got.shape == (n, 128) and got.numel() * 4 > (1 << 32)
    for lo, hi in R.windows(n, bounds):
        sel = ((ei[0] >= lo) & (ei[0] < hi)).nonzero().flatten()        # edge order kept: the sum order of the reference
        rows, cols = ei[0][sel] - lo, ei[1][sel]
        uniq, inv = torch.unique(cols, return_inverse=True)
        want = oracle.spmm(np.stack([rows.cpu().numpy(), inv.cpu().numpy()]), val[sel].cpu().numpy(), hi - lo,
                           x.index_select(0, uniq).cpu().numpy())
        assert np.array_equal(got[lo:hi].cpu().numpy(), want), f'rows [{lo}, {hi})'
    peak = torch.cuda.max_memory_allocated(dev)
    print(f'\n[large tables] spmm: peak torch.cuda.max_memory_allocated() = {peak} bytes ({peak / GB:.2f} GiB)')
