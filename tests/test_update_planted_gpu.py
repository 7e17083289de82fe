"""The marking kernels of update_hash_tables alone, through the C ABI (ss_update_mark: update_seed_kernel, update_mark_kernel<true> and
<false>, csrc/ss_update.hip), on the planted graph of tests/update_planted.py: one target row per in-degree at each end of the
marker's three tiers and around every step boundary of the cooperative ones.  Expected maps: the numpy restatement
(tests/update_restatement.py), or its closed form for a single seed that tests/test_update_host.py pins on the restatement.  Everything
is exact: byte maps equal, lists equal as sets with the front / end partition, counters equal to the lengths."""
from ctypes import byref

import numpy as np
import pytest
import torch

import update_planted as up
import update_restatement as ur

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


class Marker(object):
    """the planted graph's CSR on the device + one workspace per hop count; mark() is one ss_update_mark call, nothing synchronises"""

    def __init__(self, ssa, dev):
        self.ssa, self.dev, self.pl = ssa, dev, up.plan()
        pl = self.pl
        self.n = pl['n']
        self.csr = ssa.hashing.build_csr(torch.from_numpy(pl['edge_index']).to(dev), self.n, dev, check=False)
        self.csr.use_inferred_self_loops = True
        self.lib = ssa._native.lib()
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = {}
        for h in (1, 2, 3):
            nbytes = int(self.lib.ss_update_workspace_bytes(self.n, h))
            assert nbytes == 256 + 5 * h * ((self.n + 255) & ~255)
            self.ws[h] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.cards = torch.from_numpy(up.had_loop_cards(self.n, pl['n_self'])).to(dev)
        self.deg = torch.from_numpy(pl['deg']).to(dev)

    def mark(self, h, added=None, removed=None, cards=None, hub_threshold=None):
        """-> (counters, maps, lists): views of the workspace of hop count h (carve_workspace)"""
        from subgraph_sketching_amd._runtime import _ptr, _stream
        from subgraph_sketching_amd.update import carve_workspace
        graph = self.csr.struct()
        if hub_threshold is not None:
            graph.hub_threshold = hub_threshold
        cards = self.cards if cards is None else cards
        assert cards.dtype == torch.float32 and cards.stride(1) == 1 and cards.size(0) == self.n
        for t in (added, removed):
            assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.device.type == 'cuda')
        ws = self.ws[h]
        rc = self.lib.ss_update_mark(byref(graph), _ptr(added), 0 if added is None else added.numel(), _ptr(removed),
                                     0 if removed is None else removed.numel(), _ptr(cards), cards.stride(0), h, _ptr(self.err), _ptr(ws),
                                     ws.numel(), _stream(self.dev))
        assert rc == 0, rc
        return carve_workspace(ws, self.n, h)


@pytest.fixture(scope='module')
def marker(ssa, dev):
    return Marker(ssa, dev)


def _assert_lists(counters, maps, lists, dirty, deg, n, threshold, what):
    """maps == dirty exactly; per hop: the list's front holds the dirty rows with deg <= threshold, its end (from n - 1 downwards) those
    above, each once; ascending inside each 256-row block, the rows of a block adjacent; counters == lengths"""
    words = counters.cpu().numpy()
    h = len(maps)
    assert words[0] == int(dirty[1].sum()), (what, 'seed rows')
    for k in range(1, h + 1):
        got = maps[k - 1].cpu().numpy()
        assert set(np.unique(got).tolist()) <= {0, 1}, (what, k, 'a map byte is neither 0 nor 1')
        wrong = np.flatnonzero((got != 0) != dirty[k])
        assert wrong.size == 0, (what, f'hop {k}: map differs at rows {wrong[:8]} (in-degrees {deg[wrong[:8]]})')
        n_dirty, n_rows, n_hubs = (int(w) for w in words[4 * k:4 * k + 3])
        want_hub = dirty[k] & (deg > threshold)
        want_reg = dirty[k] & ~want_hub
        assert (n_dirty, n_rows, n_hubs) == (int(dirty[k].sum()), int(want_reg.sum()), int(want_hub.sum())), (what, k, 'counters')
        lst = lists[k - 1].cpu().numpy()
        rows, hubs = lst[:n_rows], lst[n - n_hubs:n][::-1]
        for part, want in ((rows, want_reg), (hubs, want_hub)):
            assert np.array_equal(np.sort(part), np.flatnonzero(want)), (what, k, 'a list is not its set, each row once')
            same_block = part[1:] // 256 == part[:-1] // 256
            assert (part[1:] > part[:-1])[same_block].all(), (what, k, 'not ascending inside a 256-row block')
            assert int((~same_block).sum()) + (part.size > 0) == np.unique(part // 256).size, (what, k, 'a block is listed in two pieces')


def _expected(pl, cards, added, removed, h):
    as_edges = lambda t: None if t is None else np.stack([np.zeros(len(t), dtype=np.int64), np.asarray(t, dtype=np.int64)])
    dirty = ur.dirty_sets(pl['n'], pl['edge_index'], cards, as_edges(added), as_edges(removed), h)
    assert dirty[h].sum() < pl['n']
    return dirty


def test_builder_left_every_planted_row_whole(marker):
    """the CSR the marker walks: n_self is the largest endpoint + 1, and row r_d holds each of the sources 0 .. d - 1 once -- so the loop
    over all sources below puts the one dirty in-neighbour at EVERY slot of every row, first and last slot of each tier included"""
    pl, csr = marker.pl, marker.csr
    assert int(csr.n_self_dev.item()) == pl['n_self']
    rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()
    assert np.array_equal(np.diff(rowptr), pl['deg'])
    seen = set()
    for d, r in pl['rows'].items():
        row = col[rowptr[r]:rowptr[r + 1]]
        assert np.array_equal(np.sort(row), np.arange(d)), f'row of in-degree {d}'
        if d:
            assert 0 <= row[0] < up.D and 0 <= row[-1] < up.D  # the sources at the first and the last slot are among the seeds of the loop
        seen.add(up.tier(d))
    assert seen == {'solo', 'wave', 'workgroup'}


def test_every_source_in_turn_as_the_only_target(marker, dev):
    """h = 2, 5 200 calls: dirty_1 = {s}, dirty_2 = {s} + {r_d : d > s}.  The mismatches are summed on the device and read once."""
    n, deg = marker.n, marker.deg
    thr = marker.csr.hub_threshold
    targets = torch.arange(up.D, dtype=torch.int64, device=dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    bad = torch.zeros(3, dtype=torch.int64, device=dev)  # wrong bytes of map 1, of map 2, wrong counters
    missed = torch.zeros(n, dtype=torch.int32, device=dev)  # per row: calls in which its hop-2 byte was wrong
    # seed rows | hop 1: dirty, listed rows, listed hubs | hop 2: the same (s is a regular row; r_d is a hub iff d > the CSR's threshold)
    word_ids = torch.tensor([0, 4, 5, 6, 8, 9, 10], device=dev)
    longer = np.array([[sum(d > s and d <= thr for d in up.DEGREES), sum(d > s and d > thr for d in up.DEGREES)] for s in range(up.D)])
    want_words = np.stack([np.ones(up.D), np.ones(up.D), np.ones(up.D), np.zeros(up.D), 1 + longer.sum(axis=1), 1 + longer[:, 0], longer[:, 1]], axis=1)
    want_words = torch.from_numpy(want_words.astype(np.int32)).to(dev)
    for s in range(up.D):
        counters, maps, lists = marker.mark(2, added=targets[s:s + 1])
        one = ids == s
        wrong2 = (maps[1] != 0) != (one | (deg > s))
        bad[0] += ((maps[0] != 0) != one).sum()
        bad[1] += wrong2.sum()
        missed += wrong2
        bad[2] += (counters[word_ids] != want_words[s]).sum()
    bad, missed = bad.cpu().tolist(), missed.cpu().numpy()
    rows = np.flatnonzero(missed)
    assert bad[:3] == [0, 0, 0], (f'over {up.D} single-seed calls: wrong bytes of map 1: {bad[0]}, of map 2: {bad[1]}, wrong counters: {bad[2]}; '
                                   f'rows wrong at hop 2: {rows[:8]} with in-degrees {marker.pl["deg"][rows[:8]]}')
    assert int(marker.err.item()) == 0


@pytest.mark.parametrize('h', [3])
@pytest.mark.parametrize('case', ['two', 'seventeen', 'four-hundred', 'high-sources-only', 'rows-already-seeds'])
def test_random_subsets_as_targets(marker, dev, case, h):
    pl = marker.pl
    rng = np.random.RandomState(67)
    rows = np.array(sorted(pl['rows'].values()))
    if case == 'two':
        removed, added = None, rng.choice(up.D, size=2, replace=False)
    elif case == 'seventeen':
        added, removed = rng.choice(up.D, size=9, replace=False), rng.choice(up.D, size=8, replace=False)
    elif case == 'four-hundred':
        added, removed = rng.randint(0, up.D, size=250), rng.randint(0, up.D, size=150)  # (duplicates as they fall)
    elif case == 'high-sources-only':
        # no in-neighbour of any row below in-degree 4 097 is hit: those rows stay clean, r_4097 is hit at one slot, r_5121 at all 17
        added, removed = np.arange(4096, 4096 + 17), None
    else:
        # rows that are seeds themselves skip their walk (source 40 is a dirty in-neighbour of the longer ones as well)
        added, removed = np.concatenate([rows[::2], [40]]), rows[1::2][:5]
    dirty = _expected(pl, marker.cards.cpu().numpy(), added, removed, h)
    if case == 'high-sources-only':
        assert not dirty[h][rows[pl['deg'][rows] <= 4096]].any() and dirty[2][pl['rows'][4097]] and dirty[2][pl['rows'][5121]]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    counters, maps, lists = marker.mark(h, added=t(added), removed=t(removed))
    _assert_lists(counters, maps, lists, dirty, pl['deg'], marker.n, marker.csr.hub_threshold, case)
    assert int(marker.err.item()) == 0


@pytest.mark.parametrize('threshold', [8, 2048, 10 ** 9])
def test_hub_threshold_splits_each_list(marker, dev, threshold):
    """graph.hub_threshold decides which end of a hop's list a dirty row goes to, and nothing else"""
    pl = marker.pl
    rng = np.random.RandomState(68)
    added = np.concatenate([rng.choice(up.D, size=300, replace=False), [pl['rows'][33], pl['rows'][2049], pl['rows'][5121]]])
    dirty = _expected(pl, marker.cards.cpu().numpy(), added, None, 3)
    hubs = dirty[3] & (pl['deg'] > threshold)
    assert (hubs.sum() == 0) == (threshold == 10 ** 9) and (dirty[3] & ~hubs).sum() > 256
    counters, maps, lists = marker.mark(3, added=torch.from_numpy(added).to(dev), hub_threshold=threshold)
    _assert_lists(counters, maps, lists, dirty, pl['deg'], marker.n, threshold, f'threshold {threshold}')


@pytest.mark.parametrize('h,stride', [(1, 1), (2, 2), (3, 3), (2, 5), (3, 7)])
def test_self_loop_seeds_planted_through_cards_old(marker, dev, h, stride):
    """a row below n_self whose old hop-1 cardinality is 0 gained its loop, a row from n_self on with a positive one lost it: seeds
    without any target.  Column 0 of cards_old decides alone (the other columns say the opposite); a trailing row is dirty only as a
    seed -- the hop-k rule `i < n_self && prev[i]` and the in-edge walk have nothing to say about it"""
    pl = marker.pl
    n, n_self = marker.n, pl['n_self']
    cards = up.had_loop_cards(n, n_self, stride)
    gained = [3, 4097, up.D - 1, pl['rows'][0], pl['rows'][64], n_self - 1]
    lost = [n_self, n_self + 1, n_self + 255, n - 1]
    cards[gained, 0] = 0.0
    cards[lost, 0] = np.float32(1e-30)  # (positive, however small)
    dirty = _expected(pl, cards, None, None, h)
    assert np.flatnonzero(dirty[1]).tolist() == sorted(gained + lost)
    for k in range(1, h + 1):
        assert (n_self + np.flatnonzero(dirty[k][n_self:])).tolist() == lost
    counters, maps, lists = marker.mark(h, cards=torch.from_numpy(cards).to(dev))
    _assert_lists(counters, maps, lists, dirty, pl['deg'], n, marker.csr.hub_threshold, f'h {h} stride {stride}')
    # ... and together with a target
    t = torch.tensor([17], dtype=torch.int64, device=dev)
    dirty = _expected(pl, cards, None, [17], h)
    counters, maps, lists = marker.mark(h, removed=t, cards=torch.from_numpy(cards).to(dev))
    _assert_lists(counters, maps, lists, dirty, pl['deg'], n, marker.csr.hub_threshold, f'h {h} stride {stride} + target')


def test_seed_kernel_beyond_its_grid_and_with_bad_ids(marker, dev, ssa):
    """update_seed_kernel: 1 200 000 targets (its grid is capped at 4 096 x 256 threads, so the stride loop runs) with duplicates;
    then ids outside [0, N) among good ones: the error word is set, the good targets are still marked, nothing else is"""
    pl, n = marker.pl, marker.n
    rng = np.random.RandomState(69)
    pool = rng.choice(n, size=4000, replace=False)          # every kind of row, trailing ones too
    targets = pool[rng.randint(0, pool.size - 64, size=1200000)]
    targets[1048576:1048576 + 64] = pool[-64:]               # rows that only the second trip of the stride loop names
    late_only = np.setdiff1d(pool[-64:], np.concatenate([targets[:1048576], targets[1048576 + 64:]]))
    assert late_only.size == 64 and np.unique(targets).size < targets.size
    dirty = _expected(pl, marker.cards.cpu().numpy(), targets[:700000], targets[700000:], 1)
    counters, maps, lists = marker.mark(1, added=torch.from_numpy(targets[:700000]).to(dev), removed=torch.from_numpy(targets[700000:]).to(dev))
    _assert_lists(counters, maps, lists, dirty, pl['deg'], n, marker.csr.hub_threshold, '1.2 M targets')
    assert int(marker.err.item()) == 0
    print(f'distinct targets {int(dirty[1].sum())}, named only past the first grid trip: {late_only.size}')

    good = np.array([5, pl['rows'][5121], n - 1, 0], dtype=np.int64)
    added = np.array([good[0], -1, good[1], n], dtype=np.int64)
    removed = np.array([n + 12345, good[2], -(1 << 40), good[3], 1 << 33], dtype=np.int64)
    dirty = _expected(pl, marker.cards.cpu().numpy(), good, None, 2)
    try:
        counters, maps, lists = marker.mark(2, added=torch.from_numpy(added).to(dev), removed=torch.from_numpy(removed).to(dev))
        _assert_lists(counters, maps, lists, dirty, pl['deg'], n, marker.csr.hub_threshold, 'bad ids among good ones')
        assert int(marker.err.item()) == ssa._native.SS_CSR_ERR_BOUNDS
    finally:
        marker.err.zero_()
