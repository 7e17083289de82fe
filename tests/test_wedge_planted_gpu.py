"""The two-hop kernels (csrc/ss_wedge.hip) on PLANTED graphs (wedge_planted.py: every source's endpoints are known from the plan that
wrote the graph): every LDS table size half full and one over, the tier rule at the largest table from both sides, rows of more than
one 256-neighbour slice in the fold tier, probe chains that run off the end of a table, sinks and long rows inside the emit tier's
scan, every way the emit tier's slices can meet its workgroups, what each launch writes and what it leaves alone, and sources of
2^31 walks and more.  "Equal" is rowptr, ids, common and W(u) exactly; the plan itself is pinned on scipy's A[sources] @ A by
tests/test_wedge_planted_host.py.  What ran on an MI355X: profiles/wedge_planted_tests.txt."""
import numpy as np
import pytest
import torch

from test_wedge_gpu import _bits, _brute_force, _eh, _head
import wedge_planted as planted

pytestmark = pytest.mark.gpu

GRAPHS = ('table_sizes', 'wide_fold', 'collisions', 'emit_shapes', 'walks_46341_squared', 'walks_2_to_31')
SENTINEL = -12345  # no key (keys are >= 0), not kWedgePad; as a count: no count


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
def graphs(ssa, dev):
    """per planted graph a dict(N, ei, src, expect, made, g = its WedgeGraph, ei_dev), built once; every test reads them only"""
    M = ssa._native.WEDGE_MAX_SLOTS
    build = {'table_sizes': lambda: planted.table_sizes(M), 'wide_fold': lambda: planted.wide_fold(M),
             'collisions': lambda: planted.collisions(M), 'emit_shapes': lambda: planted.emit_shapes(M), 'mixed': lambda: planted.mixed(M),
             'walks_46341_squared': lambda: planted.too_many_walks(*planted.GIANTS[0]),
             'walks_2_to_31': lambda: planted.too_many_walks(*planted.GIANTS[1])}
    made = {}

    def get(name):
        if name not in made:
            N, ei, src, expect, names = build[name]()
            ei_dev = torch.from_numpy(ei.copy()).to(dev)  # (the plan's array is read-only)
            made[name] = dict(N=N, ei=ei, src=src, expect=expect, made=names, g=ssa.WedgeGraph(N, ei_dev), ei_dev=ei_dev)
        return made[name]

    return get


def _listed(N, src, expect):
    """the planted sources, then two of them again: the one with the most listed walks as a negative id, the first with work as it is"""
    W = expect['walks']
    again = [int(np.argmax(np.where(W <= planted.MAX_WALKS, W, 0))), int(np.nonzero(W)[0][0])]
    more = {k: list(v) + [v[i] for i in again] for k, v in expect.items()}
    more['walks'] = np.array(more['walks'], dtype=np.int64)
    return np.concatenate([src, [src[again[0]] - N, src[again[1]]]]), more


def _assert_rows(got, want, dev):
    rowptr, ids, common = got[:3]
    assert rowptr.dtype == torch.int64 and ids.dtype == torch.int64 and common.dtype == torch.int32
    assert rowptr.device == dev and ids.device == dev and common.device == dev
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(ids.cpu().numpy(), want[1])
    np.testing.assert_array_equal(common.cpu().numpy(), want[2])


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GRAPHS)
def test_rows_equal_the_plan(ssa, dev, graphs, name):
    p = graphs(name)
    N, ei, g = p['N'], p['ei'], p['g']
    M = ssa._native.WEDGE_MAX_SLOTS
    src, expect = _listed(N, p['src'], p['expect'])
    want = planted.want(N, ei, src, expect)
    assert want[1].size and (expect['walks'] == 0).any(), 'a trivial expectation checks nothing'
    sd = torch.from_numpy(src).to(dev)
    for slots in (None, 64, 1) + ((256, M) if name == 'collisions' else ()):  # (collisions: the table sizes its chains were found for)
        rowptr, ids, common, info = g.candidates(sd, return_info=True, _lds_slots=slots)
        _assert_rows((rowptr, ids, common), want, dev)
        assert info['skipped_sources'] == want[3] == int((expect['walks'] > planted.MAX_WALKS).sum())
        assert info['walks'].dtype == torch.int64 and info['walks'].device == dev
        np.testing.assert_array_equal(info['walks'].cpu().numpy(), expect['walks'])
        assert (info['lds_sources'], info['large_sources']) == planted.tiers(expect['walks'], slots or M)
    if name == 'table_sizes':  # the rule at the largest table, from both sides: the last W that folds, the first that emits
        W = p['expect']['walks']
        assert all(W[p['made'][(w, shape)]] == w for w in (M // 2, M // 2 + 1) for shape in ('hub', 'spokes'))
        assert planted.tiers(W, M)[1] == 2 and planted.folds(M // 2, M) and planted.emits(M // 2 + 1, M)
    two = planted.want(N, ei, src, expect, min_common=2)
    assert 0 < two[1].size < want[1].size
    _assert_rows(g.candidates(sd, min_common=2), two, dev)
    free = planted.want(N, ei, src, expect, exclude_edges=True)
    assert 0 < free[1].size < want[1].size
    _assert_rows(g.candidates(sd, exclude=p['ei_dev']), free, dev)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_slices_against_workgroups(ssa, dev, graphs, monkeypatch):
    """the source of 12 T neighbours has 12 slices; its launch has 1, 3, 5, 12 and the most workgroups per source: one workgroup copies
    every slice, the slice index wraps around the workgroups (3, 5), one each, and workgroups without a slice"""
    p = graphs('emit_shapes')
    N, ei, g = p['N'], p['ei'], p['g']
    src, expect = p['src'], p['expect']
    most = ssa._native.WEDGE_MAX_SLICES
    assert -(-int((ei[0] == p['made']['slices']).sum()) // planted.T) == 12 < most
    want = planted.want(N, ei, src, expect)
    sd = torch.from_numpy(src).to(dev)
    largest = int(expect['walks'].max())  # (one launch: its workgroups per source follow from the largest W(u) among the sources)
    seen = []
    for slices in (1, 3, 5, 12, most):
        per = 1 if slices == most else -(-largest // slices)
        assert min(most, -(-largest // per)) == slices
        monkeypatch.setattr(ssa.wedge, '_WEDGE_SLICE_WALKS', per)
        got = g.candidates(sd, return_info=True)
        emitting = sum(planted.emits(int(expect['walks'][s]), ssa._native.WEDGE_MAX_SLOTS) for s in p['made'].values())
        assert got[3]['large_sources'] == planted.tiers(expect['walks'], ssa._native.WEDGE_MAX_SLOTS)[1] == emitting >= 5
        _assert_rows(got, want, dev)
        seen.append(got[:3])
    assert all(torch.equal(a, b) for other in seen[1:] for a, b in zip(seen[0], other))


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _block(p, N, slots):
    """the sources of one block, the tiers interleaved: [(source id, walks given to the launches, its place in the plan or None)]"""
    made, W = p['made'], p['expect']['walks']
    ts, wf, es = made['table_sizes'], made['wide_fold'], made['emit_shapes']
    M2 = max(w for w, _ in ts) - 1
    R2 = 2 * planted.R  # (a table of 64 slots half full, and one endpoint over)
    assert {(1, 'hub'), (3, 'hub'), (R2, 'hub'), (R2 + 1, 'hub')} <= set(ts), 'the block needs SS_WEDGE_MAX_SLOTS >= 128'
    a = [ts[(w, s)] for w in (1, 2, 3, R2, R2 + 1, M2) for s in ('hub', 'spokes')] + list(wf.values())
    b = [ts[(M2 + 1, 'hub')], ts[(M2 + 1, 'spokes')]] + [es[k] for k in es if k != 'sinks'] + [es[planted.T]]  # (one of them twice)
    order = [x for pair in zip(a, b + [0, es['sinks'], 0] * 8) for x in pair]  # (0 and `sinks`: W = 0)
    block = [(u, int(W[u]), u) for u in order]
    block.insert(5, (N, 0, None))                     # an id out of range: the host gives it no walks
    block.insert(9, (wf['one'], 0, None))             # sources that a cap has zeroed: one of each tier
    block.insert(12, (es['slices'], 0, None))
    block.append((-N - 1, 0, None))
    assert sum(planted.folds(w, slots) for _, w, _ in block) >= 8 and sum(planted.emits(w, slots) for _, w, _ in block) >= 8
    return block


def _guarded(total, dtype, dev, guard=256):
    whole = torch.full((total + 2 * guard,), SENTINEL, dtype=dtype, device=dev)
    return whole, whole[guard:guard + total]


def _untouched(whole, total, places, guard=256):
    """both guards and every place of `places` [(offset, length)] still hold the sentinel"""
    a = whole.cpu().numpy()
    assert (a[:guard] == SENTINEL).all() and (a[guard + total:] == SENTINEL).all() and a.size == total + 2 * guard
    for o, n in places:
        assert (a[guard + o:guard + o + n] == SENTINEL).all(), (o, n)


@pytest.mark.parametrize('slots', [None, 64])
def test_each_launch_writes_its_own_places_only(ssa, dev, graphs, slots):
    p = graphs('mixed')
    N, g = p['N'], p['g']
    slots = slots or ssa._native.WEDGE_MAX_SLOTS
    block = _block(p, N, slots)
    sources = torch.tensor([u for u, _, _ in block], dtype=torch.int64, device=dev)
    take_np = np.array([w for _, w, _ in block], dtype=np.int64)
    offsets_np = np.cumsum(take_np) - take_np
    total = int(take_np.sum())
    take, offsets = torch.from_numpy(take_np).to(dev), torch.from_numpy(offsets_np).to(dev)
    fold_places = [(int(o), w) for (_, w, _), o in zip(block, offsets_np) if planted.folds(w, slots)]
    emit_places = [(int(o), w) for (_, w, _), o in zip(block, offsets_np) if planted.emits(w, slots)]
    assert sum(n for _, n in fold_places) + sum(n for _, n in emit_places) == total

    keys_all, keys = _guarded(total, torch.int64, dev)
    counts_all, counts = _guarded(total, torch.int32, dev)
    ssa.wedge._launch_fold(g, sources, take, offsets, slots, keys, counts)
    torch.cuda.synchronize()
    _untouched(keys_all, total, emit_places)
    _untouched(counts_all, total, emit_places)
    k, c = keys.cpu().numpy(), counts.cpu().numpy()
    for s, ((u, w, at), o) in enumerate(zip(block, offsets_np)):
        if planted.folds(w, slots):
            ends = p['expect']['ends'][at]
            D = len(ends)
            assert sum(ends.values()) == w and 0 < D <= w
            assert set(zip(k[o:o + D].tolist(), c[o:o + D].tolist())) == {(s * N + v, n) for v, n in ends.items()}, (s, u)
            assert (k[o + D:o + w] == ssa.wedge._PAD).all() and (c[o + D:o + w] == 0).all(), (s, u)

    rowptr, col = planted.csr(N, p['ei'])
    for slices in (1, 3, ssa._native.WEDGE_MAX_SLICES):
        keys_all, keys = _guarded(total, torch.int64, dev)
        ssa.wedge._launch_emit(g, sources, take, offsets, slots, slices, keys)
        torch.cuda.synchronize()
        _untouched(keys_all, total, fold_places)
        k = keys.cpu().numpy()
        for s, ((u, w, at), o) in enumerate(zip(block, offsets_np)):
            if planted.emits(w, slots):
                order = planted.emit_order(rowptr, col, u)  # w ascending in row u, then v ascending in row w
                ids, n = np.unique(order, return_counts=True)
                assert dict(zip(ids.tolist(), n.tolist())) == p['expect']['ends'][at]
                np.testing.assert_array_equal(k[o:o + w], s * N + order, err_msg=f'source {u} at {slices} slices')


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['walks_46341_squared', 'walks_2_to_31'])
def test_too_many_walks(ssa, dev, graphs, name):
    """W(u) >= 2^31: counted exactly in 64 bits, skipped and reported, whatever max_walks says; the sources beside it are listed"""
    p = graphs(name)
    N, ei, g, src, expect, made = p['N'], p['ei'], p['g'], p['src'], p['expect'], p['made']
    giant = made['giant']
    assert expect['walks'][giant] == {'walks_46341_squared': 2147488281, 'walks_2_to_31': 1 << 31}[name]
    want = planted.want(N, ei, src, expect)
    assert want[3] == 1 and want[0][giant] == want[0][giant + 1] and np.diff(want[0])[[made['beside'], made['ordinary']]].tolist() == [1, 2]
    sd = torch.from_numpy(src).to(dev)
    for cap in (None, 2 ** 40):
        rowptr, ids, common, info = g.candidates(sd, max_walks=cap, return_info=True)
        _assert_rows((rowptr, ids, common), want, dev)
        assert info['walks'].dtype == torch.int64 and info['walks'].tolist() == expect['walks'].tolist()
        assert info['skipped_sources'] == 1
        assert (info['lds_sources'], info['large_sources']) == planted.tiers(expect['walks'], ssa._native.WEDGE_MAX_SLOTS)
        assert planted.emits(int(expect['walks'][made['beside']]), ssa._native.WEDGE_MAX_SLOTS), 'the source beside the giant takes the large tier'
    beside = slice(int(want[0][made['beside']]), int(want[0][made['beside'] + 1]))
    assert want[2][beside].tolist() == [int(expect['walks'][made['beside']])]  # (every walk into one node, through the large tier)
    # the k best by the head, h = 1, against score_links over the plan's pairs; the tables are those of the graph without its copies
    eh = _eh(ssa, h=1)
    table, cards = eh.build_hash_tables(N, torch.from_numpy(np.unique(ei, axis=1)).to(dev))
    head = _head(ssa, 1, False, 41)
    ids, scores = eh.topk_links_wedge(sd, table, cards, 3, head, g)
    w_ids, w_scores = _brute_force(eh, table, cards, head, None, src, N, 3, want, dev)
    np.testing.assert_array_equal(ids.cpu().numpy(), w_ids)
    np.testing.assert_array_equal(_bits(scores.cpu().numpy()), _bits(w_scores))
    assert (ids[giant] == -1).all() and torch.isinf(scores[giant]).all() and (ids[made['ordinary'], :2] >= 0).all()
