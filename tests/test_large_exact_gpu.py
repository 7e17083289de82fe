"""The exact and subgraph kernels where their two large objects pass 2^31 (shapes, graphs and expectations: tests/large_exact_helpers.py,
pinned on the CPU by tests/test_large_exact_host.py; times and peaks: profiles/large_exact_tests.txt).

Part A -- the slot arena past 2^31 uint32 words.  N = 2^22 + 2^18, 256 slots of 10 027 008 words: slots 215 .. 255 start beyond word
2^31, slots 108 .. 255 beyond byte 2^32.  ss_exact_large, ss_exact_nodes_large and ss_sampled_nodes_large answer 4 096 links with
EXACT_LDS_MAX_NODES = 0 (every link takes a slot) and must return, array for array, what the on-chip tier returns with the default
limit (no arena involved) and, for the first 256 links, what the host restatements return; afterwards every distance word of the arena
is zero and a second call returns the same tensors.
Why a wrapped slot base cannot pass: it puts two of the 256 workgroups on one slot, so their level bytes and visit lists collide and
the ordered scan of the node kernels emits or clears the other workgroup's nodes; the links' balls are all different, so a shared slot
cannot reproduce the on-chip answer, and what the row comparison might miss the zero check finds.  The tests do not assert which slot
served which link.  The argument rests on all 256 workgroups being resident at once -- one per CU of an MI355X -- and on each of them
taking links from the shared cursor: there are 16 links per workgroup and in the node kernels every link costs its workgroup at least
two scans of a slot's 1.1 M distance words, so no workgroup can drain the list before the others have started.  (In ss_exact_large a
link costs only its walk; the feature case leans on the launch being one wave of workgroups started together.)

Part B -- more than 2^31 arcs.  520 links inside a 2 048-clique, h = 1, masked, DRNL: 2 179 972 084 arcs, so adj_ptr, nbr and weight
pass index 2^31 inside row 512 and seven rows lie wholly beyond it.  One exact_subgraphs call is checked against the closed forms in
full; ss_subgraph_labels is then run on that adjacency with every row in the device workspace, and ss_subgraph_adj again walking the
id rows, into fresh buffers."""
import time
from argparse import Namespace

import numpy as np
import pytest
import torch

import large_exact_helpers as lx
from large_table_helpers import GB, require_free_memory

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


@pytest.fixture
def lds_limit(ssa):
    """sets knobs.EXACT_LDS_MAX_NODES for one test and restores it"""
    old = ssa.knobs.EXACT_LDS_MAX_NODES
    yield lambda value: setattr(ssa.knobs, 'EXACT_LDS_MAX_NODES', value)
    ssa.knobs.EXACT_LDS_MAX_NODES = old


def _eh(ssa, h):
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))


def _report(what, t0, **more):
    torch.cuda.synchronize()
    extra = ''.join(f', {k} = {v}' for k, v in more.items())
    print(f'\n[large exact] {what}: {time.time() - t0:.2f} s, torch.cuda.max_memory_allocated() = {torch.cuda.max_memory_allocated()} bytes{extra}')


# ---- Part A: the slot arena ------------------------------------------------------------------------------------------------------------
class Arena(object):
    """what the arena fixture holds; release() reports the peak of the tests that used it and drops the graph and the arena itself --
    10.3 GB that would otherwise stay with exact._ARENA for the rest of the session.  The arc fixture releases it too: a module-scoped
    fixture lives until the end of the module"""
    live = None

    def release(self, ssa, dev):
        if Arena.live is not self:
            return
        Arena.live = None
        ssa.knobs.EXACT_LARGE_SLOTS = self.old_slots
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev)
        print(f'\n[large exact] arena tests: peak torch.cuda.max_memory_allocated() = {peak} bytes ({peak / GB:.2f} GiB)')
        ssa.exact._ARENA.clear()
        for name in ('g', 'links', 'eh', 'nb', 'host'):
            setattr(self, name, None)
        torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def arena(ssa, dev):
    """the graph, the links, the engine and (lazily, once each) the host restatements of the first 256 links; 256 slots asked for"""
    require_free_memory(dev, lx.arena_needs(), 'the 256-slot arena at N = 2^22 + 2^18 (a quarter of the free memory at most) and its graph')
    a = Arena()
    a.old_slots = ssa.knobs.EXACT_LARGE_SLOTS
    ssa.knobs.EXACT_LARGE_SLOTS = lx.ARENA_SLOTS
    Arena.live = a
    torch.cuda.reset_peak_memory_stats(dev)
    try:
        a.g = lx.arena_graph(dev)
        a.links = lx.arena_links(a.g)
        a.eh = _eh(ssa, lx.ARENA_H)
        a.nb = lx.neighbourhood(a.g, a.links[:lx.ARENA_HOST_LINKS])
        a.host = {}
        yield a
    finally:
        a.release(ssa, dev)


def _host(a, kind, mask=False):
    if (kind, mask) not in a.host:
        make = {'features': lambda: lx.restate_features(a.nb, lx.ARENA_H, mask), 'nodes': lambda: lx.restate_nodes(a.nb, lx.ARENA_H, mask),
                'sampled': lambda: lx.restate_sampled(a.nb, lx.ARENA_H)}[kind]
        a.host[(kind, mask)] = make()
    return a.host[(kind, mask)]


def _same_tensors(got, want, names):
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.dtype.is_floating_point:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), name


def _first_rows(rowptr, ids, per_node, count):
    """the rows of the first `count` links on the host"""
    end = int(rowptr[count])
    return rowptr[:count + 1].cpu().numpy(), ids[:end].cpu().numpy(), per_node[:end].cpu().numpy()


def test_arena_preconditions(ssa, dev, arena):
    """from the host arithmetic alone, before any launch: 256 slots, 41 of them wholly beyond word 2^31, and the star's hub above the
    degree from which the whole workgroup walks a frontier node"""
    n = lx.ARENA_N
    words = lx.slot_words(n)
    assert ssa._native.lib().ss_exact_slot_bytes(n) == 4 * words
    slots, mem = ssa.exact._arena(dev, n)
    assert slots == lx.ARENA_SLOTS == 256 and mem.numel() == 4 * words * slots == 10267656192
    assert slots * words > (1 << 31) + 16 * words
    assert lx.first_slot_at_or_beyond(n, 1 << 31) == 215 and lx.first_slot_at_or_beyond(n, 1 << 30) == 108
    assert arena.links.size(0) == 16 * slots
    w = lx.wrap(arena.links, n)
    assert int(arena.links.min()) >= -n and int((arena.links < 0).sum()) > 1000 and int((w >= n - lx.ARENA_TOP).sum()) > 500
    assert int((w[:, 0] == w[:, 1]).sum()) >= 8 and int((w == arena.g.hub).sum()) >= 16
    first = w[:lx.ARENA_HOST_LINKS]  # the links the host restates hold every kind
    assert bool((first == arena.g.hub).any()) and bool((first[:, 0] == first[:, 1]).any()) and bool((first >= n - lx.ARENA_TOP).any())
    assert bool((arena.links[:lx.ARENA_HOST_LINKS] < 0).any())
    assert int((arena.g.ei[1] == arena.g.hub).sum()) > lx.BIG_DEGREE


@pytest.mark.parametrize('mask', [False, True])
def test_arena_exact_features(ssa, dev, arena, lds_limit, mask):
    t0 = time.time()
    n, L = lx.ARENA_N, arena.links.size(0)
    call = lambda st: ssa.exact.exact_subgraph_features(arena.eh, arena.links, n, arena.g.ei, return_counts=True, stats=st, mask_target=mask)
    lds_limit(0)
    st = {}
    slot = call(st)
    assert st['overflow'] == L and st['slots'] == lx.ARENA_SLOTS  # every link took a slot
    assert lx.arena_dist_words_are_zero(ssa, dev)
    _same_tensors(call({}), slot, ('features', 'I', 'balls'))
    assert lx.arena_dist_words_are_zero(ssa, dev)
    lds_limit(2048)
    st = {}
    chip = call(st)
    assert st['overflow'] == 0  # every link stayed on chip: the star's unions fit
    _same_tensors(slot, chip, ('features', 'I', 'balls'))
    wf, wI, wb = _host(arena, 'features', mask)
    k = lx.ARENA_HOST_LINKS
    assert np.array_equal(slot[1][:k].cpu().numpy(), wI) and np.array_equal(slot[2][:k].cpu().numpy(), wb)
    assert np.array_equal(slot[0][:k].cpu().numpy().view(np.int32), wf.view(np.int32))
    if not mask:
        assert int((slot[1][:, 1, 1] > 0).sum()) > L // 4  # the balls of the edge links meet: the counts are not all zero
    _report(f'arena exact features mask={mask}', t0, arena_bytes=ssa.exact._arena(dev, n)[1].numel(), slots=st['slots'])


@pytest.mark.parametrize('mask', [False, True])
def test_arena_exact_nodes(ssa, dev, arena, lds_limit, mask):
    t0 = time.time()
    n, L = lx.ARENA_N, arena.links.size(0)
    call = lambda: arena.eh.exact_subgraph_nodes(arena.links, n, arena.g.ei, mask_target=mask, return_info=True)
    names = ('rowptr', 'ids', 'dist')
    lds_limit(0)
    slot = call()
    assert slot[3]['large_links'] == L and slot[3]['lds_links'] == 0
    assert lx.arena_dist_words_are_zero(ssa, dev)
    _same_tensors(call()[:3], slot[:3], names)
    assert lx.arena_dist_words_are_zero(ssa, dev)
    lds_limit(2048)
    chip = call()
    assert chip[3]['large_links'] == 0 and chip[3]['lds_links'] == L
    _same_tensors(slot[:3], chip[:3], names)
    for g, w, name in zip(_first_rows(*slot[:3], lx.ARENA_HOST_LINKS), _host(arena, 'nodes', mask), names):
        np.testing.assert_array_equal(g, w, err_msg=name)
    _report(f'arena exact nodes mask={mask}', t0, listed_nodes=slot[1].numel())


def test_arena_sampled_nodes(ssa, dev, arena, lds_limit):
    t0 = time.time()
    n, L = lx.ARENA_N, arena.links.size(0)
    call = lambda: arena.eh.sampled_subgraph_nodes(arena.links, n, arena.g.ei, return_info=True, **lx.SAMPLED)
    names = ('rowptr', 'ids', 'hop')
    lds_limit(0)
    slot = call()
    assert slot[3]['large_links'] == L and slot[3]['lds_links'] == 0
    assert lx.arena_dist_words_are_zero(ssa, dev)
    _same_tensors(call()[:3], slot[:3], names)
    assert lx.arena_dist_words_are_zero(ssa, dev)
    lds_limit(2048)
    chip = call()
    assert chip[3]['large_links'] == 0 and chip[3]['lds_links'] == L
    _same_tensors(slot[:3], chip[:3], names)
    assert 0 < slot[3]['sampled_links'] == chip[3]['sampled_links'] <= L  # the caps drop nodes
    for g, w, name in zip(_first_rows(*slot[:3], lx.ARENA_HOST_LINKS), _host(arena, 'sampled'), names):
        np.testing.assert_array_equal(g, w, err_msg=name)
    _report('arena sampled nodes', t0, listed_nodes=slot[1].numel(), sampled_links=slot[3]['sampled_links'])


# ---- Part B: more than 2^31 arcs ---------------------------------------------------------------------------------------------------------
class Arcs(object):
    pass


@pytest.fixture(scope='module')
def arcs(ssa, dev):
    """the clique batch, its closed forms and ONE exact_subgraphs call (17.4 GB of nbr + weight), shared by the three tests below and
    dropped with the fixture"""
    if Arena.live is not None:
        Arena.live.release(ssa, dev)
    require_free_memory(dev, lx.arcs_needs(), 'the adjacency of 2.18e9 arcs (nbr + weight 17.4 GB), a second pair for the id-row walk and the checks')
    torch.cuda.reset_peak_memory_stats(dev)
    b = Arcs()
    b.n, b.ei = lx.clique_graph(dev)
    b.links = lx.clique_links(dev)
    b.want = lx.clique_expected(b.links)
    # from the closed form alone: the batch passes 2^31 arcs with room to spare, and whole rows lie beyond
    assert b.want.A > (1 << 31) + (1 << 24)
    assert sum(s >= 1 << 31 for s in b.want.row_start[:-1]) >= 5
    b.eh = _eh(ssa, 1)
    t0 = time.time()
    b.sg = b.eh.exact_subgraphs(b.links, b.n, b.ei, mask_target=True, node_label='drnl')
    _report('arcs: the exact_subgraphs call', t0, arcs=b.want.A)
    try:
        yield b
    finally:
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev)
        print(f'\n[large exact] arc tests: peak torch.cuda.max_memory_allocated() = {peak} bytes ({peak / GB:.2f} GiB)')
        b.__dict__.clear()
        torch.cuda.empty_cache()


def _chunks(b):
    L = b.links.size(0)
    for q0 in range(0, L, lx.CHUNK_ROWS):
        q1 = min(q0 + lx.CHUNK_ROWS, L)
        yield q0, q1, b.want.row_start[q0], b.want.row_start[q1]


def test_arcs_equal_the_closed_forms(ssa, dev, arcs):
    t0 = time.time()
    sg, want = arcs.sg, arcs.want
    for name in ('rowptr', 'ids', 'dist', 'roots', 'adj_ptr', 'z'):
        g, w = getattr(sg, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), name
    assert int(sg.adj_ptr[-1]) == want.A == sg.nbr.numel() == sg.weight.numel()
    assert sg.nbr.dtype == sg.weight.dtype == torch.int32
    for q0, q1, a0, a1 in _chunks(arcs):
        nbr, weight = lx.clique_expected_arcs(want, q0, q1)
        assert nbr.numel() == a1 - a0
        assert torch.equal(sg.nbr[a0:a1], nbr), f'nbr of links {q0} .. {q1 - 1} (arcs {a0} .. {a1 - 1})'
        assert torch.equal(sg.weight[a0:a1], weight), f'weight of links {q0} .. {q1 - 1} (arcs {a0} .. {a1 - 1})'
        del nbr, weight
    _report('arcs against the closed forms', t0, arcs=want.A)


def test_arcs_labels_through_the_device_workspace(ssa, dev, arcs):
    """ss_subgraph_labels on the adjacency just made with lds_max_nodes = 1024: every row (2 048 nodes) takes the device-workspace path
    with its int32 queues, and walks adjacency rows on both sides of arc 2^31.  The workspace is laid out as
    subgraphs._adjacency_and_labels lays it out"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    t0 = time.time()
    sg, limit = arcs.sg, 1024
    L, T = arcs.links.size(0), sg.ids.numel()
    sizes = sg.rowptr[1:] - sg.rowptr[:-1]
    ws_ptr = torch.zeros((L + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(torch.where(sizes > min(limit, 2048), sizes, torch.zeros_like(sizes)), 0, out=ws_ptr[1:])
    ws_nodes = int(ws_ptr[-1])
    assert ws_nodes == T  # every row is labelled off chip
    ws = torch.empty((4 * ws_nodes,), dtype=torch.int32, device=dev)
    z = torch.full((T,), -1, dtype=torch.int64, device=dev)
    ssa._native.check(ssa._native.lib().ss_subgraph_labels(_ptr(sg.rowptr), L, _ptr(sg.roots), _ptr(sg.adj_ptr), _ptr(sg.nbr),
                                                           ssa._native.SUBGRAPH_LABELS['drnl'], 1000, limit, _ptr(ws_ptr), _ptr(ws), _ptr(z),
                                                           _stream(dev)), 'ss_subgraph_labels')
    assert torch.equal(z, sg.z) and torch.equal(z, arcs.want.z)
    _report('arcs: labels through the device workspace', t0)


def test_arcs_id_row_walk_fills_the_same_adjacency(ssa, dev, arcs):
    """the count and the fill of ss_subgraph_adj again with switch_ratio = 0 -- every listed node walks the link's id row and takes two
    bounds in its CSR row, where the call above walked the arcs -- into fresh buffers: the same adj_ptr, nbr and weight"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    t0 = time.time()
    sg, want = arcs.sg, arcs.want
    L, T, A = arcs.links.size(0), sg.ids.numel(), want.A
    deg = torch.bincount(arcs.ei[1], minlength=arcs.n)
    assert 0 < int(deg.max()) <= int(ssa.knobs.SUBGRAPH_ADJ_SWITCH) * want.K  # the call above took the arc walk for every node
    csr = arcs.eh._csr_cache.get(arcs.ei, arcs.n, dev)
    col = arcs.eh._sorted_rows_cache.get(arcs.ei, arcs.n, dev, csr)
    lk = arcs.links.contiguous()
    lib, stream = ssa._native.lib(), _stream(dev)
    adj = lambda counts, adj_ptr, nbr, weight, roots: ssa._native.check(
        lib.ss_subgraph_adj(_ptr(csr.rowptr), _ptr(col), arcs.n, _ptr(lk), L, _ptr(sg.rowptr), _ptr(sg.ids), T, ssa._native.SS_FLAG_MASK_TARGET, 0,
                            _ptr(counts), _ptr(adj_ptr), _ptr(nbr), _ptr(weight), _ptr(roots), stream), 'ss_subgraph_adj')
    counts = torch.empty((T,), dtype=torch.int32, device=dev)
    adj(counts, None, None, None, None)
    adj_ptr = torch.zeros((T + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=adj_ptr[1:])
    assert torch.equal(adj_ptr, sg.adj_ptr)  # (so every store of the fill below lands inside its own row of A arcs)
    nbr = torch.full((A,), -1, dtype=torch.int32, device=dev)
    weight = torch.full((A,), -1, dtype=torch.int32, device=dev)
    roots = torch.full((L, 2), -1, dtype=torch.int32, device=dev)
    adj(None, adj_ptr, nbr, weight, roots)
    assert torch.equal(roots, sg.roots)
    for q0, q1, a0, a1 in _chunks(arcs):
        assert torch.equal(nbr[a0:a1], sg.nbr[a0:a1]), f'nbr of links {q0} .. {q1 - 1}'
        assert torch.equal(weight[a0:a1], sg.weight[a0:a1]), f'weight of links {q0} .. {q1 - 1}'
    _report('arcs: the id-row walk', t0)
