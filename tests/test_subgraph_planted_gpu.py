"""ss_subgraph_adj and ss_subgraph_labels (csrc/ss_subgraph.hip) called directly on the planted arrays of tests/subgraph_planted.py, and
ElphHashes.exact_subgraphs once on 3 100 links.  The adjacency: runs of equal sources across the 16-lane steps, steps of 0, 1 and 16
finds, deg == switch * n against deg == switch * n + 1, empty first / middle / last rows, a second sweep of the grid -- count then fill
at switch_ratio 0, the default and 2^31 - 1, masked and not; counts, nbr, weight and roots EQUAL subgraph_restatement.adjacency_of_rows.
The labels: paths of 2 048, 2 049 and 5 000 nodes, frontiers of 15 / 16 / 17 and 255 / 256 / 257, two sides sharing a pass of 16, a
K_{64,64} layer, a cut through the partner, one-way arcs, one root, DRNL 2^40 + 1, the tier limit at 17, 2 048 and 4 096, and 3 079
rows through 1 536 workgroups -- z EQUALS subgraph_restatement.link_labels row by row for 'drnl', 'de' and 'de+'.  Every output sits
between guard words that must stay as they were.  All comparisons are exact.  The planted claims are pinned by
tests/test_subgraph_planted_host.py; what ran on an MI355X, and which mutation of the kernels each test catches:
profiles/subgraph_planted_tests.txt."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import subgraph_planted as planted
import subgraph_restatement as sr
from test_subgraph_planted_host import scipy_adjacency

pytestmark = pytest.mark.gpu

GUARD = 64  # words on either side of every output
PATTERN = 0x5A5A5A5A  # no depth, no kUnreached / kRemoved, no local index of these rows
LABELS = ('drnl', 'de', 'de+')
RATIOS = (0, planted.DEFAULT_SWITCH, (1 << 31) - 1)


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _guarded(size, dtype, dev):
    """(the buffer, the `size` words in its middle)"""
    fill = PATTERN if dtype == torch.int32 else (PATTERN << 32) | PATTERN
    buf = torch.full((size + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + size]


def _guards_hold(buf, what):
    fill = PATTERN if buf.dtype == torch.int32 else (PATTERN << 32) | PATTERN
    assert bool((buf[:GUARD] == fill).all()) and bool((buf[buf.numel() - GUARD:] == fill).all()), f'a store left {what}'


def _to(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the planted arrays are read-only)


# ---- adjacency -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def adj(dev):
    """name -> (case, its arrays on the device, {mask: restated (roots, adj_ptr, nbr, weight)}), made once"""
    made = {}

    def get(name):
        if name not in made:
            c = planted.adj_switch_probe() if name == 'switch_probe' else planted.ADJ_CASES[name]()
            rowptr, col = c.csr()
            d = Namespace(csr_rowptr=_to(dev, rowptr), col=_to(dev, col), links=_to(dev, c.links), rowptr=_to(dev, c.rowptr), ids=_to(dev, c.ids))
            restate = scipy_adjacency if name == 'sweep' else lambda c_, m: sr.adjacency_of_rows(c_.N, c_.ei, c_.links, c_.rowptr, c_.ids, m)
            made[name] = c, d, {m: restate(c, m) for m in (False, True)}
        return made[name]

    return get


def _adj_call(ssa, dev, c, d, mask, ratio, counts, adj_ptr, nbr, weight, roots, col=None):
    from subgraph_sketching_amd._runtime import _ptr, _stream
    flags = ssa._native.SS_FLAG_MASK_TARGET if mask else 0
    ssa._native.check(ssa._native.lib().ss_subgraph_adj(_ptr(d.csr_rowptr), _ptr(d.col if col is None else col), c.N, _ptr(d.links), len(c.links),
                                                        _ptr(d.rowptr), _ptr(d.ids), c.T, flags, ratio, _ptr(counts), _ptr(adj_ptr), _ptr(nbr),
                                                        _ptr(weight), _ptr(roots), _stream(dev)), 'ss_subgraph_adj')
    torch.cuda.synchronize(dev)


def _count_then_fill(ssa, dev, c, d, mask, ratio, want):
    roots, adj_ptr, nbr, weight = want
    what = f'{c.name} mask={mask} switch_ratio={ratio}'
    cbuf, counts = _guarded(c.T, torch.int32, dev)
    _adj_call(ssa, dev, c, d, mask, ratio, counts, None, None, None, None)
    np.testing.assert_array_equal(counts.cpu().numpy(), np.diff(adj_ptr), err_msg=f'counts, {what}')
    _guards_hold(cbuf, f'counts, {what}')
    A = int(adj_ptr[-1])
    nbuf, n_out = _guarded(A, torch.int32, dev)
    wbuf, w_out = _guarded(A, torch.int32, dev)
    rbuf, r_out = _guarded(2 * len(c.links), torch.int32, dev)
    r_out.fill_(planted.PRESET_ROOT)
    offsets = _to(dev, adj_ptr)
    _adj_call(ssa, dev, c, d, mask, ratio, None, offsets, n_out, w_out, r_out)
    np.testing.assert_array_equal(n_out.cpu().numpy(), nbr, err_msg=f'nbr, {what}')
    np.testing.assert_array_equal(w_out.cpu().numpy(), weight, err_msg=f'weight, {what}')
    # the roots of an empty row are not written: they keep what they held
    np.testing.assert_array_equal(r_out.cpu().numpy().reshape(-1, 2), np.where(roots < 0, planted.PRESET_ROOT, roots), err_msg=f'roots, {what}')
    for buf, name in ((nbuf, 'nbr'), (wbuf, 'weight'), (rbuf, 'roots')):
        _guards_hold(buf, f'{name}, {what}')


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('name', list(planted.ADJ_CASES))
def test_adjacency_equals_the_restatement(ssa, dev, adj, name, mask):
    """count then fill at switch_ratio 0 (every node walks the id row), the default and 2^31 - 1 (every node walks its arcs); `switch`
    also at its own ratios, where the planted nodes fall on either side of deg > switch * n"""
    c, d, want = adj(name)
    assert (want[mask][0] < 0).any() == (name in ('empty_rows', 'sweep'))
    for ratio in RATIOS + (planted.SWITCH_RATIOS if name == 'switch' else ()):
        _count_then_fill(ssa, dev, c, d, mask, ratio, want[mask])


@pytest.mark.parametrize('mask', [False, True])
def test_switch_side_shows_on_descending_rows(ssa, dev, adj, mask):
    """the count pass on planted.descending_csr: a boundary node that walks its arcs counts its listed sources, one that walks the id
    row counts none (subgraph_planted.adj_switch_probe) -- deg == switch * n walks the arcs, deg == switch * n + 1 the id row"""
    c, d, _ = adj('switch_probe')
    col = _to(dev, planted.descending_csr(c)[1])
    for ratio in RATIOS + planted.SWITCH_RATIOS:
        want = np.zeros(c.T, dtype=np.int32)
        for b in c.claims['blocks']:
            q, x = b['link'], b['x']
            row = c.ids[c.rowptr[q]:c.rowptr[q + 1]]
            u, v = c.links[q]
            listed = set(c.in_row(x).tolist()) & set(row.tolist()) - {x} - ({u if x == v else v} if mask and u != v else set())
            walks_ids = b['deg'] > ratio * b['n']
            assert ratio != b['ratio'] or walks_ids == b['by_ids']
            want[c.rowptr[q] + np.searchsorted(row, x)] = 0 if walks_ids else len(listed)
        cbuf, counts = _guarded(c.T, torch.int32, dev)
        _adj_call(ssa, dev, c, d, mask, ratio, counts, None, None, None, None, col=col)
        np.testing.assert_array_equal(counts.cpu().numpy(), want, err_msg=f'switch_ratio={ratio}')
        _guards_hold(cbuf, 'counts')


# ---- labels ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lab(dev):
    """name -> (case, its arrays on the device, expected(label, max_dist): link_labels row by row, computed once)"""
    made = {}

    def get(name):
        if name not in made:
            c = planted.LABEL_CASES[name]()
            nbr = c.nbr if c.nbr.size else np.zeros(1, dtype=np.int32)  # (no arcs: not a null pointer, as subgraphs.py allocates it)
            d = Namespace(rowptr=_to(dev, c.rowptr), roots=_to(dev, c.roots), adj_ptr=_to(dev, c.adj_ptr), nbr=_to(dev, nbr))
            z = {}

            def expected(label, md):
                if (label, md) not in z:
                    rows = [sr.link_labels(*c.row(q), label, md) for q in range(c.B) if c.rowptr[q + 1] > c.rowptr[q]]
                    z[(label, md)] = np.concatenate(rows).astype(np.int64)
                return z[(label, md)]

            made[name] = c, d, expected
        return made[name]

    return get


def _label_call(ssa, dev, c, d, label, max_dist, lds):
    """-> z as numpy, after the guard checks of z and the workspace"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    what = f'{c.name} {label} max_dist={max_dist} lds_max_nodes={lds}'
    ws = planted.ws_ptr(c.rowptr, lds)
    ws_dev, ws_nodes = _to(dev, ws), int(ws[-1])
    sbuf, space = _guarded(4 * ws_nodes, torch.int32, dev) if ws_nodes else (None, None)
    two = label != 'drnl'
    zbuf, z = _guarded(c.T * (2 if two else 1), torch.int64, dev)
    mode = ssa._native.SUBGRAPH_LABELS[label]
    ssa._native.check(ssa._native.lib().ss_subgraph_labels(_ptr(d.rowptr), c.B, _ptr(d.roots), _ptr(d.adj_ptr), _ptr(d.nbr), mode, max_dist, lds,
                                                           _ptr(ws_dev), _ptr(space), _ptr(z), _stream(dev)), 'ss_subgraph_labels')
    torch.cuda.synchronize(dev)
    _guards_hold(zbuf, f'z, {what}')
    if ws_nodes:
        _guards_hold(sbuf, f'the workspace, {what}')
        space = space.cpu().numpy()
        for q in np.flatnonzero(np.diff(ws) > 0):  # an off-chip row keeps its depths from u in the first n words of its slice
            assert (space[4 * ws[q]:4 * ws[q] + (c.rowptr[q + 1] - c.rowptr[q])] != PATTERN).all(), f'row {q} did not use its workspace, {what}'
    z = z.cpu().numpy()
    return z.reshape(-1, 2) if two else z


LABEL_RUNS = [(name, label) for name in planted.LABEL_CASES for label in LABELS]


@pytest.mark.parametrize('name,label', LABEL_RUNS)
def test_labels_equal_the_restatement(ssa, dev, lab, name, label):
    c, d, expected = lab(name)
    for lds in c.lds:
        for md in c.max_dists:
            np.testing.assert_array_equal(_label_call(ssa, dev, c, d, label, md, lds), expected(label, md),
                                          err_msg=f'{name} {label} max_dist={md} lds_max_nodes={lds}')


def test_drnl_beyond_32_bits(ssa, dev, lab):
    c, d, _ = lab('far')
    assert _label_call(ssa, dev, c, d, 'drnl', planted.MAX_DIST_TOP, planted.LDS_NODES).tolist() == [1, 1, (1 << 40) + 1]
    assert planted.MAX_DIST_TOP == ssa._native.SUBGRAPH_MAX_DIST


def test_limit_above_the_hardware_limit_is_the_hardware_limit(ssa, dev, lab):
    """lds_max_nodes = 4 096: the 2 048-node row is labelled on chip, the 2 049-node row in its workspace slice (the only one laid out:
    _label_call finds its depths there) -- and with no workspace at all the 2 049-node row is left alone, not taken on chip"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    c, d, expected = lab('limits')
    assert planted.ws_ptr(c.rowptr, 4096)[-1] == 2049
    np.testing.assert_array_equal(_label_call(ssa, dev, c, d, 'de', 1000, 4096), expected('de', 1000))
    zbuf, z = _guarded(2 * c.T, torch.int64, dev)
    ws = _to(dev, planted.ws_ptr(c.rowptr, 4096))
    mode = ssa._native.SUBGRAPH_LABELS['de']
    ssa._native.check(ssa._native.lib().ss_subgraph_labels(_ptr(d.rowptr), c.B, _ptr(d.roots), _ptr(d.adj_ptr), _ptr(d.nbr), mode, 1000, 4096,
                                                           _ptr(ws), None, _ptr(z), _stream(dev)), 'ss_subgraph_labels')
    torch.cuda.synchronize(dev)
    z = z.cpu().numpy().reshape(-1, 2)
    last = int(c.rowptr[-2])
    np.testing.assert_array_equal(z[:last], expected('de', 1000)[:last])
    assert (z[last:] == ((PATTERN << 32) | PATTERN)).all()
    _guards_hold(zbuf, 'z')


# ---- through exact_subgraphs -----------------------------------------------------------------------------------------------------------------
def test_exact_subgraphs_on_3100_links(ssa, dev):
    """3 100 links (every label workgroup takes two or three rows) of a 300-node graph, h = 2, max_nodes at the median row and an
    on-chip limit of 8: empty, on-chip and workspace rows in one launch, every field and two label modes against the restatement"""
    n, ei, links = planted.api_graph()
    sizes = np.diff(sr.restate(n, ei, links, 2, mask_target=True).rowptr)
    cap = int(np.median(sizes))
    sub = sr.restate(n, ei, links, 2, mask_target=True, max_nodes=cap)
    kept = np.diff(sub.rowptr)
    assert (kept == 0).sum() > 500 and ((kept > 0) & (kept <= 8)).sum() > 20 and (kept > 8).sum() > 500 and len(links) > 2 * planted.LABEL_GRID
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    ld, ed = _to(dev, links), _to(dev, ei)
    old = ssa.knobs.EXACT_LDS_MAX_NODES
    ssa.knobs.EXACT_LDS_MAX_NODES = 8
    try:
        for label in ('drnl', 'de+'):
            sg = eh.exact_subgraphs(ld, n, ed, mask_target=True, max_nodes=cap, node_label=label)
            for k in ('rowptr', 'ids', 'dist', 'roots', 'adj_ptr', 'nbr', 'weight'):
                np.testing.assert_array_equal(getattr(sg, k).cpu().numpy(), getattr(sub, k), err_msg=f'{k} ({label})')
            np.testing.assert_array_equal(sg.z.cpu().numpy(), sr.labels(sub, label), err_msg=f'z ({label})')
    finally:
        ssa.knobs.EXACT_LDS_MAX_NODES = old
