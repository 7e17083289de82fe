"""The restatement of cn_pool.common_neighbour_pool (tests/cn_pool_restatement.py) against float64, the chunk rule against the one
running sum, and everything of the plan, the function, the C ABI and the byte model that can be checked without a device."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import cn_pool_restatement as cr

U = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope='module')
def case():
    rowptr, ids, coef = cr.planted()
    F = 8
    x, g = cr.features(cr.N, F), cr.features(len(rowptr) - 1, F, seed=5)
    return dict(rowptr=rowptr, ids=ids, coef=coef, x=x, g=g, out=cr.forward(rowptr, ids, coef, x), grad=cr.grad(rowptr, ids, coef, g, cr.N))


def test_the_planted_list_is_what_its_comment_says(case):
    rowptr, ids = case['rowptr'], case['ids']
    rows = np.diff(rowptr)
    L = len(rows)
    assert L % 2 == 1 and L == 1047 and ids.min() >= 1 and ids.max() == cr.N - 1  # (node 0 is named by nothing)
    assert set(cr.ROW_COUNTS) <= set(rows.tolist()) and cr.REPEAT in rows
    assert rows[0] == 1025 and rows[-1] == 512 and rows[1:4].tolist() == [0, 513, 0] and (rows == 0).sum() == 3
    groups = np.bincount(ids, minlength=cr.N)
    assert groups[list(cr.NODES)].tolist() == list(cr.COUNTS) and groups[cr.REPEAT_NODE] == cr.REPEAT and groups[cr.UNNAMED] == 0
    own = cr.owners(rowptr)
    assert len(np.unique(own[ids == cr.NODES[-1]])) == 1025      # 1 025 entries of 1 025 different links
    assert len(np.unique(own[ids == cr.REPEAT_NODE])) == 1       # 300 entries of one link
    coef = case['coef']
    assert (coef == 0).sum() >= 10 and (coef < 0).sum() >= 10 and (cr.planted(coefficients='unit')[2] == 1).all()
    nodes, nrowptr, order = cr.grouping(ids, cr.N)
    assert nodes.tolist() == np.nonzero(groups)[0].tolist() and np.diff(nrowptr).tolist() == groups[nodes].tolist()
    assert all(np.all(np.diff(order[a:b]) > 0) and np.all(ids[order[a:b]] == n) for n, a, b in zip(nodes, nrowptr[:-1], nrowptr[1:]))


def test_restatement_against_float64(case):
    """every element within gamma_k (|S| @ |x|), gamma_k = k u / (1 - k u), u = 2^-24, k = m + 2 for a row of m entries: one rounding
    per product, m - 1 adds (chunking only shortens the chains, and adds at most the chunk-sum adds, which the sequential count already
    holds), and the slack of tests/test_cn_features_host.py.  The dense S sums the coefficients of repeated ids in float64."""
    rowptr, ids, coef, x, g = (case[k] for k in ('rowptr', 'ids', 'coef', 'x', 'g'))
    S = cr.dense(rowptr, ids, coef, cr.N)
    absS = np.zeros_like(S)
    np.add.at(absS, (cr.owners(rowptr), ids), np.abs(coef.astype(np.float64)))
    worst = {}
    for name, got, want, mag, m in (('forward', case['out'], S @ x.astype(np.float64), absS @ np.abs(x).astype(np.float64), np.diff(rowptr)),
                                    ('backward', case['grad'], S.T @ g.astype(np.float64), absS.T @ np.abs(g).astype(np.float64),
                                     np.bincount(ids, minlength=cr.N))):
        k = (m + 2).astype(np.float64)
        bound = (k * U / (1 - k * U))[:, None] * mag
        err = np.abs(got.astype(np.float64) - want)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
        worst[name] = float(ratio.max())
        print(f'[cn pool] {name}: worst error / bound = {worst[name]:.4f}, max |error| = {err.max():.3e}')
        assert (err <= bound).all(), name
        assert (_bits(got[m == 0]) == 0).all()  # an empty row, a node nothing names: +0.0
    assert 0 < worst['forward'] <= 1 and 0 < worst['backward'] <= 1


def test_adjointness_in_float64(case):
    rowptr, ids, coef, x, g = (case[k] for k in ('rowptr', 'ids', 'coef', 'x', 'g'))
    S = cr.dense(rowptr, ids, coef, cr.N)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    left, right = float(((S @ x64) * g64).sum()), float((x64 * (S.T @ g64)).sum())
    assert abs(left - right) <= 1e-10 * max(abs(left), abs(right), 1.0)
    # ... and the two restated directions are each other's transpose up to float32 rounding
    a, b = float((case['out'].astype(np.float64) * g64).sum()), float((x64 * case['grad'].astype(np.float64)).sum())
    scale = float((np.abs(S) @ np.abs(x64) * np.abs(g64)).sum())
    assert abs(a - left) <= 1100 * U * scale and abs(b - right) <= 1100 * U * scale


def test_one_chunk_is_the_sequential_sum(case):
    rowptr, ids, coef, x, g = (case[k] for k in ('rowptr', 'ids', 'coef', 'x', 'g'))
    seq_out, seq_grad = cr.forward(rowptr, ids, coef, x, sequential=True), cr.grad(rowptr, ids, coef, g, cr.N, sequential=True)
    short_rows, short_groups = np.diff(rowptr) <= cr.C, np.bincount(ids, minlength=cr.N) <= cr.C
    assert (~short_rows).sum() == 6 and (~short_groups).sum() >= 6  # 257, 258, 300, 512, 513, 1 025
    assert np.array_equal(_bits(seq_out[short_rows]), _bits(case['out'][short_rows]))
    assert np.array_equal(_bits(seq_grad[short_groups]), _bits(case['grad'][short_groups]))


def test_a_row_of_258_entries_tells_the_two_sums_apart():
    """One large term in chunk 0, small ones after it: the running sum loses every small term against 2^24 one by one; the chunk rule
    adds the second chunk's own sum, 1 + 1 = 2, which 2^24 holds.  A row of 257 entries could not tell: its second chunk is one term,
    and 2^24 + 1 rounds to 2^24 in both (profiles/graph_prep_tests.txt)."""
    for m, differ in ((258, True), (257, False)):
        rowptr = np.array([0, m], dtype=np.int64)
        ids = np.arange(m, dtype=np.int64)
        coef = np.ones(m, dtype=np.float32)
        x = np.zeros((m, 3), dtype=np.float32)
        x[0] = 2.0 ** 24
        x[256:] = 1.0
        chunked, running = cr.forward(rowptr, ids, coef, x), cr.forward(rowptr, ids, coef, x, sequential=True)
        assert (running == 2.0 ** 24).all()
        assert (chunked == (2.0 ** 24 + 2 if differ else 2.0 ** 24)).all()
        assert (_bits(chunked) != _bits(running)).all() == differ
        # the backward: one node named by m entries of m links
        rowptr_b, ids_b = np.arange(m + 1, dtype=np.int64), np.zeros(m, dtype=np.int64)
        cb, rb = cr.grad(rowptr_b, ids_b, coef, x, 2), cr.grad(rowptr_b, ids_b, coef, x, 2, sequential=True)
        assert (_bits(cb[0]) != _bits(rb[0])).all() == differ and (_bits(cb[1]) == 0).all()


def test_entries_that_are_not_followed_keep_their_place():
    rowptr, ids, coef = np.array([0, 300], dtype=np.int64), np.arange(300, dtype=np.int64), np.ones(300, dtype=np.float32)
    x = cr.features(300, 4)
    use = np.ones(300, dtype=bool)
    use[[3, 255, 256]] = False
    zeroed = x.copy()
    zeroed[~use] = 0
    assert np.array_equal(_bits(cr.forward(rowptr, ids, coef, x, use=use)), _bits(cr.forward(rowptr, ids, coef, zeroed)))


def test_header_and_binding_have_the_symbols():
    import subgraph_sketching_amd as ssa
    sig = ssa._native.SIGNATURES
    for name, n_args in (('ss_cn_rows_chunk', 0), ('ss_cn_rows_workspace_bytes', 2), ('ss_cn_rows_forward', 11), ('ss_cn_rows_forward_hub_partials', 16),
                         ('ss_cn_rows_forward_hub_finish', 10), ('ss_cn_rows_grad', 14), ('ss_cn_rows_grad_hub_partials', 18),
                         ('ss_cn_rows_grad_hub_finish', 12)):
        assert name in sig and len(sig[name][1]) == n_args, name
    assert ssa.common_neighbour_pool is ssa.cn_pool.common_neighbour_pool and ssa.CommonNeighbourBatch is ssa.cn_pool.CommonNeighbourBatch
    assert {'cn_pool', 'CommonNeighbourBatch', 'common_neighbour_pool'} <= set(ssa.__all__)
    lib = ssa._native.lib()
    assert lib.ss_cn_rows_chunk() == 256 == ssa.cn_pool.CN_ROWS_CHUNK == cr.C == lib.ss_aggr_chunk() == lib.ss_link_chunk()
    wb = lib.ss_cn_rows_workspace_bytes
    assert wb(7, 260) == 7 * 260 * 4 and wb(7, 3) == 84 and wb(0, 8) == 0 and wb(-1, 8) == 0 and wb(7, 0) == 0 and wb(1 << 31, 8) == 0
    assert ssa.cn_pool.DEFAULT_HUB_ENTRIES == 256
    assert lib.ss_version() == 129  # (new entry points, no changed one: the ABI number stays)


def test_c_abi_rejects_bad_arguments_on_the_host():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(16)  # never dereferenced: every call below ends in the host-side checks
    big = 1 << 31

    def sweep(fn, ok, needed, bad_values, nothing_to_do):
        for i in needed:
            assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == -1, (fn.__name__, i)
        for i, bad in bad_values:
            assert fn(*[bad if j == i else a for j, a in enumerate(ok)]) == -1, (fn.__name__, i, bad)
        for i in nothing_to_do:  # (no links / nodes / columns / chunks / hubs: SS_OK before any pointer is looked at)
            assert fn(*[0 if j == i else (None if isinstance(a, c_void_p) else a) for j, a in enumerate(ok)]) == 0, (fn.__name__, i)

    #                             rowptr ids  coef  L  T  N  hub x     F  out   stream
    sweep(lib.ss_cn_rows_forward, [fake, fake, fake, 3, 9, 5, 64, fake, 8, fake, None], (0, 1, 2, 7, 9),
          ((3, -1), (3, big), (4, -1), (4, big), (5, -1), (5, big), (6, 0), (6, -3), (8, -1)), (3, 8))
    #                                          rowptr ids  coef  L  T  N  hubs  chunk c_hub nh nc x     F  ws    bytes   stream
    sweep(lib.ss_cn_rows_forward_hub_partials, [fake, fake, fake, 3, 9, 5, fake, fake, fake, 2, 3, fake, 8, fake, 3 * 32, None],
          (0, 1, 2, 6, 7, 8, 11, 13), ((3, -1), (3, big), (4, -1), (4, big), (5, -1), (5, big), (9, -1), (9, 4), (10, -1), (10, big), (12, -1),
                                       (14, 3 * 32 - 1)), (3, 4, 12))
    assert lib.ss_cn_rows_forward_hub_partials(None, None, None, 3, 9, 5, None, None, None, 0, 0, None, 8, None, 0, None) == 0  # no chunks
    #                                        L  hubs  chunk nh nc ws    bytes   F  out   stream
    sweep(lib.ss_cn_rows_forward_hub_finish, [3, fake, fake, 2, 3, fake, 3 * 32, 8, fake, None], (1, 2, 5, 8),
          ((0, -1), (0, big), (3, -1), (3, 4), (4, -1), (4, big), (6, 3 * 32 - 1), (7, -1)), (0, 3, 7))
    #                          nodes rowptr order M  owner coef  T  L  N  hub g     F  grad  stream
    sweep(lib.ss_cn_rows_grad, [fake, fake, fake, 3, fake, fake, 9, 4, 5, 64, fake, 8, fake, None], (0, 1, 2, 4, 5, 10, 12),
          ((3, -1), (3, 6), (3, 10), (6, -1), (6, big), (6, 2), (7, -1), (7, big), (8, -1), (8, big), (9, 0), (9, -3), (11, -1)), (3, 11))
    #                                       rowptr order M  owner coef  T  L  N  hubs  chunk c_hub nh nc g     F  ws    bytes   stream
    sweep(lib.ss_cn_rows_grad_hub_partials, [fake, fake, 3, fake, fake, 9, 4, 5, fake, fake, fake, 2, 3, fake, 8, fake, 3 * 32, None],
          (0, 1, 3, 4, 8, 9, 10, 13, 15), ((2, -1), (2, 6), (5, -1), (5, big), (5, 2), (6, -1), (6, big), (7, -1), (7, big), (11, -1), (11, 4), (12, -1),
                                           (12, big), (14, -1), (16, 3 * 32 - 1)), (2, 14))
    assert lib.ss_cn_rows_grad_hub_partials(None, None, 3, None, None, 9, 4, 5, None, None, None, 0, 0, None, 8, None, 0, None) == 0  # no chunks
    #                                     nodes M  hubs  chunk nh nc N  ws    bytes   F  grad  stream
    sweep(lib.ss_cn_rows_grad_hub_finish, [fake, 3, fake, fake, 2, 3, 5, fake, 3 * 32, 8, fake, None], (0, 2, 3, 7, 10),
          ((1, -1), (1, 6), (4, -1), (4, 4), (5, -1), (5, big), (6, -1), (6, big), (8, 3 * 32 - 1), (9, -1)), (1, 4, 9))


def test_argument_errors_need_no_device():
    import scipy.sparse as sp

    import subgraph_sketching_amd as ssa
    CNB = ssa.CommonNeighbourBatch
    A = sp.csr_matrix(np.ones((4, 4), dtype=np.float32))
    links = torch.zeros((3, 2), dtype=torch.int64)
    for bad in (links[0], links.t(), torch.zeros((3, 3), dtype=torch.int64), links.to(torch.float32), links[None]):
        with pytest.raises(ValueError):
            CNB(A, bad)
    for bad in (None, 'cn', 'JC', torch.ones(3), torch.ones((4, 1)), torch.ones(4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            CNB(A, links, weighting=bad)
    for bad in (0, -1, 2.0, True, '256', 1 << 63):
        with pytest.raises(ValueError):
            CNB(A, links, hub_entries=bad)
        with pytest.raises(ValueError):
            CNB.from_lists(4, torch.tensor([0, 1]), torch.tensor([2]), torch.ones(1), hub_entries=bad)
    with pytest.raises(ValueError):
        CNB(A, links, device='cpu')

    rowptr, ids, coef = torch.tensor([0, 2, 2, 3]), torch.tensor([1, 3, 0]), torch.ones(3)
    for num_nodes in (0, -5, 1 << 31):
        with pytest.raises(ValueError):
            CNB.from_lists(num_nodes, rowptr, ids, coef)
    bad_lists = ((rowptr.to(torch.int32), ids, coef), (rowptr[None], ids, coef), (rowptr[:0], ids, coef), (rowptr.numpy(), ids, coef),
                 (rowptr, ids.to(torch.int32), coef), (rowptr, ids[None], coef), (rowptr, ids, coef.double()), (rowptr, ids, coef[:2]),
                 (rowptr, ids, None), (rowptr, ids, coef.clone().requires_grad_(True)),
                 (torch.tensor([0, 2, 1, 3]), ids, coef),   # descends
                 (torch.tensor([0, 2, 2, 2]), ids, coef),   # ends before T
                 (torch.tensor([0, 2, 2, 4]), ids, coef),   # ends past T
                 (torch.tensor([1, 2, 2, 3]), ids, coef),   # does not start at 0
                 (torch.tensor([0]), ids, coef))            # no link, three entries
    for r, i, c in bad_lists:
        with pytest.raises(ValueError):
            CNB.from_lists(4, r, i, c)
    for bad in (torch.tensor([1, 4, 0]), torch.tensor([1, -1, 0]), torch.tensor([1, 3, 1 << 40])):
        with pytest.raises(IndexError):
            CNB.from_lists(4, rowptr, bad, coef)
    with pytest.raises(ValueError):
        CNB.from_lists(4, rowptr, ids, coef, device='cpu')

    plan = object.__new__(CNB)  # (a plan's host fields: what the function checks before it calls the library)
    plan.num_nodes, plan.device = 4, torch.device('cuda', 0)
    good = torch.zeros((4, 8))
    for x, b in ((good, None), (good, 'plan'), (good.double(), plan), (good.half(), plan), (good[0], plan), (good.numpy(), plan),
                 (torch.zeros((5, 8)), plan), (torch.zeros((3, 8)), plan), (good[None], plan),
                 (good, plan)):  # the last one: right in everything but its device -- there is no CPU fallback and no silent copy
        with pytest.raises(ValueError):
            ssa.common_neighbour_pool(x, b)


def test_byte_model_by_hand():
    """N = 10 nodes, L = 3 links of 2, 0 and 3 entries (T = 5) that name M = 4 distinct nodes"""
    from subgraph_sketching_amd import roofline
    N, L, T, M = 10, 3, 5, 4
    f = roofline.cn_rows_bytes(N, L, T, 8)
    assert f == {'gathered': 5 * 32, 'written': 3 * 32, 'cleared': 0, 'entries': 5 * 12 + 3 * 16, 'workspace': 0, 'total': 160 + 96 + 108}
    b = roofline.cn_rows_bytes(N, L, T, 8, backward=True, M=M)
    assert b == {'gathered': 5 * 32, 'written': 4 * 32, 'cleared': 10 * 32, 'entries': 5 * 16 + 4 * 24, 'workspace': 0, 'total': 160 + 128 + 320 + 176}
    assert roofline.cn_rows_bytes(N, L, T, 8, backward=True)['written'] == 5 * 32          # M defaults to min(N, T)
    # the entry words are read once per pass over the columns: 256 columns a pass with float4 pieces, 64 with scalar ones
    assert roofline.cn_rows_bytes(N, L, T, 1024)['entries'] == 4 * 5 * 12 + 48 and roofline.cn_rows_bytes(N, L, T, 260)['entries'] == 2 * 60 + 48
    assert roofline.cn_rows_bytes(N, L, T, 130)['entries'] == 3 * 60 + 48 and roofline.cn_rows_bytes(N, L, T, 130, backward=True, M=M)['entries'] == 3 * 80 + 96
    assert roofline.cn_rows_bytes(N, L, T, 8, hub_chunks=2)['workspace'] == 2 * 2 * 32     # written by the partials, read by the finish
    assert roofline.cn_rows_bytes(N, L, T, 0)['total'] == 0 and roofline.cn_rows_bytes(N, 0, 0, 8)['total'] == 0
    assert roofline.cn_rows_bytes(0, 0, 0, 8, backward=True)['total'] == 0
