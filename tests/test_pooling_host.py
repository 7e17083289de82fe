"""What subgraph_sketching_amd.pooling promises that needs no device: the restated order (tests/pooling_restatement.py) equals the
torch restatement of PyG's global_sort_pool on tie-free keys and has the documented tie / NaN / +-0 rules, the sequential fp32 sums
lie within gamma_n of float64, sort_pool_k follows the reference's rule, the byte models are counted by hand, the header and the
binding carry the new entries, and every argument error is raised before a device is needed."""
import ctypes

import numpy as np
import pytest
import torch

import pooling_restatement as pr

U = 2.0 ** -24
SIZES = (0, 1, 2, 7, 64, 65, 130, 3, 0, 40)


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    return m


def test_capacity_and_exports(ssa):
    assert ssa.pooling.SORT_CAPACITY == pr.C >= 1024 and ssa._native.lib().ss_pool_sort_capacity() == pr.C
    for name in ('global_sort_pool', 'global_add_pool', 'global_mean_pool', 'center_pool', 'sort_pool_k'):
        assert getattr(ssa, name) is getattr(ssa.pooling, name) and name in ssa.__all__
    for name in ('ss_pool_select', 'ss_pool_gather', 'ss_pool_scatter', 'ss_segment_pool', 'ss_segment_pool_grad', 'ss_center_pool',
                 'ss_center_pool_grad'):
        res, args = ssa._native.SIGNATURES[name]
        assert res is ctypes.c_int32 and args[0] is ctypes.c_void_p and args[1] is ctypes.c_int64 and args[-1] is ctypes.c_void_p
    assert ssa._native.lib().ss_version() == 129


@pytest.mark.parametrize('F', [1, 3, 8])
@pytest.mark.parametrize('k', [1, 5, 64, 200])
def test_order_equals_the_torch_restatement_on_tie_free_keys(F, k):
    rowptr = pr.sizes_to_rowptr(SIZES)
    T = int(rowptr[-1])
    x = pr.features(T, F, seed=F + k)
    out, perm = pr.sort_pool(x, rowptr, k)
    batch = torch.from_numpy(np.repeat(np.arange(len(SIZES)), SIZES))
    want = pr.torch_sort_pool(torch.from_numpy(x), batch, k, size=len(SIZES))
    assert np.array_equal(out.view(np.int32), want.numpy().view(np.int32))
    for q, n in enumerate(SIZES):
        assert sorted(perm[q, :min(n, k)].tolist()) == sorted(pr.order(x[rowptr[q]:rowptr[q + 1], -1])[:k].tolist())
        assert (perm[q, min(n, k):] == -1).all() and not out[q, min(n, k) * F:].any()


def test_tie_nan_and_zero_rules_on_known_answers():
    inf, nan = np.inf, np.nan
    neg_nan = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]  # a NaN with the sign bit set and a payload
    cases = [
        ([1.0, 3.0, 2.0], [1, 2, 0]),
        ([2.0, 2.0, 2.0, 2.0], [0, 1, 2, 3]),                                  # all equal: positions ascend
        ([1.0, 5.0, 1.0, 5.0, 1.0], [1, 3, 0, 2, 4]),                          # ties by ascending position
        ([0.0, -0.0, 1.0, -0.0, 0.0, -1.0], [2, 0, 1, 3, 4, 5]),              # -0.0 ties with +0.0
        ([1.0, nan, inf, -inf, neg_nan, 0.0], [1, 4, 2, 0, 5, 3]),            # NaN first (both signs, by position), then +inf ... -inf
        ([-inf, -3.4e38, -1e-45, 1e-45, 3.4e38, inf], [5, 4, 3, 2, 1, 0]),    # the whole range, denormals included
    ]
    for keys, want in cases:
        assert pr.order(np.array(keys, dtype=np.float32)).tolist() == want, keys
    k = pr.key_u32(np.array([nan, neg_nan, inf, 0.0, -0.0, -inf], dtype=np.float32))
    assert k.tolist() == [0, 0, 0x007FFFFF, 0x7FFFFFFF, 0x7FFFFFFF, 0xFF800000]
    # torch.sort(descending=True) agrees where it is defined: NaN first, then descending (its tie order is its own)
    v = torch.tensor([1.0, nan, inf, -inf, 0.5, 7.0])
    assert torch.sort(v, descending=True).indices.tolist() == pr.order(v.numpy()).tolist()
    # a run of equal keys straddling k: the first positions of the run are taken
    x = np.array([[9.0], [4.0], [4.0], [4.0], [4.0], [1.0]], dtype=np.float32)
    out, perm = pr.sort_pool(x, np.array([0, 6]), 3)
    assert perm.tolist() == [[0, 1, 2]] and out.tolist() == [[9.0, 4.0, 4.0]]
    out, perm = pr.sort_pool(x, np.array([0, 0, 6, 6]), 8)
    assert perm[1].tolist() == [0, 1, 2, 3, 4, 5, -1, -1] and (perm[[0, 2]] == -1).all() and not out[[0, 2]].any()


def test_add_and_mean_against_float64():
    """|fp32 sequential sum - float64 sum| <= gamma_n * sum |x|, gamma_n = n u / (1 - n u) (one more rounding for the mean's
    division); the worst error / bound is printed"""
    sizes = (0, 1, 2, 100, 1000, 5000)
    rowptr = pr.sizes_to_rowptr(sizes)
    x = (np.random.RandomState(4).standard_normal((int(rowptr[-1]), 5)) * 100).astype(np.float32)
    worst = {}
    for mean in (False, True):
        got = pr.segment_pool(x, rowptr, mean).astype(np.float64)
        for q, n in enumerate(sizes):
            rows = x[rowptr[q]:rowptr[q + 1]].astype(np.float64)
            want = rows.sum(0) / (max(n, 1) if mean else 1)
            nu = (n + (1 if mean else 0)) * U
            bound = nu / (1 - nu) * np.abs(rows).sum(0) / (max(n, 1) if mean else 1)
            err = np.abs(got[q] - want)
            assert np.all(err <= bound), (mean, n)
            if n > 1:
                worst[mean] = max(worst.get(mean, 0.0), float((err / bound).max()))
    print(f'[pooling] sequential fp32 sums, worst error / gamma_n bound: add {worst[False]:.4f}, mean {worst[True]:.4f}')
    assert not pr.segment_pool(x, rowptr)[0].any() and not pr.segment_pool(x, rowptr, True)[0].any()  # an empty graph gives 0


def test_backwards_are_the_transposes():
    """<forward(x), g> == <x, backward(g)> in float64 for the linear readouts; the centre product's gradient by its formula"""
    rowptr = pr.sizes_to_rowptr(SIZES)
    T, F, k = int(rowptr[-1]), 3, 5
    x = pr.features(T, F, seed=2)
    rng = np.random.RandomState(3)
    for mean in (False, True):
        g = rng.standard_normal((len(SIZES), F)).astype(np.float32)
        lhs = (pr.segment_pool(x, rowptr, mean).astype(np.float64) * g).sum()
        rhs = (x.astype(np.float64) * pr.segment_pool_backward(g, rowptr, T, mean)).sum()
        assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs))
    g = rng.standard_normal((len(SIZES), k * F)).astype(np.float32)
    out, perm = pr.sort_pool(x, rowptr, k)
    grad = pr.sort_pool_backward(g, rowptr, perm, T)
    assert abs((out.astype(np.float64) * g).sum() - (x.astype(np.float64) * grad).sum()) < 1e-3
    assert (np.abs(grad).sum(1) > 0).sum() == sum(min(n, k) for n in SIZES)
    roots = np.array([[-1, -1], [0, 0], [1, 0], [2, 6], [0, 63], [64, 1], [5, 5], [1, 2], [-1, -1], [39, 0]], dtype=np.int32)
    g = rng.standard_normal((len(SIZES), F)).astype(np.float32)
    tx = torch.from_numpy(x).requires_grad_(True)
    live = np.nonzero(roots[:, 0] >= 0)[0]
    ia, ib = (torch.from_numpy(rowptr[live] + roots[live, j]) for j in (0, 1))
    y = tx[ia] * tx[ib]
    assert np.array_equal(y.detach().numpy(), pr.center_pool(x, rowptr, roots)[live])
    (y * torch.from_numpy(g[live])).sum().backward()
    assert np.array_equal(tx.grad.numpy().view(np.int32), pr.center_pool_backward(x, g, rowptr, roots).view(np.int32))


def test_sort_pool_k_on_literal_lists(ssa):
    cases = [(([5, 50, 20, 30, 40], 0.6, 10), 30), (([5, 50, 20, 30, 40], 0.61, 10), 40), (([1, 2, 3], 0.6, 10), 10),
             (([1, 2, 3], 0.6, 1), 2), (([7, 7, 7, 900], 1, 10), 900), (([3, 4], 25, 10), 25), (([], 0.6, 10), 30),
             (([12, 11, 15, 14, 13, 19, 18, 17, 16, 20], 0.6, 10), 16)]
    for (sizes, ratio, minimum), want in cases:
        assert pr.sort_pool_k(sizes, ratio, minimum) == want
        rowptr = torch.from_numpy(pr.sizes_to_rowptr(sizes))
        assert ssa.sort_pool_k(rowptr, ratio, minimum) == want
    sg = ssa.ExactSubgraphs(torch.from_numpy(pr.sizes_to_rowptr([5, 50, 20, 30, 40])), *[None] * 8)
    assert ssa.sort_pool_k(sg) == 30


def test_byte_models_by_hand(ssa):
    r = ssa.roofline
    assert r.segment_pool_bytes(1000, 10, 32) == 1000 * 128 + 10 * 128 + 88
    assert r.segment_pool_bytes(0, 0, 32) == 8
    # key column 4 T, selected rows + output 2 * L k 4F, perm written and read 2 * L k 4, offsets twice
    assert r.sort_pool_bytes(1000, 10, 32, 30) == 4000 + 2 * 10 * 30 * 128 + 2 * 10 * 30 * 4 + 16 * 11


def test_rowptr_from_batch():
    f = __import__('subgraph_sketching_amd').pooling.rowptr_from_batch
    b = torch.tensor([0, 0, 2, 2, 2, 5])
    assert f(b).tolist() == [0, 2, 2, 5, 5, 5, 6]
    assert f(b, size=8).tolist() == [0, 2, 2, 5, 5, 5, 6, 6, 6]
    assert f(torch.zeros(0, dtype=torch.int64)).tolist() == [0] and f(torch.zeros(0, dtype=torch.int64), size=2).tolist() == [0, 0, 0]
    for bad in (torch.tensor([0, 1, 0]), torch.tensor([3, 2]), torch.tensor([-1, 0])):
        with pytest.raises(ValueError):
            f(bad)
    for bad in (b.to(torch.int32), b[None], b.tolist()):
        with pytest.raises(ValueError):
            f(bad)
    with pytest.raises(ValueError):
        f(b, size=-1)


def test_argument_errors_without_a_device(ssa):
    x = torch.zeros((6, 4))
    batch, rowptr = torch.tensor([0, 0, 1, 1, 1, 2]), torch.tensor([0, 2, 5, 6])
    sg = ssa.ExactSubgraphs(rowptr, None, None, torch.zeros((3, 2), dtype=torch.int32), None, None, None, None, None)
    calls = {'add': lambda x, b=batch, **kw: ssa.global_add_pool(x, b, **kw), 'mean': lambda x, b=batch, **kw: ssa.global_mean_pool(x, b, **kw),
             'sort': lambda x, b=batch, **kw: ssa.global_sort_pool(x, b, 3, **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match='GPU'):
            call(x)                                                   # a CPU x: no fallback
        with pytest.raises(ValueError, match='GPU'):
            call(x, sg)
        for bad in (x.double(), x.half(), x.to(torch.int32), x[0], x[None], x.numpy()):
            with pytest.raises(ValueError, match='float32'):
                call(bad)                                             # a wrong dtype or shape
        with pytest.raises(ValueError, match='not both'):
            call(x, batch, rowptr=rowptr)                             # both batch and rowptr
        with pytest.raises(ValueError, match='not both'):
            call(x, None)                                             # neither
    with pytest.raises(ValueError, match='GPU'):
        ssa.center_pool(x, sg)
    with pytest.raises(ValueError, match='float32'):
        ssa.center_pool(x.double(), sg)
    with pytest.raises(ValueError, match='ExactSubgraphs'):
        ssa.center_pool(x, batch)
    for k in (0, -1, pr.C + 1, 2.0, None, True):
        with pytest.raises(ValueError, match=str(pr.C)):
            ssa.global_sort_pool(x, batch, k)                         # k out of range names C, before x is looked at
    with pytest.raises(ValueError, match='non-decreasing'):
        ssa.pooling.rowptr_from_batch(torch.tensor([0, 1, 1, 0, 2, 2]))  # a decreasing batch (the check global_*_pool runs)


def test_c_entries_report_argument_errors_before_any_launch(ssa):
    """-1 for null pointers, k < 1, negative L or F; L == 0 returns 0 -- on a host without a device"""
    lib = ssa._native.lib()
    buf = ctypes.create_string_buffer(64)
    one = ctypes.c_void_p(ctypes.addressof(buf))  # (never dereferenced on the host)
    assert lib.ss_pool_select(None, 1, one, 1, 1, 1, one, None, None) == -1
    assert lib.ss_pool_select(one, 1, one, 1, 1, 1, None, None, None) == -1
    assert lib.ss_pool_select(one, 1, None, 1, 1, 1, one, None, None) == -1
    assert lib.ss_pool_select(one, 1, one, 1, 1, 0, one, None, None) == -1
    assert lib.ss_pool_select(one, 1, one, 1, 1, pr.C + 1, one, None, None) == -1
    assert lib.ss_pool_select(one, 1, one, 1, 0, 1, one, None, None) == -1
    assert lib.ss_pool_select(one, -1, one, 1, 1, 1, one, None, None) == -1
    assert lib.ss_pool_select(one, 0, one, 1, 1, 1, one, None, None) == 0
    for fn in (lib.ss_pool_gather, lib.ss_pool_scatter):
        assert fn(one, 1, one, 0, one, 1, 4, one, None, None) == -1
        assert fn(one, -1, one, 1, one, 1, 4, one, None, None) == -1
        assert fn(one, 1, one, 1, one, 1, -4, one, None, None) == -1
        assert fn(one, 1, None, 1, one, 1, 4, one, None, None) == -1
        assert fn(one, 1, one, 1, one, 1, 4, None, None, None) == -1
        assert fn(one, 0, one, 1, one, 0, 4, one, None, None) == 0
    assert lib.ss_segment_pool(None, 1, one, 1, 4, 0, one, None, None) == -1
    assert lib.ss_segment_pool(one, 1, one, 1, -1, 0, one, None, None) == -1
    assert lib.ss_segment_pool(one, 1, one, 1, 4, 0, None, None, None) == -1
    assert lib.ss_segment_pool(one, 0, one, 1, 4, 0, one, None, None) == 0
    assert lib.ss_segment_pool_grad(one, -1, one, 1, 4, 0, one, None) == -1
    assert lib.ss_segment_pool_grad(one, 1, None, 1, 4, 0, one, None) == -1
    assert lib.ss_segment_pool_grad(one, 0, one, 0, 4, 0, one, None) == 0
    assert lib.ss_center_pool(one, 1, None, one, 1, 4, one, None, None) == -1
    assert lib.ss_center_pool(one, -1, one, one, 1, 4, one, None, None) == -1
    assert lib.ss_center_pool(one, 0, one, one, 1, 4, one, None, None) == 0
    assert lib.ss_center_pool_grad(one, 1, one, None, one, 1, 4, one, None, None) == -1
    assert lib.ss_center_pool_grad(one, 1, one, one, one, 1, -1, one, None, None) == -1
    assert lib.ss_center_pool_grad(one, 0, one, one, one, 0, 4, one, None, None) == 0
