"""StructureHead and ss_pair_scores without a GPU: the BatchNorm folding, from_module's reading of a model, pickling, and the
argument checks the library makes on the host before any launch."""
import pickle
from argparse import Namespace
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

from score_restatement import U, magnitude as _magnitude, raw_head as _raw_head, unfolded64 as _unfolded64

DIMS = {3: (1, False), 6: (1, True), 8: (2, False), 16: (2, True), 15: (3, False), 30: (3, True)}  # dim -> (h, normalised)


@pytest.mark.parametrize('dim', sorted(DIMS))
def test_folding_matches_the_unfolded_layers(dim):
    import subgraph_sketching_amd as ssa
    h, normalised = DIMS[dim]
    for seed in (1, 2, 3):
        raw = _raw_head(dim, 100 * dim + seed)
        head = ssa.StructureHead(normalised=normalised, **raw)
        assert (head.dim, head.hops, head.normalised) == (dim, h, normalised)
        assert head.w1.dtype == head.shift.dtype == head.w2.dtype == np.float32 and head.w1.shape == (dim, dim)
        x = np.abs(np.random.RandomState(seed).randn(64, dim)) * 20.0
        err = np.abs(head.reference(x) - _unfolded64(raw, x))
        assert np.all(err <= 4 * U * _magnitude(head, x)), float((err / _magnitude(head, x)).max() / U)
    without = ssa.StructureHead(normalised=normalised, **dict(raw, out_bias=None))
    assert without.b2 == 0.0 and head.b2 == float(raw['out_bias'][0])
    assert ssa.hashing.StructureHead is ssa.StructureHead


def test_constructor_rejects_what_is_not_a_structure_branch():
    import subgraph_sketching_amd as ssa
    with pytest.raises(ValueError):
        ssa.StructureHead(**_raw_head(5, 0))                       # 5 is no h(h+2)
    with pytest.raises(ValueError):
        ssa.StructureHead(normalised=True, **_raw_head(8, 0))      # 8 is no 2 h(h+2)
    with pytest.raises(ValueError):
        ssa.StructureHead(**dict(_raw_head(8, 0), bn_mean=torch.zeros(7)))
    with pytest.raises(ValueError):
        ssa.StructureHead(**dict(_raw_head(8, 0), out_weight=torch.zeros(9)))
    with pytest.raises(ValueError):
        ssa.StructureHead(**dict(_raw_head(8, 0), weight=torch.zeros(8, 7)))


class _Model(torch.nn.Module):
    """a stand-in with the attribute names of both reference models"""

    def __init__(self, dim, extra=0, append_normalised=False, lin_in=None):
        super().__init__()
        self.dim, self.append_normalised = dim, append_normalised
        self.label_lin_layer = torch.nn.Linear(dim, dim)
        self.bn_labels = torch.nn.BatchNorm1d(dim)
        self.lin = torch.nn.Linear(dim + extra if lin_in is None else lin_in, 1)


def test_from_module_reads_the_label_branch():
    import subgraph_sketching_amd as ssa
    torch.manual_seed(7)
    m = _Model(8, extra=5)
    with torch.no_grad():
        m.bn_labels.running_mean.copy_(torch.randn(8))
        m.bn_labels.running_var.copy_(torch.rand(8) + 0.5)
        m.bn_labels.weight.copy_(torch.rand(8) + 0.5)
        m.bn_labels.bias.copy_(torch.randn(8))
    with pytest.raises(ValueError):
        ssa.StructureHead.from_module(m)                           # a fresh module is in training mode
    m.eval()
    head = ssa.StructureHead.from_module(m)
    assert head.dim == 8 and head.hops == 2 and not head.normalised
    assert np.array_equal(head.w2, m.lin.weight[0, :8].detach().numpy())   # a wider lin: only the label branch's columns
    assert head.b2 == float(m.lin.bias.detach()[0])
    x = np.abs(np.random.RandomState(0).randn(32, 8)) * 10
    raw = dict(weight=m.label_lin_layer.weight.detach(), bias=m.label_lin_layer.bias.detach(), bn_weight=m.bn_labels.weight.detach(),
               bn_bias=m.bn_labels.bias.detach(), bn_mean=m.bn_labels.running_mean, bn_var=m.bn_labels.running_var, bn_eps=m.bn_labels.eps,
               out_weight=m.lin.weight[0, :8].detach(), out_bias=m.lin.bias.detach())
    assert np.all(np.abs(head.reference(x) - _unfolded64(raw, x)) <= 4 * U * _magnitude(head, x))
    normed = _Model(16, append_normalised=True).eval()
    assert ssa.StructureHead.from_module(normed).normalised and ssa.StructureHead.from_module(normed).hops == 2
    with pytest.raises(ValueError):
        ssa.StructureHead.from_module(_Model(8, lin_in=5).eval())  # lin narrower than the label branch
    wrong = _Model(8).eval()
    wrong.dim = 15
    with pytest.raises(ValueError):
        ssa.StructureHead.from_module(wrong)                       # m.dim disagrees with the layers
    wrong = _Model(8).eval()
    wrong.bn_labels = torch.nn.BatchNorm1d(7).eval()
    with pytest.raises(ValueError):
        ssa.StructureHead.from_module(wrong)


def test_structure_head_pickles_without_device_state():
    import subgraph_sketching_amd as ssa
    head = ssa.StructureHead(**_raw_head(15, 4))
    head._dev['cuda:0'] = lambda: None  # whatever a device copy holds must not travel (and need not be picklable)
    back = pickle.loads(pickle.dumps(head))
    assert back._dev == {} and back.dim == 15 and back.hops == 3 and back.b2 == head.b2
    assert all(np.array_equal(getattr(back, k), getattr(head, k)) for k in ('w1', 'shift', 'w2'))


def test_ss_pair_scores_argument_errors_without_a_gpu():
    """argument validation happens on the host before any launch (fake pointers are never dereferenced)"""
    import subgraph_sketching_amd as ssa
    N = ssa._native
    lib = N.lib()
    fake = c_void_p(8)
    prm = N.HllParams(p=8, n_tbl=200, alpha_mm=1.0, threshold=1.0, lc_min_zeros=1, reserved=0, raw_est=8, bias=8, lc_table=8)
    ptrs = (c_void_p * 3)(8, 8, 8)

    def head(dim, normalised=0):
        return N.StructureHeadStruct(dim=dim, normalised=normalised, w1=8, shift=8, w2=8, bias=0.0)

    def call(B=4, h=2, hd=head(8), out=fake, degrees=None, links=fake, params=prm):
        return lib.ss_pair_scores(links, None, B, 100, h, ptrs, 128, ptrs, fake, h, byref(params) if params is not None else None, 0, degrees,
                                  byref(hd) if hd is not None else None, out, None, None)

    assert call(h=4) == -4 and call(h=0) == -4                      # no kernel for that hop count
    assert lib.ss_pair_scores(None, None, 0, 0, 4, None, 128, None, None, 0, None, 0, None, None, None, None, None) == -4
    assert call(B=0) == 0 and call(B=0, hd=None, out=None) == 0     # nothing to do
    assert call(hd=None) == -1 and call(out=None) == -1 and call(links=None) == -1 and call(params=None) == -1
    assert call(B=-1) == -1
    assert call(hd=head(15)) == -1 and call(h=3, hd=head(8)) == -1  # dim against h
    assert call(hd=head(16, 0)) == -1 and call(hd=head(8, 1)) == -1  # dim against normalised
    assert call(hd=head(16, 1)) == -1                               # normalised without degrees
    assert call(hd=head(8, 0), degrees=fake) == -1                  # degrees without normalised
    assert call(hd=N.StructureHeadStruct(dim=8, normalised=0, w1=None, shift=8, w2=8, bias=0.0)) == -1


def test_score_links_without_the_library_fails_loudly(monkeypatch):
    import subgraph_sketching_amd as ssa
    head = ssa.StructureHead(**_raw_head(8, 1))
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    table = {k: {'minhash': torch.zeros((4, 128), dtype=torch.int64), 'hll': torch.zeros((4, 256), dtype=torch.int8)} for k in range(3)}
    monkeypatch.setattr(ssa._native, '_lib', None)
    monkeypatch.setattr(ssa._native, 'LIB_PATH', '/nonexistent/libsubgraph_sketch.so')
    with pytest.raises(ssa._native.NativeLibraryMissing):
        eh.score_links(torch.zeros((3, 2), dtype=torch.int64), table, torch.zeros((4, 2)), head)


def test_score_links_argument_checks_need_no_device():
    import subgraph_sketching_amd as ssa
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
    links, cards = torch.zeros((3, 2), dtype=torch.int64), torch.zeros((4, 2))
    with pytest.raises(ValueError):
        eh.score_links(links, {}, cards, ssa.StructureHead(**_raw_head(15, 1)))                         # a 3-hop head on a 2-hop engine
    with pytest.raises(ValueError):
        eh.score_links(links, {}, cards, ssa.StructureHead(normalised=True, **_raw_head(16, 1)))        # normalised without degrees
    with pytest.raises(ValueError):
        eh.score_links(links, {}, cards, ssa.StructureHead(**_raw_head(8, 1)), degrees=torch.ones(4))   # degrees without normalised
    with pytest.raises(ValueError):
        eh.score_links(links, {}, cards, ssa.StructureHead(**_raw_head(8, 1)), mask_target=torch.zeros((2, 0), dtype=torch.int64))
    with pytest.raises(ValueError):
        eh.score_links(links, {}, cards, ssa.StructureHead(**_raw_head(8, 1)), lazy=True)
    with pytest.raises(ValueError):
        eh.score_links(links, {}, cards, object())
