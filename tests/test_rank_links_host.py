"""ElphHashes.rank_links without a GPU: the numpy restatement of its definition on a hand-made example, the argument checks that run
before anything is launched (rank_links' own and ss_rank_score_scan's), the byte model of the scan (roofline.rank_links_bytes) against
a hand count, and the new entry point in the header, the bindings and the library."""
from argparse import Namespace
import ctypes
from ctypes import byref, c_void_p
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from rank_restatement import rank_counts, tied_below
from score_restatement import raw_head


def _eh(h=2, P=128, p=8):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))


def _table(N=30, P=128, p=8, h=2):
    return {k: {'minhash': torch.zeros((N, P), dtype=torch.int64), 'hll': torch.zeros((N, 1 << p), dtype=torch.int8)}
            for k in range(h + 1)}


def _head(h=2, normalised=False):
    import subgraph_sketching_amd as ssa
    nf = h * (h + 2)
    return ssa.StructureHead(normalised=normalised, **raw_head(2 * nf if normalised else nf, 1))


CARDS = torch.zeros((30, 2))
OK = torch.tensor([[0, 1], [2, -30]])


def test_the_restatement_on_a_hand_made_example():
    """5 nodes, scores with ties (one of them -0.0 against +0.0), an exclusion given twice, a self loop in it, an excluded target"""
    S = np.array([[9, 1, 2, 2, 3],
                  [0, 9, 0, 0, 0],
                  [0.0, 4, 9, -1, -0.0],
                  [7, 7, 7, 7, 7],
                  [1, 2, 3, 4, 5]], dtype=np.float32)
    row = lambda q, u: S[u]
    links = np.array([[0, 2], [1, 1], [2, -1], [3, 0], [-1, 0]])
    # (0, 2): thr 2, candidates {1, 3, 4} = 1, 2, 3;  (1, 1): thr 9, candidates {0, 2, 3, 4} all 0;  (2, 4): thr -0.0, candidates
    # {0, 1, 3} = +0.0, 4, -1;  (3, 0): thr 7, candidates {1, 2, 4} all 7;  (4, 0): thr 1, candidates {1, 2, 3} = 2, 3, 4
    g, e = rank_counts(row, links, 5)
    assert g.tolist() == [1, 0, 1, 0, 3] and e.tolist() == [1, 0, 1, 3, 0]
    assert tied_below(row, links, 5).tolist() == [0, 0, 1, 0, 0]
    # exclude: 0 -> 4 twice, the self loop 0 -> 0, the target 0 -> 2 (immune), 2 -> 1, 3 -> 2 given as 3 -> -3, 4 -> 0 (the target)
    ex = np.array([[0, 0, 0, 0, 2, 3, 4], [4, 4, 0, 2, 1, -3, 0]])
    g, e = rank_counts(row, links, 5, ex)
    assert g.tolist() == [0, 0, 0, 0, 3] and e.tolist() == [1, 0, 1, 2, 0]
    clean = np.array([[0, 2, 3], [4, 1, 2]])
    assert [a.tolist() for a in rank_counts(row, links, 5, clean)] == [g.tolist(), e.tolist()]


@pytest.mark.parametrize('bad', [[[0, 30]], [[-31, 0]], [[1, 2], [29, 100]]])
def test_cpu_links_out_of_range(bad):
    with pytest.raises(IndexError):
        _eh().rank_links(torch.tensor(bad), _table(), CARDS, _head())


@pytest.mark.parametrize('bad', [[[0], [30]], [[-31], [1]]])
def test_cpu_exclude_out_of_range(bad):
    with pytest.raises(IndexError):
        _eh().rank_links(OK, _table(), CARDS, _head(), exclude=torch.tensor(bad))


def test_malformed_inputs():
    eh = _eh()
    with pytest.raises(ValueError):
        eh.rank_links(torch.tensor([[0, 1, 2]]), _table(), CARDS, _head())
    with pytest.raises(ValueError):
        eh.rank_links(torch.tensor([0, 1, 2]), _table(), CARDS, _head())
    with pytest.raises(ValueError):
        eh.rank_links(torch.tensor([[0.0, 1.0]]), _table(), CARDS, _head())
    with pytest.raises(ValueError):
        eh.rank_links(OK, _table(), CARDS, _head(), exclude=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError):
        eh.rank_links(OK, _table(), None, _head())
    with pytest.raises(ValueError, match='mask_target'):
        eh.rank_links(OK, _table(), CARDS, _head(), mask_target=torch.zeros((2, 0), dtype=torch.int64))
    with pytest.raises(ValueError, match='lazy'):
        eh.rank_links(OK, _table(), CARDS, _head(), lazy=True)


def test_the_head_must_fit_the_engine_and_the_degrees():
    eh = _eh()
    with pytest.raises(ValueError, match='max_hash_hops'):
        eh.rank_links(OK, _table(), CARDS, _head(h=3))
    with pytest.raises(ValueError, match='degrees'):
        eh.rank_links(OK, _table(), CARDS, _head(normalised=True))
    with pytest.raises(ValueError, match='degrees'):
        eh.rank_links(OK, _table(), CARDS, _head(), degrees=torch.ones(30))
    for not_a_head in (raw_head(8, 1), None, torch.nn.Linear(8, 1)):
        with pytest.raises(ValueError, match='StructureHead'):
            eh.rank_links(OK, _table(), CARDS, not_a_head)


@pytest.mark.parametrize('P', [6, 2052])
def test_unsupported_sketch_shape(P):
    with pytest.raises(NotImplementedError):
        _eh(P=P).rank_links(OK, _table(P=P), CARDS, _head())


def test_no_links_need_no_device():
    g, e = _eh().rank_links(torch.zeros((0, 2), dtype=torch.int64), _table(), CARDS, _head())
    assert g.shape == (0,) and e.shape == (0,) and g.dtype == torch.int64 and e.dtype == torch.int64


def test_byte_model_against_a_hand_count():
    from subgraph_sketching_amd import roofline
    # N = 1 000, L = 40, h = 2, P = 128, M = 256.  A row is 768 B.  LDS per link: 16 (ids) + 8 (cards) + 4 (degree) + 4 (threshold)
    # + 8 (sums) + 2 hops * 1 088 B = 2 216 B; 32 links need 70 912 + 12 100 B > 80 KiB, 16 fit.
    assert roofline.rank_links_queries(2, 128, 256) == 16
    # 3 blocks of links: candidates 3 * 1 000 * 2 * 768 = 4 608 000; 63 workgroups per block, each staging its links' source rows,
    # the link and the threshold: 63 * 40 * (2 * 768 + 20) = 3 921 120; counts 16 * 40 = 640
    assert roofline.rank_links_bytes(1000, 40, 2, 128, 256) == 4608000 + 3921120 + 640
    # the staged block of every instantiation is the head scan's: the 20 extra bytes move none of them
    for h in (1, 2, 3):
        for P, M in ((64, 256), (128, 256), (192, 256), (256, 256), (192, 64), (8, 16)):
            assert roofline.rank_links_queries(h, P, M) == roofline.topk_links_sources(h, P, M)
    # what is written does not grow with N: the keys of topk_links do
    n, s = 235868, 1024
    assert roofline.topk_links_bytes(n, s, 2, 128, 256) - roofline.rank_links_bytes(n, s, 2, 128, 256) > 8 * s * n - (1 << 22)


def test_the_entry_point_is_declared_bound_and_exported():
    import subgraph_sketching_amd as ssa
    text = open(os.path.join(REPO, 'include', 'subgraph_sketch.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+ss_rank_score_scan\s*\(', text)
    restype, argtypes = ssa._native.SIGNATURES['ss_rank_score_scan']
    assert restype is ctypes.c_int32 and len(argtypes) == 17
    assert os.path.exists(ssa._native.LIB_PATH), 'run `python __graft_entry__.py` first (build())'
    assert hasattr(ctypes.CDLL(ssa._native.LIB_PATH), 'ss_rank_score_scan')
    assert callable(getattr(ssa.ElphHashes, 'rank_links'))
    assert ssa.engine._RANK_LAUNCH_LINKS == 8 * 65535  # what one launch's grid.y takes at the smallest staged block


def test_argument_errors_are_reported_without_a_gpu():
    """the host-side checks of ss_rank_score_scan run before any launch (fake pointers are never dereferenced)"""
    import subgraph_sketching_amd as ssa
    N = ssa._native
    lib = N.lib()
    fake = c_void_p(8)
    prm = N.HllParams(p=8, n_tbl=200, alpha_mm=1.0, threshold=1.0, lc_min_zeros=1, reserved=0, raw_est=8, bias=8, lc_table=8)
    ptrs = (c_void_p * 3)(8, 8, 8)
    holes = (c_void_p * 3)(8, None, 8)

    def head(dim, normalised=0):
        return N.StructureHeadStruct(dim=dim, normalised=normalised, w1=8, shift=8, w2=8, bias=0.0)

    def call(L=4, h=2, hd=head(8), links=fake, thr=fake, mh=ptrs, hll=ptrs, cards=fake, stride=None, params=prm, degrees=None, counts=fake,
             n=100):
        return lib.ss_rank_score_scan(links, thr, L, n, h, mh, hll, 128, cards, h if stride is None else stride,
                                      byref(params) if params is not None else None, 0, degrees, byref(hd) if hd is not None else None,
                                      counts, None, None)

    assert call(h=4) == -4 and call(h=0) == -4                         # no kernel for that hop count
    assert call(params=None) == -1
    assert call(L=0) == 0 and call(L=0, links=None, thr=None, counts=None, hd=None) == 0   # nothing to do
    assert call(L=-1) == -1 and call(n=0) == -1 and call(n=1 << 32) == -1
    assert call(links=None) == -1 and call(thr=None) == -1 and call(counts=None) == -1 and call(cards=None) == -1
    assert call(mh=None) == -1 and call(hll=None) == -1 and call(mh=holes) == -1 and call(hll=holes) == -1
    assert call(stride=1) == -1 and call(h=3, hd=head(15), stride=2) == -1   # cards_stride < h
    assert call(hd=None) == -1
    assert call(hd=head(15)) == -1 and call(h=3, hd=head(8)) == -1     # dim against h
    assert call(hd=head(16, 0)) == -1 and call(hd=head(8, 1)) == -1    # dim against normalised
    assert call(hd=head(16, 1)) == -1                                  # normalised without degrees
    assert call(hd=head(8, 0), degrees=fake) == -1                     # degrees without normalised
    assert call(L=8 * 65535 + 1) == -1                                 # more links than one launch's grid.y takes
