"""ElphHashes.topk_links without a GPU: the argument checks that run before anything is launched, the byte model of its scan
(roofline.topk_links_bytes) against a hand count, and the new entry point in the header, the bindings and the library."""
from argparse import Namespace
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
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
OK = torch.tensor([0, 1])


@pytest.mark.parametrize('k', [0, -1, 31])
def test_k_out_of_range(k):
    with pytest.raises(ValueError):
        _eh().topk_links(OK, _table(), CARDS, k, _head())


@pytest.mark.parametrize('bad', [[0, 30], [-31], [29, 100]])
def test_cpu_sources_out_of_range(bad):
    with pytest.raises(IndexError):
        _eh().topk_links(torch.tensor(bad), _table(), CARDS, 5, _head())


@pytest.mark.parametrize('bad', [[[0], [30]], [[-31], [1]]])
def test_cpu_exclude_out_of_range(bad):
    with pytest.raises(IndexError):
        _eh().topk_links(torch.tensor([0, -30]), _table(), CARDS, 5, _head(), exclude=torch.tensor(bad))


def test_malformed_inputs():
    eh = _eh()
    with pytest.raises(ValueError):
        eh.topk_links(torch.tensor([[0, 1]]), _table(), CARDS, 5, _head())
    with pytest.raises(ValueError):
        eh.topk_links(torch.tensor([0.0]), _table(), CARDS, 5, _head())
    with pytest.raises(ValueError):
        eh.topk_links(torch.tensor([0]), _table(), CARDS, 5, _head(), exclude=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError):
        eh.topk_links(OK, _table(), None, 5, _head())


def test_the_head_must_fit_the_engine_and_the_degrees():
    eh = _eh()
    with pytest.raises(ValueError, match='max_hash_hops'):
        eh.topk_links(OK, _table(), CARDS, 5, _head(h=3))
    with pytest.raises(ValueError, match='max_hash_hops'):
        _eh(h=3).topk_links(OK, _table(h=3), torch.zeros((30, 3)), 5, _head(h=2, normalised=True))
    with pytest.raises(ValueError, match='degrees'):
        eh.topk_links(OK, _table(), CARDS, 5, _head(normalised=True))
    with pytest.raises(ValueError, match='degrees'):
        eh.topk_links(OK, _table(), CARDS, 5, _head(), degrees=torch.ones(30))
    for not_a_head in (raw_head(8, 1), None, torch.nn.Linear(8, 1)):
        with pytest.raises(ValueError, match='StructureHead'):
            eh.topk_links(OK, _table(), CARDS, 5, not_a_head)


@pytest.mark.parametrize('P', [6, 2052])
def test_unsupported_sketch_shape(P):
    with pytest.raises(NotImplementedError):
        _eh(P=P).topk_links(torch.tensor([0]), _table(P=P), CARDS, 5, _head())


def test_byte_model_against_a_hand_count():
    from subgraph_sketching_amd import roofline
    # N = 1 000, S = 40, h = 2, P = 128, M = 256.  A row is 4 * 128 + 256 = 768 B.  LDS per source: 8 (id) + 8 (cards) + 4 (degree)
    # + 2 hops * (512 B of MinHash + 16 chunks * 36 B of digest) = 2 196 B; 32 sources need 70 272 + 12 100 B > 80 KiB, 16 fit.
    assert roofline.topk_links_sources(2, 128, 256) == 16
    # 3 blocks of sources: candidates 3 * 1 000 * 2 * 768 = 4 608 000; the launch has min(ceil(4096 / 3), ceil(1000 / 16)) = 63
    # workgroups per block, each staging its sources: 63 * 40 * 2 * 768 = 3 870 720; keys 8 * 40 * 1 000 = 320 000
    assert roofline.topk_links_bytes(1000, 40, 2, 128, 256) == 4608000 + 3870720 + 320000
    # the other block sizes: one hop fits 32 sources, three hops of P = 256 only 8; the run-time-size path stages no rows
    assert roofline.topk_links_sources(1, 256, 256) == 32
    assert roofline.topk_links_sources(3, 128, 256) == 16
    assert roofline.topk_links_sources(3, 256, 256) == 8
    assert roofline.topk_links_sources(3, 192, 64) == 32
    # collab size, S = 1 024: every candidate row moves once per 16 sources, not once per pair
    n, s = 235868, 1024
    assert roofline.topk_links_bytes(n, s, 2, 128, 256) < roofline.score_query_bytes(n * s, h=2) / 25


def test_the_entry_point_is_declared_bound_and_exported():
    import subgraph_sketching_amd as ssa
    text = open(os.path.join(REPO, 'include', 'subgraph_sketch.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+ss_topk_score_scan\s*\(', text)
    restype, argtypes = ssa._native.SIGNATURES['ss_topk_score_scan']
    assert restype is ctypes.c_int32 and len(argtypes) == 17
    assert os.path.exists(ssa._native.LIB_PATH), 'run `python __graft_entry__.py` first (build())'
    assert hasattr(ctypes.CDLL(ssa._native.LIB_PATH), 'ss_topk_score_scan')
    assert callable(getattr(ssa.ElphHashes, 'topk_links'))


def test_argument_errors_are_reported_without_a_gpu():
    """the host-side checks of ss_topk_score_scan run before any launch"""
    from ctypes import byref, c_void_p
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(8)  # never dereferenced
    ptrs = (c_void_p * 2)(8, 8)
    good = ssa._native.StructureHeadStruct(dim=8, normalised=0, w1=8, shift=8, w2=8, bias=0.0)
    assert lib.ss_topk_score_scan(fake, 2, 30, 4, ptrs, ptrs, 128, fake, 2, None, 0, None, byref(good), fake, 480, None, None) == -4  # h = 4
    assert lib.ss_topk_score_scan(fake, 2, 30, 2, ptrs, ptrs, 128, fake, 2, None, 0, None, byref(good), fake, 480, None, None) == -1  # no parameters
