"""The fused stage (ss_fused_hop_stage: hop-1 MinHash + hop-2 HLL in one launch) against the unfused sequence (ss_first_hop +
ss_propagate, what SS_FUSED_STAGE=0 runs) on graphs whose rows are planted where the kernel's posts branch: `total` (the neighbours a
row folds) on either side of the 7 register landings, of the 7 LDS landings and of the 32 neighbours a lane group walks alone; short
and long rows side by side in one chunk of four; a last chunk and a last lane group that are partial; a row left to the hub pass whose
neighbours still fetch it; an isolated last node beyond the inferred self loops (the all-zero row); rows that list themselves; a
symmetric edge list (the rows skip their own row) and a one-directional one (they keep it).  Both forms of the posts -- through the
buffer descriptor and with flat addresses (SS_FUSED_POSTS) -- at P = 64 and P = 128, p = 8.  Everything is compared bit for bit."""
from argparse import Namespace
from ctypes import byref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 67          # not a multiple of 4 (rows per wavefront) or 16 (rows per workgroup)
FIRST_FILLER = 24
# in-degrees of the planted rows 0 .. 23, a short row next to a long one in every chunk of four.  A row folds `total` = in-degree + 1
# neighbours where it keeps its own row (one-directional list) and in-degree where it skips it (symmetric list, in-degree > 0)
DEGREES = [1, 33, 6, 31, 7, 16, 0, 32, 8, 15, 3, 30, 14, 5, 12, 33, 2, 14, 7, 13, 32, 6, 15, 8]
TOTALS = {1, 6, 7, 8, 13, 14, 15, 16, 31, 32, 33}  # planted in both kinds of list; 0 is the isolated last node
HUB_THRESHOLD = 40


def planted_edges(symmetric, self_edges=False, hub=False):
    """edges filler -> planted row (rows 24 .. 65 are fillers, node 66 occurs in no edge); symmetric: and back"""
    src, dst = [], []
    n_fill = N - 1 - FIRST_FILLER
    for i, d in enumerate(DEGREES):
        for k in range(d):
            src.append(FIRST_FILLER + (5 * i + k) % n_fill)
            dst.append(i)
    ei = np.array([src, dst], dtype=np.int64)
    if hub:  # every other node but the last points at filler 30: a row above the hub threshold that rows 0 .. 65 may fetch
        others = np.array([j for j in range(N - 1) if j != 30], dtype=np.int64)
        ei = np.concatenate([ei, np.stack([others, np.full_like(others, 30)]), np.stack([np.full(6, 30), np.arange(6)])], axis=1)
    if symmetric:
        ei = np.concatenate([ei, ei[::-1]], axis=1)
    else:
        ei = np.concatenate([ei, np.array([[0], [N - 2]], dtype=np.int64)], axis=1)  # (the inferred self loops reach node 65)
    if self_edges:  # rows that list themselves: a short one, a long one, a filler
        loops = np.array([2, 3, 9, 40], dtype=np.int64)
        ei = np.concatenate([ei, np.stack([loops, loops])], axis=1)
    return np.ascontiguousarray(ei)


def row_totals(ei, symmetric):
    deg = np.bincount(ei[1], minlength=N)
    n_self = int(ei.max()) + 1
    own = (np.arange(N) < n_self) & ~((deg > 0) & symmetric)
    return deg + own, n_self


VARIANTS = {
    'symmetric': dict(symmetric=True), 'one_directional': dict(symmetric=False),
    'symmetric_self_edges': dict(symmetric=True, self_edges=True), 'one_directional_self_edges': dict(symmetric=False, self_edges=True),
    'symmetric_hub': dict(symmetric=True, hub=True), 'one_directional_hub': dict(symmetric=False, hub=True),
}


def test_the_graphs_plant_what_they_claim():
    for name in ('symmetric', 'one_directional'):
        ei = planted_edges(**VARIANTS[name])
        totals, n_self = row_totals(ei, VARIANTS[name]['symmetric'])
        assert n_self == N - 1 and totals[N - 1] == 0
        assert TOTALS <= set(totals[:FIRST_FILLER].tolist()), name
        for q in range(0, FIRST_FILLER, 4):  # a short and a long row in every chunk
            assert totals[q:q + 4].min() <= 8 and totals[q:q + 4].max() >= 13
    for name in ('symmetric_hub', 'one_directional_hub'):
        deg = np.bincount(planted_edges(**VARIANTS[name])[1], minlength=N)
        assert deg[30] > HUB_THRESHOLD and (np.delete(deg, 30) <= HUB_THRESHOLD).all()
    ei = planted_edges(symmetric=True, self_edges=True)
    assert ((ei[0] == ei[1]) & (ei[0] == 3)).any()


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, P, **kw):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=P, floor_sf=False, use_zero_one=True), **kw)
    eh.hll_tables = ssa.hll_tables.load(8, prefer='regenerated')
    return eh


_unfused = {}


def unfused(ssa, dev, name, P):
    """ss_first_hop + ss_propagate, once per graph and P"""
    if (name, P) not in _unfused:
        ei = torch.from_numpy(planted_edges(**VARIANTS[name])).to(dev)
        table, cards = _eh(ssa, P, fuse_hop_stage=False).build_hash_tables(N, ei)
        torch.cuda.synchronize()
        _unfused[(name, P)] = (table[1].mh_u32.clone(), table[1].hll_u8.clone(), table[2].mh_u32.clone(), table[2].hll_u8.clone(), cards.clone())
    return _unfused[(name, P)]


def fused(ssa, dev, name, P):
    """ss_fused_hop_stage on the same graph; hop-2 MinHash is part of the stage at P = 128 only"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    eh = _eh(ssa, P)
    ei = torch.from_numpy(planted_edges(**VARIANTS[name])).to(dev)
    csr = ssa.hashing.build_csr(ei, N, dev, check=False)
    csr.use_inferred_self_loops = True
    graph = csr.struct()
    ab, params = eh._perms(dev), eh._params(dev)
    mh = [torch.full((N, P), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    hll = [torch.full((N, 256), 255, dtype=torch.uint8, device=dev) for _ in range(2)]
    cards = torch.full((N, 2), -1.0, dtype=torch.float32, device=dev)
    rc = ssa._native.lib().ss_fused_hop_stage(byref(graph), _ptr(ab[0]), _ptr(ab[1]), P, _ptr(mh[0]), _ptr(mh[1]) if P == 128 else None, 8,
                                              _ptr(hll[0]), _ptr(cards), _ptr(hll[1]), _ptr(cards[:, 1]), 2, byref(params.struct),
                                              _stream(dev))
    assert rc == 0, f'ss_fused_hop_stage returned {rc}'
    torch.cuda.synchronize()
    return mh[0], hll[0], mh[1], hll[1], cards


@pytest.mark.parametrize('posts', ['buffer', 'flat'])
@pytest.mark.parametrize('P', [64, 128])
@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_fused_stage_equals_the_unfused_sequence(ssa, dev, monkeypatch, name, P, posts):
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', HUB_THRESHOLD)
    monkeypatch.delenv('SS_FUSED_POSTS', raising=False)
    monkeypatch.delenv('SS_SELF_SKIP', raising=False)
    want = unfused(ssa, dev, name, P)
    monkeypatch.setenv('SS_FUSED_POSTS', posts)
    got = fused(ssa, dev, name, P)
    assert torch.equal(got[0], want[0]), 'hop-1 MinHash'
    assert torch.equal(got[1], want[1]), 'hop-1 HLL'
    assert torch.equal(got[3], want[3]), 'hop-2 HLL'
    assert torch.equal(got[4].view(torch.int32), want[4].view(torch.int32)), 'cards of hops 1 and 2'
    if P == 128:
        assert torch.equal(got[2], want[2]), 'hop-2 MinHash'
    assert not got[3][N - 1].any() and not got[0][N - 1].any(), 'the isolated last node is the all-zero row'
    assert got[3][:N - 1].any(dim=1).all(), 'every other row has folded something'
