"""The contract the link kernels share, in one place: pair_features_kernel, pair_features_runs_kernel, topk_score_scan_kernel,
topk_scan_kernel and masked_pairs_kernel give the same bits for the same pair (csrc/ss_pair_math.hpp).  Every assertion compares one
entry point of the library with ANOTHER one (or with float32 torch), never a code path with itself, on a graph small enough for
seconds: 300 nodes, three of them given degree 0, 2 000 links with negative ids, u == v and two ids out of range, for h = 1 .. 3 on the
four compile-time shapes (P = 64, 128, 192, 256 at p = 8) and on a run-time shape with fewer MinHash chunks than lanes (P = 36,
p = 6): every branch of the one shape dispatcher (dispatch_pair_shape), through every entry point."""
from argparse import Namespace
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

from score_restatement import raw_head

pytestmark = pytest.mark.gpu

N, L = 300, 2000
SHAPES = [(128, 8), (36, 6), (64, 8), (192, 8), (256, 8)]
FAST = [(P, p) for P, p in SHAPES if p == 8 and P in (64, 128, 192, 256)]  # the shapes with compile-time kernels (run-aware: these only)


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _eh(ssa, h, P, p):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    eh.hll_tables = ssa.hll_tables.load(eh.p, prefer='regenerated')
    eh.strict_bounds = False
    return eh


@pytest.fixture(scope='module')
def world(ssa, dev):
    """per sketch shape: the 3-hop tables, built once and left unchanged; the graph, the links and the degrees are shared"""
    rng = np.random.RandomState(23)
    e = rng.randint(0, N, size=(2, 750)).astype(np.int64)
    ei = np.concatenate([e, e[::-1]], axis=1)  # ~1 500 directed edges
    links = rng.randint(0, N, size=(L, 2)).astype(np.int64)
    links[:200] = ei[:, :200].T           # links that are edges (the masked kernel's work)
    links[5::100] -= N                    # torch-style negative ids
    links[11::250, 1] = links[11::250, 0]  # u == v
    links[17, 0] = N + 3                  # out of range: NaN rows
    links[1203, 1] = -N - 1
    deg = np.bincount(ei[0], minlength=N).astype(np.float32)
    deg[[3, 150, N - 2]] = 0.0
    out = {'ei': torch.from_numpy(ei).to(dev), 'links': torch.from_numpy(links).to(dev), 'deg': torch.from_numpy(deg).to(dev),
           'edge_keys': set((ei[0] * N + ei[1]).tolist())}
    for P, p in SHAPES:
        out[(P, p)] = _eh(ssa, 3, P, p).build_hash_tables(N, out['ei'])
    return out


def _bits(x):
    """NaN mapped to a constant, so that torch.equal compares rows with NaN"""
    return torch.nan_to_num(x.float(), nan=-12345.0, posinf=3e38, neginf=-3e38)


def _case(ssa, world, h, shape):
    table, cards = world[shape]
    return _eh(ssa, h, *shape), {k: table[k] for k in range(h + 1)}, cards[:, :h].contiguous()


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('h', [1, 2, 3])
def test_grouped_kernels_and_the_normalised_half(ssa, dev, world, h, shape):
    eh, table, cards = _case(ssa, world, h, shape)
    links, deg = world['links'], world['deg']
    nf = h * (h + 2)
    plain = eh.get_subgraph_features(links, table, cards)
    normed = eh.get_subgraph_features(links, table, cards, degrees=deg)
    assert int(torch.isnan(plain).any(dim=1).sum()) == 2
    # 2. first half: the plain row; second half: row / sqrt(d_u d_v), NaN / Inf -> 0, in float32 torch (out of range: NaN stays)
    assert torch.equal(_bits(normed[:, :nf]), _bits(plain))
    u, v = links[:, 0] % N, links[:, 1] % N
    bad = torch.isnan(plain).any(dim=1)
    want = plain / torch.sqrt(deg[u] * deg[v]).unsqueeze(1)
    want = torch.where(torch.isnan(want) | torch.isinf(want), torch.zeros_like(want), want)
    want[bad] = float('nan')
    assert torch.equal(_bits(normed[:, nf:]), _bits(want))
    assert bool((normed[~bad][:, nf:] == 0).all(dim=1).any()), 'a zero-degree endpoint must occur'
    # 1. both kernels behind ss_pair_features_grouped_kernel, with and without an order (run-aware: compile-time shape only)
    lib, H = ssa._native.lib(), ssa.hashing
    prm = eh._params(dev)
    mh_ptrs = (c_void_p * h)(*[table[k].mh_u32.data_ptr() for k in range(1, h + 1)])
    hl_ptrs = (c_void_p * h)(*[table[k].hll_u8.data_ptr() for k in range(1, h + 1)])
    order = H.group_links_by_source(links, N, dev).to(torch.int32).contiguous()
    for which in ((0, 1) if shape in FAST else (0,)):
        for o in (order, None):
            for dg, ref in ((None, plain), (deg, normed)):
                out = torch.full_like(ref, 7.0)
                rc = lib.ss_pair_features_grouped_kernel(which, H._ptr(links), H._ptr(o), L, N, h, mh_ptrs, shape[0], hl_ptrs, H._ptr(cards), cards.stride(0),
                                                         byref(prm.struct), ssa._native.SS_FLAG_USE_ZERO_ONE, H._ptr(dg), H._ptr(out), None, H._stream(dev))
                assert rc == 0
                assert torch.equal(_bits(out), _bits(ref)), (which, o is not None, dg is not None)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('h', [1, 2, 3])
def test_scans_equal_the_pair_queries(ssa, dev, world, h, shape):
    """3. topk_links(k = N) == score_links on the explicit pairs; topk_candidates(k = N, hops) == _get_intersections"""
    eh, table, cards = _case(ssa, world, h, shape)
    deg = world['deg']
    nf = h * (h + 2)
    sources = torch.tensor([0, 3, 77, 150, N - 1], device=dev)  # 3 and 150 have degree 0
    pairs = torch.stack([sources.repeat_interleave(N), torch.arange(N, device=dev).repeat(len(sources))], dim=1)
    for normalised in (False, True):
        head = ssa.StructureHead(normalised=normalised, **raw_head(2 * nf if normalised else nf, 5))
        dg = deg if normalised else None
        ids, scores = eh.topk_links(sources, table, cards, N, head, degrees=dg)
        want = eh.score_links(pairs, table, cards, head, degrees=dg).reshape(len(sources), N)
        live = ids >= 0
        assert int(live.sum()) == len(sources) * (N - 1)
        assert torch.equal(scores[live] + 0.0, torch.gather(want, 1, ids.clamp(min=0))[live] + 0.0)
    k1, k2 = h, 1
    ids, scores = eh.topk_candidates(sources, table, N, hops=(k1, k2))
    want = eh._get_intersections(pairs, table)[(k1, k2)].reshape(len(sources), N)
    live = ids >= 0
    assert int(live.sum()) == len(sources) * (N - 1)
    assert torch.equal(scores[live] + 0.0, torch.gather(want, 1, ids.clamp(min=0))[live] + 0.0)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('h', [1, 2, 3])
def test_masked_rows_of_non_edges_are_the_plain_rows(ssa, dev, world, h, shape):
    """4. the masked query on links that are not edges: the plain rows and the plain query's match / zeros"""
    eh, table, cards = _case(ssa, world, h, shape)
    links = world['links']
    got, dbg = eh.get_subgraph_features(links, table, cards, mask_target=world['ei'], return_debug=True)
    plain, pdbg = eh._pair_kernel(links, table, cards, want_debug=True)
    lk = links.cpu().numpy()
    ok = ((lk >= -N) & (lk < N)).all(axis=1)
    u, v = lk[:, 0] % N, lk[:, 1] % N
    edge = np.array([bool(o) and ((a * N + b) in world['edge_keys'] or (b * N + a) in world['edge_keys']) and a != b
                     for o, a, b in zip(ok, u, v)])
    assert np.array_equal(dbg['masked'].cpu().numpy().astype(bool), edge) and 150 < edge.sum() < L // 2
    keep = torch.from_numpy(~edge).to(dev)
    assert torch.equal(_bits(got[keep]), _bits(plain[keep]))
    in_range = torch.from_numpy(~edge & ok).to(dev)  # (the debug integers of an out-of-range link are those of node 0 in both)
    assert torch.equal(dbg['match'][in_range], pdbg['match'][in_range]) and torch.equal(dbg['zeros'][in_range], pdbg['zeros'][in_range])
