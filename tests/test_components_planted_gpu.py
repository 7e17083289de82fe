"""The entry points of csrc/ss_components.hip launched directly on the plans of tests/components_planted.py: ss_components_sizes on
label arrays built wavefront by wavefront (the peel at 1, 2, 4, 5 and 64 labels, a first leader at lane 63, one live lane; N = 3 chunks
+ 257, chunk - 1 / chunk / chunk + 1, 63 / 64 / 65), ss_components_roots on sizes of the test's choosing with the winner of the key at
chosen lanes, wavefronts, tiles and chunks and in ties, ss_induced_select by planted keys and by mask bytes 0, 1, 2, 0x80, 0xFF,
ss_induced_mapper on unsorted lists with duplicates and ids out of range, ss_induced_edges on a planted mapper, ss_components_same.
Every comparison is exact integer equality of whole arrays with the plan's numpy answer, and every output sits between guard words
that must keep their sentinel: a launch writes its own places and nothing else.  What the plans reach, and which wrong kernels they
tell from the right one, is pinned by tests/test_components_planted_host.py; what ran on an MI355X: profiles/components_planted_tests.txt."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import components_planted as P

pytestmark = pytest.mark.gpu

GUARD = 64  # words on either side of every output
SENTINEL = {torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}  # no count, id, rank or key of these plans


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    assert m._native.COMPONENTS_CHUNK == P.CHUNK
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


class Guarded(object):
    """`size` output words (possibly none) between two rows of GUARD sentinel words"""

    def __init__(self, size, dtype, dev, what):
        self.size, self.what = size, what
        self.buf = torch.full((size + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=dev)

    @property
    def ptr(self):
        return c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def result(self):
        """the output words as numpy, after the check that both guard rows kept the sentinel"""
        host = self.buf.cpu().numpy()
        fill = SENTINEL[self.buf.dtype]
        assert (host[:GUARD] == fill).all() and (host[GUARD + self.size:] == fill).all(), f'a store left {self.what}'
        return host[GUARD:GUARD + self.size]


def _to(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the planted arrays are read-only)


def _call(ssa, dev, name, *args):
    from subgraph_sketching_amd._runtime import _ptr, _stream
    args = [a.ptr if isinstance(a, Guarded) else _ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    ssa._native.check(getattr(ssa._native.lib(), name)(*args, _stream(dev)), name)
    torch.cuda.synchronize(dev)


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,first', P.label_plans())
def test_sizes_equal_the_count_of_every_label(ssa, dev, N, first):
    plan = P.label_plan(N, first)
    P.check_labels(plan.label, N)  # the kernel indexes size[label[x]]
    size = Guarded(N, torch.int32, dev, 'size')
    block_roots = Guarded(len(plan.block_roots), torch.int32, dev, 'block_roots')
    _call(ssa, dev, 'ss_components_sizes', _to(dev, plan.label), N, size, block_roots)
    np.testing.assert_array_equal(size.result(), np.bincount(plan.label, minlength=N), err_msg=f'size, patterns {plan.names[:12]}')
    np.testing.assert_array_equal(block_roots.result(), P.chunk_counts(plan.label == np.arange(N)), err_msg='block_roots')


# ---- 2. roots ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', P.ROOTS_CASES)
def test_roots_sizes_and_the_largest_key(ssa, dev, name):
    c = P.roots_case(name)
    P.check_labels(c.label, c.N)
    P.check_block_incl(c.block_incl, c.label == np.arange(c.N))  # anything else would direct stores outside roots and sizes
    roots = Guarded(len(c.roots), torch.int64, dev, 'roots')
    sizes = Guarded(len(c.roots), torch.int64, dev, 'sizes')
    best = Guarded(1, torch.int64, dev, 'best')
    best.buf[GUARD] = 0  # as components.py starts it
    _call(ssa, dev, 'ss_components_roots', _to(dev, c.label), _to(dev, c.size), c.N, _to(dev, c.block_incl), roots, sizes, best)
    np.testing.assert_array_equal(roots.result(), c.roots, err_msg='roots')
    np.testing.assert_array_equal(sizes.result(), c.sizes, err_msg='sizes')
    key = int(best.result()[0]) & 0xFFFFFFFFFFFFFFFF
    assert key == c.best, f'best: size {key >> 32} root {0xFFFFFFFF - (key & 0xFFFFFFFF)}, expected size {c.top} root {c.winner} at {P.place(c.winner)}'


# ---- 3. select, mapper, edges, same -----------------------------------------------------------------------------------------------------
def _select(ssa, dev, N, keep, mask=None, label=None, best=None):
    """the count pass, the numpy cumulative sum, the fill pass; everything compared with the kept set's numpy answer"""
    want_counts, want_nodes, want_mapper = P.select_expected(N, keep)
    counts = Guarded(len(want_counts), torch.int32, dev, 'block_count')
    _call(ssa, dev, 'ss_induced_select', mask, label, best, N, None, counts, None, None)
    np.testing.assert_array_equal(counts.result(), want_counts, err_msg='block_count')
    incl = np.cumsum(want_counts).astype(np.int64)
    P.check_block_incl(incl, keep)
    nodes = Guarded(len(want_nodes), torch.int64, dev, 'nodes')
    mapper = Guarded(N, torch.int64, dev, 'mapper')
    _call(ssa, dev, 'ss_induced_select', mask, label, best, N, _to(dev, incl), None, nodes, mapper)
    np.testing.assert_array_equal(nodes.result(), want_nodes, err_msg='nodes')
    np.testing.assert_array_equal(mapper.result(), want_mapper, err_msg='mapper')


@pytest.mark.parametrize('k', range(4))
def test_select_by_a_planted_key(ssa, dev, k):
    """*best names node 0, the last node of chunk 0, the first node of chunk 2 or the last node; its high word is not a size"""
    plan = P.label_plan(P.N_BASE)
    root, best, members = P.select_label_cases()[k]
    assert np.array_equal(np.flatnonzero(plan.label == root), members)
    _select(ssa, dev, plan.N, plan.label == root, label=_to(dev, plan.label), best=torch.tensor([best], dtype=torch.int64, device=dev))


@pytest.mark.parametrize('kind', P.MASKS)
def test_select_by_mask_bytes(ssa, dev, kind):
    m = P.mask_plan(kind)
    _select(ssa, dev, m.N, m.mask != 0, mask=_to(dev, m.mask))


@pytest.mark.parametrize('name', P.MAPPER_CASES)
def test_the_mapper_of_a_node_list(ssa, dev, name):
    """mapper[x] is the position of x for an id listed once and -1 outside the list; the two flags are exact.  For an id listed TWICE
    mapper[x] is one of its positions: which writer's compare-and-swap comes first is not specified, and no more is asserted."""
    c = P.mapper_case(name)
    mapper = Guarded(c.N, torch.int64, dev, 'mapper')
    flags = torch.zeros((2,), dtype=torch.int32, device=dev)
    _call(ssa, dev, 'ss_induced_mapper', _to(dev, c.nodes), len(c.nodes), c.N, mapper, flags[0:], flags[1:])
    assert flags.tolist() == [c.err, c.dup], 'the flags {an id out of range, an id listed twice}'
    got = mapper.result()
    want = c.mapper.copy()
    for x, positions in c.twice.items():
        assert got[x] in positions, f'mapper[{x}] = {got[x]}, listed at {positions}'
        want[x] = got[x]
    np.testing.assert_array_equal(got, want, err_msg='mapper')


@pytest.mark.parametrize('kind,E', P.EDGE_CASES)
def test_the_edges_of_a_planted_mapper(ssa, dev, kind, E):
    c = P.edges_case(kind, E)
    src, dst, mapper = _to(dev, c.src), _to(dev, c.dst), _to(dev, c.mapper)
    counts = Guarded(len(c.block_count), torch.int32, dev, 'block_count')
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    _call(ssa, dev, 'ss_induced_edges', src, dst, E, c.N, mapper, None, counts, None, None, None, err)
    np.testing.assert_array_equal(counts.result(), c.block_count, err_msg='block_count')
    assert err.item() == c.err == 1, 'the endpoint equal to N raises the error word'
    incl = np.cumsum(c.block_count).astype(np.int64)
    P.check_block_incl(incl, c.keep)
    outs = [Guarded(len(c.edge_ids), torch.int64, dev, what) for what in ('out_src', 'out_dst', 'edge_ids')]
    _call(ssa, dev, 'ss_induced_edges', src, dst, E, c.N, mapper, _to(dev, incl), None, *outs, None)
    for out, want in zip(outs, (c.out_src, c.out_dst, c.edge_ids)):
        np.testing.assert_array_equal(out.result(), want, err_msg=out.what)


@pytest.mark.parametrize('L', P.SAME_L)
def test_same_on_planted_labels(ssa, dev, L):
    c = P.same_case(L)
    plan = P.label_plan(P.N_BASE)
    out = Guarded(L, torch.uint8, dev, 'out')
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    _call(ssa, dev, 'ss_components_same', _to(dev, plan.label), c.N, _to(dev, c.links), L, out, err)
    np.testing.assert_array_equal(out.result(), c.out, err_msg='out')
    assert err.item() == c.err == 1 and c.out[100] == 0, 'the id equal to N: answer 0, the error word rises'
