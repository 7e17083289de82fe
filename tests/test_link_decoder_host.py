"""What link_decoder.link_gather / link_hadamard promise that needs no device: the restatement the GPU tests compare against
(tests/link_decoder_restatement.py) is pinned to float64 and to torch's own indexing, its grouping is a stable argsort, the planted
batch has the rows it is meant to have, four deliberate mistakes in the restated backward each change bits on it, argument errors
are raised on the host, the header and the binding carry the new symbols, and the byte model is counted by hand."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import link_decoder_restatement as lr

U = 2.0 ** -24


@pytest.fixture(scope='module')
def batch():
    links = lr.planted()
    return links, lr.features(lr.N, 8), lr.features(len(links) * 2, 8, seed=5).reshape(len(links), 2, 8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_planted_batch_has_its_rows(batch):
    links, _, _ = batch
    m = lr.slot_counts(links)
    assert tuple(m[list(lr.NODES)]) == lr.COUNTS == (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)  # exactly
    assert 650 <= lr.N <= 750 and lr.NODES[1] == 0 and lr.NODES[-1] == lr.N - 1 and lr.NODES[3] == lr.NODES[2] + 1
    assert m.sum() == 2 * len(links) and links.min() == 0 and links.max() == lr.N - 1 and m[lr.ZERO] == 0
    pool = np.setdiff1d(np.arange(lr.N), lr.NODES)
    assert m[pool].sum() == sum(lr.COUNTS) - 2 - 2 and (m[pool] == 0).sum() == 0 and m[pool].max() < 16  # every other slot is a pool node's
    loops = links[links[:, 0] == links[:, 1]]
    assert sorted(loops[:, 0].tolist()) == [lr.SELF_ONLY, lr.STRADDLE]                       # two self links
    assert ((links == lr.SELF_ONLY).any(axis=1)).sum() == 1                                  # ... one of them a node's only link
    triple = links[(links == lr.TRIPLE).any(axis=1)]
    assert len(triple) == 3 and len(np.unique(triple, axis=0)) == 1                          # one link, three times
    big = lr.NODES[-1]
    assert (links[:, 0] == big).sum() == 513 and (links[:, 1] == big).sum() == 512           # u in some links, v in others
    pairs = links[:, 0] * lr.N + links[:, 1]
    assert len(np.unique(pairs)) < len(pairs) - 2                                            # the longest row repeats partners
    qs = np.nonzero(links.reshape(-1) == lr.STRADDLE)[0]                                     # ascending: the node's group
    assert len(qs) == 257 and qs[255] + 1 == qs[256] and qs[255] % 2 == 0                    # the two slots of ONE link ...
    assert tuple(links[qs[255] >> 1]) == (lr.STRADDLE, lr.STRADDLE)                          # ... a self link, either side of slot 256
    assert (np.diff(links[:, 0]) < 0).any()                                                  # the batch itself is shuffled


def test_grouping_is_a_stable_argsort(batch):
    links, _, _ = batch
    for lk, n in ((links, lr.N), (links[:40], lr.N), (np.array([[2, 2], [2, 0], [0, 2]]), 3), (np.zeros((0, 2), dtype=np.int64), 4)):
        flat = np.asarray(lk).reshape(-1)
        nodes, rowptr, order = lr.grouping(lk, n)
        assert np.array_equal(order, np.argsort(flat, kind='stable'))
        assert np.array_equal(nodes, np.unique(flat)) and np.array_equal(np.diff(rowptr), np.bincount(flat, minlength=n)[nodes])
        assert rowptr[0] == 0 and rowptr[-1] == len(flat)


def test_forwards_are_torch_indexing(batch):
    links, x, _ = batch
    tx, tl = torch.from_numpy(x), torch.from_numpy(links)
    assert np.array_equal(_bits(lr.gather(x, links)), _bits(tx[tl].numpy())) and lr.gather(x, links).shape == (len(links), 2, 8)
    assert np.array_equal(_bits(lr.hadamard(x, links)), _bits((tx[tl][:, 0, :] * tx[tl][:, 1, :]).numpy()))


@pytest.mark.parametrize('mode', ['gather', 'product'])
def test_restatement_against_float64(batch, mode):
    """every grad_x[n] within gamma_k * sum |t_q| of float64, k = m + 2 for a row of m slots: one rounding of the term (the product)
    and at most m + 1 adds on its way (at most 256 inside its chunk, then the chunk adds)"""
    links, x, g = batch
    g = g if mode == 'gather' else g[:, 0]
    xs = None if mode == 'gather' else x
    got = lr.grad(links, lr.N, g, xs)
    want, mag = lr.grad64(links, lr.N, g, xs)
    k = (lr.slot_counts(links) + 2.0) * U
    bound = (k / (1 - k))[:, None] * mag
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err[mag > 0] / bound[mag > 0]).max())
    print(f'[link_decoder] {mode}: worst error / bound = {worst:.3f}')
    assert got.dtype == np.float32 and worst < 1 and np.all(got[mag.sum(axis=1) == 0].view(np.uint32) == 0)
    # and it is the gradient: torch autograd of the float64 composition
    tx = torch.from_numpy(x).double().requires_grad_(True)
    y = tx[torch.from_numpy(links)]
    ((y if mode == 'gather' else y[:, 0] * y[:, 1]) * torch.from_numpy(g).double()).sum().backward()
    assert np.allclose(tx.grad.numpy(), want, rtol=1e-12, atol=1e-12)


def test_mutations_change_bits(batch):
    """the planted batch tells the contract from four near misses: the wrong partner (the node's own row for the partner's), s
    swapped (the other endpoint's gradient row), descending slot order, one running sum for the chunk sums"""
    links, x, g = batch
    right = {'gather': lr.grad(links, lr.N, g), 'product': lr.grad(links, lr.N, g[:, 0], x)}
    cases = (('wrong partner', 'product'), ('s swapped', 'gather'), ('descending', 'gather'), ('descending', 'product'),
             ('one running sum', 'gather'), ('one running sum', 'product'))
    assert {m for m, _ in cases} == set(lr.MUTATIONS)
    long_rows = lr.slot_counts(links) > lr.C
    for mutation, mode in cases:
        wrong = lr.grad(links, lr.N, g if mode == 'gather' else g[:, 0], None if mode == 'gather' else x, mutation=mutation)
        differs = (_bits(wrong) != _bits(right[mode])).any(axis=1)
        assert differs.any(), (mutation, mode)
        if mutation == 'one running sum':
            assert not differs[~long_rows].any() and differs[long_rows].any()  # a row of at most 256 slots IS one running sum
        if mutation == 'wrong partner':
            assert not differs[lr.SELF_ONLY]                                   # a self link's partner is the node itself


def test_grad_rows_is_the_restatement(batch):
    links, x, g = batch
    rows = np.array([0, lr.ZERO, lr.SELF_ONLY, lr.TRIPLE, lr.STRADDLE, 100, lr.N - 1])
    g2 = g.reshape(-1, 8)
    assert np.array_equal(_bits(lr.grad_rows(links, rows, lambda i: g2[i], 8)), _bits(lr.grad(links, lr.N, g)[rows]))
    g1 = np.ascontiguousarray(g[:, 1])
    assert np.array_equal(_bits(lr.grad_rows(links, rows, lambda i: g1[i], 8, lambda i: x[i])), _bits(lr.grad(links, lr.N, g1, x)[rows]))


def test_header_and_binding_have_the_symbols():
    import subgraph_sketching_amd as ssa
    sig = ssa._native.SIGNATURES
    for name, n_args in (('ss_link_gather', 8), ('ss_link_hadamard', 8), ('ss_link_grad_rows', 14), ('ss_link_grad_hub_partials', 18),
                         ('ss_link_grad_hub_finish', 12), ('ss_link_workspace_bytes', 2), ('ss_link_chunk', 0)):
        assert name in sig and len(sig[name][1]) == n_args, name
    assert ssa.link_gather is ssa.link_decoder.link_gather and ssa.link_hadamard is ssa.link_decoder.link_hadamard
    assert ssa.LinkBatch is ssa.link_decoder.LinkBatch and 'link_decoder' in ssa.__all__ and 'LinkBatch' in ssa.__all__
    lib = ssa._native.lib()
    assert lib.ss_link_chunk() == 256 == ssa.link_decoder.LINK_CHUNK == lr.C == lib.ss_aggr_chunk()
    assert lib.ss_link_workspace_bytes(7, 260) == 7 * 260 * 4 and lib.ss_link_workspace_bytes(7, 3) == 84 and lib.ss_link_workspace_bytes(0, 8) == 0
    assert lib.ss_link_workspace_bytes(-1, 8) == 0 and lib.ss_link_workspace_bytes(7, 0) == 0 and lib.ss_link_workspace_bytes(1 << 31, 8) == 0
    assert isinstance(ssa.link_decoder.DEFAULT_HUB_ENTRIES, int) and ssa.link_decoder.DEFAULT_HUB_ENTRIES >= 1
    assert lib.ss_version() == 129  # (new entry points, no changed one: the ABI number stays)


def test_c_abi_rejects_bad_arguments_on_the_host():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    fake = c_void_p(16)  # never dereferenced: every call below ends in the host-side checks

    def sweep(fn, ok, needed, bad_values, nothing_to_do):
        for i in needed:
            assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == -1, (fn.__name__, i)
        for i, bad in bad_values:
            assert fn(*[bad if j == i else a for j, a in enumerate(ok)]) == -1, (fn.__name__, i, bad)
        for i in nothing_to_do:  # (no links / nodes / columns / chunks / hubs: SS_OK before any pointer is looked at)
            assert fn(*[0 if j == i else (None if isinstance(a, c_void_p) else a) for j, a in enumerate(ok)]) == 0, (fn.__name__, i)

    for fn in (lib.ss_link_gather, lib.ss_link_hadamard):
        #          links L  x     N  F  out   err   stream
        sweep(fn, [fake, 3, fake, 5, 8, fake, fake, None], (0, 2, 5), ((1, -1), (1, 1 << 30), (3, -1), (3, 1 << 31), (4, -1)), (1, 4))
    #                        nodes rowptr order M links L  N  hub mode g    x     F  grad  stream
    sweep(lib.ss_link_grad_rows, [fake, fake, fake, 3, fake, 4, 5, 64, 1, fake, fake, 8, fake, None], (0, 1, 2, 4, 9, 10, 12),
          ((3, -1), (3, 6), (5, -1), (5, 1), (5, 1 << 30), (6, -1), (6, 1 << 31), (7, 0), (7, -3), (8, 2), (8, -1), (11, -1)), (3, 11))
    #                                rowptr order M  links L  N  hubs  chunk c_hub nh nc mode g    x     F  ws    bytes   stream
    sweep(lib.ss_link_grad_hub_partials, [fake, fake, 3, fake, 4, 5, fake, fake, fake, 2, 3, 1, fake, fake, 8, fake, 3 * 32, None],
          (0, 1, 3, 6, 7, 8, 12, 13, 15), ((2, -1), (2, 6), (4, -1), (4, 1), (5, 1 << 31), (9, -1), (9, 4), (10, -1), (10, 1 << 31), (11, 2), (14, -1),
                                           (16, 3 * 32 - 1)), (2, 14))
    assert lib.ss_link_grad_hub_partials(None, None, 3, None, 4, 5, None, None, None, 0, 0, 1, None, None, 8, None, 0, None) == 0  # no chunks
    #                              nodes M  hubs  chunk nh nc N  ws    bytes   F  grad  stream
    sweep(lib.ss_link_grad_hub_finish, [fake, 3, fake, fake, 2, 3, 5, fake, 3 * 32, 8, fake, None], (0, 2, 3, 7, 10),
          ((1, -1), (1, 6), (4, -1), (4, 4), (5, -1), (6, -1), (6, 1 << 31), (8, 3 * 32 - 1), (9, -1)), (1, 4, 9))


def test_argument_errors_need_no_device():
    import subgraph_sketching_amd as ssa
    links = torch.zeros((3, 2), dtype=torch.int64)
    x = torch.zeros((4, 4))
    for bad in (links.to(torch.int32), links[0], links.t(), links.numpy(), torch.zeros((3, 3), dtype=torch.int64), links[None]):
        with pytest.raises(ValueError):
            ssa.LinkBatch(4, bad)
        for fn in (ssa.link_gather, ssa.link_hadamard):
            with pytest.raises(ValueError):
                fn(x, bad)
    for bad_hub in (0, -1, 2.5, True, 1 << 63, 1 << 70):  # (the C entry takes an int64)
        with pytest.raises(ValueError):
            ssa.LinkBatch(4, links, hub_entries=bad_hub)
    for bad_n in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            ssa.LinkBatch(bad_n, links)
    plan = ssa.LinkBatch.__new__(ssa.LinkBatch)
    plan.num_nodes, plan.device = 4, torch.device('meta')
    for fn in (ssa.link_gather, ssa.link_hadamard):
        for bad_x in (x.double(), x.half(), x[0], x[None], np.zeros((4, 4), dtype=np.float32)):
            with pytest.raises(ValueError):
                fn(bad_x, links)
            with pytest.raises(ValueError):
                fn(bad_x, plan)
        with pytest.raises(ValueError, match='no CPU fallback and no silent copy'):
            fn(x, links)                                   # x on the host
        with pytest.raises(ValueError, match='no CPU fallback and no silent copy'):
            fn(x, plan)                                    # x elsewhere than the plan
        with pytest.raises(ValueError):
            fn(x[:3], plan)                                # not the plan's node count
        with pytest.raises(ValueError):
            fn(x, 'not links')


def test_byte_model_on_a_hand_counted_case():
    """5 nodes, 3 links, F = 8 (rows of 32 bytes).  Forward: 6 ids of 8 bytes, 6 rows gathered, 6 rows (gather) or 3 rows (product)
    written.  Backward on M = 4 touched nodes: 5 rows cleared, 6 rows of g gathered (product: and 6 of x), 4 rows written, 6 order words
    of 4 bytes (product: and 6 partner ids of 8), 4 * (8 + 16) bytes of node ids and row pointers"""
    import subgraph_sketching_amd as ssa
    f = ssa.roofline.link_decoder_bytes
    zero = {'ids': 0, 'gathered': 0, 'written': 0, 'cleared': 0, 'entries': 0, 'workspace': 0}
    assert f(N=5, L=3, F=8) == dict(zero, ids=48, gathered=192, written=192, total=432)
    assert f(5, 3, 8, product=True) == dict(zero, ids=48, gathered=192, written=96, total=336)
    assert f(5, 3, 8, backward=True, M=4) == dict(zero, cleared=160, gathered=192, written=128, entries=24 + 96, total=600)
    assert f(5, 3, 8, product=True, backward=True, M=4) == dict(zero, cleared=160, gathered=384, written=128, entries=72 + 96, total=840)
    assert f(5, 3, 8, backward=True)['written'] == 160                                      # M defaults to min(N, 2L)
    hub = f(5, 3, 8, backward=True, M=4, hub_chunks=3)                                      # three partial rows written, then read
    assert hub['workspace'] == 192 and hub['total'] == 600 + 192
    assert f(5, 3, 260, backward=True, M=4)['entries'] == 2 * 24 + 96                       # a second pass over the slots past 256 columns
    assert f(5, 3, 130, product=True, backward=True, M=4)['entries'] == 3 * 72 + 96         # F % 4 != 0: single floats, 64 per pass
    assert f(5, 3, 6)['total'] == 48 + 2 * 6 * 24                                           # ... and no padding
    assert f(5, 0, 8)['total'] == 0 and f(5, 3, 0)['total'] == 0 and f(5, 3, 0, backward=True)['total'] == 0
    assert f(5, 0, 8, backward=True) == dict(zero, cleared=160, total=160)                  # no links: the zero fill remains
