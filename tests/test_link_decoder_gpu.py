"""link_decoder.link_gather / link_hadamard (csrc/ss_link_decoder.hip) on the GPU.  Forward bits are torch's own (`x[links]` and the
product of its halves); backward bits are the restatement's (tests/link_decoder_restatement.py, pinned to float64 and to a stable
argsort by tests/test_link_decoder_host.py): the contract fixes the accumulation order, so there is exactly one right answer, whichever
tier a row goes through and whatever else the batch holds."""
import ctypes

import numpy as np
import pytest
import torch

import large_table_helpers as lt
import link_decoder_restatement as lr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WIDTHS = (0, 1, 3, 4, 8, 20, 64, 256, 260, 1024)  # no column; scalar pieces; lane groups of 1, 2, 8 (5 pieces), 16, 64; a second pass of one piece; four passes
HUB_ENTRIES = (1, 8, 255, 256, 257, 10 ** 9)
SENTINEL = 0x7FC0BEEF  # a NaN no sum produces
MODES = ('gather', 'product')


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


class Case(object):
    """the planted batch, its plan (default hub_entries), x [N, 1024], g [L, 2, 1024] for the gather and g[:, 1] for the product (the
    first F columns are the x and g of every F: the columns do not depend on each other), and the restated gradients, computed on first
    use and kept"""

    def __init__(self, ssa, dev):
        self.dev = dev
        self.links = lr.planted()
        self.L = len(self.links)
        self.tl = torch.from_numpy(self.links).to(dev)
        self.plan = ssa.LinkBatch(lr.N, self.tl)
        self.host = {'x': lr.features(lr.N, 1024), 'g': lr.features(2 * self.L, 1024, seed=5).reshape(self.L, 2, 1024)}
        self.x, self.g = (torch.from_numpy(a).to(dev) for a in (self.host['x'], self.host['g']))
        self.counts = lr.slot_counts(self.links)
        self._memo = {}

    def g_of(self, mode, F=1024):
        """(a non-contiguous grad_out unless F = 1024 and the mode is the gather)"""
        return self.g[:, :, :F] if mode == 'gather' else self.g[:, 1, :F]

    def grad(self, mode, F=1024):
        if mode not in self._memo:
            self._memo[mode] = lr.grad(self.links, lr.N, self.host['g'] if mode == 'gather' else self.host['g'][:, 1],
                                       None if mode == 'gather' else self.host['x'])
        return self._memo[mode][:, :F]


@pytest.fixture(scope='module')
def case(ssa, dev):
    return Case(ssa, dev)


def _bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f'{what}: {tuple(g.shape)} against {tuple(w.shape)}'
    bad = torch.nonzero(g != w)
    assert len(bad) == 0, f'{what}: {len(bad)} of {g.numel()} elements differ, first at {bad[:4].tolist()}'


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _fn(ssa, mode):
    return ssa.link_gather if mode == 'gather' else ssa.link_hadamard


def _torch_forward(x, tl, mode):
    y = x[tl]
    return y if mode == 'gather' else y[:, 0, :] * y[:, 1, :]


def _run(ssa, mode, x, links, g):
    """(forward output, x.grad) of one forward + backward"""
    xs = x.detach().clone().requires_grad_(True)
    y = _fn(ssa, mode)(xs, links)
    (y * g).sum().backward()
    return y.detach(), xs.grad


def test_plan(case, ssa, dev):
    plan = case.plan
    nodes, rowptr, order = lr.grouping(case.links, lr.N)
    assert (plan.num_nodes, plan.num_links, plan.device, plan.hub_entries) == (lr.N, case.L, dev, ssa.link_decoder.DEFAULT_HUB_ENTRIES)
    assert plan.num_touched == len(nodes) == (case.counts > 0).sum() and plan.nodes.dtype == plan.rowptr.dtype == torch.int64
    assert plan.nodes.tolist() == nodes.tolist() and plan.rowptr.tolist() == rowptr.tolist()
    assert plan.order.dtype == torch.int32 and plan.order.tolist() == order.tolist() == np.argsort(case.links.reshape(-1), kind='stable').tolist()
    small = ssa.LinkBatch(lr.N, case.tl, hub_entries=256)
    m = case.counts[nodes]
    hubs = np.nonzero(m > 256)[0]                               # positions in `nodes`: the rows of 257, 511, 512, 513 and 1025 slots
    chunks = (m[hubs] + 255) // 256
    assert nodes[hubs].tolist() == [lr.STRADDLE, 440, 480, 520, lr.N - 1] and chunks.tolist() == [2, 2, 2, 3, 5]
    assert small.n_hubs == 5 and small.n_chunks == 14 and small.hub_rows.tolist() == hubs.tolist()
    assert small.hub_chunk.tolist() == [0, 2, 4, 6, 9, 14] and small.chunk_hub.tolist() == np.repeat(np.arange(5), chunks).tolist()
    assert small.hub_rows.dtype == small.hub_chunk.dtype == small.chunk_hub.dtype == torch.int32
    assert small.order.tolist() == plan.order.tolist()          # the grouping does not depend on hub_entries
    one = ssa.LinkBatch(lr.N, case.tl, hub_entries=1)
    assert one.n_hubs == (case.counts > 1).sum() and one.n_chunks == ((case.counts[case.counts > 1] + 255) // 256).sum()
    before = ssa.LinkBatch.builds
    host = ssa.LinkBatch(lr.N, torch.from_numpy(case.links))    # host links: the plan lives on the current GPU
    assert host.device.type == 'cuda' and host.order.tolist() == plan.order.tolist() and ssa.LinkBatch.builds == before + 1
    edited = case.tl.clone()
    private = ssa.LinkBatch(lr.N, edited)
    edited[5, 1] = (edited[5, 1] + 1) % lr.N                    # the plan keeps a private copy of the links
    y, grad = _run(ssa, 'product', case.x[:, :8], private, case.g_of('product', 8))
    _assert_same(grad, case.grad('product', 8), 'private copy')
    _assert_same(y, _torch_forward(case.x[:, :8], case.tl, 'product'), 'private copy, forward')


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('mode', MODES)
def test_forward_and_backward_bits(case, ssa, dev, mode, F):
    x = case.x[:, :F].clone().requires_grad_(True)
    g = case.g_of(mode, F)
    for links in (case.plan, case.tl):                          # a plan given, and one built at forward time
        x.grad = None
        y = _fn(ssa, mode)(x, links)
        assert y.shape == ((case.L, 2, F) if mode == 'gather' else (case.L, F)) and y.dtype == torch.float32 and y.device == x.device
        assert y.is_contiguous() and y.requires_grad
        _assert_same(y, _torch_forward(x.detach(), case.tl, mode), f'{mode} F={F} forward')
        (y * g).sum().backward(retain_graph=True)
        first = x.grad.clone()
        assert first.shape == (lr.N, F)
        _assert_same(first, case.grad(mode, F), f'{mode} F={F} x.grad')
        x.grad = None
        (y * g).sum().backward()
        _assert_same(x.grad, first, f'{mode} F={F} second backward')
    with torch.no_grad():
        y = _fn(ssa, mode)(x, case.tl)
        assert not y.requires_grad
        _assert_same(y, _torch_forward(x.detach(), case.tl, mode), f'{mode} F={F} forward only')
    if F in (4, 260):  # a base that is not 16-byte aligned takes single floats: the same bits
        flat = torch.zeros(lr.N * F + 1, dtype=torch.float32, device=dev)
        odd = flat[1:].view(lr.N, F)
        odd.copy_(case.x[:, :F])
        assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
        odd.requires_grad_(True)
        y = _fn(ssa, mode)(odd, case.plan)
        (y * g).sum().backward()
        _assert_same(y, _torch_forward(odd.detach(), case.tl, mode), f'{mode} F={F} unaligned x, forward')
        _assert_same(odd.grad, case.grad(mode, F), f'{mode} F={F} unaligned x, x.grad')
    ssa.link_decoder.check_errors()


def test_nan_and_inf_rows_poison_their_partners_only(case, ssa, dev):
    """NaN, +inf and -inf rows of x: the forward has torch's bits; the product's backward is non-finite in exactly the rows that have a
    poisoned partner (a self link: the node itself), every other row keeps its bits; the gather's backward never reads x"""
    F = 260
    poisoned = {int(np.setdiff1d(np.arange(lr.N), lr.NODES)[100]): np.nan, lr.SELF_ONLY: np.inf, lr.TRIPLE: -np.inf, 120: np.nan}
    x = case.host['x'][:, :F].copy()
    for node, value in poisoned.items():
        x[node] = value
    x[0, 256:] = np.nan                                         # and the last piece of one row alone (lanes past it re-read it)
    tx = torch.from_numpy(x).to(dev)
    bad = np.isin(case.links, list(poisoned))
    partner_bad = np.zeros(lr.N, dtype=bool)                    # node n has a slot whose partner is poisoned
    for s in (0, 1):
        partner_bad[case.links[bad[:, 1 - s], s]] = True
    assert partner_bad[lr.SELF_ONLY] and not partner_bad[lr.TRIPLE] and 17 < partner_bad.sum() < 80
    for hub in (256, 10 ** 9):
        plan = ssa.LinkBatch(lr.N, case.tl, hub_entries=hub)
        for mode in MODES:
            y, grad = _run(ssa, mode, tx, plan, case.g_of(mode, F))
            _assert_same(y, _torch_forward(tx, case.tl, mode), f'{mode} forward with NaN / inf rows')
            if mode == 'gather':
                _assert_same(grad, case.grad(mode, F), 'gather: x is not read by the backward')
                continue
            rows = ~torch.isfinite(y[:, :256]).all(dim=1).cpu().numpy()
            assert set(np.nonzero(rows)[0]) == set(np.nonzero(bad.any(axis=1))[0])
            got = grad.cpu().numpy()
            nonfinite = ~np.isfinite(got[:, :256]).all(axis=1)
            assert set(np.nonzero(nonfinite)[0]) == set(np.nonzero(partner_bad)[0]), hub
            tail = ~np.isfinite(got[:, 256:]).all(axis=1)       # the partner of node 0's only slot has the NaN piece as well
            assert set(np.nonzero(tail)[0]) == set(np.nonzero(partner_bad)[0]) | set(case.links[(case.links == 0).any(axis=1)].reshape(-1)) - {0}
            _assert_same(got[~nonfinite, :256], case.grad(mode, F)[~nonfinite, :256], f'beside the poisoned rows, hub_entries={hub}')


@pytest.mark.parametrize('hub', HUB_ENTRIES)
def test_rows_do_not_depend_on_the_tier(case, ssa, hub):
    """the same bits at every hub_entries: at 1 every row of two or more slots is a hub (most of one chunk), at 255 .. 257 the rows of
    256 and 257 slots change sides, at 10^9 nothing is a hub"""
    plan = ssa.LinkBatch(lr.N, case.tl, hub_entries=hub)
    assert plan.hub_entries == hub and plan.n_hubs == (case.counts > hub).sum()
    assert plan.n_hubs == {255: 6, 256: 5, 257: 4, 10 ** 9: 0}.get(hub, plan.n_hubs) and (hub > 8 or plan.n_hubs > 13)
    for F in (3, 20, 260):
        for mode in MODES:
            y, grad = _run(ssa, mode, case.x[:, :F], plan, case.g_of(mode, F))
            _assert_same(grad, case.grad(mode, F), f'hub_entries={hub} {mode} F={F} x.grad')
            _assert_same(y, _torch_forward(case.x[:, :F], case.tl, mode), f'hub_entries={hub} {mode} F={F} forward')


def test_rows_do_not_depend_on_the_other_links(case, ssa, dev):
    """the batch embedded among 5000 links over other nodes (ids N .. 2N - 1, and the planted batch's node without slots), the planted
    links keeping their relative order: rows 0 .. N - 1 keep their bits, the whole gradient is the restatement's"""
    F = 20
    rng = np.random.RandomState(7)
    extra = lr.N + rng.randint(0, lr.N, size=(5000, 2))
    extra[::50, 0] = lr.ZERO
    where = np.sort(rng.choice(case.L + 5000, size=case.L, replace=False))
    links = np.zeros((case.L + 5000, 2), dtype=np.int64)
    mask = np.zeros(len(links), dtype=bool)
    mask[where] = True
    links[mask], links[~mask] = case.links, extra
    x = np.concatenate([case.host['x'][:, :F], lr.features(lr.N, F, seed=9)])
    g = lr.features(2 * len(links), F, seed=10).reshape(len(links), 2, F)
    g[mask] = case.host['g'][:, :, :F]
    tx, tg, tlk = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(links).to(dev)
    keep = torch.from_numpy(np.setdiff1d(np.arange(lr.N), [lr.ZERO])).to(dev)
    for mode in MODES:
        gm = tg if mode == 'gather' else tg[:, 1]
        y, grad = _run(ssa, mode, tx, tlk, gm)
        _assert_same(grad[keep], case.grad(mode, F)[keep.cpu().numpy()], f'{mode}: the planted rows inside the larger batch')
        want = lr.grad(links, 2 * lr.N, g if mode == 'gather' else g[:, 1], None if mode == 'gather' else x)
        _assert_same(grad, want, f'{mode}: the larger batch')
        assert bool((grad[lr.ZERO] != 0).any())


def test_split_batches(case, ssa, dev):
    """the batch cut in two, by position and by planted node (the links of every other planted node against the rest, so that whole long
    rows fall to one side): on the rows that only one part touches, that part's gradient has the whole batch's bits"""
    F = 20
    first = np.arange(case.L) < case.L // 2
    even = np.isin(case.links, lr.NODES[::2]).any(axis=1)
    for mode in MODES:
        g = case.g_of(mode, F)
        for part, must in ((first, ()), (~first, ()), (even, lr.NODES[2::2]), (~even, lr.NODES[1::2])):
            idx = torch.from_numpy(np.nonzero(part)[0]).to(dev)
            _, grad = _run(ssa, mode, case.x[:, :F], case.tl[idx], g[idx])
            inside = lr.slot_counts(case.links[part])
            only = (inside > 0) & (inside == case.counts)
            assert only.sum() >= 8 and all(only[n] for n in must)
            _assert_same(grad[torch.from_numpy(only)], case.grad(mode, F)[only], f'{mode}: rows only this part touches')
            untouched = torch.from_numpy(inside == 0)
            assert untouched.sum() >= 1 and bool((_bits(grad[untouched]) == 0).all())


def test_link_permutations(case, ssa, dev):
    """a permutation of the links permutes the forward's rows and changes the backward only through the order of a row's slots: the
    result is the restatement of the permuted batch; rows of at most two slots keep their bits (0 + a + b = 0 + b + a); swaps of
    neighbouring links that share no node leave every row's slot order, and so every bit, alone"""
    F = 20
    rng = np.random.RandomState(21)
    perm = rng.permutation(case.L)
    tperm = torch.from_numpy(perm).to(dev)
    quiet = np.arange(case.L)
    for i in range(0, case.L - 1, 2):
        if len(set(case.links[i]) & set(case.links[i + 1])) == 0:
            quiet[[i, i + 1]] = quiet[[i + 1, i]]
    assert (quiet != np.arange(case.L)).sum() > case.L // 2
    tquiet = torch.from_numpy(quiet).to(dev)
    for mode in MODES:
        g = case.g_of(mode, F)
        y0, grad0 = _run(ssa, mode, case.x[:, :F], case.tl, g)
        y, grad = _run(ssa, mode, case.x[:, :F], case.tl[tperm], g[tperm])
        _assert_same(y, y0[tperm], f'{mode}: forward rows permuted')
        hg = case.host['g'][perm][:, :, :F] if mode == 'gather' else case.host['g'][perm][:, 1, :F]
        want = lr.grad(case.links[perm], lr.N, hg, None if mode == 'gather' else case.host['x'][:, :F])
        _assert_same(grad, want, f'{mode}: the permuted batch')
        few = torch.from_numpy(case.counts <= 2)
        _assert_same(grad[few], grad0[few], f'{mode}: rows of at most two slots')
        assert bool((_bits(grad) != _bits(grad0)).any())        # ... and the long rows do notice
        y, grad = _run(ssa, mode, case.x[:, :F], case.tl[tquiet], g[tquiet])
        _assert_same(grad, grad0, f'{mode}: swaps that keep every row order')


def test_two_runs_are_bit_identical(case, ssa):
    for mode in MODES:
        for links in (case.plan, case.tl):
            a, b = _run(ssa, mode, case.x[:, :64], links, case.g_of(mode, 64)), _run(ssa, mode, case.x[:, :64], links, case.g_of(mode, 64))
            _assert_same(a[0], b[0], f'{mode} forward, run 2 against run 1')
            _assert_same(a[1], b[1], f'{mode} backward, run 2 against run 1')


def test_an_elph_shaped_step_repeats_bit_for_bit(case, ssa, dev):
    """GCNConv -> link_hadamard -> Linear -> loss (reference runners/train.py:200 with models/elph.py:54), twice from the same seed:
    identical outputs and identical parameter gradients"""
    rng = np.random.RandomState(3)
    e = rng.randint(0, lr.N, size=(2, 4000))
    ei = torch.from_numpy(np.concatenate([e, e[::-1]], axis=1)).to(dev)
    label = (torch.arange(case.L, device=dev) % 2).float()

    def step():
        torch.manual_seed(41)
        conv, head = ssa.GCNConv(20, 32).to(dev), torch.nn.Linear(32, 1).to(dev)
        graph = ssa.GCNGraph(lr.N, ei)
        h = torch.relu(conv(case.x[:, :20].contiguous(), graph))
        out = head(ssa.link_hadamard(h, case.tl))
        torch.nn.functional.binary_cross_entropy_with_logits(out.view(-1), label).backward()
        params = list(conv.parameters()) + list(head.parameters())
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()) for p in params)
        return [out.detach().clone()] + [p.grad.detach().clone() for p in params]

    first, second = step(), step()
    assert len(first) == len(second) == 5
    for i, (a, b) in enumerate(zip(first, second)):
        _assert_same(a, b, f'run 2 against run 1, tensor {i}')


def test_gradients_against_the_float64_composition(case, ssa):
    """x.grad within gamma_k * sum |t_q| of torch autograd through x[links] (and the product of its halves) in float64, k = m + 2 for
    a row of m slots"""
    F = 64
    k = (case.counts + 2.0) * U
    for mode in MODES:
        _, grad = _run(ssa, mode, case.x[:, :F], case.plan, case.g_of(mode, F))
        x64 = torch.from_numpy(case.host['x'][:, :F]).double().requires_grad_(True)
        y = x64[torch.from_numpy(case.links)]
        g64 = torch.from_numpy(case.host['g'][:, :, :F]).double()
        ((y * g64) if mode == 'gather' else (y[:, 0] * y[:, 1] * g64[:, 1])).sum().backward()
        hg = case.host['g'][:, :, :F] if mode == 'gather' else case.host['g'][:, 1, :F]
        _, mag = lr.grad64(case.links, lr.N, hg, None if mode == 'gather' else case.host['x'][:, :F])
        bound = (k / (1 - k))[:, None] * mag
        err = np.abs(grad.cpu().numpy().astype(np.float64) - x64.grad.numpy())
        worst = float((err[mag > 0] / bound[mag > 0]).max())
        print(f'[link_decoder] {mode} on the GPU: worst error / bound = {worst:.3f}')
        assert worst < 1 and np.all(err[mag == 0] == 0)


def test_one_plan_serves_several_gathers(case, ssa, dev):
    """node features and an embedding gathered at the same links (reference runners/train.py:200-201): ONE build; a tensor builds a
    plan per differentiable call and none without a gradient to compute"""
    F = 20
    feats = case.x[:, :F].clone().requires_grad_(True)
    emb = torch.nn.Embedding(lr.N, F).to(dev)
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(lr.features(lr.N, F, seed=8)).to(dev))
    before = ssa.LinkBatch.builds
    plan = ssa.LinkBatch(lr.N, case.tl)
    a, b = ssa.link_hadamard(feats, plan), ssa.link_gather(emb.weight, plan)
    ((a * case.g_of('product', F)).sum() + (b * case.g_of('gather', F)).sum()).backward()
    assert ssa.LinkBatch.builds == before + 1
    _assert_same(feats.grad, case.grad('product', F), 'features through the shared plan')
    _assert_same(emb.weight.grad, case.grad('gather', F), 'embedding through the shared plan')
    ssa.link_hadamard(feats, case.tl)
    ssa.link_gather(emb.weight, case.tl)
    assert ssa.LinkBatch.builds == before + 3                   # a tensor: one plan per differentiable call
    with torch.no_grad():
        ssa.link_hadamard(feats, case.tl)
    ssa.link_gather(case.x[:, :F], case.tl)                     # x does not ask for a gradient (BUDDY's data.x[curr_links], train.py:63)
    ssa.link_hadamard(feats.detach(), plan)
    assert ssa.LinkBatch.builds == before + 3
    with pytest.raises(ValueError):
        ssa.link_gather(case.x[:-1, :F], plan)
    with pytest.raises(ValueError):
        ssa.link_gather(case.x[:, :F].cpu(), plan)
    y = ssa.link_hadamard(case.x[:, :8].t().contiguous().t(), plan)  # a non-contiguous x is copied, not refused
    _assert_same(y, _torch_forward(case.x[:, :8], case.tl, 'product'), 'non-contiguous x')


@pytest.mark.parametrize('F', [3, 4, 20, 260])
def test_direct_launches_into_guarded_rows(case, ssa, dev, F):
    """every C entry through the binding into the middle of sentinel-filled buffers: the forwards write their L (2L) rows and nothing
    else; at hub_entries = 256 the regular launch writes the touched rows of at most 256 slots and leaves the hub rows, the rows no
    link touches and the guard rows alone; the partials launch writes its chunk rows exactly, and with one hub struck from the list
    that hub's rows stay untouched; the finish launch writes the hub rows only"""
    lib, guard, st, L, N = ssa._native.lib(), 67, _stream(dev), case.L, lr.N
    x = case.x[:, :F].contiguous()
    inside = lambda buf, rows: ctypes.c_void_p(buf.data_ptr() + guard * F * 4)
    for mode, entry, rows in (('gather', lib.ss_link_gather, 2 * L), ('product', lib.ss_link_hadamard, L)):
        buf = torch.full((rows + 2 * guard, F), SENTINEL, dtype=torch.int32, device=dev)
        assert entry(_p(case.tl), L, _p(x), N, F, inside(buf, rows), None, st) == 0
        torch.cuda.synchronize(dev)
        got = buf.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + rows:] == SENTINEL)
        _assert_same(got[guard:guard + rows].view(torch.float32), _torch_forward(x, case.tl, mode).reshape(rows, F), f'{mode} forward F={F}')
    plan = ssa.LinkBatch(N, case.tl, hub_entries=256)
    M, C = plan.num_touched, plan.n_chunks
    hub_row = torch.from_numpy(case.counts > 256)
    regular = torch.from_numpy((case.counts > 0) & (case.counts <= 256))
    nowhere = torch.from_numpy(case.counts == 0)
    assert hub_row.sum() == 5 and nowhere.sum() >= 1 and C == 14
    for mode_id, mode in enumerate(MODES):
        g = case.g_of(mode, F).contiguous()
        want = case.grad(mode, F)
        buf = torch.full((N + 2 * guard, F), SENTINEL, dtype=torch.int32, device=dev)
        out = inside(buf, N)
        rows = lambda: lib.ss_link_grad_rows(_p(plan.nodes), _p(plan.rowptr), _p(plan.order), M, _p(plan.links), L, N, 256, mode_id, _p(g),
                                             _p(x) if mode_id else None, F, out, st)
        assert rows() == 0
        torch.cuda.synchronize(dev)
        got = buf.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + N:] == SENTINEL)
        body = got[guard:guard + N]
        assert torch.all(body[hub_row] == SENTINEL) and torch.all(body[nowhere] == SENTINEL)     # hub rows and rows outside `nodes`: untouched
        _assert_same(body[regular].view(torch.float32), want[regular.numpy()], f'regular rows {mode} F={F}')

        ws = torch.full((C + 2 * guard, F), SENTINEL, dtype=torch.int32, device=dev)
        wsp = inside(ws, C)
        struck = plan.hub_rows.clone()
        struck[3] = -1                                                                            # this hub is not followed ...
        part = lambda hubs: lib.ss_link_grad_hub_partials(_p(plan.rowptr), _p(plan.order), M, _p(plan.links), L, N, _p(hubs), _p(plan.hub_chunk),
                                                          _p(plan.chunk_hub), plan.n_hubs, C, mode_id, _p(g), _p(x) if mode_id else None, F, wsp,
                                                          C * F * 4, st)
        partials = []                                                                             # p_c of every hub chunk, restated
        hg = case.host['g'][:, :, :F].reshape(-1, F) if mode == 'gather' else case.host['g'][:, 1, :F]
        for node in np.nonzero(case.counts > 256)[0]:
            qs = np.nonzero(case.links.reshape(-1) == node)[0]
            terms = lr.slot_terms(case.links, qs, lambda i: hg[i], None if mode == 'gather' else (lambda i: case.host['x'][i, :F]))
            partials += [lr.chunked_sum(terms[a:a + 256]) for a in range(0, len(qs), 256)]
        partials = np.stack(partials)
        assert part(struck) == 0
        torch.cuda.synchronize(dev)
        got = ws.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + C:] == SENTINEL)
        assert torch.all(got[guard + 6:guard + 9] == SENTINEL)                                    # ... and its three chunk rows stay untouched
        keep = np.r_[0:6, 9:C]
        _assert_same(got[guard:guard + C][keep].view(torch.float32), partials[keep], f'partials without one hub {mode} F={F}')
        assert part(plan.hub_rows) == 0
        torch.cuda.synchronize(dev)
        got = ws.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + C:] == SENTINEL)
        _assert_same(got[guard:guard + C].view(torch.float32), partials, f'partials {mode} F={F}')

        buf.fill_(SENTINEL)
        assert lib.ss_link_grad_hub_finish(_p(plan.nodes), M, _p(plan.hub_rows), _p(plan.hub_chunk), plan.n_hubs, C, N, wsp, C * F * 4, F, out, st) == 0
        torch.cuda.synchronize(dev)
        got = buf.cpu()
        assert torch.all(got[:guard] == SENTINEL) and torch.all(got[guard + N:] == SENTINEL)
        body = got[guard:guard + N]
        assert torch.all(body[~hub_row] == SENTINEL)                                              # the finish launch writes hub rows only
        _assert_same(body[hub_row].view(torch.float32), want[hub_row.numpy()], f'hub rows {mode} F={F}')
        assert rows() == 0                                                                        # both tiers into one buffer: every touched row
        torch.cuda.synchronize(dev)
        touched = ~nowhere
        _assert_same(buf[guard:guard + N][touched.to(dev)].view(torch.float32), want[touched.numpy()], f'both tiers {mode} F={F}')
        assert torch.all(buf[guard:guard + N][nowhere.to(dev)] == SENTINEL)
        assert lib.ss_link_grad_rows(_p(plan.nodes), _p(plan.rowptr), _p(plan.order), M, _p(plan.links), L, N, 256, 2, _p(g), _p(x), F, out, st) == -1


def test_out_of_range_ids(case, ssa, dev):
    """ids outside [0, N), negative ones included, inside wavefronts of good links: with a gradient to compute the plan raises
    IndexError; forward only, the row of such a slot (product: of such a link) is zeros, every other row has torch's bits, and
    check_errors() raises late, once"""
    F = 20
    ssa.link_decoder.check_errors()
    x = case.x[:, :F].contiguous()
    where = [(3, 0), (40, 1), (41, 0), (41, 1), (1000, 1), (case.L - 1, 0)]
    ids = [lr.N, -1, lr.N + (1 << 33), -(1 << 40), lr.N + 5, -lr.N]
    bad = case.tl.clone()
    for (l, s), v in zip(where, ids):
        bad[l, s] = v
    with pytest.raises(IndexError):
        ssa.LinkBatch(lr.N, bad)
    for mode in MODES:
        with pytest.raises(IndexError):
            _fn(ssa, mode)(x.clone().requires_grad_(True), bad)
    bad_links = sorted({l for l, _ in where})
    good = torch.from_numpy(np.setdiff1d(np.arange(case.L), bad_links)).to(dev)
    y = ssa.link_hadamard(x, bad)                               # no gradient asked for: nothing is grouped, nothing is read
    want = _torch_forward(x, case.tl, 'product')
    _assert_same(y[good], want[good], 'product: the neighbours of refused links')
    assert bool((_bits(y[bad_links]) == 0).all())
    with pytest.raises(IndexError, match='reported late'):
        ssa.link_decoder.check_errors()
    ssa.link_decoder.check_errors()                             # reported once
    with torch.no_grad():
        y = ssa.link_gather(x.clone().requires_grad_(True), bad)
    want = _torch_forward(x, case.tl, 'gather').clone()
    for l, s in where:
        want[l, s] = 0                                          # the slot's row alone: the link's other endpoint is gathered
    _assert_same(y, want, 'gather: refused slots')
    with pytest.raises(IndexError, match='reported late'):
        ssa.link_hadamard(x, case.tl)                           # the next call into the module reports it as well
    ssa.link_decoder.check_errors()
    _assert_same(ssa.link_hadamard(x, case.tl), _torch_forward(x, case.tl, 'product'), 'after the report')
    ssa.link_decoder.check_errors()


def test_tiny_cases(ssa, dev):
    """no links (with and without a plan), one node, every link on one node (600 self links: 1200 slots, a hub of five chunks)"""
    x5 = torch.from_numpy(lr.features(5, 12)).to(dev)
    none = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    for n in (5, 1):
        for links in (none, ssa.LinkBatch(n, none)):
            for mode, shape in (('gather', (0, 2, 12)), ('product', (0, 12))):
                xs = x5[:n].clone().requires_grad_(True)
                y = _fn(ssa, mode)(xs, links)
                assert y.shape == shape and y.dtype == torch.float32 and y.device == xs.device
                y.sum().backward()
                assert xs.grad.shape == (n, 12) and bool((_bits(xs.grad) == 0).all())
    assert ssa.link_gather(torch.zeros((0, 4), device=dev), none).shape == (0, 2, 4)
    assert ssa.link_hadamard(torch.zeros((3, 0), device=dev), torch.zeros((2, 2), dtype=torch.int64, device=dev)).shape == (2, 0)
    rng = np.random.RandomState(4)
    star = np.stack([np.full(300, 2), rng.randint(0, 5, 300)], axis=1)
    star[::2] = star[::2, ::-1]
    batches = [(1, np.zeros((600, 2), dtype=np.int64)), (1, np.zeros((1, 2), dtype=np.int64)), (5, np.full((600, 2), 3)), (5, star),
               (2, np.array([[0, 1], [1, 0], [1, 1]]))]
    for n, links in batches:
        links = np.ascontiguousarray(links, dtype=np.int64)
        g = lr.features(2 * len(links), 12, seed=6).reshape(len(links), 2, 12)
        tg, tlk = torch.from_numpy(g).to(dev), torch.from_numpy(links).to(dev)
        for hub in (256, None, 10 ** 9):
            plan = ssa.LinkBatch(n, tlk, hub_entries=hub)
            assert plan.n_hubs == (lr.slot_counts(links, n) > plan.hub_entries).sum()
            for mode in MODES:
                gm, hg = (tg, g) if mode == 'gather' else (tg[:, 0], g[:, 0])
                y, grad = _run(ssa, mode, x5[:n], plan, gm)
                _assert_same(y, _torch_forward(x5[:n], tlk, mode), f'N={n} L={len(links)} {mode}')
                _assert_same(grad, lr.grad(links, n, hg, None if mode == 'gather' else x5[:n].cpu().numpy()), f'N={n} L={len(links)} {mode} grad')
    ssa.link_decoder.check_errors()


# ---- offsets past 2^31 elements ---------------------------------------------------------------------------------------------------

def _formula(ids, F, a, b):
    """t[i, j] = ((a i + b j) mod 1021 - 510) / 64: exact in fp32, the same numbers on the host and on the device"""
    v = (a * np.asarray(ids, dtype=np.int64)[:, None] + b * np.arange(F, dtype=np.int64)[None, :]) % 1021 - 510
    return (v.astype(np.float32) / np.float32(64)).astype(np.float32)


def _fill(t, a, b):
    rows, F = t.shape
    cols = b * torch.arange(F, dtype=torch.int32, device=t.device)[None, :]  # (a * rows + b * F stays below 2^31)
    for r0 in range(0, rows, 1 << 18):
        ids = torch.arange(r0, min(r0 + (1 << 18), rows), dtype=torch.int32, device=t.device)[:, None]
        t[r0:r0 + (1 << 18)] = ((a * ids + cols) % 1021 - 510).to(torch.float32) / 64


def test_offsets_past_two_to_the_31_elements(ssa, dev):
    """N = 2 200 000, F = 1 024, L = 1 100 000: x, the [L, 2, F] output (with its grad_out) and grad_x hold 2.25e9 elements (9.0 GB)
    each, so element offsets pass 2^31 and byte offsets 2, 4 and 8 GiB (rows 524 288, 1 048 576 and 2 097 152 of x and grad_x, the
    slots of links 262 144, 524 288 and 1 048 576).  Random endpoints, with the first, the middle and the last link between rows 0 and
    N - 1 and the links at the boundaries on the rows at the boundaries; two dozen sampled rows against the restatement"""
    n, F, L = 2_200_000, 1024, 1_100_000
    lt.require_free_memory(dev, 5 * n * F * 4, 'the large-offset link decoder case')
    rng = np.random.RandomState(29)
    links = rng.randint(0, n, size=(L, 2)).astype(np.int64)
    bounds = [(1 << 31) // F // 4, (1 << 31) // F // 2, (1 << 31) // F]
    links[0], links[L // 2], links[L - 1] = (0, n - 1), (n - 1, 0), (0, n - 1)
    for b in bounds:
        links[b // 2 - 1], links[b // 2], links[b // 2 + 1] = (b - 1, 0), (b, b + 1), (n - 1, b)
    rows = np.unique(np.concatenate([[0, 1, n - 2, n - 1], [b + d for b in bounds for d in (-1, 0, 1)], links[[7, L - 7]].reshape(-1),
                                     bounds[2] + 2 + rng.choice(n - bounds[2] - 2, size=7, replace=False)]))
    assert 20 <= len(rows) <= 28 and (rows > bounds[2]).sum() >= 8
    sample = np.unique(np.concatenate([[0, 1, L // 2, L - 2, L - 1], [b // 2 + d for b in bounds for d in (-1, 0, 1)], rng.choice(L, size=10)]))
    tlk, trows, tsample = torch.from_numpy(links).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(sample).to(dev)
    plan = ssa.LinkBatch(n, tlk)
    m = lr.slot_counts(links, n)
    assert plan.num_touched == (m > 0).sum() and m[0] >= 5 and m[n - 1] >= 6 and plan.n_hubs == 0
    x = torch.empty((n, F), dtype=torch.float32, device=dev)
    assert x.numel() > 1 << 31
    _fill(x, 131, 7)
    _assert_same(x[trows], _formula(rows, F, 131, 7), 'the formula on the device')
    x.requires_grad_(True)
    x_rows = lambda ids: _formula(ids, F, 131, 7)

    y = ssa.link_gather(x, plan)
    assert y.shape == (L, 2, F) and y.numel() > 1 << 31
    _assert_same(y[tsample], x_rows(links[sample].reshape(-1)).reshape(-1, 2, F), 'large gather')
    g = torch.empty((2 * L, F), dtype=torch.float32, device=dev)
    _fill(g, 17, 3)
    y.backward(g.view(L, 2, F))
    del y
    _assert_same(x.grad[trows], lr.grad_rows(links, rows, lambda i: _formula(i, F, 17, 3), F), 'large gather, x.grad')
    untouched = torch.from_numpy(np.nonzero(m == 0)[0][[0, 1, -2, -1]]).to(dev)
    assert bool((_bits(x.grad[untouched]) == 0).all())
    x.grad = None

    y = ssa.link_hadamard(x, plan)
    _assert_same(y[tsample], x_rows(links[sample, 0]) * x_rows(links[sample, 1]), 'large product')
    y.backward(g[:L])
    del y
    _assert_same(x.grad[trows], lr.grad_rows(links, rows, lambda i: _formula(i, F, 17, 3), F, x_rows), 'large product, x.grad')
    del x, g, plan
    torch.cuda.empty_cache()
    ssa.link_decoder.check_errors()
