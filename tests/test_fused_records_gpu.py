"""The records form of the fused stage (ss_fused_hop_stage_records with a workspace, SS_FUSED_RECORDS=1: hop-2 HLL rows built by
scatter-max of the 64-byte hop-1 code records the HLL first hop leaves) against the dense form (SS_FUSED_RECORDS=0), the unfused
sequence (ss_first_hop + ss_propagate) and, at P = 128, the CPU oracle: both MinHash tables, both HLL tables and both cardinality
columns bit for bit, P = 64 and 128.  Built as tests/test_fused_rows_gpu.py, on ONE planted graph of 65 535 nodes (N % 4 = 3: the
last chunk is partial), run asymmetric as planted (no self-row skip: a row's own record is slot `deg`) and symmetrised (skip on), at
three hub thresholds.

What is planted (ids: feeders 1 000 .. 19 999 have no in-edge, sources from 20 000, destinations from 30 000 in chunks of four):
  * capacity -- sources whose closed neighbourhood (in-edges + the self loop) has 1, 2, 16, 17, 31, 32 codes (the record holds them)
    and 33, 34, 48 (the record says "read my dense row").  Each source is gathered by a destination that sees it alone, by one that
    sees it between unflagged feeders, and the `spread` chunks put a flagged source into a different slot of each of their four
    rows; one destination has flagged sources only.  Every such destination has at most 16 slots, so the slots that must take the
    records path follow from the planted degrees: CAPACITY_SLOTS states them per case and the host test asserts them.
  * slots -- destinations of 0, 1, K - 1, K, K + 1 slots (K = 16 slots are posted, the rest of a row is folded from dense rows) and a
    chunk whose rows have 1, 40, 3 and 16 entries.
  * codes -- a source with two feeders in ONE register at different ranks and one with two at equal ranks (ids found with the
    package's reference hash), and the node below 65 536 with the highest rank -- node 44 251, rank 16: bit 4 of the 6-bit field -- as a feeder.
  * self -- ids at and above max(edge_index) + 1 (no self loop, no edge: empty rows, empty records), a row that lists itself.
  * hubs -- hub threshold 1 000: every row regular; 40: the 48-code source is a hub row (flagged by the group that skips it, served
    by the hub units as a destination); 20: the 31- and 32-code sources too, flagged although their codes would fit.
The records themselves are read back through the entry point: scatter-max of a record = the dense hop-1 row of every unflagged node,
sixteen zeros for an empty row, the marker in dword 0 of the flagged ones."""
import functools
from argparse import Namespace
from ctypes import byref

import numpy as np
import pytest
import torch

import hll_planted as hp

gpu = pytest.mark.gpu

N = 65535
M = 256
K = 16             # slots the records form posts per row
CODES = 32         # codes a record holds
MARKER = 0xFFFFFFFF
LAST = 60000       # the highest id an edge names: ids 60 001 .. N - 1 have no self loop
FEED0, SRC0, DST0 = 1000, 20000, 30000
FITS, FLAGGED = (1, 2, 16, 17, 31, 32), (33, 34, 48)
THRESHOLDS = (1000, 40, 20)


@functools.lru_cache(maxsize=None)
def hop0():
    """(register, rank) of every node's single hop-0 register, from the package's reference hash on the CPU"""
    from oracle import oracle
    x = oracle.hll_init(65536, 8)
    assert ((x != 0).sum(axis=1) == 1).all()
    return np.argmax(x, axis=1), x.max(axis=1).astype(np.int64)


class Plan:
    def __init__(self):
        self.src, self.dst = [], []
        self.next_feeder, self.next_source, self.next_dest = FEED0, SRC0, DST0
        self.sources, self.cases, self.named = {}, {}, {}

    def feeders(self, k):
        out = list(range(self.next_feeder, self.next_feeder + k))
        self.next_feeder += k
        assert self.next_feeder <= SRC0
        return out

    def edge(self, s, d):
        self.src.append(s)
        self.dst.append(d)

    def source(self, codes, feeders=None):
        """a node whose closed neighbourhood has `codes` members: codes - 1 in-edges and its self loop"""
        s = self.next_source
        self.next_source += 1
        for f in (feeders if feeders is not None else self.feeders(codes - 1)):
            self.edge(f, s)
        return s

    def chunk(self, rows):
        """four consecutive destinations from a multiple of four; rows: the in-neighbours of each"""
        assert len(rows) == 4 and self.next_dest % 4 == 0
        first = self.next_dest
        self.next_dest += 4
        for k, row in enumerate(rows):
            for s in row:
                self.edge(s, first + k)
        return first


@functools.lru_cache(maxsize=None)
def planted():
    reg, rank = hop0()
    p = Plan()
    for c in FITS + FLAGGED:
        p.sources[c] = p.source(c)
    spare = {c: p.source(c) for c in FLAGGED}  # a second flagged source of each size
    # capacity: alone / between unflagged feeders, one chunk per source (rows 2 and 3: a feeder alone, no entry)
    for c in FITS + FLAGGED:
        s = p.sources[c]
        first = p.chunk([[s], p.feeders(5) + [s] + p.feeders(4), p.feeders(1), []])
        p.cases[('alone', c)] = first
        p.cases[('mixed', c)] = first + 1
    # a flagged source in a different slot of each of the four rows (the CSR orders a row's sources as it likes: what is asserted is
    # the NUMBER of flagged slots per row, and that the rows differ in where the flagged id sorts among the others)
    for c in FLAGGED:
        s = p.sources[c]
        low, high = p.feeders(12), list(range(SRC0 + 5000 + 16 * c, SRC0 + 5000 + 16 * c + 12))
        p.cases[('spread', c)] = p.chunk([[s] + high[:3], low[:1] + [s] + high[:2], low[:2] + [s] + high[:1], low[:3] + [s]])
    p.cases['only_flagged'] = p.chunk([[p.sources[33], p.sources[34], p.sources[48]], [spare[33], spare[48]], p.feeders(2), [spare[34]]])
    # slots: 0 entries, K - 2 / K - 1 / K entries (+ the own row: K - 1, K, K + 1 slots when asymmetric), and a ragged chunk
    p.cases['slots'] = p.chunk([[], p.feeders(K - 2), p.feeders(K - 1), p.feeders(K)])
    p.cases['ragged'] = p.chunk([p.feeders(1), p.feeders(40), p.feeders(3), p.feeders(16)])
    # codes: two feeders of one source in the same register -- different ranks, equal ranks
    pool = np.arange(FEED0 + 15000, SRC0)
    by = {}
    diff = same = None
    for f in pool:
        for g in by.get(int(reg[f]), []):
            if rank[g] != rank[f] and diff is None and not (same and {int(g), int(f)} & set(same)):
                diff = (int(g), int(f))
            if rank[g] == rank[f] and same is None and not (diff and {int(g), int(f)} & set(diff)):
                same = (int(g), int(f))
        by.setdefault(int(reg[f]), []).append(f)
    assert diff and same and not set(diff) & set(same)
    p.named['same_register'] = (p.source(3, diff), p.source(3, same))
    top = int(np.argmax(rank[:65536]))
    p.named['top_rank'] = (top, int(rank[top]))
    s_top = p.source(2, [top])
    p.cases['codes'] = p.chunk([[p.named['same_register'][0]], [p.named['same_register'][1]], [s_top], [top]])
    # self: a row that lists itself (once), next to rows that do not
    first = p.chunk([p.feeders(2), [], p.feeders(1), p.feeders(3)])
    p.edge(first + 1, first + 1)
    p.cases['lists_itself'] = first + 1
    p.edge(LAST, DST0 - 1)  # the highest id named: no self loop from LAST + 1 on
    ei = np.array([p.src, p.dst], dtype=np.int64)
    return ei, p


def edges(form):
    ei, _ = planted()
    return ei if form == 'asym' else np.concatenate([ei, ei[::-1]], axis=1)


def totals(ei, n_self):
    """closed-neighbourhood size of every node as the first hop counts it: in-edges + the self loop of ids below n_self"""
    return np.bincount(ei[1], minlength=N) + (np.arange(N) < n_self)


def record_slots(ei, d, threshold):
    """asymmetric form, destination d of at most K slots -> (slots served from records, slots served from dense rows)"""
    n_self = int(ei.max()) + 1
    tot, deg = totals(ei, n_self), np.bincount(ei[1], minlength=N)
    nbrs = ei[0][ei[1] == d].tolist() + ([d] if d < n_self else [])
    assert len(nbrs) <= K
    dense = sum(1 for j in nbrs if tot[j] > CODES or deg[j] > threshold)
    return len(nbrs) - dense, dense


# per capacity case: (records slots, dense slots) at hub thresholds 1 000 / 40 / 20 -- from the planted degrees alone: the destination
# `alone` has the source and itself, `mixed` nine feeders, the source and itself
def CAPACITY_SLOTS(kind, c, threshold):
    flagged = c > CODES or c - 1 > threshold
    return {'alone': (2 - flagged, int(flagged)), 'mixed': (11 - flagged, int(flagged))}[kind]


def test_the_graph_plants_what_it_claims():
    reg, rank = hop0()
    ei, p = planted()
    assert N % 4 == 3 and int(ei.max()) == LAST and N - 1 > LAST
    tot = totals(ei, LAST + 1)
    deg = np.bincount(ei[1], minlength=N)
    for c, s in p.sources.items():
        assert tot[s] == c, (c, int(tot[s]))
    assert not deg[FEED0:SRC0].any() and (tot[FEED0:SRC0] == 1).all()       # feeders: one code, their own
    assert not tot[LAST + 1:].any()                                            # beyond the last named id: empty rows, total 0
    for threshold in THRESHOLDS:
        for c in FITS + FLAGGED:
            for kind in ('alone', 'mixed'):
                assert record_slots(ei, p.cases[(kind, c)], threshold) == CAPACITY_SLOTS(kind, c, threshold), (kind, c, threshold)
        for c in FLAGGED:  # one flagged slot in each of the four rows, five slots per row
            first = p.cases[('spread', c)]
            assert [record_slots(ei, first + k, threshold) for k in range(4)] == [(4, 1)] * 4
            below = [int((ei[0][ei[1] == first + k] < p.sources[c]).sum()) for k in range(4)]
            assert below == [0, 1, 2, 3]                                       # the flagged id sorts into a different place of each row
        first = p.cases['only_flagged']
        assert record_slots(ei, first, threshold) == (1, 3) and record_slots(ei, first + 1, threshold) == (1, 2)
        assert record_slots(ei, first + 3, threshold) == (1, 1) and record_slots(ei, first + 2, threshold) == (3, 0)
    # which sources are hub rows at which threshold
    assert [c for c in FITS + FLAGGED if c - 1 > 40] == [48] and [c for c in FITS + FLAGGED if c - 1 > 20] == [31, 32, 33, 34, 48]
    first = p.cases['slots']
    assert (tot[first:first + 4] == [1, K - 1, K, K + 1]).all() and deg[first] == 0
    first = p.cases['ragged']
    assert deg[first:first + 4].tolist() == [1, 40, 3, 16]
    a, b = p.named['same_register']
    fa, fb = ei[0][ei[1] == a], ei[0][ei[1] == b]
    assert reg[fa[0]] == reg[fa[1]] and rank[fa[0]] != rank[fa[1]] and reg[fb[0]] == reg[fb[1]] and rank[fb[0]] == rank[fb[1]]
    top, r = p.named['top_rank']
    assert (top, r) == (44251, 16) and r == rank[:65536].max() and top < LAST and (ei[0] == top).sum() == 2
    d = p.cases['lists_itself']
    assert ((ei[0] == d) & (ei[1] == d)).sum() == 1
    sym = edges('sym')
    key = lambda e: set(zip(e[0].tolist(), e[1].tolist()))
    assert key(sym) == key(sym[::-1]) and key(ei) != key(ei[::-1])


# ---- the sequences ---------------------------------------------------------------------------------------------------------------------
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
    eh.hll_tables = hp.tables(8)
    return eh


_unfused = {}


def unfused(ssa, dev, form, P, threshold):
    """ss_first_hop + ss_propagate, once per graph, P and threshold"""
    key = (form, P, threshold)
    if key not in _unfused:
        table, cards = _eh(ssa, P, fuse_hop_stage=False).build_hash_tables(N, torch.from_numpy(edges(form)).to(dev))
        torch.cuda.synchronize()
        _unfused[key] = (table[1].mh_u32.clone(), table[1].hll_u8.clone(), table[2].mh_u32.clone(), table[2].hll_u8.clone(), cards.clone())
    return _unfused[key]


def stage(ssa, dev, form, P, with_records=True, hub_list=True):
    """ss_fused_hop_stage_records on the graph -> (mh1, hll1, mh2, hll2, cards, records); hop-2 MinHash is part of it at P = 128 only.
    hub_list=False: the graph is handed over without its hub list, as the engine hands over a shape that had no hub row before"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    ei = edges(form)
    eh = _eh(ssa, P)
    csr = ssa.hashing.build_csr(torch.from_numpy(ei).to(dev), N, dev, check=False)
    csr.use_inferred_self_loops = True
    if not hub_list:
        csr.has_hub_rows = False
    graph = csr.struct()
    ab, params = eh._perms(dev), eh._params(dev)
    mh = [torch.full((N, P), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    hll = [torch.full((N, M), 255, dtype=torch.uint8, device=dev) for _ in range(2)]
    cards = torch.full((N, 2), -1.0, dtype=torch.float32, device=dev)
    records = torch.full((N, 16), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rc = ssa._native.lib().ss_fused_hop_stage_records(byref(graph), _ptr(ab[0]), _ptr(ab[1]), P, _ptr(mh[0]), _ptr(mh[1]) if P == 128 else None,
                                                      8, _ptr(hll[0]), _ptr(cards), _ptr(hll[1]), _ptr(cards[:, 1]), 2, byref(params.struct),
                                                      _ptr(records) if with_records else None, ei.shape[1], _stream(dev))
    assert rc == 0, f'ss_fused_hop_stage_records returned {rc}'
    torch.cuda.synchronize()
    return mh[0], hll[0], mh[1], hll[1], cards, records


@functools.lru_cache(maxsize=None)
def _oracle_tables(form):
    from oracle import oracle
    return oracle.build_hash_tables(N, edges(form), 2, 128, hp.oracle_params(hp.tables(8)))


def _same(got, want, P, what):
    assert torch.equal(got[0], want[0]), f'hop-1 MinHash, {what}'
    assert torch.equal(got[1], want[1]), f'hop-1 HLL, {what}'
    assert torch.equal(got[3], want[3]), f'hop-2 HLL, {what}'
    assert torch.equal(got[4].view(torch.int32), want[4].view(torch.int32)), f'cards of hops 1 and 2, {what}'
    if P == 128:
        assert torch.equal(got[2], want[2]), f'hop-2 MinHash, {what}'


@gpu
@pytest.mark.parametrize('threshold', THRESHOLDS)
@pytest.mark.parametrize('P', [64, 128])
@pytest.mark.parametrize('form', ['asym', 'sym'])
def test_records_form_equals_dense_unfused_and_oracle(ssa, dev, monkeypatch, form, P, threshold):
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', threshold)
    for name in ('SS_FUSED_POSTS', 'SS_SELF_SKIP', 'SS_FUSED_RECORDS'):
        monkeypatch.delenv(name, raising=False)
    want = unfused(ssa, dev, form, P, threshold)
    monkeypatch.setenv('SS_FUSED_RECORDS', '0')
    dense = stage(ssa, dev, form, P)
    assert (dense[5] == 0x5A5A5A5A).all(), 'the dense form leaves the workspace alone'
    monkeypatch.setenv('SS_FUSED_RECORDS', '1')
    got = stage(ssa, dev, form, P)
    _same(got, dense, P, 'records against dense')
    _same(got, want, P, 'records against the unfused sequence')
    _same(stage(ssa, dev, form, P, with_records=False), dense, P, 'no workspace: the dense form')
    if P == 128:
        otab, ocards = _oracle_tables(form)
        for k, (mh, hll) in enumerate(((got[0], got[1]), (got[2], got[3])), start=1):
            assert np.array_equal(mh.cpu().numpy().view(np.uint32), otab[k]['minhash']), f'hop-{k} MinHash against the oracle'
            assert np.array_equal(hll.cpu().numpy(), otab[k]['hll']), f'hop-{k} HLL against the oracle'
        np.testing.assert_allclose(got[4].cpu().numpy(), ocards, rtol=hp.RTOL, atol=1e-4)
    # the records themselves
    ei = edges(form)
    n_self = int(ei.max()) + 1
    tot, deg = totals(ei, n_self), np.bincount(ei[1], minlength=N)
    rec = got[5].cpu().numpy().view(np.uint32)
    flagged = (tot > CODES) | (deg > threshold)
    assert (rec[flagged, 0] == MARKER).all() and not (rec[~flagged, 0] == MARKER).any(), 'the marker, on the flagged nodes alone'
    assert not rec[tot == 0].any() and (tot == 0).sum() >= N - 1 - LAST, 'an empty row is sixteen zeros'
    assert not (rec[~flagged] & 3).any(), 'no code has its low two bits set'
    image = np.zeros((N, M), np.uint8)
    for half in (rec & 0xFFFF, rec >> 16):
        r, v = (half >> 2) & 0xFF, (half >> 10).astype(np.uint8)
        rows = np.broadcast_to(np.arange(N)[:, None], r.shape)
        np.maximum.at(image, (rows[~flagged], r[~flagged]), v[~flagged])
    assert np.array_equal(image[~flagged], got[1].cpu().numpy()[~flagged]), 'scatter-max of a record = the dense hop-1 row'
    assert ((rec[~flagged] & 0xFFFF) != 0).sum() + ((rec[~flagged] >> 16) != 0).sum() == tot[~flagged].sum(), 'one code per neighbour'
    _, p = planted()
    top, r = p.named['top_rank']
    assert got[1][top].max().item() == r


@gpu
def test_the_sparsity_rule_and_the_switch(ssa, dev, monkeypatch):
    """without SS_FUSED_RECORDS the library decides: E + N <= 24 N on a graph handed over without a hub list takes the records form (the
    workspace is written); a larger E, or a hub list, the dense form (it is not); results are the same either way"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    monkeypatch.setattr(ssa.knobs, 'HUB_THRESHOLD', 1000)
    for name in ('SS_FUSED_POSTS', 'SS_SELF_SKIP', 'SS_FUSED_RECORDS'):
        monkeypatch.delenv(name, raising=False)
    ei = edges('asym')
    assert ei.shape[1] + N <= 24 * N
    got = stage(ssa, dev, 'asym', 64, hub_list=False)
    assert not (got[5] == 0x5A5A5A5A).any(), 'every record written'
    want = unfused(ssa, dev, 'asym', 64, 1000)
    _same(got, want, 64, 'the library chose records')
    listed = stage(ssa, dev, 'asym', 64)
    assert (listed[5] == 0x5A5A5A5A).all(), 'a hub list: dense'
    _same(listed, want, 64, 'the library chose dense')
    eh = _eh(ssa, 64)
    csr = ssa.hashing.build_csr(torch.from_numpy(ei).to(dev), N, dev, check=False)
    csr.use_inferred_self_loops = True
    csr.has_hub_rows = False
    graph = csr.struct()
    ab, params = eh._perms(dev), eh._params(dev)
    mh = torch.empty((N, 64), dtype=torch.int32, device=dev)
    hll = [torch.empty((N, M), dtype=torch.uint8, device=dev) for _ in range(2)]
    cards = torch.empty((N, 2), dtype=torch.float32, device=dev)
    records = torch.full((N, 16), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rc = ssa._native.lib().ss_fused_hop_stage_records(byref(graph), _ptr(ab[0]), _ptr(ab[1]), 64, _ptr(mh), None, 8, _ptr(hll[0]), _ptr(cards),
                                                      _ptr(hll[1]), _ptr(cards[:, 1]), 2, byref(params.struct), _ptr(records), 23 * N + 1,
                                                      _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0 and (records == 0x5A5A5A5A).all(), 'E + N > 24 N: dense'
    assert torch.equal(hll[1], want[3]) and torch.equal(mh, want[0])
