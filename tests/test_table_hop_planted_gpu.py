"""The table hops on the witness tables of tests/table_hop_planted.py: every entry of every row under test decides a word of the output
(test_table_hop_planted_host.py proves it), so a walk that drops an entry, reads it at the wrong chunk, folds it into the wrong word or
folds one too many cannot pass.  Every comparison of tables is exact equality of WHOLE tables -- rows under test, pool rows, fillers -- with
the numpy reference want_rows, over output buffers pre-filled with a sentinel; a mismatch names entry point, round, row, word, the value got
and wanted and the position the wrong value encodes.

Entry points: ss_propagate (MinHash alone: propagate_kernel<128, 256> and its hosted hub units; HLL alone: hll_propagate_row16_kernel;
both; the run-time-sized propagate_kernel<0, 0> in every sub-group form; row ranges), ss_minhash_hop_rows, ss_fused_hop_stage in its input
form (cards1_out == NULL: hll1 is the caller's), the symmetric variant, and SS_HUB_LAUNCHES=1 in a child process.  Cardinalities by the
criterion of test_hll_planted_gpu._check_counts (bits where the harmonic sum is exact, the oracle at the project's RTOL elsewhere)."""
import functools
import hashlib
import os
import subprocess
import sys
from argparse import Namespace
from ctypes import byref
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hll_planted as hp
import table_hop_planted as tp
from test_hll_planted_gpu import RTOL, _check_counts

pytestmark = pytest.mark.gpu

SENT_MH, SENT_HLL, SENT_CARD = 0x5A5A5A5A, 0xA5, -1.0
S = tp.MEGA_SLICE


@pytest.fixture(scope='module')
def ssa():
    import subgraph_sketching_amd as m
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    m._native.lib()
    assert m._native.MEGA_SLICE == S
    return m


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for name in ('SS_FUSED_POSTS', 'SS_SELF_SKIP', 'SS_FUSED_RECORDS'):
        monkeypatch.delenv(name, raising=False)
    assert os.environ.get('SS_HUB_LAUNCHES', '0') in ('', '0'), 'the hosted hub units are what these tests run in this process'


@functools.lru_cache(maxsize=None)
def _eh(ssa, P, p):
    eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=p, minhash_num_perm=P, floor_sf=False, use_zero_one=True))
    eh.hll_tables = hp.tables(p, None)
    return eh


class World(object):
    """a planted graph built by the engine (check=True, hub threshold 40), its CSR read back, the hub plan asserted"""

    def __init__(self, ssa, dev, g):
        self.ssa, self.dev, self.g, self.N = ssa, dev, g, g.n
        E = g.edge_index.shape[1]
        self.csr = ssa.hashing.build_csr(torch.from_numpy(g.edge_index).to(dev), g.n, dev, check=True, hub_threshold=tp.HUB_THRESHOLD)
        torch.cuda.synchronize()
        self.rowptr, self.col = self.csr.rowptr.cpu().numpy(), self.csr.col.cpu().numpy()[:E]
        assert tp.is_csr_of(self.rowptr, self.col, g.edge_index, g.n), 'the CSR holds the edges'
        assert int(self.csr.n_self_dev.item()) == g.n_self
        deg = np.diff(self.rowptr)
        self.hub_rows = np.sort(self.csr.hub_rows[:int(self.csr.hub_count.item())].cpu().numpy().astype(np.int64))
        n_mega, n_slices = (int(x) for x in self.csr.mega_count.cpu().tolist())
        desc = self.csr.mega_rows[:n_mega].cpu().numpy()
        desc = desc[np.argsort(desc[:, 0])]
        self.mega_rows, self.n_mega = desc[:, 0].astype(np.int64), n_mega
        # the plan the shapes intend: which rows came out as hub rows, which as mega rows and with how many slices
        assert np.array_equal(self.hub_rows, np.flatnonzero((deg > tp.HUB_THRESHOLD) & (deg <= S)))
        assert np.array_equal(self.mega_rows, np.flatnonzero(deg > S))
        assert desc[:, 2].tolist() == [tp.slices_of(int(d)) for d in deg[self.mega_rows]] and n_slices == int(desc[:, 2].sum())
        if n_mega:  # (first slices: the rows' slices laid end to end, in whatever order the build appended them)
            assert sorted(desc[:, 1].tolist()) == np.concatenate([[0], np.cumsum(desc[np.argsort(desc[:, 1]), 2])[:-1]]).tolist()
        assert self.csr.has_hub_rows == bool(len(self.hub_rows) or n_mega)
        self.units = np.concatenate([self.hub_rows, self.mega_rows])
        self._plans = {}
        self.tickets = torch.zeros((), dtype=torch.bool, device=dev)

    def plan(self, self_loops, skip=False, hubs=True):
        key = (bool(self_loops), bool(skip), bool(hubs) and skip)
        if key not in self._plans:
            self._plans[key] = tp.Plan(self.rowptr, self.col, self.g.n_test, self.g.n_self if self_loops else 0, skip=skip,
                                       hub_rows=self.units if (skip and hubs) else ())
        return self._plans[key]

    def setting(self, self_loops, hubs):
        """the self loops of the next launches, and whether they see the hub list (withheld: every row is a regular row's walk)"""
        self.csr.use_inferred_self_loops = bool(self_loops)
        self.csr.has_hub_rows = bool(hubs) and bool(len(self.units))

    def note_tickets(self):
        """after every launch the ticket words of the mega rows (descriptor words 3 and 4) are zero; read once, at the end"""
        if self.n_mega:
            self.tickets |= self.csr.mega_rows[:self.n_mega, 3:5].any()

    def tickets_clean(self):
        return not bool(self.tickets.item())

    def propagate(self, mh_in=None, hll_in=None, cards=False, rows=None, hop_tables=False, p=8):
        """ss_propagate over sentinel-filled outputs -> (mh_out, hll_out, cards)"""
        dev = self.dev
        mh_out = torch.full_like(mh_in, _i32(SENT_MH)) if mh_in is not None else None
        hll_out = torch.full_like(hll_in, SENT_HLL) if hll_in is not None else None
        c = torch.full((self.N,), SENT_CARD, dtype=torch.float32, device=dev) if cards else None
        params = _eh(self.ssa, 128, p)._params(dev) if cards else None
        self.ssa.hashing._propagate(self.csr, mh_in, hll_in, dev, cards_out=c, cards_stride=1 if cards else 0, params=params, mh_out=mh_out,
                                    hll_out=hll_out, rows=rows, hop_tables=hop_tables)
        self.note_tickets()
        return mh_out, hll_out, c


def _i32(v):
    return int(np.array(v, dtype=np.uint32).view(np.int32))


@functools.lru_cache(maxsize=None)
def _world(ssa, dev, which):
    g = {'main': tp.main_graph, 'generic': tp.generic_graph, 'generic_wide': lambda: tp.generic_graph(True), 'symmetric': tp.symmetric_graph}[which]()
    return World(ssa, dev, g)


def _dev(a, dev):
    """a planted table on the device: uint32 as the int32 the engine's tensors are"""
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


class Round(object):
    """one round's input and expected tables of a sketch, on the host and on the device"""

    def __init__(self, plan, sketch, kind, k, W, dev):
        self.sketch, self.kind, self.k = sketch, kind, k
        self.table = plan.table(sketch, kind, k, W)
        self.want = plan.want(sketch, self.table)
        self.d_in, self.d_want = _dev(self.table, dev), _dev(self.want, dev)
        self.sentinel = _i32(SENT_MH) if sketch == 'minhash' else SENT_HLL

    def check(self, got, what, rows=None):
        """got == want_rows exactly; rows = (lo, hi) or an index array: those rows, and the sentinel everywhere else"""
        want_t = self.d_want
        if rows is not None:
            want_t = torch.full_like(self.d_want, self.sentinel)
            sel = slice(*rows) if isinstance(rows, tuple) else torch.as_tensor(np.asarray(rows, dtype=np.int64), device=got.device)
            want_t[sel] = self.d_want[sel]
        if torch.equal(got, want_t):
            return
        raise AssertionError(tp.first_difference(_host(got), _host(want_t), self.sketch, self.kind, self.k, what))


@functools.lru_cache(maxsize=None)
def _estimator(p):
    t = hp.tables(p, None)
    return t, hp.params(t), hp.oracle_params(t)


def _check_cards(got, r, p, what, rows):
    """cardinalities of the rows in `rows` (an index array) of round r (anything with the expected HLL table as `want`): all against the oracle at the
    project's RTOL -- the bar _check_counts applies where the harmonic sum is not exact -- and the first 400, the rows under test among
    them, by _check_counts itself (bit for bit where the sum is exact)"""
    from oracle import oracle
    t, prm, oprm = _estimator(p)
    want_hll = r.want
    if getattr(r, 'oracle_cards', None) is None:  # (once per round, whatever the number of launches compared with it)
        r.oracle_cards = oracle.hll_count(want_hll, oprm)
    ref = r.oracle_cards
    got = got.cpu().numpy()
    np.testing.assert_allclose(got[rows], ref[rows], rtol=RTOL, atol=0, err_msg=what)
    _check_counts(got[rows[:400]], want_hll[rows[:400]], t, prm, what)


def _cuts(world):
    """row ranges that cut between hub rows and through the mega rows' ids"""
    a, b = int(world.hub_rows[len(world.hub_rows) // 2]), int(world.mega_rows[len(world.mega_rows) // 2])
    assert 0 < a < b < world.N
    return [(0, a), (a, b), (b, world.N)]


# ---- ss_propagate, one sketch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('self_loops', [True, False])
def test_minhash_table_hop(ssa, dev, self_loops):
    """propagate_kernel<128, 256>: minhash_walk128 on the regular rows (with the hub list withheld on every row, the 1 025- and
    3 137-entry rows included), the hub and mega units hosted by the leading workgroups (4 wavefronts), and row ranges"""
    w = _world(ssa, dev, 'main')
    plan = w.plan(self_loops)
    for kind, k in plan.rounds(128):
        r = Round(plan, 'minhash', kind, k, 128, dev)
        for hubs in (True, False):
            w.setting(self_loops, hubs)
            r.check(w.propagate(mh_in=r.d_in)[0], f'ss_propagate MinHash alone, self_loops={self_loops} hub list {"given" if hubs else "withheld"}')
        w.setting(self_loops, True)
        for lo, hi in _cuts(w):
            r.check(w.propagate(mh_in=r.d_in, rows=(lo, hi))[0], f'ss_propagate MinHash alone, rows [{lo}, {hi}) self_loops={self_loops}', rows=(lo, hi))
    assert w.tickets_clean()


@pytest.mark.parametrize('self_loops', [True, False])
def test_hll_table_hop(ssa, dev, self_loops):
    """hll_propagate_row16_kernel: the DPP head, the solo walk to 32, the four-group walk of long rows dealt in degree order; its hosted
    hub and mega units; cardinalities; row ranges"""
    w = _world(ssa, dev, 'main')
    plan = w.plan(self_loops)
    everyone = np.arange(w.N)
    for kind, k in plan.rounds(256):
        r = Round(plan, 'hll', kind, k, 256, dev)
        for hubs in (True, False):
            w.setting(self_loops, hubs)
            what = f'ss_propagate HLL alone, self_loops={self_loops} hub list {"given" if hubs else "withheld"}'
            _, got, cards = w.propagate(hll_in=r.d_in, cards=True)
            r.check(got, what)
            _check_cards(cards, r, 8, f'{what}, {kind} round {k}: cardinalities', everyone)
        w.setting(self_loops, True)
        for lo, hi in _cuts(w):
            what = f'ss_propagate HLL alone, rows [{lo}, {hi}) self_loops={self_loops}'
            _, got, cards = w.propagate(hll_in=r.d_in, cards=True, rows=(lo, hi))
            r.check(got, what, rows=(lo, hi))
            c = cards.cpu().numpy()
            assert (c[:lo] == SENT_CARD).all() and (c[hi:] == SENT_CARD).all(), what
            _check_cards(cards, r, 8, f'{what}, {kind} round {k}: cardinalities', np.arange(lo, hi))
    assert w.tickets_clean()


def _paired(plan, P, M):
    """[(minhash round, hll round)]: the longer list of rounds, the shorter one repeated"""
    a, b = plan.rounds(P), plan.rounds(M)
    n = max(len(a), len(b))
    return [(a[q % len(a)], b[q % len(b)]) for q in range(n)]


@pytest.mark.parametrize('self_loops', [True, False])
def test_both_sketches_at_the_fast_shape(ssa, dev, self_loops):
    """ss_propagate with P = 128 and M = 256 in one call: two launches, each hosting the hub units of its own sketch"""
    w = _world(ssa, dev, 'main')
    plan = w.plan(self_loops)
    w.setting(self_loops, True)
    everyone = np.arange(w.N)
    for (mk, mi), (hk, hi) in _paired(plan, 128, 256):
        rm, rh = Round(plan, 'minhash', mk, mi, 128, dev), Round(plan, 'hll', hk, hi, 256, dev)
        mh, hll, cards = w.propagate(mh_in=rm.d_in, hll_in=rh.d_in, cards=True)
        rm.check(mh, f'ss_propagate both sketches (MinHash side), self_loops={self_loops}')
        rh.check(hll, f'ss_propagate both sketches (HLL side), self_loops={self_loops}')
        _check_cards(cards, rh, 8, f'ss_propagate both sketches, {hk} round {hi}: cardinalities', everyone)
    assert w.tickets_clean()


# ---- the run-time-sized kernel ------------------------------------------------------------------------------------------------------------
# (P, M, p of the cardinalities or None, graph): sub-groups of 1 lane (P = 4, M = 16), of 4 with an idle lane (P = 12), of 16, 32 and 64,
# more than one pass (P = 260 and 2 048, M = 2 048 and 65 536)
GENERIC = [(4, 16, 4, 'generic'), (12, 64, None, 'generic'), (64, 256, None, 'generic'), (128, 512, None, 'generic'), (256, 1024, 10, 'generic'),
           (260, 2048, None, 'generic'), (2048, 128, None, 'generic'), (256, 65536, None, 'generic_wide')]


@pytest.mark.parametrize('P,M,p,which', GENERIC)
def test_generic_kernel_both_sketches_in_one_launch(ssa, dev, P, M, p, which):
    """propagate_kernel<0, 0>: both sketches in ONE launch, every row a wavefront's (no hub units), with and without self loops"""
    w = _world(ssa, dev, which)
    everyone = np.arange(w.N)
    for self_loops in (True, False):
        plan = w.plan(self_loops)
        w.setting(self_loops, True)
        for (mk, mi), (hk, hi) in _paired(plan, P, M):
            rm, rh = Round(plan, 'minhash', mk, mi, P, dev), Round(plan, 'hll', hk, hi, M, dev)
            mh, hll, cards = w.propagate(mh_in=rm.d_in, hll_in=rh.d_in, cards=p is not None, p=p or 8)
            rm.check(mh, f'ss_propagate generic P={P} M={M} (MinHash side), self_loops={self_loops}')
            rh.check(hll, f'ss_propagate generic P={P} M={M} (HLL side), self_loops={self_loops}')
            if p is not None:
                _check_cards(cards, rh, p, f'ss_propagate generic P={P} M={M}, {hk} round {hi}: cardinalities', everyone)


# ---- ss_minhash_hop_rows ------------------------------------------------------------------------------------------------------------------
def _row_list(w):
    """rows under test at chosen places, a repeated id, negative ids, ids outside [-N, N) -> (the list, the valid rows it names)"""
    g, N = w.g, w.N
    picks = [0, 1, 5, g.n_test - 1, g.n_test, N - 1, 66, 67, 64]
    picks += [int(x[q]) for x, q in ((w.hub_rows, 0), (w.mega_rows, -1)) if len(x)]
    picks += [int(i) for i in np.flatnonzero(np.isin(g.degrees, (63, 64, 65, 128, 200, 300)))]
    lst = picks + [picks[1]] + [3 - N, 9 - N, -1] + [N, N + 5, -N - 1, 1 << 40, -(1 << 40)]
    if len(lst) % 4 == 0:
        lst.append(2)
    valid = sorted({i % N for i in lst if -N <= i < N})
    return np.array(lst, dtype=np.int64), np.array(valid, dtype=np.int64)


@pytest.mark.parametrize('P,which', [(128, 'main'), (12, 'generic'), (260, 'generic')])
def test_minhash_hop_rows(ssa, dev, P, which):
    """the listed rows -- and, at P = 128, every hub and mega row -- equal want_rows; all other rows keep the sentinel"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    w = _world(ssa, dev, which)
    lst, valid = _row_list(w)
    d_lst = torch.from_numpy(lst).to(dev)
    for self_loops in (True, False):
        plan = w.plan(self_loops)
        for hubs in ((True, False) if P == 128 else (True,)):
            w.setting(self_loops, hubs)
            graph = w.csr.struct()
            written = np.union1d(valid, w.units) if (P == 128 and hubs) else valid
            for kind, k in plan.rounds(P):
                r = Round(plan, 'minhash', kind, k, P, dev)
                out = torch.full_like(r.d_in, _i32(SENT_MH))
                rc = ssa._native.lib().ss_minhash_hop_rows(byref(graph), _ptr(r.d_in), _ptr(out), P, _ptr(d_lst), len(lst), _stream(dev))
                assert rc == 0
                w.note_tickets()
                r.check(out, f'ss_minhash_hop_rows P={P}, self_loops={self_loops} hub list {"given" if hubs else "withheld"}', rows=written)
    assert w.tickets_clean()


# ---- the fused stage in its input form ----------------------------------------------------------------------------------------------------
def _fused(w, P, hll1, with_mh2):
    """ss_fused_hop_stage with cards1_out == NULL (hll1 is the caller's table) -> (hll2, cards2)"""
    from subgraph_sketching_amd._runtime import _ptr, _stream
    ssa, dev, N = w.ssa, w.dev, w.N
    eh = _eh(ssa, P, 8)
    ab, params = eh._perms(dev), eh._params(dev)
    graph = w.csr.struct()
    mh1 = torch.empty((N, P), dtype=torch.int32, device=dev)
    mh2 = torch.empty((N, P), dtype=torch.int32, device=dev) if with_mh2 else None
    hll2 = torch.full_like(hll1, SENT_HLL)
    cards = torch.full((N,), SENT_CARD, dtype=torch.float32, device=dev)
    rc = ssa._native.lib().ss_fused_hop_stage(byref(graph), _ptr(ab[0]), _ptr(ab[1]), P, _ptr(mh1), _ptr(mh2), 8, _ptr(hll1), None, _ptr(hll2),
                                              _ptr(cards), 1, byref(params.struct), _stream(dev))
    assert rc == 0, f'ss_fused_hop_stage returned {rc}'
    w.note_tickets()
    return hll2, cards


@pytest.mark.parametrize('posts', ['unset', 'flat'])
@pytest.mark.parametrize('self_loops', [True, False])
def test_fused_stage_folds_a_planted_hop1_table(ssa, dev, monkeypatch, self_loops, posts):
    """the HLL side of fused_hop_persistent_kernel (7 register landings, 7 LDS landings, the walks behind them, every pattern of long rows
    among a wavefront's four) at P = 64 and P = 128, and the hop-2 HLL hub units in both of their homes: hosted by the second half of the
    leading workgroups of the MinHash hop (mh2_out, P = 128) and served by the hub launch (mh2_out NULL).  The stage never skips a self
    row over a table it did not build.  Only hll2_out and cards2_out are compared: the MinHash outputs come from node ids"""
    if posts == 'flat':
        monkeypatch.setenv('SS_FUSED_POSTS', 'flat')
    w = _world(ssa, dev, 'main')
    plan = w.plan(self_loops)
    everyone = np.arange(w.N)
    for kind, k in plan.rounds(256):
        r = Round(plan, 'hll', kind, k, 256, dev)
        for P, with_mh2 in ((64, False), (128, True), (128, False)):
            for hubs in (True, False):
                w.setting(self_loops, hubs)
                what = (f'ss_fused_hop_stage input form P={P} mh2_out {"given" if with_mh2 else "NULL"} posts={posts}, self_loops={self_loops} '
                        f'hub list {"given" if hubs else "withheld"}')
                hll2, cards = _fused(w, P, r.d_in, with_mh2)
                r.check(hll2, what)
                _check_cards(cards, r, 8, f'{what}, {kind} round {k}: cardinalities', everyone)
    assert w.tickets_clean()


# ---- the symmetric variant ----------------------------------------------------------------------------------------------------------------
def test_symmetric_graph_skips_only_what_it_may(ssa, dev, monkeypatch):
    """a symmetric graph (csr.symmetric == 1) with regular rows, one hub row and one mega row.  With hop_tables=True the regular rows
    with an in-edge leave their own row out -- its poison must not show -- while hub and mega rows keep theirs -- its witness must show;
    with the hub list withheld those are regular rows too.  With SS_SELF_SKIP=0, and without the bit, every row keeps its own row; so
    does the fused stage over a table that is the caller's"""
    w = _world(ssa, dev, 'symmetric')
    assert int(w.csr.symmetric.item()) == 1 and len(w.hub_rows) == 1 and len(w.mega_rows) == 1
    everyone = np.arange(w.N)
    settings = [('hop_tables', True, None, True, w.plan(True, skip=True, hubs=True)), ('hop_tables, hub list withheld', True, None, False, w.plan(True, skip=True, hubs=False)),
                ('hop_tables with SS_SELF_SKIP=0', True, '0', True, w.plan(True)), ('without the bit', False, None, True, w.plan(True))]
    assert settings[0][4].poison.sum() == len(tp.SYMMETRIC_DEGREES) - 3 and not settings[2][4].poison.any()
    for name, bit, env, hubs, plan in settings:
        if env is None:
            monkeypatch.delenv('SS_SELF_SKIP', raising=False)
        else:
            monkeypatch.setenv('SS_SELF_SKIP', env)
        w.setting(True, hubs)
        for (mk, mi), (hk, hi) in _paired(plan, 128, 256):
            rm, rh = Round(plan, 'minhash', mk, mi, 128, dev), Round(plan, 'hll', hk, hi, 256, dev)
            r_mh = w.propagate(mh_in=rm.d_in, hop_tables=bit)[0]
            rm.check(r_mh, f'ss_propagate MinHash alone, symmetric graph, {name}')
            _, r_hll, cards = w.propagate(hll_in=rh.d_in, cards=True, hop_tables=bit)
            rh.check(r_hll, f'ss_propagate HLL alone, symmetric graph, {name}')
            _check_cards(cards, rh, 8, f'symmetric graph, {name}, {hk} round {hi}: cardinalities', everyone)
            mh, hll, _ = w.propagate(mh_in=rm.d_in, hll_in=rh.d_in, hop_tables=bit)
            rm.check(mh, f'ss_propagate both (MinHash side), symmetric graph, {name}')
            rh.check(hll, f'ss_propagate both (HLL side), symmetric graph, {name}')
    monkeypatch.delenv('SS_SELF_SKIP', raising=False)
    plan = w.plan(True)
    w.setting(True, True)
    for kind, k in plan.rounds(256):
        r = Round(plan, 'hll', kind, k, 256, dev)
        hll2, cards = _fused(w, 128, r.d_in, True)
        r.check(hll2, 'ss_fused_hop_stage input form, symmetric graph')
    assert w.tickets_clean()


# ---- SS_HUB_LAUNCHES=1: the hub units as launches of their own (16 wavefronts) ---------------------------------------------------------------
_CHILD = r"""
import hashlib, sys
from argparse import Namespace
import numpy as np, torch
sys.path[:0] = [%r, %r]
import subgraph_sketching_amd as ssa
import hll_planted as hp
import table_hop_planted as tp
self_loops, out_path = sys.argv[1] == '1', sys.argv[2]
dev = torch.device('cuda:0')
g = tp.main_graph()
csr = ssa.hashing.build_csr(torch.from_numpy(g.edge_index).to(dev), g.n, dev, check=True, hub_threshold=tp.HUB_THRESHOLD)
csr.use_inferred_self_loops = self_loops
rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()[:g.edge_index.shape[1]]
plan = tp.Plan(rowptr, col, g.n_test, g.n_self if self_loops else 0)
n_mega = int(csr.mega_count[0].item())
units = np.sort(np.concatenate([csr.hub_rows[:int(csr.hub_count.item())].cpu().numpy(), csr.mega_rows[:n_mega, 0].cpu().numpy()]).astype(np.int64))
eh = ssa.ElphHashes(Namespace(max_hash_hops=2, hll_p=8, minhash_num_perm=128, floor_sf=False, use_zero_one=True))
eh.hll_tables = hp.tables(8, None)
params = eh._params(dev)
lib = ssa._native.lib()
tickets = torch.zeros((), dtype=torch.bool, device=dev)
out = {'rowptr': rowptr, 'col': col, 'units': units}
def run(mh_in, hll_in):
    global tickets
    mh_out = torch.full_like(mh_in, 0x5A5A5A5A) if mh_in is not None else None
    hll_out = torch.full_like(hll_in, 0xA5) if hll_in is not None else None
    cards = torch.full((g.n,), -1.0, dtype=torch.float32, device=dev) if hll_in is not None else None
    ssa.hashing._propagate(csr, mh_in, hll_in, dev, cards_out=cards, cards_stride=1 if cards is not None else 0,
                           params=params if cards is not None else None, mh_out=mh_out, hll_out=hll_out)
    tickets |= csr.mega_rows[:n_mega, 3:5].any()
    return mh_out, hll_out, cards
def keep(tag, t):
    a = t.cpu().numpy()
    out[tag + '_units'] = a[units]
    out[tag + '_sha'] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
rm, rh = plan.rounds(128), plan.rounds(256)
lib.ss_debug_hub_calls(1)
for q in range(max(len(rm), len(rh))):
    (mk, mi), (hk, hi) = rm[q %% len(rm)], rh[q %% len(rh)]
    mh_in = torch.from_numpy(plan.table('minhash', mk, mi, 128).view(np.int32)).to(dev)
    hll_in = torch.from_numpy(plan.table('hll', hk, hi, 256)).to(dev)
    if q < len(rm):
        keep('mh_alone_%%d' %% q, run(mh_in, None)[0])
    if q < len(rh):
        _, hll, cards = run(None, hll_in)
        keep('hll_alone_%%d' %% q, hll)
        out['cards_alone_%%d' %% q] = cards.cpu().numpy()
    mh, hll, cards = run(mh_in, hll_in)
    keep('mh_both_%%d' %% q, mh)
    keep('hll_both_%%d' %% q, hll)
    out['cards_both_%%d' %% q] = cards.cpu().numpy()
out['hub_calls'] = int(lib.ss_debug_hub_calls(0))
out['tickets'] = bool(tickets.item())
np.savez(out_path, **out)
"""


@pytest.mark.parametrize('self_loops', [True, False])
def test_hub_units_as_launches_of_their_own(tmp_path, self_loops):
    """propagate_hub_kernel<MH, HLL> in its three forms (MinHash alone, HLL alone, both after the two row launches of the fast shape),
    16 wavefronts per unit.  SS_HUB_LAUNCHES is read once per process: a fresh child process, which writes the rows of every hub and mega
    unit and a digest of each whole table; the parent compares both with want_rows and the cardinalities by _check_counts"""
    from conftest import REPO
    out = str(tmp_path / 'out.npz')
    env = dict(os.environ, SS_HUB_LAUNCHES='1')
    for name in ('SS_SELF_SKIP', 'SS_HUB_THRESHOLD'):
        env.pop(name, None)
    done = subprocess.run([sys.executable, '-c', _CHILD % (REPO, os.path.dirname(os.path.abspath(__file__))), '1' if self_loops else '0', out], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    got = np.load(out)
    g = tp.main_graph()
    plan = tp.Plan(got['rowptr'], got['col'], g.n_test, g.n_self if self_loops else 0)
    assert tp.is_csr_of(got['rowptr'], got['col'], g.edge_index, g.n)
    units = got['units']
    deg = np.diff(got['rowptr'])
    assert np.array_equal(units, np.flatnonzero(deg > tp.HUB_THRESHOLD)) and not bool(got['tickets']) and int(got['hub_calls']) > 0
    everyone = np.arange(g.n)
    rm, rh = plan.rounds(128), plan.rounds(256)

    def compare(tag, want, sketch, kind, k, what):
        msg = tp.first_difference(got[tag + '_units'], want[units], sketch, kind, k, what + ' (hub and mega rows)', rows=units)
        assert msg is None, msg
        assert got[tag + '_sha'].tobytes() == hashlib.sha256(want.tobytes()).digest(), f'{what}, {sketch} {kind} round {k}: a row outside the hub units differs'

    for q in range(max(len(rm), len(rh))):
        (mk, mi), (hk, hi) = rm[q % len(rm)], rh[q % len(rh)]
        want_mh = plan.want('minhash', plan.table('minhash', mk, mi, 128))
        want_hll = plan.want('hll', plan.table('hll', hk, hi, 256))
        rh_q = SimpleNamespace(want=want_hll)
        if q < len(rm):
            compare(f'mh_alone_{q}', want_mh, 'minhash', mk, mi, 'SS_HUB_LAUNCHES=1 ss_propagate MinHash alone')
        if q < len(rh):
            compare(f'hll_alone_{q}', want_hll, 'hll', hk, hi, 'SS_HUB_LAUNCHES=1 ss_propagate HLL alone')
            _check_cards(torch.from_numpy(got[f'cards_alone_{q}']), rh_q, 8, f'SS_HUB_LAUNCHES=1 HLL alone round {q}: cardinalities', everyone)
        compare(f'mh_both_{q}', want_mh, 'minhash', mk, mi, 'SS_HUB_LAUNCHES=1 ss_propagate both (MinHash side)')
        compare(f'hll_both_{q}', want_hll, 'hll', hk, hi, 'SS_HUB_LAUNCHES=1 ss_propagate both (HLL side)')
        _check_cards(torch.from_numpy(got[f'cards_both_{q}']), rh_q, 8, f'SS_HUB_LAUNCHES=1 both round {q}: cardinalities', everyone)
