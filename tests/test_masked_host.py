"""Target-link masking without a GPU: the numpy restatement of the rule (tests/masked_restatement.py) against the oracle run over the
edge list minus the link -- tables and counts bit-exact, features within DESIGN 4's bar --, the C-ABI argument checks of
ss_masked_pair_features (they return before any launch) and the Python argument errors of the masked and the exact query (raised before
the compute device is touched)."""
from argparse import Namespace
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import masked_restatement as mr
from conftest import load_golden, oracle_params
from oracle import oracle


def _params(p=8):
    import subgraph_sketching_amd as ssa
    return oracle_params(ssa.hll_tables.load(p))


def _eh(h=2, num_perm=128, p=8):
    import subgraph_sketching_amd as ssa
    return ssa.ElphHashes(Namespace(max_hash_hops=h, hll_p=p, minhash_num_perm=num_perm, floor_sf=False, use_zero_one=True))


def check_against_leave_one_out(n, ei, links, h, num_perm=128, p=8, expect_masked=None):
    """the restated rule on `links` against one oracle rebuild per link; -> the restatement's debug dict"""
    prm = _params(p)
    tables, cards = oracle.build_hash_tables(n, ei, h, num_perm, prm)
    feats, dbg = mr.masked_query(links, n, ei, tables, cards, h, prm)
    plain, pdbg = oracle.pair_features(links, tables, cards, h, prm, debug=True)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    for q, (u, v) in enumerate(links.tolist()):
        want_f, want_dbg, want_rows, want_cards = mr.leave_one_out(u, v, n, ei, h, num_perm, prm)
        for kind in ('minhash', 'hll'):
            assert np.array_equal(dbg['rows'][kind][q], want_rows[kind]), f'link {q} = ({u}, {v}): {kind} rows differ from the rebuild'
        assert np.array_equal(dbg['match'][q], want_dbg['match']) and np.array_equal(dbg['zeros'][q], want_dbg['zeros']), (q, u, v)
        assert np.array_equal(dbg['row_zeros'][q], (want_rows['hll'] == 0).sum(axis=2)), (q, u, v)
        np.testing.assert_allclose(dbg['cards'][q], want_cards, rtol=1e-5, atol=1e-5 * 4 * float(np.abs(cards).max()))
        mr.assert_features_bar(feats[q], want_f, cards, f'link {q} = ({u}, {v})')
        if not dbg['masked'][q]:  # nothing to remove: the plain query's row, bit for bit
            assert np.array_equal(feats[q].view(np.int32), plain[q].view(np.int32))
            assert np.array_equal(dbg['match'][q], pdbg['match'][q]) and np.array_equal(dbg['zeros'][q], pdbg['zeros'][q])
    if expect_masked is not None:
        assert dbg['masked'].tolist() == list(expect_masked)
    return dbg


def _non_edges(n, ei, count, seed):
    have = set(map(tuple, ei.T.tolist()))
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        u, v = (int(x) for x in rng.randint(0, n, size=2))
        if u != v and (u, v) not in have and (v, u) not in have:
            out.append((u, v))
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize('h', [1, 2, 3])
def test_ba40_every_edge_and_40_non_edges(h):
    g = load_golden('g3_g4_ba40.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    links = np.concatenate([ei.T, _non_edges(n, ei, 40, 5)])
    dbg = check_against_leave_one_out(n, ei, links, h)
    assert dbg['masked'][:ei.shape[1]].all() and not dbg['masked'][ei.shape[1]:].any()


def test_uniform3000_256_edge_links():
    n, e_und, seed = [int(x) for x in load_golden('g8_uniform3000.npz')['graph']]
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, e_und)).astype(np.int64)
    ei = np.concatenate([e, e[::-1]], axis=1)
    pick = np.random.RandomState(3).choice(ei.shape[1], size=256, replace=False)
    links = ei[:, pick].T
    links = links[links[:, 0] != links[:, 1]]
    assert len(links) >= 250
    dbg = check_against_leave_one_out(n, ei, links, 3)
    assert dbg['masked'].all()


@pytest.mark.parametrize('h', [1, 2, 3])
def test_directed_graph_where_only_one_direction_exists(h):
    rng = np.random.RandomState(17)
    n = 80
    ei = rng.randint(0, n, size=(2, 200)).astype(np.int64)
    have = set(map(tuple, ei.T.tolist()))
    one_way = [(u, v) for u, v in ei.T.tolist() if u != v and (v, u) not in have][:30]
    assert len(one_way) == 30
    links = np.array(one_way + [(v, u) for u, v in one_way[:10]], dtype=np.int64)  # listed forwards, and against the edge
    check_against_leave_one_out(n, ei, links, h, expect_masked=[True] * 40)


@pytest.mark.parametrize('h', [2, 3])
def test_duplicated_edges_self_edges_and_u_equals_v(h):
    rng = np.random.RandomState(23)
    n = 60
    e = rng.randint(0, n, size=(2, 90)).astype(np.int64)
    ei = np.concatenate([e, e[::-1], e[:, :30], e[::-1][:, :10]], axis=1)  # every copy of a duplicated edge has to go
    x = rng.randint(0, n, size=6)
    ei = np.concatenate([ei, np.stack([x, x])], axis=1)                    # explicit self edges stay
    dup = e[:, :30].T
    dup = dup[dup[:, 0] != dup[:, 1]]
    links = np.concatenate([dup, [[int(x[0]), int(x[0])], [7, 7], [-1, -2]]]).astype(np.int64)
    dbg = check_against_leave_one_out(n, ei, np.where(links < 0, links + n, links), h)
    assert dbg['masked'][:len(dup)].all() and not dbg['masked'][len(dup):len(dup) + 2].any()


@pytest.mark.parametrize('h', [1, 2, 3])
def test_trailing_isolated_nodes(h):
    """G7: nodes 9 .. 11 of 12 lie at or above max(edge_index) + 1 -- no self loop, all-zero rows"""
    g = load_golden('g7_edge_cases.npz')
    n, ei = int(g['num_nodes']), np.asarray(g['edge_index'], dtype=np.int64)
    edges = np.array([e for e in ei.T.tolist() if e[0] != e[1]], dtype=np.int64)
    links = np.concatenate([edges, [[10, 3], [11, 9], [2, 11]]]).astype(np.int64)
    dbg = check_against_leave_one_out(n, ei, links, h)
    assert dbg['masked'][:len(edges)].all() and not dbg['masked'][len(edges):].any()


@pytest.mark.parametrize('h', [1, 2, 3])
def test_n_self_stays_that_of_the_full_edge_list(h):
    """the link's endpoint is the largest id and that edge is its only one: a rebuild WITHOUT pinning n_self would take the self loops of
    the nodes above the second-largest id away"""
    rng = np.random.RandomState(29)
    e = rng.randint(0, 30, size=(2, 50)).astype(np.int64)
    ei = np.concatenate([e, e[::-1], [[4, 37], [37, 4]]], axis=1)
    n = 40
    assert mr.n_self_of(ei) == 38 and mr.n_self_of(mr.without_link(ei, 4, 37)) < 38
    dbg = check_against_leave_one_out(n, ei, np.array([[4, 37], [37, 4], [36, 4]]), h, expect_masked=[True, True, False])
    assert (dbg['rows']['hll'][0, 1, 0] != 0).sum() == 1  # node 37 keeps its self loop and nothing else


def test_other_sketch_shapes():
    rng = np.random.RandomState(31)
    n = 50
    e = rng.randint(0, n, size=(2, 80)).astype(np.int64)
    ei = np.concatenate([e, e[::-1]], axis=1)
    links = e[:, :12].T
    links = links[links[:, 0] != links[:, 1]]
    for num_perm, p in ((64, 6), (256, 10), (8, 4)):
        check_against_leave_one_out(n, ei, links, 3, num_perm=num_perm, p=p)


# ---- argument paths (no device) -----------------------------------------------------------------------------------------------------
def test_refused_combinations_name_what_they_refuse():
    eh = _eh()
    links = torch.tensor([[0, 1]])
    ei = torch.tensor([[0, 1], [1, 0]])
    for kw, name in (({'degrees': torch.ones(4)}, 'degrees'), ({'lazy': True}, 'lazy'), ({'out': torch.empty(1, 8)}, 'out')):
        with pytest.raises(ValueError, match=f'mask_target.*{name}'):
            eh.get_subgraph_features(links, {}, None, mask_target=ei, **kw)
    with pytest.raises(ValueError, match='return_debug'):
        eh.get_subgraph_features(links, {}, None, return_debug=True)


@pytest.mark.parametrize('bad', [torch.zeros((3, 4), dtype=torch.int64), torch.zeros(6, dtype=torch.int64), torch.zeros((2, 4), dtype=torch.float32),
                                 torch.zeros((4, 2), dtype=torch.int64)])
def test_wrong_shaped_edge_index(bad):
    with pytest.raises(ValueError, match='mask_target must be the integer edge_index'):
        _eh().get_subgraph_features(torch.tensor([[0, 1]]), {}, None, mask_target=bad)


def test_wrong_links_and_batch_size():
    eh = _eh()
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match='links must be an integer'):
        eh.get_subgraph_features(torch.zeros((3, 3), dtype=torch.int64), {}, None, mask_target=ei)
    with pytest.raises(ValueError, match='batch_size'):
        eh.get_subgraph_features(torch.tensor([[0, 1]]), {}, None, mask_target=ei, batch_size=0)


def test_exact_companion_argument_path():
    eh = _eh()
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match='mask_target of the exact query is a bool'):
        eh.exact_subgraph_features(torch.tensor([[0, 1]]), 4, ei, mask_target=ei)
    with pytest.raises(ValueError, match='edge_index must be an integer tensor'):  # the checks behind it still run
        eh.exact_subgraph_features(torch.tensor([[0, 1]]), 4, torch.zeros((3, 2), dtype=torch.int64), mask_target=True)
    with pytest.raises(IndexError):
        eh.exact_subgraph_features(torch.tensor([[0, 9]]), 4, ei, mask_target=True)
    import subgraph_sketching_amd as ssa
    assert ssa._native.SS_FLAG_MASK_TARGET == 4 and not (ssa._native.SS_FLAG_MASK_TARGET & (ssa._native.SS_FLAG_USE_ZERO_ONE | ssa._native.SS_FLAG_FLOOR_SF))


def test_cabi_argument_errors_without_a_gpu():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    assert lib.ss_masked_workspace_bytes(0) == 256 and lib.ss_masked_workspace_bytes(1000) >= 256 + 4000
    assert lib.ss_masked_workspace_bytes(-1) == 0 and lib.ss_masked_workspace_bytes(1 << 31) == 0
    fake = c_void_p(8)  # never dereferenced: every call below is rejected by the host-side checks
    g = ssa._native.CsrGraphStruct(rowptr=8, col=8, num_nodes=4, n_self_loops=4)
    tables = ssa.hll_tables.load(8)
    prm = ssa._native.HllParams(p=8, n_tbl=len(tables.bias), alpha_mm=1.0, threshold=1.0, lc_min_zeros=1, raw_est=8, bias=8, lc_table=8)
    ptrs = (c_void_p * 3)(8, 8, 8)

    def call(graph=g, B=3, N=4, h=2, P=128, params=prm, ws=fake, ws_bytes=1 << 20, a=fake):
        return lib.ss_masked_pair_features(byref(graph) if graph is not None else None, fake, B, N, h, a, fake, ptrs, P, ptrs, fake, 2,
                                           byref(params) if params is not None else None, 0, fake, None, None, None, None, None, ws, ws_bytes,
                                           None)
    assert call(h=4) == -4 and call(h=0) == -4
    assert call(B=-1) == -1 and call(B=1 << 31) == -1
    assert call(params=None) == -1
    assert call(B=0) == 0                      # no links: nothing to do
    assert call(graph=None) == -1 and call(a=None) == -1 and call(ws=None) == -1
    assert call(N=5) == -1                     # the graph is not the tables' graph
    assert call(P=130) == -1
    assert call(P=1024) == -4                  # 256 + 16 chunks per row: no kernel
    assert call(ws_bytes=16) == -3
    g.row_begin, g.row_end = 1, 3
    assert call() == -1                        # a row range has no meaning here
