"""The C-ABI library loads on a GPU-less host and exports every symbol include/subgraph_sketch.h (the drop-in boundary)
and include/subgraph_sketch_debug.h (measurement-only probes) declare (no compute calls here)."""
import ctypes
import os
import re

import pytest

from conftest import REPO


def _declared_symbols(headers=('subgraph_sketch.h', 'subgraph_sketch_debug.h')):
    names = set()
    for header in headers:
        text = open(os.path.join(REPO, 'include', header)).read()
        text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
        names |= set(re.findall(r'\b(ss_[a-z0-9_]+)\s*\(', text))
    return sorted(names)


def test_header_declares_the_expected_boundary():
    names = _declared_symbols(('subgraph_sketch.h',))
    assert not [n for n in names if n.startswith(('ss_time_', 'ss_profile_'))], 'probes belong in subgraph_sketch_debug.h'
    for needed in ('ss_minhash_init', 'ss_hll_init', 'ss_csr_build', 'ss_propagate', 'ss_hll_count', 'ss_pair_features',
                   'ss_pack_minhash', 'ss_unpack_minhash', 'ss_estimate_bias', 'ss_version', 'ss_error_string'):
        assert needed in names


def test_library_exports_every_declared_symbol():
    import subgraph_sketching_amd as ssa
    path = ssa._native.LIB_PATH
    assert os.path.exists(path), 'run `python __graft_entry__.py` first (build())'
    handle = ctypes.CDLL(path)
    declared = _declared_symbols()
    missing = [n for n in declared if not hasattr(handle, n)]
    assert not missing, f'symbols declared in the header but not exported: {missing}'
    unbound = [n for n in declared if n not in ssa._native.SIGNATURES]
    assert not unbound, f'symbols declared in the header but not bound in _native.SIGNATURES: {unbound}'
    extra = [n for n in ssa._native.SIGNATURES if n not in declared]
    assert not extra, f'bound but not declared: {extra}'


def test_version_and_error_strings():
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    assert lib.ss_version() == 129 == ssa._native.ABI_VERSION
    assert lib.ss_error_string(0) == b'ok'
    assert b'invalid' in lib.ss_error_string(-1)
    assert lib.ss_csr_workspace_bytes(1000, 5000) >= 8 * 1001


def test_profile_probe_bookkeeping_without_a_gpu():
    """the tagged span list: nothing recorded -> zero launches; bad tags are argument errors"""
    from ctypes import byref, c_float, c_int32
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    ms, n = c_float(-1.0), c_int32(-1)
    assert lib.ss_profile_enable(0) == 0
    assert lib.ss_profile_read(ssa._native.PROF_MINHASH_HOP, byref(ms), byref(n)) == 0 and n.value == 0 and ms.value == 0.0
    assert lib.ss_profile_read(99, byref(ms), byref(n)) == -1


def test_argument_errors_are_reported_without_a_gpu():
    """argument validation happens on the host before any launch"""
    import subgraph_sketching_amd as ssa
    lib = ssa._native.lib()
    assert lib.ss_minhash_init(None, 0, 10, None, None, 128, None) == -1      # null pointers
    assert lib.ss_minhash_init(None, 0, 0, None, None, 128, None) == 0        # empty is fine
    assert lib.ss_hll_init(None, 0, 10, 3, None) == -1                        # p < 4
    assert lib.ss_pack_minhash(None, None, -1, None) == -1
    assert lib.ss_fused_hop_stage(None, None, None, 128, None, None, 8, None, None, None, None, 0, None, None) == -1   # no graph
    assert lib.ss_pair_features(None, 0, 0, 4, None, 128, None, None, 0, None, 0, None, None, None, None, None, None) == -4  # h = 4
    assert lib.ss_minhash_hop_rows(None, None, None, 128, None, 0, None) == -1                                                 # no graph
    assert lib.ss_first_hop(None, None, None, 128, None, 8, None, None, 0, None, None) == -1
    assert lib.ss_propagate(None, None, None, 128, None, None, 256, None, 0, None, None) == -1
    for cn in (lib.ss_common_neighbour_scores, lib.ss_common_neighbour_scores_f32):
        assert cn(None, None, None, None, 4, None, 3, None, None, None) == -1       # null CSR / links / out
        assert cn(None, None, None, None, 4, None, -1, None, None, None) == -1
        assert cn(None, None, None, None, 4, None, 0, None, None, None) == 0        # no links: nothing to do
    g = ssa._native.CsrGraphStruct(rowptr=8, col=8, num_nodes=4, n_self_loops=0, n_self_loops_dev=None, hub_threshold=512, reserved=0,
                                   hub_rows=None, hub_count=None, mega_rows=None, mega_count=None, mega_scratch=None, row_begin=0, row_end=0)
    from ctypes import byref, c_void_p
    fake = c_void_p(8)   # never dereferenced: every call below is rejected by the host-side checks
    assert lib.ss_minhash_hop_rows(byref(g), fake, fake, 130, fake, 4, None) == -1      # P not a multiple of 4
    assert lib.ss_minhash_hop_rows(byref(g), fake, fake, 128, None, 4, None) == -1      # rows missing
    assert lib.ss_minhash_hop_rows(byref(g), fake, fake, 128, fake, -1, None) == -1
    assert lib.ss_minhash_hop_rows(byref(g), fake, fake, 128, None, 0, None) == 0       # empty list: nothing to do
    g.row_begin, g.row_end = 1, 3
    assert lib.ss_minhash_hop_rows(byref(g), fake, fake, 128, fake, 4, None) == -1      # a row list and a row range exclude each other
    assert lib.ss_first_hop(byref(g), fake, fake, 100, fake, 8, None, None, 0, None, None) == -4     # no first-hop kernel for P = 100
    assert lib.ss_first_hop(byref(g), fake, fake, 128, None, 6, fake, None, 0, None, None) == -4     # HLL first hop is p = 8 only
    g.row_begin, g.row_end = 3, 1
    assert lib.ss_propagate(byref(g), fake, fake, 128, None, None, 256, None, 0, None, None) == -1   # empty / reversed row range


# ---- return codes of the table-hop entry points ---------------------------------------------------------------------------------
# Every call below returns before a launch.  Each entry point has a base call that passes every check but the last one before its
# first launch (an empty row range, a row range beside a row list, a workspace of 0 bytes) and a list of named edits to it: every
# bad-argument class of its preamble and the early SS_OK exits.  _PINNED[entry][i][j] is the code with edits i and j applied together
# (i == j: edit i alone), so a row shows which of two errors is reported: '0' SS_OK, 'I' SS_ERR_INVALID_ARG, 'W' SS_ERR_WORKSPACE,
# 'U' SS_ERR_UNSUPPORTED.  The letters were produced by the library as it stood before the host side of these units was rewritten
# around one request record, and that rewrite had to reproduce them.
_FAKE = 8          # a non-null pointer that is never dereferenced
_LETTER = {0: '0', -1: 'I', -3: 'W', -4: 'U'}


def _edit(**fields):
    """an edit: 'g.x' sets field x of the graph, 'prm.x' of the HLL parameters, anything else the argument of that name"""
    def apply(s):
        for key, value in fields.items():
            where, _, name = key.rpartition('.')
            if not where:
                s[name] = value
            elif s[where] is not None:   # (another edit may have taken the whole struct away)
                s[where][name] = value
    return apply


def _graph_edits():
    return [('no graph', _edit(g=None)), ('N < 0', _edit(**{'g.num_nodes': -1})), ('no rowptr', _edit(**{'g.rowptr': None})),
            ('N = 0', _edit(**{'g.num_nodes': 0})), ('N = 2^31', _edit(**{'g.num_nodes': 1 << 31})),
            ('hub_rows without hub_count', _edit(**{'g.hub_rows': _FAKE}))]


def _prm_edits():
    return [('no prm', _edit(prm=None)), ('prm.p = 3', _edit(**{'prm.p': 3})), ('prm.n_tbl = 5', _edit(**{'prm.n_tbl': 5})),
            ('prm.bias missing', _edit(**{'prm.bias': None})), ('prm.p = 9', _edit(**{'prm.p': 9}))]


def _state(**args):
    g = dict(rowptr=_FAKE, col=_FAKE, num_nodes=4, n_self_loops=0, hub_threshold=512, row_begin=2, row_end=2)   # an empty row range
    prm = dict(p=8, n_tbl=6, raw_est=_FAKE, bias=_FAKE, lc_table=_FAKE)
    return dict(g=g, prm=prm, **args)


def _table_hop_entries():
    reversed_range = ('reversed row range', _edit(**{'g.row_begin': 3, 'g.row_end': 1}))
    entries = {}
    entries['ss_propagate'] = (
        _state(mh_in=_FAKE, mh_out=_FAKE, P=128, hll_in=_FAKE, hll_out=_FAKE, M=256, cards_out=_FAKE, cards_stride=1),
        ('g', 'mh_in', 'mh_out', 'P', 'hll_in', 'hll_out', 'M', 'cards_out', 'cards_stride', 'prm', None),
        _graph_edits() + [reversed_range, ('mh_in alone', _edit(mh_out=None)), ('hll_out alone', _edit(hll_in=None)),
                          ('no tables', _edit(mh_in=None, mh_out=None, hll_in=None, hll_out=None)), ('P = 130', _edit(P=130)),
                          ('M = 100', _edit(M=100)), ('cards without HLL', _edit(hll_in=None, hll_out=None)),
                          ('MinHash alone', _edit(hll_in=None, hll_out=None, cards_out=None)),
                          ('HLL alone', _edit(mh_in=None, mh_out=None)), ('M = 512', _edit(M=512))] + _prm_edits())
    entries['ss_first_hop'] = (
        _state(a=_FAKE, b=_FAKE, P=128, mh_out=_FAKE, p=8, hll_out=_FAKE, cards_out=_FAKE, cards_stride=1),
        ('g', 'a', 'b', 'P', 'mh_out', 'p', 'hll_out', 'cards_out', 'cards_stride', 'prm', None),
        _graph_edits() + [reversed_range, ('p = 6', _edit(p=6)), ('P = 100', _edit(P=100)), ('P = 0', _edit(P=0)), ('P = 320', _edit(P=320)),
                          ('no tables', _edit(mh_out=None, hll_out=None)), ('no a', _edit(a=None)), ('cards without HLL', _edit(hll_out=None)),
                          ('MinHash alone', _edit(hll_out=None, cards_out=None)), ('HLL alone', _edit(mh_out=None, a=None, b=None))]
        + _prm_edits())
    fused = [reversed_range, ('p = 6', _edit(p=6)), ('P = 100', _edit(P=100)), ('P = 192', _edit(P=192)),
             ('P = 192, no mh2_out', _edit(P=192, mh2_out=None)), ('no mh1_out', _edit(mh1_out=None)), ('no b', _edit(b=None)),
             ('no hll1', _edit(hll1=None)), ('no hll2_out', _edit(hll2_out=None)),
             # (the only check behind the empty-range exit: with cards1_out the stage computes hop 1 too and wants cards2_out)
             ('cards1_out without cards2_out, whole graph', _edit(cards2_out=None, **{'g.row_begin': 0, 'g.row_end': 0}))]
    entries['ss_fused_hop_stage'] = (
        _state(a=_FAKE, b=_FAKE, P=128, mh1_out=_FAKE, mh2_out=_FAKE, p=8, hll1=_FAKE, cards1_out=_FAKE, hll2_out=_FAKE, cards2_out=_FAKE,
               cards_stride=1),
        ('g', 'a', 'b', 'P', 'mh1_out', 'mh2_out', 'p', 'hll1', 'cards1_out', 'hll2_out', 'cards2_out', 'cards_stride', 'prm', None),
        _graph_edits() + fused + _prm_edits())
    entries['ss_fused_hop_stage_records'] = (
        dict(entries['ss_fused_hop_stage'][0], records=_FAKE, num_edges=8),
        entries['ss_fused_hop_stage'][1][:-1] + ('records', 'num_edges', None),
        _graph_edits() + fused + [('no records', _edit(records=None)), ('num_edges = -1', _edit(num_edges=-1))] + _prm_edits())
    entries['ss_minhash_hop_rows'] = (
        dict(_state(mh_in=_FAKE, mh_out=_FAKE, P=128, rows=_FAKE, n_rows=4), g=dict(_state()['g'], row_begin=1, row_end=3)),
        ('g', 'mh_in', 'mh_out', 'P', 'rows', 'n_rows', None),
        _graph_edits() + [('no mh_in', _edit(mh_in=None)), ('no mh_out', _edit(mh_out=None)), ('n_rows < 0', _edit(n_rows=-1)),
                          ('no rows', _edit(rows=None)), ('P = 130', _edit(P=130)), ('P = 0', _edit(P=0)), ('P = 2052', _edit(P=2052)),
                          ('P = 100', _edit(P=100)), ('empty list', _edit(rows=None, n_rows=0)), ('n_rows = 2^33', _edit(n_rows=1 << 33))])
    whole = dict(_state()['g'], row_begin=0, row_end=0)
    update_graph = [e for e in _graph_edits() if e[0] != 'hub_rows without hub_count'] + [
        ('no col', _edit(**{'g.col': None})), ('a row range', _edit(**{'g.row_begin': 1, 'g.row_end': 3})), ('no workspace', _edit(workspace=None)),
        ('h = 0', _edit(h=0)), ('h = 4', _edit(h=4))]
    entries['ss_update_mark'] = (
        dict(_state(added_dst=_FAKE, n_added=2, removed_dst=_FAKE, n_removed=2, cards_old=_FAKE, cards_stride=1, h=2, err_flag=_FAKE,
                    workspace=_FAKE, workspace_bytes=0), g=whole),
        ('g', 'added_dst', 'n_added', 'removed_dst', 'n_removed', 'cards_old', 'cards_stride', 'h', 'err_flag', 'workspace', 'workspace_bytes',
         None),
        update_graph + [('n_added < 0', _edit(n_added=-1)), ('no added_dst', _edit(added_dst=None)), ('no removed_dst', _edit(removed_dst=None)),
                        ('no edits', _edit(added_dst=None, n_added=0, removed_dst=None, n_removed=0)), ('no cards_old', _edit(cards_old=None)),
                        ('cards_stride = 0', _edit(cards_stride=0))])
    entries['ss_update_hop'] = (
        dict(_state(hop=1, h=2, a=_FAKE, b=_FAKE, mh_in=_FAKE, mh_out=_FAKE, P=128, hll_in=_FAKE, hll_out=_FAKE, p=8, cards_out=_FAKE,
                    cards_stride=1, workspace=_FAKE, workspace_bytes=0), g=whole),
        ('g', 'hop', 'h', 'a', 'b', 'mh_in', 'mh_out', 'P', 'hll_in', 'hll_out', 'p', 'cards_out', 'cards_stride', 'prm', 'workspace',
         'workspace_bytes', None),
        update_graph + [('hop = 0', _edit(hop=0)), ('hop = 3', _edit(hop=3)), ('hop = 2', _edit(hop=2)), ('P = 130', _edit(P=130)),
                        ('P = 100', _edit(P=100)), ('p = 3', _edit(p=3)), ('p = 6', _edit(p=6)), ('no mh_in', _edit(mh_in=None)),
                        ('no hll_in', _edit(hll_in=None)), ('no mh_out', _edit(mh_out=None)), ('no hll_out', _edit(hll_out=None)),
                        ('no cards_out', _edit(cards_out=None)), ('no a', _edit(a=None))] + _prm_edits())
    return entries


def _return_code(lib, nat, entry, state, order, edits):
    import copy
    from ctypes import byref
    s = copy.deepcopy(state)
    for apply in edits:
        apply(s)
    keep = []   # the structs outlive the call
    def arg(name):
        if name is None:
            return None     # the stream
        value = s[name]
        if name == 'g' and value is not None:
            keep.append(nat.CsrGraphStruct(**value))
            return byref(keep[-1])
        if name == 'prm' and value is not None:
            keep.append(nat.HllParams(**value))
            return byref(keep[-1])
        if name == 'head' and value is not None:
            keep.append(nat.StructureHeadStruct(**value))
            return byref(keep[-1])
        if isinstance(value, list):   # the per-hop table pointers: a ctypes array, None entries null
            keep.append((ctypes.c_void_p * len(value))(*value))
            return keep[-1]
        return value
    return getattr(lib, entry)(*[arg(name) for name in order])


def _return_code_rows(entry, entries=None):
    import subgraph_sketching_amd as ssa
    nat = ssa._native
    state, order, edits = (entries or _table_hop_entries())[entry]
    rows = []
    for name_i, edit_i in edits:
        codes = [_return_code(nat.lib(), nat, entry, state, order, [edit_i] if edit_i is edit_j else [edit_i, edit_j]) for _, edit_j in edits]
        rows.append((name_i, ''.join(_LETTER.get(c, '?') for c in codes)))
    return rows


_PINNED = {
    'ss_propagate': {
        'base call': '0',
        'no graph': 'IIIIIIIIIIIIIIIIIIIII',
        'N < 0': 'III0IIIIIIIIIIIIIIIII',
        'no rowptr': 'IIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'III0I0000000000000000',
        'N = 2^31': 'III0IIIIIIIIIIIIIIIII',
        'hub_rows without hub_count': 'III0IIIIIIIIIIIIIIIII',
        'reversed row range': 'III0IIIIIIIIIIIIIIIII',
        'mh_in alone': 'III0IIIIIIIIII0IIIIII',
        'hll_out alone': 'III0IIIIIIIII0IIIIIII',
        'no tables': 'III0IIIIIIIIIIIIIIIII',
        'P = 130': 'III0IIIIIIIIII0IIIIII',
        'M = 100': 'III0IIIIIIIII0IIIIIII',
        'cards without HLL': 'III0IIIIIIIII0IIIIIII',
        'MinHash alone': 'III0IIII0II000I000000',
        'HLL alone': 'III0III0II0III0IIUIII',
        'M = 512': 'III0IIIIIIIII0IIIUII0',
        'no prm': 'III0IIIIIIIII0IIIIIII',
        'prm.p = 3': 'III0IIIIIIIII0UUIUUUI',
        'prm.n_tbl = 5': 'III0IIIIIIIII0IIIUIII',
        'prm.bias missing': 'III0IIIIIIIII0IIIUIII',
        'prm.p = 9': 'III0IIIIIIIII0I0IUIII',
    },
    'ss_first_hop': {
        'base call': '0',
        'no graph': 'IIIIIIIIIIIIIIIIIIIII',
        'N < 0': 'III0IIIIIIIIIIIIIIIII',
        'no rowptr': 'IIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'III0I00UUUU0000000000',
        'N = 2^31': 'III0IIIUUUUIIIIIIIIII',
        'hub_rows without hub_count': 'III0IIIUUUUIIIIIIIIII',
        'reversed row range': 'III0IIIUUUUIIIIIIUIII',
        'p = 6': 'IIIUUUUUUUUIUI0UUUUUU',
        'P = 100': 'IIIUUUUUUUUUUUUUUUUUU',
        'P = 0': 'IIIUUUUUUUUUUUUUUUUUU',
        'P = 320': 'IIIUUUUUUUUUUUUUUUUUU',
        'no tables': 'III0IIIIUUUIIIIIIIIII',
        'no a': 'III0IIIUUUUIIII0IIIII',
        'cards without HLL': 'III0IIIIUUUIII0IIIIII',
        'MinHash alone': 'III0III0UUUII00I00000',
        'HLL alone': 'III0IIIUUUUI0II0IUIII',
        'no prm': 'III0IIIUUUUIII0IIIIII',
        'prm.p = 3': 'III0IIUUUUUIII0UIUUUI',
        'prm.n_tbl = 5': 'III0IIIUUUUIII0IIUIII',
        'prm.bias missing': 'III0IIIUUUUIII0IIUIII',
        'prm.p = 9': 'III0IIIUUUUIII0IIUIII',
    },
    'ss_fused_hop_stage': {
        'base call': '0',
        'no graph': 'IIIIIIIIIIIIIIIIIIIII',
        'N < 0': 'III0IIIIIIIIIIIIIIIII',
        'no rowptr': 'IIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'III0I00UUU00000000000',
        'N = 2^31': 'III0IIIUUUIIIIIIIIIII',
        'hub_rows without hub_count': 'III0IIIUUUIIIIIIIIIII',
        'reversed row range': 'III0IIIUUUIIIIIIIUIII',
        'p = 6': 'IIIUUUUUUUUUUUUUUUUUU',
        'P = 100': 'IIIUUUUUUU0UUUUUUUUUU',
        'P = 192': 'IIIUUUUUUU0UUUUUUUUUU',
        'P = 192, no mh2_out': 'III0IIIUU00IIIIIIUIII',
        'no mh1_out': 'III0IIIUUUIIIIIIIIIII',
        'no b': 'III0IIIUUUIIIIIIIIIII',
        'no hll1': 'III0IIIUUUIIIIIIIIIII',
        'no hll2_out': 'III0IIIUUUIIIIIIIIIII',
        'cards1_out without cards2_out, whole graph': 'III0IIIUUUIIIIIIIIIII',
        'no prm': 'III0IIIUUUIIIIIIIIIII',
        'prm.p = 3': 'III0IIUUUUUIIIIIIUUUI',
        'prm.n_tbl = 5': 'III0IIIUUUIIIIIIIUIII',
        'prm.bias missing': 'III0IIIUUUIIIIIIIUIII',
        'prm.p = 9': 'III0IIIUUUIIIIIIIUIII',
    },
    'ss_fused_hop_stage_records': {
        'base call': '0',
        'no graph': 'IIIIIIIIIIIIIIIIIIIIIII',
        'N < 0': 'III0IIIIIIIIIIIIIIIIIII',
        'no rowptr': 'IIIIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'III0I00UUU0000000000000',
        'N = 2^31': 'III0IIIUUUIIIIIIIIIIIII',
        'hub_rows without hub_count': 'III0IIIUUUIIIIIIIIIIIII',
        'reversed row range': 'III0IIIUUUIIIIIIIIIUIII',
        'p = 6': 'IIIUUUUUUUUUUUUUUUUUUUU',
        'P = 100': 'IIIUUUUUUU0UUUUUUUUUUUU',
        'P = 192': 'IIIUUUUUUU0UUUUUUUUUUUU',
        'P = 192, no mh2_out': 'III0IIIUU00IIIII00IUIII',
        'no mh1_out': 'III0IIIUUUIIIIIIIIIIIII',
        'no b': 'III0IIIUUUIIIIIIIIIIIII',
        'no hll1': 'III0IIIUUUIIIIIIIIIIIII',
        'no hll2_out': 'III0IIIUUUIIIIIIIIIIIII',
        'cards1_out without cards2_out, whole graph': 'III0IIIUUUIIIIIIIIIIIII',
        'no records': 'III0IIIUUU0IIIII00IUIII',
        'num_edges = -1': 'III0IIIUUU0IIIII00IUIII',
        'no prm': 'III0IIIUUUIIIIIIIIIIIII',
        'prm.p = 3': 'III0IIUUUUUIIIIIUUIUUUI',
        'prm.n_tbl = 5': 'III0IIIUUUIIIIIIIIIUIII',
        'prm.bias missing': 'III0IIIUUUIIIIIIIIIUIII',
        'prm.p = 9': 'III0IIIUUUIIIIIIIIIUIII',
    },
    'ss_minhash_hop_rows': {
        'base call': 'I',
        'no graph': 'IIIIIIIIIIIIIIII',
        'N < 0': 'III0IIIIIIIIIIII',
        'no rowptr': 'IIIIIIIIIIIIIIII',
        'N = 0': 'III0I0IIIIIII000',
        'N = 2^31': 'III0IIIIIIIIII0I',
        'hub_rows without hub_count': 'III0IIIIIIIIII0I',
        'no mh_in': 'IIIIIIIIIIIIIIII',
        'no mh_out': 'IIIIIIIIIIIIIIII',
        'n_rows < 0': 'IIIIIIIIIIIIII0I',
        'no rows': 'IIIIIIIIIIIIII0I',
        'P = 130': 'IIIIIIIIIIIIIIII',
        'P = 0': 'IIIIIIIIIIIIIIII',
        'P = 2052': 'IIIIIIIIIIIIIIII',
        'P = 100': 'III0IIIIIIIIII0I',
        'empty list': 'III000III0III00I',
        'n_rows = 2^33': 'III0IIIIIIIIII0I',
    },
    'ss_update_mark': {
        'base call': 'W',
        'no graph': 'IIIIIIIIUUIIIIII',
        'N < 0': 'III0IIIIUUIIIIII',
        'no rowptr': 'IIIIIIIIUUIIIIII',
        'N = 0': 'III0I000UUIII000',
        'N = 2^31': 'III0IIIIUUIIIIII',
        'no col': 'III0IIIIUUIIIIII',
        'a row range': 'III0IIIIUUIIIIII',
        'no workspace': 'III0IIIIUUIIIIII',
        'h = 0': 'UUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUUUU',
        'n_added < 0': 'IIIIIIIIUUIIIWII',
        'no added_dst': 'IIIIIIIIUUIIIWII',
        'no removed_dst': 'IIIIIIIIUUIIIWII',
        'no edits': 'III0IIIIUUIWWWII',
        'no cards_old': 'III0IIIIUUIIIIII',
        'cards_stride = 0': 'III0IIIIUUIIIIII',
    },
    'ss_update_hop': {
        'base call': 'W',
        'no graph': 'IIIIIIIIUUIIIIIIIIIIIIIIIIII',
        'N < 0': 'III0IIIIUUIIIIIIIIIIIIIIIIII',
        'no rowptr': 'IIIIIIIIUUIIIIIIIIIIIIIIIIII',
        'N = 0': 'III0I000UUII0I0U000000000000',
        'N = 2^31': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'no col': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'a row range': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'no workspace': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'h = 0': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'hop = 0': 'IIIIIIIIUUIIWIIIIIIIIIIIIIII',
        'hop = 3': 'IIIIIIIIUUIIWIIIIIIIIIIIIIII',
        'hop = 2': 'III0IIIIUUIIWIWUIUUIIIWIUIII',
        'P = 130': 'IIIIIIIIUUIIIIWIIIIIIIIIIIII',
        'P = 100': 'III0IIIIUUIIWIWUIUWIIIWIUIII',
        'p = 3': 'IIIUUUUUUUIIUIUUIUUUUUUUUUUU',
        'p = 6': 'III0IIIIUUIIIIIUIIUIIIIIUIII',
        'no mh_in': 'III0IIIIUUIIUIUUIWWIIIIIUIII',
        'no hll_in': 'III0IIIIUUIIUIWUUWWIIIWIUIII',
        'no mh_out': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'no hll_out': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'no cards_out': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'no a': 'III0IIIIUUIIWIWUIIWIIIWIUIII',
        'no prm': 'III0IIIIUUIIIIIUIIIIIIIIIIII',
        'prm.p = 3': 'III0IIIIUUIIUIUUUUUIIIUIUUUI',
        'prm.n_tbl = 5': 'III0IIIIUUIIIIIUIIIIIIIIUIII',
        'prm.bias missing': 'III0IIIIUUIIIIIUIIIIIIIIUIII',
        'prm.p = 9': 'III0IIIIUUIIIIIUIIIIIIIIUIII',
    },
}


@pytest.mark.parametrize('entry', sorted(_table_hop_entries()))
def test_table_hop_return_codes_are_pinned(entry):
    """every bad-argument class of the table-hop entry points, alone and in pairs, and their early SS_OK exits: the codes of the
    library before its host side was refactored (a '?' would be a code outside the four: a launch was reached)"""
    import subgraph_sketching_amd as ssa
    nat = ssa._native
    state, order, _ = _table_hop_entries()[entry]
    base = _return_code(nat.lib(), nat, entry, state, order, [])
    assert _LETTER.get(base) == _PINNED[entry]['base call'], base
    got = _return_code_rows(entry)
    assert [name for name, _ in got] == [name for name in _PINNED[entry] if name != 'base call']
    for name, row in got:
        assert row == _PINNED[entry][name], (entry, name, row, _PINNED[entry][name])


# ---- return codes of the common-neighbour entry points ---------------------------------------------------------------------------
# The same scheme for ss_common_neighbour_scores, _scores_f32, _count, _fill and _pool.  The last check before their launch is the grid's
# 2^31 cap, so the base call asks for 2^36 pairs (2^32 blocks at 16 pairs a block, 2^34 at 4) with every pointer given and comes back
# SS_ERR_INVALID_ARG; the edits are the bad-argument classes in front of it and the early SS_OK exit of an empty batch.  The letters were
# produced by the library as it stood before the five host preambles became one launcher (csrc/ss_pair_rows.hpp).
def _pair_entries():
    def sizes(*pointers):
        return [('N < 0', _edit(N=-1)), ('B < 0', _edit(B=-1)), ('N = 2^31', _edit(N=1 << 31)),
                ('B = 0, no pointers', _edit(B=0, **{name: None for name in pointers}))]

    def missing(*names):
        return [('no ' + name, _edit(**{name: None})) for name in names]

    entries = {}
    csr = dict(rowptr=_FAKE, col=_FAKE, val=_FAKE, mult=_FAKE, N=4, links=_FAKE, B=1 << 36, err_flag=_FAKE)
    scores = (dict(csr, out=_FAKE), ('rowptr', 'col', 'val', 'mult', 'N', 'links', 'B', 'out', 'err_flag', None),
              sizes('rowptr', 'col', 'val', 'mult', 'links', 'out', 'err_flag') + missing('rowptr', 'col', 'links', 'out')
              + [('no val, mult, err_flag', _edit(val=None, mult=None, err_flag=None)), ('B = 2^35', _edit(B=1 << 35))])
    entries['ss_common_neighbour_scores'] = entries['ss_common_neighbour_scores_f32'] = scores
    entries['ss_common_neighbour_count'] = (
        dict(csr, counts=_FAKE), ('rowptr', 'col', 'N', 'links', 'B', 'counts', 'err_flag', None),
        sizes('rowptr', 'col', 'links', 'counts', 'err_flag') + missing('rowptr', 'col', 'links', 'counts', 'err_flag')
        + [('B = 2^35', _edit(B=1 << 35))])
    entries['ss_common_neighbour_fill'] = (
        dict(csr, offsets=_FAKE, ids=_FAKE, coef=_FAKE),
        ('rowptr', 'col', 'val', 'mult', 'N', 'links', 'B', 'offsets', 'ids', 'coef', 'err_flag', None),
        sizes('rowptr', 'col', 'val', 'mult', 'links', 'offsets', 'ids', 'coef', 'err_flag')
        + missing('rowptr', 'col', 'links', 'offsets', 'ids') + [('no val, mult, coef, err_flag', _edit(val=None, mult=None, coef=None, err_flag=None)),
                                                                 ('B = 2^35', _edit(B=1 << 35))])
    entries['ss_common_neighbour_pool'] = (
        dict(csr, x=_FAKE, F=128, out=_FAKE), ('rowptr', 'col', 'val', 'mult', 'N', 'links', 'B', 'x', 'F', 'out', 'err_flag', None),
        sizes('rowptr', 'col', 'val', 'mult', 'links', 'x', 'out', 'err_flag') + missing('rowptr', 'col', 'links')
        + [('no val, mult, err_flag', _edit(val=None, mult=None, err_flag=None)), ('F < 0', _edit(F=-1)),
           ('F = 0, no x, no out', _edit(F=0, x=None, out=None)), ('F = 0', _edit(F=0)), ('F > 0, no x', _edit(x=None)),
           ('F > 0, no out', _edit(out=None)), ('F = 1024 (64 lanes)', _edit(F=1024)), ('B = 2^35', _edit(B=1 << 35))])
    return entries


_PAIR_PINNED = {
    'ss_common_neighbour_scores': {
        'base call': 'I',
        'N < 0': 'IIIIIIIIII',
        'B < 0': 'III0IIIIII',
        'N = 2^31': 'IIIIIIIIII',
        'B = 0, no pointers': 'III000000I',
        'no rowptr': 'III0IIIIII',
        'no col': 'III0IIIIII',
        'no links': 'III0IIIIII',
        'no out': 'III0IIIIII',
        'no val, mult, err_flag': 'III0IIIIII',
        'B = 2^35': 'III0IIIIII',
    },
    'ss_common_neighbour_scores_f32': {
        'base call': 'I',
        'N < 0': 'IIIIIIIIII',
        'B < 0': 'III0IIIIII',
        'N = 2^31': 'IIIIIIIIII',
        'B = 0, no pointers': 'III000000I',
        'no rowptr': 'III0IIIIII',
        'no col': 'III0IIIIII',
        'no links': 'III0IIIIII',
        'no out': 'III0IIIIII',
        'no val, mult, err_flag': 'III0IIIIII',
        'B = 2^35': 'III0IIIIII',
    },
    'ss_common_neighbour_count': {
        'base call': 'I',
        'N < 0': 'IIIIIIIIII',
        'B < 0': 'III0IIIIII',
        'N = 2^31': 'IIIIIIIIII',
        'B = 0, no pointers': 'III000000I',
        'no rowptr': 'III0IIIIII',
        'no col': 'III0IIIIII',
        'no links': 'III0IIIIII',
        'no counts': 'III0IIIIII',
        'no err_flag': 'III0IIIIII',
        'B = 2^35': 'III0IIIIII',
    },
    'ss_common_neighbour_fill': {
        'base call': 'I',
        'N < 0': 'IIIIIIIIIII',
        'B < 0': 'III0IIIIIII',
        'N = 2^31': 'IIIIIIIIIII',
        'B = 0, no pointers': 'III0000000I',
        'no rowptr': 'III0IIIIIII',
        'no col': 'III0IIIIIII',
        'no links': 'III0IIIIIII',
        'no offsets': 'III0IIIIIII',
        'no ids': 'III0IIIIIII',
        'no val, mult, coef, err_flag': 'III0IIIIIII',
        'B = 2^35': 'III0IIIIIII',
    },
    'ss_common_neighbour_pool': {
        'base call': 'I',
        'N < 0': 'IIIIIIIIIIIIIII',
        'B < 0': 'III0IIIIIIIIIII',
        'N = 2^31': 'IIIIIIIIIIIIIII',
        'B = 0, no pointers': 'III00000I00000I',
        'no rowptr': 'III0IIIIIIIIIII',
        'no col': 'III0IIIIIIIIIII',
        'no links': 'III0IIIIIIIIIII',
        'no val, mult, err_flag': 'III0IIIIIIIIIII',
        'F < 0': 'IIIIIIIIIIIIIII',
        'F = 0, no x, no out': 'III0IIIIIIIIIII',
        'F = 0': 'III0IIIIIIIIIII',
        'F > 0, no x': 'III0IIIIIIIIIII',
        'F > 0, no out': 'III0IIIIIIIIIII',
        'F = 1024 (64 lanes)': 'III0IIIIIIIIIII',
        'B = 2^35': 'III0IIIIIIIIIII',
    },
}


@pytest.mark.parametrize('entry', sorted(_pair_entries()))
def test_common_neighbour_return_codes_are_pinned(entry):
    """every bad-argument class of the five common-neighbour entry points, alone and in pairs, and the empty batch's SS_OK: the codes
    of the library before their preambles were merged (a '?' would be a code outside the four: a launch was reached)"""
    import subgraph_sketching_amd as ssa
    nat = ssa._native
    state, order, _ = _pair_entries()[entry]
    base = _return_code(nat.lib(), nat, entry, state, order, [])
    assert _LETTER.get(base) == _PAIR_PINNED[entry]['base call'], base
    got = _return_code_rows(entry, _pair_entries())
    assert [name for name, _ in got] == [name for name in _PAIR_PINNED[entry] if name != 'base call']
    for name, row in got:
        assert row == _PAIR_PINNED[entry][name], (entry, name, row, _PAIR_PINNED[entry][name])


# ---- return codes of the link-query entry points ---------------------------------------------------------------------------------
# The same scheme for the pair queries (ss_pairs.hip), the one-vs-all scans (ss_topk.hip, ss_topk_head.hip, ss_rank.hip), the masked
# query and the two permutation passes.  Base calls, none of which an edit can turn into a launch: the pair queries get a table-pointer
# array whose last entry is null; ss_topk_scan 32 * 65 535 + 1 sources and the head scans 8 * 65 535 + 1 entries with every byte of keys
# "given" (grid.y is the failing check); ss_topk_exclude keys one byte short and ss_masked_pair_features a workspace of 0 bytes;
# ss_gather_links a links pointer that is not 16-byte aligned; ss_scatter_feature_rows, which has no check that fails without a launch
# behind it, n = 0 (its edits give n > 0 only together with a missing pointer).  The orders the code marks as deliberate show in the
# rows: ss_pair_scores answers B = 0 before it looks at prm, the feature queries after it but before P.  The letters were produced by
# the library as it stood before the host side of these units was rewritten around one request record and one shape dispatcher.
def _link_query_entries():
    F = _FAKE
    head = dict(dim=8, normalised=0, w1=F, shift=F, w2=F, bias=0.5)   # a plain head of h = 2
    hops = [('h = 0', _edit(h=0)), ('h = 4', _edit(h=4))]
    width = [('P = 0', _edit(P=0)), ('P = 130', _edit(P=130)), ('P = 2052', _edit(P=2052)), ('P = 100', _edit(P=100))]
    tables = [('no mh', _edit(mh=None)), ('no hll', _edit(hll=None)), ('mh[0] null', _edit(mh=[None, F])), ('hll whole, no mh', _edit(hll=[F, F], mh=None)),
              ('no cards', _edit(cards=None)), ('cards_stride < h', _edit(cards_stride=1))]
    heads = [('no head', _edit(head=None)), ('head.dim = 15', _edit(**{'head.dim': 15})), ('head.w2 null', _edit(**{'head.w2': None})),
             ('degrees with a plain head', _edit(degrees=F)),
             ('normalised head without degrees', _edit(degrees=None, **{'head.dim': 16, 'head.normalised': 1})),
             ('normalised head with degrees', _edit(degrees=F, **{'head.dim': 16, 'head.normalised': 1}))]

    def sizes(n, ceilings):
        return ([(f'{n} < 0', _edit(**{n: -1})), (f'{n} = 0', _edit(**{n: 0})), ('N < 0', _edit(N=-1)), ('N = 0', _edit(N=0))]
                + [(f'N = {name}', _edit(N=value)) for name, value in ceilings])

    pair_n = [('2^31', 1 << 31)]
    scan_n = [('2^32 - 2', (1 << 32) - 2), ('2^32 - 1', (1 << 32) - 1), ('2^32', 1 << 32)]
    ordered = [('no order', _edit(order=None)), ('B = 2^31', _edit(B=1 << 31)), ('B = 2^31, no order', _edit(B=1 << 31, order=None))]
    entries = {}
    pq = dict(_state(links=F, B=4, N=4, h=2, mh=[F, F], P=128, hll=[F, None], cards=F, cards_stride=2, flags=0, out=F, err_flag=F), g=None)
    entries['ss_pair_features'] = (
        dict(pq, dbg_match=F, dbg_zero=F, dbg_inter=F),
        ('links', 'B', 'N', 'h', 'mh', 'P', 'hll', 'cards', 'cards_stride', 'prm', 'flags', 'out', 'dbg_match', 'dbg_zero', 'dbg_inter',
         'err_flag', None),
        hops + sizes('B', pair_n) + [('no links', _edit(links=None)), ('no out', _edit(out=None)),
                                     ('no dbg, no err_flag', _edit(dbg_match=None, dbg_zero=None, dbg_inter=None, err_flag=None))]
        + tables + width + _prm_edits())
    entries['ss_pair_features_normalised'] = (
        dict(pq, degrees=F),
        ('links', 'B', 'N', 'h', 'mh', 'P', 'hll', 'cards', 'cards_stride', 'prm', 'flags', 'degrees', 'out', 'err_flag', None),
        hops + sizes('B', pair_n) + [('no links', _edit(links=None)), ('no out', _edit(out=None)), ('no degrees', _edit(degrees=None)),
                                     ('no err_flag', _edit(err_flag=None))] + tables + width + _prm_edits())
    grouped_order = ('links', 'order', 'B', 'N', 'h', 'mh', 'P', 'hll', 'cards', 'cards_stride', 'prm', 'flags', 'degrees', 'out', 'err_flag', None)
    grouped = (hops + sizes('B', pair_n) + ordered + [('no links', _edit(links=None)), ('no out', _edit(out=None)),
                                                      ('no degrees, no err_flag', _edit(degrees=None, err_flag=None)), ('h = 1', _edit(h=1, hll=[None, F]))]
               + tables + width + _prm_edits())
    entries['ss_pair_features_grouped'] = (dict(pq, order=F, degrees=F), grouped_order, grouped)
    entries['ss_pair_features_grouped_kernel'] = (
        dict(pq, order=F, degrees=F, which=1), ('which',) + grouped_order,
        [('which = -1', _edit(which=-1)), ('which = 2', _edit(which=2)), ('which = 0', _edit(which=0))] + grouped)
    entries['ss_pair_scores'] = (
        dict(pq, order=F, degrees=None, head=head),
        ('links', 'order', 'B', 'N', 'h', 'mh', 'P', 'hll', 'cards', 'cards_stride', 'prm', 'flags', 'degrees', 'head', 'out', 'err_flag', None),
        hops + sizes('B', pair_n) + ordered + [('no links', _edit(links=None)), ('no out', _edit(out=None)), ('no err_flag', _edit(err_flag=None))]
        + tables + heads + width + _prm_edits())
    S_y = 32 * 65535 + 1
    entries['ss_topk_scan'] = (
        dict(_state(sources=F, S=S_y, N=4, mh_src=F, hll_src=F, mh_cand=F, hll_cand=F, P=128, keys=F, keys_bytes=(1 << 64) - 1, err_flag=F), g=None),
        ('sources', 'S', 'N', 'mh_src', 'hll_src', 'mh_cand', 'hll_cand', 'P', 'prm', 'keys', 'keys_bytes', 'err_flag', None),
        sizes('S', scan_n) + [('no ' + name, _edit(**{name: None})) for name in ('sources', 'mh_src', 'hll_src', 'mh_cand', 'hll_cand', 'keys', 'err_flag')]
        + [('keys_bytes one short', _edit(keys_bytes=8 * 4 * S_y - 1)), ('keys_bytes exact', _edit(keys_bytes=8 * 4 * S_y))] + width + _prm_edits())
    entries['ss_topk_exclude'] = (
        dict(sources=F, S=4, N=4, rowptr=F, col=F, keys=F, keys_bytes=8 * 4 * 4 - 1),
        ('sources', 'S', 'N', 'rowptr', 'col', 'keys', 'keys_bytes', None),
        sizes('S', scan_n) + [('no ' + name, _edit(**{name: None})) for name in ('sources', 'rowptr', 'col', 'keys')]
        + [('keys_bytes = 0', _edit(keys_bytes=0))])
    n_y = 8 * 65535 + 1
    hs = dict(_state(N=4, h=2, mh=[F, F], hll=[F, F], P=128, cards=F, cards_stride=2, flags=0, degrees=None, head=head, err_flag=F), g=None)
    scan_tables = [e for e in tables if e[0] != 'hll whole, no mh'] + [('hll[1] null', _edit(hll=[F, None]))]
    entries['ss_topk_score_scan'] = (
        dict(hs, sources=F, S=n_y, keys=F, keys_bytes=(1 << 64) - 1),
        ('sources', 'S', 'N', 'h', 'mh', 'hll', 'P', 'cards', 'cards_stride', 'prm', 'flags', 'degrees', 'head', 'keys', 'keys_bytes', 'err_flag', None),
        hops + sizes('S', scan_n) + [('no sources', _edit(sources=None)), ('no keys', _edit(keys=None)), ('no err_flag', _edit(err_flag=None)),
                                     ('keys_bytes one short', _edit(keys_bytes=8 * 4 * n_y - 1))] + scan_tables + heads + width + _prm_edits())
    entries['ss_rank_score_scan'] = (
        dict(hs, links=F, thr=F, L=n_y, counts=F),
        ('links', 'thr', 'L', 'N', 'h', 'mh', 'hll', 'P', 'cards', 'cards_stride', 'prm', 'flags', 'degrees', 'head', 'counts', 'err_flag', None),
        hops + sizes('L', scan_n) + [('no links', _edit(links=None)), ('no thr', _edit(thr=None)), ('no counts', _edit(counts=None)),
                                     ('no err_flag', _edit(err_flag=None))] + scan_tables + heads + width + _prm_edits())
    entries['ss_masked_pair_features'] = (
        dict(_state(links=F, B=4, N=4, h=2, a=F, b=F, mh=[F, F], P=128, hll=[F, F], cards=F, cards_stride=2, flags=0, out=F, dbg_match=F, dbg_zero=F,
                    dbg_row_zeros=F, dbg_masked=F, err_flag=F, workspace=F, workspace_bytes=0), g=dict(_state()['g'], row_begin=0, row_end=0)),
        ('g', 'links', 'B', 'N', 'h', 'a', 'b', 'mh', 'P', 'hll', 'cards', 'cards_stride', 'prm', 'flags', 'out', 'dbg_match', 'dbg_zero',
         'dbg_row_zeros', 'dbg_masked', 'err_flag', 'workspace', 'workspace_bytes', None),
        hops + sizes('B', pair_n) + [('B = 2^31', _edit(B=1 << 31)), ('N = 2^31 in the graph too', _edit(N=1 << 31, **{'g.num_nodes': 1 << 31})),
                                     ('no graph', _edit(g=None)), ('no rowptr', _edit(**{'g.rowptr': None})), ('no col', _edit(**{'g.col': None})),
                                     ('a row range', _edit(**{'g.row_begin': 1, 'g.row_end': 3})), ('no a', _edit(a=None)), ('no b', _edit(b=None)),
                                     ('no workspace', _edit(workspace=None)), ('no links', _edit(links=None)), ('no out', _edit(out=None)),
                                     ('no dbg, no err_flag', _edit(dbg_match=None, dbg_zero=None, dbg_row_zeros=None, dbg_masked=None, err_flag=None)),
                                     ('P = 1024 (272 chunks)', _edit(P=1024))]
        + [e for e in tables if e[0] != 'hll whole, no mh'] + width + _prm_edits())
    entries['ss_gather_links'] = (
        dict(links=F, order=F, n=4, out_links=16), ('links', 'order', 'n', 'out_links', None),
        [('n < 0', _edit(n=-1)), ('n = 0', _edit(n=0)), ('n = 0, no pointers', _edit(n=0, links=None, order=None, out_links=None)),
         ('no links', _edit(links=None)), ('no order', _edit(order=None)), ('no out_links', _edit(out_links=None)),
         ('out_links unaligned too', _edit(out_links=F))])
    entries['ss_scatter_feature_rows'] = (
        dict(rows=F, order=F, n=0, width=8, out=F), ('rows', 'order', 'n', 'width', 'out', None),
        [('n < 0', _edit(n=-1)), ('width = 0', _edit(width=0)), ('width < 0', _edit(width=-1)), ('n = 0, no pointers', _edit(rows=None, order=None, out=None)),
         ('n = 4, no rows', _edit(n=4, rows=None)), ('n = 4, no order', _edit(n=4, order=None)), ('n = 4, no out', _edit(n=4, out=None))])
    return entries


_LINK_PINNED = {
    'ss_pair_features': {
        'base call': 'I',
        'h = 0': 'UUUUUUUUUUUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUUUUUUUUUUUUU',
        'B < 0': 'UUI0IIIIIIIIIIIIIIIIIIIII',
        'B = 0': 'UUI0I000000000000000IUII0',
        'N < 0': 'UUIIIIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'N = 2^31': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'no links': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'no out': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'no dbg, no err_flag': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'no mh': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'no hll': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'hll whole, no mh': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'no cards': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'cards_stride < h': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'P = 0': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'UUI0IIIIIIIIIIIIIIIIIUIII',
        'no prm': 'UUIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUIUIUUUUUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'UUIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'UUIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'UUI0IIIIIIIIIIIIIIIIIUIII',
    },
    'ss_pair_features_normalised': {
        'base call': 'I',
        'h = 0': 'UUUUUUUUUIUUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUIUUUUUUUUUUUUUUUU',
        'B < 0': 'UUI0IIIIIIIIIIIIIIIIIIIIII',
        'B = 0': 'UUI0I0000I00000000000IUII0',
        'N < 0': 'UUIIIIIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'N = 2^31': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'no links': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'no out': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'no degrees': 'IIIIIIIIIIIIIIIIIIIIIIIIII',
        'no err_flag': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'no mh': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'no hll': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'hll whole, no mh': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'no cards': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'cards_stride < h': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'P = 0': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
        'no prm': 'UUIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUIUIUUUUIUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'UUIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'UUIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'UUI0IIIIIIIIIIIIIIIIIIUIII',
    },
    'ss_pair_features_grouped': {
        'base call': 'I',
        'h = 0': 'UUUUUUUUUUUUUIUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUIUUUUUUUUUUUUUUU',
        'B < 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIII',
        'B = 0': 'UUI0I000II00000000000000IUII0',
        'N < 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^31': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no order': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'B = 2^31': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'B = 2^31, no order': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no links': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no out': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no degrees, no err_flag': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'h = 1': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no mh': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no hll': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'hll whole, no mh': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no cards': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'cards_stride < h': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no prm': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUIUIUUUUUUUUUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'UUIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'UUIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'UUI0IIIIIIIIIIIIIIIIIIIIIUIII',
    },
    'ss_pair_features_grouped_kernel': {
        'base call': 'I',
        'which = -1': 'IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'which = 2': 'IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'which = 0': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'h = 0': 'IIUUUUUUUUUUUUUUIUUUUUUUUUUUUUUU',
        'h = 4': 'IIUUUUUUUUUUUUUUIUUUUUUUUUUUUUUU',
        'B < 0': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIIIII',
        'B = 0': 'II0UUI0I000II00000000000000IUII0',
        'N < 0': 'IIIUUIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^31': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no order': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'B = 2^31': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'B = 2^31, no order': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no links': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no out': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no degrees, no err_flag': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'h = 1': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no mh': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no hll': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'hll whole, no mh': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no cards': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'cards_stride < h': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 0': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
        'no prm': 'IIIUUIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'IIUUUIUIUUUUUUUUUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'IIIUUIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'IIIUUIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'IIIUUI0IIIIIIIIIIIIIIIIIIIIIUIII',
    },
    'ss_pair_scores': {
        'base call': 'I',
        'h = 0': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'B < 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'B = 0': 'UUI0I000II000000000000000000000000',
        'N < 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^31': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no order': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'B = 2^31': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'B = 2^31, no order': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no links': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no out': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no err_flag': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no mh': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no hll': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'hll whole, no mh': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no cards': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'cards_stride < h': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no head': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'head.dim = 15': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'head.w2 null': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'degrees with a plain head': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'normalised head without degrees': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'normalised head with degrees': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no prm': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUI0IUUUUUUUUUUUUUUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
    },
    'ss_topk_scan': {
        'base call': 'I',
        'S < 0': 'I0IIIIIIIIIIIIIIIIIIIUIII',
        'S = 0': 'I0II0II000000000III0IUII0',
        'N < 0': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 0': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32 - 2': 'I0IIIIIIIIIIIIWWIIIIIUIII',
        'N = 2^32 - 1': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'no sources': 'I0IIIIIIIIIIIIIIIIIIIUIII',
        'no mh_src': 'I0IIIIIIIIIIIIIIIIIIIUIII',
        'no hll_src': 'I0IIIIIIIIIIIIIIIIIIIUIII',
        'no mh_cand': 'I0IIIIIIIIIIIIIIIIIIIUIII',
        'no hll_cand': 'I0IIIIIIIIIIIIIIIIIIIUIII',
        'no keys': 'I0IIIIIIIIIIIIIIIIIIIUIII',
        'no err_flag': 'I0IIIIIIIIIIIIWIIIIIIUIII',
        'keys_bytes one short': 'I0IIWIIIIIIIIWWIIIIWIUIIW',
        'keys_bytes exact': 'I0IIWIIIIIIIIIWIIIIIIUIII',
        'P = 0': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'I0IIIIIIIIIIIIWIIIIIIUIII',
        'no prm': 'IIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUUUUUUUUUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'IIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'I0IIIIIIIIIIIIWIIIIIIUIII',
    },
    'ss_topk_exclude': {
        'base call': 'W',
        'S < 0': 'I0IIIIIIIIII',
        'S = 0': 'I0II0II00000',
        'N < 0': 'IIIIWIIIIIII',
        'N = 0': 'IIIIWIIIIIII',
        'N = 2^32 - 2': 'I0IIWIIIIIIW',
        'N = 2^32 - 1': 'IIIIWIIIIIII',
        'N = 2^32': 'IIIIWIIIIIII',
        'no sources': 'I0IIIIIIIIII',
        'no rowptr': 'I0IIIIIIIIII',
        'no col': 'I0IIIIIIIIII',
        'no keys': 'I0IIIIIIIIII',
        'keys_bytes = 0': 'I0IIWIIIIIIW',
    },
    'ss_topk_score_scan': {
        'base call': 'I',
        'h = 0': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'S < 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'S = 0': 'UUI0II0II0000000000000000III0IUII0',
        'N < 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32 - 2': 'UUI0IIIIIIIIWIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32 - 1': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no sources': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no keys': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no err_flag': 'UUI0IIIIIIIIWIIIIIIIIIIIIIIIIIUIII',
        'keys_bytes one short': 'UUI0IIWIIIIWWIIWIIWIIIIIWIIIWIUIIW',
        'no mh': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no hll': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'UUI0IIIIIIIIWIIIIIIIIIIIIIIIIIUIII',
        'no cards': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'cards_stride < h': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'hll[1] null': 'UUI0IIIIIIIIWIIIIIIIIIIIIIIIIIUIII',
        'no head': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'head.dim = 15': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'head.w2 null': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'degrees with a plain head': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'normalised head without degrees': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'normalised head with degrees': 'UUI0IIIIIIIIWIIIIIIIIIIIIIIIIIUIII',
        'P = 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'UUI0IIIIIIIIWIIIIIIIIIIIIIIIIIUIII',
        'no prm': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'UUI0IIIIIIIIWIIIIIIIIIIIIIIIIIUIII',
    },
    'ss_rank_score_scan': {
        'base call': 'I',
        'h = 0': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'L < 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'L = 0': 'UUI0II00I0000000000000000III0IUII0',
        'N < 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32 - 2': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32 - 1': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^32': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no links': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no thr': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no counts': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no err_flag': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no mh': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no hll': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no cards': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'cards_stride < h': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'hll[1] null': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no head': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'head.dim = 15': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'head.w2 null': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'degrees with a plain head': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'normalised head without degrees': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'normalised head with degrees': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 130': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 2052': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'P = 100': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no prm': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUIUUUI',
        'prm.n_tbl = 5': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
    },
    'ss_masked_pair_features': {
        'base call': 'W',
        'h = 0': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'h = 4': 'UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU',
        'B < 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'B = 0': 'UUI0I0III00000000000000000000IUII0',
        'N < 0': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'N = 0': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'N = 2^31': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'B = 2^31': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'N = 2^31 in the graph too': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'no graph': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no rowptr': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no col': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'a row range': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no a': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no b': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no workspace': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'no links': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
        'no out': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
        'no dbg, no err_flag': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
        'P = 1024 (272 chunks)': 'UUI0IIIIIIIIIIIIUUUUIIUUUIIIWIUIIU',
        'no mh': 'UUI0IIIIIIIIIIIIIIIIIIWIIIIIIIUIII',
        'no hll': 'UUI0IIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'mh[0] null': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
        'no cards': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
        'cards_stride < h': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
        'P = 0': 'UUI0IIIIIIIIIIIIIIIUIIIIIIIIWIUIII',
        'P = 130': 'UUI0IIIIIIIIIIIIIIIUIIIIIIIIWIUIII',
        'P = 2052': 'UUI0IIIIIIIIIIIIIIIUIIIIIIIIWIUIII',
        'P = 100': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
        'no prm': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII',
        'prm.p = 3': 'UUIUIUIIIUUUUUUUUUUUUUUUUUUUUIUUUW',
        'prm.n_tbl = 5': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.bias missing': 'UUIIIIIIIIIIIIIIIIIIIIIIIIIIIIUIII',
        'prm.p = 9': 'UUI0IIIIIIIIIIIIWWWUIIWWWIIIWIUIIW',
    },
    'ss_gather_links': {
        'base call': 'I',
        'n < 0': 'I00IIII',
        'n = 0': 'I000000',
        'n = 0, no pointers': 'I000000',
        'no links': 'I00IIII',
        'no order': 'I00IIII',
        'no out_links': 'I00IIII',
        'out_links unaligned too': 'I00IIII',
    },
    'ss_scatter_feature_rows': {
        'base call': '0',
        'n < 0': 'IIIIIII',
        'width = 0': 'IIIIIII',
        'width < 0': 'IIIIIII',
        'n = 0, no pointers': 'III0III',
        'n = 4, no rows': 'IIIIIII',
        'n = 4, no order': 'IIIIIII',
        'n = 4, no out': 'IIIIIII',
    },
}


@pytest.mark.parametrize('entry', sorted(_link_query_entries()))
def test_link_query_return_codes_are_pinned(entry):
    """every bad-argument class of the link-query entry points, alone and in pairs, and their early SS_OK exits: the codes of the
    library before the host side of these units was refactored (a '?' would be a code outside the four: a launch was reached)"""
    import subgraph_sketching_amd as ssa
    nat = ssa._native
    state, order, _ = _link_query_entries()[entry]
    base = _return_code(nat.lib(), nat, entry, state, order, [])
    assert _LETTER.get(base) == _LINK_PINNED[entry]['base call'], base
    got = _return_code_rows(entry, _link_query_entries())
    assert [name for name, _ in got] == [name for name in _LINK_PINNED[entry] if name != 'base call']
    for name, row in got:
        assert row == _LINK_PINNED[entry][name], (entry, name, row, _LINK_PINNED[entry][name])


def test_missing_library_fails_loudly(monkeypatch):
    import subgraph_sketching_amd as ssa
    monkeypatch.setattr(ssa._native, '_lib', None)
    monkeypatch.setattr(ssa._native, 'LIB_PATH', '/nonexistent/libsubgraph_sketch.so')
    with pytest.raises(ssa._native.NativeLibraryMissing):
        ssa._native.lib()
