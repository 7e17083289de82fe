"""Incremental update of the sketch tables (ElphHashes.update_hash_tables, csrc/ss_update.hip): after a few edges were added or
removed, hop k recomputes only the rows within k hops downstream of the touched targets; every other row of every hop is already what
build_hash_tables (reference hashing.py:139-165) would give on the changed graph.

Host side only: argument checks, the CSR of the new graph (built as build_hash_tables builds it), the workspace, one marking call and
one call per hop.  Nothing between the first and the last launch reads from the device."""
from ctypes import byref, c_void_p

import torch

from . import _native, hll_tables
from ._runtime import _Span, _compute_device, _error_flag, _ptr, _stream, _take_error
from .containers import HopSketch, SketchTable, _stamp_tables, unpack_minhash
from .csr import build_csr


def _is_int_tensor(t):
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _edge_list(x, name):
    t = torch.as_tensor(x)
    if t.dim() != 2 or t.size(0) != 2 or not _is_int_tensor(t):
        raise ValueError(f'{name} must be an integer tensor of shape [2, n], got {t.dtype} {tuple(t.shape)}')
    return t


def check_arguments(eh, hash_table, cards, num_nodes, edge_index, added, removed):
    """every check that needs no device -> (N, edge_index, added, removed, [HopSketch of hops 1 .. h])"""
    h = eh.max_hops
    if added is None and removed is None:
        raise ValueError('update_hash_tables needs the changed edges: give `added`, `removed` or both')
    N = int(num_nodes)
    if N < 0 or N >= (1 << 31):
        raise ValueError(f'num_nodes must lie in [0, 2^31), got {N}')
    ei = _edge_list(edge_index, 'edge_index')
    add = _edge_list(added, 'added') if added is not None else None
    rem = _edge_list(removed, 'removed') if removed is not None else None
    if not isinstance(cards, torch.Tensor) or cards.dim() != 2 or tuple(cards.shape) != (N, h) or cards.dtype != torch.float32:
        raise ValueError(f'cards must be the float32 [{N}, {h}] tensor build_hash_tables returned, got '
                         f'{getattr(cards, "dtype", type(cards))} {tuple(getattr(cards, "shape", ()))}')
    made_with = getattr(cards, '_ss_tables', None)
    if made_with is not None and not hll_tables.same_tables(made_with, eh.tables_id):
        raise ValueError(f'cards were estimated with HLL++ tables {made_with}, this engine uses {eh.tables_id}: '
                         f'updated rows would mix two bias tables (rebuild, or load the same tables)')
    entries = []
    for k in range(h + 1):
        if not hasattr(hash_table, 'get') or hash_table.get(k) is None:
            raise ValueError(f'hash_table must hold hops 0 .. {h} (what build_hash_tables returned), hop {k} is missing')
        if k == 0:
            continue
        entry = hash_table[k]
        if not isinstance(entry, HopSketch):
            raise ValueError(f'hop {k} must be a HopSketch (build_hash_tables / load_sketches of a packed cache), got {type(entry).__name__}')
        mh, hll = entry.mh_u32, entry.hll_u8
        if mh.dim() != 2 or hll.dim() != 2 or tuple(mh.shape) != (N, eh.num_perm) or tuple(hll.shape) != (N, eh.m):
            raise ValueError(f'hash tables of different hops must have the same shape: hop {k} holds MinHash {tuple(mh.shape)} and HLL '
                             f'{tuple(hll.shape)}, expected [{N}, {eh.num_perm}] and [{N}, {eh.m}]')
        entries.append(entry)
    return N, ei, add, rem, entries


def _refresh_leaves(entry, mh, hll):
    """reference-shaped leaves a caller materialised before the update must not go stale: they are rewritten from the updated
    packed tables (the int8 HLL leaf usually IS a view of the packed table and needs nothing)"""
    for key, leaf in list(entry._leaves.items()):
        if key == 'minhash':
            leaf.copy_(unpack_minhash(mh))
        elif leaf.data_ptr() != hll.data_ptr():
            leaf.copy_(hll.view(torch.int8))
        entry._leaf_versions[key] = leaf._version


HEADER_BYTES = 256  # kUpdHeaderBytes of ss_update.hip


def carve_workspace(ws, num_nodes, h):
    """the workspace of ss_update_mark / ss_update_hop carved exactly as carve_update_ws (ss_update.hip) carves it -> (counters,
    maps, lists), all views of `ws` (uint8, ss_update_workspace_bytes(N, h) long):
      counters  int32 [64]: word 0 = seed rows, words 4k .. 4k+2 = hop k's dirty rows, row-list length, hub-list length
      maps      h byte maps uint8 [N] (1 = dirty at that hop), pad(N) = (N + 255) & ~255 bytes apart
      lists     h int32 [pad(N)] lists: the regular rows fill one from the front, the hub rows from index N - 1 downwards"""
    N = int(num_nodes)
    pad = (N + 255) & ~255
    counters = ws[:HEADER_BYTES].view(torch.int32)
    maps = [ws[HEADER_BYTES + k * pad:HEADER_BYTES + k * pad + N] for k in range(h)]
    first = HEADER_BYTES + h * pad
    lists = [ws[first + 4 * k * pad:first + 4 * (k + 1) * pad].view(torch.int32) for k in range(h)]
    return counters, maps, lists


def workspace_info(ws, num_nodes, h, masks=False):
    """the `info` of update_hash_tables read from a marked workspace (one host read of the counters)"""
    counters, maps, lists = carve_workspace(ws, num_nodes, h)
    words = counters[:4 * (h + 1)].cpu().tolist()
    hops = range(1, h + 1)
    info = {'seed_rows': words[0], 'dirty_rows': {k: words[4 * k] for k in hops}, 'row_list': {k: words[4 * k + 1] for k in hops},
            'hub_list': {k: words[4 * k + 2] for k in hops}}
    if masks:
        N = int(num_nodes)
        info['dirty_mask'] = {k: maps[k - 1] != 0 for k in hops}
        info['rows'] = {k: lists[k - 1][:info['row_list'][k]].clone() for k in hops}
        info['hubs'] = {k: lists[k - 1][N - info['hub_list'][k]:N].flip(0) for k in hops}  # in the order the hub kernels take them
    return info


def update_hash_tables(eh, hash_table, cards, num_nodes, edge_index, added=None, removed=None, copy=False, return_info=False):
    """see ElphHashes.update_hash_tables"""
    h = eh.max_hops
    if return_info not in (False, True, 'masks'):
        raise ValueError(f"return_info must be False, True or 'masks', got {return_info!r}")
    N, ei, add, rem, entries = check_arguments(eh, hash_table, cards, num_nodes, edge_index, added, removed)
    if not cards.is_cuda or any(e.mh_u32.device != cards.device or e.hll_u8.device != cards.device for e in entries):
        raise ValueError('update_hash_tables updates the packed tables where they live: hash_table and cards must be on the compute device')
    device = cards.device
    params = eh._params(device)
    lib = _native.lib()
    # the packed twins (a leaf edited in place is packed first, as for a query), cloned for copy=True
    packed = [e.packed(device) for e in entries]
    if copy:
        table = SketchTable()
        table[0] = hash_table[0]  # hop 0 is a pure function of the node id: never changes, shared
        packed = [(m.clone(), l.clone()) for m, l in packed]
        for k, (e, (m, l)) in enumerate(zip(entries, packed), start=1):
            table[k] = HopSketch(m, l, e.home)
        out_cards = _stamp_tables(cards.clone(), getattr(cards, '_ss_tables', None) or eh.tables_id)
        out_entries = [table[k] for k in range(1, h + 1)]
    else:
        table, out_cards, out_entries = hash_table, cards, entries
        if getattr(cards, '_ss_tables', None) is None:
            _stamp_tables(cards, eh.tables_id)
    if out_cards.stride(1) != 1 or out_cards.stride(0) < h:
        raise ValueError('cards must be a row-major tensor')
    if N == 0:
        if not return_info:
            return table, out_cards
        none = {k: 0 for k in range(1, h + 1)}
        info = {'seed_rows': 0, 'dirty_rows': dict(none), 'row_list': dict(none), 'hub_list': dict(none)}
        if return_info == 'masks':
            info['dirty_mask'] = {k: torch.zeros(0, dtype=torch.bool, device=device) for k in none}
            info['rows'] = {k: torch.zeros(0, dtype=torch.int32, device=device) for k in none}
            info['hubs'] = {k: torch.zeros(0, dtype=torch.int32, device=device) for k in none}
        return table, out_cards, info

    # the CSR of the graph AFTER the change, exactly as build_hash_tables builds it (implicit self loops below max(edge_index) + 1)
    check, err_flag = eh._bounds(device, f'update_hash_tables(num_nodes={N})')
    csr = build_csr(ei, N, device, check=check, err_flag=err_flag)
    csr.use_inferred_self_loops = True
    graph = csr.struct()
    err = _error_flag(device) if check else err_flag
    targets = [t[1].to(device=device, dtype=torch.int64).contiguous() if t is not None else None for t in (add, rem)]
    n_add, n_rem = (0 if t is None else t.numel() for t in targets)
    ws_bytes = int(lib.ss_update_workspace_bytes(N, h))
    if ws_bytes == 0:
        raise NotImplementedError(f'update_hash_tables does not support {N} nodes')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    stream = _stream(device)
    stride = out_cards.stride(0)
    with _Span('update_mark', device):
        _native.check(lib.ss_update_mark(byref(graph), _ptr(targets[0]), n_add, _ptr(targets[1]), n_rem, _ptr(out_cards), stride, h,
                                         _ptr(err), _ptr(ws), ws_bytes, stream), 'ss_update_mark')
    # hop 1 from node ids where the first-hop kernels of the build do so; the other shapes read the hop-0 tables
    P, p = eh.num_perm, eh.p
    ids_mh = eh.fuse_first_hop and P % 64 == 0 and P <= 256
    ids_hll = ids_mh and p == 8
    ab = eh._perms(device)
    for k in range(1, h + 1):
        mh_out, hll_out = packed[k - 1]
        if k == 1:
            zero = None if (ids_mh and ids_hll) else hash_table[0]
            if zero is not None and not isinstance(zero, HopSketch):
                raise ValueError(f'hop 0 must be a HopSketch for this sketch shape, got {type(zero).__name__}')
            mh_in = None if ids_mh else zero.packed(device)[0]
            hll_in = None if ids_hll else zero.packed(device)[1]
        else:
            mh_in, hll_in = packed[k - 2]
        with _Span(f'update_hop{k}', device):
            _native.check(lib.ss_update_hop(byref(graph), k, h, _ptr(ab[0]), _ptr(ab[1]), _ptr(mh_in), _ptr(mh_out), P, _ptr(hll_in), _ptr(hll_out),
                                            p, c_void_p(out_cards.data_ptr() + 4 * (k - 1)), stride, byref(params.struct), _ptr(ws), ws_bytes,
                                            stream), 'ss_update_hop')
    # ---- the last launch has been issued: everything below may read
    for e, (m, l) in zip(out_entries, packed):
        if not copy:
            e._mh_u32, e._hll_u8 = m, l
            _refresh_leaves(e, m, l)
    if check and _take_error(device):
        raise IndexError(f'added / removed refer to nodes outside [0, {N})')
    if not return_info:
        return table, out_cards
    return table, out_cards, workspace_info(ws, N, h, masks=return_info == 'masks')
