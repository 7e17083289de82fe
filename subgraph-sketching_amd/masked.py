"""Target-link masking (ElphHashes.get_subgraph_features(mask_target=edge_index), csrc/ss_masked.hip): every link is
scored as if its own edge were absent from the graph the tables were built on -- what the reference's SEAL path does by removing the
target link from the enclosing subgraph (src/datasets/seal.py:338) and its sketch path (hashing.py:139-165, 258-323) cannot.

Host side only: argument checks, the CSR (the engine's cache), the workspace, one call per batch and the output tensors.  Nothing
between the first and the last launch of a call reads from the device."""
from ctypes import byref, c_void_p

import torch

from . import _native, hll_tables
from ._runtime import _Span, _compute_device, _error_flag, _ptr, _stream, _take_error
from .containers import HopSketch


def _is_int_tensor(t):
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _check_row_chunks(num_perm, p):
    if (num_perm >> 2) + ((1 << p) >> 4) > 256:
        raise NotImplementedError(f'the masked query walks a sketch row with one 16-byte chunk per thread: num_perm / 4 + 2^hll_p / 16 must '
                                  f'not exceed 256, got {num_perm} and {p}')


def check_arguments(eh, links, mask_target, batch_size, degrees=None, lazy=False, out=None):
    """-> (links [L, 2], edge_index [2, E], batch_size) after every check that needs no device"""
    for name, given in (('degrees', degrees is not None), ('lazy', bool(lazy)), ('out', out is not None)):
        if given:
            raise ValueError(f'mask_target cannot be combined with {name}: the masked query returns plain feature rows in a tensor of its own')
    if eh.max_hops not in (1, 2, 3):
        raise NotImplementedError('Only 1, 2 and 3 hop hashes are implemented')
    _check_row_chunks(eh.num_perm, eh.p)
    lk = torch.as_tensor(links)
    if lk.dim() == 1:
        lk = lk.unsqueeze(0)
    if lk.dim() != 2 or lk.size(1) != 2 or not _is_int_tensor(lk):
        raise ValueError(f'links must be an integer [L, 2] (or [2]) tensor, got {lk.dtype} {tuple(lk.shape)}')
    ei = torch.as_tensor(mask_target)
    if ei.dim() != 2 or ei.size(0) != 2 or not _is_int_tensor(ei):
        raise ValueError(f'mask_target must be the integer edge_index [2, num_edges] the tables were built on, got {ei.dtype} {tuple(ei.shape)}')
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size must be positive, got {batch_size}')
    return lk, ei, batch_size


def masked_subgraph_features(eh, links, hash_table, cards, mask_target, batch_size=11000000, return_debug=False):
    """see ElphHashes.get_subgraph_features(mask_target=...)"""
    lk, ei, batch_size = check_arguments(eh, links, mask_target, batch_size)
    h = eh.max_hops
    home, L, nf = lk.device, lk.size(0), h * (h + 2)
    if cards is None:
        raise ValueError('the masked query needs cards (the cardinalities build_hash_tables returned)')
    made_with = getattr(cards, '_ss_tables', None)
    if made_with is not None and not hll_tables.same_tables(made_with, eh.tables_id):
        raise ValueError(f'cards were estimated with HLL++ tables {made_with}, this engine uses {eh.tables_id}: '
                         f'a feature row would mix two bias tables (rebuild the cache or load the same tables)')
    first = hash_table.get(1) if hasattr(hash_table, 'get') else None
    device = _compute_device(lk, first.mh_u32 if isinstance(first, HopSketch) else None, cards, ei)
    lkd = lk.to(device=device, dtype=torch.int64).contiguous()
    mh, hll, N, P = eh._resolve_tables(hash_table, device)
    if N >= (1 << 31):
        raise NotImplementedError(f'the masked query does not support {N} nodes')
    _check_row_chunks(P, eh.p)  # (the tables' own width: check_arguments has seen the engine's)
    cd = cards if (cards.device == device and cards.dtype == torch.float32) else cards.to(device=device, dtype=torch.float32)
    if cd.dim() != 2 or cd.size(0) != N or cd.size(1) < h:
        raise ValueError(f'cards must have shape [{N}, >= {h}], got {tuple(cd.shape)}')
    if cd.stride(1) != 1:
        cd = cd.contiguous()
    feats = torch.empty((L, nf), dtype=torch.float32, device=device)
    dbg = None
    if return_debug:
        dbg = {'match': torch.empty((L, h, h), dtype=torch.int32, device=device),
               'zeros': torch.empty((L, h, h), dtype=torch.int32, device=device),
               'row_zeros': torch.empty((L, 2, h), dtype=torch.int32, device=device),
               'masked': torch.empty((L,), dtype=torch.uint8, device=device)}
    if L > 0:
        params = eh._params(device)
        # the CSR the build propagated over: the engine's cache (a repeated edge_index is not rebuilt), implicit self loops as built
        csr = eh._csr_cache.get(ei, N, device)
        graph = _native.CsrGraphStruct(rowptr=csr.rowptr.data_ptr(), col=csr.col.data_ptr(), num_nodes=N, n_self_loops=0,
                                       n_self_loops_dev=csr.n_self_dev.data_ptr())
        ab = eh._perms(device)
        mh_ptrs = (c_void_p * h)(*[t.data_ptr() for t in mh])
        hll_ptrs = (c_void_p * h)(*[t.data_ptr() for t in hll])
        flags = (_native.SS_FLAG_USE_ZERO_ONE if eh.use_zero_one else 0) | (_native.SS_FLAG_FLOOR_SF if eh.floor_sf else 0)
        strict, err = eh._bounds(device, f'get_subgraph_features({L} links, num_nodes={N}, mask_target)')
        if strict:
            err = _error_flag(device)
        lib = _native.lib()
        ws_bytes = int(lib.ss_masked_workspace_bytes(min(batch_size, L)))
        if ws_bytes == 0:
            raise NotImplementedError(f'the masked query takes fewer than 2^31 links per batch, got {min(batch_size, L)}')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        stream = _stream(device)

        def at(t, offset):
            return c_void_p(t.data_ptr() + offset * t.element_size()) if t is not None else c_void_p(0)

        for s0 in range(0, L, batch_size):
            nb = min(batch_size, L - s0)
            with _Span('masked_pair_features', device):
                _native.check(lib.ss_masked_pair_features(
                    byref(graph), at(lkd, 2 * s0), nb, N, h, _ptr(ab[0]), _ptr(ab[1]), mh_ptrs, P, hll_ptrs, _ptr(cd), cd.stride(0),
                    byref(params.struct), flags, at(feats, s0 * nf), at(dbg['match'] if dbg else None, s0 * h * h),
                    at(dbg['zeros'] if dbg else None, s0 * h * h), at(dbg['row_zeros'] if dbg else None, s0 * 2 * h),
                    at(dbg['masked'] if dbg else None, s0), _ptr(err), _ptr(ws), ws_bytes, stream), 'ss_masked_pair_features')
        if strict and _take_error(device):
            raise IndexError(f'links refer to nodes outside [-{N}, {N})')
    if dbg is not None:
        dbg['masked'] = dbg['masked'].to(torch.bool)
    if home != device:
        feats = feats.to(home)
        if dbg is not None:
            dbg = {k: v.to(home) for k, v in dbg.items()}
        if eh.strict_bounds == 'deferred':  # (the copy back has waited for the launches: the report is final)
            eh._deferred.raise_if_set()
    return (feats, dbg) if return_debug else feats
