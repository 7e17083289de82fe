"""Negative links drawn on the device from the graph's sorted CSR: NegativeSampler and the one-shot sample_negatives.
Kernel: csrc/ss_negatives.hip; design: DESIGN 3.15; numpy restatement: tests/negatives_restatement.py.

The reference draws its training negatives once, on the CPU, when the dataset is built: PyG's negative_sampling for any-source
negatives (src/data.py:199-217), get_same_source_negs for ogbl-citation2 (src/utils.py:88-99, not filtered against the graph), and its
sample_hard_negatives (src/data.py:262-304: non-edges with a common neighbour) was never finished.  Here an epoch's negatives are
one launch: O(1) per negative, a pure function of (seed, slot), fresh per seed.

Semantics.  "Edge set" = the directed pairs u -> v of edge_index, read as a set, plus those of `exclude` (validation / test positives
that must not come back as negatives).  Row u of the CSR holds {v : u -> v} sorted ascending WITH its duplicates: a repeated edge is
picked by the wedge walk in proportion to its multiplicity.  Slot q = i * num_neg + j belongs to positive i (j < num_neg); without
positives q is the sample index.  Attempt a = 0, 1, ... < max_tries of slot q draws r0 = draw(seed, q, a, 0), r1 = draw(seed, q, a, 1),
draw(seed, q, a, c) = hash(hash(seed ^ hash(q + 1)) + 0x9E3779B97F4A7C15 * (2 a + c + 1)) with hash the splitmix64 finaliser, and
proposes, with hi(r n) the high 64 bits of r * n:

    'uniform'      u = positives[i, 0], or hi(r0 N) without positives (PyG's any-source setting);  v = hi(r1 N)
    'same_source'  u = positives[i, 0];  v = hi(r1 N)            (the ogbl-citation2 protocol, filtered)
    'wedge'        u = positives[i, 0];  w = row_u[hi(r0 deg u)];  v = row_w[hi(r1 deg w)]

The attempt is accepted when v != u and u -> v is not in the edge set; the first accepted attempt is the slot's (u, v).  If none is,
the slot is (u, -1) and counted as unsampled (any-source: the u of the last attempt; a wedge source without neighbours makes no
attempt; a wedge attempt whose w has no out-neighbour -- directed graphs only -- is rejected).  The wedge walk proposes v with
probability sum_w mult(u, w) mult(w, v) / (deg u deg w): proportional to the resource-allocation score of (u, v), so the accepted
negatives are hard negatives weighted by RA among the non-neighbours of u.

Guaranteed: a slot depends on (seed, q) and the graph only -- not on the number of positives, on batch_size or on the other slots.
NOT guaranteed: distinct negatives.  Two slots may return the same pair (rarely for the uniform modes, routinely for wedge sources
with few candidates).
"""
from ctypes import c_void_p

import torch

from . import _native
from ._runtime import _DeferredErrors, _Span, _compute_device, _error_flag, _ptr, _stream, _take_error
from .candidates import _int
from .engine import _exclude_csr

_LAUNCH_SLOTS = 1 << 30  # slots per launch when batch_size is not given (rows do not depend on it; not a user knob)


def _edge_index(ei, name, N):
    """an integer [2, E] edge_index, its CPU ids checked at once (device ids: by the CSR build)"""
    ei = torch.as_tensor(ei)
    if ei.dim() != 2 or ei.size(0) != 2 or ei.dtype.is_floating_point or ei.dtype == torch.bool:
        raise ValueError(f'{name} must be an integer [2, E] edge_index, got {ei.dtype} {tuple(ei.shape)}')
    if ei.size(1) >= (1 << 31):
        raise ValueError(f'{name} holds {ei.size(1)} edges: the row sort takes fewer than 2^31')
    if not ei.is_cuda and ei.numel() and (int(ei.min()) < -N or int(ei.max()) >= N):
        raise IndexError(f'{name} refers to nodes outside [-{N}, {N})')
    return ei


def _graph_arguments(num_nodes, edge_index, exclude):
    """what NegativeSampler checks before a device is touched: (N, edge_index, exclude or None)"""
    N = _int(num_nodes, 'num_nodes', 1)
    if N >= (1 << 31):
        raise ValueError(f'negative sampling needs num_nodes < 2^31 (node ids are int32 in the CSR), got {N}')
    return N, _edge_index(edge_index, 'edge_index', N), None if exclude is None else _edge_index(exclude, 'exclude', N)


def _sorted_rows(ei, N, device):
    """CSR with row u = {v : u -> v} of an edge_index (negative ids wrapped), every row sorted ascending, duplicates kept"""
    csr, _ = _exclude_csr(ei, N, device, True, None)
    lib = _native.lib()
    E = csr.num_edges
    ws_bytes = lib.ss_csr_sort_workspace_bytes(E)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    with _Span('negatives_sort_rows', device):
        _native.check(lib.ss_csr_sort_rows(_ptr(csr.rowptr), _ptr(csr.col), N, E, None, _ptr(ws), ws_bytes, _stream(device)), 'ss_csr_sort_rows')
    return csr


def _sample_arguments(N, positives, num_neg, mode, seed, max_tries, num_samples, batch_size):
    """what .sample checks before a device is touched: (positives or None, n_slots, num_neg, max_tries, seed, batch_size)"""
    if mode not in _native.NEG_MODES:
        raise ValueError(f'mode must be one of {sorted(_native.NEG_MODES)}, got {mode!r}')
    num_neg = _int(num_neg, 'num_neg', 1, (1 << 31) - 1)
    max_tries = _int(max_tries, 'max_tries', 1, _native.NEG_MAX_TRIES)
    seed = _int(seed, 'seed', 0, (1 << 64) - 1)
    batch_size = None if batch_size is None else _int(batch_size, 'batch_size', 1)
    if positives is None:
        if mode != 'uniform':
            raise ValueError(f"mode {mode!r} draws around the sources of positives: give positives (only 'uniform' samples any source)")
        if num_samples is None:
            raise ValueError('give positives or num_samples')
        return None, _int(num_samples, 'num_samples', 0), num_neg, max_tries, seed, batch_size
    if num_samples is not None:
        raise ValueError('num_samples is for any-source sampling: with positives the result has len(positives) * num_neg slots')
    pos = torch.as_tensor(positives)
    if pos.dim() != 2 or pos.size(1) != 2 or pos.dtype.is_floating_point or pos.dtype == torch.bool:
        raise ValueError(f'positives must be an integer [L, 2] tensor, got {pos.dtype} {tuple(pos.shape)}')
    # CPU ids are checked here, as the link queries check them; device ids are reported late (strict_bounds)
    if not pos.is_cuda and pos.numel() and (int(pos[:, 0].min()) < -N or int(pos[:, 0].max()) >= N):
        raise IndexError(f'positives refer to source nodes outside [-{N}, {N})')
    return pos, pos.size(0) * num_neg, num_neg, max_tries, seed, batch_size


class NegativeSampler(object):
    """the sorted CSR of a graph (and of an optional exclude list), built once and resident on the device; .sample draws from it.

    @param num_nodes: N, 1 <= N < 2^31
    @param edge_index: int [2, E] (torch-style negative ids allowed); ids outside [-N, N) raise IndexError here
    @param exclude: optional int [2, X] edge_index whose directed pairs are no negatives either
    @param device: the HIP device (default: edge_index's, else the current one)
    `strict_bounds` says how ids outside [-N, N) in DEVICE positives are reported, as ElphHashes.strict_bounds does: 'deferred'
    (default) = IndexError at the next .sample, at check_errors() or when a result is copied to a CPU caller; True = from the
    offending call (one synchronising read); False = never.  Such a slot is (the id as given, -1) and counts as unsampled."""

    def __init__(self, num_nodes, edge_index, exclude=None, device=None):
        N, ei, ex = _graph_arguments(num_nodes, edge_index, exclude)
        self.num_nodes = N
        self.device = torch.device(device) if device is not None else _compute_device(ei, ex)
        self.strict_bounds = 'deferred'
        self._deferred = _DeferredErrors()
        self.graph = _sorted_rows(ei, N, self.device)
        self.exclude = None if ex is None else _sorted_rows(ex, N, self.device)

    def check_errors(self):
        """strict_bounds = 'deferred': wait for the launches issued so far and raise IndexError if one met a source outside [-N, N)"""
        self._deferred.raise_if_set(synchronize=True)

    def sample(self, positives=None, num_neg=1, mode='wedge', seed=0, max_tries=16, num_samples=None, batch_size=None, return_info=False):
        """negatives for `positives` (int [L, 2]; only the first column, the source, is read; torch-style negative ids allowed),
        num_neg per positive, or num_samples any-source ones (mode 'uniform', positives=None): see the module text for the modes.
        @param seed: 0 <= seed < 2^64; one seed, one result -- change it per epoch
        @param max_tries: attempts per slot, in [1, 64]
        @param batch_size: slots per launch; only splits the call, never changes the result
        @return: int64 [n_slots, 2] rows (u, v) on positives' device (any-source: the sampler's), slot i * num_neg + j for
                 positive i; v == -1: no attempt was accepted.  With return_info also {'unsampled': number of such slots} (one
                 synchronising read).  Slots may repeat each other.  No CPU fallback."""
        N, device = self.num_nodes, self.device
        pos, n_slots, num_neg, max_tries, seed, batch_size = _sample_arguments(N, positives, num_neg, mode, seed, max_tries, num_samples, batch_size)
        home = device if pos is None else pos.device
        strict, err = False, None
        if pos is not None:
            if self.strict_bounds == 'deferred':
                self._deferred.raise_if_set()
                err = self._deferred.flag(device, f'sample({pos.size(0)} positives, num_nodes={N})')
            elif self.strict_bounds:
                strict, err = True, _error_flag(device)
            pos = pos.to(device=device, dtype=torch.int64)
            if pos.stride(0) < 1:  # (an expanded view)
                pos = pos.contiguous()
        out = torch.empty((n_slots, 2), dtype=torch.int64, device=device)
        unsampled = torch.zeros((1,), dtype=torch.int32, device=device)
        lib = _native.lib()
        g, x = self.graph, self.exclude
        step = batch_size or _LAUNCH_SLOTS
        for q0 in range(0, n_slots, step):
            n = min(step, n_slots - q0)
            src, stride = None, 0
            if pos is not None:  # the source of the positive of slot q0
                src, stride = c_void_p(pos.data_ptr() + 8 * pos.stride(0) * (q0 // num_neg)), pos.stride(0)
            with _Span('sample_negatives', device):
                _native.check(lib.ss_sample_negatives(_ptr(g.rowptr), _ptr(g.col), _ptr(x.rowptr) if x is not None else None, _ptr(x.col) if x is not None else None,
                                                      N, src, stride, n, num_neg, _native.NEG_MODES[mode], seed, max_tries, q0,
                                                      c_void_p(out.data_ptr() + 16 * q0), _ptr(unsampled), _ptr(err), _stream(device)),
                              'ss_sample_negatives')
        if strict and n_slots and _take_error(device):
            raise IndexError(f'positives refer to source nodes outside [-{N}, {N})')
        if home != device:
            out = out.to(home)
            if self.strict_bounds == 'deferred':  # a copy has waited for the launches: a deferred report is final behind it
                self._deferred.raise_if_set()
        return (out, {'unsampled': int(unsampled.item())}) if return_info else out


def sample_negatives(num_nodes, edge_index, positives=None, exclude=None, device=None, num_neg=1, mode='wedge', seed=0, max_tries=16,
                     num_samples=None, batch_size=None, return_info=False):
    """NegativeSampler(num_nodes, edge_index, exclude, device).sample(positives, ...) in one call: the CSR is built, sorted and
    dropped again, so keep a NegativeSampler when there is more than one epoch.  Every argument is checked before a device is touched.
    Ids outside [-N, N) in device positives raise IndexError from this call (there is no object to report them later)."""
    N, ei, ex = _graph_arguments(num_nodes, edge_index, exclude)
    _sample_arguments(N, positives, num_neg, mode, seed, max_tries, num_samples, batch_size)
    sampler = NegativeSampler(N, ei, exclude=ex, device=device)
    sampler.strict_bounds = True
    return sampler.sample(positives, num_neg=num_neg, mode=mode, seed=seed, max_tries=max_tries, num_samples=num_samples,
                          batch_size=batch_size, return_info=return_info)
