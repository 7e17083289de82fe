"""Per-hop sampled subgraph node lists (ElphHashes.sampled_subgraph_nodes, csrc/ss_sampled_nodes.hip): per link (u, v) the node row of
the reference's k_hop_subgraph with its sample_ratio / max_nodes_per_hop (src/datasets/seal.py:291-348), deterministic in a seed -- one
joint walk from {u, v} that keeps a uniform sample of every hop's fringe and expands only what it kept.  Design: DESIGN 3.19; Python-set
restatement: tests/sampled_subgraph_restatement.py.

Host side only: the sampling arguments' checks and the two tier launches of one batch; the rest -- the other checks, the graph struct,
the slot arena and the walk over the batches (a count pass, ONE host read of the total for the allocation, a fill pass) -- is
exact.py's and exact_nodes.py's, shared with exact_subgraph_nodes."""
import numbers
from ctypes import byref

import torch

from . import _native, exact, exact_nodes, knobs
from ._runtime import _compute_device, _ptr, _stream, _Span


def sampling_arguments(max_nodes_per_hop, ratio_per_hop, seed):
    """-> (cap for the C ABI: 0 = none, ratio as float, seed as int) after the checks"""
    if max_nodes_per_hop is not None:
        if isinstance(max_nodes_per_hop, bool) or not isinstance(max_nodes_per_hop, numbers.Integral) or max_nodes_per_hop < 1:
            raise ValueError(f'max_nodes_per_hop must be None or an integer >= 1, got {max_nodes_per_hop!r}')
        if max_nodes_per_hop >= (1 << 31):
            max_nodes_per_hop = (1 << 31) - 1  # (no fringe holds 2^31 nodes: the same as no cap)
    if isinstance(ratio_per_hop, bool) or not isinstance(ratio_per_hop, numbers.Real) or not 0.0 < float(ratio_per_hop) <= 1.0:
        raise ValueError(f'ratio_per_hop must be a real number in (0, 1], got {ratio_per_hop!r}')
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < (1 << 63):
        raise ValueError(f'seed must be an integer in [0, 2^63), got {seed!r}')
    return int(max_nodes_per_hop or 0), float(ratio_per_hop), int(seed)


def sampled_subgraph_nodes(eh, links, num_nodes, edge_index, batch_size=11000000, max_nodes_per_hop=None, ratio_per_hop=1.0, seed=0,
                           max_nodes=None, return_info=False, stats=None):
    """see ElphHashes.sampled_subgraph_nodes.  stats (measurement hook, tools/probe_sampled_subgraphs.py): a dict that receives the
    milliseconds of the count pass, of the row pointer with its host read and allocation, and of the fill pass (the call then synchronises)"""
    h = eh.max_hops
    cap_hop, ratio, seed = sampling_arguments(max_nodes_per_hop, ratio_per_hop, seed)
    cap = exact_nodes._cap(max_nodes)
    lk, ei, N, batch_size = exact.check_arguments(h, links, num_nodes, edge_index, batch_size)
    home, L = lk.device, lk.size(0)
    if L == 0:
        return exact.empty_rows(home, (), return_info, sampled_links=0)
    device = _compute_device(lk, ei)
    graph, csr = exact.csr_graph(eh, ei, N, device)
    lk = lk.to(device=device, dtype=torch.int64).contiguous()
    lib = _native.lib()
    state = torch.empty((L,), dtype=torch.int32, device=device)
    slots, arena = exact._arena(device, N)
    stream = _stream(device)
    lds_nodes = max(0, int(knobs.EXACT_LDS_MAX_NODES))

    def launch(s0, nb, counts, rowptr, ids, hop, space):
        args = (byref(graph), exact._at(lk, 2 * s0), nb, N, h, cap_hop, ratio, seed)
        outs = (exact._at(counts, s0), exact._at(state, s0), exact._at(rowptr, s0), _ptr(ids), _ptr(hop))
        with _Span('sampled_nodes_pairs', device):
            _native.check(lib.ss_sampled_nodes_pairs(*args, lds_nodes, *outs, None, *space, stream), 'ss_sampled_nodes_pairs')
        with _Span('sampled_nodes_large', device):
            _native.check(lib.ss_sampled_nodes_large(*args, *outs, *space, slots, _ptr(arena), arena.numel(), stream),
                          'ss_sampled_nodes_large')

    rowptr, ids, hop, counts, _, _ = exact_nodes._two_pass_rows(device, L, batch_size, cap, stats, (), launch)
    if stats is not None:
        stats['slots'] = slots
    out = (rowptr, ids, hop)
    if return_info:
        large, sampled = torch.stack([((state >> 1) & 1).sum(), (state & 1).sum()]).tolist()
        out += (exact_nodes._info(counts, cap, large, sampled_links=sampled),)
    return exact_nodes._home(out, home)
