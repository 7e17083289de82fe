"""An independent restatement of one sketch hop for tables larger than 2^31 bytes, and the graph the large-table tests build.

Hop k of a table is computed from hop k - 1 in stock torch operators, in the reference's own dataflow (hashing.py:28-45: `x[src]`
per edge, reduced by destination) over the self-looped edge list.  The edges are sorted by destination once, so a block of
destination rows is a slice of them; a block is sized so that every tensor a torch operator sees in it stays below 2^31 elements --
the check does not lean on torch's own large-index paths.  The source rows are taken from the FULL hop k - 1 table with int64
indices (`index_select`): that is the one place an offset beyond 2^31 / 2^32 bytes is formed, and it is formed by torch, not by the
code under test.

Works on CPU and device tensors alike; tests/test_large_table_restatement_host.py pins it on the C oracle bit for bit, which is
what makes it a reference.  Sketch layouts are the engine's packed ones: MinHash int32 [N, P] holding the unsigned 32-bit values,
HLL uint8 [N, m]."""
import numpy as np
import torch

_U32 = 0xFFFFFFFF
_SENTINEL = 1 << 40  # above every unsigned 32-bit MinHash value


def self_looped_edges(edge_index):
    """the reference's add_self_loops WITHOUT num_nodes (hashing.py:148): a loop at every id below max(edge_index) + 1"""
    n_self = int(edge_index.max()) + 1 if edge_index.numel() else 0
    loops = torch.arange(n_self, dtype=torch.int64, device=edge_index.device)
    return torch.cat([edge_index[0].to(torch.int64), loops]), torch.cat([edge_index[1].to(torch.int64), loops])


class EdgeBlocks(object):
    """the self-looped edges of a graph sorted by destination and cut into blocks of whole destination rows:
    at most `max_edges` edges (a longer single row is a block of its own) and `max_rows` rows per block"""

    def __init__(self, edge_index, num_nodes, max_edges=1 << 20, max_rows=1 << 20):
        src, dst = self_looped_edges(edge_index)
        assert src.numel() < (1 << 31) and num_nodes < (1 << 31)
        dst, perm = torch.sort(dst, stable=True)
        self.src, self.dst = src[perm], dst
        del perm
        self.num_nodes = int(num_nodes)
        self.degree = torch.bincount(dst, minlength=num_nodes)            # in-degree over the self-looped list
        rowptr = np.zeros(num_nodes + 1, dtype=np.int64)
        np.cumsum(self.degree.cpu().numpy(), out=rowptr[1:])
        self.rowptr = rowptr
        self.blocks = []
        r0 = 0
        while r0 < num_nodes:
            r1 = int(np.searchsorted(rowptr, rowptr[r0] + max_edges, side='right')) - 1
            r1 = max(r0 + 1, min(r1, r0 + max_rows, num_nodes))
            self.blocks.append((r0, r1, int(rowptr[r0]), int(rowptr[r1])))
            r0 = r1

    def __iter__(self):
        return iter(self.blocks)


def _u64(x):
    """int32 holding unsigned 32-bit values -> int64 of those values"""
    return x.to(torch.int64) & _U32


def restate_block(blocks, block, prev_mh=None, prev_hll=None):
    """rows [r0, r1) of the next hop -> (MinHash int64 [r1 - r0, P] of the unsigned values or None, HLL uint8 [r1 - r0, m] or None)"""
    r0, r1, e0, e1 = block
    nr, ne = r1 - r0, e1 - e0
    src = blocks.src[e0:e1]
    local = blocks.dst[e0:e1] - r0
    empty = blocks.degree[r0:r1] == 0         # no in-edge, no loop: the reference's scatter leaves such a row zero
    mh = hll = None
    if prev_mh is not None:
        P = prev_mh.size(1)
        assert ne * P < (1 << 31) and nr * P < (1 << 31), 'block too large for the 2^31-element rule'
        mh = torch.full((nr, P), _SENTINEL, dtype=torch.int64, device=prev_mh.device)
        if ne:
            mh.scatter_reduce_(0, local[:, None].expand(-1, P), _u64(prev_mh.index_select(0, src)), 'amin', include_self=True)
        mh[empty] = 0
    if prev_hll is not None:
        m = prev_hll.size(1)
        assert ne * m < (1 << 31) and nr * m < (1 << 31), 'block too large for the 2^31-element rule'
        # registers are ranks <= 64 - p + 1 < 128: the int8 view orders them as the bytes do (and is the dtype the reference uses)
        acc = torch.zeros((nr, m), dtype=torch.int8, device=prev_hll.device)
        if ne:
            acc.scatter_reduce_(0, local[:, None].expand(-1, m), prev_hll.index_select(0, src).view(torch.int8), 'amax', include_self=True)
        hll = acc.view(torch.uint8)
    return mh, hll


def hop_mismatches(blocks, prev_mh, prev_hll, got_mh, got_hll):
    """every row of `got_*` (hop k) against the restatement from `prev_*` (hop k - 1).
    -> (sorted int64 numpy array of differing MinHash rows, the same for HLL)"""
    n = blocks.num_nodes
    assert got_mh.shape == prev_mh.shape and got_mh.size(0) == n and got_hll.shape == prev_hll.shape and got_hll.size(0) == n
    assert int(prev_hll.max()) < 128
    bad_mh, bad_hll = [], []
    for block in blocks:
        r0, r1 = block[:2]
        mh, hll = restate_block(blocks, block, prev_mh, prev_hll)
        got = _u64(got_mh[r0:r1])
        if not torch.equal(mh, got):
            bad_mh.append((mh != got).any(dim=1).nonzero().flatten().cpu().numpy() + r0)
        if not torch.equal(hll, got_hll[r0:r1]):
            bad_hll.append((hll != got_hll[r0:r1]).any(dim=1).nonzero().flatten().cpu().numpy() + r0)
        del mh, hll, got
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
    return cat(bad_mh), cat(bad_hll)


def windows(num_nodes, boundaries, width=4096):
    """`width`-row windows [lo, hi) around row 0, every boundary row and the end of the table (clipped, in order, distinct)"""
    half = width // 2
    out = [(0, min(width, num_nodes))]
    for b in boundaries:
        out.append((max(b - half, 0), min(b + half, num_nodes)))
    out.append((max(num_nodes - width, 0), num_nodes))
    return sorted(set(out))


def hop0_mismatches(oracle, mh0, hll0, num_nodes, boundaries, p, width=4096):
    """hop-0 rows against oracle.minhash_init / oracle.hll_init(first_node=...) on the windows -> list of differing row ids"""
    bad = []
    for lo, hi in windows(num_nodes, boundaries, width):
        want_mh = oracle.minhash_init(hi - lo, mh0.size(1), first_node=lo)
        want_hll = oracle.hll_init(hi - lo, p, first_node=lo)
        got_mh = mh0[lo:hi].cpu().numpy().view(np.uint32)
        got_hll = hll0[lo:hi].cpu().numpy()
        rows = np.nonzero((got_mh != want_mh).any(axis=1) | (got_hll != want_hll).any(axis=1))[0]
        bad.extend(int(r) + lo for r in rows)
    return bad


def describe_row(row, boundaries):
    """'row r: above 2^23 (+5)'-style text: where a differing row lies relative to the boundary rows"""
    row = int(row)
    below = [b for b in boundaries if row < b]
    if below:
        b = min(below)
        side = f'below row {b} = 2^{b.bit_length() - 1} ({row - b})'
    else:
        b = max(boundaries)
        side = f'at or above row {b} = 2^{b.bit_length() - 1} (+{row - b})'
    return f'row {row}: {side}'


def report(bad_rows, boundaries, what):
    """assertion text for a list of differing rows: how many, the first, and which side of which boundary it is on"""
    bad_rows = np.asarray(bad_rows)
    if not len(bad_rows):
        return ''
    return f'{what}: {len(bad_rows)} rows differ, first {describe_row(bad_rows.min(), boundaries)}, last {describe_row(bad_rows.max(), boundaries)}'


# ---------------------------------------------------------------------------------------------------
# the graph
# ---------------------------------------------------------------------------------------------------
class BoundaryGraph(object):
    """edge_index int64 [2, E] (both directions of every undirected edge), hub ids, the mega hub"""


def boundary_graph(num_nodes, boundaries, device, seed, window=1 << 12, window_degree=20, hub_degree=1500, mega_degree=6000,
                   n_hubs=3, background=1.0, tail=8):
    """A seeded graph, generated on `device`, whose boundary rows carry real work:
      * background: `background * num_nodes` uniform undirected edges (about 2 per node at 1.0) among the nodes below num_nodes - tail;
      * a dense window: every node of [b - window, b + window) for each boundary row b draws window_degree neighbours, half from
        [b - window, b) and half from [b, b + window), so rows on both sides gather rows from both sides;
      * hubs ABOVE the highest boundary (ids top + window + 64 + 37 i): n_hubs of in-degree hub_degree and one of mega_degree, their
        neighbours drawn from [top, num_nodes - tail);
      * the last `tail` nodes: num_nodes - tail .. num_nodes - 2 have no edge at all, num_nodes - 1 is a neighbour of the mega hub.
    background = 0 leaves only the windows (no hubs, no tail edge): every other node is isolated."""
    gen = torch.Generator(device=device).manual_seed(seed)
    top = max(boundaries)
    usable = num_nodes - tail
    assert min(boundaries) - window >= 0 and top + window + 64 + 37 * (n_hubs + 1) < usable
    parts = []

    def rand(lo, hi, count):
        return torch.randint(lo, hi, (count,), device=device, generator=gen, dtype=torch.int64)

    g = BoundaryGraph()
    g.num_nodes, g.boundaries, g.window = num_nodes, list(boundaries), window
    g.hubs, g.mega = [], None
    if background:
        e = int(background * num_nodes)
        parts.append(torch.stack([rand(0, usable, e), rand(0, usable, e)]))
    half = window_degree // 2
    for b in boundaries:
        v = torch.arange(b - window, b + window, device=device, dtype=torch.int64)
        parts.append(torch.stack([v.repeat_interleave(half), rand(b - window, b, half * v.numel())]))
        parts.append(torch.stack([v.repeat_interleave(half), rand(b, b + window, half * v.numel())]))
    if background:
        for i in range(n_hubs + 1):
            hub = top + window + 64 + 37 * i
            deg = mega_degree if i == n_hubs else hub_degree
            nb = rand(top, usable, deg)
            if i == n_hubs:
                nb[0] = num_nodes - 1
                g.mega = hub
            else:
                g.hubs.append(hub)
            parts.append(torch.stack([torch.full_like(nb, hub), nb]))
    und = torch.cat(parts, dim=1)
    g.edge_index = torch.cat([und, und.flip(0)], dim=1)
    return g
