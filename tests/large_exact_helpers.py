"""What tests/test_large_exact_host.py and tests/test_large_exact_gpu.py share: the shapes at which the exact kernels' two large objects
pass 2^31, the generated graphs and links, and the expected results.  No test lives here.

Part A, the slot arena (exact._arena; csrc/ss_exact_bfs.hpp exact_slot): persistent workgroup b of ss_exact_large, ss_exact_nodes_large
and ss_sampled_nodes_large owns the uint32 words [b * slot_words(N), (b + 1) * slot_words(N)).  At N = 2^22 + 2^18 a slot holds
10 027 008 words, so with 256 slots the slots from 215 on start beyond word 2^31 and those from 108 on beyond byte 2^32.  The expected
result of a slot-tier call is the on-chip tier's answer to the same links (no arena at all) and, for the first links, the host
restatements on the part of the graph those links can reach.

Part B, the arc outputs (csrc/ss_subgraph.hip): a batch of 520 links inside a 2 048-clique lists the same 2 048 nodes per link and
2 048 * 2 047 arcs per row (two fewer where the target link is masked), 2.18e9 arcs in all: adj_ptr, nbr and weight pass index 2^31
inside row 512.  Everything expected there has a closed form (clique_*), which tests/test_large_exact_host.py pins against
subgraph_restatement on a 32-clique."""
import collections

import numpy as np
import torch

import exact_nodes_restatement as nr
import exact_restatement as er
import masked_restatement as mr
import sampled_subgraph_restatement as ssr
from large_table_helpers import wrap

# ---- Part A: shapes -----------------------------------------------------------------------------------------------------------------
ARENA_N = (1 << 22) + (1 << 18)  # 4 456 448: the N of fixture S3 of the table tests
ARENA_SLOTS = 256                # knobs.EXACT_LARGE_SLOTS during the tests: one persistent workgroup per CU of an MI355X
ARENA_LINKS = 4096               # 16 per slot
ARENA_HOST_LINKS = 256           # the first links, restated on the host
ARENA_H = 2
ARENA_TOP = 1 << 18              # "high" ids: the last 2^18
BIG_DEGREE = 512                 # kBigDegree of csrc/ss_exact_bfs.hpp: a frontier node with more in-arcs is walked by the whole workgroup
STAR_LEAVES = 300
SAMPLED = dict(max_nodes_per_hop=5, ratio_per_hop=0.5, seed=20240607)
# free device memory the arena tests ask for.  exact._arena gives the arena at most a QUARTER of what is free when it is made, so 256
# slots need four arenas free at that moment; the rest (graph, CSR, links, outputs, the comparison's transients) is the measured peak
# of the module's arena tests without the arena + 10 % (profiles/large_exact_tests.txt)
ARENA_PEAK = 11053445632
# the arc tests: the measured peak + 10 % (nbr + weight of the call, 17.4 GB, a second pair for the id-row walk, the chunk checks)
ARCS_PEAK = 35359683584


def dist_words(n):
    """exact_dist_words: uint32 words of a slot's distance bytes"""
    return (n + 3) // 4


def slot_words(n):
    """exact_slot_words: the distance words and two int32 visit lists of N, rounded up to 16 bytes"""
    return (dist_words(n) + 2 * n + 3) & ~3


def first_slot_at_or_beyond(n, word):
    """the first slot whose base is at or beyond uint32 word index `word` of the arena"""
    return -(-word // slot_words(n))


def arena_needs(n=ARENA_N, slots=ARENA_SLOTS):
    arena = 4 * slot_words(n) * slots
    return 4 * arena + int(1.1 * (ARENA_PEAK - arena))


# ---- Part A: graph and links ---------------------------------------------------------------------------------------------------------
class ArenaGraph(object):
    """n, ei int64 [2, E] (symmetric), hub, leaves int64 [STAR_LEAVES]"""


def arena_graph(dev, n=ARENA_N, seed=97):
    """2 n uniform undirected edges (self loops and duplicates as they fall) and one star: hub n - 7 with 300 leaves spread over the id
    range, every star edge listed TWICE -- the hub then holds 600 in-arcs, above kBigDegree, while its ball keeps to 300 leaves and
    what they reach, so a star link's union fits the on-chip tier too"""
    g = ArenaGraph()
    gen = torch.Generator(device=dev).manual_seed(seed)
    e = torch.randint(0, n, (2, 2 * n), device=dev, generator=gen)
    g.n, g.hub = n, n - 7
    g.leaves = torch.arange(STAR_LEAVES, device=dev) * ((n - 16) // STAR_LEAVES) + 11
    star = torch.stack([torch.full_like(g.leaves, g.hub), g.leaves]).repeat(1, 2)
    und = torch.cat([e, star], 1)
    g.ei = torch.cat([und, und.flip(0)], 1).contiguous()
    return g


def arena_links(g, count=ARENA_LINKS, seed=98):
    """int64 [count, 2]: every other link an edge of the graph (the balls meet and mask_target removes something), the rest uniform
    pairs; every eighth link with an endpoint among the last 2^18 ids; a star link every 128 (hub - leaf, leaf - hub, leaf - leaf,
    leaf - anything, each with its own leaves) and the fixed corner links from row 4 on, all inside the first 256; u == v every 512;
    a third of the ids negative (torch style: id - n), alone or both"""
    dev, n = g.ei.device, g.n
    top = min(ARENA_TOP, n // 4)
    gen = torch.Generator(device=dev).manual_seed(seed)
    links = torch.randint(0, n, (count, 2), device=dev, generator=gen)
    pick = torch.randint(0, g.ei.size(1), (count,), device=dev, generator=gen)
    high = torch.randint(n - top, n, (count, 2), device=dev, generator=gen)
    links[0::2] = g.ei[:, pick[0::2]].t()
    links[3::8, 0] = high[3::8, 0]
    links[6::16] = high[6::16]
    lv, hub = g.leaves, torch.tensor(g.hub, device=dev)
    for k, at in enumerate(range(64, count, 128)):
        a, b = lv[(7 * k) % STAR_LEAVES], lv[(7 * k + 150) % STAR_LEAVES]
        links[at] = torch.stack([(hub, a), (a, hub), (a, b), (a, links[at, 1])][k % 4])
    corner = torch.tensor([[g.hub, int(lv[0])], [int(lv[-1]), g.hub], [int(lv[1]), int(lv[-2])], [g.hub, g.hub], [int(lv[3]), int(lv[3])],
                           [n - 1, n - 1], [n - 1, 0], [0, n - 2], [n - top, n - top - 1], [g.hub, n - 1]], device=dev)
    links[4:4 + len(corner)] = corner
    links[7::512, 1] = links[7::512, 0]
    row = torch.arange(count, device=dev)
    neg = torch.stack([(row % 5 == 0) | (row % 7 == 3), (row % 5 == 0) | (row % 11 == 2)], 1)
    return torch.where(neg, links - n, links).contiguous()


class Neighbourhood(object):
    """the part of an ArenaGraph within `hops` of some links, on the host: nodes int64 [m] ascending (original ids), arcs int64 [2, e]
    (original ids), and the same graph renumbered by rank in `nodes`: small_n, small_arcs, small_links.  small_loops lists a self loop
    at every kept node below the full graph's n_self = max(edge_index) + 1, the kept node that attains the maximum among them, so
    exact_restatement gives the small graph the self loops the full one has"""


def neighbourhood(g, links, hops=ARENA_H):
    dev, n = g.ei.device, g.n
    lk = wrap(links.to(torch.int64), n)
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    keep[lk.flatten()] = True
    for _ in range(hops):  # B_k(x) = the sources of the arcs into B_{k-1}(x)
        keep[g.ei[0][keep[g.ei[1]]]] = True
    top = int(g.ei.max())
    keep[top] = True
    nb = Neighbourhood()
    nb.n, nb.links = n, lk.cpu().numpy()
    nb.nodes = torch.nonzero(keep).flatten().cpu().numpy()
    nb.arcs = g.ei[:, keep[g.ei[0]] & keep[g.ei[1]]].cpu().numpy()
    nb.small_n = nb.nodes.size
    nb.small_arcs = np.searchsorted(nb.nodes, nb.arcs)
    nb.small_links = np.searchsorted(nb.nodes, nb.links)
    loops = np.nonzero(nb.nodes <= top)[0]
    nb.small_loops = np.stack([loops, loops])
    return nb


def restate_features(nb, h, mask):
    """(features, I, balls) of nb.links by exact_restatement; mask: every link that is an edge is restated on the graph without it,
    as tests/test_masked_gpu.py does (self loops listed, so n_self stays where the full graph has it)"""
    e = np.concatenate([nb.small_arcs, nb.small_loops], axis=1)
    f, I, balls = er.restate(nb.small_n, e, nb.small_links, h)
    if mask:
        for q, (u, v) in enumerate(nb.small_links.tolist()):
            e2 = mr.without_link(e, u, v)
            if e2.shape[1] != e.shape[1]:
                f[q], I[q], balls[q] = [x[0] for x in er.restate(nb.small_n, e2, np.array([[u, v]]), h)]
    return f, I, balls


def restate_nodes(nb, h, mask):
    """(rowptr, ids, dist) of nb.links by exact_nodes_restatement, ids back in the full graph's numbering"""
    rowptr, ids, dist = nr.restate(nb.small_n, nb.small_arcs, nb.small_links, h, mask_target=mask, directed=True)
    return rowptr, nb.nodes[ids], dist


def restate_sampled(nb, h):
    """(rowptr, ids, hop) of nb.links by sampled_subgraph_restatement.restate_nodes: the sampling keys hash the node ids, so this one
    walks the ORIGINAL ids, over a sparse in-neighbour table in place of a list of N sets"""
    table = collections.defaultdict(set)
    for j, x in zip(nb.arcs[0].tolist(), nb.arcs[1].tolist()):
        table[x].add(j)
    return ssr.restate_nodes(nb.n, nb.arcs, nb.links, h, cap=SAMPLED['max_nodes_per_hop'], ratio=SAMPLED['ratio_per_hop'],
                             seed=SAMPLED['seed'], nb=table)


def arena_dist_words_are_zero(ssa, dev):
    """every distance word of every slot of the current stream's arena is zero, read as int64: what the next call's walk relies on.
    (The two int32 visit lists behind a slot's distance words are scratch, written before they are read and never cleared: they are
    not part of the contract -- tests/test_exact_nodes_gpu.py::_arena_is_zero.)"""
    torch.cuda.synchronize(dev)
    n, slots, arena, _ = ssa.exact._ARENA[(str(dev), torch.cuda.current_stream(dev).cuda_stream)]
    words, dw = slot_words(n), dist_words(n)
    assert arena.numel() == 4 * words * slots
    if bool(arena.view(torch.int64).view(slots, words // 2)[:, :dw // 2].any()):
        return False
    return dw % 2 == 0 or not bool(arena.view(torch.int32).view(slots, words)[:, dw - 1].any())


# ---- Part B: the clique and its closed forms ---------------------------------------------------------------------------------------------
CLIQUE_N, CLIQUE_LO, CLIQUE_HI = 4096, 1024, 3072
CLIQUE_LINKS = 520
CLIQUE_SELF = (7, 516)  # the rows of the two u == v links (one on either side of the row in which 2^31 falls)
CHUNK_ROWS = 16


def arcs_needs():
    return int(1.1 * ARCS_PEAK)


def clique_graph(dev, n=CLIQUE_N, lo=CLIQUE_LO, hi=CLIQUE_HI):
    """(n, edge_index int64 [2, E]): both directions of every edge of the clique on lo .. hi - 1, the undirected pairs with
    (a + b) % 7 == 0 listed twice; every other node isolated"""
    ids = torch.arange(lo, hi, device=dev)
    a, b = ids[:, None].expand(-1, hi - lo), ids[None, :].expand(hi - lo, -1)
    und = torch.stack([a[a < b], b[a < b]])
    und = torch.cat([und, und[:, (und[0] + und[1]) % 7 == 0]], 1)
    return n, torch.cat([und, und.flip(0)], 1).contiguous()


def clique_links(dev, count=CLIQUE_LINKS, n=CLIQUE_N, lo=CLIQUE_LO, hi=CLIQUE_HI, self_rows=CLIQUE_SELF):
    """int64 [count, 2] inside the clique: count - 2 distinct pairs with u != v (distinct u: 3 k < hi - lo), every fourth in (v, u) order,
    ids negative (id - n) in a pattern of their own, and u == v at `self_rows`"""
    k_nodes = hi - lo
    assert 3 * (count - len(self_rows) - 1) < k_nodes
    k = torch.arange(count - len(self_rows), device=dev)
    u = lo + (3 * k) % k_nodes
    v = lo + (3 * k + 1 + (k % 5) * (k_nodes // 21)) % k_nodes
    pairs = torch.stack([torch.where(k % 4 == 1, v, u), torch.where(k % 4 == 1, u, v)], 1)
    neg = torch.stack([k % 3 == 0, k % 6 == 1], 1)
    pairs = torch.where(neg, pairs - n, pairs)
    rows = pairs.tolist()
    for i, at in enumerate(sorted(self_rows)):
        x = lo + (5 + 11 * i) % k_nodes
        rows.insert(at, [x, x - n if i else x])
    return torch.tensor(rows, dtype=torch.int64, device=dev)


class CliqueExpected(object):
    """rowptr, ids, dist, roots, adj_ptr, z as exact_subgraphs(h = 1, mask_target=True, node_label='drnl') must return them for links
    inside the clique (torch, on the links' device); lengths int64 [L, K] the adjacency row lengths; A their sum; row_start (a Python
    list, [L + 1]) the arc offset at which each link's adjacency begins"""


def clique_expected(links, n=CLIQUE_N, lo=CLIQUE_LO, hi=CLIQUE_HI):
    dev, L, K = links.device, links.size(0), hi - lo
    lk = wrap(links.to(torch.int64), n)
    x = CliqueExpected()
    x.K = K
    x.rowptr = torch.arange(L + 1, dtype=torch.int64, device=dev) * K          # every link lists the whole clique
    x.ids = torch.arange(lo, hi, dtype=torch.int64, device=dev).repeat(L)
    x.roots = (lk - lo).to(torch.int32)                                         # the local index of a node is its id - lo
    ru, rv = (lk[:, 0] - lo), (lk[:, 1] - lo)
    two = ru != rv
    row = torch.arange(L, device=dev)
    # h = 1 and the link masked: every other node is one hop from both roots; a root is 0 from itself and, without the link's own
    # edge, two hops from the other root: h + 1 = "not within h".  u == v: (0, 0)
    dist = torch.ones((L, K, 2), dtype=torch.uint8, device=dev)
    dist[row, ru, 0] = 0
    dist[row, rv, 1] = 0
    dist[row[two], ru[two], 1] = 2
    dist[row[two], rv[two], 0] = 2
    x.dist = dist.view(L * K, 2)
    # row i lists every j != i; with u != v the row of u leaves v out and the row of v leaves u out
    lengths = torch.full((L, K), K - 1, dtype=torch.int64, device=dev)
    lengths[row[two], ru[two]] -= 1
    lengths[row[two], rv[two]] -= 1
    x.lengths = lengths
    x.adj_ptr = torch.zeros((L * K + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(lengths.view(-1), 0, out=x.adj_ptr[1:])
    x.A = L * K * (K - 1) - 2 * int(two.sum())
    x.row_start = x.adj_ptr[::K].tolist()
    # DRNL with the other root removed: both roots 1; every other node is one hop from each root, 1 + 1 + 1 * (1 + 0 - 1) = 2
    z = torch.full((L, K), 2, dtype=torch.int64, device=dev)
    z[row, ru] = 1
    z[row, rv] = 1
    x.z = z.view(-1)
    return x


def clique_expected_arcs(x, q0, q1, lo=CLIQUE_LO):
    """(nbr int32, weight int32) of the links q0 .. q1 - 1, concatenated: from a [q1 - q0, K, K] mask of the arcs that are listed, the
    column index of every set entry and 1 + [(id_i + id_j) % 7 == 0]"""
    dev, K, c = x.roots.device, x.K, q1 - q0
    i = torch.arange(K, device=dev)
    mask = (i[:, None] != i[None, :]).expand(c, K, K).clone()
    ru, rv = x.roots[q0:q1, 0].to(torch.int64), x.roots[q0:q1, 1].to(torch.int64)
    two = ru != rv
    r = torch.arange(c, device=dev)[two]
    mask[r, ru[two], rv[two]] = False
    mask[r, rv[two], ru[two]] = False
    at = torch.nonzero(mask.view(-1)).flatten()
    del mask
    at %= K * K                                        # (row i, column j) of the link's K x K block
    ids = i + lo
    table = (1 + ((ids[:, None] + ids[None, :]) % 7 == 0).to(torch.int32)).view(-1)
    weight = table[at]
    at %= K
    return at.to(torch.int32), weight


def row_in_which(x, arc):
    """the link whose adjacency holds arc offset `arc`"""
    return int(np.searchsorted(np.asarray(x.row_start), arc, side='right')) - 1
