"""Planted inputs for the kernels of csrc/ss_components.hip, in numpy only: label arrays built wavefront by wavefront for
cc_sizes_kernel, (label, size, block_incl) triples that put the winner of the largest-component key at a chosen lane, wavefront, tile
and chunk for cc_roots_kernel, keys, masks, node lists, mappers, edge lists and links for the select, scatter, edge and same kernels
launched directly, and six graphs for the API (a late giant, two ties, three that pass the grid-stride cap).  Every plan comes with its
expected answer from numpy alone, and with numpy models of WRONG kernels (a half butterfly, a key from the first tile only, ties to the
larger root, workgroup 0 only, peel leftovers dropped or doubled, a tile rank without the earlier wavefronts, mask == 1, one stride
trip of the hook): tests/test_components_planted_host.py shows that each of them answers some plan differently from the right kernel.
The constants come from the sources: SS_COMPONENTS_CHUNK from the header, the block, the peel and the stride cap from the unit's text.
No test, no torch and no GPU code lives here; tests/test_components_planted_gpu.py launches the plans."""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

import components_restatement as restated

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(REPO, 'subgraph-sketching_amd', 'csrc', 'ss_components.hip')


def _constants():
    header = open(os.path.join(REPO, 'include', 'subgraph_sketch.h')).read()
    unit = open(UNIT).read()
    chunk = int(re.search(r'#define\s+SS_COMPONENTS_CHUNK\s+(\d+)', header).group(1))
    tile = int(re.search(r'constexpr int kCcBlock = (\d+);', unit).group(1))
    peel = int(re.search(r'constexpr int kCcPeel = (\d+);', unit).group(1))
    body = re.search(r'inline unsigned cc_stride_grid\(int64_t n\)[^{]*\{(.*?)\n\}', unit, flags=re.S).group(1)
    assert re.search(r'blocks = \(n \+ kCcBlock - 1\) / kCcBlock;', body), 'cc_stride_grid counts workgroups of kCcBlock items'
    lo, hi = re.search(r'return \(unsigned\)\(blocks < (\d+) \? blocks : (\d+)\);', body).groups()
    assert lo == hi, 'cc_stride_grid caps the grid at one number'
    return chunk, tile, peel, int(lo)


CHUNK, TILE, PEEL, STRIDE_BLOCKS = _constants()
WAVE = 64
TILES = CHUNK // TILE
STRIDE_CAP = STRIDE_BLOCKS * TILE  # the items one trip of a grid-stride launch covers: beyond it a thread takes a second item
N_BASE = 3 * CHUNK + TILE + 1  # three whole chunks, one whole tile, one node: the last wavefront has one live lane
SMALL_N = (CHUNK - 1, CHUNK, CHUNK + 1, WAVE - 1, WAVE, WAVE + 1)
KEY_LOW = 0xFFFFFFFF


def place(x):
    """(chunk, tile, wavefront, lane) of item x in the chunked kernels: a workgroup owns a chunk, thread t of it item t of every tile"""
    x = int(x)
    return x // CHUNK, x % CHUNK // TILE, x % TILE // WAVE, x % WAVE


def key_of(size, root):
    return (int(size) << 32) | (KEY_LOW - int(root))


def chunk_counts(flags):
    """how many of the flagged items each chunk holds"""
    n = len(flags)
    chunks = (n + CHUNK - 1) // CHUNK
    padded = np.zeros(chunks * CHUNK, dtype=np.int64)
    padded[:n] = np.asarray(flags, dtype=bool)
    return padded.reshape(chunks, CHUNK).sum(axis=1)


def check_labels(label, N):
    """what the sizes, roots, select and same kernels take for granted of a label array: they index size[label[x]]"""
    assert label.dtype == np.int32 and label.shape == (N,) and N >= 1
    assert int(label.min()) >= 0 and int(label.max()) < N, 'a label outside [0, N) would send an atomic out of bounds'


def check_block_incl(block_incl, flags):
    """a fill pass stores at block_incl[b - 1] + rank: anything but the inclusive sum of the true counts leaves the outputs"""
    assert block_incl.dtype == np.int64 and np.array_equal(block_incl, np.cumsum(chunk_counts(flags)))


def _frozen(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


# ---- 1. label arrays for ss_components_sizes --------------------------------------------------------------------------------------------
PATTERNS = ('one', 'four', 'five_60', 'five_1', 'sixty_four', 'alternate', 'leader63', 'shared', 'fixed')


def anchors(N):
    """the labels the `shared` wavefronts carry in turn; section 3 selects these four sets: node 0, the last node of chunk 0, the first
    node of chunk 2 and the last node (clipped to N - 1 in the small arrays)"""
    return [min(v, N - 1) for v in (0, CHUNK - 1, 2 * CHUNK, N - 1)]


@functools.lru_cache(maxsize=None)
def label_plan(N, first=0):
    """int32 [N] built wavefront by wavefront, cut off where N ends.  Wavefront w carries PATTERNS[(w + first) % 9]:
      one         all 64 lanes one label                            four        4 distinct labels, 16 lanes each: the peel limit
      five_60     4 labels on lanes 0..3, a fifth on the other 60   five_1      4 labels on lanes 0..62, a fifth on lane 63
      sixty_four  64 distinct labels                                alternate   two labels, lane by lane (one an anchor)
      leader63    lanes 0..62 one label, lane 63 another            shared      one of anchors(N) on all lanes, in several chunks
      fixed       label[x] == x at lanes 0 and 63, one other label between
    In the plan with first == 0 the first and the last wavefront of every chunk are `fixed` (the first and the last tile of a chunk)
    and the last node is its own label.  The other labels are drawn per wavefront, distinct within it."""
    assert N >= PEEL + 1
    rng = np.random.default_rng(20 + first)
    label = np.empty(N, dtype=np.int64)
    names, shared_seen = [], 0
    for w in range((N + WAVE - 1) // WAVE):
        b = w * WAVE
        n = min(WAVE, N - b)
        lanes = np.arange(n)
        name = 'fixed' if first == 0 and w % (CHUNK // WAVE) in (0, CHUNK // WAVE - 1) else PATTERNS[(w + first) % len(PATTERNS)]
        vals = rng.choice(N, size=min(WAVE, N), replace=False)
        if name == 'one':
            l = np.full(n, vals[0])
        elif name == 'four':
            l = vals[lanes % 4]
        elif name == 'five_60':
            l = vals[np.minimum(lanes, 4)]
        elif name == 'five_1':
            l = np.where(lanes == WAVE - 1, vals[4], vals[lanes % 4])
        elif name == 'sixty_four':
            l = vals[lanes % len(vals)]
        elif name == 'alternate':  # (one of the two is the anchor of the next `shared` wavefront: section 3 selects half wavefronts too)
            l = np.where(lanes % 2 == 0, anchors(N)[shared_seen % 4], vals[0] if vals[0] != anchors(N)[shared_seen % 4] else vals[1])
        elif name == 'leader63':
            l = np.where(lanes == WAVE - 1, vals[1], vals[0])
        elif name == 'shared':
            l = np.full(n, anchors(N)[shared_seen % 4])
            shared_seen += 1
        else:
            l = np.where((lanes == 0) | (lanes == WAVE - 1), b + lanes, vals[0])
        label[b:b + n] = l
        names.append(name)
    if first == 0:
        label[N - 1] = N - 1
    label = label.astype(np.int32)
    check_labels(label, N)
    return _frozen(SimpleNamespace(N=N, first=first, label=label, names=tuple(names), size=np.bincount(label, minlength=N).astype(np.int32),
                                   block_roots=chunk_counts(label == np.arange(N)).astype(np.int32)))


def label_plans():
    """the base array, the same patterns at the small sizes, and at N = 63, 64, 65 every rotation (one wavefront shows one pattern)"""
    plans = [(N_BASE, 0)] + [(N, 0) for N in SMALL_N]
    plans += [(N, first) for N in (WAVE - 1, WAVE, WAVE + 1) for first in range(1, len(PATTERNS) + 1)]
    return plans


def peel(l):
    """the sizes kernel on the live lanes of one wavefront: ([(label, lanes counted by one add)], the leftover lanes)"""
    rest, adds = list(range(len(l))), []
    for _ in range(PEEL):
        if not rest:
            break
        ll = l[rest[0]]
        adds.append((int(ll), sum(1 for i in rest if l[i] == ll)))
        rest = [i for i in rest if l[i] != ll]
    return adds, rest


def model_sizes(label, leftover=1):
    """size[] as cc_sizes_kernel adds it up; leftover = what a lane left over by the peel adds (1 is right, 0 drops it, 2 doubles it)"""
    N = len(label)
    size = np.zeros(N, dtype=np.int64)
    for b in range(0, N, WAVE):
        l = label[b:b + WAVE]
        adds, rest = peel(l)
        for ll, c in adds:
            size[ll] += c
        for i in rest:
            size[l[i]] += leftover
    return size


# ---- 2. (label, size, block_incl) for ss_components_roots -------------------------------------------------------------------------------
TOP = 5000  # the winning size; every other root's size is below 1 000, every non-root's word holds at least 2^20 (never to be read)
WINNERS = {
    'lane 0': 0, 'lane 31': 31, 'lane 32': 32, 'lane 63': 63, 'wavefront 1 lane 5': WAVE + 5, 'wavefront 3 lane 5': 3 * WAVE + 5,
    'last tile of a chunk': CHUNK + (TILES - 1) * TILE + 100, 'first tile of the last chunk': 3 * CHUNK + 70, 'last node': N_BASE - 1,
}
TIES = {  # name -> ((root, size), ...): the right winner first
    'tie at lanes 62 and 63': ((CHUNK + 5 * WAVE + 62, TOP), (CHUNK + 5 * WAVE + 63, TOP)),
    'tie in two wavefronts': ((CHUNK + 10, TOP), (CHUNK + 3 * TILE + 2 * WAVE + 10, TOP)),
    'tie in two workgroups': ((500, TOP), (2 * CHUNK + 500, TOP)),
    'larger size in the earlier workgroup': ((500, TOP), (2 * CHUNK + 500, TOP - 1)),
    'larger size in the later workgroup': ((2 * CHUNK + 500, TOP), (500, TOP - 1)),
    'size 2^31 - 1': ((2 * CHUNK + 77, (1 << 31) - 1), (90, (1 << 31) - 2)),
}
ROOTS_CASES = tuple(WINNERS) + tuple(TIES) + ('survives seven later tiles', 'chunk without a root', 'every node a root')


def _roots_case(name, is_root, size):
    N = len(is_root)
    x = np.arange(N, dtype=np.int64)
    assert is_root.any()
    below = np.maximum.accumulate(np.where(is_root, x, -1))  # a non-root points at the nearest root below it, or at the first root
    label = np.where(below >= 0, below, x[is_root][0]).astype(np.int32)
    check_labels(label, N)
    roots = np.flatnonzero(label == x).astype(np.int64)
    assert np.array_equal(roots, np.flatnonzero(is_root))
    block_incl = np.cumsum(chunk_counts(is_root)).astype(np.int64)
    check_block_incl(block_incl, label == x)
    sizes = size[roots].astype(np.int64)
    keys = [key_of(s, r) for r, s in zip(roots.tolist(), sizes.tolist())]
    best = max(keys)
    assert keys.count(best) == 1 and size.dtype == np.int32 and size.min() >= 1
    return _frozen(SimpleNamespace(name=name, N=N, label=label, size=size, block_incl=block_incl, roots=roots, sizes=sizes, best=best,
                                   winner=KEY_LOW - (best & KEY_LOW), top=best >> 32))


@functools.lru_cache(maxsize=None)
def roots_case(name):
    rng = np.random.default_rng(ROOTS_CASES.index(name) + 300)
    N = CHUNK + 1 if name == 'every node a root' else N_BASE
    is_root = rng.random(N) < 0.25
    if name == 'every node a root':
        is_root[:] = True
    elif name == 'chunk without a root':
        is_root[CHUNK:2 * CHUNK] = False
    size = np.where(is_root, rng.integers(1, 1000, size=N), rng.integers(1 << 20, 1 << 30, size=N)).astype(np.int32)

    def plant(x, s):
        is_root[x] = True
        size[x] = s

    if name in WINNERS:
        plant(WINNERS[name], TOP)
    elif name in TIES:
        for x, s in TIES[name]:
            plant(x, s)
    elif name == 'survives seven later tiles':  # the winner in the FIRST tile of a chunk, its thread meets a smaller root in every later tile
        for i in range(TILES):
            plant(CHUNK + 100 + i * TILE, TOP if i == 0 else 100 + i)
    elif name == 'chunk without a root':
        plant(2 * CHUNK + 300, TOP)
    else:
        plant(1500, TOP)
    size[~is_root] = np.maximum(size[~is_root], 1 << 20)
    return _roots_case(name, is_root, size)


def model_best(case, lanes=WAVE, first_tile_only=False, larger_root=False, chunk0_only=False):
    """(size, root) of the key cc_roots_kernel leaves in *best -- or a WRONG kernel: `lanes` < 64 a butterfly that brings lane 0 the
    maximum of the first `lanes` lanes only, first_tile_only a thread's key not carried past its first tile, larger_root the low word
    as the root itself (ties to the larger root), chunk0_only the maximum of workgroup 0 alone"""
    x = np.flatnonzero(case.label == np.arange(case.N))
    size = case.size[x].astype(np.int64)
    seen = x % WAVE < lanes
    if first_tile_only:
        seen &= x % CHUNK < TILE
    if chunk0_only:
        seen &= x < CHUNK
    if not seen.any():
        return 0, None
    x, size = x[seen], size[seen]
    order = np.lexsort((x if larger_root else -x, size))  # the last entry: the largest size, then the tie rule
    return int(size[order[-1]]), int(x[order[-1]])


def model_compact(keep, earlier_wavefronts=True):
    """the ids the fill passes store, by the kernels' own arithmetic (tile by tile: the running total, the kept items of the earlier
    wavefronts of the tile, the kept lanes below); earlier_wavefronts=False is the WRONG rank that forgets the earlier wavefronts.
    -1 marks an output word nobody stored to."""
    keep = np.asarray(keep, dtype=bool)
    out = np.full(int(keep.sum()), -1, dtype=np.int64)
    run = 0
    for s in range(0, len(keep), TILE):
        for w in range(0, TILE, WAVE):
            seg = keep[s + w:s + w + WAVE]
            before = int(keep[s:s + w].sum()) if earlier_wavefronts else 0
            out[run + before + np.cumsum(seg)[seg] - 1] = s + w + np.flatnonzero(seg)
        run += int(keep[s:s + TILE].sum())
    return out


# ---- 3. select, mapper, edges, same -----------------------------------------------------------------------------------------------------
def select_label_cases():
    """(root, *best, members): keys of an arbitrary high word that name each of anchors(N_BASE) over the base labels of section 1"""
    plan = label_plan(N_BASE)
    return [(root, key_of(12345 + k, root), np.flatnonzero(plan.label == root).astype(np.int64)) for k, root in enumerate(anchors(N_BASE))]


MASK_BYTES = (1, 2, 0x80, 0xFF)
MASK_RUNS = ((200, TILE), (2 * TILE, 2 * TILE + 8), (CHUNK - 3, CHUNK), (2 * CHUNK, 2 * CHUNK + 3),
             (2 * CHUNK + TILE - 2, 2 * CHUNK + TILE + 2), (3 * CHUNK - 1, 3 * CHUNK + 1), (N_BASE - 1, N_BASE))
MASKS = ('runs', 'everything', 'nothing')


@functools.lru_cache(maxsize=None)
def mask_plan(kind):
    """uint8 [N_BASE]; the kept bytes take the values 1, 2, 0x80, 0xFF in turn (the contract is != 0).  `runs`: kept runs that end at the
    last position of a tile / a chunk with the next position dropped, that start at the first position with the one before dropped, and
    that cross a tile and a chunk boundary; a sprinkle of kept nodes two positions or more away from every run"""
    N = N_BASE
    keep = np.zeros(N, dtype=bool)
    if kind == 'everything':
        keep[:] = True
    elif kind == 'runs':
        near = np.zeros(N, dtype=bool)
        for a, b in MASK_RUNS:
            near[max(a - 2, 0):b + 2] = True
        keep = (np.random.default_rng(5).random(N) < 0.3) & ~near
        for a, b in MASK_RUNS:
            keep[a:b] = True
    mask = np.zeros(N, dtype=np.uint8)
    mask[keep] = np.array(MASK_BYTES, dtype=np.uint8)[np.arange(int(keep.sum())) % len(MASK_BYTES)]
    return _frozen(SimpleNamespace(N=N, mask=mask, keep=keep))


def select_expected(N, keep):
    """(block_count, nodes, mapper) of a kept set"""
    nodes = np.flatnonzero(keep).astype(np.int64)
    mapper = np.full(N, -1, dtype=np.int64)
    mapper[nodes] = np.arange(len(nodes))
    return chunk_counts(keep).astype(np.int32), nodes, mapper


MAPPER_CASES = ('1', '255', '256', '257', '5000', 'twice in a wavefront', 'twice 4000 apart', 'twice as x and x - N', 'an id equal to N',
                'an id below -N')


@functools.lru_cache(maxsize=None)
def mapper_case(name):
    """a node list for ss_induced_mapper over N_BASE nodes, in random order, every other id written as x - N.
    -> nodes, err, dup, mapper (the ids listed once: their position; -1 outside the list), twice {id: its positions}"""
    N = N_BASE
    rng = np.random.default_rng(MAPPER_CASES.index(name) + 700)
    n = {'twice in a wavefront': 257, 'twice 4000 apart': 5000, 'twice as x and x - N': 256, 'an id equal to N': 300, 'an id below -N': 300}.get(name)
    n = int(name) if n is None else n
    ids = rng.permutation(N)[:n].astype(np.int64)
    assert n == 1 or (np.diff(ids) < 0).any()
    ids -= N * (np.arange(n) % 2)
    if name == 'twice in a wavefront':
        ids[40] = ids[3]
    elif name == 'twice 4000 apart':
        ids[4100] = ids[100]
    elif name == 'twice as x and x - N':
        ids[201] = ids[10] - N  # (position 10 is even: written as x)
    elif name == 'an id equal to N':
        ids[150] = N
    elif name == 'an id below -N':
        ids[151] = -N - 1
    w = np.where(ids < 0, ids + N, ids)
    ok = (w >= 0) & (w < N)
    mapper = np.full(N, -1, dtype=np.int64)
    twice = {}
    listed, count = np.unique(w[ok], return_counts=True)
    for x in listed[count > 1].tolist():
        twice[x] = np.flatnonzero(ok & (w == x)).tolist()
    once = ok & ~np.isin(w, list(twice))
    mapper[w[once]] = np.flatnonzero(once)
    return _frozen(SimpleNamespace(name=name, N=N, nodes=ids, err=int(not ok.all()), dup=int(bool(twice)), mapper=mapper, twice=twice))


EDGE_N = 1000
E_BASE = 2 * CHUNK + 300
EDGE_CASES = (('boundaries', E_BASE), ('hole', E_BASE), ('boundaries', CHUNK - 1), ('boundaries', CHUNK), ('boundaries', CHUNK + 1))


@functools.lru_cache(maxsize=None)
def edges_case(kind, E):
    """edges over EDGE_N nodes and a planted mapper (NOT a ranking: the new id of a kept node x is 7 x + 3; the nodes x % 3 == 0 are
    outside).  `boundaries`: kept edges at the last position of a tile / a chunk and the first of the next with their outer neighbours
    dropped, wavefront 8 kept whole beside wavefront 9 dropped whole, half of the rest kept; `hole`: nothing kept in chunk 1.  A dropped
    edge has its source, its destination or both outside.  One edge has an endpoint equal to N (dropped, the error word rises), one
    kept edge is written with negative ids."""
    N = EDGE_N
    rng = np.random.default_rng(E + len(kind))
    inside = np.arange(N) % 3 != 0
    mapper = np.where(inside, 7 * np.arange(N, dtype=np.int64) + 3, -1)
    keep = rng.random(E) < 0.5
    keep[8 * WAVE:9 * WAVE] = True
    keep[9 * WAVE:10 * WAVE] = False
    for edge in (TILE, CHUNK, 2 * CHUNK, CHUNK + 5 * TILE):  # ... dropped, KEPT | KEPT, dropped ...
        for e, k in ((edge - 2, False), (edge - 1, True), (edge, True), (edge + 1, False)):
            if e < E:
                keep[e] = k
    if kind == 'hole':
        keep[CHUNK:2 * CHUNK] = False
    kept_nodes, dropped_nodes = np.flatnonzero(inside), np.flatnonzero(~inside)
    src = np.where(keep, rng.choice(kept_nodes, size=E), rng.choice(dropped_nodes, size=E)).astype(np.int64)
    dst = np.where(keep, rng.choice(kept_nodes, size=E), rng.choice(dropped_nodes, size=E)).astype(np.int64)
    how = rng.integers(0, 3, size=E)  # a dropped edge: 0 both ends outside, 1 the source only, 2 the destination only
    dst = np.where(~keep & (how == 1), rng.choice(kept_nodes, size=E), dst)
    src = np.where(~keep & (how == 2), rng.choice(kept_nodes, size=E), src)
    bad, negative = int(np.flatnonzero(~keep)[20]), int(np.flatnonzero(keep)[33])
    dst[bad] = N
    src[bad] = kept_nodes[0]
    src[negative] -= N
    dst[negative] -= N
    ws, wd = restated.wrapped(N, src), restated.wrapped(N, dst)
    ok = (ws < N) & (wd < N)
    ids = np.flatnonzero(ok & (mapper[np.minimum(ws, N - 1)] >= 0) & (mapper[np.minimum(wd, N - 1)] >= 0)).astype(np.int64)
    assert np.array_equal(ids, np.flatnonzero(keep))
    block_incl = np.cumsum(chunk_counts(keep)).astype(np.int64)
    return _frozen(SimpleNamespace(kind=kind, N=N, E=E, src=src, dst=dst, mapper=mapper, keep=keep, block_count=chunk_counts(keep).astype(np.int32),
                                   block_incl=block_incl, out_src=mapper[ws[ids]], out_dst=mapper[wd[ids]], edge_ids=ids, err=1))


SAME_L = (255, 256, 257)


@functools.lru_cache(maxsize=None)
def same_case(L):
    """int64 [L, 2] links over the base labels of section 1: both signs and both orders of a pair, u == v, pairs inside one label and
    across two, and (position 100) one id equal to N: its answer is 0 and the error word rises"""
    plan = label_plan(N_BASE)
    N, label = plan.N, plan.label
    rng = np.random.default_rng(L)
    u = rng.integers(0, N, size=L)
    v = rng.integers(0, N, size=L)
    together = np.arange(L) % 2 == 0  # v from u's label class
    order = np.argsort(label, kind='stable')
    start = np.searchsorted(label[order], label[u], 'left')
    count = np.searchsorted(label[order], label[u], 'right') - start
    v = np.where(together, order[start + rng.integers(0, 1 << 30, size=L) % count], v)
    links = np.stack([u, v], axis=1).astype(np.int64)
    links[0::5, 0] -= N
    links[1::7, 1] -= N
    links[3] = links[2][::-1]            # both orders of one pair
    links[5] = links[4] - N              # ... and both signs
    links[6] = (77, 77)
    links[7] = (77, 77 - N)
    links[100] = (5, N)
    w = restated.wrapped(N, links)
    ok = (w < N).all(axis=1)
    out = (ok & (label[np.minimum(w[:, 0], N - 1)] == label[np.minimum(w[:, 1], N - 1)])).astype(np.uint8)
    return _frozen(SimpleNamespace(N=N, L=L, links=links, out=out, err=int(not ok.all())))


# ---- 4. graphs for the API (tests/test_components_gpu.py) -------------------------------------------------------------------------------
PATH_NODES = 777
STRIDE_N = 1_100_000
STRIDE_UNDIRECTED = 700_000


def _two_paths(a, b, step):
    """two paths of PATH_NODES nodes from a and from b in steps of `step`; the edges of the path with the larger ids come first"""
    k = np.arange(PATH_NODES - 1, dtype=np.int64) * step
    first = np.stack([a + k, a + k + step])
    return np.concatenate([first + (b - a), first], axis=1)


def late_giant():
    shift = 3 * CHUNK + 191
    return shift + 20000, restated.symmetric_random_graph(20000, 60000, 31) + shift


def tie_across_workgroups():
    return 18 * CHUNK, _two_paths(5 * CHUNK + 100, 17 * CHUNK + 63, 1)


def tie_in_one_wavefront():
    return 18 * CHUNK, _two_paths(9 * CHUNK + 62, 9 * CHUNK + 63, 2)


def stride_random():
    return STRIDE_N, restated.symmetric_random_graph(STRIDE_N, STRIDE_UNDIRECTED, 32)


def stride_random_shuffled():
    """the arcs of stride_random in a random order.  symmetric_random_graph lists the second direction of every pair behind the first,
    so the arcs of stride_random beyond STRIDE_CAP only repeat edges the first trip has seen; shuffled, they carry edges of their own"""
    n, ei = stride_random()
    return n, ei[:, np.random.default_rng(34).permutation(ei.shape[1])]


def stride_path():
    """the path over STRIDE_N nodes with its edges shuffled and its node ids permuted: a deep chain that jumps all over the id range"""
    rng = np.random.default_rng(33)
    lo = rng.permutation(STRIDE_N - 1).astype(np.int64)
    return STRIDE_N, rng.permutation(STRIDE_N)[np.stack([lo, lo + 1])]


API_GRAPHS = {'late giant': late_giant, 'tie across workgroups': tie_across_workgroups, 'tie in one wavefront': tie_in_one_wavefront,
              'stride random': stride_random, 'stride random shuffled': stride_random_shuffled, 'stride path': stride_path}
STRIDE_GRAPHS = ('stride random', 'stride random shuffled', 'stride path')
assert STRIDE_N > STRIDE_CAP and 2 * STRIDE_UNDIRECTED > STRIDE_CAP and STRIDE_N - 1 > STRIDE_CAP, 'the stride graphs pass the grid-stride cap'
