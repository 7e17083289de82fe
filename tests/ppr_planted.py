"""A graph planted on the branches of csrc/ss_ppr.hip, for tests/test_ppr_planted_host.py and tests/test_ppr_planted_gpu.py.  No
test and no GPU code lives here.

N = 257 * 64 + 1 rows: 258 row workgroups (the finalize kernel's 256 threads stride twice over the partials) and a last workgroup
of one row.  TARGET rows hold an exact number of kept in-edges from random feeders -- the trips of ppr_gather's unrolled body and
tail in both halves, the hub rule at 256 / 257, the last segments of 1, 2, 255 and 256 edges -- and sit at the first row, the
last row of workgroup 0, the first of workgroup 1, the lone last row, and side by side from 128 on.  One broadcaster B spreads
every source's mass over all feeders within three steps, so that the long sums add non-zero terms.  Forty zero-sum rows store
entries into rows 1000 and 1004 that the operator drops: 1000 stores 296 and keeps 256 (no hub), 1004 stores 297 and keeps 257
(a hub of two segments).  Every kept weight is positive, which is what lets the vectors be compared at 1e-10 RELATIVE."""
import functools

import numpy as np
import scipy.sparse as sp

from ppr_restatement import operator, pagerank_power

SEGMENT = 256                    # SS_PPR_SEGMENT
ROWS_PER_BLOCK = 64
N = 257 * ROWS_PER_BLOCK + 1     # 16 449
FEEDER_LO, FEEDER_HI = 2048, N - 1   # feeders are FEEDER_LO .. N - 2
B = 1500
KEPT_256, KEPT_257, SINK, DANGLING = 1000, 1004, 1010, 1020
ZERO_ROWS = np.arange(1100, 1140)
ISOLATED = 1050                  # one of 1021 .. 1099, which have no entry at all
SMALL_DEGREES = (0, 1, 2, 3, 7, 8, 9, 10, 15, 16, 17, 18, 255, 256)
FIXED_PLACES = (0, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, N - 1)
VARIANTS = {'one': (), 'four': (257, 512, 513), 'five': (257, 512, 513, 1025),
            'nine': (257, 258, 511, 512, 513, 768, 769, 1025)}
COUNTS = {'one': (1, 2), 'four': (4, 9), 'five': (5, 14), 'nine': (9, 25)}   # (n_hubs, n_segments), row 1004 included
QUICK = (SINK, DANGLING, ISOLATED, int(ZERO_ROWS[7]))   # sources that are their own fixed point: one step, exactly e_src

ROWS_CFG = dict(p=0.85, tol=1e-6, max_iter=12)    # every planted row, the widths, the direct launches
STOPS_CFG = dict(p=0.5, tol=1e-3, max_iter=60)    # columns that stop at different steps
MARGIN = 1e-6                                     # no restated residual within MARGIN * tol of tol: counts must be EQUAL


def planted(hub_degrees, seed=20):
    """(A, description): A float64 csr_matrix [N, N] with A[u, v] the weight of u -> v"""
    rng = np.random.RandomState(seed)
    degrees = list(SMALL_DEGREES) + list(hub_degrees)
    places = list(FIXED_PLACES) + list(range(128, 128 + len(degrees) - len(FIXED_PLACES)))
    order = rng.permutation(len(degrees))
    targets = {int(places[i]): int(degrees[order[i]]) for i in range(len(degrees))}
    feeders = np.arange(FEEDER_LO, FEEDER_HI)
    src, dst, w = [], [], []

    def add(u, v, weight):
        src.append(np.broadcast_to(np.asarray(u, dtype=np.int64), np.broadcast(u, v).shape).ravel())
        dst.append(np.broadcast_to(np.asarray(v, dtype=np.int64), np.broadcast(u, v).shape).ravel())
        w.append(np.broadcast_to(np.asarray(weight, dtype=np.float64), src[-1].shape).ravel())

    in_rows = dict(targets)
    in_rows[KEPT_256], in_rows[KEPT_257] = 256, 257
    for t in sorted(in_rows):
        d = in_rows[t]
        if d:
            add(rng.choice(feeders, size=d, replace=False), t, rng.uniform(0.05, 3.0, size=d))
        add(t, B, 1.0)
    add(B, feeders, rng.uniform(0.5, 1.5, size=len(feeders)))
    add(feeders, np.roll(feeders, -1), rng.uniform(0.5, 1.5, size=len(feeders)))   # the ring f_i -> f_(i+1)
    add(ZERO_ROWS, KEPT_256, 1.5)
    add(ZERO_ROWS, KEPT_257, 1.5)
    add(ZERO_ROWS, SINK, -3.0)
    add(feeders[11], DANGLING, 0.75)
    A = sp.csr_matrix((np.concatenate(w), (np.concatenate(src), np.concatenate(dst))), shape=(N, N))
    hubs = sorted(t for t, d in in_rows.items() if d > SEGMENT)
    feeding = np.unique(A.tocsc()[:, sorted(in_rows)].nonzero()[0])
    feeding = feeding[(feeding >= FEEDER_LO) & (feeding < FEEDER_HI)]   # feeders with an edge into a planted row
    desc = dict(feeding=feeding, N=N, targets=targets, in_rows=in_rows, hubs=hubs, hub_degrees=tuple(hub_degrees), seed=seed,
                n_hubs=len(hubs), n_segments=int(sum(-(-in_rows[t] // SEGMENT) for t in hubs)))
    return A, desc


@functools.lru_cache(maxsize=None)
def variant(name):
    A, desc = planted(VARIANTS[name])
    desc['name'] = name
    return A, desc


def sources(desc, kind):
    """'widths': 129 distinct sources -- every hub row, the four fixed places, rows 1000 and 1004, B, the four QUICK sources, every
    other target row, random feeders (of those with an edge into a planted row: the others crawl along the ring first).
    'rows' = 'stops': its first 70 (all of the named ones, then feeders)."""
    named = list(desc['hubs']) + list(FIXED_PLACES) + [KEPT_256, KEPT_257, B] + list(QUICK) + sorted(desc['targets'])
    seen, out = set(), []
    for s in named:
        if s not in seen:
            seen.add(s)
            out.append(int(s))
    rng = np.random.RandomState(desc['seed'] + 1)
    fill = rng.choice(desc['feeding'], size=129 - len(out), replace=False)
    out += [int(f) for f in fill]
    return out[:{'widths': 129, 'rows': 70, 'stops': 70}[kind]]


def kept_operator(A, p):
    """the restated operator with sorted rows: row v lists the kept in-edges of v in ascending u, the order the kernel adds them in"""
    W, z = operator(A, p)
    W.sort_indices()
    assert W.nnz == np.count_nonzero(W.data)   # no explicit zero: np.diff(W.indptr) is the kept in-degree
    return W, z


def hub_plan(deg):
    """rows with more than SEGMENT kept entries, ceil(deg / SEGMENT) segments each, ascending"""
    hubs = np.nonzero(deg > SEGMENT)[0]
    nseg = -(-deg[hubs] // SEGMENT)
    hub_seg = np.concatenate([[0], np.cumsum(nseg)])
    seg_hub = np.repeat(np.arange(len(hubs)), nseg)
    return hubs, hub_seg, seg_hub


def power(W, z, srcs, tol, max_iter, no_teleport_from=None):
    """ppr_restatement.pagerank_power on a GIVEN operator (its loop, line for line); no_teleport_from = c leaves the s (z^T x)
    term out of the columns >= c.  Returns (vectors, iterations, residuals) like pagerank_power."""
    n, K = W.shape[0], len(srcs)
    s = np.zeros((n, K))
    s[np.asarray(srcs), np.arange(K)] = n
    tele = s.copy()
    if no_teleport_from is not None:
        tele[:, no_teleport_from:] = 0.0
    x = s.copy()
    oldx = np.zeros((n, K))
    active = np.ones(K, dtype=bool)
    iters = np.zeros(K, dtype=np.int64)
    residuals = [[] for _ in range(K)]
    while True:
        res = np.sqrt(((x - oldx) ** 2).sum(axis=0))
        for j in np.nonzero(active)[0]:
            residuals[j].append(res[j])
        active &= res > tol
        if not active.any():
            break
        cols = np.nonzero(active)[0]
        oldx[:, cols] = x[:, cols]
        xa = x[:, cols]
        x[:, cols] = W @ xa + tele[:, cols] * (z @ xa)[None, :]
        iters[cols] += 1
        active &= ~(iters >= max_iter)
        for j in cols[~active[cols]]:
            residuals[j].append(np.sqrt(((x[:, j] - oldx[:, j]) ** 2).sum()))
    return (x / x.sum(axis=0)).T, iters, residuals


MUTATIONS = ('segment_end', 'odd_tail', 'stored_degree', 'no_teleport')


def mutate(W, p, name):
    """the restated operator with one of the kernel's boundaries moved (a copy; W has sorted rows):
    segment_end    the last edge of every full 256-edge segment of every hub is dropped
    odd_tail       the last odd-position edge of every row whose degree is 8k + 2 .. 8k + 8 is dropped
    stored_degree  row 1000 keeps the zero-sum rows' entries, as if its stored degree counted: weight p * 1.5 / 1
    no_teleport    W unchanged: power(..., no_teleport_from=64) leaves the source term out of the second slice"""
    W = W.tolil(copy=True)
    deg = np.diff(W.tocsr().indptr)
    if name == 'segment_end':
        for v in np.nonzero(deg > SEGMENT)[0]:
            cols = list(W.rows[v])
            for e in range(SEGMENT - 1, len(cols), SEGMENT):
                W[v, cols[e]] = 0.0
    elif name == 'odd_tail':
        for v in np.nonzero((deg >= 2) & (deg % 8 != 1))[0]:
            cols = list(W.rows[v])
            d = len(cols)
            W[v, cols[d - 1 if (d - 1) % 2 else d - 2]] = 0.0
    elif name == 'stored_degree':
        for u in ZERO_ROWS:
            W[KEPT_256, int(u)] = p * 1.5 / 1
    elif name != 'no_teleport':
        raise ValueError(name)
    W = W.tocsr()
    W.eliminate_zeros()
    W.sort_indices()
    return W


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def restated(name, kind, cfg_name):
    """pagerank_power of sources(variant, kind) under ROWS_CFG ('rows') or STOPS_CFG ('stops'): computed once per process, shared by
    every test that needs it, read-only.  Returns (sources, vectors, iterations, residuals)."""
    A, desc = variant(name)
    cfg = {'rows': ROWS_CFG, 'stops': STOPS_CFG}[cfg_name]
    srcs = sources(desc, kind)
    vec, iters, res = pagerank_power(A, srcs, **cfg)
    _frozen(vec, iters)
    return tuple(srcs), vec, iters, tuple(tuple(r) for r in res)


def closest_residual(residuals, tol):
    """min over every residual the stop rule compared of |r - tol| / tol"""
    return min(abs(r - tol) / tol for col in residuals for r in col)


def stop_order(srcs, iters):
    """128 columns for knobs.PPR_COLUMNS = 128 from the restated counts of `srcs`: pair (0, 1) stops on the left first, pair (2, 3) on
    the right first, pair (4, 5) is (quick, slow), pair (6, 7) is (slow, quick), columns 8 .. 63 are further slow sources, and
    columns 64 .. 127 are the quick sources over and over.  Returns (the list, the names of the pairs -> their columns)."""
    iters = np.asarray(iters)
    slow = [j for j in np.argsort(iters, kind='stable') if iters[j] > 1]
    quick = [j for j in range(len(srcs)) if iters[j] == 1]
    assert len(slow) >= 60 and len(quick) >= 2
    first, second, late, last = slow[0], slow[1], slow[-2], slow[-1]
    assert iters[first] < iters[last] and iters[second] < iters[late]
    rest = slow[2:-2]
    cols = [first, last, late, second, quick[0], rest.pop(0), rest.pop(0), quick[1]] + rest[:56]
    assert len(cols) == 64
    cols += [quick[i % len(quick)] for i in range(64)]
    pairs = {'left_first': (0, 1), 'right_first': (2, 3), 'quick_slow': (4, 5), 'slow_quick': (6, 7)}
    return [int(srcs[j]) for j in cols], pairs


def worst_by_row(got, want, desc):
    """text: for every target row, hub and kept-degree row, the worst relative error of its column of `got` [K, N] -- the report of
    a failing comparison names the degree that went wrong"""
    lines = []
    for v, d in sorted(desc['in_rows'].items(), key=lambda kv: kv[1]):
        g, r = got[:, v], want[:, v]
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = np.where(r != 0, np.abs(g - r) / np.abs(r), np.where(g != 0, np.inf, 0.0))
        lines.append(f'row {v:6d} kept in-degree {d:5d}: worst relative error {rel.max():.3e}')
    return '\n'.join(lines)


def worst_relative(got, want):
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got != 0, np.inf, 0.0))
    return float(rel.max())


def ring_graph(n, seed=31):
    """the graph of the index-width test: a directed ring v -> v + 1 with random positive weights, plus edges both ways between each
    of the last 64 rows and the rows 2^20 - 1, 2^20 and 2^20 + 1"""
    rng = np.random.RandomState(seed)
    v = np.arange(n, dtype=np.int64)
    last = np.arange(n - 64, n, dtype=np.int64)
    line = np.array([(1 << 20) - 1, 1 << 20, (1 << 20) + 1], dtype=np.int64)
    a, b = np.repeat(last, 3), np.tile(line, 64)
    src = np.concatenate([v, a, b])
    dst = np.concatenate([(v + 1) % n, b, a])
    w = rng.uniform(0.5, 1.5, size=len(src))
    return sp.csr_matrix((w, (src, dst)), shape=(n, n)), last, line
