"""The semantics of NegativeSampler.sample / sample_negatives (subgraph-sketching_amd/negatives.py, csrc/ss_negatives.hip)
restated in Python ints and numpy, one slot at a time, plus the graph the negative-sampling tests share.  Nothing here imports the
package: the GPU tests compare the kernel with this file, the host tests compare this file with a set-based checker of their own."""
import functools

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MODES = ('uniform', 'same_source', 'wedge')


def hash_u64(x):
    """the splitmix64 finaliser (csrc/ss_common.hpp hash_u64) on a Python int"""
    x &= MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def draw(seed, q, a, c):
    """draw c (0 or 1) of attempt a of slot q"""
    return hash_u64(hash_u64(seed ^ hash_u64(q + 1)) + GOLDEN * (2 * a + c + 1))


def pick(r, n):
    """a draw mapped to [0, n): the high 64 bits of r * n"""
    return (r * n) >> 64


@functools.lru_cache(maxsize=None)
def _graph():
    N = 400
    rng = np.random.RandomState(7)
    parts = [rng.randint(0, 360, size=(2, 1200)).astype(np.int64)]                                   # the random part: ids 0..359
    parts.append(np.stack([np.full(10, 398), np.arange(388, 398)]))                                   # a star: centre 398, leaves 388..397
    parts.append(np.array([[a, b] for a in range(383, 388) for b in range(a + 1, 388)]).T)            # a K5 on 383..387
    parts.append(np.stack([np.full(150, 382), np.arange(150)]))                                       # a hub: 382 joined to 0..149
    parts.append(np.array([[3, 3], [5, 5]]))                                                          # the edge (3, 5) twice
    e = np.concatenate(parts, axis=1).astype(np.int64)                                                # (360..381 and 399 stay isolated)
    ei = np.concatenate([e, e[::-1]], axis=1)
    ei.setflags(write=False)
    return N, ei


def negatives_graph():
    """(N, edge_index int64 [2, E], symmetric): 1 200 random undirected edges among ids 0..359, a hub of degree >= 150 (382), a K5
    (383..387), a star (398 with leaves 388..397), isolated nodes (360..381, 399) and the edge (3, 5) twice"""
    return _graph()


# the sources of directed_graph(), by what the wedge walk meets at each
DIRECTED_SOURCES = {'mixed': 0, 'all_sinks': 5, 'rejected': 20, 'repeated': 30, 'no_out_arc': 40}


@functools.lru_cache(maxsize=None)
def _directed():
    e = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 10), (1, 11), (2, 11), (2, 12), (2, 0),   # 0: 1 and 2 lead on, 3 and 4 are sinks
         (5, 6), (5, 7), (5, 8),                                                         # 5: every neighbour is a sink
         (20, 21), (20, 22), (21, 20), (21, 22), (22, 20), (22, 21),                     # 20: two steps end in 20, 21 or 22 only
         (30, 31), (30, 31), (30, 31), (30, 32), (31, 33), (31, 34), (32, 35),           # 30: the arc 30 -> 31 three times
         (41, 40), (41, 42), (42, 40)]                                                   # 40: arcs in, none out
    ei = np.array(e, dtype=np.int64).T
    ei.setflags(write=False)
    return 48, ei


def directed_graph():
    """(N, edge_index int64 [2, E], DIRECTED: no arc has its reverse unless listed): the sources DIRECTED_SOURCES -- one whose
    neighbours are partly sinks (nodes without an out-arc), one whose neighbours are all sinks (every wedge attempt stops at its w:
    every slot unsampled), one whose two-step endpoints are itself and its own out-neighbours only (every proposal rejected), one
    with a repeated out-arc, one without an out-arc"""
    return _directed()


def rows_of(N, ei):
    """row u = the sorted list of every v with u -> v in ei, duplicates kept, negative ids wrapped"""
    rows = [[] for _ in range(N)]
    if ei is not None:
        for u, v in zip(*np.asarray(ei).tolist()):
            rows[u + N if u < 0 else u].append(v + N if v < 0 else v)
    return [sorted(r) for r in rows]


def sample(N, ei, positives=None, num_neg=1, mode='wedge', seed=0, max_tries=16, num_samples=None, exclude=None, slots=None):
    """(int64 [n_slots, 2], number of unsampled slots): what .sample returns, slot by slot.  slots: a range of slot numbers -- only
    those rows are computed (a call split into launches)"""
    assert mode in MODES
    rows = rows_of(N, ei)
    sets = [set(r) for r in rows]
    gone = [set(r) for r in rows_of(N, exclude)]
    n_slots = int(num_samples) if positives is None else len(positives) * num_neg
    out, unsampled = [], 0
    for q in (range(n_slots) if slots is None else slots):
        u = None
        if positives is not None:
            u = int(positives[q // num_neg][0])
            u = u + N if u < 0 else u
        v = -1
        for a in range(max_tries):
            r0, r1 = draw(seed, q, a, 0), draw(seed, q, a, 1)
            if mode == 'wedge':
                if not rows[u]:
                    break
                w = rows[u][pick(r0, len(rows[u]))]
                if not rows[w]:
                    continue
                c = rows[w][pick(r1, len(rows[w]))]
            else:
                if positives is None:
                    u = pick(r0, N)
                c = pick(r1, N)
            if c != u and c not in sets[u] and c not in gone[u]:
                v = c
                break
        out.append((u, v))
        unsampled += v < 0
    return np.array(out, dtype=np.int64).reshape(-1, 2), int(unsampled)
