"""ElphHashes.rank_links restated in numpy from a score matrix: shared by test_rank_links_host.py and
test_rank_links_gpu.py.  Nothing here touches the engine."""
import numpy as np


def wrap(ids, N):
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids < 0, ids + N, ids)


def candidates(u, t, N, exclude=None):
    """bool [N]: C = {v : v != u, v != t, (u -> v) not in exclude}; exclude [2, E] is read as a set (wrapped ids)"""
    c = np.ones(N, dtype=bool)
    c[u] = c[t] = False
    if exclude is not None:
        ex = wrap(exclude, N)
        c[ex[1][ex[0] == u]] = False
    return c


def rank_counts(score_row, links, N, exclude=None):
    """(greater, equal) int64 [L] of links [L, 2]; score_row(q, u) -> float32 [N], the scores s(u, .) of link q's source.
    greater[q] = #{v in C_q : s(u, v) > s(u, t)}, equal[q] = #{v in C_q : s(u, v) == s(u, t)}, float compares"""
    links = wrap(links, N).reshape(-1, 2)
    greater = np.zeros(len(links), dtype=np.int64)
    equal = np.zeros(len(links), dtype=np.int64)
    for q, (u, t) in enumerate(links):
        s = np.asarray(score_row(q, int(u)), dtype=np.float32)
        c = candidates(int(u), int(t), N, exclude)
        greater[q] = int(np.count_nonzero(s[c] > s[t]))
        equal[q] = int(np.count_nonzero(s[c] == s[t]))
    return greater, equal


def tied_below(score_row, links, N, exclude=None):
    """#{v in C_q : s(u, v) == s(u, t), v < t}: with `greater`, the place of t in the row sorted by (score desc, id asc)"""
    links = wrap(links, N).reshape(-1, 2)
    out = np.zeros(len(links), dtype=np.int64)
    for q, (u, t) in enumerate(links):
        s = np.asarray(score_row(q, int(u)), dtype=np.float32)
        c = candidates(int(u), int(t), N, exclude)
        c[t:] = False
        out[q] = int(np.count_nonzero(s[c] == s[t]))
    return out
