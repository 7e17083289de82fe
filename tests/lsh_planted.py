"""Planted MinHash tables for the LSH tests (test_lsh_host.py, test_lsh_planted_gpu.py): tables whose buckets are known from a plan,
so that a test reaches a tile shape, a bucket size or a row offset on purpose and not because a graph happens to produce it.  No test
lives here.

    background row v     word j * rows of band j holds (v * UNIQUE_MULT + j * BAND_STEP) mod 2^32 -- v -> v * odd mod 2^32 is a bijection,
                         so no two rows agree on a band; every other word is a counter-based pseudo-random value of (seed, v, word)
    words >= rows * b    noise of (noise_seed, v, word): the index must not look at them
    group (members, J)   members[1:] copy members[0]'s slice in every band of J.  A node is in at most one group per band (check_plan),
                         so the bucket of (j, v) is v's group in band j, or {v}
    near miss            (v, leader, j, w): v copies the leader's slice of band j EXCEPT word w of it, where it keeps its own value, and
                         so stays alone in band j -- one word away from a bucket (a comparison that skips a word lists it)

planted_table is the numpy generator, planted_table_torch its twin in stock torch operators on any device (the table of more than
4 GiB is made by it in row blocks); expected() derives (rowptr, ids, bands) and skipped_buckets from the plan alone, never reading
a table; band_keys restates band_key / hash_u64 of csrc/ss_lsh.hip and csrc/ss_common.hpp in numpy."""
import numpy as np

import lsh_restatement as restated

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
UNIQUE_MULT = 0x9E3779B1          # odd
BAND_STEP = 0x85EBCA6B
GOLDEN = 0x9E3779B97F4A7C15
MIX_1, MIX_2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def resolve_bands(P, rows, bands):
    b = P // rows if bands is None else bands
    assert rows >= 1 and b >= 1 and rows * b <= P
    return b


def tile_rows(P):
    """rows of the table per workgroup of the keys kernel"""
    return min(64, 8192 // P)


def check_plan(N, b, groups):
    seen = set()
    for members, band_set in groups:
        assert len(members) >= 2 and len(set(members)) == len(members) and all(0 <= v < N for v in members)
        for j in band_set:
            assert 0 <= j < b
            for v in members:
                assert (j, v) not in seen, f'node {v} is in two groups of band {j}'
                seen.add((j, v))


# ---- the generator, in numpy and in torch ---------------------------------------------------------------------------------------
def mix64(x):
    """the splitmix64 finaliser (hash_u64 of ss_common.hpp) on a uint64 array; array arithmetic wraps mod 2^64"""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(MIX_1)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(MIX_2)
    return x ^ (x >> np.uint64(31))


def _word_seeds(P, rows, b, seed, noise_seed):
    """per word of a row the 64-bit offset of its counter: the words in use by `seed`, the noise behind them by `noise_seed`"""
    noise_seed = seed if noise_seed is None else noise_seed
    return [((seed if c < rows * b else noise_seed) + 1) * GOLDEN & M64 for c in range(P)]


def planted_table(N, P, rows, bands, groups, seed, noise_seed=None, near=()):
    """int64 numpy [N, P], values in [0, 2^32)"""
    b = resolve_bands(P, rows, bands)
    check_plan(N, b, groups)
    v = np.arange(N, dtype=np.uint64)[:, None]
    c = np.arange(P, dtype=np.uint64)[None, :]
    offs = np.array(_word_seeds(P, rows, b, seed, noise_seed), dtype=np.uint64)[None, :]
    t = (mix64(v * np.uint64(P) + c + offs) >> np.uint64(32)).astype(np.int64)
    ids = np.arange(N, dtype=np.int64)
    for j in range(b):
        t[:, j * rows] = (ids * UNIQUE_MULT + j * BAND_STEP) & M32
    for members, band_set in groups:
        for j in band_set:
            t[np.asarray(members[1:]), j * rows:(j + 1) * rows] = t[members[0], j * rows:(j + 1) * rows]
    for v, leader, j, w in near:
        assert 0 <= w < rows and rows >= 2 and all(v not in members for members, band_set in groups if j in band_set)
        keep = np.arange(rows) != w
        t[v, j * rows:(j + 1) * rows][keep] = t[leader, j * rows:(j + 1) * rows][keep]
    return t


def _s64(x):
    return x - (1 << 64) if x >= (1 << 63) else x


def _lsr(x, k):
    """logical shift right of an int64 torch tensor"""
    return (x >> k) & ((1 << (64 - k)) - 1)


def planted_table_torch(N, P, rows, bands, groups, seed, device, dtype=None, block=1 << 18, noise_seed=None, near=()):
    """planted_table in torch operators, `block` rows at a time: torch.int64 values in [0, 2^32) (the default) or torch.int32 holding
    the same uint32 bit patterns"""
    import torch
    dtype = torch.int64 if dtype is None else dtype
    assert dtype in (torch.int64, torch.int32)
    b = resolve_bands(P, rows, bands)
    check_plan(N, b, groups)
    out = torch.empty((N, P), dtype=dtype, device=device)
    c = torch.arange(P, dtype=torch.int64, device=device)[None, :]
    offs = torch.tensor([_s64(x) for x in _word_seeds(P, rows, b, seed, noise_seed)], dtype=torch.int64, device=device)[None, :]
    first = torch.arange(b, dtype=torch.int64, device=device) * rows
    for v0 in range(0, N, block):
        v = torch.arange(v0, min(N, v0 + block), dtype=torch.int64, device=device)[:, None]
        x = v * P + c + offs
        x = x ^ _lsr(x, 30)
        x = x * _s64(MIX_1)
        x = x ^ _lsr(x, 27)
        x = x * _s64(MIX_2)
        x = _lsr(x ^ _lsr(x, 31), 32)
        x[:, first] = (v * UNIQUE_MULT + (first // rows)[None, :] * BAND_STEP) & M32
        out[v0:v0 + block] = x if dtype == torch.int64 else ((x ^ (1 << 31)) - (1 << 31)).to(torch.int32)
    for members, band_set in groups:
        rest = torch.tensor(list(members[1:]), dtype=torch.int64, device=device)
        for j in band_set:
            out[rest, j * rows:(j + 1) * rows] = out[members[0], j * rows:(j + 1) * rows].clone()
    for v, leader, j, w in near:
        for i in range(rows):
            if i != w:
                out[v, j * rows + i] = out[leader, j * rows + i]
    return out


# ---- what the plan says ---------------------------------------------------------------------------------------------------------
def expected(N, rows, bands, groups, sources, max_bucket, exclude=None, min_bands=1):
    """((rowptr int64 [S + 1], ids int64 [T], bands int32 [T]), skipped_buckets int64 [bands]) from the plan alone (`rows` does not
    matter to it: a band is a bucket whatever its width)"""
    check_plan(N, bands, groups)
    bucket = [dict() for _ in range(bands)]
    skipped = np.zeros(bands, dtype=np.int64)
    for members, band_set in groups:
        for j in band_set:
            if len(members) > max_bucket:
                skipped[j] += 1
            else:
                bucket[j].update((v, members) for v in members)
    gone = set()
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64).reshape(2, -1)
        gone = set(zip(*np.where(ex < 0, ex + N, ex).tolist()))
    rowptr, ids, shared = [0], [], []
    for u in np.asarray(sources, dtype=np.int64).reshape(-1).tolist():
        u = u + N if u < 0 else u
        assert 0 <= u < N
        n = {}
        for j in range(bands):
            for v in bucket[j].get(u, ()):
                n[v] = n.get(v, 0) + 1
        row = sorted(v for v, k in n.items() if v != u and k >= min_bands and (u, v) not in gone)
        ids += row
        shared += [n[v] for v in row]
        rowptr.append(len(ids))
    return (np.array(rowptr, dtype=np.int64), np.array(ids, dtype=np.int64), np.array(shared, dtype=np.int32)), skipped


def bucket_sizes(N, bands, groups, sources):
    """the sizes of the planted buckets (two members or more) the sources sit in, over all bands"""
    src = set(int(u) % N for u in np.asarray(sources).reshape(-1))
    return set(len(members) for members, band_set in groups if band_set and src & set(members))


def nontrivial(rowptr, N):
    """at least half the sources have a candidate, none has all N - 1"""
    sizes = np.diff(rowptr)
    return bool(len(sizes) and np.mean(sizes > 0) >= 0.5 and sizes.max() < N - 1)


# ---- the sort key -----------------------------------------------------------------------------------------------------------------
def band_keys(table, rows, bands=None, key_bits=64):
    """int64 [b, N]: band_key of csrc/ss_lsh.hip for every band and node, in node order (the uint64 mix kept to its low key_bits bits
    and reinterpreted as the int64 the index sorts by)"""
    t = np.asarray(table).astype(np.uint64)
    N, P = t.shape
    b = resolve_bands(P, rows, bands)
    out = np.empty((b, N), dtype=np.uint64)
    for j in range(b):
        k = np.full(N, rows, dtype=np.uint64)
        for i in range(rows):
            k = mix64(k ^ t[:, j * rows + i]) + np.uint64(GOLDEN)
        out[j] = k
    if key_bits < 64:
        out &= np.uint64((1 << key_bits) - 1)
    return out.view(np.int64)


def key_run_lengths(keys):
    """int64 [b, N]: how many nodes of the band carry node v's key -- the length of the range the walk finds for v"""
    out = np.empty(keys.shape, dtype=np.int64)
    for j in range(keys.shape[0]):
        _, inv, counts = np.unique(keys[j], return_inverse=True, return_counts=True)
        out[j] = counts[inv.reshape(-1)]
    return out


def candidates_under_keys(table, sources, rows, bands, max_bucket, key_bits):
    """the restatement for a SHORT key (lsh.py's module text: the key finds the range to verify, and max_bucket applies to that
    range): membership by exact slice equality as lsh_restatement decides it, a band of a source dropped when more than max_bucket
    nodes carry the source's key.  -> ((rowptr, ids, bands), skipped int64 [b]: the key ranges of more than max_bucket nodes)"""
    mh = np.asarray(table)
    N, P = mh.shape
    b = resolve_bands(P, rows, bands)
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    src = np.where(src < 0, src + N, src)
    keys = band_keys(mh, rows, b, key_bits)
    runs = key_run_lengths(keys)
    shared = np.zeros((len(src), N), dtype=np.int32)
    for j, (group, _) in enumerate(restated.band_groups(mh, rows, b)):
        shared += (group[None, :] == group[src][:, None]) & (runs[j][src] <= max_bucket)[:, None]
    ok = shared >= 1
    ok[np.arange(len(src)), src] = False
    rowptr = np.zeros(len(src) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(ok.sum(axis=1))
    s_of, ids = np.nonzero(ok)
    skipped = np.array([int((np.unique(keys[j], return_counts=True)[1] > max_bucket).sum()) for j in range(b)], dtype=np.int64)
    return (rowptr, ids.astype(np.int64), shared[s_of, ids].astype(np.int32)), skipped


# ---- the plans ------------------------------------------------------------------------------------------------------------------
def _dedupe(xs):
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(int(x))
    return out


def _chunks(xs, sizes):
    out, at, i = [], 0, 0
    while len(xs) - at >= 2:
        out.append(xs[at:at + sizes[i % len(sizes)]])
        at += sizes[i % len(sizes)]
        i += 1
    return [c for c in out if len(c) >= 2]


# a. tile geometry: (P, rows, bands) of the keys kernel; each runs at N in {T, T + 1, 2 T - 1, 3 T + 5}, T = tile_rows(P)
TILE_CASES = [(4, 1, None), (4, 4, 1), (4, 1, 3), (12, 1, 5), (12, 5, 2), (64, 8, None), (192, 2, None), (192, 16, 12), (512, 4, None),
              (1024, 1, 7), (2048, 4, None), (2048, 2048, 1)]


def tile_sizes(P):
    T = tile_rows(P)
    return [T, T + 1, 2 * T - 1, 3 * T + 5]


def tile_plan(P, rows, bands, N):
    """(groups, sources): groups over rows 0 and N - 1, both sides of every tile boundary k T - 1 | k T and scattered rows -- one
    family in the lower half of the bands (band 0 among them), a second over the same rows shifted by one in the upper half (the last
    band among them), so that pairs share between one and many bands; sources = the members, half as many background rows, -1, -N"""
    b, T = resolve_bands(P, rows, bands), tile_rows(P)
    rng = np.random.RandomState((P * 131 + rows * 17 + b) * 1000 + N)
    lower, upper = list(range((b + 1) // 2)), list(range((b + 1) // 2, b))

    def some(of, forced):
        k = rng.randint(1, min(len(of), 6) + 1)
        return sorted(set([forced]) | set(int(x) for x in rng.choice(of, size=k, replace=False)))

    if N < 8:
        # (T = 4 only) N = T: one tile; N = T + 1: rows T - 1 | T = N - 1 in the first group; else T - 1 | T are the second group
        first, second = ([[0, N - 1]], []) if N <= T else ([[0, N - 1, T - 1]], [[1, 2]]) if N == T + 1 else ([[0, N - 1]], [[T - 1, T]])
        if not upper:  # one band: both groups in it
            first, second = first + second, []
        sources = list(range(N)) + [-1, -N]
    else:
        bounds = [k * T for k in range(1, N // T + 1) if k * T < N]
        scattered = [int(x) for x in rng.permutation(N)]
        pool = _dedupe([0, N - 1] + [x for k in bounds for x in (k - 1, k)] + scattered)[:min(24, 2 * N // 3)]
        first, second = _chunks(pool, [2, 3, 2, 4, 5]), _chunks(pool[1:], [3, 2, 4, 2])
        near = [x for k in bounds for x in (k - 2, k + 1) if 0 <= x < N]
        background = [v for v in _dedupe([1, N - 2] + near + scattered) if v not in pool][:len(pool) // 2]
        sources = pool + background + [-1, -N]
    groups = [(c, some(lower, lower[0] if i == 0 else lower[i % len(lower)])) for i, c in enumerate(first)]
    if upper:
        groups += [(c, some(upper, upper[-1 - i % len(upper)])) for i, c in enumerate(second)]
    return groups, np.array(sources, dtype=np.int64)


# b. round boundaries: P = 128, rows = 4, b = 32
ROUND_P, ROUND_ROWS, ROUND_N = 128, 4, 601
ROUND_SIZES = [2, 15, 16, 17, 31, 32, 33, 48, 49]


def round_plan():
    """(groups, by_size {m: (members, band)}): a group of every size in ROUND_SIZES, group i alone in band i; one group of three in
    all 32 bands; four nodes a, b, c, d that share 5 / 3 / 4 / 1 / 1 bands pairwise.  Rows 0, N - 1 and both sides of the tile
    boundaries 63 | 64 and 127 | 128 are members; the leaders are not the smallest ids"""
    N = ROUND_N
    pool = _dedupe([0, N - 1, 63, 64, 127, 128] + [int(x) for x in np.random.RandomState(5).permutation(N)])
    groups, by_size, at = [], {}, 0
    for i, m in enumerate(ROUND_SIZES):
        members = pool[at:at + m][::-1]
        groups.append((members, [i]))
        by_size[m] = (members, i)
        at += m
    groups.append((pool[at:at + 3], list(range(32))))
    a, b, c, d = pool[at + 3:at + 7]
    groups += [([a, b, c], [9, 10, 11]), ([b, a], [12, 13]), ([c, b, d], [14])]
    return groups, by_size


def round_near(groups):
    """three rows per group that miss its bucket by one word: the last word of the band, the first, one in the middle"""
    planted = set(v for members, _ in groups for v in members)
    free = [v for v in range(400, ROUND_N) if v not in planted]
    return [(free[3 * i + k], members[0], band_set[-1], w) for i, (members, band_set) in enumerate(groups)
            for k, w in enumerate((ROUND_ROWS - 1, 0, 1))]


def round_sources(groups):
    """first, middle and last member of every group by id, twenty background rows, and -1 / -N"""
    planted = set(v for members, _ in groups for v in members)
    picks = [x for members, _ in groups for x in (lambda s: (s[0], s[len(s) // 2], s[-1]))(sorted(members))]
    background = [v for v in [1, 62, 65, 126, 129, ROUND_N - 2] + list(range(200, 260)) if v not in planted][:20]
    return np.array(_dedupe(picks + background) + [-1, -ROUND_N], dtype=np.int64)


SIX_BIT_MAX_BUCKET = 26   # with 64 keys for 601 nodes a key range holds 9.4 nodes on average, plus a planted group


def six_bit_sources(groups):
    """every member of the groups of at most 17, ten background rows, -1: under a 6-bit key the larger groups' ranges are all dropped"""
    planted = set(v for members, _ in groups for v in members)
    small = [v for members, _ in groups if len(members) <= 17 for v in members]
    return np.array(_dedupe(small + [v for v in range(300, 340) if v not in planted][:10]) + [-1], dtype=np.int64)


# c. partly filled wavefronts: P = 128, rows = 4, bands in {1, 3, 5}
WAVE_P, WAVE_ROWS, WAVE_N = 128, 4, 101
WAVE_BANDS = [1, 3, 5]


def wave_plan(b):
    """(groups cut to the first b bands, good sources): most good sources have partners in band 0, the only band at b = 1"""
    full = [([3, 50, 100, 7], [0, 1, 2, 3, 4]), ([0, 9, 64], [0, 2]), ([63, 11], [1, 4]), ([20, 21, 22, 23, 24], [0, 3]),
            ([30, 31], [0]), ([40, 99, 41], [0, 1]), ([9, 30, 70], [4])]
    groups = [(m, [j for j in J if j < b]) for m, J in full]
    groups = [(m, J) for m, J in groups if J]
    good = [3, 0, 100, 63, 20, 50, 9, 30, 99, 24, 5, 7, 64, 40, 2, 11, 98, 41, 22, 1]
    return groups, good


# d. more than 4 GiB: P = 128, N = 2^23 + 2^18 rows of 512 bytes; row 2^22 starts at byte 2^31, row 2^23 at byte 2^32
LARGE_P, LARGE_ROWS, LARGE_BANDS, LARGE_N = 128, 2, 4, 8650752
LARGE_BOUNDS = (1 << 22, 1 << 23)


def large_plan():
    """(groups, sources): a dozen groups whose members straddle rows 2^22 and 2^23 and reach N - 1 and 0; sources = every member,
    background rows on both sides of each boundary and at both ends, and -1"""
    N, (B1, B2) = LARGE_N, LARGE_BOUNDS
    rng = np.random.RandomState(41)
    groups = [([B1 - 1, B1], [0]),
              ([B1, B2, 5], [1]),
              ([B2 - 1, B2], [2]),
              ([N - 1, 0, B2 + 1], [3]),
              ([B1 - 2, B1 + 1, B2 - 2, B2 + 1, N - 2], [0, 1, 2]),
              ([B1 - 3 - i for i in range(9)] + [B1 + 2 + i for i in range(8)], [2, 3]),        # 17 members: two rounds of the walk
              ([B2 + 2 + i for i in range(17)] + [B2 - 3 - i for i in range(16)], [0]),        # 33 members: three rounds
              ([N - 1, N - 3, B2 + 100], [0]),
              ([1, B1 + 1000, B2 + 1000, N - 5], [1, 2]),
              ([B1, B1 - 1], [3]),
              ([N - 1, B2 + 3], [2])]
    used = set(v for members, _ in groups for v in members)
    scattered = [int(x) for x in rng.randint(0, N, size=40) if int(x) not in used]
    groups.append((_dedupe(scattered)[:16], [1]))
    members = _dedupe(v for m, _ in groups for v in m)
    background = [v for v in (2, B1 - 100, B1 + 100, B2 - 100, B2 + 100, N - 100, B1 - 40, B2 + 40) if v not in members]
    return groups, np.array(members + background + [-1], dtype=np.int64)
