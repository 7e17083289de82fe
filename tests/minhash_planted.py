"""Planted permutation parameters for the two-phase MinHash first hop (csrc/ss_walks.hpp first_hop_minhash_fast, MinhashRows::row)
and its restatement in Python integers: shared by test_minhash_planted_host.py and test_minhash_planted_gpu.py.  Nothing here touches
the engine's kernels, and nothing here uses numpy arithmetic on hashes (no silent wrap-around): numpy only carries finished tables.

The permuted hash of node id under (a, b) is value = ((a * h + b) mod 2^64 mod (2^61 - 1)) mod 2^32, h = splitmix64(id + 1).  The
first hop does not evaluate it per (entry, permutation): phase 1 ranks a row's entries by key = ((lo32(x) + 8) & ~63) | slot, phase 2
evaluates the entry with the smallest key, and three documented rules send a row back to the exact walk:
  R0  the smallest key is in bucket 0 (the low word may wrap);
  R1  the two smallest keys are in the same or adjacent 64-wide buckets (order inside a bucket is by slot, x >> 61 adds up to 7);
  R2  bits 32..60 of the winner's x are all ones (MinhashRows only: lo32(x) + (x >> 61) may miss the - (2^61 - 1)).
With the engine's one parameter set they fire by chance, a few times per million (row, permutation).  Here (a_q, b_q) are SOLVED for:
x = a * h + b is linear, so two chosen entries of a chosen row can be put on any two 64-bit targets per permutation (`plant`), with
a and b inside the reference's own range 1 <= a < 2^61 - 1, 0 <= b < 2^61 - 1.  `two_phase` says what the shortcut would answer with
its flags ignored and which rules the header comments raise: it proves that a planted case discriminates, it is never the expected
output -- that is `want_row`, the plain minimum.

Slot layouts (ss_walks.hpp): MinhashRows<_, R> takes chunks of R consecutive rows (first row a multiple of R); their col entries form
one list cut into batches of 64 - R, an entry at chunk position t has slot t % (64 - R), and row r's own id sits in slot 64 - R + r;
first_hop_minhash_fast takes plain batches of 64 entries of one row, the own id in slot `deg`, and wavefront w of W walks the batches
w, w + W, ... (W = 16 in the hub walk, each wavefront judged on its share alone)."""
import functools
import random
from types import SimpleNamespace

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
M61 = (1 << 61) - 1      # the Mersenne prime, also the mask of bits 0..60
MID_ONES = (1 << 29) - 1  # bits 32..60 of x, all set
DRAW_CAP = 100000
R0, R1, R2 = 'R0', 'R1', 'R2'

_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_C1_INV, _C2_INV = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)


# ---- the hash and its inverse -------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x &= M64
    x ^= x >> 30
    x = x * _C1 & M64
    x ^= x >> 27
    x = x * _C2 & M64
    x ^= x >> 31
    return x


def _unxorshift(y, s):
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def inverse_splitmix64(h):
    x = _unxorshift(h & M64, 31)
    x = x * _C2_INV & M64
    x = _unxorshift(x, 27)
    x = x * _C1_INV & M64
    return _unxorshift(x, 30)


def node_hash(node):
    return splitmix64(node + 1)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def x_of(a, b, h):
    return (a * h + b) & M64


def value_of_x(x):
    return (x % M61) & M32


def shortcut_of_x(x):
    """lo32(x) + (x >> 61) without the reduction: what MinhashRows evaluates for the winner (right unless R2 says otherwise)"""
    return ((x & M32) + (x >> 61)) & M32


def make_x(lo32, top=0, mid=0):
    assert 0 <= lo32 <= M32 and 0 <= top <= 7 and 0 <= mid <= MID_ONES
    return (top << 61) | (mid << 32) | lo32


def parts_of_x(x, h=None):
    xp = ((x & M32) + 8) & M32
    return SimpleNamespace(h=h, x=x, value=value_of_x(x), lo32=x & M32, xp=xp, bucket=xp >> 6, top=x >> 61, mid=(x >> 32) & MID_ONES)


def parts(a, b, node):
    h = node_hash(node)
    return parts_of_x(x_of(a, b, h), h)


def want_row(entries, a, b):
    """the element-wise minimum of value over a row's entries (in-neighbours in CSR order, then the own id where the node has the
    inferred self loop); no entry at all: the all-zero row"""
    if not entries:
        return [0] * len(a)
    hs = [node_hash(e) for e in entries]
    return [min(value_of_x(x_of(aq, bq, h)) for h in hs) for aq, bq in zip(a, b)]


def _two_phase_x(xs, slots):
    """one permutation, one wavefront's share: (value, flags, winner x) from the x of its entries in walk order"""
    m1 = m2 = M32
    win = None
    for x, s in zip(xs, slots):
        key = ((((x & M32) + 8) & M32) & ~63) | s
        if key < m1:
            m1, m2, win = key, m1, x
        elif key < m2:
            m2 = key
        if win is None:  # (a first key of 0xFFFFFFFF: the only entry so far)
            win = x
    flags = set()
    if m1 < 64:
        flags.add(R0)
    if (m2 >> 6) - (m1 >> 6) <= 1:
        flags.add(R1)
    if (win >> 32) & MID_ONES == MID_ONES:
        flags.add(R2)
    return value_of_x(win), flags, win


def two_phase(entries, slots, a, b):
    """per permutation what the shortcut answers with its flags ignored -- the entry with the smallest key ((lo32(x) + 8) & ~63) | slot,
    the first one walked among equals, evaluated exactly -- and the set of rules (R0, R1, R2) the documented conditions raise.
    entries / slots: one wavefront's share in walk order.  -> [SimpleNamespace(value, flags, x)]"""
    hs = [node_hash(e) for e in entries]
    out = []
    for aq, bq in zip(a, b):
        v, f, w = _two_phase_x([x_of(aq, bq, h) for h in hs], slots)
        out.append(SimpleNamespace(value=v, flags=f, x=w))
    return out


def plain_shares(n_entries, waves=1):
    """first_hop_minhash_fast: [(positions, slots)] per wavefront that has a batch, entry t in batch t // 64 at slot t % 64"""
    shares = []
    for w in range(waves):
        pos = [t for t in range(n_entries) if (t // 64) % waves == w]
        if pos:
            shares.append((pos, [t % 64 for t in pos]))
    return shares


def rows_share(p0, deg, r, R, own=True):
    """MinhashRows<_, R>: (positions, slots) of row r of its chunk, whose col entries start at chunk position p0; the own id is
    position `deg`"""
    kNb = 64 - R
    pos = list(range(deg)) + ([deg] if own else [])
    return pos, [(p0 + t) % kNb for t in range(deg)] + ([kNb + r] if own else [])


# ---- the solver ---------------------------------------------------------------------------------------------------------------------
def solve(h0, X0, h1=None, X1=None, rng=None):
    """one attempt: (a, b) with a * h0 + b = X0 (and a * h1 + b = X1) mod 2^64, or None when it leaves the reference's range"""
    if h1 is None:
        a = rng.randrange(1, M61)
    else:
        d = (h0 - h1) & M64
        assert d & 1, 'pick entry pairs whose hash difference is odd'
        a = (X0 - X1) * pow(d, -1, 1 << 64) & M64
    b = (X0 - a * h0) & M64
    return (a, b) if (1 <= a < M61 and b < M61) else None


def plant(h0, X0, h1=None, X1=None, rng=None, accept=None):
    """(a, b) in range that puts the entry with hash h0 on X0 (and the one with hash h1 on X1).  A target is an int or a function
    rng -> int that redraws its free bits (bucket number, mid, ...); accept(a, b) may refuse a solution (another draw follows).
    -> (a, b, X0, X1, draws); raises beyond DRAW_CAP draws"""
    rng = rng or random.Random(0)
    for draw in range(1, DRAW_CAP + 1):
        x0 = X0(rng) if callable(X0) else X0
        x1 = X1(rng) if callable(X1) else X1
        ab = solve(h0, x0, h1, x1, rng)
        if ab is None or (accept is not None and not accept(*ab)):
            continue
        a, b = ab
        assert x_of(a, b, h0) == x0 and (h1 is None or x_of(a, b, h1) == x1)
        return a, b, x0, x1, draw
    raise RuntimeError(f'no parameters in range after {DRAW_CAP} draws')


# ---- targets ------------------------------------------------------------------------------------------------------------------------
def _mid(rng):
    return rng.randrange(0, MID_ONES)  # (never all ones)


def at_bucket(bucket, off, top, mid):
    """x whose x' = lo32 + 8 is word `off` of bucket `bucket` (no wrap: bucket >= 1 or off >= 8)"""
    xp = bucket * 64 + off
    assert 8 <= xp <= M32
    return make_x(xp - 8, top, mid)


def mid_range(rng):
    return at_bucket(rng.randrange(1 << 20, 1 << 25), rng.randrange(64), rng.randrange(8), _mid(rng))


TOP_BUCKET = M32 >> 6

# SHORT_VARIANTS[q % 19] is planted by permutation q; REQUIRED: the rules its row must raise there; EXACT_FLAGS: and no other
SHORT_VARIANTS = ('S1', 'S2', 'S3', 'S3m', 'S4', 'S4m', 'S5', 'S6', 'S7', 'S8m1', 'S8m', 'S8p1', 'S8p7', 'S8zero', 'S8ones', 'S9',
                  'S10top', 'S10second', 'S10third')
ONE_ENTRY = ('S10top', 'S10second', 'S10third')
REQUIRED = {'S1': {R1}, 'S2': {R1}, 'S3': {R1}, 'S3m': {R1}, 'S4': set(), 'S4m': set(), 'S5': {R0}, 'S6': {R0}, 'S7': {R0}, 'S8m1': set(),
            'S8m': {R0, R2}, 'S8p1': {R0, R2}, 'S8p7': {R0, R2}, 'S8zero': {R0}, 'S8ones': {R0, R2}, 'S9': {R2}, 'S10top': {R1},
            'S10second': {R1}, 'S10third': set()}
EXACT_FLAGS = ('S1', 'S2', 'S3', 'S3m', 'S4', 'S4m', 'S5', 'S6', 'S7', 'S9', 'S10top', 'S10second', 'S10third')
S8_VALUES = {'S8m1': 0xFFFFFFFE, 'S8m': 0, 'S8p1': 1, 'S8p7': 7, 'S8zero': 0, 'S8ones': 7}
S8_SUMS = {'S8m1': (1 << 32) - 2, 'S8m': (1 << 32) - 1, 'S8p1': 1 << 32, 'S8p7': (1 << 32) + 6}


def s8_target(name, rng, top=None):
    """mid all ones with lo32 + top on the wanted sum (r = M - 1, M, M + 1, M + 7), x = 0, or x = 2^64 - 1"""
    if name == 'S8zero':
        return 0
    if name == 'S8ones':
        return M64
    total = S8_SUMS[name]
    tops = [t for t in range(8) if 0 <= total - t <= M32]
    top = tops[rng.randrange(len(tops))] if top is None else top
    return make_x(total - top, top, MID_ONES)


def short_targets(name, rng, swap):
    """(X of e0 -- the neighbour, lower slot --, X of e1 -- the own id) of a two-entry scenario; swap: the single planted entry of
    S5 .. S9 is e1 instead of e0"""
    k = rng.randrange(1 << 12, 1 << 25)
    if name == 'S1':    # same bucket, value(e0) < value(e1)
        return at_bucket(k, 10, 0, _mid(rng)), at_bucket(k, 50, 0, _mid(rng))
    if name == 'S2':    # same bucket, value(e0) > value(e1): phase 1 picks the wrong entry
        return at_bucket(k, 50, 0, _mid(rng)), at_bucket(k, 10, 0, _mid(rng))
    if name == 'S3':    # adjacent buckets: e0 on the last word of bucket k with top 7, e1 on the first word of bucket k + 1 with top 0
        return at_bucket(k, 63, 7, _mid(rng)), at_bucket(k + 1, 0, 0, _mid(rng))
    if name == 'S3m':
        return at_bucket(k + 1, 0, 0, _mid(rng)), at_bucket(k, 63, 7, _mid(rng))
    if name == 'S4':    # buckets k and k + 2, the same offsets and tops: just outside R1
        return at_bucket(k, 63, 7, _mid(rng)), at_bucket(k + 2, 0, 0, _mid(rng))
    if name == 'S4m':
        return at_bucket(k + 2, 0, 0, _mid(rng)), at_bucket(k, 63, 7, _mid(rng))
    if name == 'S5':    # wrap without carry: the smallest key and the largest value
        x = make_x(rng.randrange((1 << 32) - 8, 1 << 32), 0, _mid(rng))
    elif name == 'S6':  # wrap with carry: value 6
        x = make_x(M32, 7, _mid(rng))
    elif name == 'S7':  # bucket 0 without wrap
        x = make_x(rng.randrange(0, 56), rng.randrange(8), _mid(rng))
    elif name in S8_VALUES:
        x = s8_target(name, rng)
    elif name == 'S9':  # mid all ones on the key winner, nothing else
        x = at_bucket(rng.randrange(1 << 12, 1 << 19), rng.randrange(64), rng.randrange(8), MID_ONES)
    else:
        raise KeyError(name)
    other = mid_range(rng)
    return (other, x) if swap else (x, other)


def one_entry_target(name, rng):
    bucket = TOP_BUCKET - ('S10top', 'S10second', 'S10third').index(name)
    return at_bucket(bucket, rng.randrange(64), rng.randrange(8), _mid(rng))


# ---- the graph ----------------------------------------------------------------------------------------------------------------------
N = 1600
SHORT_FIRST = 1104          # two-entry rows SHORT_FIRST + q
LONG = {'L61': 1400, 'L130': 1408, 'L130S': 1416, 'L210': 1424, 'L1100': 1432}  # (each the first row of a chunk of 8, and so of 4)
OWN = -1                    # a case position: the row's own id (the implicit self loop)
# (row, position of A, position of B) in the row's col entries; see the module docstring of test_minhash_planted_gpu.py
LONG_CASES = (('L61', 3, 40),        # both in one batch, in every layout
              ('L61', 11, OWN),      # B is the own id, after the second batch
              ('L130', 7, 127),      # batches 0 and 2 at R = 4 (60 per batch) with equal slots: identical keys in the same-bucket set
              ('L130', 6, 118),      # ... at R = 8 (56 per batch)
              ('L130', 8, 72),       # ... in plain batches of 64 (update_hash_tables)
              ('L130S', 64, 101),    # A is the row's explicit entry for itself (the implicit self loop is left out)
              ('L210', 18, 150),     # different batches; different wavefronts in the hub walk
              ('L210', OWN, 71),     # A is the own id
              ('L1100', 9, 1033),    # batches 0 and 16: one wavefront of the hub walk, equal slots
              ('L1100', 1000, 29))
RULES = ('clean', 'same', 'adjacent', 'bucket0')
LONG_REQUIRED = {'clean': set(), 'same': {R1}, 'adjacent': {R1}, 'bucket0': {R0}}


@functools.lru_cache(maxsize=None)
def hashes():
    return [node_hash(i) for i in range(N)]


@functools.lru_cache(maxsize=None)
def graph():
    """-> SimpleNamespace(n, edge_index int64 [2, E], entries {row: [ids]} (want_row's), col {row: [ids]}, short [(variant, s, t)],
    long {name: row}).  Every node has the inferred self loop (the last id is a source)."""
    H = hashes()
    one_entry_pool = iter(400 + 8 * j + (7 if j % 2 == 0 else 3) for j in range(40))  # (every other one the last row of its chunk)
    reserved = {400 + 8 * j + (7 if j % 2 == 0 else 3) for j in range(40)}
    t_pool = [i for i in list(range(0, 400)) + list(range(700, 1100)) if i not in reserved]
    used, short, col = set(), [], {}
    for q in range(256):
        name = SHORT_VARIANTS[q % len(SHORT_VARIANTS)]
        if name in ONE_ENTRY:
            short.append((name, next(one_entry_pool), None))
            continue
        s = SHORT_FIRST + q
        t = next(i for i in t_pool if i not in used and (H[i] - H[s]) & 1)
        used.add(t)
        short.append((name, s, t))
        col[s] = [t]
    col[LONG['L61']] = list(range(0, 61))
    col[LONG['L130']] = list(range(100, 230))
    col[LONG['L130S']] = list(range(230, 294)) + [LONG['L130S']] + list(range(294, 359))
    col[LONG['L210']] = list(range(400, 610))
    # A and B of a case belong to ONE long row (a permutation that plants them must leave the other long rows alone): the row of
    # 1 100 entries takes the ids that are nobody's A or B, and ids of its own at its four case positions
    taken = set(LONG.values()) | {N - 1, N - 2}
    special = {}
    for name, pa, pb in LONG_CASES:
        if name != 'L1100':
            taken |= {col[LONG[name]][t] for t in (pa, pb) if t != OWN}
        else:
            special[pa], special[pb] = None, None
    own_ids = iter(i for i in range(1440, 1590) if i not in taken)
    for name, pa, pb in LONG_CASES:
        if name == 'L1100':
            special[pa] = next(own_ids)
            special[pb] = next(i for i in own_ids if (H[i] - H[special[pa]]) & 1)
    taken |= set(special.values())
    pool = iter(i for i in range(N) if i not in taken)
    col[LONG['L1100']] = [special[t] if t in special else next(pool) for t in range(1100)]
    col[N - 2] = [N - 1]
    src = [u for i in sorted(col) for u in col[i]]
    dst = [i for i in sorted(col) for _ in col[i]]
    ei = np.array([src, dst], dtype=np.int64)
    assert int(ei.max()) == N - 1
    entries = {i: col.get(i, []) + [i] for i in range(N)}
    return SimpleNamespace(n=N, edge_index=ei, entries=entries, col=col, short=short, long=dict(LONG))


def case_entries(case):
    """(row, its col entries, position of A, position of B, the two node ids): OWN becomes position deg"""
    g = graph()
    name, pa, pb = case
    row = g.long[name]
    col = g.col[row]
    pa = len(col) if pa == OWN else pa
    pb = len(col) if pb == OWN else pb
    ids = col + [row]
    return row, col, pa, pb, (ids[pa], ids[pb])


def walked(row):
    """the entries the two-phase walk sees: a row that lists itself leaves its implicit self loop out"""
    col = graph().col.get(row, [])
    return col if row in col else col + [row]


def row_layouts(row):
    """{layout name: [(positions into walked(row), slots)] per wavefront}: MinhashRows at R = 8 and R = 4 (the row's col entries
    start where those of the rows before it in its chunk end), plain batches by one wavefront and by 16"""
    g = graph()
    w = walked(row)
    deg = len(g.col.get(row, []))
    own = len(w) > deg
    p0 = {R: sum(len(g.col.get(i, [])) for i in range(row - row % R, row)) for R in (8, 4)}
    return {'rows8': [rows_share(p0[8], deg, row % 8, 8, own)], 'rows4': [rows_share(p0[4], deg, row % 4, 4, own)],
            'plain1': plain_shares(len(w), 1), 'plain16': plain_shares(len(w), 16)}


def shortcut_row(row, a, b, layout):
    """what a layout answers with every flag ignored: per permutation (min over the wavefronts' two_phase values, union of flags)"""
    w = walked(row)
    per_share = [two_phase([w[t] for t in pos], slots, a, b) for pos, slots in row_layouts(row)[layout]]
    return [(min(s[q].value for s in per_share), set().union(*[s[q].flags for s in per_share])) for q in range(len(a))]


def _flags_x(xs, row):
    """per layout the union of flags of a row whose walked entries have these x (one permutation)"""
    out = {}
    for name, shares in row_layouts_cached(row).items():
        f = set()
        for pos, slots in shares:
            f |= _two_phase_x([xs[t] for t in pos], slots)[1]
        out[name] = f
    return out


@functools.lru_cache(maxsize=None)
def row_layouts_cached(row):
    return row_layouts(row)


# ---- the short-row parameter set ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_params():
    """-> SimpleNamespace(a [256], b [256], info [256]): permutation q plants scenario SHORT_VARIANTS[q % 19] on row s_q; every other
    permutation leaves that row unflagged (redrawn until the restatement says so, in every layout).  A parameter set for P < 256 is the
    first P of these."""
    g, H = graph(), hashes()
    rng = random.Random(20261)
    rows = [(s, [H[e] for e in walked(s)]) for _, s, _ in g.short]
    a, b, info = [], [], []
    for q, (name, s, t) in enumerate(g.short):
        occurrence = q // len(SHORT_VARIANTS)

        def accept(aq, bq):
            for q2, (s2, hs) in enumerate(rows):
                flags = _flags_x([x_of(aq, bq, h) for h in hs], s2)
                if q2 != q:
                    if any(flags.values()):
                        return False
                elif any(not (REQUIRED[name] <= f) or (name in EXACT_FLAGS and f != REQUIRED[name]) for f in flags.values()):
                    return False
            return True

        if t is None:
            aq, bq, x0, x1, draws = plant(H[s], lambda r: one_entry_target(name, r), rng=rng, accept=accept)
            targets = (x0,)
        else:
            swap = occurrence % 2 == 1
            pair = {}

            def first(r):
                pair['x'] = short_targets(name, r, swap)
                return pair['x'][0]

            aq, bq, x0, x1, draws = plant(H[t], first, H[s], lambda r: pair['x'][1], rng=rng, accept=accept)
            targets = (x0, x1)
        a.append(aq)
        b.append(bq)
        info.append(SimpleNamespace(q=q, name=name, row=s, neighbour=t, targets=targets, draws=draws,
                                    planted=None if t is None or name in ('S1', 'S2', 'S3', 'S3m', 'S4', 'S4m') else int(occurrence % 2 == 1)))
    return SimpleNamespace(a=a, b=b, info=info)


# ---- the long-row parameter sets ----------------------------------------------------------------------------------------------------
def long_targets(rule, rng, flip):
    """(X of A, X of B); flip: B takes the role A has otherwise"""
    k = rng.randrange(1, 255)
    if rule == 'clean':       # two buckets apart, the lower one wins by key and by value
        lo, hi = at_bucket(k, 63, 7, _mid(rng)), at_bucket(k + 2, 0, 0, _mid(rng))
    elif rule == 'same':      # one bucket: the order inside it is by slot
        lo, hi = at_bucket(k, 50, 0, _mid(rng)), at_bucket(k, 10, 0, _mid(rng))
    elif rule == 'adjacent':  # the lower key has the larger value
        lo, hi = at_bucket(k, 63, 7, _mid(rng)), at_bucket(k + 1, 0, 0, _mid(rng))
    elif rule == 'bucket0':   # a wrapped low word: the smallest key, the largest value
        lo, hi = make_x(rng.randrange((1 << 32) - 8, 1 << 32), 0, _mid(rng)), at_bucket(k + 2, rng.randrange(64), rng.randrange(8), _mid(rng))
    else:
        raise KeyError(rule)
    return (hi, lo) if flip else (lo, hi)


@functools.lru_cache(maxsize=None)
def long_params(rule, P=128):
    """-> SimpleNamespace(a [P], b [P], info [P]): permutation q plants `rule` on the entries A and B of LONG_CASES[q % 10]; the
    restatement confirms per layout that the planted row raises nothing but the rule's flag, every other long row nothing at all, and
    that A and B hold the row's two smallest buckets"""
    g, H = graph(), hashes()
    rng = random.Random(RULES.index(rule) + 77)
    long_rows = [(row, [H[e] for e in walked(row)]) for row in g.long.values()]
    a, b, info = [], [], []
    for q in range(P):
        case = LONG_CASES[q % len(LONG_CASES)]
        flip = (q // len(LONG_CASES)) % 2 == 1
        row, col, pa, pb, (ia, ib) = case_entries(case)
        w = walked(row)
        wa, wb = w.index(ia), w.index(ib)
        if not (H[ia] - H[ib]) & 1:
            raise AssertionError(f'case {case}: the hash difference of A and B is even, choose other positions')

        def accept(aq, bq):
            for row2, hs in long_rows:
                xs = [x_of(aq, bq, h) for h in hs]
                flags = _flags_x(xs, row2)
                if row2 != row:
                    if any(flags.values()):
                        return False
                    continue
                if any(not f <= LONG_REQUIRED[rule] for f in flags.values()):
                    return False
                buckets = sorted((parts_of_x(x).bucket, t) for t, x in enumerate(xs))
                if {buckets[0][1], buckets[1][1]} != {wa, wb} or buckets[2][0] - buckets[1][0] <= 1:
                    return False
            return True

        pair = {}

        def first(r):
            pair['x'] = long_targets(rule, r, flip)
            return pair['x'][0]

        aq, bq, x0, x1, draws = plant(H[ia], first, H[ib], lambda r: pair['x'][1], rng=rng, accept=accept)
        a.append(aq)
        b.append(bq)
        info.append(SimpleNamespace(q=q, case=case, row=row, flip=flip, A=ia, B=ib, targets=(x0, x1), draws=draws))
    return SimpleNamespace(a=a, b=b, info=info)


# ---- expected tables ----------------------------------------------------------------------------------------------------------------
def want_tables(n, edge_index, a, b, hops=2):
    """[hop-1 rows, hop-2 rows] as uint32 [n, P]: hop 1 by want_row over every row's entries (in-neighbours, then the own id below
    max(edge_index) + 1), hop 2 the min-fold of the hop-1 rows over the same entries (a finished table: numpy only takes minima)"""
    ei = np.asarray(edge_index)
    n_self = int(ei.max()) + 1 if ei.size else 0
    P = len(a)
    col = {}
    for u, i in zip(ei[0].tolist(), ei[1].tolist()):
        col.setdefault(i, []).append(u)
    H = {}
    vals = {}

    def value_row(node):
        if node not in vals:
            h = H.setdefault(node, node_hash(node))
            vals[node] = [value_of_x(x_of(aq, bq, h)) for aq, bq in zip(a, b)]
        return vals[node]

    hop1 = np.zeros((n, P), dtype=np.uint32)
    ent = {}
    for i in range(n):
        e = col.get(i, []) + ([i] if i < n_self else [])
        ent[i] = e
        if e:
            hop1[i] = np.array([value_row(u) for u in e], dtype=np.uint32).min(axis=0)
    out = [hop1]
    for _ in range(hops - 1):
        prev, nxt = out[-1], np.zeros((n, P), dtype=np.uint32)
        for i in range(n):
            if ent[i]:
                nxt[i] = prev[ent[i]].min(axis=0)
        out.append(nxt)
    return out


def as_u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


# ---- hop 0 on planted hashes (ss_minhash_init / ss_hll_init with first_node = inverse_splitmix64(hv) - 1) --------------------------------
PRE_MAX = (1 << 63) - 4  # (n <= 3 rows: first_node + 3 stays an int64)


def preimage_ok(hv):
    return 1 <= inverse_splitmix64(hv) <= PRE_MAX


def hll_rank(hv, p):
    return (64 - p) - (hv >> p).bit_length() + 1


def hll_row(hv, p):
    row = [0] * (1 << p)
    row[hv & ((1 << p) - 1)] = hll_rank(hv, p)
    return row


def hll_hashes(p):
    """{case name: hv} with a usable preimage: hv >> p == 0 (the top rank 64 - p + 1) and == 1, the top bit set (rank 1), register 0
    and m - 1, and each of the 16 byte positions of a 16-byte chunk"""
    rng = random.Random(p)
    m = 1 << p
    out = {}

    def search(name, make):
        for _ in range(DRAW_CAP):
            hv = make()
            if preimage_ok(hv):
                out[name] = hv
                return
        raise RuntimeError(f'no preimage in range for {name} at p = {p}')

    search('top_rank', lambda: rng.randrange(1, m))                       # hv >> p == 0 (hv = 0 has the preimage 0: node id -1)
    search('second_rank', lambda: (1 << p) | rng.randrange(m))            # hv >> p == 1
    search('rank_one', lambda: (1 << 63) | rng.getrandbits(63))
    search('register_0', lambda: rng.getrandbits(64) & ~(m - 1))
    search('register_last', lambda: rng.getrandbits(64) | (m - 1))
    for byte in range(16):
        search(f'byte_{byte}', lambda: (rng.getrandbits(64) & ~15) | byte)
    return out


def minhash_init_params(P, seed=5):
    """-> (hv, a [P], b [P], names [P]): one node hash with a usable preimage and, cycling over the permutations, the S8 targets
    planted on it"""
    rng = random.Random(seed * 4099 + P)
    names = sorted(S8_VALUES)
    while True:
        hv = rng.getrandbits(64) | 1
        if preimage_ok(hv) and preimage_ok(splitmix64(inverse_splitmix64(hv) + 1)):
            break
    a, b, used = [], [], []
    for q in range(P):
        name = names[q % len(names)]
        aq, bq, _, _, _ = plant(hv, lambda r: s8_target(name, r), rng=rng)
        a.append(aq)
        b.append(bq)
        used.append(name)
    return hv, a, b, used
