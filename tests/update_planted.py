"""A planted graph for the marking kernels of update_hash_tables (update_seed_kernel, update_mark_kernel of csrc/ss_update.hip), pure
numpy: tests/test_update_planted_gpu.py runs it through the C ABI, tests/test_update_host.py pins its closed form on the restatement.

update_mark_kernel<false> walks the in-edges of a row in one of three ways: up to 32 by the row's own lane, 33 .. 2 048 by its wavefront
(64 per step, one pending row of the wavefront after another), more by the whole workgroup (4 x 256 per step, slots past the end
clamped to the last in-edge, early exit through LDS, the rows of one 256-row block in turn).  The graph has one target row per
in-degree of DEGREES -- each tier's ends, and one below / at / one above every step boundary of the two cooperative tiers:

  ids 0 .. D - 1          sources: no in-edge (only their implicit self loop)
  row r_d                 one directed in-edge from each of the sources 0 .. d - 1
  solo and wave tiers     adjacent ids from D on: the nine wave-tier rows are pending in ONE wavefront
  workgroup tier          four rows in the 256-id block BLOCK_A, at its first id, two adjacent ones inside, its last id; the other
                          seven in the next block (the last of them at that block's last id, which is the largest endpoint)
  TRAILING ids            above the largest endpoint: no edge, no self loop (i >= n_self)

With source s as the only seed: dirty_1 = {s}, dirty_2 = {s} + {r_d : d > s} (s has its self loop, and is in-neighbour number s of
every row that is long enough) -- one dirty in-neighbour per row, at the slot the CSR builder gave s in that row; s = 0 .. D - 1 puts
it at every slot of every row."""
import numpy as np

D = 5200
TRAILING = 300
SOLO_MAX, WAVE_MAX = 32, 2048          # kMarkSolo, kMarkWave
DEGREES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 2303, 2304, 2305, 3071, 3072, 3073, 4095, 4096, 4097, 5121)
BLOCK_A = (D + len(DEGREES) + 255) // 256   # the first 256-id block wholly above the sources and the short rows
_A0, _B0 = 256 * BLOCK_A, 256 * (BLOCK_A + 1)
_BIG_IDS = {2049: _A0, 4097: _A0 + 124, 2304: _A0 + 125, 5121: _A0 + 255,
            2303: _B0 + 8, 2305: _B0 + 9, 3071: _B0 + 68, 3072: _B0 + 118, 3073: _B0 + 168, 4095: _B0 + 169, 4096: _B0 + 255}


def tier(d):
    return 'solo' if d <= SOLO_MAX else 'wave' if d <= WAVE_MAX else 'workgroup'


def row_of_degree():
    """{d: id of r_d}"""
    rows, nxt = {}, D
    for d in DEGREES:
        if tier(d) == 'workgroup':
            rows[d] = _BIG_IDS[d]
        else:
            rows[d] = nxt
            nxt += 1
    return rows


def plan():
    """-> dict(n, n_self, edge_index int64 [2, E], rows {d: id}, deg int64 [n] (planted in-degrees))"""
    rows = row_of_degree()
    src = np.concatenate([np.arange(d, dtype=np.int64) for d in DEGREES])
    dst = np.concatenate([np.full(d, rows[d], dtype=np.int64) for d in DEGREES])
    # (shuffled: the row order the CSR builder leaves is its own business, the test reads it back)
    order = np.random.RandomState(66).permutation(src.size)
    ei = np.stack([src[order], dst[order]])
    n_self = int(ei.max()) + 1
    n = n_self + TRAILING
    deg = np.zeros(n, dtype=np.int64)
    for d, r in rows.items():
        deg[r] = d
    assert n_self == max(rows.values()) + 1 and len(set(rows.values())) == len(DEGREES) and min(rows.values()) >= D
    assert np.array_equal(np.bincount(ei[1], minlength=n), deg)
    wave_rows = [rows[d] for d in DEGREES if tier(d) == 'wave']
    assert wave_rows == list(range(wave_rows[0], wave_rows[0] + len(wave_rows))) and wave_rows[0] // 64 == wave_rows[-1] // 64
    blocks = [rows[d] // 256 for d in DEGREES if tier(d) == 'workgroup']
    assert blocks.count(BLOCK_A) >= 3 and blocks.count(BLOCK_A + 1) >= 3 and _A0 in rows.values() and _A0 + 255 in rows.values()
    return dict(n=n, n_self=n_self, edge_index=ei, rows=rows, deg=deg)


def had_loop_cards(n, n_self, stride=1):
    """cards_old [n, stride] whose column 0 says "every row below n_self had its self loop, no other row": no self-loop seed; the
    other columns say the opposite, so that a kernel that reads another column is caught"""
    cards = np.zeros((n, stride), dtype=np.float32)
    cards[:n_self, 0] = 1.0
    cards[n_self:, 1:] = 1.0
    return cards


def single_seed_dirty(pl, s):
    """the closed form for source s as the only seed -> {1: bool [n], 2: bool [n]}"""
    one = np.zeros(pl['n'], dtype=bool)
    one[s] = True
    return {1: one, 2: one | (pl['deg'] > s)}
