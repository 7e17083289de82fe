"""A planted multigraph for the graph_prep tests: built from a PLAN -- the output pairs in sorted order with the number of entries of
each -- so that every output pair and count is known before anything is computed, and placed so that the runs meet the places where the
mark / fill / reduce kernels branch.  `block` is the library's ss_coalesce_block() (sorted positions per workgroup of mark / fill),
`chunk` its ss_coalesce_chunk().

  rows      0-2 empty (start); row 4 empty (a gap of 1); rows 6-7 (a gap of 2); rows 9-108 (a gap of 100); rows 651 .. N - 1 (end)
  runs      1, 2, 3, chunk - 1, chunk, chunk + 1, 2 chunk - 1, 2 chunk, 2 chunk + 1 entries in row 3; 64 chunk + 1 entries in row 5
  workgroup a run of one entry AT the last position of workgroup 1 (sorted position 2 block - 1), the head of the 64 chunk + 1 run AT
            the first position of workgroup 2, and that run straddles every boundary up to its end
  self loops (8, 8) and (109, 109)
  the last run ends at E
The list is handed over shuffled (every run scattered over the whole list), ascending (sorted order) or descending."""
import numpy as np

N = 700


def plan(block, chunk):
    """[(row, col, entries)] in sorted order"""
    runs = [(3, k, n) for k, n in enumerate((1, 2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1))]
    used = sum(n for _, _, n in runs)
    filler = 2 * block - 1 - used
    assert filler > 0
    runs.append((3, 20, filler))                 # up to sorted position 2 block - 2
    runs.append((3, 21, 1))                      # a head at the LAST position of workgroup 1
    runs.append((5, 0, 64 * chunk + 1))          # a head at the FIRST position of workgroup 2; the run crosses the boundaries after it
    runs += [(8, 8, 2), (8, 9, 1), (8, 699, 5)]
    runs += [(109, 3, 300), (109, 109, 1), (109, 110, chunk)]
    runs += [(650, 0, 7), (650, 699, 3)]         # the last run ends at E
    return runs


def edges(block, chunk, order='shuffled', seed=0):
    """(row, col int64 [E], run_of int64 [E]: the plan entry every list position belongs to) in the order asked for"""
    runs = plan(block, chunk)
    lengths = np.array([n for _, _, n in runs])
    run_of = np.repeat(np.arange(len(runs)), lengths)
    row = np.repeat(np.array([r for r, _, _ in runs], dtype=np.int64), lengths)
    col = np.repeat(np.array([c for _, c, _ in runs], dtype=np.int64), lengths)
    E = len(row)
    if order == 'shuffled':
        p = np.random.RandomState(seed).permutation(E)
    elif order == 'ascending':
        p = np.arange(E)
    elif order == 'descending':
        p = np.arange(E)[::-1].copy()
    else:
        raise ValueError(order)
    return row[p], col[p], run_of[p]


def weights(E, kind, seed=1):
    """entry values whose merge shows what it should:
    fractional32 / fractional64: magnitudes over seven decades and both signs -- a sum depends on its order
    near2to62: int64 around 2^62 -- sums of two and more wrap
    small_int: int64 in [-9, 9]
    special32 / special64: -0.0, +0.0, 1, -1 and a NaN here and there -- the min / max rules"""
    rng = np.random.RandomState(seed)
    if kind in ('fractional32', 'fractional64'):
        w = rng.uniform(-1, 1, E) * 10.0 ** rng.randint(-3, 4, E)
        return w.astype(np.float32 if kind.endswith('32') else np.float64)
    if kind == 'near2to62':
        return ((1 << 62) - rng.randint(0, 1000, E)).astype(np.int64)
    if kind == 'small_int':
        return rng.randint(-9, 10, E).astype(np.int64)
    if kind in ('special32', 'special64'):
        w = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0]), E)
        w[rng.rand(E) < 0.002] = np.nan
        return w.astype(np.float32 if kind.endswith('32') else np.float64)
    raise ValueError(kind)
