"""Byte model of the hot path: the algorithmic bytes every kernel family moves per launch under the IMPLEMENTED schedule
(DESIGN.md section 3 states each formula), the bytes a step would move under SURVEY.md 8(d)'s per-hop definition, and
where a launch's working set lives.  Pure arithmetic -- used by bench.py for the `roofline` / `step_roofline` objects and
checked by tests/test_host_logic.py; nothing here touches a device.

Symbols: N nodes, E directed edges as given (edge_index columns), E' = E + N (the reference appends one self loop per node,
hashing.py:148; here they are implicit: `col` holds E entries, the walk visits E' rows), P MinHash permutations (u32 each),
M = 2^p HLL registers (u8 each), R = 4P + M bytes per sketch row, h hops, B pairs per query batch.
"""

HBM_PEAK_GBS = 8000.0           # MI355X spec (MI355X_MICROARCH.md); a float4 copy reaches 6.29 TB/s (79 %)
INFINITY_CACHE_BYTES = 256 << 20  # MALL / L3; FETCH_SIZE counts fabric requests INCLUDING the ones it serves


def csr_bytes(N, E):
    """ss_csr_build, ALGORITHMIC bytes: the edge list read once (16E), col (4E) and rowptr (8(N+1)) written once.  The level
    plans move more than that (one level 16E + 4E + 4E + 4E, two levels 16E + 8E + 8E + 4E + 4E + 4E); the
    roofline fraction of the build is taken on the algorithmic figure."""
    return 20 * E + 8 * (N + 1)


# random whole-row gathers of 512-byte rows against the size of the table they come from: tools/micro/gather_ceiling.hip on an
# MI355X (profiles/round4_gather_ceiling.txt; best of its in-flight / grid / rows-per-item settings), with the 4-byte id the probe
# reads for every gathered row COUNTED (the tracked table counts rows only: x 516 / 512) -- a row kernel's algorithmic bytes
# count its ids too.  Infinity-Cache resident below ~256 MB, HBM resident above.  A reference point for the access pattern, not a
# bound: a kernel also streams finished rows out, which travel faster than gathers.
GATHER_PROBE_GBS = [(30e6, 8730.0 * 516 / 512), (60e6, 8120.0 * 516 / 512), (120e6, 7840.0 * 516 / 512), (200e6, 7700.0 * 516 / 512),
                    (295e6, 7650.0 * 516 / 512), (600e6, 7550.0 * 516 / 512), (1500e6, 7090.0 * 516 / 512)]


def gather_probe_gbs(table_bytes):
    """measured rate (GB/s) of random row gathers from a table of this size: log-linear interpolation of GATHER_PROBE_GBS"""
    import math
    pts = GATHER_PROBE_GBS
    if table_bytes <= pts[0][0]:
        return pts[0][1]
    if table_bytes >= pts[-1][0]:
        return pts[-1][1]
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        if x0 <= table_bytes <= x1:
            t = (math.log(table_bytes) - math.log(x0)) / (math.log(x1) - math.log(x0))
            return y0 + t * (y1 - y0)
    return pts[-1][1]


def graph_read_bytes(N, E):
    """what every propagation launch reads of the CSR: col (4E) + rowptr (8(N+1))"""
    return 4 * E + 8 * (N + 1)


def kernel_bytes(N, E, P=128, p=8, h=2, B=65536, hub_edges=0, hub_rows=0, hosted=True, symmetric=False):
    """algorithmic bytes per LAUNCH of each kernel family of one step (build_hash_tables + one query batch).
    hub_edges / hub_rows: in-edges and count of the rows above the hub threshold.  The row wavefronts SKIP those rows; they are
    walked as hub units (csrc/ss_hub.hpp) by the leading workgroups of -- `hosted`, the default since round 4 -- the HLL first-hop
    launch (both hop-1 tables), the MinHash table-hop launch of hop 2 (both hop-2 tables: the fused kernel hosts none) and, for
    hops >= 3, the launch of their own sketch; their bytes are those launches' (`minhash_hop` is the MEAN over the h - 1 MinHash
    table-hop launches of a build).  hosted=False: launches of their own (`hub_first_hop` / `hub_table_hop`, one per hop, both
    sketches; rounds 1-3 and SS_HUB_LAUNCHES=1).  Crediting hub rows to a launch that skips them gave a roofline fraction above
    1 on skewed graphs.
    symmetric=True: the build found the edge list symmetric, so the regular rows of the table hops (`minhash_hop`, `hll_hop`, the HLL
    side of `fused_first_hop_hll_hop`) gather no self row (one row fewer per written row; a row without an in-edge
    keeps it -- not modelled; hub units keep theirs).  The default stays the model bench.py divides by."""
    M = 1 << p
    R = 4 * P + M
    Er, Nr = E - hub_edges, N - hub_rows      # what the row wavefronts walk / write
    Epr = Er + (0 if symmetric else Nr)        # + one implicit self loop per written row (table hops; none on a symmetric graph)
    graph = 4 * Er + 8 * (N + 1)               # col entries of the walked rows + rowptr
    hub_graph = 4 * hub_edges + 20 * hub_rows + 4 * hub_rows   # one pass over the hub rows: col + two rowptr words + list entry
    hub_tbl = hub_edges + 2 * hub_rows                         # table rows a table-hop pass reads (+ self loop) and writes
    out = {
        'csr_build': csr_bytes(N, E),
        # hop 1 from node ids: no table reads (hop-0 rows are recomputed in registers)
        'first_hop_hll': graph + Nr * M + 4 * Nr,                          # writes the HLL rows + cards[:, 0]
        'first_hop_minhash': graph + Nr * 4 * P,                           # writes the MinHash rows
        # table hops (k = 2..h): one input row per edge and self loop, one output row per node
        'hll_hop': (Epr + Nr) * M + graph + 4 * Nr,                        # + cards[:, k-1]
        'minhash_hop': (Epr + Nr) * 4 * P + graph,
        'pair_features': B * pair_bytes(P, p, h),
        # ss_fused_hop_stage's kernel: MinHash first hop + HLL table hop of hop 2 in one launch (the CSR is read once)
        'fused_first_hop_hll_hop': graph + Nr * 4 * P + (Epr + Nr) * M + 4 * Nr,
        # hub units as launches of their own: both sketches of the hub / mega rows of one hop
        'hub_first_hop': hub_graph + hub_rows * R,
        'hub_table_hop': hub_tbl * R + hub_graph,
    }
    if hosted and hub_rows:
        out['first_hop_hll'] += 2 * hub_graph + hub_rows * R + 4 * hub_rows          # a pass per sketch over the hub rows' ids
        hop2 = 2 * hub_graph + hub_tbl * R + 4 * hub_rows                            # MinHash launch of hop 2: both hop-2 tables
        later = hub_graph + hub_tbl * 4 * P                                          # hops >= 3: the MinHash units alone
        out['minhash_hop'] += (hop2 + (h - 2) * later) // max(h - 1, 1)
        out['hll_hop'] += hub_graph + hub_tbl * M + 4 * hub_rows                     # (hops >= 3; hop 2's HLL rows are the fused kernel's)
        out['hub_first_hop'] = out['hub_table_hop'] = 0
    return out


def hub_split(in_degree, hub_threshold):
    """(hub_edges, hub_rows) of a graph from its in-degree array (numpy) -- the arguments kernel_bytes takes"""
    hub = in_degree > hub_threshold
    return int(in_degree[hub].sum()), int(hub.sum())


def minhash_rows_bytes(N, E, n_rows, P=128, symmetric=False):
    """ss_minhash_hop_rows over n_rows rows drawn uniformly: per row its (E/N + 1) neighbour rows (self loop included) and its own
    output row of 4P bytes, its col entries and two rowptr words, the int64 row id.  symmetric=True: without the self rows (what the
    same rows cost a table hop that skips them; ss_minhash_hop_rows itself, the ELPH path, keeps them)"""
    return int(n_rows * ((E / N + (1 if symmetric else 2)) * 4 * P + 4 * E / N + 16 + 8))


def pair_bytes(P=128, p=8, h=2):
    """per pair: 2h sketch rows + the two int64 ids + 2h cardinalities + h(h+2) fp32 features"""
    return 2 * h * (4 * P + (1 << p)) + 16 + 8 * h + 4 * h * (h + 2)


def score_pair_bytes(P=128, p=8, h=2, normalised=False):
    """per pair of the scoring launch (ss_pair_scores): the query's bytes with ONE fp32 score stored instead of the
    h(h+2) features; with `normalised` the two fp32 degrees are read as the normalised query reads them.  The head's parameters
    (<= 3.8 KB, staged into LDS once per workgroup out of the L2) are not per-pair bytes."""
    return 2 * h * (4 * P + (1 << p)) + 16 + 8 * h + 4 + (8 if normalised else 0)


def pair_query_bytes(pairs, P=128, p=8, h=2):
    """bytes of get_subgraph_features over `pairs` links walked as listed: pairs * pair_bytes()"""
    return pairs * pair_bytes(P, p, h)


def score_query_bytes(pairs, P=128, p=8, h=2, normalised=False):
    """bytes of score_links over `pairs` links walked as listed: pairs * score_pair_bytes()"""
    return pairs * score_pair_bytes(P, p, h, normalised)


def topk_links_sources(h, P, M):
    """sources a workgroup of the scoring scan stages (csrc/ss_topk_head.hip topk_head_sources): the most of {32, 16, 8} that
    leave two workgroups per CU -- 80 KiB each -- next to the estimator tables (8 196 B), the head (3 840 B) and 64 B of alignment;
    a source costs 12 + 4h bytes and, on the fast shapes (M = 256, P in {64, 128, 192, 256}), h rows of 4P + 576 bytes of LDS"""
    fast = M == 256 and P in (64, 128, 192, 256)
    per_source = 12 + 4 * h + (h * (4 * P + 576) if fast else 0)
    for sb in (32, 16):
        if 8196 + 3840 + 64 + sb * per_source <= 80 * 1024:
            return sb
    return 8


def topk_links_bytes(N, S, h, P, M):
    """algorithmic bytes of one ss_topk_score_scan launch (ElphHashes.topk_links): every candidate's h rows of 4P + M
    bytes once per block of staged sources, the sources' h rows once per workgroup (the launch aims for 4 096 workgroups, 16
    candidates in flight each), one int64 key per (source, candidate).  The candidates' cards / degrees (4h + 4 bytes against h
    rows), the exclude pass and torch.topk's read of the keys are not in it."""
    R = 4 * P + M
    sb = topk_links_sources(h, P, M)
    blocks_y = -(-S // sb)
    blocks_x = min(-(-4096 // max(blocks_y, 1)), -(-N // 16))
    return blocks_y * N * h * R + blocks_x * S * h * R + 8 * S * N


def rank_links_queries(h, P, M):
    """links a workgroup of the ranking scan stages (csrc/ss_rank.hip rank_queries): topk_links_sources' rule with 20 more bytes per
    staged entry -- the target id, the threshold and the two 32-bit sums -- so 32 + 4h bytes next to the h rows of the fast shapes"""
    fast = M == 256 and P in (64, 128, 192, 256)
    per_query = 32 + 4 * h + (h * (4 * P + 576) if fast else 0)
    for qb in (32, 16):
        if 8196 + 3840 + 64 + qb * per_query <= 80 * 1024:
            return qb
    return 8


def rank_links_bytes(N, L, h, P, M):
    """algorithmic bytes of one ss_rank_score_scan launch (ElphHashes.rank_links): every candidate's h rows of 4P + M
    bytes once per block of staged links -- table rows read once per workgroup pass --, the sources' h rows, the 16-byte link and its
    4-byte threshold once per workgroup (the launch aims for 4 096 workgroups, 16 candidates in flight each), and the two int64 counts
    of every link: 16 L bytes written, whatever N.  The candidates' cards / degrees, the threshold launch (score_query_bytes(L)) and
    the exclusion correction (score_query_bytes over the excluded pairs) are not in it."""
    R = 4 * P + M
    qb = rank_links_queries(h, P, M)
    blocks_y = -(-L // qb)
    blocks_x = min(-(-4096 // max(blocks_y, 1)), -(-N // 16))
    return blocks_y * N * h * R + blocks_x * L * (h * R + 20) + 16 * L


def lsh_band_keys_bytes(N, P, rows, bands):
    """algorithmic bytes of one ss_lsh_band_keys launch (ElphHashes.build_lsh_index): the hop's MinHash table read once,
    N P 4 bytes (only the 16-byte chunks that hold the rows * bands values in use), one int64 key per node and band written.  The
    sort of the bands that follows is torch's and not in it."""
    return N * 16 * -(-rows * bands // 4) + 8 * N * bands


def wedge_bytes(sources, neighbours, walks, candidates):
    """algorithmic bytes of WedgeGraph.candidates' expansion (ss_wedge_walks + ss_wedge_fold / ss_wedge_emit) over
    `sources` sources with `neighbours` = sum deg(u), `walks` = sum W(u) and `candidates` listed pairs: per source its id, two row
    pointers and W(u); row u is read twice (the walks launch, the expansion), with two row pointers per neighbour each time; every
    walk reads one col entry; the output is 8 + 4 bytes per listed pair.  What the large tier writes and the sort moves on top of
    that -- 8 bytes per walk, several times -- is the price of that tier and not in the model."""
    return sources * (8 + 16 + 8) + 2 * neighbours * (4 + 16) + 4 * walks + 12 * candidates


def cn_features_bytes(links, row_entries, hits, F, weighted=False):
    """algorithmic bytes per launch of the three kernels of heuristics.common_neighbours / common_neighbour_features
    (csrc/ss_cn_pool.hip) over `links` links whose two CSR rows hold `row_entries` entries in all and which share
    `hits` = T common neighbours.  Every launch reads the links (16 each) and the two rows per link: four row pointer words (32) and 4
    bytes per stored column (the binary search probes the longer row instead of streaming it: an upper bound there).  `weighted`
    (a matrix with values, a multiplier): the fp64 values of both rows (8 per entry) and one fp64 multiplier per hit.
      'count'  + one int64 count per link
      'fill'   + one int64 offset per link, 8 + 4 bytes written per hit (id + coefficient)
      'pool'   + hits * 4F gathered from x and links * 4F written -- the term that decides the launch at F = 128"""
    rows = 16 * links + 32 * links + 4 * row_entries
    values = (8 * row_entries + 8 * hits) if weighted else 0
    return {'count': rows + 8 * links,
            'fill': rows + values + 8 * links + 12 * hits,
            'pool': rows + values + hits * 4 * F + links * 4 * F}


def gcn_spmm_bytes(N, E, F, self_loops=0, unit=True):
    """algorithmic bytes of one product of gcn.gcn_propagate (ss_gcn_spmm_t or ss_sign_spmm, csrc/ss_spmm.hip) -- the
    same for both flows -- over N nodes and E edges of which `self_loops` are existing self loops (E' = E - self_loops entries
    gather a row; every node's remaining loop gathers its own), F fp32 columns, rounded up to a multiple of 4.
      'gathered'  (E' + N) * 4F from x          'written'  N * 4F
      'entries'   per edge the order word (4), the other endpoint (8) and its dinv (4), the weight (4) unless all are 1;
                  per node two row-pointer words (16), dinv and loop_w (8)
    F > 256 re-reads the entry words once per 256 columns: ceil(F / 256) times."""
    F = (F + 3) // 4 * 4
    if N == 0 or F == 0:
        return {'gathered': 0, 'written': 0, 'entries': 0, 'total': 0}
    passes = (F + 255) // 256
    gathered = (E - self_loops + N) * 4 * F
    written = N * 4 * F
    entries = passes * E * (16 if unit else 20) + N * 24
    return {'gathered': gathered, 'written': written, 'entries': entries, 'total': gathered + written + entries}


def aggr_bytes(N, E, F, unit=True, mean=False, root=False, hub_chunks=0):
    """algorithmic bytes of one product of aggr.aggregate (ss_aggr_rows with the hub launches, csrc/ss_aggr.hip) -- the
    same for both flows -- over N nodes and E edges (every edge is an entry: self loops too), F fp32 columns rounded up to a multiple of 4.
      'gathered'   E * 4F from x, and N * 4F more with a root term (the node's own row)
      'written'    N * 4F
      'entries'    per edge the order word (4) and the other endpoint (8), the weight (4) unless unit; per node two row-pointer
                   words (16), and den (4) for the mean
      'workspace'  hub_chunks * 4F written by the partials launch and read again by the finish launch
    F > 256 re-reads the edge words once per 256 columns: ceil(F / 256) times.  The mean's backward gathers one den word (4) per
    edge on top of this, which the model does not count."""
    F = (F + 3) // 4 * 4
    if N == 0 or F == 0:
        return {'gathered': 0, 'written': 0, 'entries': 0, 'workspace': 0, 'total': 0}
    passes = (F + 255) // 256
    gathered = (E + (N if root else 0)) * 4 * F
    written = N * 4 * F
    entries = passes * E * (12 if unit else 16) + N * (20 if mean else 16)
    workspace = 2 * hub_chunks * 4 * F
    return {'gathered': gathered, 'written': written, 'entries': entries, 'workspace': workspace,
            'total': gathered + written + entries + workspace}


def link_decoder_bytes(N, L, F, product=False, backward=False, M=None, hub_chunks=0):
    """algorithmic bytes of one launch family of link_decoder (csrc/ss_link_decoder.hip) for L links over N nodes and F
    fp32 columns: link_gather (product=False) or link_hadamard (product=True), forward or backward; M = the distinct nodes the batch
    touches (default: as many as there can be, min(N, 2L)).
      forward    'ids' the 2L endpoint ids (8 each); 'gathered' 2L rows of x (4F each); 'written' 2L rows (gather) or L rows (product)
      backward   'cleared' the zero fill of grad_x, N * 4F; 'gathered' per slot a row of g, and for the product the partner's row of x
                 as well; 'written' the M touched rows; 'entries' per slot the order word (4) and, for the product, the partner id
                 (8), re-read once per pass over the columns -- ceil(F / 256) passes with float4 pieces, ceil(F / 64) when F % 4 != 0 --
                 and per touched node its id (8) and two row-pointer words (16); 'workspace' hub_chunks * 4F written by the partials
                 launch and read again by the finish launch
    The plan's own build (a stable grouping of 2L ids and a few passes over N counters) is not part of a product and not counted."""
    zero = {'ids': 0, 'gathered': 0, 'written': 0, 'cleared': 0, 'entries': 0, 'workspace': 0, 'total': 0}
    if F == 0 or (L == 0 and not backward) or (N == 0 and backward):
        return zero
    row = 4 * F
    b = dict(zero)
    if not backward:
        b['ids'], b['gathered'], b['written'] = 2 * L * 8, 2 * L * row, (L if product else 2 * L) * row
    else:
        M = min(N, 2 * L) if M is None else M
        passes = (F + 255) // 256 if F % 4 == 0 else (F + 63) // 64
        b['cleared'] = N * row
        b['gathered'] = (2 if product else 1) * 2 * L * row
        b['written'] = M * row
        b['entries'] = passes * 2 * L * (12 if product else 4) + M * 24
        b['workspace'] = 2 * hub_chunks * row
    b['total'] = sum(v for k, v in b.items() if k != 'total')
    return b


def cn_rows_bytes(N, L, T, F, backward=False, M=None, hub_chunks=0):
    """algorithmic bytes of one launch family of cn_pool.common_neighbour_pool (csrc/ss_cn_rows.hip) for a list of T entries
    in L links over N nodes and F fp32 columns, forward or backward; M = the distinct nodes the list names (default: as many as
    there can be, min(N, T)); hub_chunks = the 256-entry chunks of the direction's hub rows.
      forward    'gathered' per entry a row of x (4F); 'written' the L rows of out (4F each); 'entries' per entry its id (8) and
                 coefficient (4), re-read once per pass over the columns -- ceil(F / 256) passes with float4 pieces, ceil(F / 64) when
                 F % 4 != 0 -- and per link two row-pointer words (16); 'workspace' hub_chunks * 4F written by the partials launch
                 and read again by the finish launch
      backward   'cleared' the zero fill of grad_x, N * 4F; 'gathered' per entry a row of g; 'written' the M named rows; 'entries'
                 per entry and pass the order word (4), the owner (8) and the coefficient (4), and per named node its id (8) and two
                 row-pointer words (16); 'workspace' as in the forward
    The plan's own build (the list, a stable grouping of T ids and a few passes over N counters) is not part of a product and not
    counted."""
    zero = {'gathered': 0, 'written': 0, 'cleared': 0, 'entries': 0, 'workspace': 0, 'total': 0}
    if F == 0 or (L == 0 and not backward) or (N == 0 and backward):
        return zero
    row = 4 * F
    passes = (F + 255) // 256 if F % 4 == 0 else (F + 63) // 64
    b = dict(zero)
    b['gathered'] = T * row
    b['workspace'] = 2 * hub_chunks * row
    if not backward:
        b['written'] = L * row
        b['entries'] = passes * T * 12 + L * 16
    else:
        M = min(N, T) if M is None else M
        b['cleared'] = N * row
        b['written'] = M * row
        b['entries'] = passes * T * 16 + M * 24
    b['total'] = sum(v for k, v in b.items() if k != 'total')
    return b


def segment_pool_bytes(T, L, F):
    """algorithmic bytes of pooling.global_add_pool / global_mean_pool forward (ss_segment_pool, csrc/ss_pool.hip)
    over T node rows in L graphs, F fp32 columns: every row of x read once (T * 4F), the output written (L * 4F), the L + 1 offsets.
    The backward moves the same bytes the other way (g read, grad_x written)."""
    return T * 4 * F + L * 4 * F + 8 * (L + 1)


def sort_pool_bytes(T, L, F, k):
    """algorithmic bytes of pooling.global_sort_pool forward (ss_pool_select + ss_pool_gather): the key column once (T * 4: one
    channel of x; the large tier re-reads it, which the model does not count), the selected rows (at most L * k * 4F), perm written
    and read (2 * L * k * 4), the output (L * k * 4F) and the L + 1 offsets twice."""
    return T * 4 + 2 * L * k * 4 * F + 2 * L * k * 4 + 16 * (L + 1)


def pair_bytes_grouped(pairs, runs, P=128, p=8, h=2):
    """bytes of a query over `pairs` links walked grouped by their first node (ss_pair_features_grouped, hashing.GROUP_LINKS_MIN):
    the first node's h rows are fetched once per RUN of pairs that share it (`runs` = distinct first nodes of a grouped list),
    everything else per pair as in pair_bytes -- the bytes the implemented walk has to move; pairs * pair_bytes() is the
    SURVEY 8(d) definition, which charges 2h rows to every pair"""
    R = 4 * P + (1 << p)
    return pairs * (h * R + 16 + 8 * h + 4 * h * (h + 2)) + runs * h * R


def step_bytes_implemented(N, E, P=128, p=8, h=2, B=65536, hub_edges=0, hub_rows=0):
    """bytes of one step under the implemented schedule: CSR build, hop 1 from node ids, h - 1 table hops, one query batch
    (the hub units included: the same rows and edges, walked by other workgroups)"""
    k = kernel_bytes(N, E, P, p, h, B, hub_edges, hub_rows, hosted=False)
    return (k['csr_build'] + k['first_hop_hll'] + k['first_hop_minhash'] + k['hub_first_hop']
            + (h - 1) * (k['hll_hop'] + k['minhash_hop'] + k['hub_table_hop']) + k['pair_features'])


def step_bytes_survey(N, E, P=128, p=8, h=2, B=65536):
    """h table hops of (E'+N)R + 4E' + 8(N+1) + 4N bytes + the query; CSR construction and hop-0
    initialisation reported separately there.  Larger than the implemented schedule's bytes because hop 1 no longer reads
    a table -- a step faster than this figure / 8 TB/s is therefore not a measurement error."""
    R, Ep = 4 * P + (1 << p), E + N
    return h * ((Ep + N) * R + 4 * Ep + 8 * (N + 1) + 4 * N) + B * pair_bytes(P, p, h)


def unique_bytes(N, E, family, P=128, p=8):
    """distinct HBM bytes a launch touches (each input row counted once however many edges read it): what the HBM
    itself must deliver when the input table fits the Infinity Cache"""
    M = 1 << p
    row = {'minhash_hop': 4 * P, 'hll_hop': M}[family]
    return 2 * N * row + graph_read_bytes(N, E) + (4 * N if family == 'hll_hop' else 0)


def resident_label(table_bytes):
    """where a gathered table lives, from the share of it the 256 MiB Infinity Cache can hold: all of it -> 'infinity-cache' (its
    random row reads are served there, `achieved` is a fabric + cache rate), at least half -> 'mixed', less -> 'hbm'.  ONE rule for
    bench.py's line and for tools/roofline_table.py (round 5's tables called a 74-91 % cached table 'hbm': VERDICT r5 weak #9b)."""
    f = cache_resident_fraction(table_bytes)
    return 'infinity-cache' if f >= 1.0 else ('mixed' if f >= 0.5 else 'hbm')


def residency(N, family, P=128, p=8, h=2):
    """resident_label of the table(s) a kernel family gathers rows from"""
    return resident_label(gathered_table_bytes(N, family, P, p, h))


def cache_resident_fraction(table_bytes):
    """share of a gathered table set the 256 MiB Infinity Cache can hold: min(1, 256 MiB / bytes)"""
    return 1.0 if table_bytes <= 0 else min(1.0, INFINITY_CACHE_BYTES / float(table_bytes))


def gathered_table_bytes(N, family, P=128, p=8, h=2):
    """bytes of the table(s) a kernel family gathers rows from"""
    M = 1 << p
    return {'minhash_hop': N * 4 * P, 'hll_hop': N * M, 'fused_first_hop_hll_hop': N * M, 'pair_features': h * N * (4 * P + M)}[family]


def update_bytes(N, E, dirty_rows, dirty_edges, P=128, p=8, hop=2, first_hop_from_ids=True):
    """algorithmic bytes of the two kernel families of ElphHashes.update_hash_tables (csrc/ss_update.hip) at one hop.
    dirty_rows / dirty_edges: |dirty_hop| and the in-edges of those rows.
      'mark'  one pull pass over the in-edge CSR: col (4E, an upper bound: a row stops at its first dirty in-neighbour) + rowptr
              (8(N+1)) + one flag byte read per walked in-edge (L2 hits: the map is N bytes) + the seed and previous-hop flags of
              the row itself (2N) + this hop's map written (N) + the list (4 dirty_rows).  Hop 1 reads no edges: the seed map (N),
              cards_old[:, 0] (4N), rowptr (8(N+1)), the map written back (N), the list.
      'rows'  the listed rows recomputed from scratch: list entry + two rowptr words (20) + col (4 per in-edge) per row; a table hop
              gathers one R-byte row per in-edge and per implicit self loop and writes R + 4 bytes (the row + its cardinality); the
              first hop from node ids reads no table."""
    M = 1 << p
    R = 4 * P + M
    if hop == 1:
        mark = N + 4 * N + 8 * (N + 1) + N + 4 * dirty_rows
    else:
        mark = 4 * E + E + 8 * (N + 1) + 2 * N + N + 4 * dirty_rows
    graph = 20 * dirty_rows + 4 * dirty_edges
    if hop == 1 and first_hop_from_ids:
        rows = graph + dirty_rows * (R + 4)
    else:
        rows = graph + (dirty_edges + dirty_rows) * R + dirty_rows * (R + 4)
    return {'mark': mark, 'rows': rows}


def masked_query_bytes(links, edge_links, mean_in_degree, P=128, p=8, h=2, two_hop_walks=0.0):
    """algorithmic bytes of ElphHashes.get_subgraph_features(mask_target=...) over `links` links of which `edge_links` are edges of the
    graph (csrc/ss_masked.hip).  mean_in_degree: mean in-degree of the endpoints of the edge links; two_hop_walks: mean
    number of 2-hop in-walks (sum of the in-degrees of the in-neighbours) of such an endpoint, read at h = 3 only.
      plain query   pair_bytes per link -- every row is written by it
      classify      the two ids (16) + two rowptr pairs (32) + the col entries of rows u and v (4 each) per link
      masked rows   per edge link: list entry + ids + rowptr (4 + 16 + 32), col of both rows once per hop walked; hop 1 reads no table
                    (node ids are hashed); hop 2 gathers one R-byte hop-1 row per in-neighbour of u and of v; hop 3 one per 2-hop
                    in-walk and per in-neighbour (+ their col entries and rowptr words); the output row is written again"""
    R = 4 * P + (1 << p)
    d = float(mean_in_degree)
    plain = links * pair_bytes(P, p, h)
    classify = links * (48 + 8 * d)
    per_edge = 52 + 8 * d + 4 * h * (h + 2)
    if h >= 2:
        per_edge += 2 * d * (R + 4)
    if h >= 3:
        per_edge += 2 * (two_hop_walks + d) * (R + 4) + 2 * d * 16
    return int(plain + classify + edge_links * per_edge)


def subgraph_bytes(links, nodes, arcs, csr_arcs, node_label='drnl', offchip_nodes=0):
    """algorithmic bytes of the two kernel families ElphHashes.exact_subgraphs adds to the node list (csrc/ss_subgraph.hip).
    nodes: listed nodes T; arcs: emitted adjacency entries A; csr_arcs: the in-arcs of the listed nodes that the intersection walks
    (sum over listed nodes of min(deg x, the probes of the id-row walk): for graphs without hubs the sum of the in-degrees);
    offchip_nodes: nodes of the rows the label kernel keeps in its device workspace.
      'adj_count'  per listed node its id (8), two CSR row pointer words (16) and 4 bytes written; 4 per walked in-arc.  The binary
                   searches (the link of a node in rowptr, an arc's source in the id row) probe arrays that the same workgroup has
                   just read: cache hits, not counted.  16 per link (its ids), once.
      'adj_fill'   the same reads + two adj_ptr words per node (8 distinct) and 8 written per emitted arc (nbr + weight), 8 per link
                   (roots)
      'labels'     per side of the BFS: two adj_ptr words per expanded node (8 distinct) and 4 per arc; 8 (drnl) or 16 (de, de+) bytes
                   of z per node, written once; an off-chip row also writes its 16 workspace bytes per node once and claims each
                   node once per side with a 4-byte atomic.  'hop' / 'zo' / None run no kernel (a torch reduction over dist: 2 read,
                   8 written per node)."""
    count = 28 * nodes + 4 * csr_arcs + 16 * links
    fill = 32 * nodes + 4 * csr_arcs + 8 * arcs + 24 * links
    if node_label in ('drnl', 'de', 'de+'):
        z = 8 if node_label == 'drnl' else 16
        labels = 2 * (8 * nodes + 4 * arcs) + z * nodes + 24 * offchip_nodes + 24 * links
    else:
        labels = 0 if node_label is None else 10 * nodes
    return {'adj_count': count, 'adj_fill': fill, 'labels': labels}


def sampled_nodes_bytes(links, kept, expanded, walked_arcs, num_nodes=0, slot_links=0, slot_visited=0, slot_selected=0, slot_kept=0):
    """algorithmic bytes of the two passes of ElphHashes.sampled_subgraph_nodes (csrc/ss_sampled_nodes.hip).
    kept: listed nodes T; expanded: the kept nodes of hops 0 .. h - 1 whose in-arcs a pass walks; walked_arcs: the sum of their
    in-degrees (the measure of the walk: a fringe can be 1000 times what is kept, and every arc into it is read).  The on-chip tier
    keeps visited, fringe and selection in LDS: beyond the walk it moves nothing.  The slot tier's links (slot_links of them, on a
    graph of num_nodes nodes) add, per pass: slot_visited nodes reached for the first time (a 4-byte atomic on the level word and a
    4-byte list entry each, and the same again to clear), slot_selected fringe nodes of the hops where a selection ran (read 9 times
    as 4-byte ids: eight digit passes and the marking pass; the keys are recomputed, there is no key array) and slot_kept kept nodes
    (a 4-byte atomic and a 4-byte list entry).
      'count'  per link its ids (16) and counts + state written (8); per expanded node two CSR row pointer words (16); 4 per walked arc
      'fill'   the same walk + two rowptr words (16) and the state (4) per link, 9 written per listed node (id + hop); a slot-tier link
               scans its num_nodes level bytes once"""
    walk = 16 * links + 16 * expanded + 4 * walked_arcs + 16 * slot_visited + 36 * slot_selected + 8 * slot_kept
    return {'count': walk + 8 * links, 'fill': walk + 20 * links + 9 * kept + num_nodes * slot_links}
