/*
 * subgraph_sketch.h -- C ABI of the MI355X (gfx950) subgraph-sketching engine.
 *
 * The reference (melifluos/subgraph-sketching) has no FFI layer: its hot path is the Python class
 * `ElphHashes` in src/hashing.py.  This header is the boundary a replacement binds to; each entry
 * point names the reference code it replaces (file:line under /root/reference).  The Python host
 * class in subgraph-sketching_amd/hashing.py is the only in-tree caller (through ctypes); the
 * reference-side binding is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  Every data pointer is a DEVICE pointer unless the
 *     comment says "host".  No torch types.
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and returns 0 on success or a negative SS_ERR_* code (argument / launch errors are detected
 *     synchronously on the host; nothing is thrown).
 *   - Canonical sketch layout in HBM ("packed"): MinHash rows are uint32[P] (every reference value
 *     is < 2^32, hashing.py:59,122), HyperLogLog rows are uint8[M], M = 2^p (values 0..64-p,
 *     hashing.py:75-76).  Row-major [N, P] / [N, M], rows 16-byte aligned (P % 4 == 0, p >= 4).
 *   - The caller owns every buffer, including workspaces.
 */
#ifndef SUBGRAPH_SKETCH_H
#define SUBGRAPH_SKETCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_OK 0
#define SS_ERR_INVALID_ARG (-1)   /* null pointer / size / unsupported P, p, h                    */
#define SS_ERR_LAUNCH (-2)        /* hipGetLastError() != hipSuccess after a launch                */
#define SS_ERR_WORKSPACE (-3)     /* workspace too small                                           */
#define SS_ERR_UNSUPPORTED (-4)   /* parameter combination has no kernel                           */

#define SS_MAX_HOPS 3             /* hashing.py:54 */
#define SS_MAX_TABLE 512          /* max entries of the HLL++ bias tables (datasketch ships <= 200) */

/* flags of ss_pair_features (hashing.py:56,67) */
#define SS_FLAG_USE_ZERO_ONE 1u
#define SS_FLAG_FLOOR_SF 2u
/* ss_exact_pairs / ss_exact_large only: the balls of (u, v) are those of the graph without the edges u -> v and v -> u */
#define SS_FLAG_MASK_TARGET 4u

/* HyperLogLog++ estimator constants -- everything ElphHashes.__init__ takes from datasketch
 * (hashing.py:69-80) plus two host-derived helpers.  All fp32 values are rounded on the host exactly
 * as torch rounds the reference's Python scalars. */
typedef struct ss_hll_params {
    int32_t p;              /* hll_p; m = 1 << p                                   (hashing.py:65-66) */
    int32_t n_tbl;          /* entries in raw_est / bias, 6 <= n_tbl <= SS_MAX_TABLE                  */
    float alpha_mm;         /* fp32(alpha * m^2)                                   (hashing.py:228)   */
    float threshold;        /* fp32(hll_threshold)                                 (hashing.py:78)    */
    int32_t lc_min_zeros;   /* linear counting is returned iff V >= lc_min_zeros (V = #zero registers,
                               V > 0); derived on the host from lc_table <= threshold (hashing.py:220-226) */
    int32_t reserved;
    const float *raw_est;   /* device [n_tbl]: estimate_vector SORTED ascending     (hashing.py:80)    */
    const float *bias;      /* device [n_tbl]: bias_vector, permuted like raw_est  (hashing.py:79)    */
    const float *lc_table;  /* device [m+1]: lc_table[V] = m*log(m/V) in fp32, V>=1 (hashing.py:194-195) */
} ss_hll_params;

/* library / build identification */
int ss_version(void);
const char *ss_error_string(int code);

/* Hop-0 MinHash rows.  Replaces ElphHashes.initialise_minhash (hashing.py:118-124); a/b are the
 * permutation parameters of _init_permutations (hashing.py:106-116, drawn on the host with numpy's
 * RandomState(1)), device uint64[P].  Writes rows for nodes first_node .. first_node+n-1
 * (node id i hashes the value i+1, hashing.py:121). */
int ss_minhash_init(uint32_t *out, int64_t first_node, int64_t n, const uint64_t *a, const uint64_t *b, int32_t P,
                    void *stream);

/* Hop-0 HyperLogLog rows.  Replaces ElphHashes.initialise_hll + _get_hll_rank (hashing.py:126-137,
 * 91-104): one non-zero register per row. */
int ss_hll_init(uint8_t *out, int64_t first_node, int64_t n, int32_t p, void *stream);

/* Destination-grouped adjacency resident on the device (built by ss_csr_build, consumed by the propagation
 * kernels).  The struct itself lives on the host and is read at launch. */
typedef struct ss_csr_graph {
    const int64_t *rowptr;            /* device int64[N+1]                                                    */
    const int32_t *col;               /* device int32[E]: source ids grouped by destination                    */
    int64_t num_nodes;                /* N                                                                     */
    int64_t n_self_loops;             /* rows i < n_self_loops also receive their own row (implicit self loop)  */
    const int64_t *n_self_loops_dev;  /* device int64 (nullable): overrides n_self_loops, read by the kernels   */
    int32_t hub_threshold;            /* rows with more than this many in-edges are "hub rows" ...              */
    int32_t reserved;                 /* flags: SS_GRAPH_* bits below (0: none)                                 */
    const int32_t *hub_rows;          /* ... listed here (device int32[*hub_count], nullable) and processed by  */
    const int32_t *hub_count;         /* a 16-wave cooperative kernel instead of a single wavefront             */
    const int32_t *mega_rows;         /* device int32[4 * max]: {row, first_slice, n_slices, done} per "mega row" */
    const int32_t *mega_count;        /* device int32[2]: {mega rows, slices}.  Rows with more than SS_MEGA_SLICE   */
    void *mega_scratch;               /* neighbours are walked slice by slice by ALL hub workgroups; the partial     */
                                      /* rows go through mega_scratch (SS_MEGA_SLOT_BYTES each), the last slice to   */
                                      /* finish combines them.  All three nullable together (then such rows are hub rows).  */
    int64_t row_begin;                /* destination rows [row_begin, row_end) are computed by ss_propagate /    */
    int64_t row_end;                  /* ss_first_hop (multi-GPU destination-range sharding);       */
                                      /* row_end == 0 means all rows.  Outputs are indexed by the GLOBAL row id.  */
    /* Peer-write build (the row-sharded build without an exchange step): every row a launch finishes is ALSO    */
    /* stored into these tables of the other ranks (device pointers into peers' memory, mapped through hipIpc / torch's       */
    /* CUDA-IPC; same shapes and strides as the launch's own mh_out / hll_out / cards_out; entries of a sketch the launch does */
    /* not produce are ignored).  The stores travel over xGMI while the kernel runs; the hop boundary then needs a cross-rank   */
    /* barrier only.  n_mirrors == 0: none.                                                                                   */
    int32_t n_mirrors;
    int32_t reserved2;
    uint32_t *mirror_mh[7];           /* SS_MAX_MIRRORS */
    uint8_t *mirror_hll[7];
    float *mirror_cards[7];
    /* Hub-row report (nullable): the first-hop launches from node ids -- the HLL first-hop kernel and the MinHash rows kernel   */
    /* of ss_first_hop, the HLL first-hop launch of ss_fused_hop_stage (not its fused kernel: a stage called with cards1_out ==  */
    /* NULL, the deferred first hop, reports nothing) -- store *report_hub_count + report_mega_count[0], the counters            */
    /* ss_csr_build left on the device, into *hub_report, a device-VISIBLE int32 such as pinned host memory, at their very start */
    /* (the store is long complete when the launch ends).  The word must stay valid until those launches have run.  The host    */
    /* may read it later WITHOUT synchronising, as a hint: a shape whose earlier build listed no such rows is propagated with    */
    /* hub_rows = NULL -- no hub units are served (leading workgroups that find nothing to do on an unskewed graph), every row   */
    /* is walked by its row kernel, so a stale hint costs time, never correctness.                                              */
    int32_t *hub_report;
    const int32_t *report_hub_count;
    const int32_t *report_mega_count;
    /* Symmetry word (nullable): the device int32 ss_csr_build_symmetric left for THIS adjacency -- 1: for every stored edge j -> i */
    /* the edge i -> j is stored as often.  With SS_GRAPH_HOP_TABLES the table-hop row kernels then leave out the implicit self row  */
    /* of every row that has an in-edge (see SS_GRAPH_HOP_TABLES).                                                                  */
    const int32_t *symmetric_dev;
} ss_csr_graph;
#define SS_MAX_MIRRORS 7
/* ss_csr_graph.reserved (the flags word) bit 0, the caller's promise about ONE call of ss_propagate: the input tables of this call are hop-(k-1) tables,
 * k - 1 >= 1, of this same graph, built with these same implicit self loops (n_self_loops_dev = the max(edge_index) + 1 ss_csr_build
 * left: every node that occurs in an edge has one).  On a symmetric graph (*symmetric_dev != 0) the own row of a node with a
 * neighbour then aggregates a subset of what its neighbours' rows aggregate -- each neighbour m is in its own row through m's self
 * loop, the node itself is in every neighbour's row by symmetry -- and min / max are idempotent: the regular-row paths skip the
 * gather of the own row, bit-identical results, N fewer row gathers per hop.  Never true of hop-0 inputs (rows that are functions of
 * the node id alone) or of arbitrary tensors; without the bit, without the word or with n_self_loops_dev == NULL nothing changes.
 * ss_fused_hop_stage, whose table hops read the hop-1 tables it has just built, applies the rule on its own.  SS_SELF_SKIP=0 in
 * the environment (read at every launch) turns it off everywhere. */
#define SS_GRAPH_HOP_TABLES 1

/* CSR-by-destination of an edge list.  Replaces the message materialisation of
 * torch_geometric MessagePassing.propagate as used by hashing.py:34,44 (flow source -> target).
 *   src/dst: device int64[E] (edge_index[0], edge_index[1]);  rowptr: device int64[N+1];
 *   col: device int32[E] (source ids grouped by destination, order inside a row unspecified).
 *   n_self_loops_out: device int64 (nullable) <- max(edge_index) + 1 (0 for E == 0): the number of self loops
 *   torch_geometric.utils.add_self_loops(edge_index) appends when num_nodes is not given (hashing.py:148), so
 *   the host never has to synchronise on edge_index.max().
 *   hub_rows / hub_count (device int32[N] / int32, both nullable): rows with more than hub_threshold in-edges.
 *   err_flag: device int32 (nullable), set to 1 if any endpoint is outside [0, N) (such edges are dropped).
 * Workspace: ss_csr_workspace_bytes(N, E) bytes (0 = unsupported size).  No per-edge global atomics: a
 * two-level counting sort (LDS histograms per edge slice -> bucket offsets -> per-bucket LDS sort). */
#define SS_MEGA_SLICE 1024      /* neighbours per slice of a mega row (one 64-neighbour chunk per wavefront of a hub workgroup) */
#define SS_MEGA_SLOT_BYTES 1280 /* scratch per slice: partial MinHash row (<= 256 x u32) + partial HLL row (256 B) */
#define SS_MEGA_DESC_WORDS 8   /* int32 words per entry of mega_rows: {row, first slice, slices, ticket (MinHash side), ticket (HLL side), 0, 0, 0} */
size_t ss_csr_workspace_bytes(int64_t N, int64_t E);
/* mega_rows / mega_count (nullable together): rows with more than max(hub_threshold, SS_MEGA_SLICE) in-edges are listed
 * there instead of in hub_rows: mega_rows must hold SS_MEGA_DESC_WORDS * (E / SS_MEGA_SLICE + 1) int32, mega_count 2 int32; the slices of
 * all mega rows number at most 3 * (E / SS_MEGA_SLICE + 1) -- the scratch ss_csr_graph.mega_scratch needs SS_MEGA_SLOT_BYTES for each. */
int ss_csr_build(const int64_t *src, const int64_t *dst, int64_t E, int64_t N, int64_t *rowptr, int32_t *col,
                 int64_t *n_self_loops_out, int32_t hub_threshold, int32_t *hub_rows, int32_t *hub_count,
                 int32_t *mega_rows, int32_t *mega_count,
                 int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream);
/* ss_csr_build (fingerprint == NULL) or ss_csr_build_cached (fingerprint given) with one more output: *symmetric_out (device int32,
 * nullable) <- 1 iff the edge MULTISET is symmetric (as many copies of j -> i as of i -> j; self edges count for nothing) and no id was
 * out of range, else 0; 0 for E == 0.  Decided on the device by the build's own launches from two independent 64-bit sums over
 * the edges (a false 1 needs both to cancel: the 128-bit kind of content fingerprint ss_csr_build_cached rests on); a cached
 * build that finds the content unchanged leaves the word of the build it keeps.  For ss_csr_graph.symmetric_dev. */
int ss_csr_build_symmetric(const int64_t *src, const int64_t *dst, int64_t E, int64_t N, int64_t *rowptr, int32_t *col,
                           int64_t *n_self_loops_out, int32_t hub_threshold, int32_t *hub_rows, int32_t *hub_count,
                           int32_t *mega_rows, int32_t *mega_count, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                           void *fingerprint, int32_t *symmetric_out, void *stream);
/* Failure of a build that was launched (every entry point that runs the builder: ss_csr_build, ss_csr_build_cached,
 * ss_group_links_by_source, ss_csr_group_ids).  Buckets too dense for one workgroup are worked off in shares by several workgroups of
 * the finish launch; the one cross-workgroup wait of that protocol is bounded (~2 s: it can only end late when the process is
 * descheduled for seconds).  A wait that gives up leaves the outputs INCOMPLETE and is reported, never silently:
 *   - bit 1 (SS_CSR_ERR_PROTOCOL) of *err_flag, when a flag was given (bit 0 = an endpoint outside [0, N), as before: test the bits);
 *   - ss_csr_protocol_faults(): 0 while no wait of this process (any device, any stream) has given up; afterwards a positive stamp
 *     that CHANGES with every further one.  Kept in pinned host memory and read WITHOUT synchronising -- compare before / after a
 *     synchronised build, or poll it as the host mirror does (ElphHashes.check_errors and every later call raise RuntimeError).
 *     -1: the word could not be allocated (no device). */
#define SS_CSR_ERR_BOUNDS 1
#define SS_CSR_ERR_PROTOCOL 2
int ss_csr_protocol_faults(void);
/* ss_csr_build preceded by a device-side content check: `fingerprint` (device buffer of SS_CSR_FINGERPRINT_BYTES, zeroed by the
 * caller before its first use and tied to THESE output buffers) holds two 64-bit sums over the edge list the outputs were last
 * built from; when the sums of (src, dst) agree every kernel of the build exits at once, otherwise the build runs and the sums are
 * replaced.  ELPH.forward (models/elph.py:186) concatenates the same self-looped edge_index into a fresh tensor every training
 * step: its CSR costs one 41 MB streaming pass instead of a rebuild.  No host synchronisation. */
#define SS_CSR_FINGERPRINT_BYTES 8448
int ss_csr_build_cached(const int64_t *src, const int64_t *dst, int64_t E, int64_t N, int64_t *rowptr, int32_t *col,
                        int64_t *n_self_loops_out, int32_t hub_threshold, int32_t *hub_rows, int32_t *hub_count,
                        int32_t *mega_rows, int32_t *mega_count, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                        void *fingerprint, void *stream);

/* One hop of sketch propagation over a CSR: out[i] = min (MinHash) / max (HLL) over the in-neighbours
 * of i, plus row i itself when i < n_self_loops (the implicit self loops of add_self_loops,
 * hashing.py:148); rows with no in-edge and no self loop are all-zero (PyG scatter default).
 * Replaces MinhashPropagation.forward / HllPropagation.forward (hashing.py:28-45) and, when
 * cards_out != NULL, the hll_count of hashing.py:163 (cards_out[i*cards_stride] = hll_count(out row)).
 * Either sketch may be NULL (both in and out). */
int ss_propagate(const ss_csr_graph *graph, const uint32_t *mh_in, uint32_t *mh_out, int32_t P,
                 const uint8_t *hll_in, uint8_t *hll_out, int32_t M,
                 float *cards_out, int64_t cards_stride, const ss_hll_params *prm, void *stream);

/* The MinHash half of ss_propagate for a LIST of destination rows: mh_out[r] = min over the in-neighbours of r (and r itself,
 * as above) for every r in rows[0 .. n_rows) -- ids may repeat, negative ids count from the end (torch indexing), ids outside
 * [-N, N) are ignored -- plus every hub row of the graph (the hub units always cover all of them); all other rows
 * of mh_out are left untouched.  For the caller whose next step reads only a few rows of the hop's table: ELPH's training
 * step (models/elph.py:209-212 followed by runners/train.py:204) propagates over the whole graph and then queries two rows
 * per link of ONE batch; the host mirror defers the last minhash_prop (hashing.py:28-35) and computes the batch's rows
 * through this entry point -- same values, 2 B instead of N rows. */
int ss_minhash_hop_rows(const ss_csr_graph *graph, const uint32_t *mh_in, uint32_t *mh_out, int32_t P, const int64_t *rows,
                        int64_t n_rows, void *stream);

/* Hop 1 straight from node ids: equivalent to ss_minhash_init + ss_hll_init + one ss_propagate
 * (hashing.py:118-137, 28-45 at k = 1, 163) but the hop-0 rows -- pure functions of the node id -- are
 * recomputed in registers instead of being written to and re-read from HBM.  a / b: device uint64[P].
 * Returns SS_ERR_UNSUPPORTED when (P, p) is outside the fused kernel's shape (p == 8, P % 64 == 0, P <= 256):
 * the caller then uses the three-call sequence. */
int ss_first_hop(const ss_csr_graph *graph, const uint64_t *a, const uint64_t *b, int32_t P,
                 uint32_t *mh_out, int32_t p, uint8_t *hll_out, float *cards_out, int64_t cards_stride,
                 const ss_hll_params *prm, void *stream);

/* Hops 1 and 2 of a build in one call: the hop-1 MinHash rows (from node ids), the hop-2 HLL rows + their cardinalities and --
 * when mh2_out is given (P == 128) -- the hop-2 MinHash rows; with cards1_out != NULL also the hop-1 HLL rows (`hll1` is then an
 * OUTPUT, cards1_out[i * cards_stride] their cardinalities), with cards1_out == NULL `hll1` is the COMPLETE hop-1 HLL table as
 * input.  Same results as ss_first_hop + ss_propagate (hashing.py:118-137, 28-45 at k = 1, 2, 163), but the VALU-bound MinHash first
 * hop and the memory-bound HLL table hop of hop 2 run interleaved inside one launch (csrc/ss_fused_hop.hip).  cards2_out:
 * nullable unless cards1_out is given.  Returns SS_ERR_UNSUPPORTED outside p == 8, P % 64 == 0, P <= 256: the caller then uses the
 * unfused calls. */
int ss_fused_hop_stage(const ss_csr_graph *graph, const uint64_t *a, const uint64_t *b, int32_t P, uint32_t *mh1_out,
                       uint32_t *mh2_out, int32_t p, uint8_t *hll1, float *cards1_out, uint8_t *hll2_out, float *cards2_out,
                       int64_t cards_stride, const ss_hll_params *prm, void *stream);

/* ss_fused_hop_stage with a workspace for the RECORDS form of its fused kernel (csrc/ss_fused_hop.hip): records, device uint32[N][16]
 * (nullable: then this is ss_fused_hop_stage), and num_edges = E, the length of graph->col (negative: unknown).  Where the stage
 * computes the hop-1 HLL table itself (cards1_out != NULL) for the whole graph on one device, the table fits a buffer descriptor
 * and the graph lists no hub rows (hub_rows == NULL) and E + N <= 24 * N, the HLL first hop also writes a 64-byte code record per node -- dword l = code(l) | code(l + 16) << 16 of the
 * node's neighbours l and l + 16 (its own id among them as the implicit self loop), code = register << 2 | rank << 10, 0 = none;
 * 0xFFFFFFFF in every dword of a node with more than 32 neighbours or a hub row: "read the dense row" -- and the fused kernel builds
 * the hop-2 HLL rows by scatter-max of those codes instead of folding dense 256-byte rows.  Same tables and cardinalities, bit for
 * bit; `records` holds the records afterwards (contents unspecified where the dense form ran).  SS_FUSED_RECORDS in the environment,
 * read at every call: 0 forces the dense form, 1 the records form wherever it is legal whatever E. */
int ss_fused_hop_stage_records(const ss_csr_graph *graph, const uint64_t *a, const uint64_t *b, int32_t P, uint32_t *mh1_out,
                               uint32_t *mh2_out, int32_t p, uint8_t *hll1, float *cards1_out, uint8_t *hll2_out, float *cards2_out,
                               int64_t cards_stride, const ss_hll_params *prm, uint32_t *records, int64_t num_edges, void *stream);

/* HLL++ cardinality of n register rows.  Replaces ElphHashes.hll_count (+ _linearcounting,
 * _estimate_bias, _refine_hll_count_estimate; hashing.py:194-232).  regs: device uint8[n, m];
 * out: device fp32, element i written to out[i*out_stride]. */
int ss_hll_count(const uint8_t *regs, int64_t n, const ss_hll_params *prm, float *out, int64_t out_stride,
                 void *stream);

/* The two estimator helpers the reference exposes on their own.  e: device fp32[n] raw estimates.
 *   refine == 0: out[i] = mean bias of the 6 nearest table entries   (_estimate_bias, hashing.py:197-204)
 *   refine != 0: out[i] = e[i] <= 5m ? e[i] - that bias : e[i]       (_refine_hll_count_estimate, :206-210) */
int ss_estimate_bias(const float *e, int64_t n, const ss_hll_params *prm, float *out, int32_t refine, void *stream);

/* Subgraph features of B node pairs.  Replaces ElphHashes._get_intersections + jaccard + _hll_merge +
 * get_subgraph_features for one chunk (hashing.py:167-189, 234-237, 247-256, 258-323).
 *   links: device int64[B,2]; negative ids wrap like torch indexing; ids outside [-N, N) set *err_flag
 *          (device int32, may be NULL) and produce NaN rows.
 *   mh / hll: HOST arrays of h device pointers, entry k-1 = hop-k table (k = 1..h).
 *   cards: device fp32, cards[i*cards_stride + k-1] = hop-k cardinality of node i.
 *   out: device fp32 [B, h(h+2)], feature order = LABEL_LOOKUP[h] (hashing.py:22-25).
 *   dbg_match / dbg_zero (device int32[B,h*h], nullable): MinHash match counts and union zero-register
 *   counts per (k1,k2) row-major; dbg_inter (device fp32[B,h*h], nullable): the intersections J*U. */
int ss_pair_features(const int64_t *links, int64_t B, int64_t N, int32_t h,
                     const uint32_t *const *mh, int32_t P, const uint8_t *const *hll,
                     const float *cards, int64_t cards_stride, const ss_hll_params *prm, uint32_t flags,
                     float *out, int32_t *dbg_match, int32_t *dbg_zero, float *dbg_inter, int32_t *err_flag,
                     void *stream);

/* The same features with BUDDY's degree-normalised copy appended (next row of the scope table: replaces
 * BUDDY._append_degree_normalised, models/elph.py:276-293, fed by HashDataset.degrees, datasets/elph.py:74).
 *   degrees: device fp32[N];  out: device fp32 [B, 2*h(h+2)]: columns [0, h(h+2)) as ss_pair_features, columns
 *   [h(h+2), 2h(h+2)) = feature / sqrt(degrees[u] * degrees[v]) with NaN and Inf (zero-degree nodes) replaced by 0. */
int ss_pair_features_normalised(const int64_t *links, int64_t B, int64_t N, int32_t h,
                                const uint32_t *const *mh, int32_t P, const uint8_t *const *hll,
                                const float *cards, int64_t cards_stride, const ss_hll_params *prm, uint32_t flags,
                                const float *degrees, float *out, int32_t *err_flag, void *stream);

/* The query exploiting LINK LOCALITY (BUDDY's precompute IS the query at ogbl-ppa / citation2 scale: datasets/elph.py:207-208
 * hands get_subgraph_features every link of a split; hashing.py:270-274, :180-183 read the rows of u and v once per pair, yet
 * the link sets repeat every source many times -- ogbl-citation2's evaluation set lists 1 000 negatives per source).
 *   ss_group_links_by_source: order[0 .. B) := a permutation of the pair indices in which all pairs with the same first node
 *     are consecutive (torch-style negative ids wrapped; ids out of range are keyed to node 0 -- nothing is dropped, the query
 *     reports them).  rowptr: int64[N + 1] scratch output (start of every node's group).  Workspace:
 *     ss_csr_workspace_bytes(N, B).  B < 2^31.
 *   ss_pair_features_grouped: ss_pair_features / ss_pair_features_normalised (degrees non-null) walking the pairs in the order
 *     given (order == NULL: as listed) and re-reading the rows of a first node only when it changes.  Row q of `out` is pair
 *     q; rows are bit-identical to the ungrouped entry points' (a pair's features depend on its own rows only). */
int ss_group_links_by_source(const int64_t *links, int64_t B, int64_t N, int32_t *order, int64_t *rowptr, void *workspace,
                             size_t workspace_bytes, void *stream);
/* The two permutations around a grouped query over a link set of gigabytes (the features of ogbl-citation2's 356 M links are
 * 21 GB): out_links[t] := links[order[t]] (int64 [n, 2]) before, out[order[t], :] := rows[t, :] (float [n, width]) after a
 * ss_pair_features_grouped(order = NULL) over the gathered chunk -- walking `order` inside the query would make every pair
 * read and write at random places of those arrays from inside its latency chain. */
/* (links and out_links must be 16-byte aligned -- a pair moves as one vector --: SS_ERR_INVALID_ARG otherwise.  `order` entries are
 * NOT validated by any of these calls: each must lie in [0, n) of the array it indexes, as ss_group_links_by_source produces them) */
int ss_gather_links(const int64_t *links, const int32_t *order, int64_t n, int64_t *out_links, void *stream);
int ss_scatter_feature_rows(const float *rows, const int32_t *order, int64_t n, int32_t width, float *out, void *stream);
int ss_pair_features_grouped(const int64_t *links, const int32_t *order, int64_t B, int64_t N, int32_t h,
                             const uint32_t *const *mh, int32_t P, const uint8_t *const *hll,
                             const float *cards, int64_t cards_stride, const ss_hll_params *prm, uint32_t flags,
                             const float *degrees, float *out, int32_t *err_flag, void *stream);

/* One score per pair instead of its feature row: the structure-feature head both reference models put behind the row --
 * x = relu(bn_labels(label_lin_layer(sf))), then the label branch's columns of lin (models/elph.py:73-86 LinkPredictor.forward,
 * :324-352 BUDDY.forward) -- computed by the 16 lanes that have just assembled the row, which is never written.  Inference only:
 * BatchNorm in eval mode, folded into the linear layer by the caller:
 *     out[q] = bias + sum_j w2[j] * max(0, shift[j] + sum_i w1[j * dim + i] * x_q[i]),
 *   x_q = the row ss_pair_features (normalised == 0, dim = h(h+2)) or ss_pair_features_normalised (normalised != 0, dim = 2h(h+2),
 *   degrees required; without `normalised` degrees must be NULL) writes for pair q.  Sums run i ascending through fmaf, hidden
 *   units in a fixed tree: a pair's score is bit-identical whatever B, `order` or the launch.
 *   w1 [dim, dim] / shift [dim] / w2 [dim]: device fp32.  order (nullable): as ss_pair_features_grouped.  out: device fp32 [B],
 *   out[q] = pair q whatever the order; an id outside [-N, N) sets *err_flag (nullable) and gives NaN. */
typedef struct ss_structure_head {
    int32_t dim;
    int32_t normalised;
    const float *w1;
    const float *shift;
    const float *w2;
    float bias;
} ss_structure_head;
int ss_pair_scores(const int64_t *links, const int32_t *order, int64_t B, int64_t N, int32_t h, const uint32_t *const *mh, int32_t P,
                   const uint8_t *const *hll, const float *cards, int64_t cards_stride, const ss_hll_params *prm, uint32_t flags,
                   const float *degrees, const ss_structure_head *head, float *out, int32_t *err_flag, void *stream);

/* Weighted common-neighbour scores of node pairs -- the other per-link precompute of HashDataset.__init__ (SURVEY 8(f)
 * row N4; reference datasets/elph.py:76-77,314 calling heuristics.py:51-70 RA; CN heuristics.py:10-27 and AA :30-48
 * are the same sum with another multiplier):
 *     out[q] = (float) sum_w A[u, w] * (A[v, w] * mult[w]),   (u, v) = links[q],
 *   in fp64 (what scipy does for int, bool and float64 matrices): products and sum in fp64, one float32 rounding.
 *   rowptr / col / val: device CSR of A (int64[N+1], int32[nnz] SORTED and duplicate-free inside a row -- what
 *   scipy.sparse.csr_matrix((w, (row, col))) holds after sum_duplicates/sort_indices --, double[nnz] or NULL = all 1);
 *   mult: device double[N] or NULL (= 1: common neighbours).  links: device int64[B, 2]; out: device fp32[B].
 *   err_flag (nullable): set to 1 when a link refers to a node outside [0, N) (its score is written as 0). */
int ss_common_neighbour_scores(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult,
                               int64_t N, const int64_t *links, int64_t B, float *out, int32_t *err_flag, void *stream);
/* The same scores in scipy's float32 arithmetic (float32 matrices): val and mult hold float32 values (exact in double); each
 * term is f32(a_u * a_v) (mult NULL) or f32(a_u * f32(a_v * mult[w])), terms equal to 0 are dropped, and the m terms of a pair,
 * in ascending column order, are added as t[0] + pairwise(t[1:]) in numpy's float32 pairwise order (CSR row sum through
 * np.add.reduceat): bit-identical to the reference on float32 matrices.  Arguments and errors as above. */
int ss_common_neighbour_scores_f32(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult,
                                   int64_t N, const int64_t *links, int64_t B, float *out, int32_t *err_flag, void *stream);

/* The common neighbours themselves, and node features pooled over them (csrc/ss_cn_pool.hip).  The common neighbours of
 * (u, v) = links[q] are the columns STORED in both row u and row v of the CSR above (a stored zero counts), ascending;
 * member w carries the coefficient
 *     c(q, w) = (float)( A[u, w] * (A[v, w] * mult[w]) )      fp64 with this association (the term of
 *   ss_common_neighbour_scores), rounded once -- for every matrix dtype; there is no float32 mode here.
 *   rowptr / col / val / mult / links / err_flag: as ss_common_neighbour_scores (val NULL = all 1, mult NULL = 1).  A link
 *   with an id outside [0, N) has no common neighbours (count 0, nothing filled, a pooled row of +0.0) and sets *err_flag.
 *     ss_common_neighbour_count  counts[q] = the number of common neighbours of link q (device int64[B])
 *     ss_common_neighbour_fill   ids[offsets[q] + k] = the k-th common neighbour of link q, coef[offsets[q] + k] = its
 *                                coefficient (coef NULL: ids only).  offsets: device int64[B], the exclusive prefix sum of the
 *                                counts of THESE links; ids device int64[T], coef device fp32[T], T = the sum of the counts.
 *                                Exactly [offsets[q], offsets[q] + counts[q]) is written for every q.
 *     ss_common_neighbour_pool   out[q, :] = sum over the common neighbours w of link q, ascending, of c(q, w) * x[w, :]:
 *                                fp32 from +0.0, product and sum rounded separately, each element accumulated by one lane in
 *                                that order -- a row's bits do not depend on B, the launch, or which of the two rows is longer.
 *                                x: device fp32 [N, F] row-major, out: device fp32 [B, F] (every row written; 64-bit offsets),
 *                                F >= 0; float4 accesses when F % 4 == 0 and x and out are 16-byte aligned, scalar ones
 *                                otherwise.  No float atomics, no workspace. */
int ss_common_neighbour_count(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *links, int64_t B, int64_t *counts,
                              int32_t *err_flag, void *stream);
int ss_common_neighbour_fill(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult, int64_t N,
                             const int64_t *links, int64_t B, const int64_t *offsets, int64_t *ids, float *coef, int32_t *err_flag,
                             void *stream);
int ss_common_neighbour_pool(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult, int64_t N,
                             const int64_t *links, int64_t B, const float *x, int32_t F, float *out, int32_t *err_flag, void *stream);

/* Personalised PageRank of many sources at once -- the fourth link heuristic (reference heuristics.py:74-113: PPR, one
 * fast_pagerank.pagerank_power(A, p, personalize=e_src, tol) power iteration per distinct source).  With r = row sums of A,
 * n = N, s_j = n e_src_j and z_u = ((1-p)[r_u != 0] + [r_u == 0]) / n, every source column j iterates
 *     x <- W x + s_j (z . x),   W[v, u] = (p A[u, v]) (1 / r_u)  (rows with r_u = 0 drop out),   x_0 = s_j
 * until ||x - x_old||_2 <= tol or max_iter steps, and its result is x / sum(x).  fp64 throughout; bit-identical for a source
 * whatever S or the column it occupies (every sum runs in an order fixed by the graph).
 *   ss_ppr_graph: device CSR of A^T (row v lists the u with A[u, v] != 0) with the weights w above, z[N], and the rows
 *   holding more than SS_PPR_SEGMENT entries ("hubs", ascending) cut into segments of SS_PPR_SEGMENT entries:
 *   hub_seg[h] .. hub_seg[h + 1] are the segments of hub_rows[h], seg_hub[s] the hub segment s belongs to.
 *   Workspace (iterates, per-block partials, per-column state): ss_ppr_workspace_bytes(N, S, n_hubs, n_segments) device
 *   bytes, 0 = unsupported size; S <= SS_PPR_MAX_COLUMNS.  One batch:
 *     ss_ppr_begin    x_0 of the S sources (device int64[S]); an id outside [0, N) sets err_flag (nullable)
 *     ss_ppr_iterate  step `iteration` (1, 2, ...) of every column still active; a column that stops keeps its iterate
 *     ss_ppr_status   iters (device int32[S], nullable) = steps taken, n_active (device int32, nullable) = columns left
 *     ss_ppr_scores   out[l] = (float)(x_c[dst[l]] / sum x_c), c = link_col[l] -- the reference's ppr[dst]
 *     ss_ppr_vectors  out [S, N] fp64 = the normalised vectors */
#define SS_PPR_SEGMENT 256
#define SS_PPR_MAX_COLUMNS 4096
typedef struct ss_ppr_graph {
    const int64_t *rowptr;    /* int64[N + 1] */
    const int32_t *col;       /* int32[nnz] */
    const double *w;          /* double[nnz] */
    const double *z;          /* double[N] */
    int64_t num_nodes;
    int64_t nnz;
    const int32_t *hub_rows;  /* int32[n_hubs] */
    const int32_t *hub_seg;   /* int32[n_hubs + 1] */
    const int32_t *seg_hub;   /* int32[n_segments] */
    int64_t n_hubs;
    int64_t n_segments;
} ss_ppr_graph;
size_t ss_ppr_workspace_bytes(int64_t N, int32_t S, int64_t n_hubs, int64_t n_segments);
int ss_ppr_begin(const ss_ppr_graph *g, const int64_t *sources, int32_t S, double tol, void *workspace, size_t workspace_bytes,
                 int32_t *err_flag, void *stream);
int ss_ppr_iterate(const ss_ppr_graph *g, int32_t S, int32_t iteration, int32_t max_iter, double tol, void *workspace,
                   size_t workspace_bytes, void *stream);
int ss_ppr_status(const ss_ppr_graph *g, int32_t S, const void *workspace, size_t workspace_bytes, int32_t *iters, int32_t *n_active,
                  void *stream);
int ss_ppr_scores(const ss_ppr_graph *g, int32_t S, const int64_t *dst, const int32_t *link_col, int64_t L, const void *workspace,
                  size_t workspace_bytes, float *out, int32_t *err_flag, void *stream);
int ss_ppr_vectors(const ss_ppr_graph *g, int32_t S, const void *workspace, size_t workspace_bytes, double *out, void *stream);

/* One-vs-all link candidates: the set-intersection estimate I[k1, k2] = J * U (reference hashing.py:167-189) of S sources
 * against every node, as ranking keys for a top-k selection -- the operation the reference's sample_hard_negatives
 * (src/data.py:262-304) sets out to do and full-ranking evaluation / candidate generation need.
 *   ss_topk_scan     keys [S, N] int64: keys[s][v] ranks v for sources[s] (device int64[S], torch-style negative ids wrapped;
 *                    an id outside [-N, N) sets err_flag (nullable) and its row is all sentinels).  mh_src / hll_src: the
 *                    hop-k1 tables, mh_cand / hll_cand: the hop-k2 tables (packed [N, P] / [N, 2^p]).  The score is
 *                    bit-identical to ss_pair_features' dbg_inter[(k1, k2)] for the pair (u, v) (-0 becomes +0).
 *                    Key = (monotone score bits as signed int32) << 32 | (0xFFFFFFFF - v): signed order == (score desc, id
 *                    asc); v == u holds INT64_MIN, below every real key.  N < 2^32 - 1.
 *   ss_topk_exclude  INT64_MIN over keys[s][v] for every v in row u of a CSR (rowptr int64[N + 1], col int32) -- the CSR of
 *                    the exclude list flipped (ss_csr_build lists row i = {j : j -> i}), so row u = {v : u -> v}.
 * Workspace: the key buffer, ss_topk_workspace_bytes(N, S) device bytes (0 = unsupported size). */
size_t ss_topk_workspace_bytes(int64_t N, int32_t S);
int ss_topk_scan(const int64_t *sources, int32_t S, int64_t N, const uint32_t *mh_src, const uint8_t *hll_src, const uint32_t *mh_cand,
                 const uint8_t *hll_cand, int32_t P, const ss_hll_params *prm, int64_t *keys, size_t keys_bytes, int32_t *err_flag,
                 void *stream);
int ss_topk_exclude(const int64_t *sources, int32_t S, int64_t N, const int64_t *rowptr, const int32_t *col, int64_t *keys,
                    size_t keys_bytes, void *stream);

/* One-vs-all link candidates ranked by the structure head: keys[s][v] ranks v for sources[s] by the score ss_pair_scores gives
 * the pair (sources[s], v) -- the source first, the row is not symmetric -- bit for bit (-0 becomes +0): all h^2 intersection
 * estimates, the feature row of ss_pair_features[_normalised] (same flags, cards, degrees), then the head, the row never written.
 * Arguments as ss_pair_scores takes them (head->dim = h(h+2), or 2h(h+2) with head->normalised, which requires degrees; without
 * it degrees must be NULL) and as ss_topk_scan does (keys [S, N] int64 of ss_topk_workspace_bytes(N, S) bytes, the same key
 * encoding and sentinel, N < 2^32 - 1, err_flag set by an id outside [-N, N), whose row is all sentinels).  ss_topk_exclude
 * applies an exclude list to these keys as it does to ss_topk_scan's. */
int ss_topk_score_scan(const int64_t *sources, int32_t S, int64_t N, int32_t h, const uint32_t *const *mh, const uint8_t *const *hll,
                       int32_t P, const float *cards, int64_t cards_stride, const ss_hll_params *prm, uint32_t flags,
                       const float *degrees, const ss_structure_head *head, int64_t *keys, size_t keys_bytes, int32_t *err_flag,
                       void *stream);

/* Each link's exact rank among all nodes by the structure head -- what MRR / Hits@K of positive links over all N candidates need
 * (reference src/evaluation.py ranks a positive among sampled negatives): for link q = (u, t) = links[q] and every node v other
 * than u and t, the score ss_pair_scores gives the pair (u, v), bit for bit, is compared with thr[q] and COUNTED:
 *     counts[q][0] += #{v : s(u, v) >  thr[q]},     counts[q][1] += #{v : s(u, v) == thr[q]}     (float compares: -0 == +0).
 *   links: device int64 [L, 2] (torch-style negative ids wrapped; a link with an id outside [-N, N) sets err_flag, nullable, and
 *   adds nothing).  thr: device fp32 [L], what ss_pair_scores wrote for the same links with the same arguments -- the scan holds no
 *   second form of the score, so thr[q] compares exactly with s(u, t).  counts: device int64 [L, 2], ZEROED by the caller: the
 *   workgroups of the launch add into it with 64-bit integer atomics, nothing else is stored, and the sums do not depend on the
 *   grid.  Every other argument as ss_topk_score_scan takes it.  N < 2^32; L <= 8 * 65535 per launch.  An exclude list is the
 *   caller's correction: subtract the comparisons of ss_pair_scores over the excluded pairs (ElphHashes.rank_links). */
int ss_rank_score_scan(const int64_t *links, const float *thr, int32_t L, int64_t N, int32_t h, const uint32_t *const *mh,
                       const uint8_t *const *hll, int32_t P, const float *cards, int64_t cards_stride, const ss_hll_params *prm,
                       uint32_t flags, const float *degrees, const ss_structure_head *head, int64_t *counts, int32_t *err_flag,
                       void *stream);

/* Locality-sensitive hashing by banding over ONE hop's packed MinHash table mh [N, P]: sub-linear link candidates for the workloads
 * that ask "who are the best partners of u" for many sources (hard-negative mining -- the reference's sample_hard_negatives,
 * src/data.py:262-304 --, candidate generation, a kNN graph), where the one-vs-all scans above score all N nodes per source.
 * Band j of node v is mh[v][j * rows .. (j + 1) * rows), j < bands, rows * bands <= P; the bucket of (j, v) is the set of nodes whose
 * band-j slice equals v's value for value.  N < 2^31, P a multiple of 4 in [4, 2048], 1 <= key_bits <= 64.
 *   ss_lsh_band_keys  keys [bands, N] int64: keys[j][v] = a 64-bit mix of band j of v, its low key_bits bits kept (64: all; fewer
 *                     only makes false matches, for tests).  The caller sorts every band (signed int64 order) and keeps the sorted
 *                     keys and the permutation perm [bands, N] int32 (perm[j][i] = the node at place i of band j).
 *   ss_lsh_count      counts [S * bands] int32: counts[s * bands + j] = the nodes v != u that share band j with u = sources[s]
 *                     (device int64 [S], torch-style negative ids wrapped; an id outside [-N, N) sets err_flag, nullable, and counts
 *                     nothing): the equal range of u's key in the sorted keys of band j by binary search; a range longer than
 *                     max_bucket is dropped whole; else every member's `rows` values are compared with u's own, so the result does
 *                     not depend on the mix or on key_bits.
 *   ss_lsh_fill       the same walk with the same arguments, writing the entries s * N + v (int64) of item s * bands + j from
 *                     out[offsets[s * bands + j]] on, offsets = the exclusive scan of ss_lsh_count's counts (device int64), in no
 *                     particular order inside an item; a node sharing several bands with u is listed once per band. */
int ss_lsh_band_keys(const uint32_t *mh, int64_t N, int32_t P, int32_t rows, int32_t bands, int32_t key_bits, int64_t *keys, void *stream);
int ss_lsh_count(const int64_t *sources, int32_t S, int64_t N, const uint32_t *mh, int32_t P, int32_t rows, int32_t bands, int32_t key_bits,
                 const int64_t *keys, const int32_t *perm, int32_t max_bucket, int32_t *counts, int32_t *err_flag, void *stream);
int ss_lsh_fill(const int64_t *sources, int32_t S, int64_t N, const uint32_t *mh, int32_t P, int32_t rows, int32_t bands, int32_t key_bits,
                const int64_t *keys, const int32_t *perm, int32_t max_bucket, const int64_t *offsets, int64_t *out, void *stream);

/* Negative links drawn on the device, O(1) per negative, fresh per seed: what the reference takes once, on the CPU, from PyG's
 * negative_sampling (src/data.py:199-217) and get_same_source_negs (src/utils.py:88-99, unfiltered there), and what its unfinished
 * sample_hard_negatives (src/data.py:262-304: non-edges with a common neighbour) wanted.
 * rowptr [N + 1] int64 / col int32: row u = {v : u -> v}, every row SORTED ascending (ss_csr_sort_rows), duplicates kept; ex_rowptr /
 * ex_col: a second such CSR of pairs that must not come back either (both null: none).  N < 2^31.
 * Slot t < n_slots of the call is slot q = first_slot + t of the whole job and belongs to positive q / num_neg; sources (device int64,
 * element stride source_stride, torch-style negative ids wrapped) points at the source of the positive of slot first_slot, null for
 * any-source sampling (SS_NEG_UNIFORM only).  Attempt a = 0 .. max_tries - 1 (max_tries in [1, SS_NEG_MAX_TRIES]) of slot q draws
 *     r_c = hash(hash(seed ^ hash(q + 1)) + 0x9E3779B97F4A7C15 * (2 a + c + 1)),  c = 0, 1   (hash: the splitmix64 finaliser, mod 2^64)
 * and proposes, with hi(r n) the high 64 bits of r * n:
 *     SS_NEG_UNIFORM      u = the source, or hi(r_0 N) without sources;  v = hi(r_1 N)
 *     SS_NEG_SAME_SOURCE  u = the source;                                v = hi(r_1 N)
 *     SS_NEG_WEDGE        u = the source;  w = row_u[hi(r_0 deg u)];  v = row_w[hi(r_1 deg w)]   (deg u == 0: no attempt is made;
 *                         deg w == 0: the attempt is rejected) -- v is proposed with probability sum_w 1 / (deg u * deg w) over the
 *                         paths u -> w -> v, multiplicities counted: proportional to the resource-allocation score of (u, v)
 * The first attempt with v != u and u -> v in neither CSR gives out[t] = (u, v); none: (u, -1) (any-source: the u of the last attempt),
 * and *unsampled (device int32, nullable, NOT cleared by the call) counts the slot -- one atomic per wavefront.  A source outside
 * [-N, N) sets err_flag (nullable), leaves (the id as given, -1) and is counted too.  out: device int64 [n_slots, 2], 16-byte aligned.
 * A slot depends on (seed, q) and the two CSRs only: a job split into calls by first_slot reproduces the unsplit one; different slots
 * may return the same pair.  Argument errors (SS_ERR_INVALID_ARG) are detected before any launch; n_slots == 0: SS_OK, no launch. */
#define SS_NEG_UNIFORM 0
#define SS_NEG_SAME_SOURCE 1
#define SS_NEG_WEDGE 2
#define SS_NEG_MAX_TRIES 64
int ss_sample_negatives(const int64_t *rowptr, const int32_t *col, const int64_t *ex_rowptr, const int32_t *ex_col, int64_t N,
                        const int64_t *sources, int64_t source_stride, int64_t n_slots, int32_t num_neg, int32_t mode, uint64_t seed,
                        int32_t max_tries, int64_t first_slot, int64_t *out, int32_t *unsampled, int32_t *err_flag, void *stream);

/* Exact two-hop link candidates: the rows `sources` of A * A with integer walk counts, over the same sorted CSR (row u = {v : u -> v},
 * duplicates kept, N < 2^31).  A walk of u is u -> w -> v, w in row u, v in row w, every copy of a repeated edge its own walk;
 * W(u) = the sum of deg(w) over w in row u.  sources: device int64 [S], torch-style negative ids wrapped, S < 2^31.
 *   ss_wedge_walks  walks[s] = W(sources[s]) (device int64 [S]); an id outside [-N, N) sets err_flag (nullable) and has 0 walks.
 *   ss_wedge_fold   the LDS tier: every source with 0 < 2 * walks[s] <= slots (a power of two <= SS_WEDGE_MAX_SLOTS) writes its D
 *                   distinct endpoints as keys[offsets[s] + i] = s * N + v, counts[..] = the walks that end in v, i < D, in no
 *                   particular order, and pads the places D .. walks[s] - 1 of its slot with key INT64_MAX / count 0.
 *   ss_wedge_emit   the large tier: every source with 2 * walks[s] > slots writes the endpoint s * N + v of each of its walks to
 *                   keys[offsets[s] .. offsets[s] + walks[s]) (w ascending in row u, then v ascending in row w); `slices` in [1, 64]
 *                   workgroups share a source's row.  Counts are not written: one walk each.
 * walks: what ss_wedge_walks returned with the sources to leave out set to 0; offsets: its exclusive scan (device int64 [S]); keys
 * int64 / counts int32 hold sum(walks) entries.  The two launches cover every source with walks > 0 exactly once, and no store leaves
 * a source's slot.  Argument errors (SS_ERR_INVALID_ARG) are detected before any launch; S == 0: SS_OK, no launch. */
#define SS_WEDGE_MAX_SLOTS 4096
int ss_wedge_walks(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S, int64_t *walks, int32_t *err_flag,
                   void *stream);
int ss_wedge_fold(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S, const int64_t *walks,
                  const int64_t *offsets, int32_t slots, int64_t *keys, int32_t *counts, void *stream);
int ss_wedge_emit(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S, const int64_t *walks,
                  const int64_t *offsets, int32_t slots, int32_t slices, int64_t *keys, void *stream);

/* Exact subgraph features: what get_subgraph_features (reference hashing.py:258-323) would return if its estimators were exact.
 * The ball B_k(x) of G' -- the graph build_hash_tables propagates over (hashing.py:139-165: the edges of the CSR, flow source ->
 * target, plus a self loop at every x < n_self, the graph's n_self_loops / n_self_loops_dev, i.e. add_self_loops without num_nodes,
 * hashing.py:148) -- is B_0(x) = {x}, B_k(x) = U_{(j -> x) in G'} B_{k-1}(j).  For a pair (u, v) and 1 <= k1, k2, k <= h:
 *   I[k1][k2] = |B_k1(u) & B_k2(v)|   (what the intersection estimate J * U of hashing.py:167-189 approximates)
 *   balls     = |B_k(u)| then |B_k(v)| (what the HLL++ cards of hashing.py:150-163 approximate)
 *   feats     = the feature algebra of hashing.py:276-320 (flags: SS_FLAG_USE_ZERO_ONE / SS_FLAG_FLOOR_SF) on float(I), float(balls):
 *               exact integers in fp32 for N < 2^20.
 * links: device int64 [B, 2] (torch-style negative ids wrapped; a pair with an id outside [-N, N) gets NaN features and zero counts
 * and sets err_flag, nullable).  I int32 [B, h, h] and balls int32 [B, 2, h] are nullable, feats fp32 [B, h(h+2)] is not.
 *   ss_exact_pairs  the on-chip tier: one workgroup per pair, both BFSs in one LDS hash table.  A pair whose union of balls has more
 *                   than lds_max_nodes nodes (at most the table's own bound; 0 = every pair) is left to the large tier: its index
 *                   goes to the overflow list of the workspace (ss_exact_workspace_bytes(B) device bytes; the call clears its counters).
 *   ss_exact_large  the large tier over that list, on the same stream after ss_exact_pairs with the same arguments: `slots`
 *                   persistent workgroups, each owning ss_exact_slot_bytes(N) bytes of `arena` (dense distance bytes + visit lists),
 *                   which must be all zero at the first call and are left all zero by every call.
 * Both return SS_ERR_UNSUPPORTED for h outside [1, 3], SS_ERR_INVALID_ARG for negative sizes or null pointers, SS_OK for B == 0
 * (before any launch), and need N < 2^31 and graph->num_nodes == N.
 * flags & SS_FLAG_MASK_TARGET (both calls alike): every pair is counted in the graph without every copy of u -> v and of v -> u -- the
 * target-link removal of the reference's SEAL path (src/datasets/seal.py:338), the exact counterpart of ss_masked_pair_features; n_self
 * and the self loops stay as they are.  The BFS leaves the partner out when it expands the root, nothing else changes. */
size_t ss_exact_workspace_bytes(int64_t B);
size_t ss_exact_slot_bytes(int64_t N);
int ss_exact_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags, int32_t lds_max_nodes,
                   int32_t *I, int32_t *balls, float *feats, int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream);
int ss_exact_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags, int32_t *I,
                   int32_t *balls, float *feats, void *workspace, size_t workspace_bytes, int32_t slots, void *arena, size_t arena_bytes,
                   void *stream);

/* Exact subgraph node lists: per pair (u, v) every node x of B_h(u) | B_h(v), ascending by id and once each, with the distance bytes
 * (d_u(x), d_v(x)) -- the balls, the graph, the links and SS_FLAG_MASK_TARGET as for ss_exact_pairs / ss_exact_large, with ONE
 * difference: a root is always in its own ball at distance 0 (n_self is not consulted), so no union is empty.  A distance is in
 * [0, h]; h + 1 stands for "not within h" and is no distance.  Rows vary in length, so every batch is walked twice with the same
 * workspace (ss_exact_workspace_bytes(B)), arena (ss_exact_slot_bytes(N) per slot; its distance bytes all zero before and after every call, its visit lists scratch) and stream:
 *   count pass (rowptr == NULL)  ss_exact_nodes_pairs writes counts[q] = the size of the union for every pair within lds_max_nodes
 *                                and lists the others in the workspace; ss_exact_nodes_large then counts those.  counts: int32 [B].
 *   fill pass (rowptr != NULL)   rowptr: int64 [B + 1], ascending offsets into ids (int64) / dist (uint8 [.., 2]) made by the caller
 *                                from the counts: rowptr[q + 1] - rowptr[q] is counts[q], or 0 for a pair that is to be left out.
 *                                ss_exact_nodes_pairs writes the rows of length 1 .. lds_max_nodes (the same value as in the count
 *                                pass), ss_exact_nodes_large those of the workspace's list; neither stores outside
 *                                [rowptr[q], rowptr[q + 1]).
 * Return codes and argument checks as ss_exact_pairs / ss_exact_large (B == 0: SS_OK before any launch); counts (count pass) or ids
 * and dist (fill pass) must not be null. */
int ss_exact_nodes_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                         int32_t lds_max_nodes, int32_t *counts, const int64_t *rowptr, int64_t *ids, uint8_t *dist, int32_t *err_flag,
                         void *workspace, size_t workspace_bytes, void *stream);
int ss_exact_nodes_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags, int32_t *counts,
                         const int64_t *rowptr, int64_t *ids, uint8_t *dist, void *workspace, size_t workspace_bytes, int32_t slots,
                         void *arena, size_t arena_bytes, void *stream);

/* Per-hop sampled subgraph node lists: the node row of the reference's k_hop_subgraph with its sample_ratio / max_nodes_per_hop
 * (src/datasets/seal.py:291-348), deterministic in a seed.  ONE joint walk from {u, v} over the in-arcs of the CSR (the target link is
 * not removed; self loops and repeated arcs change nothing; n_self is not consulted):
 *   visited = kept_0 = {u, v} (one root for u == v);  for hop = 1 .. h:
 *     fringe = in-neighbours(kept_{hop-1}) - visited;  visited |= fringe (the WHOLE fringe: a rejected node never comes back);
 *     F = |fringe|;  m = F for ratio_per_hop == 1.0, else (int64)(ratio_per_hop * (double)F);  max_nodes_per_hop > 0: m = min(m, it);
 *     kept_hop = the m fringe nodes with the smallest (key, id);  stop when m == 0
 *   key(x) = H(H(K + 0x9E3779B97F4A7C15 * hop) ^ (x + 1)),  K = H(seed ^ H(((u << 32) | v) + 1)),  H = the splitmix64 finaliser of
 *   ss_minhash_init's node hash, all in wrapping 64-bit words, u and v after the negative-id wrap.
 * The row of a link is the union of the kept, ascending by id and once each, with hop[x] = the hop x was kept at (0 for the roots): a
 * function of (graph, u, v, h, max_nodes_per_hop, ratio_per_hop, seed) alone.  Passes, tiers, workspace, arena (all level bytes zero
 * before and after every call) and stream as for ss_exact_nodes_pairs / ss_exact_nodes_large, with hop (uint8 [T]) for dist and one
 * more array for both passes: state int32 [B], written by the count pass and read by the fill pass (bit 0: some hop of the link
 * dropped a node; bit 1: the link is the slot tier's -- its VISITED set passed lds_max_nodes; counts[q] is the number of kept nodes).
 * Return codes and argument checks as ss_exact_nodes_pairs / ss_exact_nodes_large, and SS_ERR_INVALID_ARG for max_nodes_per_hop < 0
 * (0 = no cap), a ratio_per_hop outside (0, 1] or a seed of 2^63 or more, checked first. */
int ss_sampled_nodes_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, int32_t max_nodes_per_hop,
                           double ratio_per_hop, uint64_t seed, int32_t lds_max_nodes, int32_t *counts, int32_t *state,
                           const int64_t *rowptr, int64_t *ids, uint8_t *hop, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                           void *stream);
int ss_sampled_nodes_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, int32_t max_nodes_per_hop,
                           double ratio_per_hop, uint64_t seed, int32_t *counts, int32_t *state, const int64_t *rowptr, int64_t *ids,
                           uint8_t *hop, void *workspace, size_t workspace_bytes, int32_t slots, void *arena, size_t arena_bytes,
                           void *stream);

/* out = A * x for a row-grouped CSR with fp32 values -- the node-feature propagation of
 * HashDataset._generate_sign_features (reference datasets/elph.py:87-110: gcn_norm, then torch_sparse.spmm = multiply
 * and scatter-add in edge order).  Every output element is accumulated by one lane in CSR order, product and sum rounded
 * separately, so with a CSR made by a STABLE sort of the reference's edge list the result equals the sequential
 * scatter-add bit for bit.  rowptr: device int64[N+1]; col: int32[nnz]; val: fp32[nnz]; x, out: fp32 [N, F], F % 4 == 0. */
int ss_spmm_csr(const int64_t *rowptr, const int32_t *col, const float *val, int64_t N, const float *x, int32_t F,
                float *out, void *stream);

/* The entries of an id array grouped by id (the CSR builder with the entry index as payload): order[0 .. E) = entry indices with
 * equal ids consecutive, rowptr[N + 1] = where each id's group starts; unspecified order inside a group until ss_csr_sort_rows
 * makes it ascending = STABLE.  Ids outside [0, N) (after torch-style negative wrapping) raise err_flag and are keyed to node 0.
 * Workspace: ss_csr_workspace_bytes(N, E).  (reference datasets/elph.py:100-107: gcn_norm's degree sums and torch_sparse.spmm's
 * scatter-add accumulate in edge order -- sign.py groups the edge list by column and by row) */
int ss_csr_group_ids(const int64_t *ids, int64_t E, int64_t N, int32_t *order, int64_t *rowptr, int32_t *err_flag, void *workspace,
                     size_t workspace_bytes, void *stream);
/* every row of a CSR sorted ascending in place; workspace: ss_csr_sort_workspace_bytes(E) device bytes.  only_if (nullable): a
 * device word -- the rows are sorted only if it is non-zero when the launches run */
size_t ss_csr_sort_workspace_bytes(int64_t E);
int ss_csr_sort_rows(const int64_t *rowptr, int32_t *col, int64_t N, int64_t E, const int32_t *only_if, void *workspace, size_t workspace_bytes,
                     void *stream);
/* gcn_norm + torch_sparse.spmm of HashDataset._generate_sign_features (reference datasets/elph.py:100-107) without materialising
 * the normalised edge list [PyG semantics restated: add_remaining_self_loops(fill 1), deg = index_add over col, deg^-1/2 with
 * inf -> 0, norm = dinv[row] * w * dinv[col]].  ss_gcn_scan_edges: one pass over the edge list into `scan` (ss_gcn_scan_bytes(N)
 * device bytes; its first int32 word: some weight differs from 1) -- unit weights? existing self loops per node.  ss_gcn_degree:
 * dinv / loop_w [N] from the grouping by COLUMN (stable unless the weights are all 1: then the degrees are counts);
 * ss_sign_spmm: out = A_norm x from the stable grouping by ROW, every output element accumulated by one lane in edge order
 * (existing self loops skipped, the node's remaining loop last), products and sums rounded separately. */
size_t ss_gcn_scan_bytes(int64_t N);
int ss_gcn_scan_edges(const int64_t *row, const int64_t *col, const float *w, int64_t E, int64_t N, void *scan, void *stream);
int ss_gcn_degree(const int64_t *rowptr_c, const int32_t *order_c, const int64_t *row, const float *w, int64_t N, const void *scan,
                  float *dinv, float *loop_w, void *stream);
int ss_sign_spmm(const int64_t *rowptr_r, const int32_t *order_r, const int64_t *col, const float *w, const float *dinv,
                 const float *loop_w, const void *scan, int64_t N, const float *x, int32_t F, float *out, void *stream);
/* The transposed product: GCNConv's propagation with its default flow (reference models/elph.py:153-160, 214: gcn_norm, then
 * aggregation at the TARGET), out[c] = sum over e with col_e = c, row_e != c of (dinv[row_e] * w_e * dinv[c]) * x[row_e], then
 * + (dinv[c] * loop_w[c] * dinv[c]) * x[c].  rowptr_c / order_c: the STABLE grouping of the edge indices by COLUMN (always sorted:
 * the order inside a group is the accumulation order here); row = edge_index[0]; dinv, loop_w, scan as for ss_sign_spmm, and the
 * same contract: one lane per output element, ascending edge order, the remaining loop last, the norm formed left to right (the
 * bits ss_sign_spmm forms for the same edge), products and sums rounded separately, existing self loops skipped, ids out of range
 * not followed.  Each of the two products is the other's gradient with respect to x.  x, out fp32 [N, F], F % 4 == 0. */
int ss_gcn_spmm_t(const int64_t *rowptr_c, const int32_t *order_c, const int64_t *row, const float *w, const float *dinv,
                  const float *loop_w, const void *scan, int64_t N, const float *x, int32_t F, float *out, void *stream);

/* Unnormalised neighbour aggregation (csrc/ss_aggr.hip; reference models/seal.py:116-173 SEALSAGE, :259-328 SEALGIN, models/gnn.py:90-113
 * SAGE) [PyG semantics restated]: out[dst_e] (+)= w_e * x[src_e] over the edges as they are -- no gcn_norm, existing self loops are
 * ordinary entries, no loop is added, duplicates count once per copy -- for SAGEConv (sum or mean) and GINConv (sum + root term).
 * One grouping serves one product: rowptr / order = the STABLE grouping of the edge indices by the endpoint that receives (always
 * sorted: the order inside a group is the accumulation order), other = the other endpoint of every edge (device int64 [E]),
 * w = the weights (device fp32 [E]) or NULL for unit weights (w is then never gathered; the bits are those of a multiplication by 1).
 * The accumulation order is the contract.  Row i with the entries e_0 < e_1 < ... in chunks of C = ss_aggr_chunk() = 256 (the
 * unit's SS_AGGR_CHUNK define):
 *   p_c = the sequential fp32 sum from +0 of the terms t_e of chunk c, ascending;  s = ((0 + p_0) + p_1) + ...;  no entries: +0
 *   t_e = fl(w_e * v_e),  v_e = x[other_e], or fl(x[other_e] / gather_den[other_e]) when gather_den is given (the mean's backward)
 *   out_i = s,  then fl(s / den[i]) when den is given (the mean),  then + fl(*root * root_x[i]) when root is given (GIN: 1 + eps,
 *   one fp32 word read on the device; root_x is x in the forward and the incoming gradient in the backward)
 * products, quotients (IEEE, correctly rounded) and sums rounded separately; every output element is accumulated by one lane per
 * chunk; no float atomics, no inter-workgroup waits; an id outside [0, N) is not followed.  A row of at most C entries
 * is the plain sequential sum.  Since a row is its chunk sums added in chunk order, its bits do not depend on the tier:
 *   ss_aggr_rows          the regular tier: one row group walks a whole row and stores it; rows of more than hub_entries (>= 1)
 *                         entries are left untouched
 *   ss_aggr_hub_partials  one row group per (hub row, chunk): p_c of chunk g goes to row g of the workspace [n_chunks, F].  hub_rows
 *                         (int32 [n_hubs]) lists the rows of more than hub_entries entries, hub_chunk (int32 [n_hubs + 1]) where each
 *                         hub's chunks start, chunk_hub (int32 [n_chunks]) the hub of every chunk
 *   ss_aggr_hub_finish    per hub row: its partials added in chunk order, the same epilogue (den, root), the row stored
 *   ss_aggr_workspace_bytes(hub_chunks, F) = hub_chunks * F * 4, 0 for a shape that is refused
 *   ss_aggr_degree        den [N]: the same chunked sum over w_e alone (w NULL: the count, exact up to 2^24); 1 for a row without entries
 * x, out, root_x: device fp32 [N, F] row-major, F % 4 == 0, 64-bit offsets.  SS_ERR_INVALID_ARG before any launch for a null pointer
 * (w, gather_den, den, root may be null; root_x only with root), negative sizes, F <= 0, F % 4 != 0, N >= 2^31, hub_entries < 1, a
 * workspace smaller than ss_aggr_workspace_bytes; N == 0 (hub launches: or no chunks / hubs) returns SS_OK without a launch. */
int ss_aggr_chunk(void);
size_t ss_aggr_workspace_bytes(int64_t hub_chunks, int32_t F);
int ss_aggr_degree(const int64_t *rowptr, const int32_t *order, const float *w, int64_t N, float *den, void *stream);
int ss_aggr_rows(const int64_t *rowptr, const int32_t *order, const int64_t *other, const float *w, int64_t N, int64_t hub_entries,
                 const float *x, int32_t F, const float *gather_den, const float *den, const float *root, const float *root_x,
                 float *out, void *stream);
int ss_aggr_hub_partials(const int64_t *rowptr, const int32_t *order, const int64_t *other, const float *w, int64_t N,
                         const int32_t *hub_rows, const int32_t *hub_chunk, const int32_t *chunk_hub, int64_t n_hubs, int64_t n_chunks,
                         const float *x, int32_t F, const float *gather_den, void *workspace, size_t workspace_bytes, void *stream);
int ss_aggr_hub_finish(const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs, int64_t n_chunks, int64_t N,
                       const void *workspace, size_t workspace_bytes, int32_t F, const float *den, const float *root,
                       const float *root_x, float *out, void *stream);

/* The link decoder's endpoint gather and Hadamard product, forward and backward (csrc/ss_link_decoder.hip).  Replaces the torch
 * indexing `x[curr_links]` of reference runners/train.py:56, :63, :200, :201 and the product `x[:, 0, :] * x[:, 1, :]` of
 * models/elph.py:54 (`x_i * x_j`, models/gnn.py:212), whose backward is an index_put with float atomics.
 * links: device int64 [L, 2] row-major, L < 2^30; slot q = 2l + s is endpoint s of link l.  x: device fp32 [N, F] row-major,
 * N < 2^31; every offset is 64-bit (N * F and 2 * L * F may pass 2^31); float4 accesses when F % 4 == 0 and the float bases are
 * 16-byte aligned, scalar ones otherwise -- the bits are the same either way.
 *   ss_link_gather    out[l, s] = x[links[l, s]]                      out: device fp32 [L, 2, F]
 *   ss_link_hadamard  out[l] = fl(x[links[l, 0]] * x[links[l, 1]])    out: device fp32 [L, F]; no [L, 2, F] tensor is made
 *                     An id outside [0, N), negative ones included, is not followed: its row (hadamard: the link's row) is zeros and
 *                     *err_flag (int32 the device can write, nullable) is set -- one word per launch.
 * The backward runs on a grouping of the 2L slots by node: nodes (device int64 [M], the distinct touched nodes ascending), rowptr
 * (device int64 [M + 1]), order (device int32 [2L], the slot ids of every node ascending: a STABLE grouping).  Only the M listed
 * rows of grad_x (device fp32 [N, F]) are written; the caller clears the others.  mode 0 (gather): g is device fp32 [L, 2, F], x is
 * not read and may be null; mode 1 (product): g is device fp32 [L, F].  The accumulation order is the contract, the one ss_aggr_rows is
 * pinned to.  Row nodes[r] with the slots q_0 < q_1 < ... in chunks of C = ss_link_chunk() = 256:
 *   p_c = the sequential fp32 sum from +0 of the terms t_q of chunk c, ascending;  s = ((0 + p_0) + p_1) + ...
 *   t_q = g[l, s, :] (mode 0),  fl(g[l, :] * x[links[l, 1 - s], :]) (mode 1),  l = q >> 1, s = q & 1;  a self link is two slots
 * products and sums rounded separately, one lane per output element and chunk, no float atomics, no inter-workgroup waits; a slot
 * id outside [0, 2L) and a partner id outside [0, N) are not followed.  A row's bits depend on its own slots and their order, not
 * on the tier, on hub_entries or on the other links of the batch:
 *   ss_link_grad_rows          the regular tier: one row group per listed node; rows of more than hub_entries (>= 1) slots are left
 *                              untouched
 *   ss_link_grad_hub_partials  one row group per (hub row, chunk): p_c of chunk t goes to row t of the workspace [n_chunks, F].
 *                              hub_rows (int32 [n_hubs]) lists the POSITIONS in nodes of the rows of more than hub_entries slots,
 *                              hub_chunk (int32 [n_hubs + 1]) where each hub's chunks start, chunk_hub (int32 [n_chunks]) the hub of
 *                              every chunk
 *   ss_link_grad_hub_finish    per hub row: its partials added in chunk order, the row of grad_x stored
 *   ss_link_workspace_bytes(hub_chunks, F) = hub_chunks * F * 4, 0 for a shape that is refused
 * SS_ERR_INVALID_ARG before any launch for a null pointer (err_flag may be null; x in mode 0), negative sizes, L >= 2^30, N >= 2^31,
 * M > N or M > 2L, hub_entries < 1, a mode other than 0 or 1, n_hubs > n_chunks, a workspace smaller than ss_link_workspace_bytes;
 * L == 0, M == 0, F == 0 (hub launches: or no chunks / hubs) return SS_OK without a launch. */
int ss_link_chunk(void);
size_t ss_link_workspace_bytes(int64_t hub_chunks, int32_t F);
int ss_link_gather(const int64_t *links, int64_t L, const float *x, int64_t N, int32_t F, float *out, int32_t *err_flag, void *stream);
int ss_link_hadamard(const int64_t *links, int64_t L, const float *x, int64_t N, int32_t F, float *out, int32_t *err_flag, void *stream);
int ss_link_grad_rows(const int64_t *nodes, const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *links, int64_t L,
                      int64_t N, int64_t hub_entries, int32_t mode, const float *g, const float *x, int32_t F, float *grad_x, void *stream);
int ss_link_grad_hub_partials(const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *links, int64_t L, int64_t N,
                              const int32_t *hub_rows, const int32_t *hub_chunk, const int32_t *chunk_hub, int64_t n_hubs, int64_t n_chunks,
                              int32_t mode, const float *g, const float *x, int32_t F, void *workspace, size_t workspace_bytes,
                              void *stream);
int ss_link_grad_hub_finish(const int64_t *nodes, int64_t M, const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs,
                            int64_t n_chunks, int64_t N, const void *workspace, size_t workspace_bytes, int32_t F, float *grad_x,
                            void *stream);

/* Node features pooled over a list of weighted entries per link, forward and backward (csrc/ss_cn_rows.hip): the trainable form of
 * ss_common_neighbour_pool -- the sum of learned embeddings over every link's common neighbours (Neural Common Neighbour) -- which
 * torch writes as `coef[:, None] * x[ids]` and an index_add_, a [T, F] tensor and float atomics in both directions.
 * A list is rowptr (device int64 [L + 1], non-decreasing, inside [0, T]), ids (device int64 [T]) and coef (device fp32 [T]): entry k
 * belongs to link owner[k], the q with rowptr[q] <= k < rowptr[q + 1] (ss_common_neighbour_count / _fill make such a list; ids need
 * not ascend or be distinct inside a row).  T, L, N < 2^31; x: device fp32 [N, F], out: device fp32 [L, F], row-major; every offset
 * is 64-bit (N * F and L * F may pass 2^31); float4 accesses when F % 4 == 0 and the float bases are 16-byte aligned, scalar ones
 * otherwise -- the bits are the same either way.  The accumulation order is the contract, the one ss_aggr_rows is pinned to.  A row
 * with the entries k_0 < k_1 < ... in chunks of C = ss_cn_rows_chunk() = 256:
 *   p_c = the sequential fp32 sum from +0 of the terms t_k of chunk c, in that order;  s = ((0 + p_0) + p_1) + ...
 *   forward   row q of out, its entries rowptr[q] .. rowptr[q + 1] - 1 in list order,        t_k = fl(coef[k] * x[ids[k], :])
 *   backward  row nodes[r] of grad_x, its entries order[rowptr[r] .. rowptr[r + 1]),          t_k = fl(coef[k] * g[owner[k], :])
 * products and sums rounded separately, one lane per output element and chunk, no float atomics, no inter-workgroup waits; an empty
 * row is +0.  A list position outside [0, T), an id outside [0, N) and an owner outside [0, L) are not followed.  Up to 256 entries
 * a forward row is the sequential sum of ss_common_neighbour_pool bit for bit; longer rows follow the chunk rule.  A row's bits
 * depend on its own entries and their order, not on the tier, on hub_entries or on the other rows.
 * The backward runs on a grouping of the T entries by id: nodes (device int64 [M], the distinct named nodes ascending), rowptr
 * (device int64 [M + 1]), order (device int32 [T], the list positions of every node ascending: a STABLE grouping), owner (device
 * int64 [T]); g: device fp32 [L, F].  Only the M listed rows of grad_x (device fp32 [N, F]) are written; the caller clears the others.
 *   ss_cn_rows_forward / ss_cn_rows_grad    the regular tier: one row group per link / per listed node; rows of more than
 *                              hub_entries (>= 1) entries are left untouched
 *   ss_cn_rows_forward_hub_partials / ss_cn_rows_grad_hub_partials    one row group per (hub row, chunk): p_c of chunk t goes to row t
 *                              of the workspace [n_chunks, F].  hub_rows (int32 [n_hubs]) lists the rows of more than hub_entries
 *                              entries (forward: links; backward: POSITIONS in nodes), hub_chunk (int32 [n_hubs + 1]) where each
 *                              hub's chunks start, chunk_hub (int32 [n_chunks]) the hub of every chunk
 *   ss_cn_rows_forward_hub_finish / ss_cn_rows_grad_hub_finish    per hub row: its partials added in chunk order, the row stored
 *   ss_cn_rows_workspace_bytes(hub_chunks, F) = hub_chunks * F * 4, 0 for a shape that is refused
 * SS_ERR_INVALID_ARG before any launch for a null pointer while there is work, negative sizes, T, L or N >= 2^31, M > N or M > T,
 * hub_entries < 1, n_hubs > n_chunks, a workspace smaller than ss_cn_rows_workspace_bytes; L == 0, M == 0, F == 0 (hub launches:
 * or no chunks / hubs) return SS_OK without a launch, with null pointers too; T == 0 with L > 0 stores rows of +0. */
int ss_cn_rows_chunk(void);
size_t ss_cn_rows_workspace_bytes(int64_t hub_chunks, int32_t F);
int ss_cn_rows_forward(const int64_t *rowptr, const int64_t *ids, const float *coef, int64_t L, int64_t T, int64_t N, int64_t hub_entries,
                       const float *x, int32_t F, float *out, void *stream);
int ss_cn_rows_forward_hub_partials(const int64_t *rowptr, const int64_t *ids, const float *coef, int64_t L, int64_t T, int64_t N,
                                    const int32_t *hub_rows, const int32_t *hub_chunk, const int32_t *chunk_hub, int64_t n_hubs,
                                    int64_t n_chunks, const float *x, int32_t F, void *workspace, size_t workspace_bytes, void *stream);
int ss_cn_rows_forward_hub_finish(int64_t L, const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs, int64_t n_chunks,
                                  const void *workspace, size_t workspace_bytes, int32_t F, float *out, void *stream);
int ss_cn_rows_grad(const int64_t *nodes, const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *owner, const float *coef,
                    int64_t T, int64_t L, int64_t N, int64_t hub_entries, const float *g, int32_t F, float *grad_x, void *stream);
int ss_cn_rows_grad_hub_partials(const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *owner, const float *coef, int64_t T,
                                 int64_t L, int64_t N, const int32_t *hub_rows, const int32_t *hub_chunk, const int32_t *chunk_hub,
                                 int64_t n_hubs, int64_t n_chunks, const float *g, int32_t F, void *workspace, size_t workspace_bytes,
                                 void *stream);
int ss_cn_rows_grad_hub_finish(const int64_t *nodes, int64_t M, const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs,
                               int64_t n_chunks, int64_t N, const void *workspace, size_t workspace_bytes, int32_t F, float *grad_x,
                               void *stream);

/* Graph readouts over a disjoint-union batch of subgraphs (csrc/ss_pool.hip; reference models/seal.py: global_sort_pool :245,
 * global_add_pool / global_mean_pool :42-45, :101-106, :161, centre pooling :88-95, :149-156) [PyG semantics restated].
 * Shared by every entry: graph q owns the rows rowptr[q] .. rowptr[q + 1] of x (rowptr: device int64 [L + 1], non-decreasing,
 * inside [0, T]); x: device fp32 [T, F] row-major; every offset is 64-bit (T * F and L * k * F may pass 2^31); float4 accesses
 * when F % 4 == 0 and the float bases are 16-byte aligned, scalar ones otherwise; no float atomics, no workspace.  A graph whose
 * rowptr pair leaves [0, T] or descends, and an id or root outside its graph, is not followed: its places are not written
 * (ss_pool_select: its row of perm is all -1) and *err_flag (device int32, nullable) is set.  Returns -1 before any launch for a
 * null pointer (a float pointer may be null where it has no elements), k < 1, negative L, T or F, L >= 2^31; L == 0 returns 0.
 * ss_pool_sort_capacity() = C = 1024: the words the on-chip sort of ss_pool_select holds; k <= C.
 *   ss_pool_select   perm[q, j] (device int32 [L, k]) = the position inside graph q of its j-th row in the order: LAST channel
 *                    x[., F - 1] descending, NaN (any sign) first, -0.0 ties with +0.0, ties by ascending position; -1 for
 *                    j >= n.  The order is that of the 64-bit words (key << 32 | position) ascending, key = ~(monotone u32
 *                    image of the float), NaN -> 0: all distinct, so a row of perm depends on its graph alone -- not on the
 *                    tier (n <= C sorted in LDS; larger, any n < 2^31: radix select of the k-th key over the key column re-read
 *                    with stride F, ordered compaction, the same sort), on L or on other graphs.  F >= 1.  One workgroup per graph.
 *   ss_pool_gather   out[q, j * F .. (j + 1) * F) = x[rowptr[q] + perm[q, j]], zeros for perm -1 (out: device fp32 [L, k * F]).
 *   ss_pool_scatter  its gradient: grad_x (device fp32 [T, F]) is cleared by the call, then grad_x[rowptr[q] + perm[q, j]] =
 *                    g[q, j * F ..) for perm >= 0 (g: device fp32 [L, k * F]); perm must not name a row twice (ss_pool_select's does not).
 *   ss_segment_pool  out[q, f] (device fp32 [L, F]) = the fp32 sum from +0.0 of x[t, f], t ascending over the graph, by ONE
 *                    lane: the sequential loop bit for bit; mean != 0: then one division by (float)max(n, 1).  An empty graph
 *                    gives 0.  A graph of 10^5 rows runs on one lane group (no hub tier).
 *   ss_segment_pool_grad  grad_x[t] = g[q(t)] (mean != 0: / (float)max(n, 1)), q(t) by bisection of rowptr; rows in no graph get
 *                    zeros; every row of grad_x [T, F] is written exactly once (g: device fp32 [L, F]).
 *   ss_center_pool   out[q] (device fp32 [L, F]) = x[rowptr[q] + roots[q, 0]] * x[rowptr[q] + roots[q, 1]]; roots: device int32
 *                    [L, 2], local indices read on the device; (-1, -1) gives zeros.
 *   ss_center_pool_grad  grad_x [T, F] is cleared by the call, then with a, b the two root rows of link q: grad_x[a] = g[q] * x[b],
 *                    grad_x[b] = g[q] * x[a]; a == b: grad_x[a] = g[q] * x[a] + g[q] * x[a], each product rounded first. */
int ss_pool_sort_capacity(void);
int ss_pool_select(const int64_t *rowptr, int64_t L, const float *x, int64_t T, int32_t F, int32_t k, int32_t *perm, int32_t *err_flag,
                   void *stream);
int ss_pool_gather(const int64_t *rowptr, int64_t L, const int32_t *perm, int32_t k, const float *x, int64_t T, int32_t F, float *out,
                   int32_t *err_flag, void *stream);
int ss_pool_scatter(const int64_t *rowptr, int64_t L, const int32_t *perm, int32_t k, const float *g, int64_t T, int32_t F, float *grad_x,
                    int32_t *err_flag, void *stream);
int ss_segment_pool(const int64_t *rowptr, int64_t L, const float *x, int64_t T, int32_t F, int32_t mean, float *out, int32_t *err_flag,
                    void *stream);
int ss_segment_pool_grad(const int64_t *rowptr, int64_t L, const float *g, int64_t T, int32_t F, int32_t mean, float *grad_x, void *stream);
int ss_center_pool(const int64_t *rowptr, int64_t L, const int32_t *roots, const float *x, int64_t T, int32_t F, float *out,
                   int32_t *err_flag, void *stream);
int ss_center_pool_grad(const int64_t *rowptr, int64_t L, const int32_t *roots, const float *x, const float *g, int64_t T, int32_t F,
                        float *grad_x, int32_t *err_flag, void *stream);

/* 128-bit content digest of a device buffer (bytes % 16 == 0, 16-byte aligned): out[0] = sum, out[1] = xor over its 16-byte chunks
 * of a 64-bit mix of (chunk, chunk index) -- order-independent to compute, position-dependent in value.  out: device uint64[2],
 * overwritten (the call clears it first).  One streaming pass at HBM rate.  For the multi-GPU builds: the reference has ONE
 * table (hashing.py:139-165); a build that leaves a replica on every rank -- above all the peer-write build, whose rows arrive
 * through other GPUs' stores -- compares the digests of all replicas after its first build (dist.verify_replicas). */
int ss_table_digest(const void *data, int64_t bytes, uint64_t *out, void *stream);

/* int64 <-> packed uint32 MinHash tables (the reference's tensors are int64, hashing.py:124). */
int ss_pack_minhash(const int64_t *in, uint32_t *out, int64_t count, void *stream);
int ss_unpack_minhash(const uint32_t *in, int64_t *out, int64_t count, void *stream);

/* Incremental update of the tables of build_hash_tables after a few edges were added or removed.  The reference has no such
 * operation: build_hash_tables (hashing.py:139-165) recomputes every row of every hop, and get_hashed_train_val_test_datasets
 * (src/data.py:173-176 with datasets/elph.py) does so once per split for graphs that differ by a few per cent of their edges.  A hop-k
 * row depends only on the closed in-neighbourhood of its node, so with `graph` the CSR of the edge list AFTER the change:
 *   seed    = targets of the added / removed edges + rows whose implicit self loop (i < n_self) appeared or disappeared, read off the
 *             old hop-1 cardinalities: (i < n_self) != (cards_old[i * cards_stride] > 0)
 *   dirty_1 = seed;  dirty_k = seed + { i : an in-neighbour of i is in dirty_{k-1}, or i < n_self and i is in dirty_{k-1} }
 * and hop k of the update recomputes exactly the rows of dirty_k -- from scratch, so removals need nothing of their own.
 *   ss_update_mark  dirty_1 .. dirty_h as byte maps, int32 row lists and device-side counts, all in `workspace`
 *                   (ss_update_workspace_bytes(N, h) device bytes, 0 = unsupported size; the call clears what it needs).
 *                   added_dst / removed_dst: device int64[n_added] / [n_removed] target ids (either may be empty); an id outside
 *                   [0, N) sets bit 0 of *err_flag (nullable) and is dropped.  One pull pass over `col` per hop beyond the first.
 *   ss_update_hop   rows dirty_hop of the hop's MinHash table, HLL table and cardinalities (cards_out[i * cards_stride]) from the
 *                   UPDATED tables of hop - 1 (mh_in / hll_in); every other row and cardinality is left untouched.  mh_in == NULL:
 *                   MinHash rows from node ids (hop 1 only; a / b as ss_first_hop, P % 64 == 0, P <= 256); hll_in == NULL: HLL rows
 *                   from node ids (hop 1 only, p == 8); SS_ERR_UNSUPPORTED otherwise.  To be called for hop = 1 .. h in order, on the
 *                   stream of ss_update_mark with the same graph and workspace.  Launches are sized by N; the row counts are read
 *                   on the device, so nothing between the first and the last launch of an update waits for the host.
 * After the calls the first words of the workspace hold, as int32: [0] = |seed|, [4k] = |dirty_k|, [4k + 1] / [4k + 2] = how many of
 * them were listed as regular / hub rows (more in-edges than graph->hub_threshold: one 16-wavefront workgroup each), k = 1 .. h.
 * The hub lists of the graph itself are not used: a hub row that is not dirty is not recomputed. */
size_t ss_update_workspace_bytes(int64_t N, int32_t h);
int ss_update_mark(const ss_csr_graph *graph, const int64_t *added_dst, int64_t n_added, const int64_t *removed_dst, int64_t n_removed,
                   const float *cards_old, int64_t cards_stride, int32_t h, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                   void *stream);
int ss_update_hop(const ss_csr_graph *graph, int32_t hop, int32_t h, const uint64_t *a, const uint64_t *b, const uint32_t *mh_in,
                  uint32_t *mh_out, int32_t P, const uint8_t *hll_in, uint8_t *hll_out, int32_t p, float *cards_out, int64_t cards_stride,
                  const ss_hll_params *prm, const void *workspace, size_t workspace_bytes, void *stream);

/* Target-link masking: ss_pair_features for links that may be edges of the graph the tables were built on, each scored as if its own
 * edge were absent.  The reference does this on its SEAL path only (src/datasets/seal.py:338 removes the target link from every
 * enclosing subgraph); its sketch path (hashing.py:139-165 build, :258-323 query) cannot, a table row being a min / max fold.  For a link
 * (u, v) let G_uv be the graph of `graph` (its edges, flow source -> target, plus the implicit self loops below n_self) without every copy
 * of u -> v and of v -> u; n_self is that of the full graph.  Row q of `out` is what ss_pair_features returns for link q from tables and
 * cards built on G_uv: MinHash match counts and HLL zero counts exactly, features to fp32 rounding.  A link with u == v, with neither
 * direction present, or with an id out of range keeps the row (and err_flag report) of ss_pair_features bit for bit.
 *   graph    the CSR the tables were built on (ss_csr_build of the same edge list; n_self_loops / n_self_loops_dev as in the build;
 *            whole graph: no row range), graph->num_nodes == N < 2^31.  Nothing checks that the tables belong to it.
 *   a, b     the permutation parameters of ss_minhash_init (device uint64[P]): hop 0 is recomputed from node ids
 *   mh, hll, cards, prm, flags, out, dbg_match, dbg_zero, err_flag: as ss_pair_features (cards: those of the FULL graph; the masked
 *            rows' cardinalities are computed from the masked rows)
 *   dbg_row_zeros (device int32[B, 2, h], nullable): zero registers of the hop-k row of u, then of v, as used for the link
 *   dbg_masked    (device uint8[B], nullable): 1 where the link was found in the graph and rebuilt
 *   workspace     ss_masked_workspace_bytes(B) device bytes (0 = unsupported size; B < 2^31); after the call its first int32 holds
 *                 the number of links rebuilt
 * Launches: the plain query, one classify pass over rows u and v of the CSR, one pass over the links found (their count never leaves
 * the device).  Cost per edge link: the in-degrees of u and v at h <= 2, their 2-hop in-walk counts at h = 3.  Returns
 * SS_ERR_UNSUPPORTED when a sketch row has more than 256 16-byte chunks (P / 4 + 2^p / 16 > 256). */
size_t ss_masked_workspace_bytes(int64_t B);
int ss_masked_pair_features(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, const uint64_t *a,
                            const uint64_t *b, const uint32_t *const *mh, int32_t P, const uint8_t *const *hll, const float *cards,
                            int64_t cards_stride, const ss_hll_params *prm, uint32_t flags, float *out, int32_t *dbg_match,
                            int32_t *dbg_zero, int32_t *dbg_row_zeros, uint8_t *dbg_masked, int32_t *err_flag, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Exact enclosing subgraphs: the induced adjacency and the node labels of the node rows of ss_exact_nodes_pairs / ss_exact_nodes_large
 * (rowptr int64 [B + 1], ids int64 [T], T = rowptr[B]; listed node t of link q has the LOCAL index t - rowptr[q]) -- what the reference
 * builds per link in Python: k_hop_subgraph's A[nodes, :][:, nodes] with the target link zeroed (src/datasets/seal.py:291-348), the
 * edge list and weights of construct_pyg_graph (:351-389) and drnl / de / de+ (src/labelling_tricks.py:11-27, 63-134).
 *   ss_subgraph_adj     csr_rowptr / csr_col: the destination-grouped CSR of the graph (row x = the sources j of the arcs j -> x) with
 *                       every row ASCENDING (ss_csr_sort_rows), N < 2^31 nodes; links: int64 [B, 2] (negative ids wrapped).  The
 *                       adjacency row of listed node t (id x, link (u, v)) holds every distinct j != x of the link's id row with an
 *                       arc j -> x, as local indices, ascending, with the number of copies of the arc; flags & SS_FLAG_MASK_TARGET and
 *                       u != v: without (x = u, j = v) and (x = v, j = u).
 *                         count pass (adj_ptr == NULL)  counts[t] (int32 [T]) = the length of t's adjacency row
 *                         fill pass  (adj_ptr != NULL)  adj_ptr: int64 [T + 1], the caller's cumulative sum of counts; writes nbr and
 *                                                       weight (int32 [adj_ptr[T]]) inside [adj_ptr[t], adj_ptr[t + 1]) and
 *                                                       roots[q] (int32 [B, 2]) = the local indices of u and v for every link with a
 *                                                       non-empty row (the caller presets the others)
 *                       switch_ratio >= 0: a node with more than switch_ratio * (row length) in-arcs walks the id row and searches its
 *                       CSR row, every other node walks its arcs and searches the id row; the rows do not depend on it.
 *   ss_subgraph_labels  z from two BFSs per link over that adjacency (depth from u, depth from v; unreachable = max_dist; all clipped
 *                       to max_dist in [1, SS_SUBGRAPH_MAX_DIST]):  SS_SUBGRAPH_LABEL_DE  z: int64 [T, 2] = (d_u, d_v);
 *                       SS_SUBGRAPH_LABEL_DE_PLUS  the same with v removed for d_u and u removed for d_v, the removed root's entry 1;
 *                       SS_SUBGRAPH_LABEL_DRNL  z: int64 [T], those two distances with the removed root's entry 0 through
 *                       1 + min(d_u, d_v) + (d / 2)(d / 2 + d % 2 - 1), d = d_u + d_v, and 1 where either is 0.  u == v: one root,
 *                       nothing removed, d_u == d_v.  Rows of at most min(lds_max_nodes, 2048) nodes are labelled on chip; row q of the
 *                       others uses workspace[4 ws_ptr[q] .. 4 ws_ptr[q + 1]) (int32), ws_ptr: int64 [B + 1] = the cumulative sum of
 *                       the lengths of exactly those rows (workspace may be null when there is none).
 * Both return SS_OK for B == 0 (ss_subgraph_adj: or T == 0) before any launch, SS_ERR_INVALID_ARG for negative sizes, null pointers,
 * a max_dist out of range; ss_subgraph_labels returns SS_ERR_UNSUPPORTED for an unknown label mode. */
#define SS_SUBGRAPH_LABEL_DRNL 0
#define SS_SUBGRAPH_LABEL_DE 1
#define SS_SUBGRAPH_LABEL_DE_PLUS 2
#define SS_SUBGRAPH_MAX_DIST (1 << 20)
int ss_subgraph_adj(const int64_t *csr_rowptr, const int32_t *csr_col, int64_t N, const int64_t *links, int64_t B, const int64_t *rowptr,
                    const int64_t *ids, int64_t T, uint32_t flags, int32_t switch_ratio, int32_t *counts, const int64_t *adj_ptr,
                    int32_t *nbr, int32_t *weight, int32_t *roots, void *stream);
int ss_subgraph_labels(const int64_t *rowptr, int64_t B, const int32_t *roots, const int64_t *adj_ptr, const int32_t *nbr,
                       int32_t label_mode, int64_t max_dist, int32_t lds_max_nodes, const int64_t *ws_ptr, int32_t *workspace, int64_t *z,
                       void *stream);

/* Connected components of an edge_index and the induced subgraph of a node set: what the reference does on the host with a Python set
 * walk that scans `row` once per visited node and a per-edge `i in lcc` test (O(N E) interpreter work).  src / dst: the two rows of the
 * edge list (device int64 [E], torch-style negative ids wrapped; an edge with an id outside [-N, N) sets err_flag (nullable) and is
 * ignored).  An edge counts in both directions: the WEAK components of a directed list.  N < 2^31, E < 2^31.
 *   ss_components_labels  label[x] (int32 [N]) = the smallest node id of x's component, by a lock-free union-find over the edges
 *                         (parent: int32 [N] scratch; larger root hooked under the smaller by atomicCAS, path halving by atomicMin;
 *                         no lane waits on another) and a flattening launch -- get_component, src/lcc.py:34-44.
 *   ss_components_sizes   size[r] (int32 [N], cleared by the call) = the nodes labelled r, one aggregated atomic per wavefront and
 *                         label; block_roots[b] (int32) = the roots (label[x] == x) among the nodes [b, b + 1) * SS_COMPONENTS_CHUNK.
 *   ss_components_roots   block_incl: int64, the caller's INCLUSIVE cumulative sum of block_roots.  roots / sizes (int64 [C]): the
 *                         roots ascending and their sizes; *best (uint64, preset to 0) = max over the roots of
 *                         (size << 32) | (0xFFFFFFFF - root): the largest component, ties to the smallest root, which is what
 *                         np.argmax picks from the discovery order of get_largest_connected_component, src/lcc.py:7-15.
 *   ss_components_same    out[q] (uint8 [L]) = whether the two nodes of links[q] (int64 [L, 2], negative ids wrapped) carry one label;
 *                         an id outside [-N, N) sets err_flag and gives 0.
 *   ss_induced_select     the node set as mask (uint8 [N], non-zero = kept), or (mask null) as the component whose root is in *best
 *                         (label and best as above).  Count pass (block_incl null): block_count[b] = the kept nodes of chunk b.  Fill
 *                         pass (block_incl = the inclusive cumulative sum of those counts): nodes (int64) = the kept ids ascending,
 *                         mapper[x] (int64 [N]) = the position of x in nodes, -1 outside -- get_node_mapper, src/lcc.py:18-24.
 *   ss_induced_mapper     the node set as a list: mapper[x] = -1 everywhere, then mapper[nodes[i]] = i, i < n (negative ids wrapped;
 *                         an id outside [-N, N) sets err_flag and is skipped; a node listed twice sets dup_flag).
 *   ss_induced_edges      the edges with mapper >= 0 at both ends.  Count pass (block_incl null): block_count[b] = the kept edges of
 *                         chunk b.  Fill pass: out_src / out_dst (int64 [E']) = mapper of the two ends, edge_ids (int64 [E']) = the
 *                         position in the input, all in the input's order -- remap_edges, src/lcc.py:27-32, over the filter of
 *                         use_lcc, src/data.py:241-249.
 * Order inside every compacted output comes from ballot ranks and the caller's cumulative sum, never from an atomic.  Argument errors
 * (SS_ERR_INVALID_ARG: a size out of range, a null pointer with a non-zero count) are detected before any launch; nothing to do (N == 0;
 * ss_induced_edges: E == 0; ss_components_same: L == 0): SS_OK, no launch. */
#define SS_COMPONENTS_CHUNK 2048 /* consecutive items per workgroup of the count / fill passes: the length of a block_* array is ceil(n / this) */
int ss_components_labels(const int64_t *src, const int64_t *dst, int64_t E, int64_t N, int32_t *parent, int32_t *label, int32_t *err_flag,
                         void *stream);
int ss_components_sizes(const int32_t *label, int64_t N, int32_t *size, int32_t *block_roots, void *stream);
int ss_components_roots(const int32_t *label, const int32_t *size, int64_t N, const int64_t *block_incl, int64_t *roots, int64_t *sizes,
                        uint64_t *best, void *stream);
int ss_components_same(const int32_t *label, int64_t N, const int64_t *links, int64_t L, uint8_t *out, int32_t *err_flag, void *stream);
int ss_induced_select(const uint8_t *mask, const int32_t *label, const uint64_t *best, int64_t N, const int64_t *block_incl,
                      int32_t *block_count, int64_t *nodes, int64_t *mapper, void *stream);
int ss_induced_mapper(const int64_t *nodes, int64_t n, int64_t N, int64_t *mapper, int32_t *err_flag, int32_t *dup_flag, void *stream);
int ss_induced_edges(const int64_t *src, const int64_t *dst, int64_t E, int64_t N, const int64_t *mapper, const int64_t *block_incl,
                     int32_t *block_count, int64_t *out_src, int64_t *out_dst, int64_t *edge_ids, int32_t *err_flag, void *stream);

/* The merge of equal (row, col) entries of an edge list, on the device: what torch_sparse.coalesce (reference src/datasets/elph.py:54-66,
 * src/datasets/seal.py:58-60, 111-113) and PyG's to_undirected(..., reduce='add') (src/datasets/elph.py:54-66 for directed data,
 * src/data.py:137, 174) do at the head of every dataset constructor [semantics restated; graph_prep.py].
 * row / col: device int64 [E], the list (for to_undirected: the list followed by its reverse); perm: device int32 [E], the positions of
 * the list sorted by (row, col, position) -- a permutation of [0, E), NOT validated: two stable groupings by ss_csr_group_ids +
 * ss_csr_sort_rows, least significant key first.  1 <= N < 2^31, E < 2^31.  A RUN is the entries of one pair in list order.
 *   ss_coalesce_mark        block_heads[b] (int32) = the run heads among the sorted positions [b, b + 1) * ss_coalesce_block(); position i
 *                           is a head when i == 0 or its pair differs from position i - 1's.  An id outside [0, N) -- negative ones
 *                           included, nothing wraps -- sets err_flag (nullable).
 *   ss_coalesce_fill        block_incl: int64, the caller's INCLUSIVE cumulative sum of block_heads; n_runs = its last entry.  Every head
 *                           takes slot = workgroup offset + ballot rank: out_row / out_col [n_runs] (int64) = its pair, run_start[slot]
 *                           (int32 [n_runs + 1]) = its sorted position, run_start[n_runs] = E; rowptr (int64 [N + 1]) = where each row
 *                           of out_row starts: where out_row steps from a to b the head fills rowptr[a + 1 .. b], the first gap starts
 *                           at row 0 and the last ends at N.  With ids out of range (reported by the mark pass) no store leaves the
 *                           outputs.
 *   ss_coalesce_reduce      one lane per slot: out_count[slot] (int32) = the run's length; out_value[slot] = op over the run's values
 *                           value[p] (p < n_values) or value[p - n_values] (the doubled list) in list order under the CHUNK RULE: the run
 *                           is cut into chunks of ss_coalesce_chunk() entries from its start, every chunk folded sequentially from its
 *                           first entry, the chunk results folded in chunk order.  add: the sum (int64 wraps); mean: that sum divided
 *                           by the count in the value's type (int64: floor division); min / max: the canonical quiet NaN if any entry
 *                           is NaN, else the extreme, of equal values (-0.0, +0.0) the one listed first.  A run of more than
 *                           long_entries entries is not reduced but listed: long_runs (int32 [max_long], max_long >= E / long_entries),
 *                           info[0] (int32) = how many, info[1] = the longest run; info is cleared by the call.  value null: counts and
 *                           info[1] only.
 *   ss_coalesce_reduce_long on the same stream after ss_coalesce_reduce: one wavefront per listed run, lane l folding chunks l, l + 64,
 *                           ..., the chunk results joined in chunk order -- the bits ss_coalesce_reduce would have given.
 *   ss_coalesce_symmetric   *asymmetric (int32, cleared by the call) = 1 if some output pair (u, v) has no pair (v, u) -- one lane per
 *                           pair, a binary search of row v -- or (value given) one with another value (NaN equals NaN).
 * dtype: 0 int64, 1 float32, 2 float64; op: 0 add, 1 mean, 2 min, 3 max; any other returns SS_ERR_UNSUPPORTED.  ss_coalesce_chunk() = 256
 * entries per chunk of the accumulation order, ss_coalesce_block() = 2048 sorted positions per workgroup of the mark / fill passes.  Argument errors (SS_ERR_INVALID_ARG: a size out of range, a null
 * pointer with a non-zero count) are detected before any launch; E == 0 / n_runs == 0: SS_OK, no launch.  No float atomics anywhere. */
int ss_coalesce_chunk(void);
int ss_coalesce_block(void);
int ss_coalesce_mark(const int64_t *row, const int64_t *col, const int32_t *perm, int64_t E, int64_t N, int32_t *block_heads, int32_t *err_flag,
                     void *stream);
int ss_coalesce_fill(const int64_t *row, const int64_t *col, const int32_t *perm, int64_t E, int64_t N, const int64_t *block_incl,
                     int64_t n_runs, int64_t *out_row, int64_t *out_col, int32_t *run_start, int64_t *rowptr, void *stream);
int ss_coalesce_reduce(const int32_t *perm, const int32_t *run_start, int64_t n_runs, const void *value, int64_t n_values, int32_t dtype,
                       int32_t op, int32_t long_entries, void *out_value, int32_t *out_count, int32_t *long_runs, int64_t max_long,
                       int32_t *info, void *stream);
int ss_coalesce_reduce_long(const int32_t *perm, const int32_t *run_start, int64_t n_runs, const void *value, int64_t n_values, int32_t dtype,
                            int32_t op, void *out_value, const int32_t *long_runs, const int32_t *info, int64_t max_long, void *stream);
int ss_coalesce_symmetric(const int64_t *rowptr, const int64_t *out_row, const int64_t *out_col, int64_t n_runs, int64_t N, const void *value,
                          int32_t dtype, int32_t *asymmetric, void *stream);

/* Measurement-only entry points (launch-duration probes used by bench.py and tools/) are declared in
 * subgraph_sketch_debug.h; they are not part of the drop-in boundary. */

#ifdef __cplusplus
}
#endif
#endif /* SUBGRAPH_SKETCH_H */
