// ss_first_hop.hip -- hop 1 computed straight from node ids (fused hop-0 init + first propagation).
//
// Hop-0 sketches are pure functions of the node id (reference hashing.py:118-137): row t of the MinHash
// table is ((a_j * hv_t + b_j) mod 2^64 mod (2^61-1)) & 0xFFFFFFFF, row t of the HLL table has the single
// register (hv_t & (m-1)) = rank(hv_t).  Reading them back from HBM for the first propagation
// (hashing.py:160-161 at k = 1) costs (E' + N) * 768 B; recomputing them in registers costs 3 integer
// multiplies + 7 simple VALU per (neighbour, permutation) and no table traffic at all -- the kernel reads only
// the CSR and writes the hop-1 rows.  Results are identical to ss_minhash_init + ss_hll_init + ss_propagate.
// (VALU-bound: v_mul_lo_u32 / v_mad_u64_u32 issue at quarter rate, 16 cycles per wave64 on gfx950; measured
// 0.17 ms vs 0.36 ms for init + propagate on the bench graph.)
//
// Mapping of a walk (first_hop_walk, ss_walks.hpp): lane l owns permutations l, l+64, .. (P/64 of them) and
// HLL registers 4l..4l+3 (M = 256).  Neighbour ids are fetched 64 at a time (one coalesced load), every
// lane hashes ITS neighbour (64 hashes in parallel) and scatter-maxes that neighbour's single HLL register
// into an LDS row; then the wave walks the batch with v_readlane: the neighbour's hash is
// wave-uniform (SGPR pair), each lane evaluates its own permutations on it.  The row kernels below give a wavefront
// several MinHash rows, a 16-lane group an HLL row.
// Hub rows are hub units (ss_hub.hpp): a whole workgroup per row or slice of a row, waves take alternate 64-neighbour
// batches and combine through LDS atomics -- the HLL side hosted by the leading workgroups of hll_first_hop_kernel's launch,
// the MinHash side by the fused kernel's (ss_fused_hop.hip) or by first_hop_hub_kernel, a launch of its own.
#include "ss_hub.hpp"

namespace ss {

// ---- MinHash first hop, several consecutive rows per wavefront ---------------------------------------------------------
// One row per wavefront spends about as many VALU instructions per row on fixed work (permutation parameters, neighbour-id
// load + splitmix64, winner fetch, exact evaluation: ~105) as on the walk itself at the bench graph's degree (9 per
// neighbour x 11), and is bound by VALU issue (VALUBusy 88 %).  Rows that are consecutive in the CSR are also
// consecutive in `col`, so a wavefront that owns kRowsPerWave consecutive rows
//   * loads a / b and sets up its lane constants once,
//   * fetches and hashes the neighbour ids of ALL its rows in batches of 64 - kRowsPerWave col entries with one coalesced
//     load + one splitmix64 per batch (the last kRowsPerWave lanes of every batch hold the hashes of the rows' own ids: the
//     implicit self loop of row r is slot 64 - kRowsPerWave + r of whatever batch is current),
//   * and then walks row after row over its slice of the batch (two-phase evaluation of ss_walks.hpp: phase 1 finds which
//     neighbour attains the minimum, phase 2 evaluates that one exactly).
// Rows flagged ambiguous (and rows that list themselves: duplicates of the implicit self loop) are redone by the exact walk.
// (The walk itself is MinhashRows of ss_walks.hpp, shared with the fused kernel of ss_fused_hop.hip.)
constexpr int kRowsPerWave = 8;

template <int PPL, int R, bool MIR>
__global__ __launch_bounds__(256) void first_hop_rows_kernel(GraphArgs g, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb,
                                                             uint32_t *__restrict__ mh_out, int p, bool skip_hubs)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    report_hub_rows(g);
    MinhashRows<PPL, R, MIR> m;
    if (!m.init(g, g.row0 + ((int64_t)blockIdx.x * (blockDim.x / kWave) + wave) * R, pa, pb, p, skip_hubs)) return;
    for (int r = 0; r < m.rows; ++r) m.row(r, mh_out);  // wave-uniform
}

// HLL-only first hop, latency-optimised: one 16-lane DPP row per destination (4 destinations in flight per wave).
// Used when the caller asks for the HLL sketch alone (the two-stream build runs the HLL chain beside the MinHash
// chain); one row per wavefront is a single dependent chain per wave and takes 4x longer for this.
constexpr int kHllRows = 4;  // (2, 6 and 8 measured the same 25 us on the bench graph: the kernel is not bound by its prefetch depth;
                             // round 6, 3 / 4 / 6 / 8 rows: 25.5 / 25.7 / 25.4 / 37.9 us -- 8 spills 100 bytes at the 64-VGPR budget)

// PPL only matters to the leading workgroups (hub units, ss_hub.hpp): with hub_mh_out they also serve the hop-1 MinHash table
// (P = 64 * PPL) -- ss_fused_hop_stage's row kernel has no register to spare for them.  The register allocator is held to the 64
// VGPRs of the row path's eight wavefronts per SIMD; what the MinHash units spill they spill on their own, cold, path.
// REC: every lane group also stores its rows' code records (hll_first_hop_row16; `records`: uint32[N][16]) -- an instantiation of its
// own, so that the kernel without records keeps its registers.
template <int PPL, bool REC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void hll_first_hop_kernel(
    GraphArgs g, int p, uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm, bool skip_hubs,
    int hub_blocks, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb, uint32_t *__restrict__ hub_mh_out,
    uint32_t *__restrict__ records)
{
    // only the linear-counting table is staged (this kernel is only launched for p = 8: 257 entries): a hop-1 row leaves the
    // linear-counting range at 147 neighbours, and those few read raw / bias from global memory.  17 KB of LDS and 60 VGPRs
    // instead of 24.5 KB and 73: 8 workgroups per CU instead of 6 (24.4-25.9 -> 22.9 us on the bench graph)
    __shared__ LcLds<257> lds;
    __shared__ __attribute__((aligned(16))) uint32_t rows[256 / kRow][256];  // one u32 per register and 16-lane group
    const bool want_cards = cards_out != nullptr;
    report_hub_rows(g);
    EstimatorTables est;
    if (want_cards) est = stage_lc_only(lds, prm);
    if ((int)blockIdx.x < hub_blocks) {  // workgroup-uniform: a leading workgroup serves hub units of the hop-1 HLL table (its rows
                                         // leave the linear-counting range: raw / bias come from global memory)
        static_assert(sizeof(FirstHopHubLds<PPL>) <= sizeof(rows), "the hub units' LDS rows live in the row image");
        FirstHopHubLds<PPL> &hub = *reinterpret_cast<FirstHopHubLds<PPL> *>(&rows[0][0]);
        // (with hub_mh_out the first QUARTER of the leading workgroups serves the HLL units, the rest the MinHash units -- tickets of
        // their own; a MinHash unit costs several times an HLL unit, and this launch is a short one to hide them in)
        const int first = hub_mh_out ? hub_blocks / 4 : hub_blocks;
        if ((int)blockIdx.x < first)
            first_hop_hub_units<PPL, kHubLeadWaves, false, true>(g, (int)blockIdx.x, first, nullptr, nullptr, nullptr, p, hll_out, cards_out,
                                                                 cards_stride, est, want_cards, hub);
        else
            first_hop_hub_units<PPL, kHubLeadWaves, true, false>(g, (int)blockIdx.x - first, hub_blocks - first, pa, pb, hub_mh_out, p, nullptr,
                                                                 nullptr, 0, est, false, hub);
        return;
    }
    const int l = threadIdx.x & (kRow - 1);
    const int grp = threadIdx.x / kRow;
    // kHllRows rows per lane group, one after the other through the same LDS row image; the row bounds and the first
    // neighbour ids of ALL of them are requested up front, so the two dependent global round trips (rowptr -> col) of
    // the later rows hide under the work of the earlier ones
    // Row r of lane group `grp` is row r * 16 + grp of the workgroup's 64: at any moment the 16 lane groups work on 16 CONSECUTIVE rows
    // -- consecutive stretches of `col` and of the output (round 6; four consecutive rows per lane group, the map of rounds 2-5,
    // fetched the shared boundary lines twice at ogbl-ppa size)
    const int groups = (int)(blockDim.x / kRow);
    const int64_t wg_first = g.row0 + (int64_t)((int)blockIdx.x - hub_blocks) * groups * kHllRows;
    const int64_t first = wg_first + grp;
    const int64_t row_step = groups;
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    uint32_t *row = rows[grp];
    int64_t rbs[kHllRows];
    int degs[kHllRows], nid0[kHllRows];
    bool oks[kHllRows];
#pragma unroll
    for (int r = 0; r < kHllRows; ++r) {
        oks[r] = first + r * row_step < g.row1;
        const int64_t i = oks[r] ? first + r * row_step : g.row1 - 1;
        rbs[r] = g.rowptr[i];
        degs[r] = (int)(g.rowptr[i + 1] - rbs[r]);
    }
    // (unconditional loads from an address that is always valid -- lanes past the end of their row read the first word of
    // rowptr and never look at it: a load under `if (l < deg)` is awaited with vmcnt(0) at the end of its branch, which put
    // the four rows' id loads one round trip behind the other)
    const int32_t *always_valid = reinterpret_cast<const int32_t *>(g.rowptr);
    // ... of the first TWO rows; the first ids of row r + 2 are requested when row r is about to be walked.  (All four up front, as
    // rounds 2-4 had it: the line a later row's first ids sit in also holds its next ids, and by the time a lane group has walked
    // three rows of 74 neighbours -- ogbl-ppa -- that line has left the L2 again and is fetched a second time: PMC 0.398 GB for
    // 0.324 GB algorithmic at that size against 1.03x at collab size, where four rows span two lines; VERDICT r4 #5.)
#pragma unroll
    for (int r = 0; r < kHllRows; ++r) nid0[r] = r < 2 ? *(l < degs[r] ? g.col + rbs[r] + l : always_valid) : 0;
#pragma unroll
    for (int r = 0; r < kHllRows; ++r) {
        if (r + 2 < kHllRows) nid0[r + 2] = *(l < degs[r + 2] ? g.col + rbs[r + 2] + l : always_valid);
        const bool ok = oks[r];
        const int64_t i = ok ? first + r * row_step : g.row1 - 1;
        const int deg = degs[r];
        const bool hub = skip_hubs && deg > g.hub_threshold;
        const int total = hub ? 0 : deg + (i < n_self ? 1 : 0);
        if constexpr (REC)  // (no mirrors: the records form belongs to the unsharded build)
            hll_first_hop_row16<false, true>(row, g.col + rbs[r], deg, total, i, nid0[r], always_valid, p, ok && !hub, hll_out, cards_out,
                                             cards_stride, est, want_cards, l, g.mir, records, ok && hub);
        else
            hll_first_hop_row16<true>(row, g.col + rbs[r], deg, total, i, nid0[r], always_valid, p, ok && !hub, hll_out, cards_out, cards_stride, est,
                                      want_cards, l, g.mir);
    }
}

// ---- hub units as a launch of their own (16 wavefronts per workgroup) --------------------------------------------------------
constexpr int kHubThreads = 1024;
constexpr int kHubWaves = kHubThreads / kWave;
constexpr int kHubGrid = 256;  // one workgroup per CU; workgroups beyond the unit count exit at once

template <int PPL, bool DO_MH, bool DO_HLL>
__global__ __launch_bounds__(kHubThreads) void first_hop_hub_kernel(GraphArgs g, const uint64_t *__restrict__ pa,
                                                                    const uint64_t *__restrict__ pb, uint32_t *__restrict__ mh_out, int p,
                                                                    uint8_t *__restrict__ hll_out, float *__restrict__ cards_out,
                                                                    int64_t cards_stride, ss_hll_params prm)
{
    __shared__ EstimatorLds lds;
    __shared__ FirstHopHubLds<PPL> hub;
    const HubCounts n = hub_counts(g);
    if ((int)blockIdx.x >= n.hubs + n.slices) return;  // the common case (no hub rows) costs three scalar loads per workgroup
    const bool want_cards = DO_HLL && cards_out != nullptr;
    EstimatorTables est = {};
    if (want_cards) est = stage_tables(lds, prm);
    first_hop_hub_units<PPL, kHubWaves, DO_MH, DO_HLL>(g, (int)blockIdx.x, (int)gridDim.x, pa, pb, mh_out, p, hll_out, cards_out, cards_stride, est,
                                                       want_cards, hub);
}

// ---- host: each kernel template above has ONE launch expression, its instantiation picked by the constants it is handed ------------

// MinHash rows: kRowsPerWave consecutive rows per wavefront
static int launch_minhash_rows(const HopRequest &r)
{
    constexpr int rows_per_block = 4 * kRowsPerWave;
    const dim3 grid((unsigned)((r.g.rows() + rows_per_block - 1) / rows_per_block));
    {
        ProfileSpan span(r.stream, SS_PROF_FIRST_HOP_MH);
        for_ppl(r.P, [&](auto ppl) {
            const auto launch = [&](auto mirrors) {
                hipLaunchKernelGGL((first_hop_rows_kernel<decltype(ppl)::value, kRowsPerWave, decltype(mirrors)::value>), grid, dim3(256), 0, r.stream,
                                   r.g, r.a, r.b, r.mh_out, r.p, r.hubs);
            };
            if (r.g.mir.n > 0) launch(std::true_type{});
            else launch(std::false_type{});
        });
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}

// HLL first hop of the regular rows (what follows for the hub rows is the caller's: ss_first_hop, ss_fused_hop_stage).  r.lead leading
// workgroups serve the hub units of the HLL table; where r.mh_out is set as well, twice as many serve those of both hop-1 tables (a
// quarter for the HLL units, the rest for the MinHash units, P = 64 * PPL values per row from the permutations a / b).  lead = 0: the
// caller launches first_hop_hub_kernel
int launch_hll_first_hop_rows(const HopRequest &r, uint32_t *records)
{
    if (r.g.mir.n > 0) records = nullptr;  // (the records instantiation stores no mirrors; ss_fused_hop_stage_records never asks for both)
    const bool host_mh = r.lead > 0 && r.mh_out;
    const int lead = host_mh ? 2 * r.lead : r.lead;
    ProfileSpan span(r.stream, SS_PROF_FIRST_HOP_HLL);
    const dim3 grid((unsigned)((r.g.rows() + 16 * kHllRows - 1) / (16 * kHllRows) + lead));
    for_ppl(host_mh ? r.P : kWave, [&](auto ppl) {  // (PPL only matters to the MinHash units)
        const auto launch = [&](auto rec) {
            hipLaunchKernelGGL((hll_first_hop_kernel<decltype(ppl)::value, decltype(rec)::value>), grid, dim3(256), 0, r.stream, r.g, r.p, r.hll_out,
                               r.cards_out, r.cards_stride, r.prm, r.hubs, lead, host_mh ? r.a : nullptr, host_mh ? r.b : nullptr,
                               host_mh ? r.mh_out : nullptr, records);
        };
        if (records) launch(std::true_type{});
        else launch(std::false_type{});
    });
    SS_LAUNCH_CHECK();
    return SS_OK;
}

// hub units as a launch of their own, for the tables the request names
static int launch_first_hop_hubs(const HopRequest &r)
{
    for_ppl(r.P, [&](auto ppl) {
        const auto launch = [&](auto mh, auto hll) {
            hipLaunchKernelGGL((first_hop_hub_kernel<decltype(ppl)::value, decltype(mh)::value, decltype(hll)::value>), dim3(kHubGrid),
                               dim3(kHubThreads), 0, r.stream, r.g, r.a, r.b, r.mh_out, r.p, r.hll_out, r.cards_out, r.cards_stride, r.prm);
        };
        if (r.mh_out && r.hll_out) launch(std::true_type{}, std::true_type{});
        else if (r.mh_out) launch(std::true_type{}, std::false_type{});
        else launch(std::false_type{}, std::true_type{});
    });
    SS_LAUNCH_CHECK();
    return SS_OK;
}

// ... as ONE hub pass under a span of its own: what a call that builds both hop-1 tables, or the fused stage, did not have hosted
int launch_first_hop_hub_only(const HopRequest &r)
{
    if (!r.g.hub_rows || !r.g.hub_count || (!r.mh_out && !r.hll_out)) return SS_OK;
    ProfileSpan span(r.stream, SS_PROF_HUB);
    return launch_first_hop_hubs(r);
}

}  // namespace ss

extern "C" int ss_first_hop(const ss_csr_graph *graph, const uint64_t *a, const uint64_t *b, int32_t P,
                            uint32_t *mh_out, int32_t p, uint8_t *hll_out, float *cards_out, int64_t cards_stride,
                            const ss_hll_params *prm, void *stream)
{
    using namespace ss;
    if (!graph_given(graph)) return SS_ERR_INVALID_ARG;
    // written out: a shape without a kernel is answered before N is looked at (the caller falls back to init + propagate)
    // (the MinHash rows do not depend on p: a MinHash-only call is served for every hll_p; the HLL row image is 256 registers)
    if ((hll_out && p != 8) || P <= 0 || P % kWave || P > 256) return SS_ERR_UNSUPPORTED;
    if (graph->num_nodes == 0) return SS_OK;
    if ((!mh_out && !hll_out) || (mh_out && (!a || !b))) return SS_ERR_INVALID_ARG;  // either sketch may be NULL; a / b only feed MinHash
    if (!graph_fits(*graph)) return SS_ERR_INVALID_ARG;
    HopRequest r;
    r.a = a;
    r.b = b;
    r.P = P;
    r.p = p;
    r.M = 256;
    r.mh_out = mh_out;
    r.hll_out = hll_out;
    r.cards_out = cards_out;
    r.cards_stride = cards_stride;
    r.stream = (hipStream_t)stream;
    int rc = take_params(r, prm);
    if (rc != SS_OK) return rc;
    if (!row_range_ok(*graph)) return SS_ERR_INVALID_ARG;  // (here the parameters are judged before the row range)
    r.g = to_args(*graph);
    if (r.g.rows() == 0) return SS_OK;
    schedule_hubs(r, true);
    // both sketches: the latency-optimised HLL kernel + the MinHash kernel beat the combined kernel (37 + 134 us vs 184 us on the
    // bench graph); the HLL launch hosts the hub units of both tables, or ONE hub pass serves both.  HLL alone: 16-lane-per-row
    // kernel for the regular rows, the cooperative hub kernel for the rest
    if (!hll_out) {  // MinHash alone: its row kernel hosts no units, the hub launch follows under either schedule (and gets no stride)
        r.lead = 0;
        r.cards_stride = 0;
    }
    if (hll_out) rc = launch_hll_first_hop_rows(r, nullptr);
    if (rc == SS_OK && mh_out) rc = launch_minhash_rows(r);
    if (rc != SS_OK || !r.hub_launch_follows()) return rc;
    return mh_out && hll_out ? launch_first_hop_hub_only(r) : launch_first_hop_hubs(r);  // (a single sketch's hub launch leaves no span)
}
