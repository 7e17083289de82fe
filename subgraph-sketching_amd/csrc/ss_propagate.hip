// ss_propagate.hip -- one hop of sketch propagation (CSR pull) + fused HLL++ cardinality.
//
// Replaces MinhashPropagation / HllPropagation (reference hashing.py:28-45) and the per-hop hll_count of
// build_hash_tables (hashing.py:160-163).  HBM-bound: per hop it streams (E' + N) sketch rows.
//
// Mapping: one wavefront per destination row.  A 16-byte chunk per lane; a MinHash row of P u32 is
// CM = P/4 chunks, an HLL row of M bytes is CH = M/16 chunks.  The wave is split into G = 64/SG
// sub-groups (SG = pow2 >= chunks per row, <= 64) that walk G neighbours concurrently
// (P=128: 2 neighbours per step, M=256: 4), so every global load is a coalesced dwordx4 and a step
// moves 1 KiB per wave.  Partial min / max are combined across sub-groups once per row with
// cross-lane shuffles.  The implicit self loop (i < n_self) is one extra virtual neighbour -- left out, for rows that have an
// in-edge, when the graph is symmetric and the inputs are hop tables of it (GraphArgs.skip_self, ss_common.hpp table_hop_total).
//
// Hub rows (in-degree > graph.hub_threshold, listed by ss_csr_build) would serialise tens of thousands of
// dependent 1 KiB loads on one wavefront (power-law graphs: ogbl-ppa, ogbl-citation2).  The row wavefronts
// skip them; the LEADING `hub_blocks` workgroups of the same launch walk them as hub units (ss_hub.hpp: a whole
// workgroup per row or slice of a row, partials combined through LDS).
#include "ss_hub.hpp"

namespace ss {

// TP / TM > 0: compile-time row sizes (fast path); 0: run-time.
template <int TP, int TM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void propagate_kernel(GraphArgs g, const uint32_t *__restrict__ mh_in, uint32_t *__restrict__ mh_out,
                                                        int P_rt, const uint8_t *__restrict__ hll_in, uint8_t *__restrict__ hll_out,
                                                        int M_rt, float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm,
                                                        bool skip_hubs, int hub_blocks, const uint8_t *__restrict__ hub_hll_in,
                                                        uint8_t *__restrict__ hub_hll_out, float *__restrict__ hub_cards_out)
{
    __shared__ EstimatorLds lds;
    // (workgroup-uniform; the row workgroups of a MinHash-only launch must not pay for the tables a leading workgroup needs: staged
    // by all 59 000 workgroups of the bench graph's launch they cost it 13 us)
    const bool hub_hll_block = TP == 128 && TM == 256 && hub_hll_out != nullptr && (int)blockIdx.x < hub_blocks && (int)blockIdx.x >= hub_blocks / 2;
    const bool want_cards = (cards_out != nullptr && hll_out != nullptr) || (hub_hll_block && hub_cards_out != nullptr);
    EstimatorTables est;
    if (want_cards) est = stage_tables(lds, prm);
    if constexpr (TP == 128 && TM == 256) {  // (this instantiation is only ever launched for the MinHash rows alone)
        if ((int)blockIdx.x < hub_blocks) {
            // workgroup-uniform: a leading workgroup serves hub units (ss_hub.hpp) of this hop's MinHash table or -- with hub_hll_out,
            // the second half of the leading workgroups, tickets of their own -- of its HLL table (ss_fused_hop_stage: the kernel
            // that computes the HLL rows has no register to spare for them)
            __shared__ TableHubLds<kHubLeadWaves> hub;
            const int half = hub_hll_out ? hub_blocks / 2 : hub_blocks;
            if ((int)blockIdx.x < half)
                table_hub_units<kHubLeadWaves, true, false>(g, (int)blockIdx.x, half, mh_in, mh_out, nullptr, nullptr, nullptr, 0, est, false, hub);
            else
                table_hub_units<kHubLeadWaves, false, true>(g, (int)blockIdx.x - half, hub_blocks - half, nullptr, nullptr, hub_hll_in, hub_hll_out,
                                                            hub_cards_out, cards_stride, est, hub_cards_out != nullptr, hub);
            return;
        }
    }

    const bool row_cards = cards_out != nullptr && hll_out != nullptr;
    const int P = TP ? TP : P_rt;
    const int M = TM ? TM : M_rt;
    const int lane = threadIdx.x & (kWave - 1);
    // wave-uniform row id (readfirstlane makes the uniformity visible to the compiler: scalar loads, scalar loop control)
    int64_t i = g.row0 + (int64_t)((int)blockIdx.x - hub_blocks) * (blockDim.x / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (g.row_list) {  // ss_minhash_hop_rows: the q-th wavefront computes row row_list[q]
        const int64_t q = i - g.row0;
        if (q >= g.n_list) return;
        i = g.row_list[q];
        i = i < 0 ? i + g.N : i;
        if ((uint64_t)i >= (uint64_t)g.N) return;  // the query kernel reports such ids; nothing to compute here
    } else if (i >= g.row1) {
        return;
    }

    const int64_t rb = g.rowptr[i];
    const int deg = (int)(g.rowptr[i + 1] - rb);
    if (skip_hubs && deg > g.hub_threshold) return;  // a hub unit (ss_hub.hpp)
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    const bool skip_self = g.skip_self && *g.skip_self != 0;  // (one scalar load per wavefront)
    const int total = table_hop_total(deg, i < n_self, skip_self);
    const int32_t *nb = g.col + rb;

    // ---------------- MinHash: min over neighbours ----------------
    if (mh_out)
        minhash_hop_row<TP>(mh_in, nb, deg, total, i, P, lane, 0, 1, [&](int c, bool mine, const u32x4 &acc) {
            if (mine) {
                *reinterpret_cast<u32x4 *>(mh_out + i * P + 4 * c) = acc;
                mirror_mh4(g.mir, i * P + 4 * c, acc);
            }
        });

    // ---------------- HLL: byte-wise max over neighbours, fused cardinality ----------------
    if (hll_out)
        hll_hop_row<TM>(
            hll_in, nb, deg, total, i, M, lane, 0, 1, row_cards, est,
            [&](int c, bool mine, const u32x4 &acc) {
                if (mine) {
                    *reinterpret_cast<u32x4 *>(hll_out + i * M + 16 * c) = acc;
                    mirror_hll16(g.mir, i * M + 16 * c, acc);
                }
                return mine;
            },
            [&](float card) {
                cards_out[i * cards_stride] = card;
                mirror_card(g.mir, i * cards_stride, card);
            });
}

// HLL-only hop, 4 destinations per wavefront (fast path of ss_propagate when the MinHash sketch is absent)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void hll_propagate_row16_kernel(GraphArgs g, const uint8_t *__restrict__ hll_in,
                                                                  uint8_t *__restrict__ hll_out, float *__restrict__ cards_out,
                                                                  int64_t cards_stride, ss_hll_params prm, bool skip_hubs, int hub_blocks)
{
    __shared__ EstimatorLds lds;
    const bool want_cards = cards_out != nullptr;
    EstimatorTables est;
    if (want_cards) est = stage_tables(lds, prm);
    if ((int)blockIdx.x < hub_blocks) {  // workgroup-uniform: a leading workgroup serves hub units of this hop's HLL table
        __shared__ TableHubLds<kHubLeadWaves> hub;
        table_hub_units<kHubLeadWaves, false, true>(g, (int)blockIdx.x, hub_blocks, nullptr, nullptr, hll_in, hll_out, cards_out, cards_stride, est,
                                                    want_cards, hub);
        return;
    }
    // the 16 rows of this workgroup are dealt to its 16 lane groups in DEGREE order: the four rows that share a wavefront
    // then have similar degrees, and the walk of a wavefront lasts as long as its longest row
    __shared__ int s_deg[256 / kRow], s_owner[256 / kRow];
    const int grp = threadIdx.x / kRow, c16 = threadIdx.x & (kRow - 1);
    const int64_t first = g.row0 + (int64_t)((int)blockIdx.x - hub_blocks) * (blockDim.x / kRow);
    {
        const int64_t r = first + grp;
        const int d = r < g.row1 ? (int)(g.rowptr[r + 1] - g.rowptr[r]) : -1;
        if (c16 == 0) s_deg[grp] = d;
        __syncthreads();
        const int dj = s_deg[c16];
        const bool before = dj < d || (dj == d && c16 < grp);
        const unsigned long long b = __ballot(before);
        const int rank = __popcll((b >> (kRow * ((threadIdx.x & (kWave - 1)) / kRow))) & 0xFFFFull);
        if (c16 == 0) s_owner[rank] = grp;
        __syncthreads();
    }
    const int64_t row = first + s_owner[grp];
    hll_hop_row16(g, row < g.row1 ? row : -1, skip_hubs, hll_in, hll_out, cards_out, cards_stride, est, want_cards, threadIdx.x & (kRow - 1));
}

// ---- hub units as a launch of their own (16 wavefronts per workgroup): the shapes / calls whose row kernel does not host them,
// and SS_HUB_LAUNCHES=1; P = 128, M = 256 only
constexpr int kHubThreads = 1024;
constexpr int kHubWaves = kHubThreads / kWave;
constexpr int kHubGrid = 256;  // one workgroup per CU; workgroups beyond the unit count exit at once

template <bool DO_MH, bool DO_HLL>
__global__ __launch_bounds__(kHubThreads) void propagate_hub_kernel(GraphArgs g, const uint32_t *__restrict__ mh_in,
                                                                    uint32_t *__restrict__ mh_out, const uint8_t *__restrict__ hll_in,
                                                                    uint8_t *__restrict__ hll_out, float *__restrict__ cards_out,
                                                                    int64_t cards_stride, ss_hll_params prm)
{
    __shared__ EstimatorLds lds;
    __shared__ TableHubLds<kHubWaves> hub;
    const HubCounts n = hub_counts(g);
    if ((int)blockIdx.x >= n.hubs + n.slices) return;  // the common case (no hub rows) costs three scalar loads per workgroup
    const bool want_cards = DO_HLL && cards_out != nullptr;
    EstimatorTables est = {};
    if (want_cards) est = stage_tables(lds, prm);
    table_hub_units<kHubWaves, DO_MH, DO_HLL>(g, (int)blockIdx.x, (int)gridDim.x, mh_in, mh_out, hll_in, hll_out, cards_out, cards_stride, est,
                                              want_cards, hub);
}

// ---- host: each kernel above has ONE launch expression --------------------------------------------------------------------------

// propagate_kernel, four rows per workgroup behind r.lead leading workgroups: n_rows of the row range, or entries of the row list.
// <128, 256> is only ever launched for the MinHash rows alone and hosts the hub units of the MinHash table -- with `hub_hll`, the
// request whose HLL tables the stage computes beside it, the second half of the leading workgroups serves that table's units;
// <0, 0> takes r.P / r.M at run time and has no hub units
template <int TP, int TM>
static void launch_propagate_kernel(ProfileSpan &span, const HopRequest &r, int64_t n_rows, const HopRequest *hub_hll)
{
    span.launch(propagate_kernel<TP, TM>, dim3((unsigned)((n_rows + 3) / 4 + r.lead)), dim3(256), r.g, r.mh_in, r.mh_out, TP ? TP : r.P, r.hll_in,
                r.hll_out, TM ? TM : r.M, r.cards_out, r.cards_stride, r.prm, r.hubs, r.lead, hub_hll ? hub_hll->hll_in : nullptr,
                hub_hll ? hub_hll->hll_out : nullptr, hub_hll ? hub_hll->cards_out : nullptr);
}

// the MinHash table hop alone (P = 128) of a request that may name HLL tables too: the regular rows and -- r.lead leading workgroups --
// the hub units of the MinHash table and, with host_hll, of the HLL table of the same hop (r.cards_out / cards_stride / prm: its
// cardinalities)
int launch_minhash_hop(const HopRequest &r, bool host_hll)
{
    HopRequest rows = r;
    rows.hll_in = nullptr;
    rows.hll_out = nullptr;
    rows.cards_out = nullptr;
    if (!host_hll) rows.cards_stride = 0;
    ProfileSpan span(r.stream, SS_PROF_MINHASH_HOP, true);
    launch_propagate_kernel<128, 256>(span, rows, r.g.rows(), host_hll ? &r : nullptr);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

// the hub units of a table hop as a launch of their own (16-wave workgroups): what the row launches above did not host
int launch_propagate_hub_only(const HopRequest &r)
{
    if (!r.g.hub_rows || !r.g.hub_count || (!r.mh_out && !r.hll_out)) return SS_OK;
    ProfileSpan span(r.stream, SS_PROF_HUB);
    const auto launch = [&](auto mh, auto hll) {
        hipLaunchKernelGGL((propagate_hub_kernel<decltype(mh)::value, decltype(hll)::value>), dim3(kHubGrid), dim3(kHubThreads), 0, r.stream, r.g,
                           r.mh_in, r.mh_out, r.hll_in, r.hll_out, r.cards_out, r.cards_stride, r.prm);
    };
    if (r.mh_out && r.hll_out) launch(std::true_type{}, std::true_type{});
    else if (r.mh_out) launch(std::true_type{}, std::false_type{});
    else launch(std::false_type{}, std::true_type{});
    SS_LAUNCH_CHECK();
    return SS_OK;
}

// the HLL table hop alone (M = 256): 4 destinations per wavefront + the hub units of the HLL table
static int launch_hll_hop(const HopRequest &r)
{
    ProfileSpan span(r.stream, SS_PROF_HLL_HOP);
    hipLaunchKernelGGL(hll_propagate_row16_kernel, dim3((unsigned)((r.g.rows() + 15) / 16 + r.lead)), dim3(256), 0, r.stream, r.g, r.hll_in,
                       r.hll_out, r.cards_out, r.cards_stride, r.prm, r.hubs, r.lead);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

}  // namespace ss

// MinHash table hop of the listed rows only (+ the hub units, which always cover every hub row)
extern "C" int ss_minhash_hop_rows(const ss_csr_graph *graph, const uint32_t *mh_in, uint32_t *mh_out, int32_t P, const int64_t *rows,
                                   int64_t n_rows, void *stream)
{
    using namespace ss;
    if (!graph_given(graph) || !mh_in || !mh_out || n_rows < 0 || (n_rows > 0 && !rows)) return SS_ERR_INVALID_ARG;
    if (P <= 0 || (P & 3) || P > 2048) return SS_ERR_INVALID_ARG;
    if (graph->num_nodes == 0 || n_rows == 0) return SS_OK;
    if (!graph_fits(*graph) || n_rows >= ((int64_t)1 << 33)) return SS_ERR_INVALID_ARG;
    if (graph->row_begin != 0 || graph->row_end != 0) return SS_ERR_INVALID_ARG;  // a row list and a row range exclude each other
    HopRequest r;
    r.g = to_args(*graph);
    r.mh_in = mh_in;
    r.mh_out = mh_out;
    r.P = P;
    r.M = 256;
    r.stream = (hipStream_t)stream;
    schedule_hubs(r, P == 128);  // (the hub units of the table hops are P = 128 only, as in ss_propagate)
    HopRequest listed = r;
    listed.g.row_list = rows;
    listed.g.n_list = n_rows;
    {
        ProfileSpan span(r.stream, SS_PROF_MINHASH_ROWS);
        if (P == 128) launch_propagate_kernel<128, 256>(span, listed, n_rows, nullptr);
        else launch_propagate_kernel<0, 0>(span, listed, n_rows, nullptr);
    }
    SS_LAUNCH_CHECK();
    return r.hub_launch_follows() ? launch_propagate_hub_only(r) : SS_OK;
}

extern "C" int ss_propagate(const ss_csr_graph *graph, const uint32_t *mh_in, uint32_t *mh_out, int32_t P,
                            const uint8_t *hll_in, uint8_t *hll_out, int32_t M,
                            float *cards_out, int64_t cards_stride, const ss_hll_params *prm, void *stream)
{
    using namespace ss;
    if (!graph_given(graph)) return SS_ERR_INVALID_ARG;
    if (graph->num_nodes == 0) return SS_OK;
    if (!row_range_ok(*graph)) return SS_ERR_INVALID_ARG;  // (here the row range is judged before the parameters)
    if ((mh_in == nullptr) != (mh_out == nullptr) || (hll_in == nullptr) != (hll_out == nullptr)) return SS_ERR_INVALID_ARG;
    if (!mh_out && !hll_out) return SS_ERR_INVALID_ARG;
    if (mh_out && (P <= 0 || (P & 3) || P > 2048)) return SS_ERR_INVALID_ARG;
    if (hll_out && (M < 16 || (M & (M - 1)) || M > 65536)) return SS_ERR_INVALID_ARG;
    if (!graph_fits(*graph)) return SS_ERR_INVALID_ARG;
    HopRequest r;
    r.mh_in = mh_in;
    r.mh_out = mh_out;
    r.P = P;
    r.hll_in = hll_in;
    r.hll_out = hll_out;
    r.M = M;
    r.cards_out = cards_out;
    r.cards_stride = cards_stride;
    r.stream = (hipStream_t)stream;
    int rc = take_params(r, prm);
    if (rc != SS_OK) return rc;
    r.g = to_args(*graph);
    if (r.g.rows() == 0) return SS_OK;
    schedule_hubs(r, true);
    if (hll_out && M == 256 && (!mh_out || P == 128)) {
        // HLL alone: 4 destinations per wavefront.  Both sketches: one launch per sketch is faster than the two-sketch kernel
        // (192 + 111 us vs 326 us on the bench graph): the HLL kernel keeps 4 destinations in flight per wavefront, the MinHash kernel
        // one; each launch hosts the hub units of its own sketch
        rc = launch_hll_hop(r);
        if (rc == SS_OK && mh_out) rc = launch_minhash_hop(r, false);
        return rc != SS_OK || !r.hub_launch_follows() ? rc : launch_propagate_hub_only(r);
    }
    if (!hll_out && P == 128) {  // MinHash alone on the fast path: the row kernel that hosts its hub units
        if (r.hubs) note_hub_call();  // (this path has always been counted twice; ss_debug_hub_calls is compared between builds)
        {
            ProfileSpan span(r.stream, SS_PROF_MINHASH_HOP);
            launch_propagate_kernel<128, 256>(span, r, r.g.rows(), nullptr);
        }
        SS_LAUNCH_CHECK();
        return r.hub_launch_follows() ? launch_propagate_hub_only(r) : SS_OK;
    }
    // any other shape: row sizes at run time, every row a wavefront's (no hub units, no span family)
    r.hubs = false;
    r.lead = 0;
    {
        ProfileSpan span(r.stream, SS_PROF_TAGS);
        launch_propagate_kernel<0, 0>(span, r, r.g.rows(), nullptr);
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}
