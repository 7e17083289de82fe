// ss_hub.hpp -- hub units: the rows the row kernels leave out (in-degree > graph.hub_threshold, listed by ss_csr_build), walked by
// whole workgroups.
//
// A row of tens of thousands of neighbours on one wavefront is tens of thousands of dependent loads (power-law graphs: ogbl-ppa,
// ogbl-citation2).  The CSR build lists such rows -- `hub_rows` (at most SS_MEGA_SLICE neighbours: one unit each) and `mega_rows`
// (more: one unit per slice of SS_MEGA_SLICE neighbours; the partial rows go through mega_scratch and the workgroup that finishes a
// row's LAST slice -- ticket counter -- combines them) -- and a unit is walked by all wavefronts of a workgroup, 64-neighbour chunks
// dealt round robin, partials combined through LDS.
//
// Round 4: the units are served by the LEADING workgroups of a row kernel's own launch (`hub_blocks` of them, 256 threads = 4
// wavefronts each; the row workgroups follow).  As launches of their own (rounds 1-3: 256 workgroups of 16 wavefronts after every
// row kernel) the passes were a serial chain of ~15-40 us per hop that nothing overlapped -- 35 us of a 0.49 ms step at rank^-0.5,
// 113 us of 0.52 ms at rank^-0.9 --, and on a second stream they only started in the row kernel's tail.  Inside the
// launch they start FIRST (workgroups are dispatched in index order) and the row workgroups fill the chip around them.
// Which launch hosts what: the HLL first-hop launch both hop-1 tables' units, the MinHash table-hop launch both tables' units of
// its hop (ss_fused_hop_stage) or its own sketch's (ss_propagate); the fused kernel hosts none -- it has no register to spare.
// The stand-alone kernels remain for the shapes without a specialised row kernel and for A/B runs (SS_HUB_LAUNCHES=1).
//
// Tickets: a mega row has one counter per sketch side (descriptor words 3 / 4), because MinHash units and HLL units of the same
// rows are served by different workgroups of ONE launch, at the same time.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "ss_walks.hpp"

namespace ss {

constexpr int kHubLeadBlocks = 1024;  // leading workgroups of a row launch (four per CU); those beyond the unit count exit at once
constexpr int kHubLeadWaves = 4;
constexpr int kMegaDesc = SS_MEGA_DESC_WORDS;  // int32 words per mega-row descriptor: {row, first slice, slices, ticket (MinHash side), ticket (HLL side), 0, 0, 0}

// host: how many leading workgroups a row launch gets (0: the stand-alone hub kernels follow the launch instead)
void note_hub_call();  // ss_debug.hip: ss_debug_hub_calls counts the library calls that served hub units
inline int hub_lead_blocks(bool hubs)
{
    if (hubs) note_hub_call();
    static const bool launches = getenv("SS_HUB_LAUNCHES") && atoi(getenv("SS_HUB_LAUNCHES")) != 0;
    // (the launches split the leading workgroups by integer division -- a quarter of them for the hop-1 HLL units, half for the MinHash
    // units -- and every share must hold a workgroup)
    static_assert(kHubLeadBlocks >= 4, "every share of the leading workgroups holds one");
    return hubs && !launches ? kHubLeadBlocks : 0;
}

// ---- host side of the table build (ss_first_hop.hip, ss_propagate.hip, ss_fused_hop.hip, the tail of ss_update.hip) -----------------
// What one call asks of its launches.  An extern "C" entry point fills one record after its checks; where its launches differ in a
// few fields it copies the record and sets those by name.  A null table: that sketch is not part of the launch.
struct HopRequest {
    GraphArgs g;
    const uint64_t *a = nullptr, *b = nullptr;  // MinHash permutations (the hops from node ids)
    int P = 0, p = 0, M = 0;                    // permutations, hll_p, HLL registers
    const uint32_t *mh_in = nullptr;            // input tables: the table hops only
    uint32_t *mh_out = nullptr;
    const uint8_t *hll_in = nullptr;
    uint8_t *hll_out = nullptr;
    float *cards_out = nullptr;
    int64_t cards_stride = 0;
    ss_hll_params prm = {};                     // (zeros unless cards_out, take_params)
    hipStream_t stream = nullptr;
    // the hub schedule (schedule_hubs): the row kernels leave the listed rows out, `lead` leading workgroups of a row launch serve them
    bool hubs = false;
    int lead = 0;
    bool hub_launch_follows() const { return hubs && lead == 0; }  // no row launch hosted the units: the stand-alone hub kernel runs
};

// The hub schedule of one library call, asked once: are hub rows listed, does a row launch host their units, or does a hub launch
// follow.  (hub_lead_blocks also counts the call for ss_debug_hub_calls.)  `served`: the call's kernels have hub units for its shape
inline void schedule_hubs(HopRequest &r, bool served)
{
    r.hubs = served && r.g.hub_rows && r.g.hub_count;
    r.lead = hub_lead_blocks(r.hubs);
}

// f(std::integral_constant<int, PPL>) for the PPL = P / 64 permutations a lane owns, 1 .. 4 (anything else: 4)
template <class F>
inline void for_ppl(int P, F &&f)
{
    switch (P / kWave) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// The entry preamble's shared checks, in the two places every entry point has them: before its N == 0 exit ...
inline bool graph_given(const ss_csr_graph *graph) { return graph && graph->num_nodes >= 0 && graph->rowptr; }
// ... and after it: node ids fit 31 bits and the hub list comes with its count
inline bool graph_fits(const ss_csr_graph &graph)
{
    return graph.num_nodes < ((int64_t)1 << 31) && (graph.hub_rows == nullptr) == (graph.hub_count == nullptr);
}
// r.cards_out asks for cardinalities: of an HLL table this call writes, with usable parameters for rows of r.M registers
inline int take_params(HopRequest &r, const ss_hll_params *prm)
{
    if (!r.cards_out) return SS_OK;
    if (!r.hll_out) return SS_ERR_INVALID_ARG;
    const int rc = check_params(prm);
    if (rc != SS_OK) return rc;
    if ((1 << prm->p) != r.M) return SS_ERR_INVALID_ARG;
    r.prm = *prm;
    return SS_OK;
}

// launches defined in ss_first_hop.hip / ss_propagate.hip that ss_fused_hop_stage strings together as well
// (records: nullable; the regular-row groups also leave every row's code record there, hll_first_hop_row16)
int launch_hll_first_hop_rows(const HopRequest &r, uint32_t *records);
int launch_first_hop_hub_only(const HopRequest &r);
int launch_minhash_hop(const HopRequest &r, bool host_hll);
int launch_propagate_hub_only(const HopRequest &r);

struct HubCounts {
    int hubs, mega, slices;
};
__device__ __forceinline__ HubCounts hub_counts(const GraphArgs &g)
{
    return HubCounts{*g.hub_count, g.mega_count ? g.mega_count[0] : 0, g.mega_count ? g.mega_count[1] : 0};
}

// the mega row global slice `gs` belongs to: every thread looks at some descriptors (a per-row loop over all mega rows cost every
// workgroup three dependent loads per ROW, slices or not).  Called by all threads; ends with a barrier.
template <int THREADS>
__device__ __forceinline__ int mega_row_of_slice(const GraphArgs &g, int gs, int n_mega, int &s_m)
{
    for (int t = threadIdx.x; t < n_mega; t += THREADS) {
        const int4 d = *reinterpret_cast<const int4 *>(g.mega_rows + (int64_t)kMegaDesc * t);
        if (gs >= d.y && gs < d.y + d.z) s_m = t;
    }
    __syncthreads();
    return s_m;
}

// ---- table hops (P = 128, M = 256): min / byte-wise max over the neighbours' rows of the previous hop ------------------------
template <int WAVES>
struct TableHubLds {
    u32x4 part_mh[WAVES][32];
    u32x4 part_hll[WAVES][16];
    int s_last, s_m;
};

// worker / n_workers: this workgroup's place among the workgroups that serve units (units are dealt round robin: hub row h to
// worker h % n_workers, global slice gs to (hubs + gs) % n_workers)
template <int WAVES, bool DO_MH, bool DO_HLL>
__device__ __forceinline__ void table_hub_units(const GraphArgs &g, int worker, int n_workers, const uint32_t *__restrict__ mh_in,
                                                uint32_t *__restrict__ mh_out, const uint8_t *__restrict__ hll_in,
                                                uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride,
                                                const EstimatorTables &est, bool want_cards, TableHubLds<WAVES> &s)
{
    constexpr int P = 128, M = 256, CM = 32, CH = 16, THREADS = WAVES * kWave;
    constexpr int kTicket = DO_MH ? 3 : 4;
    const HubCounts n = hub_counts(g);
    if (worker >= n.hubs + n.slices) return;  // the common case (few or no hub rows) costs three scalar loads per workgroup
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;

    // all waves walk the neighbours t in [lo, hi) of row i; wave 0 ends up with the combined partial rows
    // (MinHash chunk `lane` in lanes 0..31, HLL chunk `lane - 32` in lanes 32..47)
    // (wave w takes the CONTIGUOUS 64-neighbour chunks w, w + WAVES, ... of [lo, hi): ids by one coalesced load per chunk, handed
    // out with v_readlane (MinHash) / DPP row broadcasts (HLL: 16 neighbours per lane group) -- one round trip per chunk instead
    // of the generic walk's two per batch of four)
    auto walk = [&](int64_t i, const int32_t *nb, int deg, int lo, int hi, u32x4 &mh_acc, u32x4 &hll_acc) {
        if constexpr (DO_MH) {
            const int sg = lane >> 5, c = lane & 31;
            u32x4 acc = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            for (int b = lo + wave * kWave; b < hi; b += WAVES * kWave)  // wave-uniform
                acc = min4(acc, minhash_chunk64(mh_in, nb + b, deg - b, hi - b < kWave ? hi - b : kWave, i, lane));
            acc = min4(acc, shfl_xor4(acc, 32));
            if (sg == 0) s.part_mh[wave][c] = acc;
        }
        if constexpr (DO_HLL) {
            const int sg = lane >> 4, c = lane & 15;
            u32x4 acc = {0u, 0u, 0u, 0u};
            for (int b = lo + wave * kWave; b < hi; b += WAVES * kWave) {
                const int bg = b + kRow * sg;  // this lane group's 16 neighbours of the chunk
                acc = bytemax16(acc, hll_walk_first16(hll_in, nb + bg, deg - bg, hi - bg, i, c));
            }
            acc = bytemax16(acc, shfl_xor4(acc, 16));
            acc = bytemax16(acc, shfl_xor4(acc, 32));
            if (sg == 0) s.part_hll[wave][c] = acc;
        }
        __syncthreads();
        if (wave == 0) {
            if (DO_MH && lane < CM) {
                mh_acc = s.part_mh[0][lane];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) mh_acc = min4(mh_acc, s.part_mh[w][lane]);
            }
            if (DO_HLL && lane >= 32 && lane < 32 + CH) {
                hll_acc = s.part_hll[0][lane - 32];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) hll_acc = bytemax16(hll_acc, s.part_hll[w][lane - 32]);
            }
        }
    };
    // wave 0 stores the finished row (+ its cardinality)
    auto finish = [&](int64_t i, u32x4 mh_acc, u32x4 hll_acc) {
        if (DO_MH && lane < CM) {
            *reinterpret_cast<u32x4 *>(mh_out + i * P + 4 * lane) = mh_acc;
            mirror_mh4(g.mir, i * P + 4 * lane, mh_acc);
        }
        if (DO_HLL && lane >= 32 && lane < 32 + CH) {  // lanes 32..47 = one DPP row
            const int c = lane - 32;
            *reinterpret_cast<u32x4 *>(hll_out + i * M + 16 * c) = hll_acc;
            mirror_hll16(g.mir, i * M + 16 * c, hll_acc);
            if (want_cards) {
                int nonzero = 0;
                float hsum = 0.0f;
                hll_chunk_stats(hll_acc, nonzero, hsum);
                nonzero = row16_sum_i(nonzero);
                hsum = row16_sum_f(hsum);
                if (c == 0) {
                    const float card = hll_estimate(est, M - nonzero, hsum);
                    cards_out[i * cards_stride] = card;
                    mirror_card(g.mir, i * cards_stride, card);
                }
            }
        }
    };

    for (int h = worker; h < n.hubs; h += n_workers) {
        const int64_t i = g.hub_rows[h];
        if (!g.owns(i)) continue;  // workgroup-uniform
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        u32x4 mh_acc = {0u, 0u, 0u, 0u}, hll_acc = {0u, 0u, 0u, 0u};
        walk(i, g.col + rb, deg, 0, total, mh_acc, hll_acc);
        if (wave == 0) finish(i, mh_acc, hll_acc);
        __syncthreads();
    }

    // ---- mega rows: the slices of ALL mega rows form one list (slice s of the row with first slice f is global slice f + s) that
    // continues the round robin of the hub rows above.  A row with a million neighbours is spread over the whole chip instead of
    // being one workgroup's serial walk.
    for (int gs = (int)((unsigned)(worker + n_workers - n.hubs % n_workers) % (unsigned)n_workers); gs < n.slices; gs += n_workers) {
        const int m = mega_row_of_slice<THREADS>(g, gs, n.mega, s.s_m);
        int32_t *desc = g.mega_rows + (int64_t)kMegaDesc * m;
        const int4 e = *reinterpret_cast<const int4 *>(desc);  // {row, first slice, slices, -}
        const int64_t i = e.x;
        if (!g.owns(i)) { __syncthreads(); continue; }  // workgroup-uniform
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        const int sl = gs - e.y;
        const int lo = sl * SS_MEGA_SLICE < total ? sl * SS_MEGA_SLICE : total;
        const int hi = lo + SS_MEGA_SLICE < total ? lo + SS_MEGA_SLICE : total;
        u32x4 mh_acc = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hll_acc = {0u, 0u, 0u, 0u};
        walk(i, g.col + rb, deg, lo, hi, mh_acc, hll_acc);
        uint8_t *mine = g.mega_scratch + (int64_t)(e.y + sl) * kMegaSlot;
        if (wave == 0) {
            if (DO_MH && lane < CM) coherent_store4(mine + 16 * lane, mh_acc);
            if (DO_HLL && lane >= 32 && lane < 32 + CH) coherent_store4(mine + kMegaHllOffset + 16 * (lane - 32), hll_acc);
        }
        publish_drain();  // every wave: the slot stores are acknowledged before the barrier that precedes the ticket
        __syncthreads();
        if (threadIdx.x == 0) {
            const int prev = take_ticket(desc + kTicket);
            s.s_last = prev == e.z - 1;
            if (s.s_last) reset_ticket(desc + kTicket);  // every slice has arrived: ready for the next hop
        }
        __syncthreads();
        if (s.s_last) {  // workgroup-uniform.  All waves read the slots (wave w: slots w, w + WAVES, ...: a row of 70 000 neighbours has
                         // 69 of them), wave 0 combines and stores
            u32x4 mh_all = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hll_all = {0u, 0u, 0u, 0u};
            constexpr int kSlotsInFlight = WAVES >= 16 ? 1 : 2;  // (more would cost the hosting row kernels registers they do not have)
            for (int q = wave; q < e.z; q += kSlotsInFlight * WAVES) {
                u32x4 v[kSlotsInFlight];
#pragma unroll
                for (int k = 0; k < kSlotsInFlight; ++k) {
                    const int qq = q + k * WAVES < e.z ? q + k * WAVES : q;  // (past the end: slot q again -- min / max do not mind)
                    const uint8_t *part = g.mega_scratch + (int64_t)(e.y + qq) * kMegaSlot;
                    v[k] = u32x4{0u, 0u, 0u, 0u};
                    if (DO_MH && lane < CM) v[k] = coherent_load4(part + 16 * lane);
                    if (DO_HLL && lane >= 32 && lane < 32 + CH) v[k] = coherent_load4(part + kMegaHllOffset + 16 * (lane - 32));
                }
#pragma unroll
                for (int k = 0; k < kSlotsInFlight; ++k) {
                    if (DO_MH && lane < CM) mh_all = min4(mh_all, v[k]);
                    if (DO_HLL && lane >= 32 && lane < 32 + CH) hll_all = bytemax16(hll_all, v[k]);
                }
            }
            if (DO_MH && lane < CM) s.part_mh[wave][lane] = mh_all;
            if (DO_HLL && lane >= 32 && lane < 32 + CH) s.part_hll[wave][lane - 32] = hll_all;
            __syncthreads();
            if (wave == 0) {
                if (DO_MH && lane < CM) {
#pragma unroll
                    for (int w = 1; w < WAVES; ++w) mh_all = min4(mh_all, s.part_mh[w][lane]);
                }
                if (DO_HLL && lane >= 32 && lane < 32 + CH) {
#pragma unroll
                    for (int w = 1; w < WAVES; ++w) hll_all = bytemax16(hll_all, s.part_hll[w][lane - 32]);
                }
                finish(i, mh_all, hll_all);
            }
        }
        __syncthreads();
    }
}

// ---- first hop (hop 1 from node ids, ss_first_hop.hip): P = 64 * PPL, M = 256 ---------------------------------------------------
template <int PPL>
struct FirstHopHubLds {
    __attribute__((aligned(16))) uint32_t hll_row[256];
    uint32_t mh_row[PPL * kWave];
    int s_last, s_m;
};

// all WAVES wavefronts of the workgroup hash the neighbours t in [lo, hi) of row i (batches of 64, one batch per wave and step); the
// combined partial rows are left in s.mh_row / s.hll_row.  Called by every thread; begins and ends with a barrier.
// (first_hop_hub_units below: a hub row or a slice of a mega row; update_hub_first_kernel of ss_update.hip: a whole listed row)
template <int PPL, int WAVES, bool DO_MH, bool DO_HLL>
__device__ __forceinline__ void first_hop_hub_walk(FirstHopHubLds<PPL> &s, int64_t i, const int32_t *__restrict__ nb, int deg, int lo, int hi,
                                                   int p, const uint64_t (&a)[PPL], const uint64_t (&b)[PPL], int lane, int wave)
{
    constexpr int P = PPL * kWave, THREADS = WAVES * kWave;
    for (int t = threadIdx.x; t < 256; t += THREADS) s.hll_row[t] = 0u;
    for (int t = threadIdx.x; t < P; t += THREADS) s.mh_row[t] = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t acc[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) acc[q] = 0xFFFFFFFFu;
    // slice = the same walk over nb + lo with the degree counted from lo (slot deg - lo is the implicit self loop)
    if (DO_HLL) first_hop_walk<PPL, false, true>(nb + lo, deg - lo, hi - lo, i, wave, WAVES, p, a, b, acc, s.hll_row, lane);
    if (DO_MH) {
        // the two-phase walk (ss_walks.hpp: 4-5 instead of 10 VALU per neighbour and permutation) over this wavefront's batches; a
        // wavefront whose share is ambiguous (duplicated minimum, key collision) redoes its share exactly
        first_hop_minhash_row<PPL>(nb + lo, deg - lo, hi - lo, i, p, a, b, acc, lane, false, wave, WAVES);
#pragma unroll
        for (int q = 0; q < PPL; ++q) atomicMin(&s.mh_row[lane + kWave * q], acc[q]);
    }
    __syncthreads();
}

// wave 0 stores the finished row that the walk left in `s` (+ its cardinality): lane l takes MinHash values l, l + 64, .. and HLL
// registers 4l .. 4l+3.  zero_mh: the MinHash row is stored as zeros (a row without in-edge and self loop -- no build hub row is
// one, they have in-edges by definition; the update passes total == 0).  MIR: the row also goes to the peers' tables.
template <int PPL, bool DO_MH, bool DO_HLL, bool MIR>
__device__ __forceinline__ void first_hop_hub_finish(const FirstHopHubLds<PPL> &s, int64_t i, bool zero_mh, uint32_t *__restrict__ mh_out,
                                                     uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride,
                                                     const EstimatorTables &est, bool want_cards, int lane, const Mirrors &mir)
{
    constexpr int P = PPL * kWave;
    uint32_t mh[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) mh[q] = DO_MH && !zero_mh ? s.mh_row[lane + kWave * q] : 0u;
    const uint32_t regs = DO_HLL ? pack_hll_quad(s.hll_row, lane) : 0u;
    if (DO_MH) {
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            mh_out[i * P + lane + kWave * q] = mh[q];
            if constexpr (MIR) mirror_mh1(mir, i * P + lane + kWave * q, mh[q]);
        }
    }
    if (DO_HLL) {
        *reinterpret_cast<uint32_t *>(hll_out + i * 256 + 4 * lane) = regs;
        if constexpr (MIR) mirror_hll4(mir, i * 256 + 4 * lane, regs);
    }
    if (DO_HLL && want_cards) {
        int nonzero = 0;
        float hsum = 0.0f;
        hll_dword_stats(regs, nonzero, hsum);
        wave_sum_stats(nonzero, hsum);
        if (lane == 0) {
            const float card = hll_estimate(est, 256 - nonzero, hsum);
            cards_out[i * cards_stride] = card;
            if constexpr (MIR) mirror_card(mir, i * cards_stride, card);
        }
    }
}

template <int PPL, int WAVES, bool DO_MH, bool DO_HLL>
__device__ __forceinline__ void first_hop_hub_units(const GraphArgs &g, int worker, int n_workers, const uint64_t *__restrict__ pa,
                                                    const uint64_t *__restrict__ pb, uint32_t *__restrict__ mh_out, int p,
                                                    uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride,
                                                    const EstimatorTables &est, bool want_cards_in, FirstHopHubLds<PPL> &s)
{
    constexpr int P = PPL * kWave, THREADS = WAVES * kWave;
    constexpr int kTicket = DO_MH ? 3 : 4;
    const HubCounts n = hub_counts(g);
    if (worker >= n.hubs + n.slices) return;
    const bool want_cards = DO_HLL && want_cards_in;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    uint64_t a[PPL], b[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        a[q] = DO_MH ? pa[lane + kWave * q] : 0ULL;
        b[q] = DO_MH ? pb[lane + kWave * q] : 0ULL;
    }
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;

    auto walk = [&](int64_t i, const int32_t *nb, int deg, int lo, int hi) {
        first_hop_hub_walk<PPL, WAVES, DO_MH, DO_HLL>(s, i, nb, deg, lo, hi, p, a, b, lane, wave);
    };
    auto finish = [&](int64_t i) {  // (no hub row is empty)
        first_hop_hub_finish<PPL, DO_MH, DO_HLL, true>(s, i, false, mh_out, hll_out, cards_out, cards_stride, est, want_cards, lane, g.mir);
    };

    for (int h = worker; h < n.hubs; h += n_workers) {
        const int64_t i = g.hub_rows[h];
        if (!g.owns(i)) continue;  // workgroup-uniform
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        walk(i, g.col + rb, deg, 0, total);
        if (wave == 0) finish(i);
        __syncthreads();
    }

    // ---- mega rows (see table_hub_units); scratch layout per slice: MinHash u32[P] (P <= 256: the first 1024 B) then the packed
    // HLL row at kMegaHllOffset
    for (int gs = (int)((unsigned)(worker + n_workers - n.hubs % n_workers) % (unsigned)n_workers); gs < n.slices; gs += n_workers) {
        const int m = mega_row_of_slice<THREADS>(g, gs, n.mega, s.s_m);
        int32_t *desc = g.mega_rows + (int64_t)kMegaDesc * m;
        const int4 e = *reinterpret_cast<const int4 *>(desc);
        const int64_t i = e.x;
        if (!g.owns(i)) { __syncthreads(); continue; }  // workgroup-uniform
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        const int sl = gs - e.y;
        const int lo = sl * SS_MEGA_SLICE < total ? sl * SS_MEGA_SLICE : total;
        const int hi = lo + SS_MEGA_SLICE < total ? lo + SS_MEGA_SLICE : total;
        walk(i, g.col + rb, deg, lo, hi);
        uint8_t *mine = g.mega_scratch + (int64_t)(e.y + sl) * kMegaSlot;
        if (wave == 0) {
            if (DO_MH) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) coherent_store(reinterpret_cast<uint32_t *>(mine) + lane + kWave * q, s.mh_row[lane + kWave * q]);
            }
            if (DO_HLL) coherent_store(reinterpret_cast<uint32_t *>(mine + kMegaHllOffset) + lane, pack_hll_quad(s.hll_row, lane));
        }
        publish_drain();  // every wave: the slot stores are acknowledged before the barrier that precedes the ticket
        __syncthreads();
        if (threadIdx.x == 0) {
            const int prev = take_ticket(desc + kTicket);
            s.s_last = prev == e.z - 1;
            if (s.s_last) reset_ticket(desc + kTicket);
        }
        __syncthreads();
        if (s.s_last) {  // workgroup-uniform.  All waves read the slots (wave w: slots w, w + WAVES, ...), combined through the
                         // LDS rows of the walk (which the barrier above has released), wave 0 stores
            uint32_t mh[PPL], regs = 0u;
#pragma unroll
            for (int q = 0; q < PPL; ++q) mh[q] = 0xFFFFFFFFu;
            for (int s2 = wave; s2 < e.z; s2 += 2 * WAVES) {
                const int s3 = s2 + WAVES < e.z ? s2 + WAVES : s2;  // two slots requested together (past the end: s2 again)
                const uint8_t *part0 = g.mega_scratch + (int64_t)(e.y + s2) * kMegaSlot;
                const uint8_t *part1 = g.mega_scratch + (int64_t)(e.y + s3) * kMegaSlot;
                uint32_t v0[PPL], v1[PPL], h0 = 0u, h1 = 0u;
                if (DO_MH) {
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        v0[q] = coherent_load(reinterpret_cast<const uint32_t *>(part0) + lane + kWave * q);
                        v1[q] = coherent_load(reinterpret_cast<const uint32_t *>(part1) + lane + kWave * q);
                    }
                }
                if (DO_HLL) {
                    h0 = coherent_load(reinterpret_cast<const uint32_t *>(part0 + kMegaHllOffset) + lane);
                    h1 = coherent_load(reinterpret_cast<const uint32_t *>(part1 + kMegaHllOffset) + lane);
                }
                if (DO_MH) {
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        const uint32_t v = v0[q] < v1[q] ? v0[q] : v1[q];
                        mh[q] = v < mh[q] ? v : mh[q];
                    }
                }
                if (DO_HLL) {
                    const uint32_t v = bytemax4(h0, h1);
                    regs = bytemax4(regs, v);
                }
            }
            for (int t = threadIdx.x; t < 256; t += THREADS) s.hll_row[t] = 0u;
            for (int t = threadIdx.x; t < P; t += THREADS) s.mh_row[t] = 0xFFFFFFFFu;
            __syncthreads();
            if (DO_MH) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) atomicMin(&s.mh_row[lane + kWave * q], mh[q]);
            }
            if (DO_HLL) {
#pragma unroll
                for (int k = 0; k < 4; ++k) atomicMax(&s.hll_row[4 * lane + k], (regs >> (8 * k)) & 0xFFu);
            }
            __syncthreads();
            if (wave == 0) finish(i);
        }
        __syncthreads();
    }
}

}  // namespace ss
