// ss_fused_hop.hip -- the MinHash first hop and the HLL table hop of hop 2 in ONE launch, interleaved inside every wavefront.
//
// Why: of the kernels of a build the MinHash first hop (hop 1 recomputed from node ids, ss_first_hop.hip) is bound by VALU issue
// (VALUBusy 88 %) and the HLL table hop (ss_propagate.hip) by memory (VALUBusy 47 %); they use different pipes but as separate
// kernels they cannot overlap -- on two streams they share the wave slots and each runs at half rate (both are latency-bound by
// occupancy; tools/probe_overlap.py: 385 us against 392 us back to back).  Inside one wavefront they can: the wave POSTS the HLL
// row loads of four of its rows, walks the MinHash first hop of those rows while the loads travel, and only then folds the HLL
// rows -- the memory pipe works under the VALU pipe.
//
// Data dependencies make this the only such pair of a build: hop-2 HLL rows need the COMPLETE hop-1 HLL table (so the HLL first
// hop and its hub pass run before this launch); hop-1 MinHash rows need nothing but the graph.  A build of h >= 2 hops is
//     ss_fused_hop_stage [this file]  ->  ss_propagate for hops 3..h
// where ss_fused_hop_stage = HLL first hop of the regular rows, ONE hub pass for both hop-1 sketches, this kernel, the MinHash
// table hop of hop 2 (propagate_kernel<128,256>) and ONE hub pass for both hop-2 sketches -- as many hub launches as the unfused
// schedule.  (With cards1_out == NULL the hop-1 HLL table is an input -- the deferred first hop of the ELPH call sequence, hashing.py
// DEFER_FIRST_HOP -- and the hop-1 MinHash hub rows get a pass of their own after the kernel.)
// Results are bit-identical to the unfused sequence: the MinHash side is MinhashRows (ss_walks.hpp, shared with
// first_hop_rows_kernel), the HLL side folds the same rows with the same byte-wise max and runs the same cardinality epilogue.
//
// Mapping: a wavefront owns kFusedRows = 4 consecutive destination rows.  MinHash side: as first_hop_rows_kernel (with 4 rows the
// 60 col entries of a batch almost always cover the whole chunk: a batch reload in the middle of the walk would have to wait for
// its ids with vmcnt(0) -- vmcnt retires in order -- and so for every HLL row posted before it).  HLL side: one 16-lane DPP row
// per destination (lane c = 16-byte chunk c of the 256-byte row); the first kHllInFlight = 7 neighbour chunks per lane are
// requested into registers up front and the next kHllLds = 7 into LDS (LDS-DMA loads; both through a buffer descriptor of the table where
// it fits one, HllSource below; ids by one coalesced load per
// lane group, handed out by DPP row_newbcast), the rest of rows longer than 14 after the MinHash walk (hll_row16_finish).  Hub rows are skipped by both sides:
// they are hub units (ss_hub.hpp) hosted by the launches before and after this one -- not by this one: the kernel sits exactly at its
// 96-VGPR budget, and a hub branch, whatever it contained, cost the row path 64 bytes of scratch and 30 us (round 4).
// P = 64 * PPL, M = 256 (p = 8) only -- the shapes ss_first_hop has a kernel for.
#include <cstring>
#include <type_traits>

#include "ss_hub.hpp"

namespace ss {

constexpr int kFusedRows = 4;
constexpr int kHllInFlight = 7;  // neighbour chunks per lane requested into registers up front

struct HllPosted {  // one lane group's view of its row while the row's first chunks are in flight
    int64_t i;
    const int32_t *nb;
    int deg, total;
    bool write;
    u32x4 x[kHllInFlight];
};

// How the posts address the hop-1 HLL table.  The ids a lane group hands out by DPP (Ids::my_nb, load_ids below) already say what to
// fetch: lane t < total of the group holds the id of the row's neighbour t -- its own row for the implicit self loop -- and every
// other lane the id N, the row after the table's last.
// BUF: through a raw buffer descriptor over the table's N * 256 bytes (table_rsrc, ss_common.hpp).  A post is the DPP broadcast, one
// shift-or for the 32-bit offset and a buffer_load_dwordx4; the row N lies beyond the records and the range check answers it with
// zeros: no compare, no select, no zeroed landing, no exec-mask frame around the load, no 64-bit id or address.
// !BUF: flat 64-bit addresses under a branch on t < total, for tables the descriptor cannot hold (buffer_describable, asked by ss_fused_hop_stage).
struct HllSource {
    const uint8_t *base;
    __amdgpu_buffer_rsrc_t rsrc;
};

template <bool BUF>
__device__ __forceinline__ HllSource hll_source(const uint8_t *__restrict__ hll_in, int64_t N)
{
    HllSource s;
    s.base = hll_in;
    if constexpr (BUF) s.rsrc = table_rsrc(hll_in, (uint32_t)(N * 256));  // (the host has checked that it fits)
    return s;
}

// lane T of the caller's 16-lane row, by DPP row_newbcast.  (No old value: every lane is written, and a zero handed in as one costs a
// v_mov per broadcast)
template <int T>
__device__ __forceinline__ int row_bcast(int v)
{
    return __builtin_amdgcn_mov_dpp(v, 0x150 + T, 0xF, 0xF, true);
}

// requests chunk c (c16 = 16 * c) of the first min(total, kHllInFlight) neighbour rows
template <bool BUF, int T0>
__device__ __forceinline__ void hll_post(HllPosted &h, const HllSource &src, int my_nb, uint32_t c16)
{
    if constexpr (T0 < kHllInFlight) {
        const int nbt = row_bcast<T0>(my_nb);
        if constexpr (BUF) {
            h.x[T0] = buffer_load16(src.rsrc, ((uint32_t)nbt << 8) | c16);  // (node ids are < 2^31, and < 2^24 for a describable table)
        } else {
            h.x[T0] = u32x4{0u, 0u, 0u, 0u};
            if (T0 < h.total) h.x[T0] = *reinterpret_cast<const u32x4 *>(src.base + (int64_t)nbt * 256 + c16);
        }
        hll_post<BUF, T0 + 1>(h, src, my_nb, c16);
    }
}

// neighbour rows kHllInFlight .. kHllInFlight + kHllLds - 1 of every lane group travel into LDS instead of registers
// (global_load_lds_dwordx4 / buffer_load_dwordx4 ... lds: no VGPR destination; one instruction = one neighbour of each of the
// wavefront's four rows, landing as 64 lanes x 16 B = 1 KiB at the wave-uniform LDS address): rows of up to 16 neighbours need no load
// after the MinHash walk.  A slot that none of the wavefront's four rows reaches is not posted (one compare and a scalar branch), nor
// any slot after it; the fold leaves the same slots out.  What an out-of-range lane of the buffer form leaves in its 16 bytes of the
// slot is not relied on: the fold masks the slots beyond a row's total in both forms.
constexpr int kHllLds = 7;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(1))) const uint32_t global_u32;
typedef __attribute__((address_space(1))) const int64_t global_i64;

template <bool BUF, int T>
__device__ __forceinline__ void hll_post_lds(const HllPosted &h, const HllSource &src, int my_nb, uint32_t c16, uint32_t lds_wave)
{
    if constexpr (T < kHllInFlight + kHllLds) {
        if (!__any(T < h.total)) return;  // wave-uniform
        const int nbt = row_bcast<T>(my_nb);
        lds_u32 *const slot = (lds_u32 *)(uintptr_t)(lds_wave + 1024u * (T - kHllInFlight));
        if constexpr (BUF) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src.rsrc, slot, 16, (int)(((uint32_t)nbt << 8) | c16), 0, 0, 0);
        } else {
            if (T < h.total) __builtin_amdgcn_global_load_lds((global_u32 *)(uintptr_t)(src.base + (int64_t)nbt * 256 + c16), slot, 16, 0, 0);
        }
        hll_post_lds<BUF, T + 1>(h, src, my_nb, c16, lds_wave);
    }
}

__device__ __forceinline__ void hll_fold(const HllPosted &h, u32x4 &ae, u32x4 &ao)
{
#pragma unroll
    for (int k = 0; k < kHllInFlight; ++k) hll_acc(ae, ao, h.x[k]);
}

// ---- the kernel: persistent, software-pipelined -------------------------------------------------------------------------------
// Four or five wavefronts per SIMD are too few to hide the three dependent round trips at the head of a chunk (row
// bounds -> neighbour ids -> HLL rows): a one-chunk-per-wavefront form of this kernel gained 6 % over the two separate launches
// (174 us against 184).  Here a wavefront keeps walking chunks (chunk = kFusedRows rows; chunk q, q + waves, ...) and the loads of the NEXT chunks are posted
// before the MinHash walk of the current one:
//     ids(k) arrive  ->  post HLL rows(k)  ->  post ids(k+1) [bounds(k+1) arrived an iteration ago]  ->  post bounds(k+2)
//     ->  MinHash walk(k)  [VALU; everything above travels]  ->  fold HLL rows(k), finish, store
// vmcnt retires in order and that is exactly the order of use, so no wait ever covers a younger load.
// Measured (bench graph): two separate launches 82 + 102 = 184 us; one chunk per wavefront 174 us; this kernel 166-170 us with 12
// chunks in registers and nothing in LDS (step 0.494 -> 0.478 ms), 151 us as it stands.  The VALU work alone would be
// ~100-120 us: what is left are the loads of rows with more than 16 neighbours, issued and awaited after the walk.  Register-only
// attempts at more coverage: a rolling window (fold four posted chunks after every MinHash row and re-post their registers with the
// row's next four neighbours) covered 24 neighbours but cost 157-167 VGPRs (three wavefronts per SIMD): 181-196 us; a single re-post of
// 8 chunks before the last MinHash row (coverage 16, 134 VGPRs): 184 us.  Not shipped: the kernel lives on its occupancy.
// Round 3: 11 register + 5 LDS landings at ~125 VGPRs (four wavefronts per SIMD) was 151-152 us; held to 96 VGPRs by
// amdgpu_waves_per_eu (no scratch) with 7 + 7 landings and a 3 KB estimator image (31 KB of LDS: five workgroups per CU) it is
// 146 us -- and 1 946 -> 1 730 / 3 650 -> 3 410 us at ppa / citation2 size, where the table hop's gathers come from HBM and a fifth
// wavefront hides more of them.  (6 + 7, 7 + 6: the same within noise; 4 + 6: 154-158 us -- coverage still matters; six wavefronts spill.)
// A second use of the register landings -- folded before the LAST MinHash row and sent out again for neighbours 14 .. 20 (ids from a
// second id word per lane), coverage 21 -- needs the accumulators alive through that row's walk: 96 / 64 / 32 bytes of scratch with
// 7 / 6 / 5 register landings and 197 / 177 / 154 us; with 4 (no scratch, coverage 15) 146 us, the same as without.  Not shipped.
template <int PPL, bool BUF>
__device__ __forceinline__ void fused_hop_body(const GraphArgs &g, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb,
                                               uint32_t *__restrict__ mh_out, int p, const uint8_t *__restrict__ hll_in,
                                               uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride,
                                               const ss_hll_params &prm, bool skip_hubs)
{
    constexpr int R = kFusedRows, kNb = kWave - R;
    // 3 KB of estimator tables (the kernel is p = 8 only: 257 linear-counting entries; raw / bias up to 256 entries, longer tables stay
    // in global memory) + 7 KB of landings per wavefront = 31 KB: five workgroups per CU
    __shared__ CompactEstimatorLds<257, 256> lds;
    __shared__ __attribute__((aligned(16))) uint8_t landing[256 / kWave][kHllLds > 0 ? kHllLds : 1][1024];
    const bool want_cards = cards_out != nullptr;
    EstimatorTables est = {};
    if (want_cards) est = stage_tables_compact(lds, prm);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const uint32_t lds_wave = (uint32_t)(uintptr_t)&landing[wave][0][0];  // LDS byte address (low half of the generic pointer)
    const int64_t n_chunks = (g.rows() + R - 1) / R;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x / kWave);
    int64_t chunk = (int64_t)blockIdx.x * (blockDim.x / kWave) + wave;
    if (chunk >= n_chunks) return;
    MinhashRows<PPL, R> m;
    m.setup(g, pa, pb, p, skip_hubs);
    const int lane = m.lane, grp = lane >> 4, c = lane & (kRow - 1);
    const uint32_t c16 = 16u * (uint32_t)c;
    const HllSource src = hll_source<BUF>(hll_in, g.N);
    const bool skip_self = g.skip_self && *g.skip_self != 0;  // HLL side only (one scalar load per wavefront); the first hop keeps its self loop

    auto chunk_rows = [&](int64_t q) -> int { return q < n_chunks ? (int)(g.row1 - (g.row0 + q * R) < R ? g.row1 - (g.row0 + q * R) : R) : 0; };
    auto load_bounds = [&](int64_t q) -> int64_t {  // lane l: rowptr[first row of chunk q + l]
        const int nr = chunk_rows(q);
        // a scalar base and a 32-bit lane offset.  (The empty asm hides the base from hipcc, which otherwise splits the address into a
        // per-lane 64-bit rowptr + 8 * lane, kept in two VGPRs for the whole kernel, and a scalar rest: the two registers this
        // kernel does not have)
        const int64_t *first_bound = g.rowptr + (g.row0 + q * R);
        asm volatile("" : "+s"(first_bound));
        return (nr > 0 && lane <= nr) ? ((global_i64 *)first_bound)[(uint32_t)lane] : 0;  // (global, not flat: a flat load counts in lgkmcnt too)
    };
    // the row of this lane group in a chunk of `nr` rows from row `first` whose bounds have arrived (rel: lane l holds the chunk-relative
    // rowptr[first + l]); total = 0: no row to write (past the end, or a hub row left to the hub pass)
    struct GroupRow { int64_t i; int rel0, deg, total; bool write; };
    auto group_row = [&](int64_t first, int nr, int rel) -> GroupRow {
        GroupRow w;
        const bool ok = grp < nr;
        w.rel0 = __shfl(rel, ok ? grp : 0);
        w.deg = ok ? __shfl(rel, ok ? grp + 1 : 0) - w.rel0 : 0;
        w.i = first + (ok ? grp : 0);
        w.write = ok && !(skip_hubs && w.deg > g.hub_threshold);
        w.total = w.write ? table_hop_total(w.deg, w.i < m.n_self, skip_self) : 0;
        return w;
    };
    // what a lane fetches for a chunk whose bounds have arrived: its batch id (MinHash side) and its lane group's neighbour id (HLL side:
    // lane c < total the id of neighbour c, the row itself as neighbour `deg`; the other lanes N, the row after the table's last)
    // (nid stays 32 bits wide until it is used: widening it here would be a use of the load's result, and hipcc would wait
    // -- vmcnt(0): for every HLL row posted just before -- right behind the load instead of after the MinHash walk)
    struct Ids { int nid; int my_nb; };
    auto load_ids = [&](int64_t q, int64_t rp) -> Ids {
        const int nr = chunk_rows(q);
        if (nr == 0) return Ids{0, 0};
        const int64_t first = g.row0 + q * R;
        const int64_t c_lo = ((int64_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)rp >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)rp);
        const int rel = (int)(rp - c_lo);
        const int c_n = __builtin_amdgcn_readlane(rel, nr);
        const int32_t *nb = g.col + c_lo;
        Ids out;
        out.nid = lane >= kNb ? (int)(first + (lane - kNb)) : 0;  // node ids are < 2^31 (checked by the entry point)
        if (lane < kNb && lane < c_n) out.nid = nb[lane];
        const GroupRow w = group_row(first, nr, rel);
        out.my_nb = c < w.total ? (int)w.i : (int)g.N;
        if (c < (w.total < w.deg ? w.total : w.deg)) out.my_nb = nb[w.rel0 + c];
        return out;
    };

    // prologue: bounds of the first two chunks, ids of the first
    int64_t rp_cur = load_bounds(chunk);
    int64_t rp_next = load_bounds(chunk + stride);
    Ids ids_cur = load_ids(chunk, rp_cur);

    for (; chunk < n_chunks; chunk += stride) {  // wave-uniform
        const int64_t first = g.row0 + chunk * R;
        m.begin(g, first, chunk_rows(chunk), rp_cur);
        m.set_batch((int64_t)ids_cur.nid);
        // HLL side of this chunk: the row of this lane group
        HllPosted h;
        const GroupRow w = group_row(m.i0, m.rows, m.rel);
        h.i = w.i;
        h.nb = m.nb + w.rel0;
        h.deg = w.deg;
        h.write = w.write;
        h.total = w.total;
        hll_post<BUF, 0>(h, src, ids_cur.my_nb, c16);          // HLL rows of chunk k
        // (the slots' addresses go to m0; hidden from hipcc here, they are one s_add each -- known to be loop constants, the seven of
        // them are kept in spilled SGPRs and cost a v_readlane per post)
        uint32_t lds_slots = lds_wave;
        asm volatile("" : "+s"(lds_slots));
        hll_post_lds<BUF, kHllInFlight>(h, src, ids_cur.my_nb, c16, lds_slots);
        const Ids ids_next = load_ids(chunk + stride, rp_next); // ids of chunk k + 1 (its bounds arrived during the last walk)
        const int64_t rp_after = load_bounds(chunk + 2 * stride);  // bounds of chunk k + 2
#pragma unroll 1
        for (int r = 0; r < m.rows; ++r) m.row(r, mh_out);       // MinHash first hop of chunk k: VALU work under all of the above
        u32x4 ae = {0u, 0u, 0u, 0u}, ao = {0u, 0u, 0u, 0u};
        hll_fold(h, ae, ao);
        if constexpr (kHllLds > 0) {
            // (hll_fold waited for h.x; the LDS landings were issued after them and vmcnt retires in order -- but hipcc does not
            // count a global_load_lds against the ds_read below, so the wait is spelled out; everything posted before the walk
            // is long back by now)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < kHllLds; ++k) {
                if (!__any(kHllInFlight + k < h.total)) break;  // wave-uniform: not posted either
                u32x4 v = *reinterpret_cast<const u32x4 *>(&landing[wave][k][16 * lane]);
                if (!(kHllInFlight + k < h.total)) v = u32x4{0u, 0u, 0u, 0u};  // slot not written this round (stale bytes)
                hll_acc(ae, ao, v);
            }
        }
        const u32x4 acc = hll_acc_result(ae, ao);
        // (the fused stage is the unsharded build's: no peers)
        if constexpr (BUF) {
            hll_row16_finish_by<false>(h.i, h.write, h.nb, h.deg, h.total, acc, kHllInFlight + kHllLds,
                                       [&](const int32_t *nb, int deg, int total, int64_t self_row, int first, int stride) {
                                           return hll_walk_buffer(src.rsrc, (uint32_t)(g.N * 256), reinterpret_cast<const int32_t *>(hll_in), nb, deg,
                                                                  total, self_row, first, stride, c16);
                                       },
                                       hll_out, cards_out, cards_stride, est, want_cards, c, Mirrors{});
        } else {
            hll_row16_finish<false>(h.i, h.write, h.nb, h.deg, h.total, acc, kHllInFlight + kHllLds, hll_in, hll_out, cards_out, cards_stride, est, want_cards, c, Mirrors{});
        }
        rp_cur = rp_next;
        rp_next = rp_after;
        ids_cur = ids_next;
    }
}

// P = 64 / 128: the register allocator is held to 96 VGPRs (amdgpu_waves_per_eu: at least FIVE wavefronts per SIMD; it gets there
// without scratch -- left alone it spreads to ~125 and four wavefronts).  P = 192 / 256 would spill at 96: they are held to the 128
// VGPRs of FOUR wavefronts, which they had without being asked until the row body changed shape (left alone: 139 and three; held:
// 104 / 124, no scratch).
template <int PPL, bool BUF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PPL <= 2 ? 5 : 4))) void fused_hop_persistent_kernel(
    GraphArgs g, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb, uint32_t *__restrict__ mh_out, int p,
    const uint8_t *__restrict__ hll_in, uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm,
    bool skip_hubs)
{
    fused_hop_body<PPL, BUF>(g, pa, pb, mh_out, p, hll_in, hll_out, cards_out, cards_stride, prm, skip_hubs);
}

}  // namespace ss

extern "C" int ss_fused_hop_stage(const ss_csr_graph *graph, const uint64_t *a, const uint64_t *b, int32_t P, uint32_t *mh1_out,
                                  uint32_t *mh2_out, int32_t p, uint8_t *hll1, float *cards1_out, uint8_t *hll2_out, float *cards2_out,
                                  int64_t cards_stride, const ss_hll_params *prm, void *stream)
{
    const uint8_t *hll1_in = hll1;
    using namespace ss;
    if (!graph || graph->num_nodes < 0 || !graph->rowptr) return SS_ERR_INVALID_ARG;
    if (p != 8 || P <= 0 || P % kWave || P > 256) return SS_ERR_UNSUPPORTED;  // caller uses ss_first_hop + ss_propagate
    if (mh2_out && P != 128) return SS_ERR_UNSUPPORTED;                        // the hub pass of the table hop is P = 128 only
    const int64_t N = graph->num_nodes;
    if (N == 0) return SS_OK;
    if (!mh1_out || !a || !b || !hll1_in || !hll2_out || N >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    if ((graph->hub_rows == nullptr) != (graph->hub_count == nullptr)) return SS_ERR_INVALID_ARG;
    ss_hll_params p0 = {};
    if (cards2_out) {
        const int rc = check_params(prm);
        if (rc != SS_OK) return rc;
        if (prm->p != p) return SS_ERR_INVALID_ARG;
        p0 = *prm;
    }
    if (!row_range_ok(*graph)) return SS_ERR_INVALID_ARG;
    GraphArgs g = to_args(*graph);
    if (g.rows() == 0) return SS_OK;
    // both table hops of this stage read hop-1 tables of `graph`: the MinHash one this stage computes from node ids, the HLL one it
    // computes too unless it is the caller's (cards1_out == NULL) -- the promise of SS_GRAPH_HOP_TABLES, made here for the whole-graph,
    // single-device build (a row range or mirrors: the sharded builds, left alone)
    const bool whole = graph->row_begin == 0 && graph->row_end == 0 && g.mir.n == 0;
    const int32_t *const skip_word = self_skip_word(*graph, whole);
    g.skip_self = nullptr;
    hipStream_t s = (hipStream_t)stream;
    const bool hubs = g.hub_rows && g.hub_count;
    // hub units: `lead` leading workgroups of the HLL first-hop launch serve both hop-1 tables, of the MinHash table hop both hop-2
    // tables (0: launches of their own, as in rounds 1-3)
    const int lead = hub_lead_blocks(hubs);
    const bool own_hop1 = cards1_out != nullptr;  // the hop-1 HLL table is computed here as well (build_hash_tables)
    if (own_hop1) {
        if (!cards2_out) return SS_ERR_INVALID_ARG;
        int rc1 = launch_hll_first_hop_rows(g, p, hll1, cards1_out, cards_stride, p0, hubs, lead, a, b, lead > 0 ? mh1_out : nullptr, P, s);
        if (rc1 != SS_OK) return rc1;
        // ONE hub pass from node ids for both hop-1 sketches: the MinHash hub rows are not needed before the table hop below,
        // but computing them here saves the hub launch after the fused kernel
        if (lead == 0) rc1 = launch_first_hop_hub_only(g, a, b, P, mh1_out, p, hll1, cards1_out, cards_stride, p0, s);
        if (rc1 != SS_OK) return rc1;
    }
    constexpr int rows_per_block = 4 * kFusedRows;
    const unsigned blocks = (unsigned)((g.rows() + rows_per_block - 1) / rows_per_block);
    // 5 workgroups are resident per CU; several times that many balance the tail.  Bench graph (58 blocks per CU): 12 / 15 / 20 / 25 / 30 /
    // 40 per CU: 148.7 / 147.8 / 146.2-146.9 / 149.9 / 149.2 / 151.2 us.  ppa / citation2 size (140 / 715 blocks per CU): 15 / 20 / 30 /
    // 48 / 64 / 100 / 200 / all: 1 832 / 1 819 / 1 774 / 1 724 / 1 738 / 1 728 / 1 751 / 1 748 us and 3 540 / 3 499 / 3 448 / 3 418 / 3 408 /
    // 3 419 / 3 457 / 3 814 us
    const int wg_per_cu = blocks > 256u * 128u ? 64 : 20;
    const unsigned grid = blocks < (unsigned)(256 * wg_per_cu) ? blocks : (unsigned)(256 * wg_per_cu);
    g.skip_self = own_hop1 ? skip_word : nullptr;
    // how the kernel posts its hop-1 HLL rows: through a buffer descriptor when the table and the row after it fit the descriptor's
    // 32-bit byte count, with flat addresses otherwise.  SS_FUSED_POSTS=flat, read at every launch, forces the flat form at any size
    // (test hook; any other value, `buffer` included, leaves the choice to the size: a larger table cannot be described)
    const char *posts_env = getenv("SS_FUSED_POSTS");
    const bool buf_posts = buffer_describable(N * 256, 2 * 256) && !(posts_env && !strcmp(posts_env, "flat"));  // (lanes with nothing to fetch ask for row N)
    {
        ProfileSpan span(s, SS_PROF_FUSED, true);
        auto launch = [&](auto buf) {
            constexpr bool B = decltype(buf)::value;
            switch (P / kWave) {
                case 1: span.launch(fused_hop_persistent_kernel<1, B>, dim3(grid), dim3(256), g, a, b, mh1_out, p, hll1_in, hll2_out, cards2_out, cards_stride, p0, hubs); break;
                case 2: span.launch(fused_hop_persistent_kernel<2, B>, dim3(grid), dim3(256), g, a, b, mh1_out, p, hll1_in, hll2_out, cards2_out, cards_stride, p0, hubs); break;
                case 3: span.launch(fused_hop_persistent_kernel<3, B>, dim3(grid), dim3(256), g, a, b, mh1_out, p, hll1_in, hll2_out, cards2_out, cards_stride, p0, hubs); break;
                default: span.launch(fused_hop_persistent_kernel<4, B>, dim3(grid), dim3(256), g, a, b, mh1_out, p, hll1_in, hll2_out, cards2_out, cards_stride, p0, hubs); break;
            }
        };
        if (buf_posts) launch(std::true_type{});
        else launch(std::false_type{});
    }
    SS_LAUNCH_CHECK();
    g.skip_self = skip_word;  // (the MinHash table hop below; the hub launches do not look at it)
    // hub rows of the hop-1 MinHash table (from node ids): they must be in place before anything reads that table
    int rc = own_hop1 ? SS_OK : launch_first_hop_hub_only(g, a, b, P, mh1_out, p, nullptr, nullptr, 0, p0, s);
    if (rc != SS_OK) return rc;
    if (!mh2_out)  // hop-2 HLL hub rows alone
        return launch_propagate_hub_only(g, nullptr, nullptr, hll1_in, hll2_out, cards2_out, cards_stride, p0, s);
    // MinHash table hop of hop 2; its launch hosts the hub units of both hop-2 tables (or ONE hub pass for both follows)
    if (lead > 0) return launch_minhash_hop(g, mh1_out, mh2_out, hubs, lead, hll1_in, hll2_out, cards2_out, cards_stride, p0, s);
    rc = launch_minhash_hop(g, mh1_out, mh2_out, hubs, 0, nullptr, nullptr, nullptr, 0, p0, s);
    if (rc != SS_OK) return rc;
    return launch_propagate_hub_only(g, mh1_out, mh2_out, hll1_in, hll2_out, cards2_out, cards_stride, p0, s);
}
