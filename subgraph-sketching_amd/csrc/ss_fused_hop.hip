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
//
// The RECORDS form of the HLL side (third template flag, with buffer posts only; "the records form" below): on sparse graphs without
// hub rows the stage's HLL first hop also leaves a 64-byte code record per node, the posts fetch one dword of it per lane and slot, and
// the fold is a scatter-max of (register, rank) codes into a 1 KB row image per lane group in LDS -- on the LDS pipe, which is idle
// here, instead of the byte-wise max of mostly empty 256-byte rows on the VALU pipe, which is what the kernel waits for.  Same rows
// bit for bit: a record that cannot hold its node's neighbourhood says so and that slot is folded from the dense row.  Which form a
// launch takes is decided in ss_fused_hop_stage_records; the dense instantiations are the object code they were.
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
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
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

// ---- the records form of the HLL side (REC) ---------------------------------------------------------------------------------------
// A hop-1 HLL row of node j has at most deg(j) + 1 non-zero registers of 256, and the dense fold spends VALU issue slots -- the one
// thing this kernel is short of -- on the max of zeros.  In the records form the fold moves to the LDS pipe: the HLL first hop leaves a
// 64-byte CODE RECORD per node (hll_first_hop_row16, ss_walks.hpp: up to 32 codes register << 2 | rank << 10, two per dword), a post
// fetches ONE dword per lane -- lane c of a group dword c of neighbour t's record, 64 contiguous bytes per group, one VGPR per slot --
// and after the MinHash rows every lane scatters its two codes into its group's private 1 KB row image with LDS atomic max, exactly as
// hll_first_hop_row16 builds a hop-1 row.  Lane c then packs registers 16c .. 16c + 15 of the image into the 16 bytes the dense fold
// would have produced, and everything after it (rows beyond the posted slots, the statistics, the estimator, the stores) is the dense
// form's code on the dense table.
// Exact by construction: a record holds EVERY neighbour of its node or says so -- a node of more than 32 neighbours, and a hub row
// the first hop left to the hub units, carries kRecordDense in every dword.  Lane 0 of a group sees dword 0 of the slot's record: a
// flagged slot is folded from the node's dense row (byte-wise max into a dense accumulator that joins the packed image), and the flagged
// lanes scatter nothing.
// kRecSlots = 16 slots are posted, the ids a lane group hands out by DPP, two at a time: a pair of slots that none of the wavefront's
// rows reaches is neither posted nor scattered (one scalar compare against the largest of the four totals; the odd slot of a pair
// that is reached by half asks for the row N like every lane with nothing to fetch).
// What a slot costs in VALU issue: the post is ONE instruction (the ids are shifted once per chunk, and v_or_b32 takes the DPP
// broadcast as its operand); whether any record of the chunk is flagged is asked once, of the maximum over the slots (v_max3_u32,
// half an instruction per slot), and the slot-by-slot test runs only then; a dword's first code is a compare (most dwords are empty,
// and their lanes would all meet at register 0), the address and the rank; the second code -- neighbours 16 .. 31 of a node -- is
// looked at only where some lane of the wavefront has one.
constexpr int kRecSlots = kRow;

__device__ __forceinline__ uint32_t buffer_load4(__amdgpu_buffer_rsrc_t rsrc, uint32_t byte_offset)
{
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)byte_offset, 0, 0);
}

__device__ __forceinline__ void lds_max(uint32_t addr, uint32_t v)  // (no return value asked for: ds_max_u32, not ds_max_rtn_u32)
{
    __hip_atomic_fetch_max((lds_u32 *)(uintptr_t)addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// my_nb64 = 64 * the id the lane hands out (Ids::my_nb), c4 = 4 * (lane & 15): lane c fetches dword c of the record
template <int T>
__device__ __forceinline__ void rec_post(uint32_t (&x)[kRecSlots], __amdgpu_buffer_rsrc_t rec, int my_nb64, uint32_t c4, int reach)
{
    if constexpr (T < kRecSlots) {
        if (T >= reach) return;  // scalar
        x[T] = buffer_load4(rec, (uint32_t)row_bcast<T>(my_nb64) | c4);  // (the id N of a lane with nothing to fetch: zeros)
        x[T + 1] = buffer_load4(rec, (uint32_t)row_bcast<T + 1>(my_nb64) | c4);
        rec_post<T + 2>(x, rec, my_nb64, c4, reach);
    }
}

// the largest dword among the posted slots: kRecordDense where a record is flagged
template <int T>
__device__ __forceinline__ void rec_max(const uint32_t (&x)[kRecSlots], int reach, uint32_t &mx)
{
    if constexpr (T < kRecSlots) {
        if (T >= reach) return;  // scalar
        mx = max(mx, max(x[T], x[T + 1]));
        rec_max<T + 2>(x, reach, mx);
    }
}

// the two codes of one dword into the image at LDS byte address `img` (1 KB-aligned: the word offset is OR-ed in)
__device__ __forceinline__ void rec_scatter_codes(uint32_t v, uint32_t img)
{
    if (v) lds_max(img | (v & 0x3FCu), (v >> 10) & 63u);
    // a scalar branch, which hipcc would merge into the lanes' condition: under an exec mask alone the three instructions of the
    // second code issue for nobody
    if (__any(v > 0xFFFFu)) {
        asm volatile("");  // (keeps the two conditions apart)
        if (v > 0xFFFFu) lds_max(img | ((v >> 16) & 0x3FCu), v >> 26);
    }
}

// What a lane group needs of its row to fold a flagged slot: nb / deg / self_row, `bytes` = the row after the dense table's last
struct RecRow {
    const int32_t *nb;
    int deg;
    int64_t self_row;
    uint32_t bytes;
};

// slot T of every lane group; img = the group's image, c16 = 16 * (lane & 15).  FLAGS (some record of the chunk is flagged): a slot
// with a flagged record in any group also fetches chunk c of the flagged nodes' dense rows -- `bytes` for the other groups: zeros --
// into the dense accumulator `dacc`, which joins the packed image at the end, and the lanes of a flagged record scatter nothing
template <int T, bool FLAGS>
__device__ __forceinline__ void rec_slot(uint32_t v, uint32_t img, const HllSource &src, const RecRow &w, uint32_t c16, u32x4 &dacc)
{
    if constexpr (FLAGS) {
        // dword 0 of a record sits in lane 0 of its group
        const bool dense = (uint32_t)row_bcast<0>((int)v) == kRecordDense;
        if (__any(dense)) {
            // (a flagged slot is a neighbour of the row: T < total.  Its id comes from the CSR again -- the lanes' ids left their
            // register when the next chunk's arrived)
            uint32_t off = w.bytes;
            if (dense) off = ((T < w.deg ? (uint32_t)w.nb[T] : (uint32_t)w.self_row) << 8) | c16;
            dacc = bytemax16(dacc, buffer_load16(src.rsrc, off));
        }
        if (!dense) rec_scatter_codes(v, img);
    } else {
        rec_scatter_codes(v, img);
    }
}

template <int T, bool FLAGS>
__device__ __forceinline__ void rec_scatter(const uint32_t (&x)[kRecSlots], uint32_t img, int reach, const HllSource &src, const RecRow &w,
                                            uint32_t c16, u32x4 &dacc)
{
    if constexpr (T < kRecSlots) {
        if (T >= reach) return;  // scalar: not posted either
        rec_slot<T, FLAGS>(x[T], img, src, w, c16, dacc);
        rec_slot<T + 1, FLAGS>(x[T + 1], img, src, w, c16, dacc);
        rec_scatter<T + 2, FLAGS>(x, img, reach, src, w, c16, dacc);
    }
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
template <int PPL, bool BUF, bool REC>
__device__ __forceinline__ void fused_hop_body(const GraphArgs &g, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb,
                                               uint32_t *__restrict__ mh_out, int p, const uint8_t *__restrict__ hll_in,
                                               uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride,
                                               const ss_hll_params &prm, bool skip_hubs, const uint32_t *__restrict__ records)
{
    static_assert(BUF || !REC, "the records form posts through buffer descriptors");
    constexpr int R = kFusedRows, kNb = kWave - R;
    // 3 KB of estimator tables (the kernel is p = 8 only: 257 linear-counting entries; raw / bias up to 256 entries, longer tables stay
    // in global memory) + 7 KB of landings per wavefront = 31 KB: five workgroups per CU.  REC: four 1 KB row images per wavefront
    // in place of the landings, 19 KB
    __shared__ CompactEstimatorLds<257, 256> lds;
    __shared__ __attribute__((aligned(REC ? 1024 : 16))) uint8_t landing[256 / kWave][REC ? kWave / kRow : (kHllLds > 0 ? kHllLds : 1)][1024];
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
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rec_rsrc;
    if constexpr (REC) rec_rsrc = table_rsrc(records, (uint32_t)(g.N * 4 * kRow));
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
        [[maybe_unused]] uint32_t rx[kRecSlots];
        [[maybe_unused]] int reach = 0;  // REC: the slots some row of the wavefront reaches, at most kRecSlots
        if constexpr (REC) {
            const int t01 = max(__builtin_amdgcn_readlane(h.total, 0), __builtin_amdgcn_readlane(h.total, kRow));
            const int t23 = max(__builtin_amdgcn_readlane(h.total, 2 * kRow), __builtin_amdgcn_readlane(h.total, 3 * kRow));
            reach = max(t01, t23);
            rec_post<0>(rx, rec_rsrc, ids_cur.my_nb << 6, c16 >> 2, reach);  // code records of chunk k
        } else {
        hll_post<BUF, 0>(h, src, ids_cur.my_nb, c16);          // HLL rows of chunk k
        // (the slots' addresses go to m0; hidden from hipcc here, they are one s_add each -- known to be loop constants, the seven of
        // them are kept in spilled SGPRs and cost a v_readlane per post)
        uint32_t lds_slots = lds_wave;
        asm volatile("" : "+s"(lds_slots));
        hll_post_lds<BUF, kHllInFlight>(h, src, ids_cur.my_nb, c16, lds_slots);
        }
        const Ids ids_next = load_ids(chunk + stride, rp_next); // ids of chunk k + 1 (its bounds arrived during the last walk)
        const int64_t rp_after = load_bounds(chunk + 2 * stride);  // bounds of chunk k + 2
#pragma unroll 1
        for (int r = 0; r < m.rows; ++r) m.row(r, mh_out);       // MinHash first hop of chunk k: VALU work under all of the above
        u32x4 ae = {0u, 0u, 0u, 0u}, ao = {0u, 0u, 0u, 0u};
        [[maybe_unused]] u32x4 packed;
        if constexpr (REC) {
            // the group's row image: zeroed, fed with the codes, packed -- fenced as hll_first_hop_row16 fences its image
            // (its LDS byte address is formed here, chunk by chunk, hidden from hipcc: as loop constants the image's addresses are
            // hoisted out of the chunk loop and live in VGPRs through the MinHash walk -- registers the kernel does not have)
            uint32_t img = lds_wave + 1024u * (uint32_t)grp, z = 0u;
            asm volatile("" : "+v"(img), "+v"(z));  // (the zero too: four registers of zeros otherwise)
            const u32x4 zero = {z, z, z, z};
#pragma unroll
            for (int k = 0; k < 4; ++k) *(lds_u32x4 *)(uintptr_t)(img + c16 + 256u * k) = zero;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t mx = 0u;
            rec_max<0>(rx, reach, mx);
            const bool flags = (__ballot(mx == kRecordDense) & 0x0001000100010001ull) != 0ull;  // wave-uniform, rare
            u32x4 dacc = zero;
            if (flags) rec_scatter<0, true>(rx, img, reach, src, RecRow{h.nb, h.deg, h.i, (uint32_t)(g.N * 256)}, c16, dacc);
            else rec_scatter<0, false>(rx, img, reach, src, RecRow{}, c16, dacc);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t *pw = reinterpret_cast<uint32_t *>(&packed);
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // lane c: registers 16 c .. 16 c + 15, a byte each
                const u32x4 r4 = *(const lds_u32x4 *)(uintptr_t)(img + 4u * c16 + 16u * k);
                pw[k] = r4.x | (r4.y << 8) | (r4.z << 16) | (r4.w << 24);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (flags) packed = bytemax16(packed, dacc);
        } else {
        hll_fold(h, ae, ao);
        }
        if constexpr (kHllLds > 0 && !REC) {
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
        u32x4 acc;
        if constexpr (REC) acc = packed;
        else acc = hll_acc_result(ae, ao);
        // (the fused stage is the unsharded build's: no peers)
        if constexpr (BUF) {
            hll_row16_finish_by<false>(h.i, h.write, h.nb, h.deg, h.total, acc, REC ? kRecSlots : kHllInFlight + kHllLds,
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
// REC (with BUF only): the records form; `records` is the table the HLL first hop of this stage has just written, NULL otherwise.
template <int PPL, bool BUF, bool REC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PPL <= 2 ? 5 : 4))) void fused_hop_persistent_kernel(
    GraphArgs g, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb, uint32_t *__restrict__ mh_out, int p,
    const uint8_t *__restrict__ hll_in, uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm,
    bool skip_hubs, const uint32_t *__restrict__ records)
{
    fused_hop_body<PPL, BUF, REC>(g, pa, pb, mh_out, p, hll_in, hll_out, cards_out, cards_stride, prm, skip_hubs, records);
}

}  // namespace ss

extern "C" int ss_fused_hop_stage(const ss_csr_graph *graph, const uint64_t *a, const uint64_t *b, int32_t P, uint32_t *mh1_out,
                                  uint32_t *mh2_out, int32_t p, uint8_t *hll1, float *cards1_out, uint8_t *hll2_out, float *cards2_out,
                                  int64_t cards_stride, const ss_hll_params *prm, void *stream)
{
    return ss_fused_hop_stage_records(graph, a, b, P, mh1_out, mh2_out, p, hll1, cards1_out, hll2_out, cards2_out, cards_stride, prm, nullptr, 0,
                                      stream);
}

extern "C" int ss_fused_hop_stage_records(const ss_csr_graph *graph, const uint64_t *a, const uint64_t *b, int32_t P, uint32_t *mh1_out,
                                          uint32_t *mh2_out, int32_t p, uint8_t *hll1, float *cards1_out, uint8_t *hll2_out,
                                          float *cards2_out, int64_t cards_stride, const ss_hll_params *prm, uint32_t *records,
                                          int64_t num_edges, void *stream)
{
    using namespace ss;
    if (!graph_given(graph)) return SS_ERR_INVALID_ARG;
    // written out: a shape without a kernel is answered before N is looked at (the caller uses ss_first_hop + ss_propagate)
    if (p != 8 || P <= 0 || P % kWave || P > 256) return SS_ERR_UNSUPPORTED;
    if (mh2_out && P != 128) return SS_ERR_UNSUPPORTED;  // the hub pass of the table hop is P = 128 only
    const int64_t N = graph->num_nodes;
    if (N == 0) return SS_OK;
    if (!mh1_out || !a || !b || !hll1 || !hll2_out || !graph_fits(*graph)) return SS_ERR_INVALID_ARG;
    // the stage's second hop, a table hop from the hop-1 tables: the record the checks fill; hop 1 is a copy with its own tables
    HopRequest hop2;
    hop2.a = a;
    hop2.b = b;
    hop2.P = P;
    hop2.p = p;
    hop2.M = 256;
    hop2.mh_in = mh2_out ? mh1_out : nullptr;
    hop2.mh_out = mh2_out;
    hop2.hll_in = hll1;
    hop2.hll_out = hll2_out;
    hop2.cards_out = cards2_out;
    hop2.cards_stride = cards_stride;
    hop2.stream = (hipStream_t)stream;
    int rc = take_params(hop2, prm);
    if (rc != SS_OK) return rc;
    if (!row_range_ok(*graph)) return SS_ERR_INVALID_ARG;
    hop2.g = to_args(*graph);
    if (hop2.g.rows() == 0) return SS_OK;
    // both table hops of this stage read hop-1 tables of `graph`: the MinHash one this stage computes from node ids, the HLL one it
    // computes too unless it is the caller's (cards1_out == NULL) -- the promise of SS_GRAPH_HOP_TABLES, made here for the whole-graph,
    // single-device build (a row range or mirrors: the sharded builds, left alone)
    const bool whole = graph->row_begin == 0 && graph->row_end == 0 && hop2.g.mir.n == 0;
    hop2.g.skip_self = self_skip_word(*graph, whole);
    // hub units: `lead` leading workgroups of the HLL first-hop launch serve both hop-1 tables, of the MinHash table hop both hop-2
    // tables (0: launches of their own, as in rounds 1-3)
    schedule_hubs(hop2, true);
    const bool own_hop1 = cards1_out != nullptr;  // the hop-1 HLL table is computed here as well (build_hash_tables)
    // how the kernel posts its hop-1 HLL rows: through a buffer descriptor when the table and the row after it fit the descriptor's
    // 32-bit byte count, with flat addresses otherwise.  SS_FUSED_POSTS=flat, read at every launch, forces the flat form at any size
    // (test hook; any other value, `buffer` included, leaves the choice to the size: a larger table cannot be described)
    const char *posts_env = getenv("SS_FUSED_POSTS");
    const bool buf_posts = buffer_describable(N * 256, 2 * 256) && !(posts_env && !strcmp(posts_env, "flat"));  // (lanes with nothing to fetch ask for row N)
    // the records form (fused_hop_body, REC): where the caller gave a workspace, the stage writes the hop-1 HLL table itself -- the
    // records are a by-product of that launch -- for the whole graph on one device, and the posts go through descriptors; and only on
    // graphs whose mean closed neighbourhood fills at most three quarters of a record, E + N <= 24 N, and that list no hub rows.
    // (Measured at 11 codes per node, the bench graph: 0.3958 -> 0.3875 ms per step, and at 21.8, citation2 size, where 2 % of the
    // gathered slots are flagged: 17.61 -> 17.50 ms; not beyond.)  Denser ones flag too many of their nodes and gather 64 bytes for
    // what a dense row answers better; on a skewed one most gathered slots name a
    // flagged node -- 28 % on the power-law bench graph (alpha 0.9) -- and every flagged slot is a dense load issued and awaited
    // AFTER the MinHash walk: 0.496 ms per step against 0.457 dense there.  (The caller's hub hint, csr.py / engine.py, drops the hub
    // list of a shape whose earlier build found none: the first build of a shape runs dense.)  SS_FUSED_RECORDS, read at every
    // launch: 0 forces the dense form, 1 the records form wherever it is legal (tests and measurements).
    const char *rec_env = getenv("SS_FUSED_RECORDS");
    const bool rec_legal = records && own_hop1 && whole && buf_posts;
    const bool rec_sparse = num_edges >= 0 && num_edges + N <= 24 * N && !hop2.hubs;
    const bool use_rec = rec_legal && (rec_env && !strcmp(rec_env, "1") ? true : rec_sparse && !(rec_env && !strcmp(rec_env, "0")));
    // hop 1 from node ids: both tables where the stage owns the HLL one (ONE hub pass from node ids for both hop-1 sketches: the
    // MinHash hub rows are not needed before the table hop below, but computing them here saves the hub launch after the fused
    // kernel), the MinHash table alone otherwise
    HopRequest hop1 = hop2;
    hop1.g.skip_self = nullptr;  // (the first hop keeps its self loop)
    hop1.mh_in = nullptr;
    hop1.mh_out = mh1_out;
    hop1.hll_in = nullptr;
    hop1.hll_out = own_hop1 ? hll1 : nullptr;
    hop1.cards_out = cards1_out;
    if (!own_hop1) hop1.cards_stride = 0;
    if (own_hop1) {
        if (!cards2_out) return SS_ERR_INVALID_ARG;
        rc = launch_hll_first_hop_rows(hop1, use_rec ? records : nullptr);
        if (rc == SS_OK && hop1.hub_launch_follows()) rc = launch_first_hop_hub_only(hop1);
        if (rc != SS_OK) return rc;
    }
    constexpr int rows_per_block = 4 * kFusedRows;
    const unsigned blocks = (unsigned)((hop2.g.rows() + rows_per_block - 1) / rows_per_block);
    // 5 workgroups are resident per CU; several times that many balance the tail.  Bench graph (58 blocks per CU): 12 / 15 / 20 / 25 / 30 /
    // 40 per CU: 148.7 / 147.8 / 146.2-146.9 / 149.9 / 149.2 / 151.2 us.  ppa / citation2 size (140 / 715 blocks per CU): 15 / 20 / 30 /
    // 48 / 64 / 100 / 200 / all: 1 832 / 1 819 / 1 774 / 1 724 / 1 738 / 1 728 / 1 751 / 1 748 us and 3 540 / 3 499 / 3 448 / 3 418 / 3 408 /
    // 3 419 / 3 457 / 3 814 us
    const int wg_per_cu = blocks > 256u * 128u ? 64 : 20;
    const unsigned grid = blocks < (unsigned)(256 * wg_per_cu) ? blocks : (unsigned)(256 * wg_per_cu);
    {
        // the fused kernel: hop-1 MinHash rows from node ids beside the hop-2 HLL rows (their self rows skipped only over a hop-1 HLL
        // table this stage has just built)
        GraphArgs g = hop2.g;
        if (!own_hop1) g.skip_self = nullptr;
        ProfileSpan span(hop2.stream, SS_PROF_FUSED, true);
        const uint32_t *const rec_in = use_rec ? records : nullptr;
        const auto launch = [&](auto buf, auto rec) {
            for_ppl(P, [&](auto ppl) {
                span.launch(fused_hop_persistent_kernel<decltype(ppl)::value, decltype(buf)::value, decltype(rec)::value>, dim3(grid), dim3(256), g, a,
                            b, mh1_out, p, hop2.hll_in, hll2_out, cards2_out, cards_stride, hop2.prm, hop2.hubs, rec_in);
            });
        };
        if (use_rec) launch(std::true_type{}, std::true_type{});
        else if (buf_posts) launch(std::true_type{}, std::false_type{});
        else launch(std::false_type{}, std::false_type{});
    }
    SS_LAUNCH_CHECK();
    // hub rows of the hop-1 MinHash table (from node ids): they must be in place before anything reads that table
    rc = own_hop1 ? SS_OK : launch_first_hop_hub_only(hop1);
    if (rc != SS_OK) return rc;
    if (!mh2_out) return launch_propagate_hub_only(hop2);  // hop-2 HLL hub rows alone
    // MinHash table hop of hop 2; its launch hosts the hub units of both hop-2 tables (or ONE hub pass for both follows)
    rc = launch_minhash_hop(hop2, hop2.lead > 0);
    return rc != SS_OK || !hop2.hub_launch_follows() ? rc : launch_propagate_hub_only(hop2);
}
