// ss_walks.hpp -- the neighbour walks shared by the propagation kernels (ss_propagate.hip, ss_first_hop.hip): table-reading walks (one 16-byte chunk per lane) and the table-free first-hop walk;
// and the ROW BODIES built on them -- one row folded by a wavefront or a 16-lane group, reduced, given its statistics and stored (minhash_hop_row, hll_hop_row, hll_hop_row16,
// first_hop_minhash_row, hll_first_hop_row16) -- that the build kernels and the update kernels of ss_update.hip both call: an updated table equals a rebuilt one bit for bit because of that.
#pragma once
#include "ss_common.hpp"

namespace ss {

__device__ __forceinline__ u32x4 shfl_xor4(u32x4 v, int mask)
{
    u32x4 r;
    r.x = (uint32_t)__shfl_xor((int)v.x, mask);
    r.y = (uint32_t)__shfl_xor((int)v.y, mask);
    r.z = (uint32_t)__shfl_xor((int)v.z, mask);
    r.w = (uint32_t)__shfl_xor((int)v.w, mask);
    return r;
}

__host__ __device__ constexpr int pow2_ceil(int x)
{
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// The generic walks below take the neighbours t = first, first + stride, ... < total four at a time: four id loads, then four
// row loads, then the four folds.  Two rules keep the loads of a batch in flight together (both learnt from the ISA): an id is
// loaded UNCONDITIONALLY (lanes past the row's end read a word that always exists and ignore it) -- a load inside `if (t < deg)`
// is awaited with vmcnt(0) at the end of its branch -- and nothing touches a loaded id (not even the widening to int64) before
// every load of the batch is issued.  The plain `#pragma unroll 4` loop they replace cost two dependent round trips per neighbour.
constexpr int kWalkBatch = 4;

// min over the neighbours t = first, first + stride, ... < total of MinHash chunk c (16 bytes per lane)
__device__ __forceinline__ u32x4 minhash_walk(const uint32_t *__restrict__ mh_in, const int32_t *__restrict__ nb, int deg, int total,
                                              int64_t self_row, int first, int stride, int P, int c)
{
    u32x4 acc = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const int32_t *always_valid = reinterpret_cast<const int32_t *>(mh_in);
    for (int t = first; t < total; t += kWalkBatch * stride) {
        int id[kWalkBatch];
        u32x4 x[kWalkBatch];
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) id[k] = *(t + k * stride < deg ? nb + t + k * stride : always_valid);
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) {
            const int tk = t + k * stride;
            const int64_t j = tk < deg ? (int64_t)id[k] : self_row;
            x[k] = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            if (tk < total) x[k] = *reinterpret_cast<const u32x4 *>(mh_in + j * P + 4 * c);
        }
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) acc = min4(acc, x[k]);
    }
    return acc;
}

// P = 128 (two 32-lane subgroups, subgroup sg takes the neighbours t = sg, sg + 2, ...): the first <= 64 neighbour ids of
// the row arrive with ONE coalesced load (lane l holds id l) and are handed out with v_readlane -- scalar, no memory
// pipeline -- instead of one broadcast load per neighbour and subgroup; the rest of a longer row is walked as before
__device__ __forceinline__ u32x4 minhash_walk128(const uint32_t *__restrict__ mh_in, const int32_t *__restrict__ nb, int deg, int total,
                                                 int64_t self_row, int lane)
{
    const int sg = lane >> 5, c = lane & 31;
    const int my_nb = lane < deg ? nb[lane] : 0;
    const int head = total < kWave ? total : kWave;
    u32x4 acc = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    // one pair of neighbours per iteration, NOT batched: batches of 2 / 4 pairs (masked or clamped) measured 194-198 us
    // against 187 us for this loop -- eight waves per SIMD already cover the latency, extra instructions only cost issue slots.
    // Round 3, all three shapes (1 / 2 / 3 / 4 pairs per iteration): collab size 191.4 / 193.1 / 196.2 / 199.4 us, ppa size
    // 2 936 / 2 977 / 2 972 / 2 975 us, citation2 size (1.5 GB table, HBM-resident) 5 661 / 5 566-5 591 / 5 572-5 604 / 5 581-5 593 us:
    // -1.5 % where the table lives in HBM, +1 % where it does not.  Not worth a second instantiation.
    for (int t0 = 0; t0 < head; t0 += 2) {  // wave-uniform trip count
        const int s0 = __builtin_amdgcn_readlane(my_nb, t0), s1 = __builtin_amdgcn_readlane(my_nb, (t0 + 1) & (kWave - 1));
        const int t = t0 + sg;
        const int64_t j = t < deg ? (int64_t)(sg ? s1 : s0) : self_row;
        if (t < head) acc = min4(acc, *reinterpret_cast<const u32x4 *>(mh_in + j * 128 + 4 * c));
    }
    if (total > kWave) acc = min4(acc, minhash_walk(mh_in, nb, deg, total, self_row, kWave + sg, 2, 128, c));
    return acc;
}

// hub / mega rows (propagate_hub_kernel): ONE wavefront folds a CONTIGUOUS chunk of <= 64 neighbours, nb[0 .. total) with
// nb[t >= deg] = the implicit self loop.  Ids arrive with one coalesced load and are handed out with v_readlane, the two
// 32-lane halves take alternating neighbours, four row loads per lane are requested before the first is folded (the generic
// batched walk pays a second, dependent, round trip per batch for its broadcast id loads)
__device__ __forceinline__ u32x4 minhash_chunk64(const uint32_t *__restrict__ mh_in, const int32_t *__restrict__ nb, int deg, int total,
                                                 int64_t self_row, int lane)
{
    const int sg = lane >> 5, c = lane & 31;
    const int my_nb = lane < deg ? nb[lane] : 0;
    u32x4 acc = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (int t0 = 0; t0 < total; t0 += 8) {  // wave-uniform trip count
        u32x4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s0 = __builtin_amdgcn_readlane(my_nb, (t0 + 2 * k) & (kWave - 1));
            const int s1 = __builtin_amdgcn_readlane(my_nb, (t0 + 2 * k + 1) & (kWave - 1));
            const int t = t0 + 2 * k + sg;
            const int64_t j = t < deg ? (int64_t)(sg ? s1 : s0) : self_row;
            x[k] = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            if (t < total) x[k] = *reinterpret_cast<const u32x4 *>(mh_in + j * 128 + 4 * c);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = min4(acc, x[k]);
    }
    return acc;
}

// byte-wise max over the same neighbour walk of HLL chunk c; even / odd bytes accumulated as packed u16
__device__ __forceinline__ u32x4 hll_walk(const uint8_t *__restrict__ hll_in, const int32_t *__restrict__ nb, int deg, int total,
                                          int64_t self_row, int first, int stride, int M, int c)
{
    u32x4 ae = {0u, 0u, 0u, 0u}, ao = {0u, 0u, 0u, 0u};
    const int32_t *always_valid = reinterpret_cast<const int32_t *>(hll_in);
    for (int t = first; t < total; t += kWalkBatch * stride) {
        int id[kWalkBatch];
        u32x4 x[kWalkBatch];
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) id[k] = *(t + k * stride < deg ? nb + t + k * stride : always_valid);
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) {
            const int tk = t + k * stride;
            const int64_t j = tk < deg ? (int64_t)id[k] : self_row;
            x[k] = u32x4{0u, 0u, 0u, 0u};
            if (tk < total) x[k] = *reinterpret_cast<const u32x4 *>(hll_in + j * M + 16 * c);
        }
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) hll_acc(ae, ao, x[k]);
    }
    return hll_acc_result(ae, ao);
}

// the same walk of a p = 8 table through its buffer descriptor (table_rsrc, ss_common.hpp: `bytes` records): one shift-or per load for
// a 32-bit offset instead of a 64-bit multiply-add, and the neighbours past `total` ask for the offset `bytes`, which the range check
// answers with zeros -- no branch around the loads.  c16 = 16 * c; always_valid: a word that lanes past the row's end may load
__device__ __forceinline__ u32x4 hll_walk_buffer(__amdgpu_buffer_rsrc_t rsrc, uint32_t bytes, const int32_t *always_valid,
                                                 const int32_t *__restrict__ nb, int deg, int total, int64_t self_row, int first, int stride,
                                                 uint32_t c16)
{
    u32x4 ae = {0u, 0u, 0u, 0u}, ao = {0u, 0u, 0u, 0u};
    for (int t = first; t < total; t += kWalkBatch * stride) {
        int id[kWalkBatch];
        u32x4 x[kWalkBatch];
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) id[k] = *(t + k * stride < deg ? nb + t + k * stride : always_valid);
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) {
            const int tk = t + k * stride;
            const uint32_t j = tk < deg ? (uint32_t)id[k] : (uint32_t)self_row;
            x[k] = buffer_load16(rsrc, tk < total ? (j << 8) | c16 : bytes);
        }
#pragma unroll
        for (int k = 0; k < kWalkBatch; ++k) hll_acc(ae, ao, x[k]);
    }
    return hll_acc_result(ae, ao);
}

// ---- one table-hop row by one wavefront (propagate_kernel, and the update kernels of ss_update.hip: ONE body, so that a row
// recomputed by an update carries the bits a rebuild gives it) ---------------------------------------------------------------
// A 16-byte chunk per lane; the wavefront is split into G = 64 / SG sub-groups (SG = pow2 >= chunks per row, <= 64) that walk G
// neighbours at a time, and their partial folds meet in sub-group 0 through cross-lane shuffles.  A row shared by the wavefronts of
// a workgroup: this one is wavefront `part` of `parts` (its sub-group sg takes the neighbours part * G + sg, + parts * G, ...).
// Every lane hands each of its chunks to emit(c, mine, acc) -- c: chunk index, mine: the lane holds the wavefront's fold of an
// existing chunk; emit is called by all lanes, so it may contain a barrier.
// MinHash: min over the neighbours; TP > 0: the row size at compile time (TP == 128 walks the whole row: part 0 of 1 only)
template <int TP, typename Emit>
__device__ __forceinline__ void minhash_hop_row(const uint32_t *__restrict__ mh_in, const int32_t *__restrict__ nb, int deg, int total,
                                                int64_t i, int P, int lane, int part, int parts, Emit emit)
{
    const int CM = P >> 2;
    const int SG = TP ? (pow2_ceil(TP >> 2) > kWave ? kWave : pow2_ceil(TP >> 2)) : (pow2_ceil(CM) > kWave ? kWave : pow2_ceil(CM));
    const int G = kWave / SG;
    const int sg = lane / SG, cl = lane % SG;
    for (int cb = 0; cb < CM; cb += SG) {
        const int c = cb + cl;
        const bool act = c < CM;
        u32x4 acc = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if constexpr (TP == 128) acc = minhash_walk128(mh_in, nb, deg, total, i, lane);
        else if (act) acc = minhash_walk(mh_in, nb, deg, total, i, part * G + sg, parts * G, P, c);
        for (int off = SG; off < kWave; off <<= 1) acc = min4(acc, shfl_xor4(acc, off));
        if (total == 0) acc = u32x4{0u, 0u, 0u, 0u};  // no in-edge, no self loop: all-zero row (PyG default)
        emit(c, act && sg == 0, acc);
    }
}

// HLL: byte-wise max over the neighbours, and -- want_card, wave-uniform -- the row's cardinality from the statistics of the chunks
// as they are emitted: emit(c, mine, acc) returns whether the lane now holds the FINISHED chunk (it may have folded other wavefronts'
// partials into acc); lane 0 hands the estimate to put_card.  TM > 0: the row size at compile time.
template <int TM, typename Emit, typename PutCard>
__device__ __forceinline__ void hll_hop_row(const uint8_t *__restrict__ hll_in, const int32_t *__restrict__ nb, int deg, int total, int64_t i,
                                            int M, int lane, int part, int parts, bool want_card, const EstimatorTables &est, Emit emit,
                                            PutCard put_card)
{
    const int CH = M >> 4;
    const int SG = TM ? (pow2_ceil(TM >> 4) > kWave ? kWave : pow2_ceil(TM >> 4)) : (pow2_ceil(CH) > kWave ? kWave : pow2_ceil(CH));
    const int G = kWave / SG;
    const int sg = lane / SG, cl = lane % SG;
    int nonzero = 0;
    float hsum = 0.0f;
    for (int cb = 0; cb < CH; cb += SG) {
        const int c = cb + cl;
        const bool act = c < CH;
        u32x4 acc = {0u, 0u, 0u, 0u};
        if (act) acc = hll_walk(hll_in, nb, deg, total, i, part * G + sg, parts * G, M, c);
        for (int off = SG; off < kWave; off <<= 1) acc = bytemax16(acc, shfl_xor4(acc, off));
        if (emit(c, act && sg == 0, acc) && want_card) hll_chunk_stats(acc, nonzero, hsum);
    }
    if (want_card) {
        // the lanes of sub-group 0 hold the partial statistics, the rest 0
        if (SG == kRow) {  // the 16 lanes of sub-group 0 are one DPP row
            nonzero = row16_sum_i(nonzero);
            hsum = row16_sum_f(hsum);
        } else {
            wave_sum_stats(nonzero, hsum);
        }
        if (lane == 0) put_card(hll_estimate(est, M - nonzero, hsum));
    }
}

// the first <= 16 neighbours of a row walked by ONE 16-lane DPP row: lane c fetches neighbour id c (one coalesced 64-byte
// load per row instead of one broadcast load per neighbour), the ids reach the other lanes through DPP row_newbcast, and
// four row chunks are requested before the first is consumed
template <int T0>
__device__ __forceinline__ void hll_visit16(const uint8_t *__restrict__ hll_in, int my_nb, int deg, int count, int64_t self_row, int c,
                                            u32x4 &ae, u32x4 &ao)
{
    if constexpr (T0 < 16) {
        if (__any(T0 < count)) {  // wave-uniform: skip batches no lane group needs
            u32x4 x[4];
            const int nbt[4] = {__builtin_amdgcn_update_dpp(0, my_nb, 0x150 + T0, 0xF, 0xF, false),  // row_newbcast:T0 ..
                                __builtin_amdgcn_update_dpp(0, my_nb, 0x150 + T0 + 1, 0xF, 0xF, false),
                                __builtin_amdgcn_update_dpp(0, my_nb, 0x150 + T0 + 2, 0xF, 0xF, false),
                                __builtin_amdgcn_update_dpp(0, my_nb, 0x150 + T0 + 3, 0xF, 0xF, false)};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = T0 + k < deg ? (int64_t)nbt[k] : self_row;
                x[k] = u32x4{0u, 0u, 0u, 0u};
                if (T0 + k < count) x[k] = *reinterpret_cast<const u32x4 *>(hll_in + j * 256 + 16 * c);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hll_acc(ae, ao, x[k]);
            }
            hll_visit16<T0 + 4>(hll_in, my_nb, deg, count, self_row, c, ae, ao);
        }
    }
}

__device__ __forceinline__ u32x4 hll_walk_first16(const uint8_t *__restrict__ hll_in, const int32_t *__restrict__ nb, int deg, int total,
                                                  int64_t self_row, int c)
{
    const int count = total < 16 ? total : 16;
    const int my_nb = c < deg ? nb[c] : 0;
    u32x4 ae = {0u, 0u, 0u, 0u}, ao = {0u, 0u, 0u, 0u};
    hll_visit16<0>(hll_in, my_nb, deg, count, self_row, c, ae, ao);
    return hll_acc_result(ae, ao);
}

__device__ __forceinline__ uint32_t permuted_hash(uint64_t a, uint64_t b, uint64_t hv)
{
    return (uint32_t)mod_mersenne61(a * hv + b);
}

// processes neighbour batches base = first_batch*64, += batch_stride*64 of one row; acc / hll_row accumulate
template <int PPL, bool DO_MH, bool DO_HLL>
__device__ __forceinline__ void first_hop_walk(const int32_t *__restrict__ nb, int deg, int total, int64_t self_row, int first_batch,
                                               int batch_stride, int p, const uint64_t (&a)[PPL], const uint64_t (&b)[PPL],
                                               uint32_t (&acc)[PPL], uint32_t *hll_row, int lane)
{
    for (int base = first_batch * kWave; base < total; base += batch_stride * kWave) {
        const int t = base + lane;
        const int64_t nid = t < deg ? (int64_t)nb[t] : self_row;  // t == deg is the implicit self loop; t > deg unused
        const uint64_t hv = hash_u64((uint64_t)(nid + 1));
        const uint32_t hv_lo = (uint32_t)hv, hv_hi = (uint32_t)(hv >> 32);
        // HLL (hashing.py:126-137): every lane scatters ITS neighbour's single register into the LDS row
        if (DO_HLL && t < total) atomicMax(&hll_row[hll_register_of(hv, 256)], hll_rank_of(hv, p));
        // MinHash: walk the batch; the neighbour's hash is wave-uniform, each lane evaluates its own permutations
        if (!DO_MH) continue;
        const int cnt = total - base < kWave ? total - base : kWave;
        int k = 0;
        // 4 neighbours per iteration: 4 * PPL independent multiply chains per lane (the integer multiplies have long
        // issue + latency; a single chain per wave leaves the VALU idle)
        for (; k + 3 < cnt; k += 4) {
            uint64_t hh[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                hh[u] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hv_hi, k + u) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k + u);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const uint32_t v0 = permuted_hash(a[q], b[q], hh[0]);
                const uint32_t v1 = permuted_hash(a[q], b[q], hh[1]);
                const uint32_t v2 = permuted_hash(a[q], b[q], hh[2]);
                const uint32_t v3 = permuted_hash(a[q], b[q], hh[3]);
                const uint32_t m01 = v0 < v1 ? v0 : v1, m23 = v2 < v3 ? v2 : v3;
                const uint32_t v = m01 < m23 ? m01 : m23;
                acc[q] = v < acc[q] ? v : acc[q];
            }
        }
        for (; k + 1 < cnt; k += 2) {
            const uint64_t h0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hv_hi, k) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k);
            const uint64_t h1 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hv_hi, k + 1) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k + 1);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const uint32_t v0 = permuted_hash(a[q], b[q], h0);
                const uint32_t v1 = permuted_hash(a[q], b[q], h1);
                const uint32_t v = v0 < v1 ? v0 : v1;
                acc[q] = v < acc[q] ? v : acc[q];
            }
        }
        if (k < cnt) {
            const uint64_t h0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hv_hi, k) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const uint32_t v = permuted_hash(a[q], b[q], h0);
                acc[q] = v < acc[q] ? v : acc[q];
            }
        }
    }
}

// one lane-quad of HLL registers (u32 each in LDS) -> packed bytes, stored + optional stats for the cardinality
__device__ __forceinline__ uint32_t pack_hll_quad(const uint32_t *row, int lane)
{
    const u32x4 r4 = *reinterpret_cast<const u32x4 *>(row + 4 * lane);
    return r4.x | (r4.y << 8) | (r4.z << 16) | (r4.w << 24);
}

// ---- two-phase MinHash first hop ----------------------------------------------------------------------------------------
// With x = (a*h + b) mod 2^64, the permuted hash is r = x mod (2^61 - 1) = (x & M) + (x >> 61) [- M], so unless the
// low word of x is within 8 of 2^32 its low 32 bits are simply   r32 = lo32(x) + (x >> 61),   0 <= x >> 61 <= 7.
// The first-hop kernel is bound by its VALU instruction count (measured: ~5 cycles per wave64 instruction whatever the
// opcode), and the exact hash costs 10 instructions per (neighbour, permutation).  Phase 1 therefore only finds, per
// permutation, WHICH neighbour attains the minimum, with 4 instructions per pair: x' = lo32(a_lo*h_lo + b_lo + 8)
// (v_mad_u64_u32; the +8 makes any low word that could wrap show up as x' < 8), key = x' with its low 6 bits replaced
// by the neighbour's slot in the 64-neighbour batch (v_bfi_b32), and the two smallest keys (v_med3_u32, v_min_u32).
// After each batch the hash of the slot holding the smallest key is fetched across lanes; phase 2 evaluates the
// exact hash once, for that neighbour.  The result is exact unless the two smallest keys fall into the same or
// adjacent 64-wide buckets (the order inside a bucket is by slot, not by value, and r32 may add up to 7) or a wrap is
// possible (bucket 0): probability ~4e-6 per (row, permutation); such rows are reported and redone by the exact walk.
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t d;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// first_batch / batch_stride: the wavefront takes the 64-neighbour batches first_batch, first_batch + batch_stride, ... of the row
// (first_hop_hub_kernel: 16 wavefronts share a hub row or a slice of a mega row; each one's minimum is exact -- or flagged --
// on its own, the workgroup combines them with an exact min)
template <int PPL>
__device__ __forceinline__ bool first_hop_minhash_fast(const int32_t *__restrict__ nb, int deg, int total, int64_t self_row,
                                                       const uint64_t (&a)[PPL], const uint64_t (&b)[PPL], uint32_t (&acc)[PPL], int lane,
                                                       int first_batch = 0, int batch_stride = 1)
{
    uint32_t m1[PPL], m2[PPL], h1_lo[PPL], h1_hi[PPL], a_lo[PPL], b8[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        m1[q] = m2[q] = 0xFFFFFFFFu;
        h1_lo[q] = h1_hi[q] = 0u;
        a_lo[q] = (uint32_t)a[q];
        b8[q] = (uint32_t)b[q] + 8u;
    }
    bool seen_self = false;  // the row lists its own node explicitly (graphs that already carry self loops)
    // (the ids of the NEXT batch are requested before the current one is walked -- unconditionally, from a word that always exists
    // for the lanes past the row's end: a hub unit's wavefront walks 4 - 16 batches, each of which began with an exposed round trip)
    const int32_t *always_valid = nb;  // (deg >= 1 whenever a batch exists beyond the self loop; nb[0] is never out of bounds then)
    int t_first = first_batch * kWave + lane;
    int cur = deg > 0 ? *(t_first < deg ? nb + t_first : always_valid) : 0;
    for (int base = first_batch * kWave; base < total; base += batch_stride * kWave) {
        const int t = base + lane;
        const int tn = t + batch_stride * kWave;
        const int nxt = deg > 0 ? *(tn < deg ? nb + tn : always_valid) : 0;
        const int64_t nid = t < deg ? (int64_t)cur : self_row;
        cur = nxt;
        const uint64_t hv = hash_u64((uint64_t)(nid + 1));
        const uint32_t hv_lo = (uint32_t)hv, hv_hi = (uint32_t)(hv >> 32);
        int cnt = total - base < kWave ? total - base : kWave;
        // a duplicated neighbour makes the two smallest keys collide for EVERY permutation (exact, but through the slow
        // path); the common duplicate is an explicit self edge + the implicit self loop (slot `deg`, always the last):
        // drop the implicit one, it adds nothing to a min
        seen_self |= __any(t < deg && nid == self_row);
        if (seen_self && total > deg && base + cnt == total) --cnt;
        uint32_t before[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) before[q] = m1[q];
        auto update = [&](uint32_t h_lo, uint32_t slot) {
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const uint32_t x = a_lo[q] * h_lo + b8[q];
                // key = (x & ~63) | slot as ONE v_bfi_b32 with the inline constant 63 as the mask: left to itself the compiler
                // keeps ~63 in an SGPR, and a VOP3 instruction may read only one scalar register, so the wave-uniform
                // slot costs a second instruction (and + add) -- 11 instead of 9 VALU per neighbour in the unrolled walk
                uint32_t key;
                asm("v_bfi_b32 %0, 63, %1, %2" : "=v"(key) : "s"(slot), "v"(x));
                m2[q] = umed3(m1[q], m2[q], key);       // second smallest key so far
                m1[q] = key < m1[q] ? key : m1[q];
            }
        };
        int k = 0;
        for (; k + 3 < cnt; k += 4) {
            uint32_t hl[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) hl[u] = (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k + u);
#pragma unroll
            for (int u = 0; u < 4; ++u) update(hl[u], (uint32_t)(k + u));
        }
        for (; k < cnt; ++k) update((uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k), (uint32_t)k);
        // the batch's hashes still sit one per lane: fetch the one whose slot now holds the smallest key
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int slot = (int)(m1[q] & 63u);
            const uint32_t cand_lo = (uint32_t)__shfl((int)hv_lo, slot), cand_hi = (uint32_t)__shfl((int)hv_hi, slot);
            const bool changed = m1[q] != before[q];
            h1_lo[q] = changed ? cand_lo : h1_lo[q];
            h1_hi[q] = changed ? cand_hi : h1_hi[q];
        }
    }
    bool ambiguous = false;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        acc[q] = permuted_hash(a[q], b[q], ((uint64_t)h1_hi[q] << 32) | h1_lo[q]);
        ambiguous |= (m1[q] < 64u) | ((m2[q] >> 6) - (m1[q] >> 6) <= 1u);
    }
    return ambiguous;
}

// ---- one first-hop row (hop 1 from node ids), shared by the build kernels and the update kernels -----------------------------------
// MinHash by one wavefront, over its batches first_batch, first_batch + batch_stride, ...: the two-phase walk, the wavefront's share
// redone by the exact walk when any lane flags it ambiguous, `acc` left at 0xFFFFFFFF when the wavefront has no batch.
// zero_empty: a row without in-edge and self loop becomes the all-zero row (PyG default) -- for a wavefront that owns the whole row.
template <int PPL>
__device__ __forceinline__ void first_hop_minhash_row(const int32_t *__restrict__ nb, int deg, int total, int64_t self_row, int p,
                                                      const uint64_t (&a)[PPL], const uint64_t (&b)[PPL], uint32_t (&acc)[PPL], int lane,
                                                      bool zero_empty, int first_batch = 0, int batch_stride = 1)
{
#pragma unroll
    for (int q = 0; q < PPL; ++q) acc[q] = 0xFFFFFFFFu;
    if (first_batch * kWave < total) {  // (wave-uniform) the wavefront has at least one batch
        const bool amb = first_hop_minhash_fast<PPL>(nb, deg, total, self_row, a, b, acc, lane, first_batch, batch_stride);
        if (__any(amb)) {
#pragma unroll
            for (int q = 0; q < PPL; ++q) acc[q] = 0xFFFFFFFFu;
            first_hop_walk<PPL, true, false>(nb, deg, total, self_row, first_batch, batch_stride, p, a, b, acc, nullptr, lane);
        }
    }
    if (zero_empty && total == 0) {
#pragma unroll
        for (int q = 0; q < PPL; ++q) acc[q] = 0u;
    }
}

// HLL (p = 8) by one 16-lane group through its LDS row image `row` (256 words, touched by this group alone): every lane scatters
// its neighbours' single registers with LDS atomics, then lane l packs registers 16l .. 16l+15, stores them and -- want_cards --
// lane 0 the cardinality.  nid0: the id of the lane's first neighbour (col[l], requested by the caller, who may do so rows ahead);
// always_valid: a word that lanes past the row's end may load; total = 0 with write = false: a group without a row to write.
// MIR: the row also goes to the peers' tables.
// REC: the group also leaves the row's CODE RECORD, 16 dwords at records + 16 * i, for the records form of the fused stage
// (ss_fused_hop.hip): lane l stores code(l) | code(l + 16) << 16 of its neighbours t = l and l + 16, code = register << 2 | rank << 10
// (a word offset into a row image and a rank <= 57; 0: no such neighbour -- rank 0 is a no-op under max).  No dedup, no sort, no
// count: two neighbours in one register are two codes.  A row of more than kRecordCodes neighbours, and -- rec_flag -- a row this
// group leaves to the hub units, gets kRecordDense in every dword: "read my dense row" (no code has its low two bits set).
constexpr int kRecordCodes = 2 * kRow;
constexpr uint32_t kRecordDense = 0xFFFFFFFFu;

template <bool MIR, bool REC = false>
__device__ __forceinline__ void hll_first_hop_row16(uint32_t *row, const int32_t *__restrict__ nb, int deg, int total, int64_t i, int nid0,
                                                    const int32_t *always_valid, int p, bool write, uint8_t *__restrict__ hll_out,
                                                    float *__restrict__ cards_out, int64_t cards_stride, const EstimatorTables &est,
                                                    bool want_cards, int l /* lane & 15 */, const Mirrors &mir,
                                                    uint32_t *__restrict__ records = nullptr, bool rec_flag = false)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x4 *>(row + 64 * k + 4 * l) = u32x4{0u, 0u, 0u, 0u};
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // (the id of the lane's NEXT neighbour is requested before the current one is hashed -- unconditionally, from an address
    // that always exists: rows of more than 16 neighbours otherwise pay one exposed round trip per 16 neighbours)
    int cur = nid0;
    int fresh = 0;  // registers this lane was the FIRST to set (the LDS atomic returns what was there: 0 exactly once per register)
    [[maybe_unused]] uint32_t rec = 0u;
    for (int t = l; t < total; t += kRow) {
        const int nxt = *(t + kRow < deg ? nb + t + kRow : always_valid);
        const int64_t nid = t < deg ? (int64_t)cur : i;
        cur = nxt;
        const uint64_t hv = hash_u64((uint64_t)(nid + 1));
        if constexpr (REC) {
            const uint32_t code = (hll_register_of(hv, 256) << 2) | (hll_rank_of(hv, p) << 10);
            if (t < kRow) rec = code;
            else if (t < kRecordCodes) rec |= code << 16;
        }
        fresh += atomicMax(&row[hll_register_of(hv, 256)], hll_rank_of(hv, p)) == 0u ? 1 : 0;  // (ranks are >= 1)
    }
    if constexpr (REC) {
        if (write || rec_flag) records[i * kRow + l] = (rec_flag || total > kRecordCodes) ? kRecordDense : rec;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // lane l owns registers 16l .. 16l+15
    u32x4 packed;
    uint32_t *pw = reinterpret_cast<uint32_t *>(&packed);
#pragma unroll
    for (int k = 0; k < 4; ++k) pw[k] = pack_hll_quad(row + 16 * l, k);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int nonzero = 0;
    float hsum = 0.0f;
    if (want_cards) {
        // A hop-1 row has at most deg + 1 non-zero registers, so nearly every row -- every one below 147 neighbours at p = 8 --
        // is estimated by linear counting, which needs the number of zero registers and nothing else (hashing.py:221-226):
        // that number comes out of the atomics above.  Only a wavefront holding a row that leaves the linear-counting range
        // digests the packed registers for the harmonic sum (12 instructions per dword, a third of this kernel's VALU work).
        nonzero = row16_sum_i(fresh);
        const int zeros = 256 - nonzero;
        if (__any(!(zeros > 0 && zeros >= est.lc_min_zeros))) {  // wave-uniform
            int nz2 = 0;
            hll_chunk_stats(packed, nz2, hsum);
            hsum = row16_sum_f(hsum);
        }
    }
    if (write) {
        *reinterpret_cast<u32x4 *>(hll_out + i * 256 + 16 * l) = packed;
        if constexpr (MIR) mirror_hll16(mir, i * 256 + 16 * l, packed);
        if (want_cards && l == 0) {
            const float card = hll_estimate(est, 256 - nonzero, hsum);
            cards_out[i * cards_stride] = card;
            if constexpr (MIR) mirror_card(mir, i * cards_stride, card);
        }
    }
}

// ---- MinHash first hop of R consecutive rows by one wavefront (first_hop_rows_kernel, fused_hop_persistent_kernel) ------
// init() reads the bounds of all rows with one load (lane l holds rowptr[first + l] as an offset from the first row's start),
// the permutation parameters, and the first batch; load_batch() fetches 64 - R consecutive `col` entries of the chunk and
// hashes them, one per lane -- lanes 64 - R .. 63 always carry the hashes of the rows' OWN ids, so the implicit self loop of
// row r is slot 64 - R + r of whatever batch is current; row(r) walks row r over its slice of the batch(es) with the
// two-phase evaluation (first_hop_minhash_fast above), evaluates the winner exactly and stores the row.  Rows flagged
// ambiguous are redone by the exact walk; a row that lists itself leaves its implicit self loop out (a duplicate would flag it).
// row() has two forms of the walk: a row whose entries all lie in the current batch -- nearly every row -- takes one pass without
// the bookkeeping of a winner carried from batch to batch; the others loop over their batches.
// MIR: rows also go to the peers' tables (peer-write build); a compile-time switch -- the store loop and the pointer it needs
// cost first_hop_rows_kernel 14 registers and fused_hop_persistent_kernel a wavefront per SIMD
template <int PPL, int R, bool MIR = false>
struct MinhashRows {
    static constexpr int P = PPL * kWave;
    static constexpr int kNb = kWave - R;  // col entries per batch
    int lane, rows, rel, c_n, base, p, hub_threshold, n_self32;
    int own;  // the batch id of this lane minus the chunk's first row: slot k of the batch holds row r's own id iff own == r there
    const Mirrors *mir;  // peers' tables (kernel-argument memory: the pointer stays valid for the kernel's lifetime)
    bool skip_hubs;
    int64_t i0, n_self;
    const int32_t *nb;
    uint64_t a[PPL], b[PPL];
    uint32_t a_lo[PPL], b8[PPL], hv_lo, hv_hi;

    __device__ __forceinline__ void load_batch() { set_batch(batch_id()); }

    // once per wavefront: lane constants (permutation parameters, self-loop count, hub rule)
    __device__ __forceinline__ void setup(const GraphArgs &g, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb, int p_, bool skip)
    {
        lane = threadIdx.x & (kWave - 1);
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            a[q] = pa[lane + kWave * q];
            b[q] = pb[lane + kWave * q];
            a_lo[q] = (uint32_t)a[q];
            b8[q] = (uint32_t)b[q] + 8u;
        }
        n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
        n_self32 = (int)(n_self < 0x7FFFFFFF ? n_self : 0x7FFFFFFF);  // row ids are < 2^31: i < n_self is (int)i < n_self32
        p = p_;
        skip_hubs = skip;
        hub_threshold = g.hub_threshold;
        mir = MIR ? &g.mir : nullptr;
    }

    // rows [first_row, first_row + n_rows) become the current chunk; rp: lane l holds rowptr[first_row + l] (l <= n_rows)
    __device__ __forceinline__ void begin(const GraphArgs &g, int64_t first_row, int n_rows, int64_t rp)
    {
        i0 = first_row;
        rows = n_rows;
        const int64_t c_lo = ((int64_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)rp >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((int)rp);
        rel = (int)(rp - c_lo);
        c_n = __builtin_amdgcn_readlane(rel, rows);  // col entries of the whole chunk
        nb = g.col + c_lo;
        base = 0;  // chunk-relative position of the current batch's first col entry
    }

    // the id lane `lane` contributes to the batch at `base`: a col entry, or (lanes kNb..) the id of one of the chunk's own rows
    __device__ __forceinline__ int64_t batch_id() const
    {
        const int t = base + lane;
        return lane >= kNb ? i0 + (lane - kNb) : (t < c_n ? (int64_t)nb[t] : 0);
    }
    __device__ __forceinline__ void set_batch(int64_t id)
    {
        own = (int)id - (int)i0;  // (node ids are < 2^31: checked by the entry points)
        const uint64_t hv = hash_u64((uint64_t)(id + 1));
        hv_lo = (uint32_t)hv;
        hv_hi = (uint32_t)(hv >> 32);
    }

    // false: this wavefront owns no row of [g.row0, g.row1)
    __device__ __forceinline__ bool init(const GraphArgs &g, int64_t first_row, const uint64_t *__restrict__ pa,
                                         const uint64_t *__restrict__ pb, int p_, bool skip)
    {
        if (first_row >= g.row1) return false;
        const int n_rows = (int)(g.row1 - first_row < R ? g.row1 - first_row : R);
        const int l = threadIdx.x & (kWave - 1);
        const int64_t rp = l <= n_rows ? g.rowptr[first_row + l] : 0;
        setup(g, pa, pb, p_, skip);
        begin(g, first_row, n_rows, rp);
        load_batch();
        return true;
    }

    __device__ __forceinline__ void row(int r, uint32_t *__restrict__ mh_out)
    {
        const int64_t i = i0 + r;
        const int p0 = __builtin_amdgcn_readlane(rel, r), p1 = __builtin_amdgcn_readlane(rel, r + 1);
        const int deg = p1 - p0;
        if (skip_hubs && deg > hub_threshold) return;  // left to first_hop_hub_kernel
        const bool self = (int)i < n_self32;  // (a scalar compare; the 64-bit one is a VALU instruction)
        uint32_t acc[PPL];
        bool redo = false;
        if (deg + (self ? 1 : 0) == 0) {
#pragma unroll
            for (int q = 0; q < PPL; ++q) acc[q] = 0u;  // no in-edge, no self loop: all-zero row (PyG default)
        } else {
            uint32_t m1[PPL], m2[PPL], h1_lo[PPL], h1_hi[PPL];
            auto key_of = [&](int q, uint32_t h_lo, uint32_t slot) {
                const uint32_t x = a_lo[q] * h_lo + b8[q];
                uint32_t key;
                asm("v_bfi_b32 %0, 63, %1, %2" : "=v"(key) : "s"(slot), "v"(x));  // (x & ~63) | slot, see first_hop_minhash_fast
                return key;
            };
            auto update = [&](uint32_t h_lo, uint32_t slot) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    const uint32_t key = key_of(q, h_lo, slot);
                    m2[q] = umed3(m1[q], m2[q], key);
                    m1[q] = key < m1[q] ? key : m1[q];
                }
            };
            bool seen_self = false;
            // a row that lists itself would meet its implicit self loop as a duplicate (ambiguous for every permutation).
            // One compare per row (`own`, formed once per batch, against the wave-uniform r) and the row's slots [s_lo, s_hi) as a
            // mask from the scalar unit: an entry equal to ANOTHER row of the chunk, or the own-id lanes kNb.., are not in it
            auto note_self = [&](int s_lo, int s_hi) {
                if (s_hi > s_lo) seen_self |= (__ballot(own == r) & ((~0ull >> (kWave - (s_hi - s_lo))) << s_lo)) != 0ull;
            };
            // slots [s_lo, s_hi) of the current batch, entries of this row
            auto walk = [&](int s_lo, int s_hi) {
                int k = s_lo;
                for (; k + 3 < s_hi; k += 4) {
                    uint32_t hl[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) hl[u] = (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k + u);
#pragma unroll
                    for (int u = 0; u < 4; ++u) update(hl[u], (uint32_t)(k + u));
                }
                for (; k < s_hi; ++k) update((uint32_t)__builtin_amdgcn_readlane((int)hv_lo, k), (uint32_t)k);
            };
            auto update_own = [&]() { update((uint32_t)__builtin_amdgcn_readlane((int)hv_lo, kNb + r), (uint32_t)(kNb + r)); };
            // the batch's hashes still sit one per lane: fetch the one whose slot now holds the smallest key.  (ds_bpermute takes a
            // byte address and uses its bits 2..7, the lane: the key shifted left by two IS the address of its slot)
            auto winner = [&](int q, uint32_t &lo, uint32_t &hi) {
                const int slot4 = (int)(m1[q] << 2);
                lo = (uint32_t)__builtin_amdgcn_ds_bpermute(slot4, (int)hv_lo);
                hi = (uint32_t)__builtin_amdgcn_ds_bpermute(slot4, (int)hv_hi);
            };
            if (p1 <= base + kNb) {
                // (wave-uniform) the row's col entries all lie in the current batch -- p0 >= base always: the batch only moves up to
                // the position a row has reached.  Nearly every row at four rows per wavefront (bench graph: 99.9 % of the chunks have
                // at most kNb entries).  Its winner is whatever slot m1 names after the one pass: none carried from an earlier batch,
                // so none to initialise, to remember m1 for, or to select against.  (A row whose only key is 0xFFFFFFFF has it in
                // m1 and m2, is flagged below and redone, as before.)  And its first key -- of its first entry, or of its self loop
                // when it has no entry -- has nothing to be compared with: m1 = key, m2 = the start value, which is what an update
                // of m1 = m2 = 0xFFFFFFFF gives, without the two initialisations and the two comparisons
                const int s_lo = p0 - base, s_hi = p1 - base;
                note_self(s_lo, s_hi);
                const int first_slot = deg > 0 ? s_lo : kNb + r;
                const uint32_t first_h = (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, first_slot);
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    m1[q] = key_of(q, first_h, (uint32_t)first_slot);
                    m2[q] = 0xFFFFFFFFu;
                }
                walk(s_lo + 1, s_hi);
                if (deg > 0 && self && !seen_self) update_own();
#pragma unroll
                for (int q = 0; q < PPL; ++q) winner(q, h1_lo[q], h1_hi[q]);
            } else {
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    m1[q] = m2[q] = 0xFFFFFFFFu;
                    h1_lo[q] = h1_hi[q] = 0u;
                }
                int pos = p0;
                for (;;) {
                    if (pos < p1 && pos >= base + kNb) {  // the row starts (or continues) beyond the current batch
                        base += (pos - base) / kNb * kNb;  // (a skipped hub row may lie in between: jump, do not step)
                        load_batch();
                    }
                    const int s_lo = pos - base;
                    const int s_hi = p1 - base < kNb ? p1 - base : kNb;
                    uint32_t before[PPL];
#pragma unroll
                    for (int q = 0; q < PPL; ++q) before[q] = m1[q];
                    note_self(s_lo, s_hi);
                    walk(s_lo, s_hi);
                    pos = base + (s_hi > s_lo ? s_hi : s_lo);
                    const bool last = pos >= p1;
                    if (last && self && !seen_self) update_own();
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        uint32_t cand_lo, cand_hi;
                        winner(q, cand_lo, cand_hi);
                        const bool changed = m1[q] != before[q];
                        h1_lo[q] = changed ? cand_lo : h1_lo[q];
                        h1_hi[q] = changed ? cand_hi : h1_hi[q];
                    }
                    if (last) break;
                }
            }
            bool ambiguous = false;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                // x = a * h + b (mod 2^64); the permuted hash is x mod (2^61 - 1) = (x & M) + (x >> 61) [- M], whose low word
                // is lo32(x) + (x >> 61) unless the sum reaches M -- only possible when bits 32..60 of x are all ones: such
                // a row (2^-29 per evaluation) is flagged and redone exactly like the key collisions
                const uint64_t lo = (uint64_t)a_lo[q] * h1_lo[q] + b[q];
                const uint32_t hi = (uint32_t)(lo >> 32) + a_lo[q] * h1_hi[q] + (uint32_t)(a[q] >> 32) * h1_lo[q];
                acc[q] = (uint32_t)lo + (hi >> 29);
                // (same or adjacent buckets, (m2 >> 6) - (m1 >> 6) <= 1 with m2 >= m1, is m2 below the end of the bucket after m1's)
                ambiguous |= ((hi & 0x1FFFFFFFu) == 0x1FFFFFFFu) | (m1[q] < 64u) | (m2[q] - (m1[q] & ~63u) < 128u);
            }
            redo = __any(ambiguous);
        }
        if (redo) {
#pragma unroll
            for (int q = 0; q < PPL; ++q) acc[q] = 0xFFFFFFFFu;
            first_hop_walk<PPL, true, false>(nb + p0, deg, deg + (self ? 1 : 0), i, 0, 1, p, a, b, acc, nullptr, lane);
        }
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            mh_out[i * P + lane + kWave * q] = acc[q];
            if constexpr (MIR) mirror_mh1(*mir, i * P + lane + kWave * q, acc[q]);
        }
    }
};

// the number of non-zero registers among the 16 of one chunk (the integer half of hll_chunk_stats)
__device__ __forceinline__ int hll_chunk_nonzero(u32x4 x)
{
    return __builtin_popcount(nonzero_byte_flags(x.x)) + __builtin_popcount(nonzero_byte_flags(x.y)) +
           __builtin_popcount(nonzero_byte_flags(x.z)) + __builtin_popcount(nonzero_byte_flags(x.w));
}

// everything after the first `walked` neighbours of the four rows of a wavefront have been folded into `acc` (one 16-lane
// group per row, lane c = chunk c): the rest of rows up to kSolo neighbours by their own group, what is left of longer rows
// by all four groups together, then the row's statistics, its store and its cardinality.  `total` = 0 marks a group without
// a row to write (past the end, or a hub row left to the hub pass).
// walk(nb, deg, total, self_row, first, stride): the fold of chunk c of those neighbours (hll_walk, or hll_walk_buffer)
template <bool MIR, typename Walk>
__device__ __forceinline__ void hll_row16_finish_by(int64_t i, bool write, const int32_t *__restrict__ nb, int deg, int total, u32x4 acc,
                                                    int walked, Walk walk, uint8_t *__restrict__ hll_out, float *__restrict__ cards_out,
                                                    int64_t cards_stride, const EstimatorTables &est, bool want_cards, int c /* lane & 15 */,
                                                    const Mirrors &mir)
{
    constexpr int M = 256;
    // every lane group walks the first kSolo neighbours of its own row; what is left of longer rows is walked by the whole
    // wavefront, one row at a time (group g takes every 4th neighbour), so a wavefront lasts about sum(excess)/4 instead
    // of max(degree) iterations -- skewed graphs put rows of 10 and of 500 neighbours into the same wavefront
    constexpr int kSolo = 32;
    if (__any(total > walked)) acc = bytemax16(acc, walk(nb, deg, total < kSolo ? total : kSolo, i, walked, 1));
    const unsigned long long long_rows = __ballot(total > kSolo);
    if (long_rows) {
        const int grp = (threadIdx.x & (kWave - 1)) / kRow;
#pragma unroll
        for (int gg = 0; gg < kWave / kRow; ++gg) {
            if (!((long_rows >> (kRow * gg)) & 1ull)) continue;  // wave-uniform
            const uint64_t nb_bits = (uint64_t)(uintptr_t)nb;
            const int32_t *nb_g = (const int32_t *)(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(nb_bits >> 32), kRow * gg) << 32) |
                                                             (uint32_t)__builtin_amdgcn_readlane((int)nb_bits, kRow * gg));
            const int deg_g = __builtin_amdgcn_readlane(deg, kRow * gg), total_g = __builtin_amdgcn_readlane(total, kRow * gg);
            const int64_t i_g = ((int64_t)__builtin_amdgcn_readlane((int)((uint64_t)i >> 32), kRow * gg) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)i, kRow * gg);
            u32x4 part = walk(nb_g, deg_g, total_g, i_g, kSolo + grp, kWave / kRow);
            part = bytemax16(part, shfl_xor4(part, 16));
            part = bytemax16(part, shfl_xor4(part, 32));
            if (grp == gg) acc = bytemax16(acc, part);
        }
    }
    int nonzero = 0;
    float hsum = 0.0f;
    if (want_cards) {
        // the zero count first: a row that stays in the linear-counting range (hll_estimate: zeros > 0 && zeros >= lc_min_zeros) is
        // estimated from it alone, and nearly every hop-2 row of a sparse graph does (bench graph: 99.5 % of the rows, 98 % of the
        // wavefronts).  Only a wavefront holding a row that leaves the range digests the registers for the harmonic sum -- the same
        // dwords in the same order, the same row reduction (hll_chunk_stats, row16_sum_f): the sum that is read has the bits it had
        nonzero = row16_sum_i(hll_chunk_nonzero(acc));
        const int zeros = M - nonzero;
        if (__any(!(zeros > 0 && zeros >= est.lc_min_zeros))) {  // wave-uniform
            int nz2 = 0;
            hll_chunk_stats(acc, nz2, hsum);
            hsum = row16_sum_f(hsum);
        }
    }
    if (write) {
        *reinterpret_cast<u32x4 *>(hll_out + i * M + 16 * c) = acc;
        if constexpr (MIR) mirror_hll16(mir, i * M + 16 * c, acc);
        if constexpr (MIR) {
            if (want_cards && c == 0) {
                const float card = hll_estimate(est, M - nonzero, hsum);
                cards_out[i * cards_stride] = card;
                mirror_card(mir, i * cards_stride, card);
            }
        } else {
            if (want_cards && c == 0) cards_out[i * cards_stride] = hll_estimate(est, M - nonzero, hsum);
        }
    }
}

template <bool MIR = true>
__device__ __forceinline__ void hll_row16_finish(int64_t i, bool write, const int32_t *__restrict__ nb, int deg, int total, u32x4 acc,
                                                 int walked, const uint8_t *__restrict__ hll_in, uint8_t *__restrict__ hll_out,
                                                 float *__restrict__ cards_out, int64_t cards_stride, const EstimatorTables &est,
                                                 bool want_cards, int c /* lane & 15 */, const Mirrors &mir)
{
    hll_row16_finish_by<MIR>(i, write, nb, deg, total, acc, walked,
                             [&](const int32_t *nb_, int deg_, int total_, int64_t self_row, int first, int stride) {
                                 return hll_walk(hll_in, nb_, deg_, total_, self_row, first, stride, 256, c);
                             },
                             hll_out, cards_out, cards_stride, est, want_cards, c, mir);
}

// HLL table hop for FOUR destination rows per wavefront: one 16-lane DPP row per destination, lane c owns the 16-byte
// chunk c of the 256-byte HLL row.  Compared with one destination per wave (hll_walk + two cross-group shuffles +
// an epilogue that uses 16 of 64 lanes) this keeps 4x the loads in flight per wave and runs the cardinality
// epilogue for 4 rows at once.  `row` < 0 marks an inactive group.  M = 256 only.
__device__ __forceinline__ void hll_hop_row16(const GraphArgs &g, int64_t row, bool skip_hubs, const uint8_t *__restrict__ hll_in,
                                              uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride,
                                              const EstimatorTables &est, bool want_cards, int c /* lane & 15 */)
{
    const bool ok = row >= 0;
    const int64_t i = ok ? row : 0;
    const int64_t rb = g.rowptr[i];
    const int deg = (int)(g.rowptr[i + 1] - rb);
    const bool hub = skip_hubs && deg > g.hub_threshold;
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    const bool skip_self = g.skip_self && *g.skip_self != 0;  // (one scalar load per wavefront)
    const int total = (!ok || hub) ? 0 : table_hop_total(deg, i < n_self, skip_self);
    const int32_t *nb = g.col + rb;
    const u32x4 acc = hll_walk_first16(hll_in, nb, deg, total, i, c);
    hll_row16_finish(i, ok && !hub, nb, deg, total, acc, 16, hll_in, hll_out, cards_out, cards_stride, est, want_cards, c, g.mir);
}

}  // namespace ss
