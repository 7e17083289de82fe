// ss_pair_math.hpp -- the per-pair arithmetic of the set-intersection estimate I[k1, k2] = J * U (reference hashing.py:167-189),
// shared by the pair query (ss_pairs.hip), the masked query (ss_masked.hip) and the one-vs-all scans (ss_topk.hip, ss_topk_head.hip).
// Every kernel gives lane l of a 16-lane row the chunks l, l + 16, ... of a sketch row, accumulates a pair's statistics per lane with
// these helpers in chunk order, and reduces them with row16_sum_i / row16_sum_f: that is what makes their fp32 harmonic sums -- and so
// their estimates -- bit-identical.  The run-time-shape statistic (pair_stats_generic), the lane select and the degree-normalised copy
// have ONE source here for pair_features_kernel, pair_features_runs_kernel, topk_score_scan_kernel and masked_pairs_kernel.  The finish
// of a pair between them -- lane c < h^2: intersection_estimate, __shfl of I to the row, assemble_features -- stays written out in each
// of the four: as one function it changed their registers (DESIGN_EXPERIMENTS "One source for the pair finish").  The host half at the
// end is what their entry points share: the table pointers, the pair query's request record, the (h, P, M) -> template arguments
// dispatch of the five scan / query kernels and the argument checks.  rank_score_scan_kernel (ss_rank.hip) repeats the
// body of topk_score_scan_kernel: one source for the two was built and measured -- two instantiations changed occupancy and the scan
// was 1 - 2 % slower -- so both stay written out and share their host half only (ss_head_scan.hpp, DESIGN_EXPERIMENTS 3.13).
#pragma once
#include <type_traits>
#include <utility>
#include "ss_feature_algebra.hpp"

namespace ss {

struct HeadArgs;  // (ss_head.hpp: PairQuery below names it by pointer only)

// (measured and rejected in round 3: counting equal dwords as 4 - sum(min(a ^ b, 1)) instead of v_cmp_eq_u32 + v_addc_co_u32 -- hipcc
// puts an `s_nop 1` behind each of the 72 compares of a pair at h = 3, gfx950 wanting two wait states between a VALU write of VCC
// and its VALU read -- removes 59 of 102 s_nops but adds 47 VALU instructions: level on cache-resident tables, 3.5 % SLOWER on
// citation2-size tables (3 713 against 3 580 us for 4 M pairs): other wavefronts fill the wait states, nobody fills extra instructions)
__device__ __forceinline__ int eq4(u32x4 a, u32x4 b)
{
    return (int)(a.x == b.x) + (int)(a.y == b.y) + (int)(a.z == b.z) + (int)(a.w == b.w);
}

// generic path: union of two 16-register chunks -> non-zero count and harmonic sum
__device__ __forceinline__ void union_stats(u32x4 a, u32x4 b, int &nonzero, float &hsum)
{
    hll_chunk_stats(bytemax16(a, b), nonzero, hsum);
}

// fast path: a 16-register HLL chunk pre-digested once per row so that each of the h^2 unions costs
// 4 instructions per dword: bf16 patterns of 2^-r (even / odd registers; max of registers == unsigned min of
// patterns) and a 16-bit "register is zero" mask (union register zero <=> zero in both rows).
// The sums it feeds are the generic path's, term for term: the pattern of a byte-wise max is the min of the patterns.
struct HllChunk {
    uint32_t pe[4], po[4];
    uint32_t zero_mask;
};

__device__ __forceinline__ HllChunk digest_chunk(u32x4 x)
{
    HllChunk c;
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    uint32_t nzbits = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        c.pe[d] = regs_even_to_bf16(w[d]);
        c.po[d] = regs_odd_to_bf16(w[d]);
        nzbits |= nonzero_byte_flags(w[d]) >> (7 - d);  // flags live in bits 7,15,23,31 -> bits d, 8+d, 16+d, 24+d
    }
    c.zero_mask = ~nzbits & 0x0F0F0F0Fu;
    return c;
}

__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
    u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
}

__device__ __forceinline__ void union_stats_digested(const HllChunk &a, const HllChunk &b, int &zeros, float &hsum)
{
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        hsum = dot2_ones(pk_min_u16(a.pe[d], b.pe[d]), hsum);
        hsum = dot2_ones(pk_min_u16(a.po[d], b.po[d]), hsum);
    }
    zeros += __builtin_popcount(a.zero_mask & b.zero_mask);
}

// I = (match / P) * hll_count(union) from the row totals of one combination (hashing.py:184-187)
__device__ __forceinline__ float intersection_estimate(const EstimatorTables &est, int match, int zeros, float hsum, int P)
{
    const float jac = (float)match / (float)P;
    return jac * hll_estimate(est, zeros, hsum);
}

// lane k of a row keeps element k of an array every lane holds (lanes >= N keep element 0).  Every element is read BEFORE its select:
// with `(l == k) ? a[k] : x` the optimiser, which sees this function before it is inlined, sinks the conditional loads into one load at
// a selected offset, and the caller's array then stays in scratch / LDS instead of registers.
template <typename T, int N>
__device__ __forceinline__ T lane_select(const T (&a)[N], int l)
{
    T x = a[0];
#pragma unroll
    for (int k = 1; k < N; ++k) {
        const T ak = a[k];
        x = (l == k) ? ak : x;
    }
    return x;
}

// run-time sketch shape: the row totals (match << 20) | zeros and harmonic sum of ONE (k1, k2) from rows of CM MinHash and CH HLL
// chunks, in global memory or LDS (P <= 2048: the packed word uses all 32 bits)
__device__ __forceinline__ void pair_stats_generic(const u32x4 *mh_u, const u32x4 *mh_v, const u32x4 *hll_u, const u32x4 *hll_v, int CM,
                                                   int CH, int l, int &mz, float &hs)
{
    int match = 0, nonzero = 0, chunks = 0;
    float hsum = 0.0f;
    for (int c = l; c < CM; c += kRow) match += eq4(mh_u[c], mh_v[c]);
    for (int c = l; c < CH; c += kRow, ++chunks) union_stats(hll_u[c], hll_v[c], nonzero, hsum);
    mz = row16_sum_i((match << 20) | (16 * chunks - nonzero));
    hs = row16_sum_f(hsum);
}

// BUDDY._append_degree_normalised (reference models/elph.py:276-293) for one feature: f / sqrt(d_u * d_v), NaN / Inf (zero-degree nodes)
// replaced by 0.  What a pair with ids out of range gets differs per caller on purpose and stays there: the feature epilogue NaNs my_f
// before this copy and the copy after it, the head path NaNs only the score, the run-aware kernel writes its NaN row before it gets here.
__device__ __forceinline__ float degree_normalised(float my_f, float du, float dv)
{
    const float normed = my_f / sqrtf(du * dv);
    return (isnan(normed) || isinf(normed)) ? 0.0f : normed;
}

// ---- host side: what the entry points of these kernels share ----------------------------------------------------------------------
struct HopTables {
    const uint32_t *mh[SS_MAX_HOPS];
    const uint8_t *hll[SS_MAX_HOPS];
};

inline bool fill_hop_tables(const uint32_t *const *mh, const uint8_t *const *hll, int h, HopTables &out)
{
    out = {};
    for (int k = 0; k < h; ++k) {
        if (!mh[k] || !hll[k]) return false;
        out.mh[k] = mh[k];
        out.hll[k] = hll[k];
    }
    return true;
}

// What one launch of the pair kernels takes (ss_pairs.hip): every entry point there fills it by name, the launchers read it.
struct PairQuery {
    const int64_t *links;
    const int32_t *order;  // nullable: position t of the walk is pair order[t]
    int64_t B, N;
    int h;
    HopTables tabs;
    int P, M;
    const float *cards;
    int64_t cards_stride;
    ss_hll_params prm;
    uint32_t flags;
    const float *degrees;  // nullable: the degree-normalised copy is appended / fed to the head
    float *out;
    int32_t *dbg_match, *dbg_zero;  // the three dbg_*: ss_pair_features alone
    float *dbg_inter;
    int32_t *err;
    hipStream_t stream;
    bool grouped;            // the walk has locality: the capped register budget whatever the batch size
    const HeadArgs *head;    // nullable: ss_pair_scores (ss_head.hpp)
};

// the shapes with compile-time kernels: p = 8 and the permutation counts the first hop is specialised for (ss_first_hop: P / 64 = 1 .. 4)
inline bool is_fast_pair_shape(int P, int M) { return M == 256 && (P == 64 || P == 128 || P == 192 || P == 256); }

// launch(H, CMPL), both std::integral_constant<int, .>, for a checked hop count and sketch shape: instantiation I = 5 (H - 1) + CMPL
// of PairShapes.  CMPL > 0: fast shape (p = 8, P = 64 * CMPL: TP = 64 * CMPL, TM = 256 in the pair kernels); 0: any other supported
// shape (TP = TM = 0).  The one place where h, P and M become template arguments for the pair query, the run-aware query and the three
// one-vs-all scans; a kernel without a hop count (topk_scan_kernel) passes h = 1 and ignores H.
using PairShapes = std::make_integer_sequence<int, 5 * SS_MAX_HOPS>;
template <class Launch, int... I>
void dispatch_pair_shape(int h, int P, int M, Launch &&launch, std::integer_sequence<int, I...>)
{
    const int i = 5 * (h - 1) + (is_fast_pair_shape(P, M) ? P / 64 : 0);
    ((i == I ? launch(std::integral_constant<int, I / 5 + 1>{}, std::integral_constant<int, I % 5>{}) : void()), ...);
}

// Hop count, the caller's own size checks, HLL parameters, sketch width -- in the one order that decides which code comes back.
// `empty`: the entry points that answer an empty query with SS_OK before they look at P pass B == 0 (and return right after).
inline int check_pair_query_args(int h, bool sizes_ok, const ss_hll_params *prm, int P, bool empty)
{
    if (h < 1 || h > SS_MAX_HOPS) return SS_ERR_UNSUPPORTED;  // hashing.py:54, 308-309
    if (!sizes_ok) return SS_ERR_INVALID_ARG;
    const int rc = check_params(prm);
    if (rc != SS_OK) return rc;
    if (!empty && (P <= 0 || (P & 3) || P > 2048)) return SS_ERR_INVALID_ARG;
    return SS_OK;
}

}  // namespace ss
