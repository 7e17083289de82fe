// ss_pair_math.hpp -- the per-pair arithmetic of the set-intersection estimate I[k1, k2] = J * U (reference hashing.py:167-189),
// shared by the pair query (ss_pairs.hip) and the one-vs-all scan (ss_topk.hip).  Both kernels give lane l of a 16-lane row the
// chunks l, l + 16, ... of a sketch row, accumulate a pair's statistics per lane with these helpers in chunk order, and reduce
// them with row16_sum_i / row16_sum_f: that is what makes their fp32 harmonic sums -- and so their estimates -- bit-identical.
#pragma once
#include "ss_common.hpp"

namespace ss {

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

}  // namespace ss
