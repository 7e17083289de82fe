// ss_topk_key.hpp -- the ranking key of the one-vs-all scans (ss_topk.hip: one intersection estimate; ss_topk_head.hip: the structure
// head's score) and the launch constants they share.
//
// Key: high word = the score's bits made monotone (signed int32 order == float order, -0 folded into +0), low word = 0xFFFFFFFF - v:
// signed int64 order == (score descending, id ascending).  Ineligible entries (v == u, an out-of-range source, excluded edges)
// hold kTopkSentinel, below every real key.
#pragma once
#include "ss_common.hpp"

namespace ss {

constexpr int kTopkRows = 256 / kRow;       // candidates in flight per workgroup
constexpr int kTopkGrid = 4096;             // workgroups a scan launch aims for (all blocks of sources together)
constexpr int64_t kTopkSentinel = INT64_MIN;

__device__ __forceinline__ int64_t topk_key(float score, int64_t v)
{
    uint32_t b = __float_as_uint(score);
    if (b == 0x80000000u) b = 0u;                                     // -0 ranks (and decodes) as +0
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // unsigned order == float order
    const uint64_t hi = (uint64_t)(m ^ 0x80000000u);                  // signed order == float order
    return (int64_t)((hi << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)v));
}

}  // namespace ss
