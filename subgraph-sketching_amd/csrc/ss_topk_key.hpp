// ss_topk_key.hpp -- the ranking key of the one-vs-all scans (ss_topk.hip: one intersection estimate; ss_topk_head.hip: the structure
// head's score; ss_rank.hip counts instead of keys) and the launch constants and the grid they share.
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

// the grid of a one-vs-all scan (topk_scan_kernel, topk_score_scan_kernel, rank_score_scan_kernel): grid.y blocks of `per_block`
// staged entries, grid.x workgroups of candidates so that a launch aims at kTopkGrid workgroups (the caller has checked grid.y <= 65535).
// It lives here, not beside dispatch_pair_shape in ss_pair_math.hpp: it is made of the two constants above, which the pair and masked
// queries -- the other users of that header -- have no use for, and the three scan units all include this file.
inline dim3 scan_grid(int64_t n, int per_block, int64_t N)
{
    const int64_t blocks_y = (n + per_block - 1) / per_block;
    int64_t blocks_x = (kTopkGrid + blocks_y - 1) / blocks_y;
    const int64_t need_x = (N + kTopkRows - 1) / kTopkRows;
    if (blocks_x > need_x) blocks_x = need_x;
    return dim3((unsigned)blocks_x, (unsigned)blocks_y);
}

__device__ __forceinline__ int64_t topk_key(float score, int64_t v)
{
    uint32_t b = __float_as_uint(score);
    if (b == 0x80000000u) b = 0u;                                     // -0 ranks (and decodes) as +0
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // unsigned order == float order
    const uint64_t hi = (uint64_t)(m ^ 0x80000000u);                  // signed order == float order
    return (int64_t)((hi << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)v));
}

}  // namespace ss
