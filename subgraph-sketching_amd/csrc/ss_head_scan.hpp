// ss_head_scan.hpp -- the host half of the two one-vs-all scans by the structure head, topk_score_scan_kernel (ss_topk_head.hip) and
// rank_score_scan_kernel (ss_rank.hip): the LDS budget of a staged entry (a source / a link) and the checks both entry points make.
// Their launch geometry (scan_grid, ss_topk_key.hpp) and their (h, CMPL) dispatch (dispatch_pair_shape, ss_pair_math.hpp) are the ones
// topk_scan_kernel and the pair query use.  The DEVICE body -- staging, candidate rows, the score of (u, v) -- stays written
// out in each kernel: as one source it kept scratch and LDS in all 30 instantiations and lowered the VGPRs of 29, but at <1, 0> that
// moved both kernels from 7 to 8 waves per SIMD, and the rule was "equal" (DESIGN_EXPERIMENTS 3.13).
#pragma once
#include "ss_head.hpp"
#include "ss_pair_math.hpp"
#include "ss_topk_key.hpp"

namespace ss {

constexpr int kHeadScanLds = 80 * 1024;  // LDS a workgroup may take: two per CU

// bytes of LDS per staged entry: its id, cards, degree, the `extra` bytes of the kernel's own and, on the fast shapes (CMPL > 0),
// h rows of MinHash chunks and HLL digests
constexpr int head_scan_entry_bytes(int H, int CMPL, int extra)
{
    return 8 + 4 * H + 4 + extra + (CMPL > 0 ? H * (CMPL * kRow * 16 + kRow * (16 + 16 + 4)) : 0);
}

// entries per workgroup: as many of {32, 16, 8} as leave TWO workgroups per CU next to the estimator and head tables
constexpr int head_scan_entries(int H, int CMPL, int extra)
{
    const int fixed = (int)sizeof(EstimatorLds) + (int)sizeof(HeadLds) + 64;  // (64: alignment between the arrays)
    for (int sb = 32; sb > 8; sb >>= 1)
        if (fixed + sb * head_scan_entry_bytes(H, CMPL, extra) <= kHeadScanLds) return sb;
    return 8;  // (8 .. 32 either way: threads 0 .. 2 * entries - 1 of a workgroup stage the entries and hand their sums over)
}

// The checks both entry points make, in their order, up to the head.  n == 0 answers SS_OK before the pointers are looked at: the
// caller returns when rc != SS_OK || n == 0.  N_end: the first N the kernel cannot take; own: the entry point's own pointers are there.
inline int check_head_scan_args(int32_t n, int64_t N, int64_t N_end, bool own, int32_t h, const uint32_t *const *mh, const uint8_t *const *hll,
                                int32_t P, const float *cards, int64_t cards_stride, const ss_hll_params *prm, const float *degrees,
                                const ss_structure_head *head, HeadArgs &args)
{
    const int rc = check_pair_query_args(h, true, prm, P, false);
    if (rc != SS_OK) return rc;
    if (n < 0 || N <= 0 || N >= N_end) return SS_ERR_INVALID_ARG;
    if (n == 0) return SS_OK;
    if (!own || !mh || !hll || !cards || cards_stride < h) return SS_ERR_INVALID_ARG;
    return make_head_args(head, h, degrees, args) ? SS_OK : SS_ERR_INVALID_ARG;
}

// ... and the two behind it: the hop tables, and grid.y at the smallest block of entries
inline bool fill_head_scan_tables(const uint32_t *const *mh, const uint8_t *const *hll, int h, int32_t n, HopTables &tabs)
{
    return fill_hop_tables(mh, hll, h, tabs) && ((int64_t)n + 7) / 8 <= 65535;
}

}  // namespace ss
