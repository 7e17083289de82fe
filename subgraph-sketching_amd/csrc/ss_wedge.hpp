// ss_wedge.hpp -- the arithmetic of the two-hop expansion (ss_wedge.hip) that the host and the kernels must agree on:
// which tier serves a source, how large its LDS table is, where a node hashes to, and the argument checks of the entry points.
// Plain C++ behind __host__ __device__, so tools/wedge_host_check.hip can run it under the host sanitizers without a device.
#pragma once
#include "ss_common.hpp"

namespace ss {

constexpr int kWedgeMaxSlots = SS_WEDGE_MAX_SLOTS;  // (key, count) slots of the LDS table at most: 2 * 4 * 4096 = 32 KiB of the CU's 160
constexpr int kWedgeThreads = 256;
constexpr int64_t kWedgePad = INT64_MAX;            // the key of an unused place of a folded source's W(u)-sized slot
constexpr int kWedgeMaxSlices = 64;                 // workgroups a large-tier source may be spread over

__host__ __device__ inline bool is_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

// W = the walks of a source as the caller filtered them (0: skipped or none).  2 W <= slots: the table is never more than half full.
__host__ __device__ inline bool wedge_folds(int64_t W, int slots) { return W > 0 && 2 * W <= (int64_t)slots; }
__host__ __device__ inline bool wedge_emits(int64_t W, int slots) { return W > 0 && 2 * W > (int64_t)slots; }

// the table of a folded source: the smallest power of two >= 2 W (>= 2), so that clearing and reading it back cost what the source
// needs, not what the largest one does
__host__ __device__ inline int wedge_table_slots(int64_t W, int slots)
{
    int m = slots;
    while (m > 2 && (int64_t)(m >> 1) >= 2 * W) m >>= 1;
    return m;
}

// the first slot a node is tried at in a table of 2^k slots, 1 <= k <= 12: the high k bits of a Fibonacci multiply
__host__ __device__ inline int wedge_log2(int m)
{
    int k = 0;
    while ((1 << (k + 1)) <= m) ++k;
    return k;
}
__host__ __device__ inline int wedge_slot(int32_t v, int k) { return (int)(((uint32_t)v * 2654435761u) >> (32 - k)); }

inline int check_wedge_graph(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S)
{
    if (N < 0 || N >= ((int64_t)1 << 31) || S < 0 || S >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;  // (col is int32; grid.x)
    if (S == 0) return SS_OK;
    if (N == 0 || !rowptr || !col || !sources) return SS_ERR_INVALID_ARG;
    return SS_OK;
}

inline int check_wedge_expand(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S, const int64_t *walks,
                              const int64_t *offsets, int32_t slots, const int64_t *keys, const int32_t *counts)
{
    const int rc = check_wedge_graph(rowptr, col, N, sources, S);
    if (rc != SS_OK) return rc;
    if (!is_pow2(slots) || slots > kWedgeMaxSlots) return SS_ERR_INVALID_ARG;
    if (S == 0) return SS_OK;
    if (!walks || !offsets || !keys || !counts) return SS_ERR_INVALID_ARG;
    return SS_OK;
}

}  // namespace ss
