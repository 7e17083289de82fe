// ss_topk.hip -- one-vs-all link candidates: the intersection estimate I[k1, k2] of a block of sources against EVERY node,
// written as unique 64-bit ranking keys that torch.topk then selects from (ElphHashes.topk_candidates).
//
// Serves what the reference's sample_hard_negatives (src/data.py:262-304, never finished) set out to do -- rank the non-edges of a
// source by shared neighbourhood -- with the score of hashing.py:167-189.  The pair query (ss_pairs.hip) gathers 2h rows per pair
// and is HBM-bound; here the sources' rows are staged once per workgroup and every candidate row is streamed once per block of
// sources, so the scan is bound by its VALU work per pair instead.
//
// Mapping (the pair query's): one 16-lane DPP row per candidate v, lane l owning the 16-byte chunks l, l + 16, ... of a row.
// A workgroup (16 rows) stages kTopkSources sources; each row holds its candidate's hop-k2 chunks in registers and walks the staged
// sources.  Per (u, v) the statistics are accumulated per lane with the helpers of ss_pair_math.hpp and reduced with row16_sum_*,
// as pair_features_kernel does for that sketch shape (the generic shapes through pair_stats_generic, the function it calls): the fast shapes (p = 8, P in {64, 128, 192, 256}) compare digested
// HLL chunks (the candidate's digest made once per candidate, the sources' once per workgroup, kept in LDS), every other shape
// takes the generic byte-wise union, reading the sources' rows from global memory (cache-resident: every row of the workgroup
// reads them).  The harmonic sums therefore add the same terms in the same order and the estimate is bit-identical to the
// query's dbg_inter.  Lane j of a row then finishes source j of each group of 16: estimator, key, store.
//
// Key (ss_topk_key.hpp, shared with the scan that ranks by the structure head, ss_topk_head.hip): signed int64 order == (score
// descending, id ascending); ineligible entries (v == u, an out-of-range source, excluded edges) hold kTopkSentinel.
#include "ss_pair_math.hpp"
#include "ss_topk_key.hpp"

namespace ss {

constexpr int kTopkSources = 32;            // sources staged per workgroup

struct TopkTables {
    const uint32_t *mh_u;   // hop-k1 rows (sources)
    const uint8_t *hll_u;
    const uint32_t *mh_v;   // hop-k2 rows (candidates)
    const uint8_t *hll_v;
};

// CMPL > 0: fast shape (p = 8, P = 64 * CMPL); 0: any other supported shape
template <int CMPL>
__global__ __launch_bounds__(256) void topk_scan_kernel(const int64_t *__restrict__ sources, int S, int64_t N, TopkTables tabs,
                                                         int P, int M, ss_hll_params prm, int64_t *__restrict__ keys,
                                                         int32_t *__restrict__ err)
{
    constexpr int SB = kTopkSources;
    constexpr int CM = CMPL > 0 ? CMPL * kRow : 1;  // staged MinHash chunks per source
    constexpr int CH = CMPL > 0 ? kRow : 1;         // staged HLL chunks per source (M = 256)
    __shared__ EstimatorLds est_lds;
    __shared__ u32x4 s_mh[SB][CM];
    __shared__ u32x4 s_pe[SB][CH], s_po[SB][CH];
    __shared__ uint32_t s_zm[SB][CH];
    __shared__ int64_t s_u[SB];  // wrapped source id, -1: none / out of range

    const int s0 = blockIdx.y * SB;
    const int ns = S - s0 < SB ? S - s0 : SB;
    if (threadIdx.x < SB) {
        int64_t u = -1;
        if ((int)threadIdx.x < ns) {
            u = sources[s0 + threadIdx.x];
            u = u < 0 ? u + N : u;  // torch-style negative indexing, as the pair query
            if ((uint64_t)u >= (uint64_t)N) {
                if (err) *err = 1;
                u = -1;
            }
        }
        s_u[threadIdx.x] = u;
    }
    __syncthreads();
    if constexpr (CMPL > 0) {
        for (int i = threadIdx.x; i < SB * CM; i += blockDim.x) {
            const int s = i / CM, c = i % CM;
            const int64_t u = s_u[s];
            s_mh[s][c] = u >= 0 ? *reinterpret_cast<const u32x4 *>(tabs.mh_u + u * (CMPL * 64) + 4 * c) : u32x4{0u, 0u, 0u, 0u};
        }
        for (int i = threadIdx.x; i < SB * CH; i += blockDim.x) {
            const int s = i / CH, c = i % CH;
            const int64_t u = s_u[s];
            const HllChunk d = digest_chunk(u >= 0 ? *reinterpret_cast<const u32x4 *>(tabs.hll_u + u * 256 + 16 * c) : u32x4{0u, 0u, 0u, 0u});
            s_pe[s][c] = u32x4{d.pe[0], d.pe[1], d.pe[2], d.pe[3]};
            s_po[s][c] = u32x4{d.po[0], d.po[1], d.po[2], d.po[3]};
            s_zm[s][c] = d.zero_mask;
        }
    }
    const EstimatorTables est = stage_tables(est_lds, prm);  // (its barrier also publishes the staged rows)

    const int l = threadIdx.x & (kRow - 1);
    const int64_t stride = (int64_t)gridDim.x * kTopkRows;
    // no barrier below: rows may run different numbers of candidates
    for (int64_t v = (int64_t)blockIdx.x * kTopkRows + threadIdx.x / kRow; v < N; v += stride) {
        u32x4 mv[CMPL > 0 ? CMPL : 1];
        HllChunk hv;
        if constexpr (CMPL > 0) {
#pragma unroll
            for (int c = 0; c < CMPL; ++c) mv[c] = *reinterpret_cast<const u32x4 *>(tabs.mh_v + v * (CMPL * 64) + 4 * (l + kRow * c));
            hv = digest_chunk(*reinterpret_cast<const u32x4 *>(tabs.hll_v + v * 256 + 16 * l));
        }
        for (int g = 0; g < ns; g += kRow) {  // a group of 16 sources: lane j finishes source g + j
            int my_mz = 0;
            float my_hs = 0.0f;
            const int nj = ns - g < kRow ? ns - g : kRow;
            for (int j = 0; j < nj; ++j) {  // row-uniform
                const int s = g + j;
                int mz;
                float hs;
                if constexpr (CMPL > 0) {
                    int match = 0, zeros = 0;
                    float hsum = 0.0f;
#pragma unroll
                    for (int c = 0; c < CMPL; ++c) match += eq4(s_mh[s][l + kRow * c], mv[c]);
                    const u32x4 pe = s_pe[s][l], po = s_po[s][l];
                    const HllChunk hu = {{pe.x, pe.y, pe.z, pe.w}, {po.x, po.y, po.z, po.w}, s_zm[s][l]};
                    union_stats_digested(hu, hv, zeros, hsum);
                    mz = row16_sum_i((match << 20) | zeros);
                    hs = row16_sum_f(hsum);
                } else {
                    const int64_t u = s_u[s] < 0 ? 0 : s_u[s];  // (an invalid source's entries become the sentinel below)
                    pair_stats_generic(reinterpret_cast<const u32x4 *>(tabs.mh_u + u * P), reinterpret_cast<const u32x4 *>(tabs.mh_v + v * P),
                                       reinterpret_cast<const u32x4 *>(tabs.hll_u + u * M), reinterpret_cast<const u32x4 *>(tabs.hll_v + v * M),
                                       P >> 2, M >> 4, l, mz, hs);
                }
                my_mz = l == j ? mz : my_mz;
                my_hs = l == j ? hs : my_hs;
            }
            if (l < nj) {
                const int s = g + l;
                const int64_t u = s_u[s];
                int64_t key = kTopkSentinel;
                if (u >= 0 && u != v)
                    key = topk_key(intersection_estimate(est, (int)((uint32_t)my_mz >> 20), my_mz & 0xFFFFF, my_hs, P), v);
                keys[(int64_t)(s0 + s) * N + v] = key;
            }
        }
    }
}

// one wavefront per source: the sentinel over every v with an edge u -> v (row u of the CSR of the flipped exclude list)
__global__ __launch_bounds__(256) void topk_exclude_kernel(const int64_t *__restrict__ sources, int S, int64_t N,
                                                            const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            int64_t *__restrict__ keys)
{
    const int s = blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (s >= S) return;
    int64_t u = sources[s];
    u = u < 0 ? u + N : u;
    if ((uint64_t)u >= (uint64_t)N) return;  // (reported by the scan; its row is all sentinels)
    const int64_t e1 = rowptr[u + 1];
    for (int64_t e = rowptr[u] + (threadIdx.x & (kWave - 1)); e < e1; e += kWave) {
        const int32_t v = col[e];
        if (v >= 0 && v < N) keys[(int64_t)s * N + v] = kTopkSentinel;
    }
}

}  // namespace ss

extern "C" size_t ss_topk_workspace_bytes(int64_t N, int32_t S)
{
    if (N <= 0 || S < 0 || N >= ((int64_t)1 << 32) - 1) return 0;
    const unsigned __int128 b = (unsigned __int128)N * (unsigned __int128)S * 8u;
    return b > (unsigned __int128)SIZE_MAX ? 0 : (size_t)b;
}

extern "C" int ss_topk_scan(const int64_t *sources, int32_t S, int64_t N, const uint32_t *mh_src, const uint8_t *hll_src,
                            const uint32_t *mh_cand, const uint8_t *hll_cand, int32_t P, const ss_hll_params *prm, int64_t *keys,
                            size_t keys_bytes, int32_t *err_flag, void *stream)
{
    using namespace ss;
    const int rc = check_pair_query_args(/*h=*/1, true, prm, P, false);  // (one hop pair: no hop count of its own)
    if (rc != SS_OK) return rc;
    if (S < 0 || N <= 0 || N >= ((int64_t)1 << 32) - 1) return SS_ERR_INVALID_ARG;  // (the key's low word holds 0xFFFFFFFF - v)
    if (S == 0) return SS_OK;
    if (!sources || !mh_src || !hll_src || !mh_cand || !hll_cand || !keys) return SS_ERR_INVALID_ARG;
    if (keys_bytes < ss_topk_workspace_bytes(N, S)) return SS_ERR_WORKSPACE;
    const int M = 1 << prm->p;
    const TopkTables tabs = {mh_src, hll_src, mh_cand, hll_cand};
    if (((int64_t)S + kTopkSources - 1) / kTopkSources > 65535) return SS_ERR_INVALID_ARG;  // grid.y
    dispatch_pair_shape(/*h=*/1, P, M, [&](auto, auto CMPL) {
        hipLaunchKernelGGL(topk_scan_kernel<CMPL()>, scan_grid(S, kTopkSources, N), dim3(256), 0, (hipStream_t)stream, sources, (int)S, N, tabs,
                           (int)P, M, *prm, keys, err_flag);
    }, PairShapes{});
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_topk_exclude(const int64_t *sources, int32_t S, int64_t N, const int64_t *rowptr, const int32_t *col, int64_t *keys,
                               size_t keys_bytes, void *stream)
{
    using namespace ss;
    if (S < 0 || N <= 0 || N >= ((int64_t)1 << 32) - 1) return SS_ERR_INVALID_ARG;
    if (S == 0) return SS_OK;
    if (!sources || !rowptr || !col || !keys) return SS_ERR_INVALID_ARG;
    if (keys_bytes < ss_topk_workspace_bytes(N, S)) return SS_ERR_WORKSPACE;
    const int per_block = 256 / kWave;
    hipLaunchKernelGGL(topk_exclude_kernel, dim3((unsigned)((S + per_block - 1) / per_block)), dim3(256), 0, (hipStream_t)stream, sources,
                       (int)S, N, rowptr, col, keys);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
