// ss_topk_head.hip -- one-vs-all link candidates ranked by the structure head: for a block of sources and EVERY node v, the score
// ss_pair_scores gives the pair (u, v), written as the unique 64-bit ranking keys of ss_topk.hip (ElphHashes.topk_links).
//
// Serves what a trained ELPH / BUDDY model is asked at full ranking -- the k nodes it ranks highest for a source, its hard
// negatives, MRR / Hits@K over all nodes (reference models/elph.py:73-86, :324-352 on the rows of hashing.py:258-323) -- without
// the [S * N, 2] link list and the 2h gathered rows per pair of the composition score_links + torch.topk.
//
// Mapping (topk_scan_kernel's): one 16-lane DPP row per candidate v, lane l owning the 16-byte chunks l, l + 16, ... of a sketch
// row.  A workgroup (16 rows) stages a block of sources once -- ALL h hops of each: MinHash chunks, HLL digests, cards[u][0..h)
// and degrees[u] -- and every candidate row holds ITS h hops in registers (digests made once per candidate, cards[v] / degrees[v]
// loaded once per candidate) while it walks the staged sources.  Per (u, v) all h^2 (match, zeros, harmonic sum) statistics are
// accumulated with the helpers of ss_pair_math.hpp under the chunk ownership of pair_features_kernel (generic shapes: its own
// pair_stats_generic) and reduced with row16_sum_*, then the pair kernel's epilogue runs on the row through the functions it calls: lane
// c < h^2 estimates combination c (lane_select, intersection_estimate), the row assembles the features (assemble_features), lane i
// makes the degree-normalised copy of feature i (degree_normalised), head_score sums the head (DESIGN 3.11's orders).  Every operation
// and every order is the pair kernel's, so the score is bit-identical to ss_pair_scores' for the link (u, v).
// The key of source j of a group of 16 is parked in lane j and the group's keys leave in one store.
//
// Sources per workgroup (kernel parameter SB, topk_head_sources()): as many of {32, 16, 8} as leave TWO workgroups per CU
// (2 x 80 KiB of the 160 KiB LDS) next to the estimator and head tables -- a source costs 256 * CMPL + 576 bytes per hop.
// The budget behind it and the shared entry checks: ss_head_scan.hpp; the launch geometry: scan_grid (ss_topk_key.hpp); the (h, CMPL)
// dispatch: dispatch_pair_shape (ss_pair_math.hpp).  The kernel body is
// written out here and in ss_rank.hip: one source for both was measured and dropped (DESIGN_EXPERIMENTS 3.13).
#include "ss_feature_algebra.hpp"
#include "ss_head_scan.hpp"
#include "ss_pair_math.hpp"
#include "ss_topk_key.hpp"

extern "C" size_t ss_topk_workspace_bytes(int64_t N, int32_t S);

namespace ss {

// sources per workgroup: a source stages nothing of its own next to the entry of ss_head_scan.hpp
constexpr int topk_head_sources(int H, int CMPL) { return head_scan_entries(H, CMPL, 0); }

// CMPL > 0: fast shape (p = 8, P = 64 * CMPL); 0: any other supported shape (the sources' rows are read from global memory)
template <int H, int CMPL>
__global__ __launch_bounds__(256) void topk_score_scan_kernel(const int64_t *__restrict__ sources, int S, int64_t N, HopTables tabs,
                                                               int P_rt, int M, const float *__restrict__ cards, int64_t cards_stride,
                                                               ss_hll_params prm, uint32_t flags, const float *__restrict__ degrees,
                                                               HeadArgs head, int64_t *__restrict__ keys, int32_t *__restrict__ err)
{
    constexpr int SB = topk_head_sources(H, CMPL);
    constexpr int NF = H * (H + 2);
    constexpr int NC = H * H;
    constexpr int CM = CMPL > 0 ? CMPL * kRow : 1;  // staged MinHash chunks per source and hop
    constexpr int CH = CMPL > 0 ? kRow : 1;         // staged HLL chunks per source and hop (M = 256)
    constexpr int HS = CMPL > 0 ? H : 1;
    __shared__ EstimatorLds est_lds;
    __shared__ HeadLds head_lds;
    __shared__ u32x4 s_mh[SB][HS][CM];
    __shared__ u32x4 s_pe[SB][HS][CH], s_po[SB][HS][CH];
    __shared__ uint32_t s_zm[SB][HS][CH];
    __shared__ int64_t s_u[SB];  // wrapped source id, -1: none / out of range
    __shared__ float s_c1[SB][H];
    __shared__ float s_deg[SB];

    const int P = CMPL > 0 ? CMPL * 64 : P_rt;
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
#pragma unroll
        for (int k = 0; k < H; ++k) s_c1[threadIdx.x][k] = u >= 0 ? cards[u * cards_stride + k] : 0.0f;
        s_deg[threadIdx.x] = (u >= 0 && degrees) ? degrees[u] : 0.0f;
    }
    __syncthreads();
    if constexpr (CMPL > 0) {
        for (int i = threadIdx.x; i < SB * H * CM; i += blockDim.x) {
            const int s = i / (H * CM), k = (i / CM) % H, c = i % CM;
            const int64_t u = s_u[s];
            s_mh[s][k][c] = u >= 0 ? *reinterpret_cast<const u32x4 *>(tabs.mh[k] + u * (CMPL * 64) + 4 * c) : u32x4{0u, 0u, 0u, 0u};
        }
        for (int i = threadIdx.x; i < SB * H * CH; i += blockDim.x) {
            const int s = i / (H * CH), k = (i / CH) % H, c = i % CH;
            const int64_t u = s_u[s];
            const HllChunk d = digest_chunk(u >= 0 ? *reinterpret_cast<const u32x4 *>(tabs.hll[k] + u * 256 + 16 * c) : u32x4{0u, 0u, 0u, 0u});
            s_pe[s][k][c] = u32x4{d.pe[0], d.pe[1], d.pe[2], d.pe[3]};
            s_po[s][k][c] = u32x4{d.po[0], d.po[1], d.po[2], d.po[3]};
            s_zm[s][k][c] = d.zero_mask;
        }
    }
    stage_head(head_lds, head);                              // (no barrier of its own: the one inside stage_tables)
    const EstimatorTables est = stage_tables(est_lds, prm);  // (its barrier also publishes the staged rows)

    const int l = threadIdx.x & (kRow - 1);
    const int row_base = (threadIdx.x & (kWave - 1)) & ~(kRow - 1);
    const bool normalised = degrees != nullptr;
    const int64_t stride = (int64_t)gridDim.x * kTopkRows;
    // no barrier below: rows may run different numbers of candidates (the shuffles of the epilogue stay inside a row, whose lanes
    // share v)
    for (int64_t v = (int64_t)blockIdx.x * kTopkRows + threadIdx.x / kRow; v < N; v += stride) {
        u32x4 mv[HS][CMPL > 0 ? CMPL : 1];
        HllChunk hv[HS];
        if constexpr (CMPL > 0) {
#pragma unroll
            for (int k = 0; k < H; ++k) {
#pragma unroll
                for (int c = 0; c < CMPL; ++c) mv[k][c] = *reinterpret_cast<const u32x4 *>(tabs.mh[k] + v * (CMPL * 64) + 4 * (l + kRow * c));
            }
#pragma unroll
            for (int k = 0; k < H; ++k) hv[k] = digest_chunk(*reinterpret_cast<const u32x4 *>(tabs.hll[k] + v * 256 + 16 * l));
        }
        float c2[H];
#pragma unroll
        for (int k = 0; k < H; ++k) c2[k] = cards[v * cards_stride + k];
        const float deg_v = normalised ? degrees[v] : 0.0f;

        for (int g = 0; g < ns; g += kRow) {  // a group of 16 sources: the key of source g + j is parked in lane j
            int64_t my_key = kTopkSentinel;
            const int nj = ns - g < kRow ? ns - g : kRow;
            for (int j = 0; j < nj; ++j) {  // row-uniform
                const int s = g + j;
                const int64_t u = s_u[s];
                int mz[NC];    // (match << 20) | zeros, row total
                float hs[NC];  // harmonic sum, row total
                if constexpr (CMPL > 0) {
#pragma unroll
                    for (int k1 = 0; k1 < H; ++k1) {
                        const u32x4 pe = s_pe[s][k1][l], po = s_po[s][k1][l];
                        const HllChunk hu = {{pe.x, pe.y, pe.z, pe.w}, {po.x, po.y, po.z, po.w}, s_zm[s][k1][l]};
                        u32x4 mu[CMPL];
#pragma unroll
                        for (int c = 0; c < CMPL; ++c) mu[c] = s_mh[s][k1][l + kRow * c];
#pragma unroll
                        for (int k2 = 0; k2 < H; ++k2) {
                            int match = 0, zeros = 0;
                            float hsum = 0.0f;
#pragma unroll
                            for (int c = 0; c < CMPL; ++c) match += eq4(mu[c], mv[k2][c]);
                            union_stats_digested(hu, hv[k2], zeros, hsum);
                            mz[k1 * H + k2] = row16_sum_i((match << 20) | zeros);
                            hs[k1 * H + k2] = row16_sum_f(hsum);
                        }
                    }
                } else {
                    const int64_t ur = u < 0 ? 0 : u;  // (an invalid source's entries become the sentinel below)
#pragma unroll
                    for (int k1 = 0; k1 < H; ++k1)
#pragma unroll
                        for (int k2 = 0; k2 < H; ++k2)
                            pair_stats_generic(reinterpret_cast<const u32x4 *>(tabs.mh[k1] + ur * P), reinterpret_cast<const u32x4 *>(tabs.mh[k2] + v * P),
                                               reinterpret_cast<const u32x4 *>(tabs.hll[k1] + ur * M), reinterpret_cast<const u32x4 *>(tabs.hll[k2] + v * M),
                                               P >> 2, M >> 4, l, mz[k1 * H + k2], hs[k1 * H + k2]);
                }
                // from here on the epilogue of pair_features_kernel<..., HeadArgs>: its finish line for line, then the functions it calls
                // (written out, not a shared function: that moved the VGPRs at h >= 2 -- DESIGN_EXPERIMENTS "One source for the pair finish")
                const int my_mz = lane_select(mz, l);
                const float my_hs = lane_select(hs, l);
                float my_I = 0.0f;
                if (l < NC) my_I = intersection_estimate(est, (int)((uint32_t)my_mz >> 20), my_mz & 0xFFFFF, my_hs, P);
                float I[H][H];
#pragma unroll
                for (int c = 0; c < NC; ++c) I[c / H][c % H] = __shfl(my_I, row_base + c);
                float c1[H];
#pragma unroll
                for (int k = 0; k < H; ++k) c1[k] = s_c1[s][k];
                float f[NF];
                assemble_features<H>(I, c1, c2, flags, f);
                const float normed = normalised ? degree_normalised(lane_select(f, l), s_deg[s], deg_v) : 0.0f;
                const float score = head_score<NF>(head_lds, head.dim, head.bias, f, normed, normalised, l, row_base);
                const int64_t key = (u >= 0 && u != v) ? topk_key(score, v) : kTopkSentinel;
                my_key = l == j ? key : my_key;
            }
            if (l < nj) keys[(int64_t)(s0 + g + l) * N + v] = my_key;
        }
    }
}

}  // namespace ss

extern "C" int ss_topk_score_scan(const int64_t *sources, int32_t S, int64_t N, int32_t h, const uint32_t *const *mh, const uint8_t *const *hll,
                                  int32_t P, const float *cards, int64_t cards_stride, const ss_hll_params *prm, uint32_t flags,
                                  const float *degrees, const ss_structure_head *head, int64_t *keys, size_t keys_bytes, int32_t *err_flag,
                                  void *stream)
{
    using namespace ss;
    HeadArgs args;  // (N_end: the key's low word holds 0xFFFFFFFF - v)
    const int rc = check_head_scan_args(S, N, ((int64_t)1 << 32) - 1, sources && keys, h, mh, hll, P, cards, cards_stride, prm, degrees, head, args);
    if (rc != SS_OK || S == 0) return rc;
    if (keys_bytes < ss_topk_workspace_bytes(N, S)) return SS_ERR_WORKSPACE;
    HopTables tabs;
    if (!fill_head_scan_tables(mh, hll, h, S, tabs)) return SS_ERR_INVALID_ARG;
    const int M = 1 << prm->p;
    dispatch_pair_shape(h, P, M, [&](auto H, auto CMPL) {
        hipLaunchKernelGGL((topk_score_scan_kernel<H(), CMPL()>), scan_grid(S, topk_head_sources(H(), CMPL()), N), dim3(256), 0,
                           (hipStream_t)stream, sources, (int)S, N, tabs, (int)P, M, cards, cards_stride, *prm, flags, degrees, args, keys, err_flag);
    }, PairShapes{});
    SS_LAUNCH_CHECK();
    return SS_OK;
}
