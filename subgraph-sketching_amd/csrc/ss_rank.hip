// ss_rank.hip -- each link's exact rank among all nodes by the structure head: for a block of links (u, t) and EVERY node v, the score
// ss_pair_scores gives the pair (u, v), compared with the link's own score thr = s(u, t) and COUNTED -- how many candidates score
// strictly higher, how many tie (ElphHashes.rank_links).
//
// Serves what full-ranking evaluation asks of a trained ELPH / BUDDY model -- MRR / Hits@K of its positive links (reference
// src/evaluation.py, ogbl-citation2's MRR over sampled negatives) over all N nodes -- without the [L, N] ranking keys, the exclude
// pass over them and the selection of the one-vs-all top-k (ss_topk_head.hip), whose answer is the k best partners, not a rank.
//
// Mapping (topk_score_scan_kernel's): one 16-lane DPP row per candidate v, lane l owning the 16-byte chunks l, l + 16, ... of a
// sketch row.  A workgroup (16 rows) stages a block of links once -- ALL h hops of each source: MinHash chunks, HLL digests,
// cards[u][0..h) and degrees[u], and next to them the link's target t and threshold thr -- and every candidate row holds ITS h hops
// in registers while it walks the staged links.  Per (u, v) the statistics, the epilogue and the head are that kernel's, operation
// for operation and order for order, so the score is bit-identical to ss_pair_scores' for the link (u, v) -- and thr, which that
// entry point wrote, compares with it exactly.
// Counters instead of keys: for link g + j of a group of 16, lane j of the row keeps two int32 counters (> and ==), one pair per group
// of the staged block, in registers across the whole grid-stride loop over v.  After the loop the 16 rows of the workgroup add them
// up in LDS and the workgroup issues one 64-bit integer atomicAdd per link and counter: integer sums, so the result does not depend
// on the grid or the schedule.  The kernel stores nothing else.
//
// Links per workgroup (rank_queries()): as many of {32, 16, 8} as leave TWO workgroups per CU (2 x 80 KiB of the 160 KiB LDS) next
// to the estimator and head tables -- a link costs 256 * CMPL + 576 bytes per hop plus 32 + 4 h bytes of ids, sizes, threshold and sums.
// The budget behind it and the shared entry checks: ss_head_scan.hpp; the launch geometry: scan_grid (ss_topk_key.hpp); the (h, CMPL)
// dispatch: dispatch_pair_shape (ss_pair_math.hpp).  The kernel body is
// written out here and in ss_topk_head.hip: one source for both was measured and dropped (DESIGN_EXPERIMENTS 3.13).
#include "ss_feature_algebra.hpp"
#include "ss_head_scan.hpp"
#include "ss_pair_math.hpp"
#include "ss_topk_key.hpp"

namespace ss {

// links per workgroup: next to the entry of ss_head_scan.hpp a link stages its target id, its threshold and two sums
constexpr int rank_queries(int H, int CMPL) { return head_scan_entries(H, CMPL, 8 + 4 + 8); }

// CMPL > 0: fast shape (p = 8, P = 64 * CMPL); 0: any other supported shape (the sources' rows are read from global memory)
template <int H, int CMPL>
__global__ __launch_bounds__(256) void rank_score_scan_kernel(const int64_t *__restrict__ links, const float *__restrict__ thr, int L, int64_t N,
                                                               HopTables tabs, int P_rt, int M, const float *__restrict__ cards,
                                                               int64_t cards_stride, ss_hll_params prm, uint32_t flags,
                                                               const float *__restrict__ degrees, HeadArgs head,
                                                               unsigned long long *__restrict__ counts, int32_t *__restrict__ err)
{
    constexpr int QB = rank_queries(H, CMPL);
    constexpr int NG = (QB + kRow - 1) / kRow;  // groups of 16 links: one pair of counters each
    constexpr int NF = H * (H + 2);
    constexpr int NC = H * H;
    constexpr int CM = CMPL > 0 ? CMPL * kRow : 1;  // staged MinHash chunks per link and hop
    constexpr int CH = CMPL > 0 ? kRow : 1;         // staged HLL chunks per link and hop (M = 256)
    constexpr int HS = CMPL > 0 ? H : 1;
    __shared__ EstimatorLds est_lds;
    __shared__ HeadLds head_lds;
    __shared__ u32x4 s_mh[QB][HS][CM];
    __shared__ u32x4 s_pe[QB][HS][CH], s_po[QB][HS][CH];
    __shared__ uint32_t s_zm[QB][HS][CH];
    __shared__ int64_t s_u[QB];  // wrapped source id, -1: no link / an id of the link out of range
    __shared__ int64_t s_t[QB];  // wrapped target id, -1 with s_u
    __shared__ float s_thr[QB];
    __shared__ float s_c1[QB][H];
    __shared__ float s_deg[QB];
    __shared__ uint32_t s_cnt[QB][2];  // the workgroup's sums (> and ==): at most N - 1 each

    const int P = CMPL > 0 ? CMPL * 64 : P_rt;
    const int q0 = blockIdx.y * QB;
    const int nq = L - q0 < QB ? L - q0 : QB;
    if (threadIdx.x < QB) {
        int64_t u = -1, t = -1;
        float th = 0.0f;
        if ((int)threadIdx.x < nq) {
            u = links[2 * (int64_t)(q0 + threadIdx.x)];
            t = links[2 * (int64_t)(q0 + threadIdx.x) + 1];
            u = u < 0 ? u + N : u;  // torch-style negative indexing, as the pair query
            t = t < 0 ? t + N : t;
            if ((uint64_t)u >= (uint64_t)N || (uint64_t)t >= (uint64_t)N) {
                if (err) *err = 1;
                u = t = -1;
            } else {
                th = thr[q0 + threadIdx.x];
            }
        }
        s_u[threadIdx.x] = u;
        s_t[threadIdx.x] = t;
        s_thr[threadIdx.x] = th;
        s_cnt[threadIdx.x][0] = s_cnt[threadIdx.x][1] = 0u;
#pragma unroll
        for (int k = 0; k < H; ++k) s_c1[threadIdx.x][k] = u >= 0 ? cards[u * cards_stride + k] : 0.0f;
        s_deg[threadIdx.x] = (u >= 0 && degrees) ? degrees[u] : 0.0f;
    }
    __syncthreads();
    if constexpr (CMPL > 0) {
        for (int i = threadIdx.x; i < QB * H * CM; i += blockDim.x) {
            const int s = i / (H * CM), k = (i / CM) % H, c = i % CM;
            const int64_t u = s_u[s];
            s_mh[s][k][c] = u >= 0 ? *reinterpret_cast<const u32x4 *>(tabs.mh[k] + u * (CMPL * 64) + 4 * c) : u32x4{0u, 0u, 0u, 0u};
        }
        for (int i = threadIdx.x; i < QB * H * CH; i += blockDim.x) {
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
    int above[NG], tied[NG];  // lane j: link 16 * i + j of the staged block; a row meets at most N / 16 candidates
#pragma unroll
    for (int i = 0; i < NG; ++i) above[i] = tied[i] = 0;
    // no barrier inside the loop: rows may run different numbers of candidates (the shuffles of the epilogue stay inside a row, whose
    // lanes share v)
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

        for (int g = 0; g < nq; g += kRow) {  // a group of 16 links: what link g + j adds is parked in lane j
            int my_above = 0, my_tied = 0;
            const int nj = nq - g < kRow ? nq - g : kRow;
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
                    const int64_t ur = u < 0 ? 0 : u;  // (an invalid link adds nothing below)
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
                const float th = s_thr[s];
                const bool counted = u >= 0 && u != v && s_t[s] != v && l == j;
                my_above += (counted && score > th) ? 1 : 0;
                my_tied += (counted && score == th) ? 1 : 0;
            }
#pragma unroll
            for (int i = 0; i < NG; ++i) {  // (g is row-uniform: the counters stay in registers)
                above[i] += g == i * kRow ? my_above : 0;
                tied[i] += g == i * kRow ? my_tied : 0;
            }
        }
    }
    // the 16 rows of the workgroup add up in LDS (integer adds: any order), then one 64-bit add per link and counter leaves
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        if (i * kRow + l < nq) {
            atomicAdd(&s_cnt[i * kRow + l][0], (uint32_t)above[i]);
            atomicAdd(&s_cnt[i * kRow + l][1], (uint32_t)tied[i]);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * nq) {
        const uint32_t c = s_cnt[threadIdx.x >> 1][threadIdx.x & 1];
        if (c) atomicAdd(counts + 2 * (int64_t)q0 + threadIdx.x, (unsigned long long)c);
    }
}

}  // namespace ss

extern "C" int ss_rank_score_scan(const int64_t *links, const float *thr, int32_t L, int64_t N, int32_t h, const uint32_t *const *mh,
                                  const uint8_t *const *hll, int32_t P, const float *cards, int64_t cards_stride, const ss_hll_params *prm,
                                  uint32_t flags, const float *degrees, const ss_structure_head *head, int64_t *counts, int32_t *err_flag,
                                  void *stream)
{
    using namespace ss;
    HeadArgs args;  // (N_end: a workgroup's sums are 32-bit words)
    const int rc = check_head_scan_args(L, N, (int64_t)1 << 32, links && thr && counts, h, mh, hll, P, cards, cards_stride, prm, degrees, head, args);
    if (rc != SS_OK || L == 0) return rc;
    HopTables tabs;
    if (!fill_head_scan_tables(mh, hll, h, L, tabs)) return SS_ERR_INVALID_ARG;
    const int M = 1 << prm->p;
    dispatch_pair_shape(h, P, M, [&](auto H, auto CMPL) {
        hipLaunchKernelGGL((rank_score_scan_kernel<H(), CMPL()>), scan_grid(L, rank_queries(H(), CMPL()), N), dim3(256), 0,
                           (hipStream_t)stream, links, thr, (int)L, N, tabs, (int)P, M, cards, cards_stride, *prm, flags, degrees, args,
                           reinterpret_cast<unsigned long long *>(counts), err_flag);
    }, PairShapes{});
    SS_LAUNCH_CHECK();
    return SS_OK;
}
