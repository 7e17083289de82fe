// ss_cn_pool.hip -- the common neighbours of node pairs as lists, and the node features of those neighbours pooled per pair:
//     members(u, v) = the columns stored in both row u and row v of A (structural: a stored zero is a member)
//     c(u, v, w)    = float32( A[u, w] * (A[v, w] * mult[w]) )      fp64 with this association, ONE rounding -- coefficient()
//                     of csrc/ss_pair_rows.hpp, the term the fp64 scores add up, for every matrix dtype
//     pool(u, v)    = sum over the members w, ASCENDING, of c(u, v, w) * x[w, :]      fp32, from +0.0, product and sum rounded
//                     separately (-ffp-contract=off), every output element accumulated by ONE lane
// A is a CSR with sorted, duplicate-free column ids.  One unit of lanes per pair: the lanes stride over the SHORTER row in chunks
// of one entry per lane and binary-search the longer one; a ballot over the chunk puts the hits in ascending column order (the
// shorter row is sorted), so neither the list nor the sum needs a sort, and a member's rank inside the pair is the running
// popcount plus the prefix inside the ballot.  Three kernels on that step (pair_rows, member, unit_ballot: csrc/ss_pair_rows.hpp):
//   count  16 lanes per pair, the membership step alone
//   fill   16 lanes per pair, ids[offsets[q] + rank] = w and, when asked for, coef[...] = c
//   pool   U = 16 | 32 | 64 lanes per pair, chosen from F as ss_spmm chooses lanes_per_row (F = 128 -> 32 lanes, two pairs per
//          wavefront).  After each chunk's ballot the hits are taken in order, (w, c) broadcast to the unit, and every lane adds
//          its own float4 of x[w]; the rows of four hits are requested before the first is used, the adds stay in hit order.
//          Columns beyond one pass of the unit (F > 4 U) go in further passes that walk the hits again.  HBM-bound gather of
//          4 F-byte rows, no MFMA, no LDS, no atomics.  A pair whose shorter row is long is walked chunk after chunk by its one
//          unit: slow, never wrong.
// A pair's row has ONE value: it does not depend on the grid, the unit size, the batch or which row was the shorter one.
#include "ss_pair_rows.hpp"
#include "ss_walks.hpp"

namespace ss {

__host__ __device__ constexpr int pieces_of(int F) { return (F >> 2) + ((F & 3) ? 1 : 0); }  // four-column pieces of a feature row

// FILL: the fill pass (ids and, when coef is non-null, the coefficients); otherwise the count pass
template <bool FILL>
__global__ __launch_bounds__(256) void cn_list_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      const double *__restrict__ val, const double *__restrict__ mult, int64_t N,
                                                      const int64_t *__restrict__ links, int64_t B, int64_t *__restrict__ counts,
                                                      const int64_t *__restrict__ offsets, int64_t *__restrict__ ids,
                                                      float *__restrict__ coef, int32_t *__restrict__ err_flag)
{
    int l;
    int64_t q;
    if (!group_pair(B, l, q)) return;
    const int base = (threadIdx.x & (kWave - 1)) - l;
    const int64_t u = links[2 * q], v = links[2 * q + 1];
    if (!ids_in_range(u, v, N)) {
        if (l == 0) {
            if (!FILL) counts[q] = 0;
            if (err_flag) *err_flag = 1;
        }
        return;
    }
    const PairRows r = pair_rows(rowptr, u, v);
    const int64_t first = FILL ? offsets[q] : 0;
    int rank = 0;
    for (int i0 = 0; i0 < r.ds; i0 += kPairLanes) {
        const int i = i0 + l;
        Member m = {};
        const bool hit = i < r.ds && member(col, r, i, m);
        const uint32_t mask = (uint32_t)unit_ballot(hit, base, kPairLanes);
        if (FILL && hit) {
            const int64_t at = first + rank + __popc(mask & ((1u << l) - 1u));
            ids[at] = m.w;
            if (coef) coef[at] = coefficient(val, mult, r, m);
        }
        rank += __popc(mask);
    }
    if (!FILL && l == 0) counts[q] = rank;
}

// one lane's four columns of a feature row: a float4 when VEC (F % 4 == 0 and both arrays 16-byte aligned), else column by column
// with the columns past F left out
template <bool VEC>
__device__ __forceinline__ float4 load_cols(const float *__restrict__ row, int c, int F)
{
    if (VEC) return *reinterpret_cast<const float4 *>(row + 4 * c);
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int j = 4 * c;
    r.x = row[j];
    if (j + 1 < F) r.y = row[j + 1];
    if (j + 2 < F) r.z = row[j + 2];
    if (j + 3 < F) r.w = row[j + 3];
    return r;
}

template <bool VEC>
__device__ __forceinline__ void store_cols(float *__restrict__ row, int c, int F, float4 a)
{
    if (VEC) {
        *reinterpret_cast<float4 *>(row + 4 * c) = a;
        return;
    }
    const int j = 4 * c;
    row[j] = a.x;
    if (j + 1 < F) row[j + 1] = a.y;
    if (j + 2 < F) row[j + 2] = a.z;
    if (j + 3 < F) row[j + 3] = a.w;
}

template <bool VEC>
__global__ __launch_bounds__(256) void cn_pool_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      const double *__restrict__ val, const double *__restrict__ mult, int64_t N,
                                                      const int64_t *__restrict__ links, int64_t B, const float *__restrict__ x, int F,
                                                      float *__restrict__ out, int32_t *__restrict__ err_flag, int U)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int cl = lane & (U - 1), base = lane - cl;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t q = wave * (kWave / U) + lane / U;
    if (q >= B) return;
    const int CF = pieces_of(F);  // four-column pieces per row, the last one short when F % 4 != 0
    float *__restrict__ orow = out + q * (int64_t)F;
    const int64_t u = links[2 * q], v = links[2 * q + 1];
    if (!ids_in_range(u, v, N)) {
        for (int c = cl; c < CF; c += U) store_cols<VEC>(orow, c, F, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        if (cl == 0 && err_flag) *err_flag = 1;
        return;
    }
    const PairRows r = pair_rows(rowptr, u, v);
    for (int cbase = 0; cbase < CF; cbase += U) {  // (one pass unless F > 4 U = 256)
        const int c = cbase + cl;
        const bool mine = c < CF;  // lanes past the last piece still search and shuffle: the unit needs every lane
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int i0 = 0; i0 < r.ds; i0 += U) {
            const int i = i0 + cl;
            Member m = {};
            const bool hit = i < r.ds && member(col, r, i, m);
            const float cf = hit ? coefficient(val, mult, r, m) : 0.0f;
            uint64_t mask = unit_ballot(hit, base, U);
            while (mask) {  // (uniform inside the unit) four hits at a time: their rows are requested before the first is used
                float4 rw[4];
                float ck[4];
                int n = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool take = mask != 0;
                    const int src = base + (take ? __ffsll((unsigned long long)mask) - 1 : 0);
                    mask &= mask - 1;  // (0 stays 0)
                    const int32_t wk = __shfl(m.w, src);
                    ck[k] = __shfl(cf, src);
                    n += take ? 1 : 0;
                    rw[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (take && mine) rw[k] = load_cols<VEC>(x + (int64_t)wk * F, c, F);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) {  // the adds stay in hit order
                        acc.x += ck[k] * rw[k].x;
                        acc.y += ck[k] * rw[k].y;
                        acc.z += ck[k] * rw[k].z;
                        acc.w += ck[k] * rw[k].w;
                    }
            }
        }
        if (mine) store_cols<VEC>(orow, c, F, acc);
    }
}

}  // namespace ss

extern "C" int ss_common_neighbour_count(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *links, int64_t B,
                                         int64_t *counts, int32_t *err_flag, void *stream)
{
    return ss::launch_pairs(ss::cn_list_kernel<false>, ss::kPairLanes, N, B, rowptr && col && links && counts, stream, rowptr, col,
                            (const double *)nullptr, (const double *)nullptr, N, links, B, counts, (const int64_t *)nullptr,
                            (int64_t *)nullptr, (float *)nullptr, err_flag);
}

extern "C" int ss_common_neighbour_fill(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult, int64_t N,
                                        const int64_t *links, int64_t B, const int64_t *offsets, int64_t *ids, float *coef,
                                        int32_t *err_flag, void *stream)
{
    return ss::launch_pairs(ss::cn_list_kernel<true>, ss::kPairLanes, N, B, rowptr && col && links && offsets && ids, stream, rowptr, col,
                            val, mult, N, links, B, (int64_t *)nullptr, offsets, ids, coef, err_flag);
}

extern "C" int ss_common_neighbour_pool(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult, int64_t N,
                                        const int64_t *links, int64_t B, const float *x, int32_t F, float *out, int32_t *err_flag,
                                        void *stream)
{
    using namespace ss;
    if (F < 0) return SS_ERR_INVALID_ARG;
    int U = pow2_ceil(pieces_of(F));  // the unit: lanes per pair, so 256 / U pairs per block
    U = U < kPairLanes ? kPairLanes : (U > kWave ? kWave : U);
    const bool vec = (F & 3) == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    return launch_pairs(vec ? cn_pool_kernel<true> : cn_pool_kernel<false>, U, N, B, rowptr && col && links && (F == 0 || (x && out)),
                        stream, rowptr, col, val, mult, N, links, B, x, (int)F, out, err_flag, U);
}
