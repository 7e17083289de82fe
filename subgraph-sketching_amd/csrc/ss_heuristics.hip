// ss_heuristics.hip -- weighted common-neighbour scores of node pairs: the per-link precompute next to the sketches in
// HashDataset.__init__ (reference datasets/elph.py:76-77,314 -> heuristics.py:10-70: CN, AA and RA are the same sum
//     score(u, v) = sum_w A[u, w] * (A[v, w] * mult[w])        mult = 1 | 1/log(colsum) | 1/colsum
// over the columns both rows hold).  A is a CSR with sorted, duplicate-free column ids (what scipy hands the reference).
// 16 lanes per pair, 4 pairs per wavefront: the lanes stride over the SHORTER row and binary-search the longer one, so a
// pair costs deg_short/16 * log2(deg_long) probes.  HBM-bound gather of two short rows per pair.  Two arithmetic modes,
// chosen by the matrix's dtype:
//   fp64 (int, bool and float64 matrices; common_neighbour_kernel): fp64 products with the reference's association, summed
//     in fp64 in lane order, one fp32 rounding at the end.  scipy sums these matrices in int64 / fp64 and torch.FloatTensor
//     casts, so CN of integer weights is exact and the rest is within one float32 ulp.
//   fp32 (float32 matrices; common_neighbour_f32_kernel): scipy works in float32 throughout.  Each term is
//     f32(a_src * a_dst) (CN) or f32(a_src * f32(a_dst * mult)) (AA / RA), terms equal to 0 are dropped (scipy's
//     element-wise product does not store them), and CSR row sum = np.add.reduceat adds the m terms of a row, in ascending
//     column order, as t[0] + pairwise(t[1:]) -- numpy's float32 pairwise sum: fewer than 8 terms in order; up to 128 in 8
//     strided accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the rest in order; above 128 split at n/2
//     rounded down to a multiple of 8 and both halves summed so.  The kernel reproduces that order bit for bit: a ballot
//     over the 16 lanes puts the matches of each 16-column chunk in rank order, and the group replays numpy's recursion as
//     a stream (the leaves are contiguous runs of at most 128 terms, met left to right).
#include "ss_common.hpp"

namespace ss {

constexpr int kPairLanes = 16;

__device__ inline double row16_sum_d(double x)
{
    for (int off = 1; off < kPairLanes; off <<= 1) x += __shfl_xor(x, off);
    return x;
}

__global__ __launch_bounds__(256) void common_neighbour_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                               const double *__restrict__ val, const double *__restrict__ mult,
                                                               int64_t N, const int64_t *__restrict__ links, int64_t B,
                                                               float *__restrict__ out, int32_t *__restrict__ err_flag)
{
    const int l = threadIdx.x & (kPairLanes - 1);
    const int64_t q = (int64_t)blockIdx.x * (blockDim.x / kPairLanes) + threadIdx.x / kPairLanes;
    if (q >= B) return;
    const int64_t u = links[2 * q], v = links[2 * q + 1];
    if (u < 0 || u >= N || v < 0 || v >= N) {
        if (l == 0) {
            out[q] = 0.0f;
            if (err_flag) *err_flag = 1;
        }
        return;
    }
    const int64_t ub = rowptr[u], vb = rowptr[v];
    const int du = (int)(rowptr[u + 1] - ub), dv = (int)(rowptr[v + 1] - vb);
    // walk the shorter row, search the longer one; `swapped` keeps the roles of the reference's product:
    // term = A[src, w] * (A[dst, w] * mult[w])
    const bool swapped = du > dv;
    const int64_t sb = swapped ? vb : ub, lb = swapped ? ub : vb;
    const int ds = swapped ? dv : du, dl = swapped ? du : dv;
    double acc = 0.0;
    for (int i = l; i < ds; i += kPairLanes) {
        const int32_t w = col[sb + i];
        int lo = 0, hi = dl;  // first position in the long row with col >= w
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (col[lb + mid] < w) lo = mid + 1;
            else hi = mid;
        }
        if (lo < dl && col[lb + lo] == w) {
            const double a_short = val ? val[sb + i] : 1.0, a_long = val ? val[lb + lo] : 1.0;
            const double a_src = swapped ? a_long : a_short, a_dst = swapped ? a_short : a_long;
            acc += a_src * (mult ? a_dst * mult[w] : a_dst);
        }
    }
    acc = row16_sum_d(acc);
    if (l == 0) out[q] = (float)acc;
}


// ---- fp32 mode ---------------------------------------------------------------------------------------------------------------
// Control flow is uniform inside a 16-lane group (every value below except `r` and the stack slots is the same in all 16
// lanes), so ballots and width-16 shuffles see the whole group.

__device__ inline uint32_t group_ballot(bool pred)  // this group's 16 bits of the wavefront ballot
{
    return (uint32_t)(__ballot(pred) >> (threadIdx.x & 48)) & 0xFFFFu;
}

// numpy's float32 pairwise sum of s[0..n) fed one term at a time, in order.  A node of more than 128 terms splits at
// n2 = n/2 - (n/2) % 8; the leaves (<= 128 terms) are met left to right, so only the pending left halves need keeping: a
// stack of (left value, right length) entries, entry d held by lane d % 16 in slot d / 16 (32 entries; n < 2^31 needs 25).
// Inside a leaf of 8 or more terms lane j (< 8) is the strided accumulator r[j].
struct PairwiseF32 {
    int pos, leaf_start, block_end, leaf_end, sp;
    float res, r, total;
    float left0, left1;
    int right0, right1;

    __device__ void start_node(int len, int lane)
    {
        while (len > 128) {
            const int n2 = len / 2 - (len / 2) % 8;
            push(len - n2, lane);
            len = n2;
        }
        leaf_start = pos;
        leaf_end = pos + len;
        block_end = len >= 8 ? pos + len - len % 8 : pos;
        res = -0.0f;  // numpy starts the in-order part at -0.0
        r = -0.0f;
    }
    __device__ void push(int right_len, int lane)
    {
        if (lane == (sp & 15)) {
            if (sp >> 4) right1 = right_len;
            else right0 = right_len;
        }
        ++sp;
    }
    __device__ void init(int n, int lane)
    {
        pos = 0;
        sp = 0;
        total = -0.0f;  // pairwise of nothing
        if (n > 0) start_node(n, lane);
    }
    __device__ void finish_leaf(int lane)
    {
        float v = res;
        for (;;) {
            if (sp == 0) {
                total = v;
                return;
            }
            const int top = sp - 1, owner = top & 15;
            const int right_len = __shfl((top >> 4) ? right1 : right0, owner, kPairLanes);
            if (right_len > 0) {  // v is the left half: keep it, walk into the right half
                if (lane == owner) {
                    if (top >> 4) left1 = v, right1 = 0;
                    else left0 = v, right0 = 0;
                }
                start_node(right_len, lane);
                return;
            }
            v = __shfl((top >> 4) ? left1 : left0, owner, kPairLanes) + v;  // left + right
            sp = top;
        }
    }
    __device__ void feed(float t, int lane)
    {
        if (pos < block_end) {
            if (lane == ((pos - leaf_start) & 7)) r += t;
        } else {
            res += t;
        }
        ++pos;
        if (pos == block_end) {  // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)): the butterfly adds exactly these pairs into lane 0
            float x = r;
            x += __shfl_xor(x, 1, kPairLanes);
            x += __shfl_xor(x, 2, kPairLanes);
            x += __shfl_xor(x, 4, kPairLanes);
            res = __shfl(x, 0, kPairLanes);
        }
        if (pos == leaf_end) finish_leaf(lane);
    }
};

// the term of short-row entry i, 0.0f when its column is not in the long row (or the product is 0: scipy drops it too)
__device__ inline float f32_term(const int32_t *__restrict__ col, const double *__restrict__ val, const double *__restrict__ mult,
                                 int64_t sb, int64_t lb, int i, int dl, bool swapped)
{
    const int32_t w = col[sb + i];
    int lo = 0, hi = dl;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[lb + mid] < w) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= dl || col[lb + lo] != w) return 0.0f;
    // the values are float32 numbers held in fp64: these casts are exact
    const float a_short = val ? (float)val[sb + i] : 1.0f, a_long = val ? (float)val[lb + lo] : 1.0f;
    const float a_src = swapped ? a_long : a_short, a_dst = swapped ? a_short : a_long;
    return a_src * (mult ? a_dst * (float)mult[w] : a_dst);  // A_ = A.multiply(mult) is stored rounded, then the product
}

__global__ __launch_bounds__(256) void common_neighbour_f32_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                   const double *__restrict__ val, const double *__restrict__ mult,
                                                                   int64_t N, const int64_t *__restrict__ links, int64_t B,
                                                                   float *__restrict__ out, int32_t *__restrict__ err_flag)
{
    const int l = threadIdx.x & (kPairLanes - 1);
    const int64_t q = (int64_t)blockIdx.x * (blockDim.x / kPairLanes) + threadIdx.x / kPairLanes;
    if (q >= B) return;
    const int64_t u = links[2 * q], v = links[2 * q + 1];
    if (u < 0 || u >= N || v < 0 || v >= N) {
        if (l == 0) {
            out[q] = 0.0f;
            if (err_flag) *err_flag = 1;
        }
        return;
    }
    const int64_t ub = rowptr[u], vb = rowptr[v];
    const int du = (int)(rowptr[u + 1] - ub), dv = (int)(rowptr[v + 1] - vb);
    const bool swapped = du > dv;
    const int64_t sb = swapped ? vb : ub, lb = swapped ? ub : vb;
    const int ds = swapped ? dv : du, dl = swapped ? du : dv;
    // pass 1: m, the number of non-zero terms (numpy's split points depend on it); the first chunk's terms are kept
    const float first = l < ds ? f32_term(col, val, mult, sb, lb, l, dl, swapped) : 0.0f;
    int m = __popc(group_ballot(first != 0.0f));
    for (int c = kPairLanes; c < ds; c += kPairLanes) {
        const float t = c + l < ds ? f32_term(col, val, mult, sb, lb, c + l, dl, swapped) : 0.0f;
        m += __popc(group_ballot(t != 0.0f));
    }
    // pass 2: the terms in column order -> t[0] + pairwise(t[1:])
    PairwiseF32 pw;
    pw.init(m > 1 ? m - 1 : 0, l);
    float head = 0.0f;
    int rank = 0;
    for (int c = 0; c < ds && rank < m; c += kPairLanes) {
        const float t = c == 0 ? first : (c + l < ds ? f32_term(col, val, mult, sb, lb, c + l, dl, swapped) : 0.0f);
        uint32_t mask = group_ballot(t != 0.0f);
        while (mask) {
            const int src = __ffs(mask) - 1;
            mask &= mask - 1;
            const float x = __shfl(t, src, kPairLanes);
            if (rank == 0) head = x;
            else pw.feed(x, l);
            ++rank;
        }
    }
    if (l == 0) out[q] = m == 0 ? 0.0f : head + pw.total;
}

}  // namespace ss

extern "C" int ss_common_neighbour_scores(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult,
                                          int64_t N, const int64_t *links, int64_t B, float *out, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (N < 0 || B < 0 || N >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    if (B == 0) return SS_OK;
    if (!rowptr || !col || !links || !out) return SS_ERR_INVALID_ARG;
    const int pairs_per_block = 256 / kPairLanes;
    const int64_t blocks = (B + pairs_per_block - 1) / pairs_per_block;
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(common_neighbour_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, mult, N,
                       links, B, out, err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_common_neighbour_scores_f32(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult,
                                              int64_t N, const int64_t *links, int64_t B, float *out, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (N < 0 || B < 0 || N >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    if (B == 0) return SS_OK;
    if (!rowptr || !col || !links || !out) return SS_ERR_INVALID_ARG;
    const int pairs_per_block = 256 / kPairLanes;
    const int64_t blocks = (B + pairs_per_block - 1) / pairs_per_block;
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(common_neighbour_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, mult,
                       N, links, B, out, err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
