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
// The row pair, the membership search and the term itself are csrc/ss_pair_rows.hpp's, shared with the lists of ss_cn_pool.hip.
#include "ss_pair_rows.hpp"

namespace ss {

__device__ inline double row16_sum_d(double x)
{
    for (int off = 1; off < kPairLanes; off <<= 1) x += __shfl_xor(x, off);
    return x;
}

// the pair of this 16-lane group (lane l of it) and its two rows; false: no pair is left, or one with an id outside [0, N), which
// scores 0 and raises the error flag
__device__ __forceinline__ bool scored_pair(const int64_t *__restrict__ rowptr, int64_t N, const int64_t *__restrict__ links, int64_t B,
                                            float *__restrict__ out, int32_t *__restrict__ err_flag, int &l, int64_t &q, PairRows &r)
{
    if (!group_pair(B, l, q)) return false;
    const int64_t u = links[2 * q], v = links[2 * q + 1];
    if (!ids_in_range(u, v, N)) {
        if (l == 0) {
            out[q] = 0.0f;
            if (err_flag) *err_flag = 1;
        }
        return false;
    }
    r = pair_rows(rowptr, u, v);
    return true;
}

__global__ __launch_bounds__(256) void common_neighbour_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                               const double *__restrict__ val, const double *__restrict__ mult,
                                                               int64_t N, const int64_t *__restrict__ links, int64_t B,
                                                               float *__restrict__ out, int32_t *__restrict__ err_flag)
{
    int l;
    int64_t q;
    PairRows r;
    if (!scored_pair(rowptr, N, links, B, out, err_flag, l, q, r)) return;
    double acc = 0.0;
    for (int i = l; i < r.ds; i += kPairLanes) {
        Member m;
        if (member(col, r, i, m)) acc += term_f64(val, mult, r, m);
    }
    acc = row16_sum_d(acc);
    if (l == 0) out[q] = (float)acc;
}


// ---- fp32 mode ---------------------------------------------------------------------------------------------------------------
// Control flow is uniform inside a 16-lane group (every value below except `r` and the stack slots is the same in all 16
// lanes), so ballots and width-16 shuffles see the whole group.

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

// the term of short-row entry i, 0.0f past the row's end and when its column is not in the long row (or the product is 0: scipy
// drops it too)
__device__ inline float f32_term(const int32_t *__restrict__ col, const double *__restrict__ val, const double *__restrict__ mult,
                                 const PairRows &r, int i)
{
    Member m;
    return i < r.ds && member(col, r, i, m) ? term_f32(val, mult, r, m) : 0.0f;
}

__global__ __launch_bounds__(256) void common_neighbour_f32_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                   const double *__restrict__ val, const double *__restrict__ mult,
                                                                   int64_t N, const int64_t *__restrict__ links, int64_t B,
                                                                   float *__restrict__ out, int32_t *__restrict__ err_flag)
{
    int l;
    int64_t q;
    PairRows r;
    if (!scored_pair(rowptr, N, links, B, out, err_flag, l, q, r)) return;
    const int base = (threadIdx.x & (kWave - 1)) - l;
    // pass 1: m, the number of non-zero terms (numpy's split points depend on it); the first chunk's terms are kept
    const float first = f32_term(col, val, mult, r, l);
    int m = __popc((uint32_t)unit_ballot(first != 0.0f, base, kPairLanes));
    for (int c = kPairLanes; c < r.ds; c += kPairLanes)
        m += __popc((uint32_t)unit_ballot(f32_term(col, val, mult, r, c + l) != 0.0f, base, kPairLanes));
    // pass 2: the terms in column order -> t[0] + pairwise(t[1:])
    PairwiseF32 pw;
    pw.init(m > 1 ? m - 1 : 0, l);
    float head = 0.0f;
    int rank = 0;
    for (int c = 0; c < r.ds && rank < m; c += kPairLanes) {
        const float t = c == 0 ? first : f32_term(col, val, mult, r, c + l);
        uint32_t mask = (uint32_t)unit_ballot(t != 0.0f, base, kPairLanes);
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
    return ss::launch_pairs(ss::common_neighbour_kernel, ss::kPairLanes, N, B, rowptr && col && links && out, stream, rowptr, col, val,
                            mult, N, links, B, out, err_flag);
}

extern "C" int ss_common_neighbour_scores_f32(const int64_t *rowptr, const int32_t *col, const double *val, const double *mult,
                                              int64_t N, const int64_t *links, int64_t B, float *out, int32_t *err_flag, void *stream)
{
    return ss::launch_pairs(ss::common_neighbour_f32_kernel, ss::kPairLanes, N, B, rowptr && col && links && out, stream, rowptr, col,
                            val, mult, N, links, B, out, err_flag);
}
