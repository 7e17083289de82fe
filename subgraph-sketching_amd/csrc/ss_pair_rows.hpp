// ss_pair_rows.hpp -- the sorted-row step of a node pair, shared by the CN / AA / RA scores (ss_heuristics.hip) and the
// common-neighbour lists and pools (ss_cn_pool.hip).  A is a CSR with sorted, duplicate-free column ids.  The lanes of a pair stride
// over the SHORTER of rows u and v and bisect the longer one; a column found in both is a common neighbour w, and its term is
//     A[u, w] * (A[v, w] * mult[w])        (mult null = 1, val null = a matrix of ones)
// with src = u and dst = v whichever row was walked.  ONE product, rounded two ways:
//   term_f64   fp64 with this association: the scores of int, bool and float64 matrices add it up in fp64; coefficient() is its one
//              rounding to float, the c(u, v, w) of the lists and pools for every matrix dtype
//   term_f32   the same roles in float32 arithmetic, every product rounded: what scipy computes for a float32 matrix
#pragma once
#include "ss_common.hpp"

namespace ss {

constexpr int kPairLanes = 16;  // lanes per pair of every kernel here but the pool kernel, which picks 16 | 32 | 64

// which pair this 16-lane group owns: l = the lane inside the group, q = the pair; false: the group lies beyond the batch
__device__ __forceinline__ bool group_pair(int64_t B, int &l, int64_t &q)
{
    l = threadIdx.x & (kPairLanes - 1);
    q = (int64_t)blockIdx.x * (blockDim.x / kPairLanes) + threadIdx.x / kPairLanes;
    return q < B;
}

__device__ __forceinline__ bool ids_in_range(int64_t u, int64_t v, int64_t N)
{
    return (uint64_t)u < (uint64_t)N && (uint64_t)v < (uint64_t)N;
}

// this unit's bits of the wavefront ballot (U lanes starting at lane `base`); control flow is uniform inside a unit
__device__ __forceinline__ uint64_t unit_ballot(bool pred, int base, int U)
{
    const uint64_t all = __ballot(pred) >> base;
    return U == kWave ? all : all & (((uint64_t)1 << U) - 1);
}

// the two rows of a pair, the shorter one first; `swapped`: the shorter row is v's
struct PairRows {
    int64_t sb, lb;
    int ds, dl;
    bool swapped;
};

__device__ __forceinline__ PairRows pair_rows(const int64_t *__restrict__ rowptr, int64_t u, int64_t v)
{
    const int64_t ub = rowptr[u], vb = rowptr[v];
    const int du = (int)(rowptr[u + 1] - ub), dv = (int)(rowptr[v + 1] - vb);
    PairRows r;
    r.swapped = du > dv;
    r.sb = r.swapped ? vb : ub;
    r.lb = r.swapped ? ub : vb;
    r.ds = r.swapped ? dv : du;
    r.dl = r.swapped ? du : dv;
    return r;
}

// a common neighbour: the column and where it sits in the shorter and the longer row -- positions in col and val, so that one address
// sum serves the column's load and its value's
struct Member {
    int32_t w;
    int64_t at_short, at_long;
};

// entry i of the shorter row: is its column in the longer row?
__device__ __forceinline__ bool member(const int32_t *__restrict__ col, const PairRows &r, int i, Member &m)
{
    m.at_short = r.sb + i;
    m.w = col[m.at_short];
    const int pos = bound<false>(col + r.lb, 0, r.dl, m.w);
    m.at_long = r.lb + pos;
    return pos < r.dl && col[m.at_long] == m.w;
}

// the term of a member in fp64 and in float32 arithmetic: the roles of src and dst stay the reference's whichever row was walked
__device__ __forceinline__ double term_f64(const double *__restrict__ val, const double *__restrict__ mult, const PairRows &r,
                                           const Member &m)
{
    const double a_short = val ? val[m.at_short] : 1.0, a_long = val ? val[m.at_long] : 1.0;
    const double a_src = r.swapped ? a_long : a_short, a_dst = r.swapped ? a_short : a_long;
    return a_src * (mult ? a_dst * mult[m.w] : a_dst);
}
__device__ __forceinline__ float term_f32(const double *__restrict__ val, const double *__restrict__ mult, const PairRows &r,
                                          const Member &m)
{
    // the values are float32 numbers held in fp64: these casts are exact
    const float a_short = val ? (float)val[m.at_short] : 1.0f, a_long = val ? (float)val[m.at_long] : 1.0f;
    const float a_src = r.swapped ? a_long : a_short, a_dst = r.swapped ? a_short : a_long;
    return a_src * (mult ? a_dst * (float)mult[m.w] : a_dst);  // A_ = A.multiply(mult) is stored rounded, then the product
}
__device__ __forceinline__ float coefficient(const double *__restrict__ val, const double *__restrict__ mult, const PairRows &r,
                                             const Member &m)
{
    return (float)term_f64(val, mult, r, m);
}

// The host preamble of the pair entry points, in their order: the sizes, the empty batch, `given` (the entry point's own null checks,
// which an empty batch is spared), a grid of 256 / lanes pairs per block below 2^31 blocks, the launch.
template <typename F, typename... Args>
int launch_pairs(F kernel, int lanes, int64_t N, int64_t B, bool given, void *stream, Args... args)
{
    if (N < 0 || B < 0 || N >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    if (B == 0) return SS_OK;
    if (!given) return SS_ERR_INVALID_ARG;
    const int per_block = 256 / lanes;
    const int64_t blocks = (B + per_block - 1) / per_block;
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, args...);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

}  // namespace ss
