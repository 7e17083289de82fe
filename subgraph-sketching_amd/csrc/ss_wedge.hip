// ss_wedge.hip -- exact two-hop link candidates: the rows `sources` of A * A with integer walk counts, from the sorted CSR that
// NegativeSampler already builds (wedge.py).  A walk of source u is u -> w -> v with w in row u and v in row w, every
// copy of a repeated edge its own walk; W(u) = sum over w in row u of deg(w); common[u, v] = the walks of u that end in v.
//
//   wedge_walks_kernel  W(u) per source, one 16-lane DPP row per source (the lanes share row u, each adds the degrees of its w).
//   wedge_fold_kernel   the LDS tier, one workgroup per source with 2 W(u) <= slots: the endpoints are folded into an open-addressing
//                       (key, count) table in LDS -- atomicCAS claims the key, atomicAdd counts, linear probing, never more than half
//                       full -- and the D <= W(u) distinct entries leave as (s * N + v, count) at the front of the source's W(u)-sized
//                       slot of the output; the other W(u) - D places are padded with kWedgePad / 0, which the host drops.
//   wedge_emit_kernel   the large tier, workgroups (source, y): the raw endpoints s * N + v of every walk at offsets[s] + its place in
//                       the order (w ascending in row u, then v ascending in row w).  Row u is taken 256 neighbours at a time; every
//                       workgroup of the source scans the degrees of all slices (the running offset), workgroup y copies the rows of
//                       slices y, y + Y, ... only, a 16-lane row per neighbour.  The host's sort + run-length count folds them.
//
// Both expansion kernels are given the walks the host read back (0: the source is skipped) and the exclusive scan of them; which tier
// serves a source follows from W(u) and `slots` alone (ss_wedge.hpp), so the two launches cover every source exactly once.  Every store
// is bounded by the source's slot [offsets[s], offsets[s] + W(u)).  Vector stores only, int64 offsets into col, N < 2^31.
#include "ss_wedge.hpp"

namespace ss {

constexpr int kWedgeGroups = kWedgeThreads / kRow;

// the wrapped id of sources[s], or -1 when it lies outside [-N, N)
__device__ __forceinline__ int64_t wedge_source(const int64_t *__restrict__ sources, int64_t s, int64_t N)
{
    int64_t u = sources[s];
    u = u < 0 ? u + N : u;  // torch-style negative indexing, as the one-vs-all scans
    return (uint64_t)u < (uint64_t)N ? u : -1;
}

__global__ __launch_bounds__(256) void wedge_walks_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                           const int64_t *__restrict__ sources, int64_t S, int64_t *__restrict__ walks,
                                                           int32_t *__restrict__ err)
{
    const int64_t g = (int64_t)blockIdx.x * kWedgeGroups + threadIdx.x / kRow;
    if (g >= S) return;
    const int l = threadIdx.x & (kRow - 1);
    const int64_t u = wedge_source(sources, g, N);
    if (u < 0) {
        if (l == 0) {
            if (err) *err = 1;
            walks[g] = 0;
        }
        return;
    }
    const int64_t ub = rowptr[u], ue = rowptr[u + 1];
    long long w = 0;
    for (int64_t i = ub + l; i < ue; i += kRow) {
        const int64_t x = col[i];
        w += rowptr[x + 1] - rowptr[x];
    }
    for (int off = kRow / 2; off; off >>= 1) w += __shfl_xor(w, off, kRow);
    if (l == 0) walks[g] = w;
}

// every walk endpoint of the neighbours [i0, i0 + n) of row u (n <= 256): a 16-lane row per neighbour, f(place of the neighbour in
// the slice, place of v in row w, v)
template <typename F>
__device__ __forceinline__ void wedge_rows(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t ub, int64_t i0, int n, F f)
{
    const int l = threadIdx.x & (kRow - 1);
    for (int g = threadIdx.x / kRow; g < n; g += kWedgeGroups) {
        const int64_t w = col[ub + i0 + g];
        const int64_t wb = rowptr[w], d = rowptr[w + 1] - wb;
        for (int64_t t = l; t < d; t += kRow) f(g, t, col[wb + t]);
    }
}

__global__ __launch_bounds__(256) void wedge_fold_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                          const int64_t *__restrict__ sources, const int64_t *__restrict__ walks,
                                                          const int64_t *__restrict__ offsets, int slots, int64_t *__restrict__ keys,
                                                          int32_t *__restrict__ counts)
{
    __shared__ int32_t tk[kWedgeMaxSlots];
    __shared__ int32_t tc[kWedgeMaxSlots];
    __shared__ int32_t n_out;
    const int64_t s = blockIdx.x;
    const int64_t W = walks[s];
    if (!wedge_folds(W, slots)) return;  // (the whole workgroup)
    const int64_t u = wedge_source(sources, s, N);
    if (u < 0) return;
    const int m = wedge_table_slots(W, slots), k = wedge_log2(m);
    for (int i = threadIdx.x; i < m; i += kWedgeThreads) {
        tk[i] = -1;
        tc[i] = 0;
    }
    if (threadIdx.x == 0) n_out = 0;
    __syncthreads();
    const int64_t ub = rowptr[u], deg = rowptr[u + 1] - ub;
    for (int64_t i0 = 0; i0 < deg; i0 += kWedgeThreads) {
        const int n = deg - i0 < kWedgeThreads ? (int)(deg - i0) : kWedgeThreads;
        wedge_rows(rowptr, col, ub, i0, n, [&](int, int64_t, int32_t v) {
            int h = wedge_slot(v, k);
            for (int tries = 0; tries < m; ++tries) {  // (at most half full: an empty slot is met long before m tries)
                const int32_t was = atomicCAS(&tk[h], -1, v);
                if (was == -1 || was == v) {
                    atomicAdd(&tc[h], 1);
                    break;
                }
                h = (h + 1) & (m - 1);
            }
        });
    }
    __syncthreads();
    const int64_t base = offsets[s];
    for (int i = threadIdx.x; i < m; i += kWedgeThreads)
        if (tk[i] >= 0) {
            const int64_t p = atomicAdd(&n_out, 1);
            if (p < W) {
                keys[base + p] = s * N + tk[i];
                counts[base + p] = tc[i];
            }
        }
    __syncthreads();
    for (int64_t i = (int64_t)n_out + threadIdx.x; i < W; i += kWedgeThreads) {
        keys[base + i] = kWedgePad;
        counts[base + i] = 0;
    }
}

// exclusive scan of one value per thread over the workgroup; total: the sum, in every thread
__device__ __forceinline__ int64_t wedge_block_scan(long long x, int64_t *wave_sums, int64_t &total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    long long incl = x;
    for (int off = 1; off < kWave; off <<= 1) {
        const long long t = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += t;
    }
    if (lane == kWave - 1) wave_sums[wave] = incl;
    __syncthreads();
    int64_t before = 0;
    total = 0;
    for (int i = 0; i < kWedgeThreads / kWave; ++i) {
        if (i < wave) before += wave_sums[i];
        total += wave_sums[i];
    }
    __syncthreads();  // (wave_sums is written again by the next slice)
    return before + incl - x;
}

__global__ __launch_bounds__(256) void wedge_emit_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                          const int64_t *__restrict__ sources, const int64_t *__restrict__ walks,
                                                          const int64_t *__restrict__ offsets, int slots, int64_t *__restrict__ keys)
{
    __shared__ int64_t wave_sums[kWedgeThreads / kWave];
    __shared__ int64_t at[kWedgeThreads];
    const int64_t s = blockIdx.x;
    const int64_t W = walks[s];
    if (!wedge_emits(W, slots)) return;  // (the whole workgroup)
    const int64_t u = wedge_source(sources, s, N);
    if (u < 0) return;
    const int64_t ub = rowptr[u], deg = rowptr[u + 1] - ub;
    const int64_t end = offsets[s] + W;
    int64_t base = offsets[s];
    for (int64_t i0 = 0, slice = 0; i0 < deg; i0 += kWedgeThreads, ++slice) {
        const int n = deg - i0 < kWedgeThreads ? (int)(deg - i0) : kWedgeThreads;
        long long d = 0;
        if ((int)threadIdx.x < n) {
            const int64_t w = col[ub + i0 + threadIdx.x];
            d = rowptr[w + 1] - rowptr[w];
        }
        int64_t total;
        const int64_t before = wedge_block_scan(d, wave_sums, total);
        if (slice % gridDim.y == blockIdx.y) {
            at[threadIdx.x] = base + before;
            __syncthreads();
            wedge_rows(rowptr, col, ub, i0, n, [&](int g, int64_t t, int32_t v) {
                const int64_t o = at[g] + t;
                if (o < end) keys[o] = s * N + v;
            });
            __syncthreads();
        }
        base += total;
    }
}

}  // namespace ss

extern "C" int ss_wedge_walks(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S, int64_t *walks,
                              int32_t *err_flag, void *stream)
{
    using namespace ss;
    const int rc = check_wedge_graph(rowptr, col, N, sources, S);
    if (rc != SS_OK || S == 0) return rc;
    if (!walks) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(wedge_walks_kernel, dim3((unsigned)((S + kWedgeGroups - 1) / kWedgeGroups)), dim3(kWedgeThreads), 0, (hipStream_t)stream,
                       rowptr, col, N, sources, S, walks, err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_wedge_fold(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S, const int64_t *walks,
                             const int64_t *offsets, int32_t slots, int64_t *keys, int32_t *counts, void *stream)
{
    using namespace ss;
    const int rc = check_wedge_expand(rowptr, col, N, sources, S, walks, offsets, slots, keys, counts);
    if (rc != SS_OK || S == 0) return rc;
    if (slots < 2) return SS_OK;  // (no source has 2 W <= 1)
    hipLaunchKernelGGL(wedge_fold_kernel, dim3((unsigned)S), dim3(kWedgeThreads), 0, (hipStream_t)stream, rowptr, col, N, sources, walks, offsets,
                       (int)slots, keys, counts);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_wedge_emit(const int64_t *rowptr, const int32_t *col, int64_t N, const int64_t *sources, int64_t S, const int64_t *walks,
                             const int64_t *offsets, int32_t slots, int32_t slices, int64_t *keys, void *stream)
{
    using namespace ss;
    const int32_t some = 0;
    const int rc = check_wedge_expand(rowptr, col, N, sources, S, walks, offsets, slots, keys, &some);
    if (rc != SS_OK) return rc;
    if (slices < 1 || slices > kWedgeMaxSlices) return SS_ERR_INVALID_ARG;
    if (S == 0) return SS_OK;
    hipLaunchKernelGGL(wedge_emit_kernel, dim3((unsigned)S, (unsigned)slices), dim3(kWedgeThreads), 0, (hipStream_t)stream, rowptr, col, N, sources,
                       walks, offsets, (int)slots, keys);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
