// ss_csr_sort_rows.hip -- the rows of a CSR sorted ascending, in place.  The builder (ss_csr.hip) leaves the order inside a row
// unspecified (min / max do not care); who does care sorts afterwards: binary-searched rows (negatives.py, subgraphs.py) and the
// STABLE groupings of sign.py (ss_csr_group_ids with the entry index as payload, then this).  Nothing here knows how the CSR was built.
#include "ss_common.hpp"

namespace ss {

// ---- rows of a CSR sorted ascending ----------------------------------------------------------------------------------------------
// compare-exchange network over the low `G` lanes of a lane group (G = 16 or 64, a power of two): ascending
template <int G>
__device__ __forceinline__ int bitonic_lanes(int v, int lane)
{
#pragma unroll
    for (int k = 2; k <= G; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = __shfl_xor(v, j);
            const bool up = (lane & k) == 0, low = (lane & j) == 0;
            v = (low == up) ? (v < o ? v : o) : (v > o ? v : o);
        }
    return v;
}

// rows of at most 64 entries: four rows per wavefront (16 lanes each) where all four have at most 16 entries, else one after the
// other over the whole wavefront; longer rows are listed for sort_rows_long_kernel
__global__ __launch_bounds__(256) void sort_rows_short_kernel(const int64_t *__restrict__ rowptr, int32_t *__restrict__ col, int64_t N,
                                                              int32_t *__restrict__ long_rows, int32_t *__restrict__ n_long,
                                                              const int32_t *__restrict__ keep_word)
{
    if (keep_word && *keep_word == 0) return;  // (see ss_csr_sort_rows)
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t r0 = wave * 4;
    if (r0 >= N) return;
    // lanes 0..4 read the five row bounds of this wavefront's four rows
    const int64_t my = lane <= 4 ? rowptr[r0 + lane < N ? r0 + lane : N] : 0;
    int64_t b[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) b[k] = __shfl(my, k);
    const int64_t max_len = [&] { int64_t m = 0; for (int k = 0; k < 4; ++k) m = b[k + 1] - b[k] > m ? b[k + 1] - b[k] : m; return m; }();
    if (max_len <= 16) {  // (wave-uniform)
        const int g = lane >> 4, l = lane & 15;
        const int64_t a = b[0] + 0 * g;  // (keep b[] in SGPRs: select by comparisons)
        const int64_t lo = g == 0 ? b[0] : g == 1 ? b[1] : g == 2 ? b[2] : b[3];
        const int64_t hi = g == 0 ? b[1] : g == 1 ? b[2] : g == 2 ? b[3] : b[4];
        (void)a;
        const int len = (int)(hi - lo);
        int v = l < len ? col[lo + l] : 0x7FFFFFFF;
        if (len > 1) v = bitonic_lanes<16>(v, l);  // (the whole 16-lane group takes the same branch)
        if (l < len) col[lo + l] = v;
        return;
    }
    for (int k = 0; k < 4; ++k) {
        const int64_t lo = b[k], len = b[k + 1] - b[k];
        if (len > kWave) {
            if (lane == 0) long_rows[atomicAdd(n_long, 1)] = (int32_t)(r0 + k);
            continue;
        }
        if (len < 2) continue;
        int v = lane < len ? col[lo + lane] : 0x7FFFFFFF;
        v = bitonic_lanes<kWave>(v, lane);
        if (lane < len) col[lo + lane] = v;
    }
}

// rows above 64 entries, one workgroup each (grid-stride over the list): bitonic sort in LDS up to 16 384 entries; longer rows (hub
// rows of power-law graphs) are sorted in LDS chunk by chunk and the chunks merged pairwise (merge path: every thread finds where
// its stretch of the output begins in both runs by a binary search along a diagonal, then merges sequentially), ping-ponging
// between col and scratch (the row's own stretch of an E-entry scratch array)
constexpr int kSortRowLds = 16384;

// ascending bitonic sort of buf[0 .. n2), n2 a power of two <= kSortRowLds (all 1024 threads)
__device__ __forceinline__ void bitonic_lds(int32_t *buf, int n2)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += 1024) {
                const int p = i ^ j;
                if (p > i) {
                    const int32_t a = buf[i], c = buf[p];
                    if ((a > c) == ((i & k) == 0)) { buf[i] = c; buf[p] = a; }
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(1024) void sort_rows_long_kernel(const int64_t *__restrict__ rowptr, int32_t *__restrict__ col,
                                                              int32_t *__restrict__ scratch, const int32_t *__restrict__ long_rows,
                                                              const int32_t *__restrict__ n_long)
{
    __shared__ int32_t buf[kSortRowLds];
    const int n_rows = *n_long;
    for (int q = blockIdx.x; q < n_rows; q += gridDim.x) {
        const int64_t lo = rowptr[long_rows[q]], len = rowptr[long_rows[q] + 1] - lo;
        int32_t *base = col + lo;
        for (int64_t c0 = 0; c0 < len; c0 += kSortRowLds) {  // sorted chunks of up to 16 384 entries
            const int n = (int)(len - c0 < kSortRowLds ? len - c0 : kSortRowLds);
            int n2 = 1;
            while (n2 < n) n2 <<= 1;
            for (int i = threadIdx.x; i < n2; i += 1024) buf[i] = i < n ? base[c0 + i] : 0x7FFFFFFF;
            __syncthreads();
            bitonic_lds(buf, n2);
            for (int i = threadIdx.x; i < n; i += 1024) base[c0 + i] = buf[i];
            __syncthreads();
        }
        int32_t *src = base, *dst = scratch + lo;
        for (int64_t width = kSortRowLds; width < len; width <<= 1) {  // pairwise merges of runs of `width`
            for (int64_t s0 = 0; s0 < len; s0 += 2 * width) {
                const int64_t na = len - s0 < width ? len - s0 : width, nb = len - s0 - na < width ? len - s0 - na : width;
                const int32_t *A = src + s0, *Bp = A + na;
                int32_t *O = dst + s0;
                const int64_t m = na + nb, per = (m + 1023) / 1024;
                const int64_t d0 = per * threadIdx.x < m ? per * threadIdx.x : m, d1 = d0 + per < m ? d0 + per : m;
                // merge path: the number i of A's entries among the first d0 outputs (ties: A first -- the sort need not be
                // stable, the entries of a row are distinct positions / may repeat harmlessly)
                int64_t a_lo = d0 > nb ? d0 - nb : 0, a_hi = d0 < na ? d0 : na;
                while (a_lo < a_hi) {
                    const int64_t i = (a_lo + a_hi) >> 1;  // try i entries of A, d0 - i of B
                    if (A[i] <= Bp[d0 - i - 1]) a_lo = i + 1; else a_hi = i;
                }
                int64_t i = a_lo, j = d0 - a_lo;
                for (int64_t o = d0; o < d1; ++o) {
                    const bool take_a = j >= nb || (i < na && A[i] <= Bp[j]);
                    O[o] = take_a ? A[i++] : Bp[j++];
                }
            }
            __syncthreads();
            int32_t *t = src; src = dst; dst = t;
        }
        if (src != base) {
            for (int64_t i = threadIdx.x; i < len; i += 1024) base[i] = src[i];
        }
        __syncthreads();
    }
}

}  // namespace ss

// Every row of a CSR sorted ascending in place (col of rows [0, N)).  With the entry indices as payload (ss_csr_group_ids,
// ss_group_links_by_source) that makes the grouping STABLE -- the reference's edge order inside every group; with source ids it
// gives the sorted adjacency scipy / torch_sparse hold.  Workspace: ss_csr_sort_workspace_bytes(E) device bytes.
extern "C" size_t ss_csr_sort_workspace_bytes(int64_t E) { return E < 0 ? 0 : (size_t)(E / ss::kWave + 2) * 4 + 256 + (size_t)(E > 0 ? E : 1) * 4; }

// only_if (nullable): device word; the rows are sorted only if it is NON-zero when the launches run (sign.py: the grouping by column
// needs its order only when some edge weight differs from 1 -- ss_gcn_scan_edges leaves that in the first word of its buffer)
extern "C" int ss_csr_sort_rows(const int64_t *rowptr, int32_t *col, int64_t N, int64_t E, const int32_t *only_if, void *workspace,
                                size_t workspace_bytes, void *stream_)
{
    using namespace ss;
    if (N < 0 || E < 0 || N >= ((int64_t)1 << 31) || E >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    if (N == 0 || E == 0) return SS_OK;
    if (!rowptr || !col) return SS_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < ss_csr_sort_workspace_bytes(E)) return SS_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    int32_t *n_long = reinterpret_cast<int32_t *>(workspace);
    int32_t *long_rows = n_long + 64;  // (its own cache lines)
    int32_t *scratch = long_rows + (E / kWave + 2);
    if (hipMemsetAsync(n_long, 0, 4, stream) != hipSuccess) return SS_ERR_LAUNCH;
    const int64_t waves = (N + 3) / 4;
    hipLaunchKernelGGL(sort_rows_short_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, rowptr, col, N, long_rows, n_long, only_if);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(sort_rows_long_kernel, dim3(512), dim3(1024), 0, stream, rowptr, col, scratch, long_rows, n_long);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
