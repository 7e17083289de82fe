// ss_aggr.hip -- unnormalised neighbour aggregation for SAGEConv and GINConv (reference models/seal.py:116-173, 259-328 and
// models/gnn.py:90-113) [PyG semantics restated]: out[dst_e] (+)= w_e * x[src_e] over the edges as they are -- no gcn_norm, existing
// self loops are ordinary entries, no loop is added -- then a division by the row's weight sum (mean) and / or a root term
// (1 + eps) * x_i (GIN).  The gather idiom is sign_spmm_kernel's (ss_spmm.hip): a lane owns one float4 of the feature row,
// pow2(F / 4) lanes (at most 64) form a row group, entries are fetched one per lane and handed out by shuffles, feature rows are
// requested four ahead, F > 256 loops over chunk bases.
//
// The accumulation order is what the family is pinned to.  Output row i with the entries e_0 < e_1 < ... (edge indices
// grouped at i, ascending) in chunks of SS_AGGR_CHUNK = 256:
//   p_c = the sequential fp32 sum, from +0, of the terms of chunk c        s = ((0 + p_0) + p_1) + ...
// term t_e = fl(w_e * v_e) (unit weights: w is never gathered, the bits are those of * 1), v_e = x[src_e], or fl(x[src_e] / d[src_e])
// when a gather divisor is given (the mean's backward).  One lane per output element and chunk, products and adds rounded separately,
// no float atomics, no inter-workgroup waits.  Because a row IS its chunk sums added in chunk order, the chunks of a long row (a hub:
// more than hub_entries entries) can be walked by other row groups (aggr_hub_partials_kernel) and added afterwards
// (aggr_hub_finish_kernel) without changing a bit: a row's bits do not depend on the tier.
#include "ss_common.hpp"
#include "ss_walks.hpp"

#define SS_AGGR_CHUNK 256  // entries per chunk of the accumulation order; ss_aggr_chunk() tells it to callers

namespace ss {

constexpr int kAggrChunk = SS_AGGR_CHUNK;

// p_c for the float4 column c of the entries at the group positions [a, b), 0 < b - a <= kAggrChunk, of row i: every lane of the row
// group calls it with the same (a, b, i).  An id outside [0, N) is not followed (the plan reports it on the host).
template <bool kDiv>
__device__ __forceinline__ float4 aggr_chunk_sum(const int32_t *__restrict__ order, const int64_t *__restrict__ other,
                                                 const float *__restrict__ w, const float *__restrict__ gden, int64_t N,
                                                 const float *__restrict__ x, int F, int64_t i, int64_t a, int64_t b, int c, int cl, int base,
                                                 int lanes_per_row)
{
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int64_t j0 = a; j0 < b; j0 += lanes_per_row) {
        const int64_t j = j0 + cl;  // this lane's entry of the stretch
        const int32_t e = order[j < b ? j : a];
        const int64_t raw = other[e];
        const bool in_range = (uint64_t)raw < (uint64_t)N;
        const int64_t my_c = in_range ? raw : i;
        const float my_w = w ? w[e] : 1.0f;
        const float my_d = kDiv ? gden[my_c] : 1.0f;
        const int my_use = j < b && in_range;
        const int n = (int)(b - j0 < lanes_per_row ? b - j0 : lanes_per_row);
        for (int k0 = 0; k0 < n; k0 += 4) {  // (uniform per row group)
            float4 r[4];
            float wk[4], dk[4];
            int use[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int src = base + (k0 + k < lanes_per_row ? k0 + k : 0);
                const int64_t cj = ((int64_t)__shfl((int)(my_c >> 32), src) << 32) | (uint32_t)__shfl((int)my_c, src);
                wk[k] = __shfl(my_w, src);
                dk[k] = kDiv ? __shfl(my_d, src) : 1.0f;
                use[k] = k0 + k < n ? __shfl(my_use, src) : 0;
                r[k] = *reinterpret_cast<const float4 *>(x + (use[k] ? cj : i) * F + 4 * c);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (use[k]) {
                    float4 v = r[k];
                    if (kDiv) {
                        v.x = v.x / dk[k];
                        v.y = v.y / dk[k];
                        v.z = v.z / dk[k];
                        v.w = v.w / dk[k];
                    }
                    p.x += v.x * wk[k];
                    p.y += v.y * wk[k];
                    p.z += v.z * wk[k];
                    p.w += v.w * wk[k];
                }
        }
    }
    return p;
}

// what follows the sum of a row: the mean's division, then the root term
__device__ __forceinline__ float4 aggr_epilogue(float4 s, const float *__restrict__ den, const float *__restrict__ root,
                                                const float *__restrict__ root_x, int F, int64_t i, int c)
{
    if (den) {
        const float d = den[i];
        s.x = s.x / d;
        s.y = s.y / d;
        s.z = s.z / d;
        s.w = s.w / d;
    }
    if (root) {
        const float r = *root;
        const float4 xi = *reinterpret_cast<const float4 *>(root_x + i * F + 4 * c);
        s.x += r * xi.x;
        s.y += r * xi.y;
        s.z += r * xi.z;
        s.w += r * xi.w;
    }
    return s;
}

// the regular tier: one row group walks the whole row, chunk after chunk, and stores it.  Rows past N shadow row N - 1 and do not
// store (the shuffles need every lane); rows of more than hub_entries entries belong to the hub tier and are left alone.
template <bool kDiv>
__global__ __launch_bounds__(256) void aggr_rows_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ order,
                                                        const int64_t *__restrict__ other, const float *__restrict__ w,
                                                        const float *__restrict__ gden, int64_t N, int64_t hub_entries,
                                                        const float *__restrict__ x, int F, const float *__restrict__ den,
                                                        const float *__restrict__ root, const float *__restrict__ root_x,
                                                        float *__restrict__ out, int lanes_per_row)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int rows_per_wave = kWave / lanes_per_row;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t i_raw = wave * rows_per_wave + lane / lanes_per_row;
    const int64_t i = i_raw < N ? i_raw : N - 1;
    const int cl = lane % lanes_per_row, base = lane - cl;
    const int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
    if (e1 - e0 > hub_entries) return;  // (the whole row group leaves)
    const int CF = F >> 2;
    for (int cbase = 0; cbase < CF; cbase += lanes_per_row) {  // (one iteration unless F > 256)
        const int c = cbase + cl < CF ? cbase + cl : CF - 1;  // lanes past the last chunk read it and do not store, in every iteration
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int64_t a = e0; a < e1; a += kAggrChunk) {
            const int64_t b = e1 - a < kAggrChunk ? e1 : a + kAggrChunk;
            const float4 p = aggr_chunk_sum<kDiv>(order, other, w, gden, N, x, F, i, a, b, c, cl, base, lanes_per_row);
            s.x += p.x;
            s.y += p.y;
            s.z += p.z;
            s.w += p.w;
        }
        s = aggr_epilogue(s, den, root, root_x, F, i, c);
        if (i_raw < N && cbase + cl < CF) *reinterpret_cast<float4 *>(out + i * F + 4 * c) = s;
    }
}

// the hub tier, first launch: one row group per (hub row, chunk) writes p_c to row g of the workspace [n_chunks, F].  Chunk g belongs
// to hub chunk_hub[g], whose chunks are hub_chunk[h] .. hub_chunk[h + 1].  A list entry that names no row of the graph, or no entries
// of its row, is not followed and writes nothing.
template <bool kDiv>
__global__ __launch_bounds__(256) void aggr_hub_partials_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ order,
                                                                const int64_t *__restrict__ other, const float *__restrict__ w,
                                                                const float *__restrict__ gden, int64_t N,
                                                                const int32_t *__restrict__ hub_rows, const int32_t *__restrict__ hub_chunk,
                                                                const int32_t *__restrict__ chunk_hub, int64_t n_hubs, int64_t n_chunks,
                                                                const float *__restrict__ x, int F, float *__restrict__ ws,
                                                                int lanes_per_row)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int rows_per_wave = kWave / lanes_per_row;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t g_raw = wave * rows_per_wave + lane / lanes_per_row;
    const int64_t g = g_raw < n_chunks ? g_raw : n_chunks - 1;
    const int cl = lane % lanes_per_row, base = lane - cl;
    const int64_t h = chunk_hub[g];
    if ((uint64_t)h >= (uint64_t)n_hubs) return;
    const int64_t i = hub_rows[h];
    if ((uint64_t)i >= (uint64_t)N) return;
    const int64_t a = rowptr[i] + (g - hub_chunk[h]) * kAggrChunk, e1 = rowptr[i + 1];
    if (a < rowptr[i] || a >= e1) return;
    const int64_t b = e1 - a < kAggrChunk ? e1 : a + kAggrChunk;
    const int CF = F >> 2;
    for (int cbase = 0; cbase < CF; cbase += lanes_per_row) {
        const int c = cbase + cl < CF ? cbase + cl : CF - 1;
        const float4 p = aggr_chunk_sum<kDiv>(order, other, w, gden, N, x, F, i, a, b, c, cl, base, lanes_per_row);
        if (g_raw < n_chunks && cbase + cl < CF) *reinterpret_cast<float4 *>(ws + g * F + 4 * c) = p;
    }
}

// the hub tier, second launch: one lane per float4 of a hub row adds the row's partials in chunk order, applies the epilogue of the
// regular tier and stores the row
__global__ __launch_bounds__(256) void aggr_hub_finish_kernel(const int32_t *__restrict__ hub_rows, const int32_t *__restrict__ hub_chunk,
                                                              int64_t n_hubs, int64_t n_chunks, int64_t N, const float *__restrict__ ws, int F,
                                                              const float *__restrict__ den, const float *__restrict__ root,
                                                              const float *__restrict__ root_x, float *__restrict__ out)
{
    const int CF = F >> 2;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t h = t / CF;
    const int c = (int)(t - h * CF);
    if (h >= n_hubs) return;
    const int64_t i = hub_rows[h];
    if ((uint64_t)i >= (uint64_t)N) return;
    int64_t g0 = hub_chunk[h], g1 = hub_chunk[h + 1];
    g0 = g0 < 0 ? 0 : g0;
    g1 = g1 > n_chunks ? n_chunks : g1;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int64_t g = g0; g < g1; ++g) {
        const float4 p = *reinterpret_cast<const float4 *>(ws + g * F + 4 * c);
        s.x += p.x;
        s.y += p.y;
        s.z += p.z;
        s.w += p.w;
    }
    s = aggr_epilogue(s, den, root, root_x, F, i, c);
    *reinterpret_cast<float4 *>(out + i * F + 4 * c) = s;
}

// den[i]: the chunked sum of the weights of row i's entries, 1 for a row without entries.  Unit weights (w null): the count, which
// the chunked sum of ones equals exactly up to 2^24.  Otherwise one 16-lane group per row, 16 loads at a time, added lane by lane.
__global__ __launch_bounds__(256) void aggr_degree_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ order,
                                                          const float *__restrict__ w, int64_t N, float *__restrict__ den)
{
    if (!w) {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= N) return;
        const int64_t m = rowptr[i + 1] - rowptr[i];
        den[i] = m > 0 ? (float)m : 1.0f;
        return;
    }
    const int l = threadIdx.x & (kRow - 1);
    const int base = (threadIdx.x & (kWave - 1)) & ~(kRow - 1);
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kRow; i < N; i += (int64_t)gridDim.x * blockDim.x / kRow) {
        const int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
        float s = 0.0f;
        for (int64_t a = e0; a < e1; a += kAggrChunk) {
            const int64_t b = e1 - a < kAggrChunk ? e1 : a + kAggrChunk;
            float p = 0.0f;
            for (int64_t j0 = a; j0 < b; j0 += kRow) {
                const int64_t j = j0 + l;
                const float we = w[order[j < b ? j : a]];
                const int n = (int)(b - j0 < kRow ? b - j0 : kRow);
                for (int k = 0; k < n; ++k) p += __shfl(we, base + k);  // (group-uniform trip count)
            }
            s += p;
        }
        if (l == 0) den[i] = e1 > e0 ? s : 1.0f;
    }
}

static inline int aggr_lanes(int F)
{
    int lanes = pow2_ceil(F >> 2);
    return lanes > kWave ? kWave : lanes;
}

static inline bool aggr_shape_ok(int64_t N, int32_t F) { return N >= 0 && F > 0 && !(F & 3) && N < ((int64_t)1 << 31); }

}  // namespace ss

extern "C" int ss_aggr_chunk(void) { return SS_AGGR_CHUNK; }

extern "C" size_t ss_aggr_workspace_bytes(int64_t hub_chunks, int32_t F)
{
    if (hub_chunks < 0 || F <= 0 || (F & 3) || hub_chunks >= ((int64_t)1 << 31)) return 0;
    return (size_t)hub_chunks * (size_t)F * sizeof(float);
}

extern "C" int ss_aggr_degree(const int64_t *rowptr, const int32_t *order, const float *w, int64_t N, float *den, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    if (N == 0) return SS_OK;
    if (!rowptr || !order || !den) return SS_ERR_INVALID_ARG;
    int64_t blocks = (N + 255) / 256;  // (unit weights: one thread per row; else 16-lane groups striding over the rows)
    if (w && blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(aggr_degree_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, order, w, N, den);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_aggr_rows(const int64_t *rowptr, const int32_t *order, const int64_t *other, const float *w, int64_t N, int64_t hub_entries,
                            const float *x, int32_t F, const float *gather_den, const float *den, const float *root, const float *root_x,
                            float *out, void *stream)
{
    using namespace ss;
    if (!aggr_shape_ok(N, F) || hub_entries < 1) return SS_ERR_INVALID_ARG;
    if (N == 0) return SS_OK;
    if (!rowptr || !order || !other || !x || !out || (root && !root_x)) return SS_ERR_INVALID_ARG;
    const int lanes = aggr_lanes(F);
    const int rows_per_block = (256 / kWave) * (kWave / lanes);
    const int64_t blocks = (N + rows_per_block - 1) / rows_per_block;
    if (gather_den)
        hipLaunchKernelGGL(aggr_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, order, other, w, gather_den, N,
                           hub_entries, x, (int)F, den, root, root_x, out, lanes);
    else
        hipLaunchKernelGGL(aggr_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, order, other, w, gather_den, N,
                           hub_entries, x, (int)F, den, root, root_x, out, lanes);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_aggr_hub_partials(const int64_t *rowptr, const int32_t *order, const int64_t *other, const float *w, int64_t N,
                                    const int32_t *hub_rows, const int32_t *hub_chunk, const int32_t *chunk_hub, int64_t n_hubs,
                                    int64_t n_chunks, const float *x, int32_t F, const float *gather_den, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    using namespace ss;
    if (!aggr_shape_ok(N, F) || n_hubs < 0 || n_chunks < 0 || n_chunks >= ((int64_t)1 << 31) || n_hubs > n_chunks) return SS_ERR_INVALID_ARG;
    if (N == 0 || n_chunks == 0) return SS_OK;
    if (!rowptr || !order || !other || !hub_rows || !hub_chunk || !chunk_hub || !x || !workspace) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_aggr_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    const int lanes = aggr_lanes(F);
    const int groups_per_block = (256 / kWave) * (kWave / lanes);
    const int64_t blocks = (n_chunks + groups_per_block - 1) / groups_per_block;
    float *ws = static_cast<float *>(workspace);
    if (gather_den)
        hipLaunchKernelGGL(aggr_hub_partials_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, order, other, w,
                           gather_den, N, hub_rows, hub_chunk, chunk_hub, n_hubs, n_chunks, x, (int)F, ws, lanes);
    else
        hipLaunchKernelGGL(aggr_hub_partials_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, order, other, w,
                           gather_den, N, hub_rows, hub_chunk, chunk_hub, n_hubs, n_chunks, x, (int)F, ws, lanes);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_aggr_hub_finish(const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs, int64_t n_chunks, int64_t N,
                                  const void *workspace, size_t workspace_bytes, int32_t F, const float *den, const float *root,
                                  const float *root_x, float *out, void *stream)
{
    using namespace ss;
    if (!aggr_shape_ok(N, F) || n_hubs < 0 || n_chunks < 0 || n_chunks >= ((int64_t)1 << 31) || n_hubs > n_chunks) return SS_ERR_INVALID_ARG;
    if (N == 0 || n_hubs == 0) return SS_OK;
    if (!hub_rows || !hub_chunk || !workspace || !out || (root && !root_x)) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_aggr_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    const int64_t blocks = (n_hubs * (F >> 2) + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(aggr_hub_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, hub_rows, hub_chunk, n_hubs, n_chunks, N,
                       static_cast<const float *>(workspace), (int)F, den, root, root_x, out);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
