// ss_aggr.hip -- unnormalised neighbour aggregation for SAGEConv and GINConv (reference models/seal.py:116-173, 259-328 and
// models/gnn.py:90-113) [PyG semantics restated]: out[dst_e] (+)= w_e * x[src_e] over the edges as they are -- no gcn_norm, existing
// self loops are ordinary entries, no loop is added -- then a division by the row's weight sum (mean) and / or a root term
// (1 + eps) * x_i (GIN).  The gather idiom, the accumulation order the family is pinned to and the three tier kernels are
// those of ss_feature_rows.hpp; this unit says what a term is and what follows the sum:
//   term t_e = fl(w_e * v_e) (unit weights: w is never gathered, the bits are those of * 1), v_e = x[src_e], or fl(x[src_e] / d[src_e])
//   when a gather divisor is given (the mean's backward); after the sum the mean's division, then the root term.
#include "ss_feature_rows.hpp"

#define SS_AGGR_CHUNK 256  // entries per chunk of the accumulation order; ss_aggr_chunk() tells it to callers
static_assert(SS_AGGR_CHUNK == ss::kRowChunk, "the tier kernels of ss_feature_rows.hpp sum chunks of kRowChunk entries");

namespace ss {

constexpr int kAggrChunk = SS_AGGR_CHUNK;

struct AggrArgs {
    const int32_t *order;
    const int64_t *other;
    const float *w, *gden;
    int64_t N, rows;  // (rows == N: every node owns its row of out)
    const float *x;
    int F;
    const float *den, *root, *root_x;
    float *out;
};

// an entry is an edge index e = order[j]; its row other[e] of x is not followed when it lies outside [0, N) (the plan reports it on the
// host): such a lane's loads go to the group's own row i
template <bool kDiv>
struct AggrTerms : AggrArgs {
    using V = float4;
    using Args = AggrArgs;
    struct Entry {
        int64_t c;
        float w, d;
        int use;
    };
    struct Term {
        float4 r;
        float w, d;
        int use;
    };
    __device__ __forceinline__ Entry fetch(int64_t i, int64_t j, bool live) const
    {
        const int32_t e = order[j];
        const int64_t raw = other[e];
        const bool in_range = (uint64_t)raw < (uint64_t)N;
        Entry m;
        m.c = in_range ? raw : i;
        m.w = w ? w[e] : 1.0f;
        m.d = kDiv ? gden[m.c] : 1.0f;
        m.use = live && in_range;
        return m;
    }
    __device__ __forceinline__ Term request(int64_t i, const Entry &m, int src, bool live, int c) const
    {
        Term t;
        const int64_t cj = shfl64(m.c, src);
        t.w = __shfl(m.w, src);
        t.d = kDiv ? __shfl(m.d, src) : 1.0f;
        t.use = live ? __shfl(m.use, src) : 0;
        t.r = piece_load<float4>(x + (t.use ? cj : i) * F, c);
        return t;
    }
    __device__ __forceinline__ float4 add(float4 p, const Term &t) const
    {
        return piece_add(p, piece_mul(kDiv ? piece_div(t.r, t.d) : t.r, t.w));
    }
    __device__ __forceinline__ bool span_ok(int64_t, int64_t) const { return true; }
    __device__ __forceinline__ int64_t out_row(int64_t r) const { return r; }
    // what follows the sum of a row: the mean's division, then the root term
    __device__ __forceinline__ float4 finish(float4 s, int64_t i, int c) const
    {
        if (den) s = piece_div(s, den[i]);
        if (root) s = piece_add(s, piece_mul(piece_load<float4>(root_x + i * F, c), *root));
        return s;
    }
};

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
    const AggrArgs args{order, other, w, gather_den, N, N, x, (int)F, den, root, root_x, out};
    const RowShape sh = row_shape(N, F, 0);
    if (gather_den)
        hipLaunchKernelGGL(chunked_rows_kernel<AggrTerms<true>>, dim3((unsigned)sh.blocks), dim3(256), 0, (hipStream_t)stream, args, rowptr,
                           hub_entries, sh.lanes);
    else
        hipLaunchKernelGGL(chunked_rows_kernel<AggrTerms<false>>, dim3((unsigned)sh.blocks), dim3(256), 0, (hipStream_t)stream, args, rowptr,
                           hub_entries, sh.lanes);
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
    const AggrArgs args{order, other, w, gather_den, N, N, x, (int)F, nullptr, nullptr, nullptr, nullptr};
    const RowShape sh = row_shape(n_chunks, F, 0);
    float *ws = static_cast<float *>(workspace);
    if (gather_den)
        hipLaunchKernelGGL(chunked_hub_partials_kernel<AggrTerms<true>>, dim3((unsigned)sh.blocks), dim3(256), 0, (hipStream_t)stream, args, rowptr,
                           hub_rows, hub_chunk, chunk_hub, n_hubs, n_chunks, ws, sh.lanes);
    else
        hipLaunchKernelGGL(chunked_hub_partials_kernel<AggrTerms<false>>, dim3((unsigned)sh.blocks), dim3(256), 0, (hipStream_t)stream, args, rowptr,
                           hub_rows, hub_chunk, chunk_hub, n_hubs, n_chunks, ws, sh.lanes);
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
    const int64_t blocks = (n_hubs * (F >> 2) + 255) / 256;  // one lane per piece
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    const AggrArgs args{nullptr, nullptr, nullptr, nullptr, N, N, nullptr, (int)F, den, root, root_x, out};
    hipLaunchKernelGGL(chunked_hub_finish_kernel<AggrTerms<false>>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, args, hub_rows,
                       hub_chunk, n_hubs, n_chunks, static_cast<const float *>(workspace));
    SS_LAUNCH_CHECK();
    return SS_OK;
}
