// ss_cn_rows.hip -- node features pooled over a list of weighted entries per link, forward and backward: the trainable form of the
// common-neighbour readout (Neural Common Neighbour: the sum of LEARNED embeddings h[w] over a link's common neighbours).  A list is
// (rowptr int64 [L + 1], ids int64 [T], coef fp32 [T]), the shape heuristics.common_neighbours returns; entry k belongs to link
// owner[k], the q with rowptr[q] <= k < rowptr[q + 1]:
//   forward   out[q, :]    = the chunked sum of fl(coef[k] * x[ids[k], :])   over k = rowptr[q] .. rowptr[q + 1] - 1, list order
//   backward  grad_x[n, :] = the chunked sum of fl(coef[k] * g[owner[k], :]) over the entries with ids[k] == n, ascending k
// The chunked sum, its two tiers and the gather idiom are those of ss_feature_rows.hpp: chunks of SS_CN_ROWS_CHUNK = 256
// entries summed sequentially from +0, the chunk sums added in chunk order; one lane per output element and chunk, products and adds
// rounded separately, no float atomics, no inter-workgroup waits.  A row's bits depend on its own entries and their order alone.
// ss_cn_pool.hip's ss_common_neighbour_pool is the inference form: one sequential sum, straight off the CSR, no list.
#include "ss_feature_rows.hpp"

#define SS_CN_ROWS_CHUNK 256  // entries per chunk of the accumulation order; ss_cn_rows_chunk() tells it to callers
static_assert(SS_CN_ROWS_CHUNK == ss::kRowChunk, "the tier kernels of ss_feature_rows.hpp sum chunks of kRowChunk entries");

namespace ss {

struct CnRowsArgs {
    const int64_t *nodes;  // (backward) the row of grad_x every row of rowptr owns
    const int32_t *order;  // (backward) the list positions of every node, ascending
    const int64_t *from;   // per list position the row of src its term reads: ids (forward), owner (backward)
    const float *coef;
    int64_t T, S, N, rows;  // list entries; rows of src; rows of out; rows of rowptr (forward L, backward M)
    const float *src;       // x (forward), g (backward)
    int F;
    float *out;
};

// an entry is a list position k: j itself (forward), order[j] (backward).  A position outside [0, T) and a source row outside [0, S)
// are not followed (the plan reports them on the host); the loads such a lane issues all the same go to position 0 and row 0, which
// exist.  A row whose pointer pair leaves [0, T], or whose output row is no row of out, is left alone.
template <class Piece, bool kGrad>
struct CnRowsTerms : CnRowsArgs {
    using V = Piece;
    using Args = CnRowsArgs;
    struct Entry {
        int src, use;
        float coef;
    };
    struct Term {
        V x;
        float coef;
        int use;
    };
    __device__ __forceinline__ Entry fetch(int64_t, int64_t j, bool live) const
    {
        const int64_t k_raw = kGrad ? (int64_t)order[j] : j;
        const bool k_ok = (uint64_t)k_raw < (uint64_t)T;
        const int64_t k = k_ok ? k_raw : 0;
        const int64_t raw = from[k];
        const bool in_range = (uint64_t)raw < (uint64_t)S;
        Entry m;
        m.src = in_range ? (int)raw : 0;  // (S < 2^31)
        m.coef = coef[k];
        m.use = live && k_ok && in_range;
        return m;
    }
    __device__ __forceinline__ Term request(int64_t, const Entry &m, int src_lane, bool live, int c) const
    {
        Term t;
        const int64_t row = (int64_t)(uint32_t)__shfl(m.src, src_lane);
        t.coef = __shfl(m.coef, src_lane);
        t.use = live ? __shfl(m.use, src_lane) : 0;
        t.x = piece_load<V>(src + row * F, c);
        return t;
    }
    __device__ __forceinline__ V add(V p, const Term &t) const { return piece_add(p, piece_mul(t.x, t.coef)); }
    __device__ __forceinline__ bool span_ok(int64_t e0, int64_t e1) const { return e0 >= 0 && e1 <= T && e1 >= e0; }
    __device__ __forceinline__ int64_t out_row(int64_t r) const { return kGrad ? nodes[r] : r; }
    __device__ __forceinline__ V finish(V s, int64_t, int) const { return s; }
};

static inline bool cn_rows_sizes_ok(int64_t T, int64_t L, int64_t N, int32_t F)
{
    const int64_t lim = (int64_t)1 << 31;
    return T >= 0 && L >= 0 && N >= 0 && F >= 0 && T < lim && L < lim && N < lim;
}
static inline bool cn_rows_hub_sizes_ok(int64_t n_hubs, int64_t n_chunks)
{
    return n_hubs >= 0 && n_chunks >= 0 && n_chunks < ((int64_t)1 << 31) && n_hubs <= n_chunks;
}

// the three launches of either direction; `rows` row groups of rowptr, out with out_rows rows
template <bool kGrad>
static int cn_rows_regular(const CnRowsArgs &args, const int64_t *rowptr, int64_t hub_entries, void *stream)
{
    const RowShape sh = row_shape(args.rows, args.F, (uintptr_t)args.src | (uintptr_t)args.out);
    SS_ROWS_LAUNCH(sh, (chunked_rows_kernel<CnRowsTerms<float4, kGrad>>), (chunked_rows_kernel<CnRowsTerms<float, kGrad>>), args, rowptr, hub_entries,
                   sh.lanes);
    return SS_OK;
}

template <bool kGrad>
static int cn_rows_partials(const CnRowsArgs &args, const int64_t *rowptr, const int32_t *hub_rows, const int32_t *hub_chunk,
                            const int32_t *chunk_hub, int64_t n_hubs, int64_t n_chunks, float *ws, void *stream)
{
    const RowShape sh = row_shape(n_chunks, args.F, (uintptr_t)args.src | (uintptr_t)ws);
    SS_ROWS_LAUNCH(sh, (chunked_hub_partials_kernel<CnRowsTerms<float4, kGrad>>), (chunked_hub_partials_kernel<CnRowsTerms<float, kGrad>>), args, rowptr,
                   hub_rows, hub_chunk, chunk_hub, n_hubs, n_chunks, ws, sh.lanes);
    return SS_OK;
}

template <bool kGrad>
static int cn_rows_finish(const CnRowsArgs &args, const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs, int64_t n_chunks,
                          const float *ws, void *stream)
{
    RowShape sh = row_shape(0, args.F, (uintptr_t)ws | (uintptr_t)args.out);
    sh.blocks = (n_hubs * (sh.vec ? args.F >> 2 : args.F) + 255) / 256;  // one lane per piece
    SS_ROWS_LAUNCH(sh, (chunked_hub_finish_kernel<CnRowsTerms<float4, kGrad>>), (chunked_hub_finish_kernel<CnRowsTerms<float, kGrad>>), args, hub_rows,
                   hub_chunk, n_hubs, n_chunks, ws);
    return SS_OK;
}

}  // namespace ss

extern "C" int ss_cn_rows_chunk(void) { return SS_CN_ROWS_CHUNK; }

extern "C" size_t ss_cn_rows_workspace_bytes(int64_t hub_chunks, int32_t F)
{
    if (hub_chunks < 0 || F <= 0 || hub_chunks >= ((int64_t)1 << 31)) return 0;
    return (size_t)hub_chunks * (size_t)F * sizeof(float);
}

extern "C" int ss_cn_rows_forward(const int64_t *rowptr, const int64_t *ids, const float *coef, int64_t L, int64_t T, int64_t N,
                                  int64_t hub_entries, const float *x, int32_t F, float *out, void *stream)
{
    using namespace ss;
    if (!cn_rows_sizes_ok(T, L, N, F) || hub_entries < 1) return SS_ERR_INVALID_ARG;
    if (L == 0 || F == 0) return SS_OK;
    if (!rowptr || !out || (T > 0 && (!ids || !coef || !x))) return SS_ERR_INVALID_ARG;
    const CnRowsArgs args{nullptr, nullptr, ids, coef, T, N, L, L, x, (int)F, out};
    return cn_rows_regular<false>(args, rowptr, hub_entries, stream);
}

extern "C" int ss_cn_rows_forward_hub_partials(const int64_t *rowptr, const int64_t *ids, const float *coef, int64_t L, int64_t T, int64_t N,
                                               const int32_t *hub_rows, const int32_t *hub_chunk, const int32_t *chunk_hub, int64_t n_hubs,
                                               int64_t n_chunks, const float *x, int32_t F, void *workspace, size_t workspace_bytes,
                                               void *stream)
{
    using namespace ss;
    if (!cn_rows_sizes_ok(T, L, N, F) || !cn_rows_hub_sizes_ok(n_hubs, n_chunks)) return SS_ERR_INVALID_ARG;
    if (L == 0 || T == 0 || F == 0 || n_chunks == 0) return SS_OK;
    if (!rowptr || !ids || !coef || !hub_rows || !hub_chunk || !chunk_hub || !x || !workspace) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_cn_rows_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    const CnRowsArgs args{nullptr, nullptr, ids, coef, T, N, L, L, x, (int)F, nullptr};
    return cn_rows_partials<false>(args, rowptr, hub_rows, hub_chunk, chunk_hub, n_hubs, n_chunks, static_cast<float *>(workspace), stream);
}

extern "C" int ss_cn_rows_forward_hub_finish(int64_t L, const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs, int64_t n_chunks,
                                             const void *workspace, size_t workspace_bytes, int32_t F, float *out, void *stream)
{
    using namespace ss;
    if (L < 0 || L >= ((int64_t)1 << 31) || F < 0 || !cn_rows_hub_sizes_ok(n_hubs, n_chunks)) return SS_ERR_INVALID_ARG;
    if (L == 0 || F == 0 || n_hubs == 0) return SS_OK;
    if (!hub_rows || !hub_chunk || !workspace || !out) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_cn_rows_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    const CnRowsArgs args{nullptr, nullptr, nullptr, nullptr, 0, 0, L, L, nullptr, (int)F, out};
    return cn_rows_finish<false>(args, hub_rows, hub_chunk, n_hubs, n_chunks, static_cast<const float *>(workspace), stream);
}

extern "C" int ss_cn_rows_grad(const int64_t *nodes, const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *owner,
                               const float *coef, int64_t T, int64_t L, int64_t N, int64_t hub_entries, const float *g, int32_t F,
                               float *grad_x, void *stream)
{
    using namespace ss;
    if (!cn_rows_sizes_ok(T, L, N, F) || M < 0 || M > N || M > T || hub_entries < 1) return SS_ERR_INVALID_ARG;
    if (M == 0 || F == 0) return SS_OK;
    if (!nodes || !rowptr || !order || !owner || !coef || !g || !grad_x) return SS_ERR_INVALID_ARG;
    const CnRowsArgs args{nodes, order, owner, coef, T, L, N, M, g, (int)F, grad_x};
    return cn_rows_regular<true>(args, rowptr, hub_entries, stream);
}

extern "C" int ss_cn_rows_grad_hub_partials(const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *owner, const float *coef,
                                            int64_t T, int64_t L, int64_t N, const int32_t *hub_rows, const int32_t *hub_chunk,
                                            const int32_t *chunk_hub, int64_t n_hubs, int64_t n_chunks, const float *g, int32_t F,
                                            void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ss;
    if (!cn_rows_sizes_ok(T, L, N, F) || M < 0 || M > N || M > T || !cn_rows_hub_sizes_ok(n_hubs, n_chunks)) return SS_ERR_INVALID_ARG;
    if (M == 0 || F == 0 || n_chunks == 0) return SS_OK;
    if (!rowptr || !order || !owner || !coef || !hub_rows || !hub_chunk || !chunk_hub || !g || !workspace) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_cn_rows_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    const CnRowsArgs args{nullptr, order, owner, coef, T, L, N, M, g, (int)F, nullptr};
    return cn_rows_partials<true>(args, rowptr, hub_rows, hub_chunk, chunk_hub, n_hubs, n_chunks, static_cast<float *>(workspace), stream);
}

extern "C" int ss_cn_rows_grad_hub_finish(const int64_t *nodes, int64_t M, const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs,
                                          int64_t n_chunks, int64_t N, const void *workspace, size_t workspace_bytes, int32_t F,
                                          float *grad_x, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= ((int64_t)1 << 31) || F < 0 || M < 0 || M > N || !cn_rows_hub_sizes_ok(n_hubs, n_chunks)) return SS_ERR_INVALID_ARG;
    if (M == 0 || F == 0 || n_hubs == 0) return SS_OK;
    if (!nodes || !hub_rows || !hub_chunk || !workspace || !grad_x) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_cn_rows_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    const CnRowsArgs args{nodes, nullptr, nullptr, nullptr, 0, 0, N, M, nullptr, (int)F, grad_x};
    return cn_rows_finish<true>(args, hub_rows, hub_chunk, n_hubs, n_chunks, static_cast<const float *>(workspace), stream);
}
