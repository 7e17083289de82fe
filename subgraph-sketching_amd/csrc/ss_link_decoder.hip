// ss_link_decoder.hip -- the endpoint gather of a batch of links and its Hadamard product, forward and backward (reference
// runners/train.py:56, :63, :200, :201 `x[curr_links]`, models/elph.py:54 `x[:, 0, :] * x[:, 1, :]`, models/gnn.py:212 `x_i * x_j`):
//   gather    out[l, s] = x[links[l, s]]                          float32 [L, 2, F]
//   hadamard  out[l]    = x[links[l, 0]] * x[links[l, 1]]         float32 [L, F], one fp32 multiply; no [L, 2, F] tensor exists
// The gather idiom (a lane owns one piece of a feature row, a float4 or a single float; pow2(pieces) lanes form a row group) is that of
// ss_feature_rows.hpp, as are the accumulation order of the backward and its three tier kernels.
//
// The backward groups the 2L endpoint slots q = 2l + s by node (link_decoder.LinkBatch: nodes, rowptr, order).  Row `node` of grad_x
// takes its slots q_0 < q_1 < ... in the accumulation order of DESIGN 3.24, chunks of SS_LINK_CHUNK = 256:
//   p_c = the sequential fp32 sum, from +0, of the terms of chunk c        s = ((0 + p_0) + p_1) + ...
//   term t_q = g[l, s, :] (gather)    or    fl(g[l, :] * x[links[l, 1 - s], :]) (product),    l = q >> 1, s = q & 1
// A self link (u, u) is two slots of u.  One lane per output element and chunk, products and adds rounded separately, no float
// atomics, no inter-workgroup waits.  Because a row IS its chunk sums added in chunk order, the chunks of a long row (more than
// hub_entries slots) are walked by other row groups (chunked_hub_partials_kernel) and added afterwards (chunked_hub_finish_kernel)
// without changing a bit: a row's bits depend on its own slots and their order alone.
#include "ss_feature_rows.hpp"

#define SS_LINK_CHUNK 256  // slots per chunk of the accumulation order; ss_link_chunk() tells it to callers
static_assert(SS_LINK_CHUNK == ss::kRowChunk, "the tier kernels of ss_feature_rows.hpp sum chunks of kRowChunk entries");

namespace ss {

// the forwards: one row group per link (product) or per slot (gather).  An id outside [0, N) -- negative ones too -- is not followed:
// the row is zeros and *err_flag is raised.  No shuffles here, so a row group past the end simply leaves.
template <class V, bool kProduct>
__global__ __launch_bounds__(256) void link_forward_kernel(const int64_t *__restrict__ links, int64_t L, const float *__restrict__ x, int64_t N,
                                                           int F, float *__restrict__ out, int32_t *__restrict__ err_flag, int lanes)
{
    const int64_t item = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / lanes;
    const int cl = threadIdx.x % lanes;
    if (item >= (kProduct ? L : 2 * L)) return;
    const int W = piece_width<V>(F);
    float *o = out + item * F;
    const int64_t u = kProduct ? links[2 * item] : links[item];
    const int64_t v = kProduct ? links[2 * item + 1] : u;
    if ((uint64_t)u < (uint64_t)N && (uint64_t)v < (uint64_t)N) {
        const float *xu = x + u * F, *xv = x + v * F;
        for (int c = cl; c < W; c += lanes) piece_store<V>(o, c, kProduct ? piece_mul(piece_load<V>(xu, c), piece_load<V>(xv, c)) : piece_load<V>(xu, c));
    } else {
        if (cl == 0 && err_flag) *err_flag = 1;
        for (int c = cl; c < W; c += lanes) piece_store<V>(o, c, piece_zero<V>());
    }
}

struct LinkArgs {
    const int64_t *nodes;
    const int32_t *order;
    const int64_t *links;
    int64_t slots, N, rows;  // (rows: M, the touched nodes)
    const float *g, *x;
    int F;
    float *out;  // grad_x
};

// an entry is a slot q = order[j].  A slot id outside [0, slots) and a partner id outside [0, N) are not followed (the plan reports them
// on the host); the loads such a lane issues all the same go to slot 0 and row 0, which exist.  A row whose pointer pair leaves
// [0, slots], or whose node is no row of grad_x, is left alone.
template <class Piece, bool kProduct>
struct LinkTerms : LinkArgs {
    using V = Piece;
    using Args = LinkArgs;
    struct Entry {
        int g, x, use;
    };
    struct Term {
        V g, x;
        int use;
    };
    __device__ __forceinline__ Entry fetch(int64_t, int64_t j, bool live) const
    {
        const int64_t q_raw = order[j];
        const bool q_ok = (uint64_t)q_raw < (uint64_t)slots;
        const int64_t q = q_ok ? q_raw : 0;
        bool in_range = true;
        Entry m;
        m.x = 0;
        if (kProduct) {
            const int64_t raw = links[q ^ 1];  // the other endpoint of link q >> 1
            in_range = (uint64_t)raw < (uint64_t)N;
            m.x = in_range ? (int)raw : 0;  // (N < 2^31)
        }
        m.g = (int)(kProduct ? q >> 1 : q);  // the row of g this slot's term comes from (slots < 2^31)
        m.use = live && q_ok && in_range;
        return m;
    }
    __device__ __forceinline__ Term request(int64_t, const Entry &m, int src, bool live, int c) const
    {
        Term t;
        const int64_t gk = (int64_t)(uint32_t)__shfl(m.g, src);
        t.use = live ? __shfl(m.use, src) : 0;
        t.g = piece_load<V>(g + gk * F, c);
        if (kProduct) {
            const int64_t xk = (int64_t)(uint32_t)__shfl(m.x, src);
            t.x = piece_load<V>(x + xk * F, c);
        }
        return t;
    }
    __device__ __forceinline__ V add(V p, const Term &t) const { return piece_add(p, kProduct ? piece_mul(t.g, t.x) : t.g); }
    __device__ __forceinline__ bool span_ok(int64_t e0, int64_t e1) const { return e0 >= 0 && e1 <= slots && e1 >= e0; }
    __device__ __forceinline__ int64_t out_row(int64_t r) const { return nodes[r]; }
    __device__ __forceinline__ V finish(V s, int64_t, int) const { return s; }
};

static inline bool link_sizes_ok(int64_t L, int64_t N, int32_t F)
{
    return L >= 0 && N >= 0 && F >= 0 && L < ((int64_t)1 << 30) && N < ((int64_t)1 << 31);
}
static inline bool link_hub_sizes_ok(int64_t n_hubs, int64_t n_chunks)
{
    return n_hubs >= 0 && n_chunks >= 0 && n_chunks < ((int64_t)1 << 31) && n_hubs <= n_chunks;
}

}  // namespace ss

extern "C" int ss_link_chunk(void) { return SS_LINK_CHUNK; }

extern "C" size_t ss_link_workspace_bytes(int64_t hub_chunks, int32_t F)
{
    if (hub_chunks < 0 || F <= 0 || hub_chunks >= ((int64_t)1 << 31)) return 0;
    return (size_t)hub_chunks * (size_t)F * sizeof(float);
}

static int link_forward(bool product, const int64_t *links, int64_t L, const float *x, int64_t N, int32_t F, float *out, int32_t *err_flag,
                        void *stream)
{
    using namespace ss;
    if (!link_sizes_ok(L, N, F)) return SS_ERR_INVALID_ARG;
    if (L == 0 || F == 0) return SS_OK;  // (without columns the ids are not looked at: there is no row to refuse)
    if (!links || !out || (N > 0 && !x)) return SS_ERR_INVALID_ARG;
    const RowShape sh = row_shape(product ? L : 2 * L, F, (uintptr_t)x | (uintptr_t)out);
    if (product)
        SS_ROWS_LAUNCH(sh, (link_forward_kernel<float4, true>), (link_forward_kernel<float, true>), links, L, x, N, (int)F, out, err_flag, sh.lanes);
    else
        SS_ROWS_LAUNCH(sh, (link_forward_kernel<float4, false>), (link_forward_kernel<float, false>), links, L, x, N, (int)F, out, err_flag, sh.lanes);
    return SS_OK;
}

extern "C" int ss_link_gather(const int64_t *links, int64_t L, const float *x, int64_t N, int32_t F, float *out, int32_t *err_flag, void *stream)
{
    return link_forward(false, links, L, x, N, F, out, err_flag, stream);
}

extern "C" int ss_link_hadamard(const int64_t *links, int64_t L, const float *x, int64_t N, int32_t F, float *out, int32_t *err_flag, void *stream)
{
    return link_forward(true, links, L, x, N, F, out, err_flag, stream);
}

extern "C" int ss_link_grad_rows(const int64_t *nodes, const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *links, int64_t L,
                                 int64_t N, int64_t hub_entries, int32_t mode, const float *g, const float *x, int32_t F, float *grad_x,
                                 void *stream)
{
    using namespace ss;
    if (!link_sizes_ok(L, N, F) || M < 0 || M > N || M > 2 * L || hub_entries < 1 || (mode != 0 && mode != 1)) return SS_ERR_INVALID_ARG;
    if (M == 0 || F == 0) return SS_OK;
    if (!nodes || !rowptr || !order || !links || !g || !grad_x || (mode == 1 && !x)) return SS_ERR_INVALID_ARG;
    const RowShape sh = row_shape(M, F, (uintptr_t)g | (uintptr_t)grad_x | (mode == 1 ? (uintptr_t)x : 0));
    const LinkArgs args{nodes, order, links, 2 * L, N, M, g, x, (int)F, grad_x};
    if (mode == 1)
        SS_ROWS_LAUNCH(sh, (chunked_rows_kernel<LinkTerms<float4, true>>), (chunked_rows_kernel<LinkTerms<float, true>>), args, rowptr, hub_entries, sh.lanes);
    else
        SS_ROWS_LAUNCH(sh, (chunked_rows_kernel<LinkTerms<float4, false>>), (chunked_rows_kernel<LinkTerms<float, false>>), args, rowptr, hub_entries, sh.lanes);
    return SS_OK;
}

extern "C" int ss_link_grad_hub_partials(const int64_t *rowptr, const int32_t *order, int64_t M, const int64_t *links, int64_t L, int64_t N,
                                         const int32_t *hub_rows, const int32_t *hub_chunk, const int32_t *chunk_hub, int64_t n_hubs,
                                         int64_t n_chunks, int32_t mode, const float *g, const float *x, int32_t F, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    using namespace ss;
    if (!link_sizes_ok(L, N, F) || M < 0 || M > N || M > 2 * L || !link_hub_sizes_ok(n_hubs, n_chunks) || (mode != 0 && mode != 1))
        return SS_ERR_INVALID_ARG;
    if (M == 0 || F == 0 || n_chunks == 0) return SS_OK;
    if (!rowptr || !order || !links || !hub_rows || !hub_chunk || !chunk_hub || !g || !workspace || (mode == 1 && !x)) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_link_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    float *ws = static_cast<float *>(workspace);
    const RowShape sh = row_shape(n_chunks, F, (uintptr_t)g | (uintptr_t)ws | (mode == 1 ? (uintptr_t)x : 0));
    const LinkArgs args{nullptr, order, links, 2 * L, N, M, g, x, (int)F, nullptr};
    if (mode == 1)
        SS_ROWS_LAUNCH(sh, (chunked_hub_partials_kernel<LinkTerms<float4, true>>), (chunked_hub_partials_kernel<LinkTerms<float, true>>), args, rowptr, hub_rows, hub_chunk,
                       chunk_hub, n_hubs, n_chunks, ws, sh.lanes);
    else
        SS_ROWS_LAUNCH(sh, (chunked_hub_partials_kernel<LinkTerms<float4, false>>), (chunked_hub_partials_kernel<LinkTerms<float, false>>), args, rowptr, hub_rows, hub_chunk,
                       chunk_hub, n_hubs, n_chunks, ws, sh.lanes);
    return SS_OK;
}

extern "C" int ss_link_grad_hub_finish(const int64_t *nodes, int64_t M, const int32_t *hub_rows, const int32_t *hub_chunk, int64_t n_hubs,
                                       int64_t n_chunks, int64_t N, const void *workspace, size_t workspace_bytes, int32_t F, float *grad_x,
                                       void *stream)
{
    using namespace ss;
    if (N < 0 || N >= ((int64_t)1 << 31) || F < 0 || M < 0 || M > N || !link_hub_sizes_ok(n_hubs, n_chunks)) return SS_ERR_INVALID_ARG;
    if (M == 0 || F == 0 || n_hubs == 0) return SS_OK;
    if (!nodes || !hub_rows || !hub_chunk || !workspace || !grad_x) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_link_workspace_bytes(n_chunks, F)) return SS_ERR_INVALID_ARG;
    const float *ws = static_cast<const float *>(workspace);
    RowShape sh = row_shape(0, F, (uintptr_t)ws | (uintptr_t)grad_x);
    sh.blocks = (n_hubs * (sh.vec ? F >> 2 : F) + 255) / 256;  // one lane per piece
    const LinkArgs args{nodes, nullptr, nullptr, 0, N, M, nullptr, nullptr, (int)F, grad_x};
    SS_ROWS_LAUNCH(sh, (chunked_hub_finish_kernel<LinkTerms<float4, false>>), (chunked_hub_finish_kernel<LinkTerms<float, false>>), args, hub_rows, hub_chunk, n_hubs, n_chunks, ws);
    return SS_OK;
}
