// ss_link_decoder.hip -- the endpoint gather of a batch of links and its Hadamard product, forward and backward (reference
// runners/train.py:56, :63, :200, :201 `x[curr_links]`, models/elph.py:54 `x[:, 0, :] * x[:, 1, :]`, models/gnn.py:212 `x_i * x_j`):
//   gather    out[l, s] = x[links[l, s]]                          float32 [L, 2, F]
//   hadamard  out[l]    = x[links[l, 0]] * x[links[l, 1]]         float32 [L, F], one fp32 multiply; no [L, 2, F] tensor exists
// The gather idiom is that of ss_aggr.hip / ss_spmm.hip: a lane owns one piece of a feature row (a float4; a single float when
// F % 4 != 0 or a base is not 16-byte aligned), pow2(pieces) lanes (at most 64) form a row group, wider rows loop over piece bases,
// entries are fetched one per lane and handed out by shuffles, feature rows are requested four ahead, offsets are 64-bit.
//
// The backward groups the 2L endpoint slots q = 2l + s by node (link_decoder.LinkBatch: nodes, rowptr, order).  Row `node` of grad_x
// takes its slots q_0 < q_1 < ... in the accumulation order DESIGN 3.24 pins ss_aggr.hip to, chunks of SS_LINK_CHUNK = 256:
//   p_c = the sequential fp32 sum, from +0, of the terms of chunk c        s = ((0 + p_0) + p_1) + ...
//   term t_q = g[l, s, :] (gather)    or    fl(g[l, :] * x[links[l, 1 - s], :]) (product),    l = q >> 1, s = q & 1
// A self link (u, u) is two slots of u.  One lane per output element and chunk, products and adds rounded separately, no float
// atomics, no inter-workgroup waits.  Because a row IS its chunk sums added in chunk order, the chunks of a long row (more than
// hub_entries slots) are walked by other row groups (link_grad_hub_partials_kernel) and added afterwards (link_grad_hub_finish_kernel)
// without changing a bit: a row's bits depend on its own slots and their order alone.
#include "ss_common.hpp"
#include "ss_walks.hpp"

#define SS_LINK_CHUNK 256  // slots per chunk of the accumulation order; ss_link_chunk() tells it to callers

namespace ss {

constexpr int kLinkChunk = SS_LINK_CHUNK;

// a lane's piece of a feature row: V = float4 or float
template <class V>
__device__ __forceinline__ V link_zero();
template <>
__device__ __forceinline__ float4 link_zero<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
template <>
__device__ __forceinline__ float link_zero<float>() { return 0.0f; }
template <class V>
__device__ __forceinline__ V link_load(const float *row, int c) { return reinterpret_cast<const V *>(row)[c]; }
template <class V>
__device__ __forceinline__ void link_store(float *row, int c, V v) { reinterpret_cast<V *>(row)[c] = v; }
__device__ __forceinline__ float4 link_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float link_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 link_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float link_add(float a, float b) { return a + b; }
template <class V>
__host__ __device__ constexpr int link_width(int F) { return sizeof(V) == 16 ? F >> 2 : F; }

// the forwards: one row group per link (product) or per slot (gather).  An id outside [0, N) -- negative ones too -- is not followed:
// the row is zeros and *err_flag is raised.  No shuffles here, so a row group past the end simply leaves.
template <class V, bool kProduct>
__global__ __launch_bounds__(256) void link_forward_kernel(const int64_t *__restrict__ links, int64_t L, const float *__restrict__ x, int64_t N,
                                                           int F, float *__restrict__ out, int32_t *__restrict__ err_flag, int lanes)
{
    const int64_t item = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / lanes;
    const int cl = threadIdx.x % lanes;
    if (item >= (kProduct ? L : 2 * L)) return;
    const int W = link_width<V>(F);
    float *o = out + item * F;
    const int64_t u = kProduct ? links[2 * item] : links[item];
    const int64_t v = kProduct ? links[2 * item + 1] : u;
    if ((uint64_t)u < (uint64_t)N && (uint64_t)v < (uint64_t)N) {
        const float *xu = x + u * F, *xv = x + v * F;
        for (int c = cl; c < W; c += lanes) link_store<V>(o, c, kProduct ? link_mul(link_load<V>(xu, c), link_load<V>(xv, c)) : link_load<V>(xu, c));
    } else {
        if (cl == 0 && err_flag) *err_flag = 1;
        for (int c = cl; c < W; c += lanes) link_store<V>(o, c, link_zero<V>());
    }
}

// p_c for piece c of the slots at the group positions [a, b), 0 < b - a <= kLinkChunk: every lane of the row group calls it with the
// same (a, b).  A slot id outside [0, slots) and a partner id outside [0, N) are not followed (the plan reports them on the host);
// the loads such a lane issues all the same go to slot 0 and row 0, which exist.
template <class V, bool kProduct>
__device__ __forceinline__ V link_chunk_sum(const int32_t *__restrict__ order, const int64_t *__restrict__ links, int64_t slots, int64_t N,
                                            const float *__restrict__ g, const float *__restrict__ x, int F, int64_t a, int64_t b, int c, int cl,
                                            int base, int lanes)
{
    V p = link_zero<V>();
    for (int64_t j0 = a; j0 < b; j0 += lanes) {
        const int64_t j = j0 + cl;  // this lane's slot of the stretch
        const int64_t q_raw = order[j < b ? j : a];
        const bool q_ok = (uint64_t)q_raw < (uint64_t)slots;
        const int64_t q = q_ok ? q_raw : 0;
        bool in_range = true;
        int my_x = 0;
        if (kProduct) {
            const int64_t raw = links[q ^ 1];  // the other endpoint of link q >> 1
            in_range = (uint64_t)raw < (uint64_t)N;
            my_x = in_range ? (int)raw : 0;  // (N < 2^31)
        }
        const int my_g = (int)(kProduct ? q >> 1 : q);  // the row of g this slot's term comes from (slots < 2^31)
        const int my_use = j < b && q_ok && in_range;
        const int n = (int)(b - j0 < lanes ? b - j0 : lanes);
        for (int k0 = 0; k0 < n; k0 += 4) {  // (uniform per row group)
            V gr[4], xr[4];
            int use[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int src = base + (k0 + k < lanes ? k0 + k : 0);
                const int64_t gk = (int64_t)(uint32_t)__shfl(my_g, src);
                use[k] = k0 + k < n ? __shfl(my_use, src) : 0;
                gr[k] = link_load<V>(g + gk * F, c);
                if (kProduct) {
                    const int64_t xk = (int64_t)(uint32_t)__shfl(my_x, src);
                    xr[k] = link_load<V>(x + xk * F, c);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (use[k]) p = link_add(p, kProduct ? link_mul(gr[k], xr[k]) : gr[k]);
        }
    }
    return p;
}

// the regular tier: one row group per touched node walks the node's slots, chunk after chunk, and stores the row of grad_x.  Row
// groups past M shadow row M - 1 and do not store (the shuffles need every lane); rows of more than hub_entries slots belong to the
// hub tier and are left alone, as is a row whose pointer pair leaves [0, slots] or whose node is no row of grad_x.
template <class V, bool kProduct>
__global__ __launch_bounds__(256) void link_grad_rows_kernel(const int64_t *__restrict__ nodes, const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ order, int64_t M, const int64_t *__restrict__ links,
                                                             int64_t slots, int64_t N, int64_t hub_entries, const float *__restrict__ g,
                                                             const float *__restrict__ x, int F, float *__restrict__ grad_x, int lanes)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int rows_per_wave = kWave / lanes;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t r_raw = wave * rows_per_wave + lane / lanes;
    const int64_t r = r_raw < M ? r_raw : M - 1;
    const int cl = lane % lanes, base = lane - cl;
    const int64_t e0 = rowptr[r], e1 = rowptr[r + 1];
    if (e0 < 0 || e1 > slots || e1 < e0 || e1 - e0 > hub_entries) return;  // (the whole row group leaves)
    const int64_t node = nodes[r];
    const bool mine = r_raw < M && (uint64_t)node < (uint64_t)N;
    const int W = link_width<V>(F);
    for (int cbase = 0; cbase < W; cbase += lanes) {  // (one iteration unless the row has more than 64 pieces)
        const int c = cbase + cl < W ? cbase + cl : W - 1;  // lanes past the last piece read it and do not store, in every iteration
        V s = link_zero<V>();
        for (int64_t a = e0; a < e1; a += kLinkChunk) {
            const int64_t b = e1 - a < kLinkChunk ? e1 : a + kLinkChunk;
            s = link_add(s, link_chunk_sum<V, kProduct>(order, links, slots, N, g, x, F, a, b, c, cl, base, lanes));
        }
        if (mine && cbase + cl < W) link_store<V>(grad_x + node * F, c, s);
    }
}

// the hub tier, first launch: one row group per (hub row, chunk) writes p_c to row t of the workspace [n_chunks, F].  Chunk t belongs
// to hub chunk_hub[t], whose chunks are hub_chunk[h] .. hub_chunk[h + 1]; hub_rows[h] is the hub's position in nodes / rowptr.  A list
// entry that names no row of the plan, or no slots of its row, is not followed and writes nothing.
template <class V, bool kProduct>
__global__ __launch_bounds__(256) void link_grad_hub_partials_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ order, int64_t M,
                                                                     const int64_t *__restrict__ links, int64_t slots, int64_t N,
                                                                     const int32_t *__restrict__ hub_rows, const int32_t *__restrict__ hub_chunk,
                                                                     const int32_t *__restrict__ chunk_hub, int64_t n_hubs, int64_t n_chunks,
                                                                     const float *__restrict__ g, const float *__restrict__ x, int F,
                                                                     float *__restrict__ ws, int lanes)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int rows_per_wave = kWave / lanes;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t t_raw = wave * rows_per_wave + lane / lanes;
    const int64_t t = t_raw < n_chunks ? t_raw : n_chunks - 1;
    const int cl = lane % lanes, base = lane - cl;
    const int64_t h = chunk_hub[t];
    if ((uint64_t)h >= (uint64_t)n_hubs) return;
    const int64_t r = hub_rows[h];
    if ((uint64_t)r >= (uint64_t)M) return;
    const int64_t e0 = rowptr[r], e1 = rowptr[r + 1];
    const int64_t a = e0 + (t - hub_chunk[h]) * kLinkChunk;
    if (e0 < 0 || e1 > slots || a < e0 || a >= e1) return;
    const int64_t b = e1 - a < kLinkChunk ? e1 : a + kLinkChunk;
    const int W = link_width<V>(F);
    for (int cbase = 0; cbase < W; cbase += lanes) {
        const int c = cbase + cl < W ? cbase + cl : W - 1;
        const V p = link_chunk_sum<V, kProduct>(order, links, slots, N, g, x, F, a, b, c, cl, base, lanes);
        if (t_raw < n_chunks && cbase + cl < W) link_store<V>(ws + t * F, c, p);
    }
}

// the hub tier, second launch: one lane per piece of a hub row adds the row's partials in chunk order and stores the row
template <class V>
__global__ __launch_bounds__(256) void link_grad_hub_finish_kernel(const int64_t *__restrict__ nodes, int64_t M, const int32_t *__restrict__ hub_rows,
                                                                   const int32_t *__restrict__ hub_chunk, int64_t n_hubs, int64_t n_chunks, int64_t N,
                                                                   const float *__restrict__ ws, int F, float *__restrict__ grad_x)
{
    const int W = link_width<V>(F);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t h = i / W;
    const int c = (int)(i - h * W);
    if (h >= n_hubs) return;
    const int64_t r = hub_rows[h];
    if ((uint64_t)r >= (uint64_t)M) return;
    const int64_t node = nodes[r];
    if ((uint64_t)node >= (uint64_t)N) return;
    int64_t t0 = hub_chunk[h], t1 = hub_chunk[h + 1];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > n_chunks ? n_chunks : t1;
    V s = link_zero<V>();
    for (int64_t t = t0; t < t1; ++t) s = link_add(s, link_load<V>(ws + t * F, c));
    link_store<V>(grad_x + node * F, c, s);
}

// the launch shape of `items` row groups over rows of F floats: float4 pieces when F % 4 == 0 and every base is 16-byte aligned
struct LinkShape {
    bool vec;
    int lanes;
    int64_t blocks;
};
static inline LinkShape link_shape(int64_t items, int F, uintptr_t bases)
{
    LinkShape s;
    s.vec = (F & 3) == 0 && (bases & 15) == 0;
    s.lanes = pow2_ceil(s.vec ? F >> 2 : F);
    s.lanes = s.lanes > kWave ? kWave : s.lanes;
    const int per_block = (256 / kWave) * (kWave / s.lanes);
    s.blocks = (items + per_block - 1) / per_block;
    return s;
}

static inline bool link_sizes_ok(int64_t L, int64_t N, int32_t F)
{
    return L >= 0 && N >= 0 && F >= 0 && L < ((int64_t)1 << 30) && N < ((int64_t)1 << 31);
}
static inline bool link_hub_sizes_ok(int64_t n_hubs, int64_t n_chunks)
{
    return n_hubs >= 0 && n_chunks >= 0 && n_chunks < ((int64_t)1 << 31) && n_hubs <= n_chunks;
}

}  // namespace ss

// the float4 or the float instance of a kernel by the shape; SS_ERR_INVALID_ARG for a grid that does not fit
#define SS_LINK_LAUNCH(shape, vec_kernel, scalar_kernel, ...)                                                                  \
    do {                                                                                                                       \
        if ((shape).blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;                                                   \
        if ((shape).vec)                                                                                                       \
            hipLaunchKernelGGL(vec_kernel, dim3((unsigned)(shape).blocks), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);    \
        else                                                                                                                   \
            hipLaunchKernelGGL(scalar_kernel, dim3((unsigned)(shape).blocks), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        SS_LAUNCH_CHECK();                                                                                                     \
    } while (0)

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
    const LinkShape sh = link_shape(product ? L : 2 * L, F, (uintptr_t)x | (uintptr_t)out);
    if (product)
        SS_LINK_LAUNCH(sh, (link_forward_kernel<float4, true>), (link_forward_kernel<float, true>), links, L, x, N, (int)F, out, err_flag, sh.lanes);
    else
        SS_LINK_LAUNCH(sh, (link_forward_kernel<float4, false>), (link_forward_kernel<float, false>), links, L, x, N, (int)F, out, err_flag, sh.lanes);
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
    const LinkShape sh = link_shape(M, F, (uintptr_t)g | (uintptr_t)grad_x | (mode == 1 ? (uintptr_t)x : 0));
    if (mode == 1)
        SS_LINK_LAUNCH(sh, (link_grad_rows_kernel<float4, true>), (link_grad_rows_kernel<float, true>), nodes, rowptr, order, M, links, 2 * L, N, hub_entries, g, x, (int)F, grad_x,
                       sh.lanes);
    else
        SS_LINK_LAUNCH(sh, (link_grad_rows_kernel<float4, false>), (link_grad_rows_kernel<float, false>), nodes, rowptr, order, M, links, 2 * L, N, hub_entries, g, x, (int)F, grad_x,
                       sh.lanes);
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
    const LinkShape sh = link_shape(n_chunks, F, (uintptr_t)g | (uintptr_t)ws | (mode == 1 ? (uintptr_t)x : 0));
    if (mode == 1)
        SS_LINK_LAUNCH(sh, (link_grad_hub_partials_kernel<float4, true>), (link_grad_hub_partials_kernel<float, true>), rowptr, order, M, links, 2 * L, N, hub_rows, hub_chunk, chunk_hub,
                       n_hubs, n_chunks, g, x, (int)F, ws, sh.lanes);
    else
        SS_LINK_LAUNCH(sh, (link_grad_hub_partials_kernel<float4, false>), (link_grad_hub_partials_kernel<float, false>), rowptr, order, M, links, 2 * L, N, hub_rows, hub_chunk, chunk_hub,
                       n_hubs, n_chunks, g, x, (int)F, ws, sh.lanes);
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
    LinkShape sh = link_shape(0, F, (uintptr_t)ws | (uintptr_t)grad_x);
    sh.blocks = (n_hubs * (sh.vec ? F >> 2 : F) + 255) / 256;  // one lane per piece
    SS_LINK_LAUNCH(sh, link_grad_hub_finish_kernel<float4>, link_grad_hub_finish_kernel<float>, nodes, M, hub_rows, hub_chunk, n_hubs, n_chunks, N, ws, (int)F, grad_x);
    return SS_OK;
}
