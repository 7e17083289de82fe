// ss_feature_rows.hpp -- what the feature-row kernels share (ss_spmm.hip, ss_aggr.hip, ss_link_decoder.hip, ss_pool.hip): a lane's piece
// of a feature row and its arithmetic, the launch shape of row groups, the row-group preamble, the gather loop and the chunked row sum
// with its two tiers.
//
// The gather idiom: a lane owns one piece of a feature row (a float4; a single float when F % 4 != 0 or a base is not 16-byte aligned),
// pow2(pieces) lanes (at most 64) form a row group, wider rows loop over piece bases, entries are fetched one per lane and handed out by
// shuffles, feature rows are requested four ahead, offsets are 64-bit.
//
// The chunked row sum: output row i with the entries e_0 < e_1 < ... in chunks of kRowChunk = 256:
//   p_c = the sequential fp32 sum, from +0, of the terms of chunk c        s = ((0 + p_0) + p_1) + ...
// One lane per output element and chunk, products and adds rounded separately, no float atomics, no inter-workgroup waits.  Because a
// row IS its chunk sums added in chunk order, the chunks of a long row (a hub: more than hub_entries entries) can be walked by other row
// groups (chunked_hub_partials_kernel) and added afterwards (chunked_hub_finish_kernel) without changing a bit: a row's bits do not
// depend on the tier.  What an entry is, which output row a group owns and what follows the sum is the TERMS type's business:
//   V                                the piece type
//   Args                             the kernel argument (a plain struct the Terms type derives from), with rows, N, F, out
//   Entry fetch(row, j, live)        this lane's entry: position j of the order (live: j is one of the stretch, else a stand-in)
//   Term request(row, entry, src, live, c)   the entry of lane src, handed out, with the loads of piece c it needs issued; .use: it counts
//   V add(p, term)                   p + the term
//   span_ok(e0, e1), out_row(r), finish(s, row, c)   (the tier kernels only) a pointer pair to follow, the row of `out` that group r
//                                    owns, what follows the sum
#pragma once
#include "ss_common.hpp"
#include "ss_walks.hpp"

namespace ss {

constexpr int kRowChunk = 256;  // entries per chunk of the accumulation order (SS_AGGR_CHUNK, SS_LINK_CHUNK)

// ---- a lane's piece of a feature row: V = float4 or float -------------------------------------------------------------------------
template <class V> __device__ __forceinline__ V piece_zero();
template <> __device__ __forceinline__ float piece_zero<float>() { return 0.0f; }
template <> __device__ __forceinline__ float4 piece_zero<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float piece_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 piece_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float piece_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 piece_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 piece_mul(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float piece_div(float a, float d) { return a / d; }
__device__ __forceinline__ float4 piece_div(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }
template <class V> __host__ __device__ constexpr int piece_width(int F) { return sizeof(V) == 16 ? F >> 2 : F; }
template <class V> __device__ __forceinline__ V piece_load(const float *row, int c) { return reinterpret_cast<const V *>(row)[c]; }
template <class V> __device__ __forceinline__ void piece_store(float *row, int c, V v) { reinterpret_cast<V *>(row)[c] = v; }

__device__ __forceinline__ int64_t shfl64(int64_t v, int src)
{
    return ((int64_t)__shfl((int)(v >> 32), src) << 32) | (uint32_t)__shfl((int)v, src);
}

// ---- the launch shape of `items` row groups over rows of F floats: float4 pieces when F % 4 == 0 and every base is 16-byte aligned ----
struct RowShape {
    bool vec;
    int lanes;
    int64_t blocks;
};
static inline RowShape row_shape(int64_t items, int F, uintptr_t bases)
{
    RowShape s;
    s.vec = (F & 3) == 0 && (bases & 15) == 0;
    s.lanes = pow2_ceil(s.vec ? F >> 2 : F);
    s.lanes = s.lanes > kWave ? kWave : (s.lanes < 1 ? 1 : s.lanes);  // (F == 0: one lane)
    const int per_block = (256 / kWave) * (kWave / s.lanes);
    s.blocks = (items + per_block - 1) / per_block;
    return s;
}

// the float4 or the float instance of a kernel by the shape; SS_ERR_INVALID_ARG for a grid that does not fit
#define SS_ROWS_LAUNCH(shape, vec_kernel, scalar_kernel, ...)                                                                  \
    do {                                                                                                                       \
        if ((shape).blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;                                                   \
        if ((shape).vec)                                                                                                       \
            hipLaunchKernelGGL(vec_kernel, dim3((unsigned)(shape).blocks), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);    \
        else                                                                                                                   \
            hipLaunchKernelGGL(scalar_kernel, dim3((unsigned)(shape).blocks), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        SS_LAUNCH_CHECK();                                                                                                     \
    } while (0)

// ---- which item (a row group of `lanes` lanes) this lane works on.  Kernels that shuffle need every lane: their groups past the end
// shadow the last item (`item`) and do not store; the others leave at item_raw >= items. ------------------------------------------------
struct RowGroup {
    int64_t item_raw, item;
    int cl, base;  // the lane inside its group, the group's first lane in the wavefront
};
__device__ __forceinline__ RowGroup row_group(int lanes, int64_t items)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    RowGroup g;
    g.item_raw = wave * (kWave / lanes) + lane / lanes;
    g.item = g.item_raw < items ? g.item_raw : items - 1;
    g.cl = lane % lanes;
    g.base = lane - g.cl;
    return g;
}

// ---- the gather loop: the terms of the entries at the group positions [a, b) added in entry order into a piece that starts at +0.
// Every lane of the row group calls it with the same (row, a, b).
template <class P>
__device__ __forceinline__ typename P::V gather_sum(const P &pol, int64_t row, int64_t a, int64_t b, int c, int cl, int base, int lanes)
{
    typename P::V p = piece_zero<typename P::V>();
    for (int64_t j0 = a; j0 < b; j0 += lanes) {
        const int64_t j = j0 + cl;  // this lane's entry of the stretch
        const typename P::Entry mine = pol.fetch(row, j < b ? j : a, j < b);
        const int n = (int)(b - j0 < lanes ? b - j0 : lanes);
        for (int k0 = 0; k0 < n; k0 += 4) {  // (uniform per row group)
            typename P::Term t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = pol.request(row, mine, base + (k0 + k < lanes ? k0 + k : 0), k0 + k < n, c);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t[k].use) p = pol.add(p, t[k]);
        }
    }
    return p;
}

// ---- the regular tier: one row group walks the whole row, chunk after chunk, and stores it.  Row groups past the end shadow the last
// row and do not store (the shuffles need every lane); rows of more than hub_entries entries belong to the hub tier and are left
// alone, as is a row whose pointer pair the terms do not follow.
template <class P>
__global__ __launch_bounds__(256) void chunked_rows_kernel(const typename P::Args args, const int64_t *__restrict__ rowptr, int64_t hub_entries,
                                                           int lanes)
{
    using V = typename P::V;
    const P pol{args};
    const RowGroup rg = row_group(lanes, pol.rows);
    const int64_t r = rg.item;
    const int64_t e0 = rowptr[r], e1 = rowptr[r + 1];
    if (!pol.span_ok(e0, e1) || e1 - e0 > hub_entries) return;  // (the whole row group leaves)
    const int64_t row = pol.out_row(r);
    const bool mine = rg.item_raw < pol.rows && (uint64_t)row < (uint64_t)pol.N;
    const int W = piece_width<V>(pol.F);
    for (int cbase = 0; cbase < W; cbase += lanes) {  // (one iteration unless the row has more than 64 pieces)
        const int c = cbase + rg.cl < W ? cbase + rg.cl : W - 1;  // lanes past the last piece read it and do not store, in every iteration
        V s = piece_zero<V>();
        for (int64_t a = e0; a < e1; a += kRowChunk) {
            const int64_t b = e1 - a < kRowChunk ? e1 : a + kRowChunk;
            s = piece_add(s, gather_sum(pol, r, a, b, c, rg.cl, rg.base, lanes));
        }
        s = pol.finish(s, row, c);
        if (mine && cbase + rg.cl < W) piece_store<V>(pol.out + row * pol.F, c, s);
    }
}

// ---- the hub tier, first launch: one row group per (hub row, chunk) writes p_c to row g of the workspace [n_chunks, F].  Chunk g belongs
// to hub chunk_hub[g], whose chunks are hub_chunk[h] .. hub_chunk[h + 1]; hub_rows[h] is the hub's row of rowptr.  A list entry that
// names no row, or no entries of its row, is not followed and writes nothing.
template <class P>
__global__ __launch_bounds__(256) void chunked_hub_partials_kernel(const typename P::Args args, const int64_t *__restrict__ rowptr,
                                                                   const int32_t *__restrict__ hub_rows, const int32_t *__restrict__ hub_chunk,
                                                                   const int32_t *__restrict__ chunk_hub, int64_t n_hubs, int64_t n_chunks,
                                                                   float *__restrict__ ws, int lanes)
{
    using V = typename P::V;
    const P pol{args};
    const RowGroup rg = row_group(lanes, n_chunks);
    const int64_t g = rg.item;
    const int64_t h = chunk_hub[g];
    if ((uint64_t)h >= (uint64_t)n_hubs) return;
    const int64_t r = hub_rows[h];
    if ((uint64_t)r >= (uint64_t)pol.rows) return;
    const int64_t e0 = rowptr[r], e1 = rowptr[r + 1];
    const int64_t a = e0 + (g - hub_chunk[h]) * kRowChunk;
    if (!pol.span_ok(e0, e1) || a < e0 || a >= e1) return;
    const int64_t b = e1 - a < kRowChunk ? e1 : a + kRowChunk;
    const int W = piece_width<V>(pol.F);
    for (int cbase = 0; cbase < W; cbase += lanes) {
        const int c = cbase + rg.cl < W ? cbase + rg.cl : W - 1;
        const V p = gather_sum(pol, r, a, b, c, rg.cl, rg.base, lanes);
        if (rg.item_raw < n_chunks && cbase + rg.cl < W) piece_store<V>(ws + g * pol.F, c, p);
    }
}

// ---- the hub tier, second launch: one lane per piece of a hub row adds the row's partials in chunk order, applies what follows the
// sum in the regular tier and stores the row
template <class P>
__global__ __launch_bounds__(256) void chunked_hub_finish_kernel(const typename P::Args args, const int32_t *__restrict__ hub_rows,
                                                                 const int32_t *__restrict__ hub_chunk, int64_t n_hubs, int64_t n_chunks,
                                                                 const float *__restrict__ ws)
{
    using V = typename P::V;
    const P pol{args};
    const int W = piece_width<V>(pol.F);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t h = t / W;
    const int c = (int)(t - h * W);
    if (h >= n_hubs) return;
    const int64_t r = hub_rows[h];
    if ((uint64_t)r >= (uint64_t)pol.rows) return;
    const int64_t row = pol.out_row(r);
    if ((uint64_t)row >= (uint64_t)pol.N) return;
    int64_t g0 = hub_chunk[h], g1 = hub_chunk[h + 1];
    g0 = g0 < 0 ? 0 : g0;
    g1 = g1 > n_chunks ? n_chunks : g1;
    V s = piece_zero<V>();
    for (int64_t g = g0; g < g1; ++g) s = piece_add(s, piece_load<V>(ws + g * pol.F, c));
    piece_store<V>(pol.out + row * pol.F, c, pol.finish(s, row, c));
}

}  // namespace ss
