// ss_exact.hip -- exact subgraph features: the sizes of the intersections of the k-hop balls of u and v, counted by BFS, and the
// feature algebra of get_subgraph_features applied to them (ElphHashes.exact_subgraph_features).
//
// The sketches of build_hash_tables (reference hashing.py:139-165) summarise, for every node x and hop k, the ball
//   B_0(x) = {x},  B_k(x) = U_{(j -> x) in G'} B_{k-1}(j)
// of G' = edge_index (flow source -> target) + a self loop at every x < max(edge_index) + 1 (add_self_loops without num_nodes,
// hashing.py:148).  Every node that occurs in an edge lies below that bound, so for u below it B_k(u) is the set of nodes within k
// in-edge hops of u (monotone in k), and for u at or above it B_k(u) is empty for k >= 1.  The query's I[k1, k2] = J * U
// (hashing.py:167-189) estimates |B_k1(u) & B_k2(v)|, cards[u][k - 1] estimates |B_k(u)|; here both are counted.
//
// Two tiers, two launches on one stream (the kernel boundary is the only ordering between them; no data passes between workgroups
// inside a launch):
//   exact_lds_kernel   one workgroup per pair at a time (grid-stride).  A level-synchronous BFS from u to depth h over the in-edge
//                      CSR, then one from v, both inserting into ONE open-addressing table in LDS (key = node id, value = one byte
//                      per side, bit d set = reached at level d).  Every insert of a level carries the same bit, so an atomicOr is
//                      idempotent and its old value tells the one lane that reached the node first on that side: that lane appends
//                      the node's slot to the side's visit list, whose level ranges are the frontiers.  A pair whose union of balls
//                      passes the table's node limit is abandoned and its index appended to the overflow list.
//   exact_large_kernel persistent "slots" take the overflow list through an atomic counter.  A slot owns a dense distance byte per
//                      node (same encoding, addressed directly) and a visit list per side; after a pair it clears only the bytes it
//                      visited, so the arena is zeroed once, when it is allocated.  Frontier nodes of high degree are walked by the
//                      whole workgroup instead of one 16-lane group.
// Both tiers then count a (h + 2) x (h + 2) histogram of (d_u, d_v) (h + 1 = not within h) over the visited nodes; I and the two
// ball sizes are its prefix sums.  Integer counts: the result does not depend on the order of anything.
// The tables and the BFS of both tiers live in ss_exact_bfs.hpp (ss_exact_nodes.hip lists the visited nodes with the same walk).
#include "ss_exact_bfs.hpp"
#include "ss_feature_algebra.hpp"

namespace ss {

struct ExactOut {
    int32_t *I;      // [B, H, H]  (nullable)
    int32_t *balls;  // [B, 2, H]  (nullable)
    float *feats;    // [B, H(H+2)]
    int32_t *err;    // (nullable) set for ids outside [-N, N)
};

// (d_u, d_v) bucket of a node from its two side bytes: the lowest level bit, H + 1 when unreached
template <int H>
__device__ __forceinline__ int exact_bucket(uint32_t b)
{
    const uint32_t bu = b & 0xFFu, bv = (b >> 8) & 0xFFu;
    const int du = bu ? __builtin_ctz(bu) : H + 1;
    const int dv = bv ? __builtin_ctz(bv) : H + 1;
    return du * (H + 2) + dv;
}

// the outputs of one pair from its histogram (one thread): prefix sums, then the feature algebra
template <int H>
__device__ void exact_finish(const int *hist, int64_t q, uint32_t flags, const ExactOut &o)
{
    constexpr int W = H + 2;
    int I[H][H], bu[H], bv[H];
#pragma unroll
    for (int k1 = 0; k1 < H; ++k1)
#pragma unroll
        for (int k2 = 0; k2 < H; ++k2) {
            int s = 0;
            for (int a = 0; a <= k1 + 1; ++a)
                for (int b = 0; b <= k2 + 1; ++b) s += hist[a * W + b];
            I[k1][k2] = s;
        }
#pragma unroll
    for (int k = 0; k < H; ++k) {
        int su = 0, sv = 0;
        for (int a = 0; a <= k + 1; ++a)
            for (int b = 0; b < W; ++b) {
                su += hist[a * W + b];
                sv += hist[b * W + a];
            }
        bu[k] = su;
        bv[k] = sv;
    }
    float fI[H][H], c1[H], c2[H], f[H * (H + 2)];
#pragma unroll
    for (int k1 = 0; k1 < H; ++k1) {
        c1[k1] = (float)bu[k1];
        c2[k1] = (float)bv[k1];
#pragma unroll
        for (int k2 = 0; k2 < H; ++k2) fI[k1][k2] = (float)I[k1][k2];
    }
    assemble_features<H>(fI, c1, c2, flags, f);
#pragma unroll
    for (int k = 0; k < H * (H + 2); ++k) o.feats[q * (H * (H + 2)) + k] = f[k];
    if (o.I) {
#pragma unroll
        for (int k1 = 0; k1 < H; ++k1)
#pragma unroll
            for (int k2 = 0; k2 < H; ++k2) o.I[q * (H * H) + k1 * H + k2] = I[k1][k2];
    }
    if (o.balls) {
#pragma unroll
        for (int k = 0; k < H; ++k) {
            o.balls[q * (2 * H) + k] = bu[k];
            o.balls[q * (2 * H) + H + k] = bv[k];
        }
    }
}

// a pair with an id outside [-N, N): NaN features, zero counts (the host checks ids before it launches)
template <int H>
__device__ void exact_bad(int64_t q, const ExactOut &o)
{
    for (int k = 0; k < H * (H + 2); ++k) o.feats[q * (H * (H + 2)) + k] = __uint_as_float(0x7FC00000u);
    if (o.I)
        for (int k = 0; k < H * H; ++k) o.I[q * (H * H) + k] = 0;
    if (o.balls)
        for (int k = 0; k < 2 * H; ++k) o.balls[q * (2 * H) + k] = 0;
    if (o.err) *o.err = 1;
}

// ---- on-chip tier ---------------------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(kExactThreads) void exact_lds_kernel(ss_csr_graph g, const int64_t *__restrict__ links, int64_t B,
                                                                   int64_t N, int limit, uint32_t flags, ExactOut o,
                                                                   ExactWs *__restrict__ ws, int32_t *__restrict__ overflow)
{
    __shared__ ExactLds s;
    const int t = threadIdx.x;
    const int64_t n_self = exact_n_self(g);
    for (int i = t; i < kExactSlots; i += kExactThreads) {
        s.key[i] = kEmpty;
        if (i < kExactSlots / 2) s.val[i] = 0;
    }
    for (int64_t q = blockIdx.x; q < B; q += gridDim.x) {
        int64_t u, v;
        const bool ok = link_ids(links, q, N, u, v);  // (workgroup-uniform)
        if (t < 25) s.hist[t] = 0;
        if (t == 0) {
            s.n_nodes = 0;
            s.ovf = limit <= 0;
            s.cnt[0] = s.cnt[1] = 0;
        }
        __syncthreads();
        if (!ok) {
            if (t == 0) exact_bad<H>(q, o);
            continue;  // (nothing was inserted; the next pair's barrier keeps the counters in step)
        }
        const bool ovf = exact_lds_bfs<H>(s, g, u, v, n_self, flags, limit);
        if (ovf) {
            if (t == 0) overflow[atomicAdd(&ws->count, 1)] = (int32_t)q;
            __syncthreads();
            for (int i = t; i < kExactSlots; i += kExactThreads) {
                s.key[i] = kEmpty;
                if (i < kExactSlots / 2) s.val[i] = 0;
            }
            __syncthreads();
            continue;
        }
        const int cu = s.cnt[0], cv = s.cnt[1];
        for (int i = t; i < cu + cv; i += kExactThreads) {
            const int slot = i < cu ? s.list[0][i] : s.list[1][i - cu];
            const uint32_t b = (s.val[slot >> 1] >> (16 * (slot & 1))) & 0xFFFFu;
            if (i < cu || (b & 0xFFu) == 0) atomicAdd(&s.hist[exact_bucket<H>(b)], 1);  // (nodes on both sides: counted from u's list)
        }
        __syncthreads();
        if (t == 0) exact_finish<H>(s.hist, q, flags, o);
        for (int i = t; i < cu + cv; i += kExactThreads) {
            const int slot = i < cu ? s.list[0][i] : s.list[1][i - cu];
            s.key[slot] = kEmpty;
            atomicAnd(&s.val[slot >> 1], ~(0xFFFFu << (16 * (slot & 1))));  // (the other half may be cleared by another lane)
        }
        __syncthreads();
    }
}

// ---- large tier -----------------------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(kExactThreads) void exact_large_kernel(ss_csr_graph g, const int64_t *__restrict__ links, int64_t N,
                                                                     uint32_t flags, ExactOut o, ExactWs *__restrict__ ws,
                                                                     const int32_t *__restrict__ overflow, uint32_t *__restrict__ arena)
{
    __shared__ int hist[25];
    __shared__ int cnt[2];
    __shared__ int big[kBigList];
    __shared__ int n_big;
    __shared__ int64_t next_q;
    const int t = threadIdx.x;
    const int64_t n_self = exact_n_self(g);
    const ExactSlot sl = exact_slot(arena, N);
    const int total = ws->count;
    for (;;) {
        if (t == 0) {
            const int i = atomicAdd(&ws->cursor, 1);
            next_q = i < total ? (int64_t)overflow[i] : -1;
            cnt[0] = cnt[1] = 0;
            n_big = 0;
        }
        if (t < 25) hist[t] = 0;
        __syncthreads();
        const int64_t q = next_q;
        if (q < 0) break;
        int64_t u, v;
        if (!link_ids(links, q, N, u, v)) {  // (the LDS tier has written this pair already: never listed)
            __syncthreads();
            continue;
        }
        exact_slot_bfs<H>(sl, g, u, v, n_self, flags, cnt, big, &n_big);
        const int64_t cu = cnt[0], cv = cnt[1];
        for (int64_t i = t; i < cu + cv; i += kExactThreads) {
            const int32_t x = i < cu ? sl.list[0][i] : sl.list[1][i - cu];
            const uint32_t b = slot_byte(sl, x);
            if (i < cu || (b & 0xFFu) == 0) atomicAdd(&hist[exact_bucket<H>(b)], 1);
        }
        __syncthreads();
        if (t == 0) exact_finish<H>(hist, q, flags, o);
        for (int64_t i = t; i < cu + cv; i += kExactThreads) {  // back to all-zero for the next pair
            const int32_t x = i < cu ? sl.list[0][i] : sl.list[1][i - cu];
            atomicAnd(&sl.dist[x >> 2], ~(0xFFu << (8 * (x & 3))));
        }
        __syncthreads();
    }
}

template <int H>
void launch_exact_lds(const ss_csr_graph &g, const int64_t *links, int64_t B, int64_t N, int limit, uint32_t flags, const ExactOut &o,
                      ExactWs *ws, int32_t *overflow, hipStream_t s)
{
    const int64_t blocks = B < kExactGrid ? B : kExactGrid;
    hipLaunchKernelGGL(exact_lds_kernel<H>, dim3((unsigned)blocks), dim3(kExactThreads), 0, s, g, links, B, N, limit, flags, o, ws,
                       overflow);
}

template <int H>
void launch_exact_large(const ss_csr_graph &g, const int64_t *links, int64_t N, uint32_t flags, const ExactOut &o, ExactWs *ws,
                        const int32_t *overflow, uint32_t *arena, int slots, hipStream_t s)
{
    hipLaunchKernelGGL(exact_large_kernel<H>, dim3((unsigned)slots), dim3(kExactThreads), 0, s, g, links, N, flags, o, ws, overflow,
                       arena);
}

}  // namespace ss

extern "C" size_t ss_exact_workspace_bytes(int64_t B)
{
    if (B < 0 || B >= ((int64_t)1 << 31)) return 0;
    return sizeof(ss::ExactWs) + 4 * (size_t)(B > 0 ? B : 1);
}

extern "C" size_t ss_exact_slot_bytes(int64_t N)
{
    if (N <= 0 || N >= ((int64_t)1 << 31)) return 0;
    return 4 * (size_t)ss::exact_slot_words(N);
}

// argument checks before any launch: SS_ERR_UNSUPPORTED for h outside [1, 3] (as ss_pair_features), SS_ERR_INVALID_ARG for negative
// sizes or null pointers, 1 (nothing to do) for B == 0
static int exact_check(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, float *feats, void *workspace,
                       size_t workspace_bytes)
{
    if (h < 1 || h > SS_MAX_HOPS) return SS_ERR_UNSUPPORTED;
    if (B < 0 || N < 0) return SS_ERR_INVALID_ARG;
    if (B == 0) return 1;
    if (!graph || !links || !feats || !workspace || N == 0 || N >= ((int64_t)1 << 31) || graph->num_nodes != N || !graph->rowptr ||
        !graph->col)
        return SS_ERR_INVALID_ARG;
    const size_t need = ss_exact_workspace_bytes(B);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    return SS_OK;
}

extern "C" int ss_exact_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                              int32_t lds_max_nodes, int32_t *I, int32_t *balls, float *feats, int32_t *err_flag, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    using namespace ss;
    const int rc = exact_check(graph, links, B, N, h, feats, workspace, workspace_bytes);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (lds_max_nodes < 0) return SS_ERR_INVALID_ARG;
    const int limit = lds_max_nodes < kExactMaxNodes ? lds_max_nodes : kExactMaxNodes;
    hipStream_t s = (hipStream_t)stream;
    ExactWs *ws = static_cast<ExactWs *>(workspace);
    int32_t *overflow = reinterpret_cast<int32_t *>(ws + 1);
    if (hipMemsetAsync(ws, 0, sizeof(ExactWs), s) != hipSuccess) return SS_ERR_LAUNCH;
    const ExactOut o = {I, balls, feats, err_flag};
    switch (h) {
        case 1: launch_exact_lds<1>(*graph, links, B, N, limit, flags, o, ws, overflow, s); break;
        case 2: launch_exact_lds<2>(*graph, links, B, N, limit, flags, o, ws, overflow, s); break;
        default: launch_exact_lds<3>(*graph, links, B, N, limit, flags, o, ws, overflow, s); break;
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_exact_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                              int32_t *I, int32_t *balls, float *feats, void *workspace, size_t workspace_bytes, int32_t slots,
                              void *arena, size_t arena_bytes, void *stream)
{
    using namespace ss;
    const int rc = exact_check(graph, links, B, N, h, feats, workspace, workspace_bytes);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (slots <= 0 || !arena) return SS_ERR_INVALID_ARG;
    if (arena_bytes / ss_exact_slot_bytes(N) < (size_t)slots) return SS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    ExactWs *ws = static_cast<ExactWs *>(workspace);
    const int32_t *overflow = reinterpret_cast<const int32_t *>(ws + 1);
    const ExactOut o = {I, balls, feats, nullptr};
    uint32_t *a = static_cast<uint32_t *>(arena);
    switch (h) {
        case 1: launch_exact_large<1>(*graph, links, N, flags, o, ws, overflow, a, slots, s); break;
        case 2: launch_exact_large<2>(*graph, links, N, flags, o, ws, overflow, a, slots, s); break;
        default: launch_exact_large<3>(*graph, links, N, flags, o, ws, overflow, a, slots, s); break;
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}
