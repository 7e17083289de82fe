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
// The tables, the BFS of both tiers, their leaf helpers and the host prelude of the entry points live in ss_exact_bfs.hpp, shared with
// ss_exact_nodes.hip (lists the visited nodes with the same walk) and ss_sampled_nodes.hip; this file keeps its two kernels' loops.
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
    lds_clear(s);
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
            lds_clear(s);
            __syncthreads();
            continue;
        }
        const int cu = s.cnt[0], cv = s.cnt[1];
        for_union(s, cu, cv, [&](int, uint32_t b) { atomicAdd(&s.hist[exact_bucket<H>(b)], 1); });  // (nodes on both sides: once)
        __syncthreads();
        if (t == 0) exact_finish<H>(s.hist, q, flags, o);
        for (int i = t; i < cu + cv; i += kExactThreads) lds_release(s, i < cu ? s.list[0][i] : s.list[1][i - cu]);
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
        large_claim(ws, overflow, total, &next_q);
        if (t == 0) {
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
        for_union(sl, cu, cv, [&](int32_t, uint32_t b) { atomicAdd(&hist[exact_bucket<H>(b)], 1); });
        __syncthreads();
        if (t == 0) exact_finish<H>(hist, q, flags, o);
        for (int64_t i = t; i < cu + cv; i += kExactThreads) slot_clear(sl, i < cu ? sl.list[0][i] : sl.list[1][i - cu]);  // all-zero again
        __syncthreads();
    }
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

extern "C" int ss_exact_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                              int32_t lds_max_nodes, int32_t *I, int32_t *balls, float *feats, int32_t *err_flag, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    using namespace ss;
    Tier t;
    int rc = tier_check(graph, links, B, N, h, workspace, workspace_bytes, feats != nullptr);
    if (rc == SS_OK) rc = tier_lds(lds_max_nodes, workspace, stream, t);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (hipMemsetAsync(t.ws, 0, sizeof(ExactWs), t.stream) != hipSuccess) return SS_ERR_LAUNCH;
    const ExactOut o = {I, balls, feats, err_flag};
    const dim3 grid((unsigned)(B < kExactGrid ? B : kExactGrid)), block(kExactThreads);
    dispatch_h(h, [&](auto H) {
        hipLaunchKernelGGL(exact_lds_kernel<decltype(H)::value>, grid, block, 0, t.stream, *graph, links, B, N, t.limit, flags, o, t.ws,
                           t.overflow);
    });
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_exact_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                              int32_t *I, int32_t *balls, float *feats, void *workspace, size_t workspace_bytes, int32_t slots,
                              void *arena, size_t arena_bytes, void *stream)
{
    using namespace ss;
    Tier t;
    int rc = tier_check(graph, links, B, N, h, workspace, workspace_bytes, feats != nullptr);
    if (rc == SS_OK) rc = tier_large(N, slots, arena, arena_bytes, workspace, stream, t);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    const ExactOut o = {I, balls, feats, nullptr};  // (ss_exact_pairs has zeroed the cursor)
    dispatch_h(h, [&](auto H) {
        hipLaunchKernelGGL(exact_large_kernel<decltype(H)::value>, dim3((unsigned)slots), dim3(kExactThreads), 0, t.stream, *graph, links,
                           N, flags, o, t.ws, t.overflow, static_cast<uint32_t *>(arena));
    });
    SS_LAUNCH_CHECK();
    return SS_OK;
}
