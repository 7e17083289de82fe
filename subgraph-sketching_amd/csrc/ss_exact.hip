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
#include "ss_feature_algebra.hpp"

namespace ss {

constexpr int kExactThreads = 256;
constexpr int kExactGroups = kExactThreads / kRow;   // 16-lane groups per workgroup (one frontier node each)
constexpr int kExactSlotsLog = 12;
constexpr int kExactSlots = 1 << kExactSlotsLog;      // LDS table entries
constexpr int kExactMaxNodes = kExactSlots / 2;       // node limit of the LDS tier (load factor <= 1/2 + one insert per lane)
constexpr int kExactGrid = 256 * 4;                   // LDS-tier workgroups (4 per CU: 32.1 KiB of LDS each, ExactLds)
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr int kBigDegree = 512;                       // large tier: frontier nodes with more in-edges are walked by the whole workgroup
constexpr int kBigList = 64;

struct ExactOut {
    int32_t *I;      // [B, H, H]  (nullable)
    int32_t *balls;  // [B, 2, H]  (nullable)
    float *feats;    // [B, H(H+2)]
    int32_t *err;    // (nullable) set for ids outside [-N, N)
};

// workspace of one call: int32 {overflow count, large-tier cursor, pad, pad}, then int32 overflow list [B]
struct ExactWs {
    int32_t count, cursor, pad0, pad1;
};

__device__ __forceinline__ int64_t exact_n_self(const ss_csr_graph &g)
{
    return g.n_self_loops_dev ? *g.n_self_loops_dev : g.n_self_loops;
}

// SS_FLAG_MASK_TARGET: the balls are those of the graph without the edges u -> v and v -> u.  Level 1 expands the root alone, so the
// root's expansion leaves the partner out (-1: nothing is left out -- no node id is negative); when the partner is reached another
// way and expanded, it finds the root visited already, so its own removed in-edge needs nothing.
__device__ __forceinline__ int32_t exact_skip(uint32_t flags, int64_t partner) { return (flags & SS_FLAG_MASK_TARGET) ? (int32_t)partner : -1; }

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
// the value of slot i is the 16-bit half (i & 1) of val[i >> 1] (two side bytes; only ds_or_b32 exists, so halves share a word)
struct ExactLds {
    uint32_t key[kExactSlots];
    uint32_t val[kExactSlots / 2];
    uint16_t list[2][kExactMaxNodes];  // slots in the order each side first reached them (level ranges = frontiers)
    int hist[25];
    int n_nodes, ovf;
    int cnt[2];
};

// slot of node x (inserted if new; -1: the pair has passed its node limit)
__device__ __forceinline__ int lds_slot(ExactLds &s, uint32_t x, int limit)
{
    uint32_t i = (x * 2654435761u) >> (32 - kExactSlotsLog);
    for (int probe = 0; probe < kExactSlots; ++probe) {
        const uint32_t k = s.key[i];
        if (k == x) return (int)i;
        if (k == kEmpty) {
            const uint32_t old = atomicCAS(&s.key[i], kEmpty, x);
            if (old == kEmpty) {
                if (atomicAdd(&s.n_nodes, 1) >= limit) {
                    s.ovf = 1;
                    return -1;
                }
                return (int)i;
            }
            if (old == x) return (int)i;
        }
        i = (i + 1) & (kExactSlots - 1);
    }
    s.ovf = 1;  // (unreachable: at most limit + one key per lane are ever inserted)
    return -1;
}

__device__ __forceinline__ void lds_visit(ExactLds &s, uint32_t x, int side, int level, int limit)
{
    const int i = lds_slot(s, x, limit);
    if (i < 0) return;
    const int sh = 16 * (i & 1) + 8 * side;
    const uint32_t old = atomicOr(&s.val[i >> 1], (1u << level) << sh);
    if (((old >> sh) & 0xFFu) == 0) {
        const int at = atomicAdd(&s.cnt[side], 1);
        if (at < kExactMaxNodes) s.list[side][at] = (uint16_t)i;
    }
}

template <int H>
__global__ __launch_bounds__(kExactThreads) void exact_lds_kernel(ss_csr_graph g, const int64_t *__restrict__ links, int64_t B,
                                                                   int64_t N, int limit, uint32_t flags, ExactOut o,
                                                                   ExactWs *__restrict__ ws, int32_t *__restrict__ overflow)
{
    __shared__ ExactLds s;
    const int t = threadIdx.x;
    const int grp = t / kRow, lane = t & (kRow - 1);
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
        // `ovf` is the workgroup's copy of s.ovf, read only between a barrier that follows every write of a phase and the barrier
        // before the next phase's writes (the next root insert, the next level's appends): every wave takes the same branches
        bool ovf = limit <= 0;
        for (int side = 0; side < 2 && !ovf; ++side) {
            const int64_t root = side ? v : u;
            const int32_t skip = exact_skip(flags, side ? u : v);
            if (root < n_self && t == 0) lds_visit(s, (uint32_t)root, side, 0, limit);
            __syncthreads();
            int lo = 0, hi = s.cnt[side];
            ovf = s.ovf;
            for (int d = 1; d <= H && lo < hi && !ovf; ++d) {
                __syncthreads();  // every thread has read hi before the level appends
                for (int f = lo + grp; f < hi; f += kExactGroups) {
                    const int64_t y = s.key[s.list[side][f]];
                    const int64_t e1 = g.rowptr[y + 1];
                    for (int64_t e = g.rowptr[y] + lane; e < e1; e += kRow) {
                        if (s.ovf) break;
                        const int32_t x = g.col[e];
                        if (d == 1 && x == skip) continue;  // SS_FLAG_MASK_TARGET: the root's expansion leaves the partner out
                        lds_visit(s, (uint32_t)x, side, d, limit);  // (the self loop of y: y is in the list already)
                    }
                }
                __syncthreads();
                lo = hi;
                hi = s.cnt[side] < kExactMaxNodes ? s.cnt[side] : kExactMaxNodes;
                ovf = s.ovf;
            }
            __syncthreads();  // every thread has read s.ovf / s.cnt before the next side's root insert
        }
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
// slot arena: uint32 dist[ceil(N / 4)] (one byte per node: bits 0-3 side u, 4-7 side v), int32 list_u[N], int32 list_v[N]
__host__ __device__ __forceinline__ int64_t exact_dist_words(int64_t N) { return (N + 3) / 4; }
__host__ __device__ __forceinline__ int64_t exact_slot_words(int64_t N) { return (exact_dist_words(N) + 2 * N + 3) & ~(int64_t)3; }

struct ExactSlot {
    uint32_t *dist;
    int32_t *list[2];
};

// first reach of x on `side` at `level`?  (the byte's bits are all the information: every access is an agent-scope atomic)
__device__ __forceinline__ bool slot_reach(const ExactSlot &sl, int32_t x, int side, int level)
{
    const int sh = 8 * (x & 3);
    const uint32_t bit = ((1u << level) << (4 * side)) << sh;
    const uint32_t old = atomicOr(&sl.dist[x >> 2], bit);
    return ((old >> sh) & (0xFu << (4 * side))) == 0;
}

__device__ __forceinline__ uint32_t slot_byte(const ExactSlot &sl, int32_t x)
{
    const uint32_t w = __hip_atomic_load(&sl.dist[x >> 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t b = (w >> (8 * (x & 3))) & 0xFFu;
    return (b & 0xFu) | ((b >> 4) << 8);  // -> the LDS tier's layout for exact_bucket
}

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
    const int grp = t / kRow, lane = t & (kRow - 1);
    const int64_t n_self = exact_n_self(g);
    uint32_t *base = arena + (int64_t)blockIdx.x * exact_slot_words(N);
    const ExactSlot sl = {base, {reinterpret_cast<int32_t *>(base + exact_dist_words(N)),
                                 reinterpret_cast<int32_t *>(base + exact_dist_words(N)) + N}};
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
        for (int side = 0; side < 2; ++side) {
            const int64_t root = side ? v : u;
            const int32_t skip = exact_skip(flags, side ? u : v);
            if (root < n_self && t == 0 && slot_reach(sl, (int32_t)root, side, 0)) sl.list[side][cnt[side]++] = (int32_t)root;
            __syncthreads();
            int64_t lo = 0, hi = cnt[side];
            for (int d = 1; d <= H && lo < hi; ++d) {
                __syncthreads();
                for (int64_t f = lo + grp; f < hi; f += kExactGroups) {
                    const int32_t y = sl.list[side][f];
                    const int64_t e0 = g.rowptr[y], e1 = g.rowptr[y + 1];
                    if (e1 - e0 > kBigDegree) {  // walked by the whole workgroup below (or here, if the big list is full)
                        int at = kBigList;
                        if (lane == 0) at = atomicAdd(&n_big, 1);
                        at = __shfl(at, (t & (kWave - 1)) & ~(kRow - 1));
                        if (at < kBigList) {
                            if (lane == 0) big[at] = y;
                            continue;
                        }
                    }
                    for (int64_t e = e0 + lane; e < e1; e += kRow) {
                        const int32_t x = g.col[e];
                        if (d == 1 && x == skip) continue;
                        if (slot_reach(sl, x, side, d)) sl.list[side][atomicAdd(&cnt[side], 1)] = x;
                    }
                }
                __syncthreads();
                const int nb = n_big < kBigList ? n_big : kBigList;
                for (int b = 0; b < nb; ++b) {
                    const int32_t y = big[b];
                    const int64_t e1 = g.rowptr[y + 1];
                    for (int64_t e = g.rowptr[y] + t; e < e1; e += kExactThreads) {
                        const int32_t x = g.col[e];
                        if (d == 1 && x == skip) continue;
                        if (slot_reach(sl, x, side, d)) sl.list[side][atomicAdd(&cnt[side], 1)] = x;
                    }
                }
                __syncthreads();
                if (t == 0) n_big = 0;
                lo = hi;
                hi = cnt[side];
            }
            __syncthreads();
        }
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
