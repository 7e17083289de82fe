// ss_exact_bfs.hpp -- everything the two tiers of the exact family share: the exact counts (ss_exact.hip), the exact node lists
// (ss_exact_nodes.hip) and the sampled node lists (ss_sampled_nodes.hip) keep their own kernels (loop, barriers, what a link's end
// writes) and take the rest from here:
//   on-chip tier  the LDS hash table with its leaf helpers (clear, value, release, find, the union walk), the two-sided BFS into it,
//                 the bitonic sort and the ordered emit of a table's chosen keys
//   large tier    the slot of device memory with its leaf helpers (byte, clear, the union walk), the two-sided BFS into it, the
//                 claim of the next overflow entry and the ordered scan of a slot's bytes
//   both          a fill pass's row fetch
//   host          the argument checks (tier_check), what an entry point hands its launch (Tier, tier_lds, tier_large); dispatch_h: ss_common.hpp
// The sampled walk is its own (one joint walk, its own level byte: ss_sampled_nodes.hip); it uses the tables, the slots and the leaves.
#pragma once
#include "ss_common.hpp"

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

// where the probe for node x starts
__device__ __forceinline__ uint32_t lds_hash(uint32_t x) { return (x * 2654435761u) >> (32 - kExactSlotsLog); }

// an empty table (whole workgroup; no barrier inside)
__device__ __forceinline__ void lds_clear(ExactLds &s)
{
    for (int i = threadIdx.x; i < kExactSlots; i += kExactThreads) {
        s.key[i] = kEmpty;
        if (i < kExactSlots / 2) s.val[i] = 0;
    }
}

__device__ __forceinline__ uint32_t lds_value(const ExactLds &s, int slot) { return (s.val[slot >> 1] >> (16 * (slot & 1))) & 0xFFFFu; }

// one slot back to empty: the key and its half of the value word (the other half may be cleared by another lane)
__device__ __forceinline__ void lds_release(ExactLds &s, int slot)
{
    s.key[slot] = kEmpty;
    atomicAnd(&s.val[slot >> 1], ~(0xFFFFu << (16 * (slot & 1))));
}

// slot of a node x that is in the table (lds_slot's probe without the insert)
__device__ __forceinline__ int lds_find(const ExactLds &s, uint32_t x)
{
    uint32_t i = lds_hash(x);
    while (s.key[i] != x) i = (i + 1) & (kExactSlots - 1);
    return (int)i;
}

// slot of node x (inserted if new; -1: the pair has passed its node limit)
__device__ __forceinline__ int lds_slot(ExactLds &s, uint32_t x, int limit)
{
    uint32_t i = lds_hash(x);
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

// both BFSs of the pair (u, v) into the workgroup's table (whole workgroup; a root at or above n_self is not visited).  The caller
// has emptied the table, zeroed s.n_nodes and s.cnt, set s.ovf = (limit <= 0) and passed a barrier since.  -> the pair passed the
// node limit (workgroup-uniform); every thread has passed a barrier after the last write when this returns
template <int H>
__device__ __forceinline__ bool exact_lds_bfs(ExactLds &s, const ss_csr_graph &g, int64_t u, int64_t v, int64_t n_self, uint32_t flags,
                                              int limit)
{
    const int t = threadIdx.x;
    const int grp = t / kRow, lane = t & (kRow - 1);
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
    return ovf;
}

// ascending bitonic sort of sorted[0 .. P) in LDS, P a power of two (whole workgroup; the caller has passed a barrier since the array
// was written, and every thread has passed one after the last exchange when this returns)
__device__ __forceinline__ void lds_bitonic_sort(uint32_t *sorted, int P)
{
    const int t = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += kExactThreads) {
                const int p = i ^ j;
                if (p > i) {
                    const uint32_t a = sorted[i], b = sorted[p];
                    if ((a > b) == ((i & k) == 0)) {
                        sorted[i] = b;
                        sorted[p] = a;
                    }
                }
            }
            __syncthreads();
        }
}

// the union of the two balls (whole workgroup): f(slot, value) for u's list, then for the nodes only v reached
template <class F>
__device__ __forceinline__ void for_union(const ExactLds &s, int cu, int cv, F f)
{
    for (int i = threadIdx.x; i < cu + cv; i += kExactThreads) {
        const int slot = i < cu ? s.list[0][i] : s.list[1][i - cu];
        const uint32_t b = lds_value(s, slot);
        if (i < cu || (b & 0xFFu) == 0) f(slot, b);
    }
}

// chosen keys of the table in ascending order (whole workgroup): sorted[0 .. n) holds them (n workgroup-uniform, written since the
// last barrier at the earliest); they are padded to a power of two (no node id is 2^32 - 1: N < 2^31), sorted, and emit(i, x, slot)
// is called for place i < min(n, len) with its key and the key's slot (n == len: a store never leaves the row)
template <class Emit>
__device__ __forceinline__ void lds_ordered_emit(const ExactLds &s, uint32_t *sorted, int n, int64_t len, Emit emit)
{
    const int t = threadIdx.x;
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = n + t; i < P; i += kExactThreads) sorted[i] = kEmpty;
    __syncthreads();
    lds_bitonic_sort(sorted, P);
    const int m = n < len ? n : (int)len;
    for (int i = t; i < m; i += kExactThreads) {
        const uint32_t x = sorted[i];
        emit(i, x, lds_find(s, x));
    }
}

// a fill pass's row of link q
__device__ __forceinline__ void fill_row(const int64_t *rowptr, int64_t q, int64_t &row, int64_t &len)
{
    row = rowptr[q];
    len = rowptr[q + 1] - row;
}

// ---- large tier -----------------------------------------------------------------------------------------------------------------
// slot arena: uint32 dist[ceil(N / 4)] (one byte per node: bits 0-3 side u, 4-7 side v), int32 list_u[N], int32 list_v[N]
__host__ __device__ __forceinline__ int64_t exact_dist_words(int64_t N) { return (N + 3) / 4; }
__host__ __device__ __forceinline__ int64_t exact_slot_words(int64_t N) { return (exact_dist_words(N) + 2 * N + 3) & ~(int64_t)3; }

struct ExactSlot {
    uint32_t *dist;
    int32_t *list[2];
};

__device__ __forceinline__ ExactSlot exact_slot(uint32_t *arena, int64_t N)
{
    uint32_t *base = arena + (int64_t)blockIdx.x * exact_slot_words(N);
    return {base, {reinterpret_cast<int32_t *>(base + exact_dist_words(N)), reinterpret_cast<int32_t *>(base + exact_dist_words(N)) + N}};
}

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

// the byte of node x back to zero
__device__ __forceinline__ void slot_clear(const ExactSlot &sl, int32_t x) { atomicAnd(&sl.dist[x >> 2], ~(0xFFu << (8 * (x & 3)))); }

// the union of the two balls (whole workgroup): f(node, slot_byte) for u's list, then for the nodes only v reached
template <class F>
__device__ __forceinline__ void for_union(const ExactSlot &sl, int64_t cu, int64_t cv, F f)
{
    for (int64_t i = threadIdx.x; i < cu + cv; i += kExactThreads) {
        const int32_t x = i < cu ? sl.list[0][i] : sl.list[1][i - cu];
        const uint32_t b = slot_byte(sl, x);
        if (i < cu || (b & 0xFFu) == 0) f(x, b);
    }
}

// thread 0 takes the next entry of the overflow list into the workgroup's *next_q (-1: none left; `total` = ws->count); the caller's
// barrier hands it to the other threads
__device__ __forceinline__ void large_claim(ExactWs *ws, const int32_t *overflow, int total, int64_t *next_q)
{
    if (threadIdx.x == 0) {
        const int i = atomicAdd(&ws->cursor, 1);
        *next_q = i < total ? (int64_t)overflow[i] : -1;
    }
}

// both BFSs of the pair (u, v) into the slot (whole workgroup).  cnt[2], big[kBigList] and *n_big are the workgroup's LDS; the caller
// has zeroed cnt and *n_big and passed a barrier since.  Afterwards sl.list[side][0 .. cnt[side]) are the nodes of side's ball; every
// thread has passed a barrier after the last write when this returns
template <int H>
__device__ __forceinline__ void exact_slot_bfs(const ExactSlot &sl, const ss_csr_graph &g, int64_t u, int64_t v, int64_t n_self,
                                               uint32_t flags, int *cnt, int *big, int *n_big)
{
    const int t = threadIdx.x;
    const int grp = t / kRow, lane = t & (kRow - 1);
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
                    if (lane == 0) at = atomicAdd(n_big, 1);
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
            const int nb = *n_big < kBigList ? *n_big : kBigList;
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
            if (t == 0) *n_big = 0;
            lo = hi;
            hi = cnt[side];
        }
        __syncthreads();
    }
}

constexpr int kScanWords = 4;                        // slot bytes as words (16 nodes) per thread and step of the ordered scan
constexpr int kScanWaves = kExactThreads / kWave;

// the ordered scan of a slot's bytes (whole workgroup): emit(place, id, byte) for every node with a non-zero byte, in id order -- place
// counts them from 0 -- and every word is zero afterwards.  Thread t owns words [w0 + kScanWords * t, + kScanWords) of each step, so
// ids ascend with (step, t, word, byte); a workgroup prefix sum over the non-zero counts gives the places.  wave_sum: the workgroup's
// LDS; the caller has passed a barrier since its last use and since the last write of a byte
template <class Emit>
__device__ __forceinline__ void slot_ordered_scan(const ExactSlot &sl, int64_t N, int (*wave_sum)[kScanWaves], Emit emit)
{
    const int t = threadIdx.x;
    const int64_t W = exact_dist_words(N);
    const int wave = t / kWave, wl = t & (kWave - 1);
    int64_t done = 0;
    int buf = 0;
    for (int64_t w0 = 0; w0 < W; w0 += kScanWords * kExactThreads, buf ^= 1) {
        const int64_t w = w0 + kScanWords * t;
        uint32_t word[kScanWords];
        int c = 0;
#pragma unroll
        for (int k = 0; k < kScanWords; ++k) {
            word[k] = w + k < W ? __hip_atomic_load(&sl.dist[w + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) c += ((word[k] >> (8 * j)) & 0xFFu) != 0;
        }
        int inc = c;  // inclusive prefix sum within the wave
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int y = __shfl_up(inc, d);
            if (wl >= d) inc += y;
        }
        if (wl == kWave - 1) wave_sum[buf][wave] = inc;
        __syncthreads();  // (one barrier per step: the next step writes the other buffer)
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kScanWaves; ++k) {
            const int sum = wave_sum[buf][k];
            before += k < wave ? sum : 0;
            all += sum;
        }
        if (c) {
            int64_t at = done + before + inc - c;
#pragma unroll
            for (int k = 0; k < kScanWords; ++k) {
                if (word[k] == 0) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t b = (word[k] >> (8 * j)) & 0xFFu;
                    if (b) emit(at, 4 * (w + k) + j, b);
                    at += b != 0;
                }
                __hip_atomic_store(&sl.dist[w + k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // all zero for the next pair
            }
        }
        done += all;
    }
}

// ---- host side of an entry point ------------------------------------------------------------------------------------------------
// argument checks before any launch: SS_ERR_UNSUPPORTED for h outside [1, 3] (as ss_pair_features), SS_ERR_INVALID_ARG for negative
// sizes, null pointers or missing outputs, SS_ERR_WORKSPACE for a workspace below ss_exact_workspace_bytes(B), 1 (nothing to do) for B == 0
inline int tier_check(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, const void *workspace,
                      size_t workspace_bytes, bool outputs)
{
    if (h < 1 || h > SS_MAX_HOPS) return SS_ERR_UNSUPPORTED;
    if (B < 0 || N < 0) return SS_ERR_INVALID_ARG;
    if (B == 0) return 1;
    if (!graph || !links || !outputs || !workspace || N == 0 || N >= ((int64_t)1 << 31) || graph->num_nodes != N || !graph->rowptr ||
        !graph->col)
        return SS_ERR_INVALID_ARG;
    const size_t need = ss_exact_workspace_bytes(B);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    return SS_OK;
}

struct Tier {
    int limit;          // on-chip node limit (on-chip entry points)
    ExactWs *ws;
    int32_t *overflow;  // [B] behind ws
    hipStream_t stream;
};

// what an on-chip entry point launches with, after a tier_check that returned SS_OK
inline int tier_lds(int32_t lds_max_nodes, void *workspace, void *stream, Tier &t)
{
    if (lds_max_nodes < 0) return SS_ERR_INVALID_ARG;
    ExactWs *ws = static_cast<ExactWs *>(workspace);
    t = {lds_max_nodes < kExactMaxNodes ? lds_max_nodes : kExactMaxNodes, ws, reinterpret_cast<int32_t *>(ws + 1), (hipStream_t)stream};
    return SS_OK;
}

// the same for a large-tier entry point, with the checks of its slots and arena
inline int tier_large(int64_t N, int32_t slots, const void *arena, size_t arena_bytes, void *workspace, void *stream, Tier &t)
{
    if (slots <= 0 || !arena) return SS_ERR_INVALID_ARG;
    if (arena_bytes / ss_exact_slot_bytes(N) < (size_t)slots) return SS_ERR_WORKSPACE;
    return tier_lds(0, workspace, stream, t);
}

}  // namespace ss
