// ss_exact_nodes.hip -- exact subgraph node lists: per link (u, v) every node of B_h(u) | B_h(v), ascending by id, with the pair of
// distances (d_u, d_v) (ElphHashes.exact_subgraph_nodes).  The walk is the two-sided BFS of the exact counts (ss_exact_bfs.hpp, tiers
// as in ss_exact.hip); what differs is the end of a pair: the counts fold the visited nodes into a histogram, this file writes them out.
//
// A root is always in its own ball at distance 0 here (n_self = N is handed to the BFS: a node at or above max(edge_index) + 1 has no
// in-edges, so nothing else changes), which is what a node list wants; the sketch balls of such a node are empty.
//
// Variable-length rows, so two passes over the links with the same tiers:
//   count  the size of each union.  On-chip tier: the number of keys in the LDS table; a pair that passes the node limit goes to the
//          overflow list.  Large tier: |list_u| + the nodes of list_v that u's side did not reach.
//   (host) rows larger than max_nodes become empty, a cumulative sum gives rowptr, ids / dist are allocated.
//   fill   on-chip tier: every link with 0 < row length <= the node limit (the pairs its count pass did not overflow, minus the capped
//          ones).  The table's keys are copied to an LDS array, sorted there (bitonic, padded to a power of two), and written out in
//          order, each with the two distance bytes looked up in the table.  Large tier: the count pass's overflow list again; after
//          the BFS the slot's dense distance bytes are scanned in id order (4096 nodes per step, a workgroup prefix sum places the
//          non-zero ones), which emits ascending ids without a sort and clears the bytes on the way: every distance byte of the arena is zero
//          afterwards (the visit lists behind them are scratch, as in ss_exact.hip: written before they are read).
// Both tiers write row q to [rowptr[q], rowptr[q + 1]) and nothing else; a row is a function of the graph, the link and the flags.
#include "ss_exact_bfs.hpp"

namespace ss {

struct NodesOut {
    int32_t *counts;        // count pass: [B] union sizes
    const int64_t *rowptr;  // fill pass: [B + 1] offsets into ids / dist (null = count pass)
    int64_t *ids;
    uint8_t *dist;          // [.., 2]
    int32_t *err;           // (nullable) set for ids outside [-N, N)
};

// the distance a side's level bits stand for: the lowest one, H + 1 when unreached
template <int H>
__device__ __forceinline__ uint8_t nodes_distance(uint32_t bits) { return (uint8_t)(bits ? __builtin_ctz(bits) : H + 1); }

__device__ __forceinline__ void lds_clear_table(ExactLds &s)
{
    for (int i = threadIdx.x; i < kExactSlots; i += kExactThreads) {
        s.key[i] = kEmpty;
        if (i < kExactSlots / 2) s.val[i] = 0;
    }
}

// ---- on-chip tier ---------------------------------------------------------------------------------------------------------------
template <int H, bool FILL>
__global__ __launch_bounds__(kExactThreads) void nodes_lds_kernel(ss_csr_graph g, const int64_t *__restrict__ links, int64_t B, int64_t N,
                                                                   int limit, uint32_t flags, NodesOut o, ExactWs *__restrict__ ws,
                                                                   int32_t *__restrict__ overflow)
{
    __shared__ ExactLds s;
    __shared__ uint32_t sorted[FILL ? kExactMaxNodes : 1];
    __shared__ int n_sorted;
    const int t = threadIdx.x;
    lds_clear_table(s);
    for (int64_t q = blockIdx.x; q < B; q += gridDim.x) {
        int64_t u, v;
        const bool ok = link_ids(links, q, N, u, v);  // (workgroup-uniform)
        int64_t row = 0, len = 0;
        if (FILL) {
            row = o.rowptr[q];
            len = o.rowptr[q + 1] - row;
            if (!ok || len <= 0 || len > limit) continue;  // capped, or the large tier's (nothing touched: no barrier needed)
        }
        if (t == 0) {
            s.n_nodes = 0;
            s.ovf = limit <= 0;
            s.cnt[0] = s.cnt[1] = 0;
            n_sorted = 0;
        }
        __syncthreads();
        if (!ok) {  // (count pass; the host checks ids before it launches)
            if (t == 0) {
                o.counts[q] = 0;
                if (o.err) *o.err = 1;
            }
            continue;
        }
        const bool ovf = exact_lds_bfs<H>(s, g, u, v, N, flags, limit);
        if (ovf) {  // (fill pass: never -- the row length is the number of keys, and it is within the limit)
            if (!FILL && t == 0) overflow[atomicAdd(&ws->count, 1)] = (int32_t)q;
            __syncthreads();
            lds_clear_table(s);
            __syncthreads();
            continue;
        }
        const int cu = s.cnt[0], cv = s.cnt[1];
        if (!FILL) {
            if (t == 0) o.counts[q] = s.n_nodes;
        } else {
            for (int i = t; i < cu + cv; i += kExactThreads) {  // the union: u's list, then what only v reached
                const int slot = i < cu ? s.list[0][i] : s.list[1][i - cu];
                const uint32_t b = (s.val[slot >> 1] >> (16 * (slot & 1))) & 0xFFFFu;
                if (i < cu || (b & 0xFFu) == 0) sorted[atomicAdd(&n_sorted, 1)] = s.key[slot];
            }
            __syncthreads();
            const int n = n_sorted;  // (<= s.n_nodes <= limit <= kExactMaxNodes)
            int P = 1;
            while (P < n) P <<= 1;
            for (int i = n + t; i < P; i += kExactThreads) sorted[i] = kEmpty;  // (no node id is 2^32 - 1: N < 2^31)
            __syncthreads();
            lds_bitonic_sort(sorted, P);
            const int m = n < len ? n : (int)len;  // (n == len; a store never leaves the row)
            for (int i = t; i < m; i += kExactThreads) {
                const uint32_t x = sorted[i];
                uint32_t at = (x * 2654435761u) >> (32 - kExactSlotsLog);  // (lds_slot's probe; x is in the table)
                while (s.key[at] != x) at = (at + 1) & (kExactSlots - 1);
                const uint32_t b = (s.val[at >> 1] >> (16 * (at & 1))) & 0xFFFFu;
                o.ids[row + i] = (int64_t)x;
                o.dist[2 * (row + i)] = nodes_distance<H>(b & 0xFFu);
                o.dist[2 * (row + i) + 1] = nodes_distance<H>(b >> 8);
            }
            __syncthreads();
        }
        for (int i = t; i < cu + cv; i += kExactThreads) {
            const int slot = i < cu ? s.list[0][i] : s.list[1][i - cu];
            s.key[slot] = kEmpty;
            atomicAnd(&s.val[slot >> 1], ~(0xFFFFu << (16 * (slot & 1))));  // (the other half may be cleared by another lane)
        }
        __syncthreads();
    }
}

// ---- large tier -----------------------------------------------------------------------------------------------------------------
constexpr int kNodesFillGrid = 256 * 3;                    // on-chip fill workgroups (3 per CU: 40.1 KiB of LDS each with the sort array)

template <int H, bool FILL>
__global__ __launch_bounds__(kExactThreads) void nodes_large_kernel(ss_csr_graph g, const int64_t *__restrict__ links, int64_t N,
                                                                     uint32_t flags, NodesOut o, ExactWs *__restrict__ ws,
                                                                     const int32_t *__restrict__ overflow, uint32_t *__restrict__ arena)
{
    __shared__ int cnt[2];
    __shared__ int big[kBigList];
    __shared__ int n_big;
    __shared__ int only_v;
    __shared__ int wave_sum[2][kScanWaves];
    __shared__ int64_t next_q;
    const int t = threadIdx.x;
    const ExactSlot sl = exact_slot(arena, N);
    const int total = ws->count;
    for (;;) {
        if (t == 0) {
            const int i = atomicAdd(&ws->cursor, 1);
            next_q = i < total ? (int64_t)overflow[i] : -1;
            cnt[0] = cnt[1] = 0;
            n_big = 0;
            only_v = 0;
        }
        __syncthreads();
        const int64_t q = next_q;
        if (q < 0) break;
        int64_t u, v;
        int64_t row = 0, len = 0;
        bool skip = !link_ids(links, q, N, u, v);  // (never listed: the on-chip tier has answered such a pair)
        if (FILL && !skip) {
            row = o.rowptr[q];
            len = o.rowptr[q + 1] - row;
            skip = len <= 0;  // capped by max_nodes
        }
        if (skip) {
            __syncthreads();
            continue;
        }
        exact_slot_bfs<H>(sl, g, u, v, N, flags, cnt, big, &n_big);
        const int64_t cu = cnt[0], cv = cnt[1];
        if (!FILL) {
            int mine = 0;
            for (int64_t i = cu + t; i < cu + cv; i += kExactThreads) mine += (slot_byte(sl, sl.list[1][i - cu]) & 0xFFu) == 0;
            if (mine) atomicAdd(&only_v, mine);
            __syncthreads();
            if (t == 0) o.counts[q] = (int32_t)cu + only_v;
            for (int64_t i = t; i < cu + cv; i += kExactThreads) {  // back to all-zero for the next pair
                const int32_t x = i < cu ? sl.list[0][i] : sl.list[1][i - cu];
                atomicAnd(&sl.dist[x >> 2], ~(0xFFu << (8 * (x & 3))));
            }
            __syncthreads();
            continue;
        }
        // the row holds exactly the non-zero bytes (a store never leaves it); the scan leaves them all zero for the next pair
        slot_ordered_scan(sl, N, wave_sum, [&](int64_t at, int64_t x, uint32_t b) {
            if (at < len) {
                o.ids[row + at] = x;
                o.dist[2 * (row + at)] = nodes_distance<H>(b & 0xFu);
                o.dist[2 * (row + at) + 1] = nodes_distance<H>(b >> 4);
            }
        });
        __syncthreads();
    }
}

template <int H>
void launch_nodes_lds(bool fill, const ss_csr_graph &g, const int64_t *links, int64_t B, int64_t N, int limit, uint32_t flags,
                      const NodesOut &o, ExactWs *ws, int32_t *overflow, hipStream_t s)
{
    const int64_t most = fill ? kNodesFillGrid : kExactGrid;
    const dim3 grid((unsigned)(B < most ? B : most)), block(kExactThreads);
    if (fill)
        hipLaunchKernelGGL((nodes_lds_kernel<H, true>), grid, block, 0, s, g, links, B, N, limit, flags, o, ws, overflow);
    else
        hipLaunchKernelGGL((nodes_lds_kernel<H, false>), grid, block, 0, s, g, links, B, N, limit, flags, o, ws, overflow);
}

template <int H>
void launch_nodes_large(bool fill, const ss_csr_graph &g, const int64_t *links, int64_t N, uint32_t flags, const NodesOut &o, ExactWs *ws,
                        const int32_t *overflow, uint32_t *arena, int slots, hipStream_t s)
{
    const dim3 grid((unsigned)slots), block(kExactThreads);
    if (fill)
        hipLaunchKernelGGL((nodes_large_kernel<H, true>), grid, block, 0, s, g, links, N, flags, o, ws, overflow, arena);
    else
        hipLaunchKernelGGL((nodes_large_kernel<H, false>), grid, block, 0, s, g, links, N, flags, o, ws, overflow, arena);
}

}  // namespace ss

// argument checks before any launch (those of ss_exact_pairs / ss_exact_large): 1 = nothing to do
static int nodes_check(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, int32_t *counts,
                       const int64_t *rowptr, int64_t *ids, uint8_t *dist, void *workspace, size_t workspace_bytes)
{
    if (h < 1 || h > SS_MAX_HOPS) return SS_ERR_UNSUPPORTED;
    if (B < 0 || N < 0) return SS_ERR_INVALID_ARG;
    if (B == 0) return 1;
    if (!graph || !links || !workspace || N == 0 || N >= ((int64_t)1 << 31) || graph->num_nodes != N || !graph->rowptr || !graph->col)
        return SS_ERR_INVALID_ARG;
    if (rowptr ? (!ids || !dist) : !counts) return SS_ERR_INVALID_ARG;
    const size_t need = ss_exact_workspace_bytes(B);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    return SS_OK;
}

extern "C" int ss_exact_nodes_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                                    int32_t lds_max_nodes, int32_t *counts, const int64_t *rowptr, int64_t *ids, uint8_t *dist,
                                    int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ss;
    const int rc = nodes_check(graph, links, B, N, h, counts, rowptr, ids, dist, workspace, workspace_bytes);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (lds_max_nodes < 0) return SS_ERR_INVALID_ARG;
    const int limit = lds_max_nodes < kExactMaxNodes ? lds_max_nodes : kExactMaxNodes;
    hipStream_t s = (hipStream_t)stream;
    ExactWs *ws = static_cast<ExactWs *>(workspace);
    int32_t *overflow = reinterpret_cast<int32_t *>(ws + 1);
    const bool fill = rowptr != nullptr;
    if (!fill && hipMemsetAsync(ws, 0, sizeof(ExactWs), s) != hipSuccess) return SS_ERR_LAUNCH;
    const NodesOut o = {counts, rowptr, ids, dist, err_flag};
    switch (h) {
        case 1: launch_nodes_lds<1>(fill, *graph, links, B, N, limit, flags, o, ws, overflow, s); break;
        case 2: launch_nodes_lds<2>(fill, *graph, links, B, N, limit, flags, o, ws, overflow, s); break;
        default: launch_nodes_lds<3>(fill, *graph, links, B, N, limit, flags, o, ws, overflow, s); break;
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_exact_nodes_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                                    int32_t *counts, const int64_t *rowptr, int64_t *ids, uint8_t *dist, void *workspace,
                                    size_t workspace_bytes, int32_t slots, void *arena, size_t arena_bytes, void *stream)
{
    using namespace ss;
    const int rc = nodes_check(graph, links, B, N, h, counts, rowptr, ids, dist, workspace, workspace_bytes);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (slots <= 0 || !arena) return SS_ERR_INVALID_ARG;
    if (arena_bytes / ss_exact_slot_bytes(N) < (size_t)slots) return SS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    ExactWs *ws = static_cast<ExactWs *>(workspace);
    const int32_t *overflow = reinterpret_cast<const int32_t *>(ws + 1);
    const bool fill = rowptr != nullptr;
    if (hipMemsetAsync(&ws->cursor, 0, sizeof(int32_t), s) != hipSuccess) return SS_ERR_LAUNCH;  // (the list is walked once per pass)
    const NodesOut o = {counts, rowptr, ids, dist, nullptr};
    uint32_t *a = static_cast<uint32_t *>(arena);
    switch (h) {
        case 1: launch_nodes_large<1>(fill, *graph, links, N, flags, o, ws, overflow, a, slots, s); break;
        case 2: launch_nodes_large<2>(fill, *graph, links, N, flags, o, ws, overflow, a, slots, s); break;
        default: launch_nodes_large<3>(fill, *graph, links, N, flags, o, ws, overflow, a, slots, s); break;
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}
