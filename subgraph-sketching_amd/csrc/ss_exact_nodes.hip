// ss_exact_nodes.hip -- exact subgraph node lists: per link (u, v) every node of B_h(u) | B_h(v), ascending by id, with the pair of
// distances (d_u, d_v) (ElphHashes.exact_subgraph_nodes).  The walk is the two-sided BFS of the exact counts (ss_exact_bfs.hpp, which
// also holds the tiers' leaf helpers and the entry points' host prelude; tiers as in ss_exact.hip); what differs is the end of a pair:
// the counts fold the visited nodes into a histogram, this file writes them out.
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
    lds_clear(s);
    for (int64_t q = blockIdx.x; q < B; q += gridDim.x) {
        int64_t u, v;
        const bool ok = link_ids(links, q, N, u, v);  // (workgroup-uniform)
        int64_t row = 0, len = 0;
        if (FILL) {
            fill_row(o.rowptr, q, row, len);
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
            lds_clear(s);
            __syncthreads();
            continue;
        }
        const int cu = s.cnt[0], cv = s.cnt[1];
        if (!FILL) {
            if (t == 0) o.counts[q] = s.n_nodes;
        } else {
            for_union(s, cu, cv, [&](int slot, uint32_t) { sorted[atomicAdd(&n_sorted, 1)] = s.key[slot]; });
            __syncthreads();
            // (n_sorted <= s.n_nodes <= limit <= kExactMaxNodes)
            lds_ordered_emit(s, sorted, n_sorted, len, [&](int i, uint32_t x, int slot) {
                const uint32_t b = lds_value(s, slot);
                o.ids[row + i] = (int64_t)x;
                o.dist[2 * (row + i)] = nodes_distance<H>(b & 0xFFu);
                o.dist[2 * (row + i) + 1] = nodes_distance<H>(b >> 8);
            });
            __syncthreads();
        }
        for (int i = t; i < cu + cv; i += kExactThreads) lds_release(s, i < cu ? s.list[0][i] : s.list[1][i - cu]);
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
        large_claim(ws, overflow, total, &next_q);
        if (t == 0) {
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
            fill_row(o.rowptr, q, row, len);
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
            for (int64_t i = t; i < cu + cv; i += kExactThreads) slot_clear(sl, i < cu ? sl.list[0][i] : sl.list[1][i - cu]);  // all-zero again
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

}  // namespace ss

extern "C" int ss_exact_nodes_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                                    int32_t lds_max_nodes, int32_t *counts, const int64_t *rowptr, int64_t *ids, uint8_t *dist,
                                    int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ss;
    const bool fill = rowptr != nullptr;
    Tier t;
    int rc = tier_check(graph, links, B, N, h, workspace, workspace_bytes, fill ? ids && dist : counts != nullptr);
    if (rc == SS_OK) rc = tier_lds(lds_max_nodes, workspace, stream, t);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (!fill && hipMemsetAsync(t.ws, 0, sizeof(ExactWs), t.stream) != hipSuccess) return SS_ERR_LAUNCH;
    const NodesOut o = {counts, rowptr, ids, dist, err_flag};
    const int64_t most = fill ? kNodesFillGrid : kExactGrid;
    const dim3 grid((unsigned)(B < most ? B : most)), block(kExactThreads);
    dispatch_h(h, [&](auto H) {
        constexpr int kH = decltype(H)::value;
        const auto kernel = fill ? nodes_lds_kernel<kH, true> : nodes_lds_kernel<kH, false>;
        hipLaunchKernelGGL(kernel, grid, block, 0, t.stream, *graph, links, B, N, t.limit, flags, o, t.ws, t.overflow);
    });
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_exact_nodes_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, uint32_t flags,
                                    int32_t *counts, const int64_t *rowptr, int64_t *ids, uint8_t *dist, void *workspace,
                                    size_t workspace_bytes, int32_t slots, void *arena, size_t arena_bytes, void *stream)
{
    using namespace ss;
    const bool fill = rowptr != nullptr;
    Tier t;
    int rc = tier_check(graph, links, B, N, h, workspace, workspace_bytes, fill ? ids && dist : counts != nullptr);
    if (rc == SS_OK) rc = tier_large(N, slots, arena, arena_bytes, workspace, stream, t);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (hipMemsetAsync(&t.ws->cursor, 0, sizeof(int32_t), t.stream) != hipSuccess) return SS_ERR_LAUNCH;  // (the list is walked once per pass)
    const NodesOut o = {counts, rowptr, ids, dist, nullptr};
    dispatch_h(h, [&](auto H) {
        constexpr int kH = decltype(H)::value;
        const auto kernel = fill ? nodes_large_kernel<kH, true> : nodes_large_kernel<kH, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)slots), dim3(kExactThreads), 0, t.stream, *graph, links, N, flags, o, t.ws, t.overflow,
                           static_cast<uint32_t *>(arena));
    });
    SS_LAUNCH_CHECK();
    return SS_OK;
}
