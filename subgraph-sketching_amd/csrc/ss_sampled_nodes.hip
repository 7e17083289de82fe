// ss_sampled_nodes.hip -- per-hop sampled enclosing subgraphs: per link (u, v) the node row of the reference's k_hop_subgraph with its
// sample_ratio / max_nodes_per_hop (src/datasets/seal.py:291-348), made deterministic (ElphHashes.sampled_subgraph_nodes).
//
// One JOINT walk from {u, v} over in-arcs (not the two-sided BFS of ss_exact_nodes.hip):
//   visited = kept_0 = {u, v};  for hop = 1 .. h:  fringe = in-neighbours(kept_{hop-1}) - visited;  visited |= fringe (ALL of it: a node
//   that is rejected never comes back);  m = sampled_take(|fringe|);  kept_hop = the m fringe nodes with the smallest (key, id)
//   (ss_sampled.hpp);  stop when m == 0.  The row is the union of the kept, ascending by id, each with the hop it joined at.
// The target link is NOT removed from the walk (the reference walks A with it; the roots are visited from the start anyway).
//
// A node's level byte: 0 = not visited, 0x80 = visited (in a fringe; rejected unless more is set), 0x80 | (hop + 1) = kept at `hop`.
// Two lists per link: list 0 the visited nodes in the order they were reached (a hop's fringe is a range of it), list 1 the kept ones
// (a hop's frontier is a range of it).
//
// Tiers as in ss_exact_nodes.hip (tables, slots, their leaf helpers and the entry points' host prelude: ss_exact_bfs.hpp; the helpers
// that know this walk's level byte are here), and two passes over the links (count, one host read for the allocation, fill):
//   on-chip   visited stays within the LDS table of ss_exact_bfs.hpp (key / val / the two slot lists; the value half holds the level
//             byte).  A link whose visited set passes the node limit goes to the batch's overflow list and gets state bit 1, which
//             is how the fill pass knows the tier (a row's length says nothing about the size of what was visited).  Fill: the kept
//             keys are sorted in LDS (bitonic) and written with the hop looked up in the table.
//   slot      exact._arena's slot: dense level bytes and the two int32 lists.  Frontier nodes above kBigDegree are walked by the whole
//             workgroup.  Rejected nodes are cleared through list 0; fill scans the level bytes in id order (ascending without a
//             sort) and clears them on the way, count clears through list 0: every level byte of the arena is zero afterwards.
// Selection in either tier: sampled_select over the fringe range of list 0, keys recomputed from the ids.
// Both tiers write row q to [rowptr[q], rowptr[q + 1]) and nothing else; a row is a function of (graph, u, v, h, cap, ratio, seed).
#include "ss_exact_bfs.hpp"
#include "ss_sampled.hpp"

namespace ss {

static_assert(kExactThreads == kSelThreads, "sampled_select is written for the exact tiers' workgroup");

constexpr int kStateSampled = 1;  // state[q] bit 0: some hop dropped a node
constexpr int kStateSlot = 2;     // state[q] bit 1: the slot tier's link

struct SampledArgs {
    int h, cap;     // cap: INT32_MAX when there is none
    double ratio;
    uint64_t seed;
};

struct SampledOut {
    int32_t *counts;        // count pass: [B] kept nodes
    int32_t *state;         // [B] kState*: written by the count pass, read by the fill pass
    const int64_t *rowptr;  // fill pass: [B + 1] offsets into ids / hop (null = count pass)
    int64_t *ids;
    uint8_t *hop;
    int32_t *err;           // (nullable) set for ids outside [-N, N)
};

// ---- on-chip tier ---------------------------------------------------------------------------------------------------------------
// first visit of x: into the table and onto list 0 (nothing when the link has passed its node limit: s.ovf is set)
__device__ __forceinline__ void sampled_lds_visit(ExactLds &s, uint32_t x, int limit)
{
    const int i = lds_slot(s, x, limit);
    if (i < 0) return;
    const int sh = 16 * (i & 1);
    const uint32_t old = atomicOr(&s.val[i >> 1], 0x80u << sh);
    if (((old >> sh) & 0xFFu) == 0) {
        const int at = atomicAdd(&s.cnt[0], 1);
        if (at < kExactMaxNodes) s.list[0][at] = (uint16_t)i;
    }
}

// slot (visited already) is kept at `hop`: at place `at` of list 1
__device__ __forceinline__ void sampled_lds_keep(ExactLds &s, int slot, int hop, int at)
{
    atomicOr(&s.val[slot >> 1], (uint32_t)(hop + 1) << (16 * (slot & 1)));
    if (at < kExactMaxNodes) s.list[1][at] = (uint16_t)slot;
}

template <bool FILL>
__global__ __launch_bounds__(kExactThreads) void sampled_lds_kernel(ss_csr_graph g, const int64_t *__restrict__ links, int64_t B, int64_t N,
                                                                     int limit, SampledArgs a, SampledOut o, ExactWs *__restrict__ ws,
                                                                     int32_t *__restrict__ overflow)
{
    __shared__ ExactLds s;
    __shared__ SampledSelect sel;
    __shared__ uint32_t sorted[FILL ? kExactMaxNodes : 1];
    const int t = threadIdx.x;
    const int grp = t / kRow, lane = t & (kRow - 1);
    lds_clear(s);
    for (int64_t q = blockIdx.x; q < B; q += gridDim.x) {
        int64_t u, v;
        const bool ok = link_ids(links, q, N, u, v);  // (workgroup-uniform)
        int64_t row = 0, len = 0;
        if (FILL) {
            fill_row(o.rowptr, q, row, len);
            if (!ok || len <= 0 || (o.state[q] & kStateSlot)) continue;  // emptied, or the slot tier's (nothing touched: no barrier needed)
        }
        __syncthreads();  // the table is empty and the last link's reads of s are over
        if (t == 0) {
            s.n_nodes = 0;
            s.ovf = limit <= 0;
            s.cnt[0] = s.cnt[1] = 0;
        }
        __syncthreads();
        if (!ok) {  // (count pass; the host checks ids before it launches)
            if (t == 0) {
                o.counts[q] = 0;
                o.state[q] = 0;
                if (o.err) *o.err = 1;
            }
            continue;
        }
        if (t == 0) {
            sampled_lds_visit(s, (uint32_t)u, limit);
            if (v != u) sampled_lds_visit(s, (uint32_t)v, limit);
            const int roots = s.cnt[0];  // (0 when the limit is below the roots: s.ovf is set)
            for (int i = 0; i < roots && i < 2; ++i) sampled_lds_keep(s, s.list[0][i], 0, i);
            s.cnt[1] = roots;
        }
        __syncthreads();
        const uint64_t link_key = sampled_link_key(a.seed, u, v);
        bool ovf = s.ovf, dropped = false;
        int kept_lo = 0, kept_hi = s.cnt[1];
        for (int hop = 1; hop <= a.h && !ovf; ++hop) {
            const int fringe_lo = s.cnt[0];
            __syncthreads();  // every thread has read the counters before the hop appends
            for (int f = kept_lo + grp; f < kept_hi; f += kExactGroups) {
                const int64_t y = s.key[s.list[1][f]];
                const int64_t e1 = g.rowptr[y + 1];
                for (int64_t e = g.rowptr[y] + lane; e < e1; e += kRow) {
                    if (s.ovf) break;
                    sampled_lds_visit(s, (uint32_t)g.col[e], limit);
                }
            }
            __syncthreads();
            ovf = s.ovf;
            if (ovf) break;
            const int F = s.cnt[0] - fringe_lo;  // (<= limit <= kExactMaxNodes: every entry of the range was stored)
            const int m = sampled_take(F, a.ratio, a.cap);
            dropped |= m < F;
            if (m == 0) break;
            auto id_at = [&](int i) -> int64_t { return (int64_t)s.key[s.list[0][fringe_lo + i]]; };
            if (m == F) {
                for (int i = t; i < F; i += kExactThreads) sampled_lds_keep(s, s.list[0][fringe_lo + i], hop, kept_hi + i);
                __syncthreads();
                if (t == 0) s.cnt[1] = kept_hi + F;
            } else {
                const SampledThreshold th = sampled_select(sel, id_at, F, m, sampled_hop_key(link_key, hop));
                for (int i = t; i < F; i += kExactThreads) {
                    const int slot = s.list[0][fringe_lo + i];
                    if (sampled_keep(th, id_at, F, sampled_hop_key(link_key, hop), (int64_t)s.key[slot]))
                        sampled_lds_keep(s, slot, hop, atomicAdd(&s.cnt[1], 1));
                }
            }
            __syncthreads();
            kept_lo = kept_hi;
            kept_hi = s.cnt[1];
        }
        __syncthreads();
        if (ovf) {  // (fill pass: never -- the count pass gave such a link to the slot tier)
            if (!FILL && t == 0) {
                overflow[atomicAdd(&ws->count, 1)] = (int32_t)q;
                o.state[q] = kStateSlot;
            }
            __syncthreads();
            lds_clear(s);
            continue;
        }
        const int visited = s.cnt[0] < kExactMaxNodes ? s.cnt[0] : kExactMaxNodes, kept = s.cnt[1] < kExactMaxNodes ? s.cnt[1] : kExactMaxNodes;
        if (!FILL) {
            if (t == 0) {
                o.counts[q] = kept;
                o.state[q] = dropped ? kStateSampled : 0;
            }
        } else {
            for (int i = t; i < kept; i += kExactThreads) sorted[i] = s.key[s.list[1][i]];
            lds_ordered_emit(s, sorted, kept, len, [&](int i, uint32_t x, int slot) {
                o.ids[row + i] = (int64_t)x;
                o.hop[row + i] = (uint8_t)((lds_value(s, slot) & 0x7Fu) - 1);
            });
            __syncthreads();
        }
        for (int i = t; i < visited; i += kExactThreads) lds_release(s, s.list[0][i]);  // back to an empty table
    }
}

// ---- slot tier ------------------------------------------------------------------------------------------------------------------
constexpr int kSampledFillGrid = 256 * 3;  // on-chip fill workgroups (3 per CU with the sort array)

// first visit of x?  (every access of a level byte is an agent-scope atomic, as in exact_slot_bfs)
__device__ __forceinline__ bool sampled_slot_reach(const ExactSlot &sl, int32_t x)
{
    const int sh = 8 * (x & 3);
    const uint32_t old = atomicOr(&sl.dist[x >> 2], 0x80u << sh);
    return ((old >> sh) & 0xFFu) == 0;
}
__device__ __forceinline__ void sampled_slot_keep(const ExactSlot &sl, int32_t x, int hop) { atomicOr(&sl.dist[x >> 2], (uint32_t)(hop + 1) << (8 * (x & 3))); }
__device__ __forceinline__ uint32_t sampled_slot_byte(const ExactSlot &sl, int32_t x)
{
    return (__hip_atomic_load(&sl.dist[x >> 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (8 * (x & 3))) & 0xFFu;
}

template <bool FILL>
__global__ __launch_bounds__(kExactThreads) void sampled_slot_kernel(ss_csr_graph g, const int64_t *__restrict__ links, int64_t N, SampledArgs a,
                                                                      SampledOut o, ExactWs *__restrict__ ws,
                                                                      const int32_t *__restrict__ overflow, uint32_t *__restrict__ arena)
{
    __shared__ SampledSelect sel;
    __shared__ int cnt[2];  // visited (list 0), kept (list 1)
    __shared__ int big[kBigList];
    __shared__ int n_big;
    __shared__ int wave_sum[2][kScanWaves];
    __shared__ int64_t next_q;
    const int t = threadIdx.x;
    const int grp = t / kRow, lane = t & (kRow - 1);
    const ExactSlot sl = exact_slot(arena, N);
    const int total = ws->count;
    for (;;) {
        __syncthreads();  // the last link's reads of the LDS words are over
        large_claim(ws, overflow, total, &next_q);
        if (t == 0) n_big = 0;
        __syncthreads();
        const int64_t q = next_q;
        if (q < 0) break;
        int64_t u, v;
        int64_t row = 0, len = 0;
        bool skip = !link_ids(links, q, N, u, v);  // (never listed: the on-chip tier has answered such a link)
        if (FILL && !skip) {
            fill_row(o.rowptr, q, row, len);
            skip = len <= 0;  // emptied by max_nodes
        }
        if (skip) continue;
        if (t == 0) {
            int roots = 0;
            sampled_slot_reach(sl, (int32_t)u);
            sl.list[0][roots++] = (int32_t)u;
            if (v != u) {
                sampled_slot_reach(sl, (int32_t)v);
                sl.list[0][roots++] = (int32_t)v;
            }
            for (int i = 0; i < roots; ++i) {
                sampled_slot_keep(sl, sl.list[0][i], 0);
                sl.list[1][i] = sl.list[0][i];
            }
            cnt[0] = cnt[1] = roots;
        }
        __syncthreads();
        const uint64_t link_key = sampled_link_key(a.seed, u, v);
        bool dropped = false;
        int kept_lo = 0, kept_hi = cnt[1];
        for (int hop = 1; hop <= a.h; ++hop) {
            const int fringe_lo = cnt[0];
            __syncthreads();  // every thread has read the counters before the hop appends
            for (int f = kept_lo + grp; f < kept_hi; f += kExactGroups) {
                const int32_t y = sl.list[1][f];
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
                    if (sampled_slot_reach(sl, x)) sl.list[0][atomicAdd(&cnt[0], 1)] = x;  // (each node once: at most N entries)
                }
            }
            __syncthreads();
            const int nb = n_big < kBigList ? n_big : kBigList;
            for (int b = 0; b < nb; ++b) {
                const int32_t y = big[b];
                const int64_t e1 = g.rowptr[y + 1];
                for (int64_t e = g.rowptr[y] + t; e < e1; e += kExactThreads) {
                    const int32_t x = g.col[e];
                    if (sampled_slot_reach(sl, x)) sl.list[0][atomicAdd(&cnt[0], 1)] = x;
                }
            }
            __syncthreads();
            if (t == 0) n_big = 0;
            const int F = cnt[0] - fringe_lo;
            const int m = sampled_take(F, a.ratio, a.cap);
            dropped |= m < F;
            if (m == 0) break;
            const int32_t *fringe = sl.list[0] + fringe_lo;
            auto id_at = [&](int i) -> int64_t { return (int64_t)fringe[i]; };
            if (m == F) {
                for (int i = t; i < F; i += kExactThreads) {
                    sampled_slot_keep(sl, fringe[i], hop);
                    sl.list[1][kept_hi + i] = fringe[i];
                }
                __syncthreads();
                if (t == 0) cnt[1] = kept_hi + F;
            } else {
                const SampledThreshold th = sampled_select(sel, id_at, F, m, sampled_hop_key(link_key, hop));
                for (int i = t; i < F; i += kExactThreads) {
                    const int32_t x = fringe[i];
                    if (sampled_keep(th, id_at, F, sampled_hop_key(link_key, hop), (int64_t)x)) {
                        sampled_slot_keep(sl, x, hop);
                        sl.list[1][atomicAdd(&cnt[1], 1)] = x;  // (a subset of list 0: at most N entries)
                    }
                }
            }
            __syncthreads();
            kept_lo = kept_hi;
            kept_hi = cnt[1];
        }
        __syncthreads();
        const int visited = cnt[0], kept = cnt[1];
        if (!FILL) {
            if (t == 0) {
                o.counts[q] = kept;
                o.state[q] = kStateSlot | (dropped ? kStateSampled : 0);
            }
            for (int i = t; i < visited; i += kExactThreads) slot_clear(sl, sl.list[0][i]);  // back to all-zero for the next link
            continue;
        }
        // the rejected nodes are cleared through list 0; what stays non-zero is the row
        for (int i = t; i < visited; i += kExactThreads) {
            const int32_t x = sl.list[0][i];
            if (sampled_slot_byte(sl, x) == 0x80u) slot_clear(sl, x);
        }
        __syncthreads();
        // the row holds exactly the non-zero bytes (a store never leaves it); the scan leaves them all zero for the next link
        slot_ordered_scan(sl, N, wave_sum, [&](int64_t at, int64_t x, uint32_t b) {
            if (at < len) {
                o.ids[row + at] = x;
                o.hop[row + at] = (uint8_t)((b & 0x7Fu) - 1);
            }
        });
    }
}

}  // namespace ss

// the sampling arguments' own checks, in front of tier_check and of its B == 0 early-out (h outside [1, 3] is tier_check's to answer:
// SS_ERR_UNSUPPORTED comes first)
static bool sampled_bad(int32_t h, int32_t max_nodes_per_hop, double ratio_per_hop, uint64_t seed)
{
    return h >= 1 && h <= SS_MAX_HOPS &&
           (max_nodes_per_hop < 0 || !(ratio_per_hop > 0.0 && ratio_per_hop <= 1.0) || seed >= ((uint64_t)1 << 63));  // (a NaN ratio fails too)
}

extern "C" int ss_sampled_nodes_pairs(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h,
                                      int32_t max_nodes_per_hop, double ratio_per_hop, uint64_t seed, int32_t lds_max_nodes, int32_t *counts,
                                      int32_t *state, const int64_t *rowptr, int64_t *ids, uint8_t *hop, int32_t *err_flag, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    using namespace ss;
    if (sampled_bad(h, max_nodes_per_hop, ratio_per_hop, seed)) return SS_ERR_INVALID_ARG;
    const bool fill = rowptr != nullptr;
    Tier t;
    int rc = tier_check(graph, links, B, N, h, workspace, workspace_bytes, state && (fill ? ids && hop : counts != nullptr));
    if (rc == SS_OK) rc = tier_lds(lds_max_nodes, workspace, stream, t);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (!fill && hipMemsetAsync(t.ws, 0, sizeof(ExactWs), t.stream) != hipSuccess) return SS_ERR_LAUNCH;
    const SampledArgs a = {h, max_nodes_per_hop ? max_nodes_per_hop : INT32_MAX, ratio_per_hop, seed};
    const SampledOut o = {counts, state, rowptr, ids, hop, err_flag};
    const int64_t most = fill ? kSampledFillGrid : kExactGrid;
    const dim3 grid((unsigned)(B < most ? B : most)), block(kExactThreads);
    const auto kernel = fill ? sampled_lds_kernel<true> : sampled_lds_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, t.stream, *graph, links, B, N, t.limit, a, o, t.ws, t.overflow);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_sampled_nodes_large(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h,
                                      int32_t max_nodes_per_hop, double ratio_per_hop, uint64_t seed, int32_t *counts, int32_t *state,
                                      const int64_t *rowptr, int64_t *ids, uint8_t *hop, void *workspace, size_t workspace_bytes,
                                      int32_t slots, void *arena, size_t arena_bytes, void *stream)
{
    using namespace ss;
    if (sampled_bad(h, max_nodes_per_hop, ratio_per_hop, seed)) return SS_ERR_INVALID_ARG;
    const bool fill = rowptr != nullptr;
    Tier t;
    int rc = tier_check(graph, links, B, N, h, workspace, workspace_bytes, state && (fill ? ids && hop : counts != nullptr));
    if (rc == SS_OK) rc = tier_large(N, slots, arena, arena_bytes, workspace, stream, t);
    if (rc != SS_OK) return rc > 0 ? SS_OK : rc;
    if (hipMemsetAsync(&t.ws->cursor, 0, sizeof(int32_t), t.stream) != hipSuccess) return SS_ERR_LAUNCH;  // (the list is walked once per pass)
    const SampledArgs a = {h, max_nodes_per_hop ? max_nodes_per_hop : INT32_MAX, ratio_per_hop, seed};
    const SampledOut o = {counts, state, rowptr, ids, hop, nullptr};
    const auto kernel = fill ? sampled_slot_kernel<true> : sampled_slot_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)slots), dim3(kExactThreads), 0, t.stream, *graph, links, N, a, o, t.ws, t.overflow,
                       static_cast<uint32_t *>(arena));
    SS_LAUNCH_CHECK();
    return SS_OK;
}
