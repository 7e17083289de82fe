// ss_subgraph.hip -- exact enclosing subgraphs (ElphHashes.exact_subgraphs): the induced adjacency and the SEAL node labels of the node
// rows ss_exact_nodes.hip lists.  Row q of the node list is ids[rowptr[q] .. rowptr[q + 1]), ascending; listed node t of link q has the
// LOCAL index t - rowptr[q].  Two kernel families:
//
//   ss_subgraph_adj     per listed node t (id x, link q = (u, v)): the distinct j != x of row q with an arc j -> x, as local indices,
//                       ascending, with the number of copies of the arc.  It is the intersection of two ascending lists -- row x of the
//                       CSR with SORTED rows (in-arcs, duplicates adjacent) and the link's id row -- walked from the shorter side:
//                         arcs  (deg x <= switch * n)  a lane takes an arc that starts a run of equal sources, binary-searches the id
//                                                      row for it and counts the run: the weight
//                         ids   (deg x >  switch * n)  a lane takes an id of the row and takes lower and upper bound in the CSR row:
//                                                      weight = ub - lb.  (A hub reached at the last level of a small row.)
//                       Both emit in ascending local index, so both give the same row.  One 16-lane group per listed node: rows of
//                       the modelled graphs hold about ten arcs, so a wavefront per node would idle three quarters of its lanes and a
//                       lane per node would serialise a hub's row and scatter its loads; the group's prefix sum (4 shuffles) places
//                       what its lanes found.  SS_FLAG_MASK_TARGET with u != v leaves (x = u, j = v) and (x = v, j = u) out.
//                       Variable-length rows: a count pass (int32 per listed node), the caller's cumulative sum, a fill pass that
//                       also writes the local indices of u and v (roots), once per link, by the group of the row's first node.
//   ss_subgraph_labels  one workgroup per link: level-synchronous BFS from u and from v over the emitted local adjacency ('de+' and
//                       'drnl': the other root removed first), then the label formula of the reference's labelling_tricks.py as the
//                       epilogue, straight into z.  Rows of at most lds_max_nodes (<= 2048) nodes keep the distances and the frontier
//                       queues in LDS (24 KiB: 6 workgroups per CU), larger rows in the slice of a device workspace the caller lays
//                       out (4 int32 per node of such a row).  One frontier node per 16-lane group, as the exact BFS walks.
//
// Every offset into ids, adj_ptr, nbr, weight, z and the workspace is 64-bit; a local index and a row length are below N < 2^31.
#include "ss_common.hpp"

namespace ss {

constexpr int kSubThreads = 256;
constexpr int kSubGroups = kSubThreads / kRow;
constexpr int kSubAdjGrid = 256 * 32;      // adjacency workgroups at most (grid-stride over the listed nodes)
constexpr int kSubLabelGrid = 256 * 6;     // label workgroups at most (6 per CU: 24 KiB of LDS each)
constexpr int kSubLdsNodes = 2048;         // largest row whose distances and queues live in LDS
constexpr int32_t kUnreached = 0x7FFFFFFF;
constexpr int32_t kRemoved = 0x7FFFFFFE;   // the other root in 'de+' / 'drnl': never entered

struct AdjArgs {
    const int64_t *csr_rowptr;  // [N + 1]
    const int32_t *csr_col;     // rows ascending
    const int64_t *links;       // [B, 2]
    const int64_t *rowptr;      // [B + 1]
    const int64_t *ids;         // [T]
    int64_t B, N, T;
    uint32_t flags;
    int32_t switch_ratio;
    int32_t *counts;            // count pass: [T]
    const int64_t *adj_ptr;     // fill pass: [T + 1]
    int32_t *nbr, *weight, *roots;
};

// the link that lists node t: the last q with rowptr[q] <= t (rowptr[0] = 0 <= t < T = rowptr[B]; empty rows are passed over)
__device__ __forceinline__ int64_t owner_link(const int64_t *__restrict__ rowptr, int64_t B, int64_t t)
{
    int64_t lo = 0, hi = B;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

template <bool FILL>
__global__ __launch_bounds__(kSubThreads) void subgraph_adj_kernel(AdjArgs a)
{
    const int lane = threadIdx.x & (kRow - 1);
    const int64_t stride = (int64_t)gridDim.x * kSubGroups;
    for (int64_t t = (int64_t)blockIdx.x * kSubGroups + threadIdx.x / kRow; t < a.T; t += stride) {  // (uniform in the group)
        const int64_t q = owner_link(a.rowptr, a.B, t);
        const int64_t row = a.rowptr[q], n = a.rowptr[q + 1] - row;
        int64_t u, v;
        link_ids(a.links, q, a.N, u, v);  // (the host has checked the ids)
        const int64_t x = a.ids[t];
        const bool mask = (a.flags & SS_FLAG_MASK_TARGET) && u != v;
        const int64_t skip = !mask ? -1 : x == u ? v : x == v ? u : -1;
        const int64_t e0 = a.csr_rowptr[x], deg = a.csr_rowptr[x + 1] - e0;
        const int32_t *__restrict__ col = a.csr_col + e0;
        const int64_t *__restrict__ idr = a.ids + row;
        int64_t at = 0, end = 0;
        if (FILL) {
            at = a.adj_ptr[t];
            end = a.adj_ptr[t + 1];
        }
        int total = 0;
        const bool by_ids = deg > (int64_t)a.switch_ratio * n;
        const int64_t steps = by_ids ? n : deg;
        for (int64_t i0 = 0; i0 < steps; i0 += kRow) {
            const int64_t i = i0 + lane;
            int64_t loc = 0;
            int32_t w = 0;
            if (i < steps) {
                if (by_ids) {
                    const int64_t j = idr[i];
                    if (j != x && j != skip) {
                        const int64_t lb = bound<false>(col, (int64_t)0, deg, j);
                        if (lb < deg && col[lb] == j) w = (int32_t)(bound<true>(col, (int64_t)0, deg, j) - lb);
                    }
                    loc = i;
                } else {
                    const int64_t j = col[i];
                    if ((i == 0 || col[i - 1] != j) && j != x && j != skip) {  // the first arc of a run of equal sources
                        loc = bound<false>(idr, (int64_t)0, n, j);
                        if (loc < n && idr[loc] == j) {
                            int64_t e = i + 1;
                            while (e < deg && col[e] == j) ++e;
                            w = (int32_t)(e - i);
                        }
                    }
                }
            }
            int inc = w > 0;  // inclusive prefix sum over the group: the lanes' finds ascend with the lane
#pragma unroll
            for (int d = 1; d < kRow; d <<= 1) {
                const int y = __shfl_up(inc, d, kRow);
                if (lane >= d) inc += y;
            }
            if (FILL && w > 0) {
                const int64_t o = at + total + inc - 1;
                if (o < end) {  // (the count pass found exactly these: a store never leaves the node's adjacency row)
                    a.nbr[o] = (int32_t)loc;
                    a.weight[o] = w;
                }
            }
            total += __shfl(inc, kRow - 1, kRow);
        }
        if (!FILL && lane == 0) a.counts[t] = total;
        if (FILL && t == row && lane < 2) {  // once per link: where its roots are listed (they always are)
            const int64_t r = bound<false>(idr, (int64_t)0, n, lane ? v : u);
            a.roots[2 * q + lane] = r < n ? (int32_t)r : -1;
        }
    }
}

// ---- labels -----------------------------------------------------------------------------------------------------------------------
struct LabelArgs {
    const int64_t *rowptr;   // [B + 1]
    const int32_t *roots;    // [B, 2]
    const int64_t *adj_ptr;  // [T + 1]
    const int32_t *nbr;
    const int64_t *ws_ptr;   // [B + 1]: nodes of the rows longer than the on-chip limit before row q
    int32_t *workspace;      // 4 int32 per such node
    int64_t *z;
    int64_t B, max_dist;
    int32_t mode, limit;
};

__device__ __forceinline__ int64_t label_distance(int32_t d, int64_t max_dist, int64_t partner)
{
    if (d == kRemoved) return partner < max_dist ? partner : max_dist;
    return d < max_dist ? (int64_t)d : max_dist;  // (kUnreached > max_dist: unreachable is max_dist)
}

// a depth other threads of the workgroup claim with atomics (device workspace: read where the atomics act, not from the CU's L1)
__device__ __forceinline__ int32_t depth_of(const int32_t *d, int i) { return __hip_atomic_load(&d[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// both BFSs of one row and its labels (whole workgroup).  dist0 / dist1: [n] depths from u / v; que0 / que1: [n] the nodes in the order
// each side reached them (level ranges = frontiers); cnt: the workgroup's LDS int[2].  Every thread has passed a barrier after the
// last read of dist / que / cnt when this returns
template <typename Q>
__device__ __forceinline__ void label_row(int32_t *dist0, int32_t *dist1, Q *que0, Q *que1, int *cnt, const LabelArgs &a, int64_t row,
                                          int n, int ru, int rv)
{
    const int t = threadIdx.x;
    const int grp = t / kRow, lane = t & (kRow - 1);
    const bool two = ru != rv;  // u == v: one root, nothing removed, both distances equal
    const bool remove = two && a.mode != SS_SUBGRAPH_LABEL_DE;
    for (int i = t; i < n; i += kSubThreads) {
        dist0[i] = kUnreached;
        if (two) dist1[i] = kUnreached;
    }
    __syncthreads();
    if (t == 0) {
        dist0[ru] = 0;
        que0[0] = (Q)ru;
        cnt[0] = 1;
        cnt[1] = 0;
        if (two) {
            dist1[rv] = 0;
            que1[0] = (Q)rv;
            cnt[1] = 1;
            if (remove) {
                dist0[rv] = kRemoved;
                dist1[ru] = kRemoved;
            }
        }
    }
    __syncthreads();
    int lo0 = 0, lo1 = 0, hi0 = cnt[0], hi1 = cnt[1];
    for (int level = 1; lo0 < hi0 || lo1 < hi1; ++level) {  // (workgroup-uniform)
        __syncthreads();  // every thread has read cnt before the level appends
        const int f0 = hi0 - lo0, f1 = hi1 - lo1;
        for (int f = grp; f < f0 + f1; f += kSubGroups) {
            const int side = f >= f0;
            int32_t *d = side ? dist1 : dist0;
            Q *que = side ? que1 : que0;
            const int64_t y = row + (int64_t)que[side ? lo1 + f - f0 : lo0 + f];
            const int64_t e1 = a.adj_ptr[y + 1];
            for (int64_t e = a.adj_ptr[y] + lane; e < e1; e += kRow) {
                const int32_t j = a.nbr[e];
                if ((uint32_t)j >= (uint32_t)n) continue;  // (never: a local index of the row)
                if (depth_of(d, j) == kUnreached && atomicCAS(&d[j], kUnreached, level) == kUnreached) {
                    const int p = atomicAdd(&cnt[side], 1);
                    if (p < n) que[p] = (Q)j;  // (always: a node is claimed once)
                }
            }
        }
        __syncthreads();
        lo0 = hi0;
        lo1 = hi1;
        hi0 = cnt[0] < n ? cnt[0] : n;
        hi1 = cnt[1] < n ? cnt[1] : n;
    }
    // the epilogue: labelling_tricks.py on the two distances
    const int64_t md = a.max_dist;
    const int64_t partner = a.mode == SS_SUBGRAPH_LABEL_DRNL ? 0 : 1;
    for (int i = t; i < n; i += kSubThreads) {
        const int64_t du = label_distance(depth_of(dist0, i), md, partner);
        const int64_t dv = two ? label_distance(depth_of(dist1, i), md, partner) : du;
        if (a.mode == SS_SUBGRAPH_LABEL_DRNL) {
            const int64_t s = du + dv, half = s / 2;
            int64_t z = 1 + (du < dv ? du : dv) + half * (half + s % 2 - 1);
            if (du == 0 || dv == 0) z = 1;
            a.z[row + i] = z;
        } else {
            a.z[2 * (row + i)] = du;
            a.z[2 * (row + i) + 1] = dv;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kSubThreads) void subgraph_labels_kernel(LabelArgs a)
{
    __shared__ int32_t s_dist[2][kSubLdsNodes];
    __shared__ uint16_t s_que[2][kSubLdsNodes];
    __shared__ int cnt[2];
    for (int64_t q = blockIdx.x; q < a.B; q += gridDim.x) {
        const int64_t row = a.rowptr[q], len = a.rowptr[q + 1] - row;
        if (len <= 0) continue;  // capped by max_nodes
        const int n = (int)len;
        const int ru = a.roots[2 * q], rv = a.roots[2 * q + 1];
        if ((uint32_t)ru >= (uint32_t)n || (uint32_t)rv >= (uint32_t)n) continue;  // (never: a row lists its roots)
        if (n <= a.limit) {
            label_row<uint16_t>(s_dist[0], s_dist[1], s_que[0], s_que[1], cnt, a, row, n, ru, rv);
        } else if (a.workspace) {
            int32_t *base = a.workspace + 4 * a.ws_ptr[q];
            label_row<int32_t>(base, base + n, base + 2 * (int64_t)n, base + 3 * (int64_t)n, cnt, a, row, n, ru, rv);
        }
    }
}

}  // namespace ss

extern "C" int ss_subgraph_adj(const int64_t *csr_rowptr, const int32_t *csr_col, int64_t N, const int64_t *links, int64_t B,
                               const int64_t *rowptr, const int64_t *ids, int64_t T, uint32_t flags, int32_t switch_ratio, int32_t *counts,
                               const int64_t *adj_ptr, int32_t *nbr, int32_t *weight, int32_t *roots, void *stream)
{
    using namespace ss;
    if (B < 0 || N < 0 || T < 0) return SS_ERR_INVALID_ARG;
    if (B == 0 || T == 0) return SS_OK;
    if (!csr_rowptr || !csr_col || !links || !rowptr || !ids || N == 0 || N >= ((int64_t)1 << 31) || switch_ratio < 0) return SS_ERR_INVALID_ARG;
    const bool fill = adj_ptr != nullptr;
    if (fill ? (!nbr || !weight || !roots) : !counts) return SS_ERR_INVALID_ARG;
    const AdjArgs a = {csr_rowptr, csr_col, links, rowptr, ids, B, N, T, flags, switch_ratio, counts, adj_ptr, nbr, weight, roots};
    const int64_t blocks = (T + kSubGroups - 1) / kSubGroups;
    const dim3 grid((unsigned)(blocks < kSubAdjGrid ? blocks : kSubAdjGrid)), block(kSubThreads);
    if (fill)
        hipLaunchKernelGGL((subgraph_adj_kernel<true>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((subgraph_adj_kernel<false>), grid, block, 0, (hipStream_t)stream, a);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_subgraph_labels(const int64_t *rowptr, int64_t B, const int32_t *roots, const int64_t *adj_ptr, const int32_t *nbr,
                                  int32_t label_mode, int64_t max_dist, int32_t lds_max_nodes, const int64_t *ws_ptr, int32_t *workspace,
                                  int64_t *z, void *stream)
{
    using namespace ss;
    if (label_mode != SS_SUBGRAPH_LABEL_DRNL && label_mode != SS_SUBGRAPH_LABEL_DE && label_mode != SS_SUBGRAPH_LABEL_DE_PLUS)
        return SS_ERR_UNSUPPORTED;
    if (B < 0 || max_dist < 1 || max_dist > SS_SUBGRAPH_MAX_DIST || lds_max_nodes < 0) return SS_ERR_INVALID_ARG;
    if (B == 0) return SS_OK;
    if (!rowptr || !roots || !adj_ptr || !nbr || !ws_ptr || !z) return SS_ERR_INVALID_ARG;  // (workspace: null when no row needs it)
    const int limit = lds_max_nodes < kSubLdsNodes ? lds_max_nodes : kSubLdsNodes;
    const LabelArgs a = {rowptr, roots, adj_ptr, nbr, ws_ptr, workspace, z, B, max_dist, label_mode, limit};
    const dim3 grid((unsigned)(B < kSubLabelGrid ? B : kSubLabelGrid)), block(kSubThreads);
    hipLaunchKernelGGL(subgraph_labels_kernel, grid, block, 0, (hipStream_t)stream, a);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
