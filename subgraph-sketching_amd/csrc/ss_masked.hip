// ss_masked.hip -- target-link masking: the subgraph features of a link (u, v) as the tables of the graph WITHOUT that link would give
// them, for every link of a batch at once (ElphHashes.get_subgraph_features(mask_target=edge_index)).
//
// The reference removes the target link from every enclosing subgraph on its SEAL path (src/datasets/seal.py:338); its sketch path
// (hashing.py:139-165, 258-323) cannot: a table row is a min / max fold over a neighbourhood, and a fold cannot be undone for one
// neighbour.  Here the leave-one-out rows are REBUILT, on chip, from what does not change:
//   N'(x)  the in-neighbours of x with the partner left out when x is u or v (every copy of u -> v and v -> u goes; self loops stay)
//   R1(x)  x in {u, v}: fold of the hop-0 values -- pure functions of the node id -- over N'(x) and x itself
//   H1(y)  R1(y) for y in {u, v}, the stored hop-1 row T1(y) for every other node (its closed in-neighbourhood holds no removed edge)
//   R2(x)  fold of H1(w) over w in N'(x), and R1(x)
//   R3(x)  R2(x), folded with H1(w) and H1(y), y in N'(w), for every w in N'(x)
// (fold = min for MinHash, byte-wise max for HLL; folds are idempotent, so walks are not de-duplicated).  An endpoint of an edge lies
// below n_self = max(edge_index) + 1, so u, v and every in-neighbour carry their implicit self loop and no fold is ever empty.
//
// Launches of one call, none of them sized by anything read from the device, nothing read by the host in between:
//   ss_pair_features         the plain query writes EVERY row: a link that is not an edge keeps those bits
//   masked_classify_kernel   one 16-lane group per link scans rows u and v of the CSR for the partner; links that are edges (either
//                            direction) are compacted into an int32 list with a device-side count
//   masked_row_zeros_kernel  (debug outputs only) the zero-register counts of the 2h stored rows of every link
//   masked_pairs_kernel      workgroups stride over the list: the 2h masked rows of a link are built in LDS (4P + M bytes each), then
//                            one 16-lane group runs the pair arithmetic of ss_pair_math.hpp and the feature algebra of
//                            ss_feature_algebra.hpp on them, with the cardinalities of the masked rows from hll_row16_stats +
//                            hll_estimate -- the statistics function is shared with masked_row_zeros_kernel, the hop-0 values
//                            (permuted_hash, hll_rank_of / hll_register_of) with the first-hop kernels of the build -- and
//                            overwrites the link's output row
// A workgroup walks a row with 256 / (P / 4 + M / 16) neighbours in flight (one 16-byte chunk per thread), whatever the row's length:
// a link next to a hub is slow, never wrong.
#include "ss_feature_algebra.hpp"
#include "ss_pair_math.hpp"
#include "ss_walks.hpp"

namespace ss {

constexpr int kMaskedThreads = 256;
constexpr int kMaskedHeaderBytes = 256;  // int32 word 0: links listed
constexpr int kMaskedGrid = 4096;        // workgroups of masked_pairs_kernel (they stride over the device-side count)

// ---- which links are edges ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMaskedThreads) void masked_classify_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                         int64_t N, const int64_t *__restrict__ links, int64_t B,
                                                                         int32_t *__restrict__ counter, int32_t *__restrict__ list,
                                                                         uint8_t *__restrict__ dbg_masked)
{
    const int l = threadIdx.x & (kRow - 1), lane = threadIdx.x & (kWave - 1);
    const int groups = kMaskedThreads / kRow;
    for (int64_t q0 = (int64_t)blockIdx.x * groups; q0 < B; q0 += (int64_t)gridDim.x * groups) {  // workgroup-uniform
        const int64_t q = q0 + threadIdx.x / kRow;
        int hit = 0;
        if (q < B) {
            int64_t u, v;
            if (link_ids(links, q, N, u, v) && u != v) {
                // row x of the CSR lists the sources j of the edges j -> x: v -> u sits in row u, u -> v in row v
                const int64_t ue = rowptr[u + 1], ve = rowptr[v + 1];
                for (int64_t e = rowptr[u] + l; e < ue && !hit; e += kRow) hit = col[e] == (int32_t)v;
                for (int64_t e = rowptr[v] + l; e < ve && !hit; e += kRow) hit = col[e] == (int32_t)u;
            }
        }
        const bool edge = row16_sum_i(hit) != 0;
        const bool mark = edge && l == 0 && q < B;
        const unsigned long long bal = __ballot(mark);
        if (bal) {  // wave-uniform: one add per wavefront
            const int leader = __ffsll((long long)bal) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(counter, __popcll(bal));
            base = __shfl(base, leader);
            const unsigned long long below = lane ? (~0ull >> (kWave - lane)) : 0ull;
            if (mark) list[base + __popcll(bal & below)] = (int32_t)q;
        }
        if (dbg_masked && l == 0 && q < B) dbg_masked[q] = edge ? 1 : 0;
    }
}

// ---- debug: zero registers of the stored rows of every link (the masked kernel overwrites those of the links it serves) ------------
__global__ __launch_bounds__(kMaskedThreads) void masked_row_zeros_kernel(const int64_t *__restrict__ links, int64_t B, int64_t N, int h,
                                                                          HopTables tabs, int M, int32_t *__restrict__ row_zeros)
{
    const int l = threadIdx.x & (kRow - 1);
    const int groups = kMaskedThreads / kRow;
    const int CH = M >> 4;
    for (int64_t q0 = (int64_t)blockIdx.x * groups; q0 < B; q0 += (int64_t)gridDim.x * groups) {  // workgroup-uniform
        const int64_t q = q0 + threadIdx.x / kRow;
        int64_t u = 0, v = 0;
        const bool ok = q < B && link_ids(links, q, N, u, v);
        for (int side = 0; side < 2; ++side)
            for (int k = 0; k < h; ++k) {
                const int64_t x = side ? v : u;
                int nonzero;
                float hsum;
                hll_row16_stats(reinterpret_cast<const u32x4 *>(tabs.hll[k] + x * M), ok ? CH : 0, l, nonzero, hsum);
                if (q < B && l == 0) row_zeros[q * (2 * h) + side * h + k] = ok ? M - nonzero : 0;
            }
    }
}

// ---- the masked rows of one link, built by one workgroup ----------------------------------------------------------------------------
// A sketch row in LDS: CM = P / 4 MinHash chunks, then CH = M / 16 HLL chunks (W4 = CM + CH <= 256 chunks of 16 bytes).  Thread t owns
// chunk t % W4 of neighbour slot t / W4: S = 256 / W4 neighbours of a walk are in flight, their partial folds meet in `partial`.
struct MaskedLink {
    const int64_t *rowptr;
    const int32_t *col;
    HopTables tabs;
    int64_t u, v;
    int P, M, CM, W4, S;
    u32x4 *rows;     // [2][H][W4]: side (u, v), hop - 1
    u32x4 *partial;  // [256]
    uint32_t *regs;  // [M]: the HLL registers of a first hop, one word each
    int H;

    __device__ __forceinline__ u32x4 *row(int side, int k) const { return rows + (side * H + k) * W4; }
    __device__ __forceinline__ int64_t partner_of(int64_t x) const { return x == u ? v : (x == v ? u : -1); }
    __device__ __forceinline__ u32x4 identity(int c) const
    {
        return c < CM ? u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu} : u32x4{0u, 0u, 0u, 0u};
    }
    __device__ __forceinline__ u32x4 fold(u32x4 acc, u32x4 x, int c) const { return c < CM ? min4(acc, x) : bytemax16(acc, x); }
    // chunk c of H1(y)
    __device__ __forceinline__ u32x4 h1(int64_t y, int c) const
    {
        if (y == u) return row(0, 0)[c];
        if (y == v) return row(1, 0)[c];
        return c < CM ? *reinterpret_cast<const u32x4 *>(tabs.mh[0] + y * P + 4 * c)
                      : *reinterpret_cast<const u32x4 *>(tabs.hll[0] + y * M + 16 * (c - CM));
    }
    // the slots' partial folds and `extra` (a finished row of the same node) -> dst; workgroup-uniform call
    __device__ __forceinline__ void reduce(u32x4 acc, bool active, int slot, int c, const u32x4 *extra, u32x4 *dst) const
    {
        if (active) partial[slot * W4 + c] = acc;
        __syncthreads();
        const int t = threadIdx.x;
        if (t < W4) {
            u32x4 r = partial[t];
            for (int s = 1; s < S; ++s) r = fold(r, partial[s * W4 + t], t);
            r = fold(r, extra[t], t);
            dst[t] = r;
        }
        __syncthreads();
    }
};

// R1(x): MinHash and HLL first hop of x over N'(x) + x from node ids (hop-0 values by permuted_hash and hll_rank_of / hll_register_of,
// the helpers of the first-hop kernels)
__device__ __forceinline__ void masked_first_hop(const MaskedLink &L, int side, const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb,
                                                 int p, bool self)
{
    const int t = threadIdx.x;
    const int64_t x = side ? L.v : L.u, partner = side ? L.u : L.v;
    const int64_t rb = L.rowptr[x];
    const int deg = (int)(L.rowptr[x + 1] - rb);
    const int32_t *nb = L.col + rb;
    const int total = deg + (self ? 1 : 0);
    uint32_t *dst = reinterpret_cast<uint32_t *>(L.row(side, 0));
    // MinHash: thread = (neighbour slot, permutation) while P <= 256, else one slot and permutations t, t + 256, ...
    const int P = L.P;
    const int S1 = P <= kMaskedThreads ? kMaskedThreads / P : 1;
    uint32_t *part = reinterpret_cast<uint32_t *>(L.partial);
    const int slot = P <= kMaskedThreads ? t / P : 0;
    for (int j = P <= kMaskedThreads ? t % P : t; j < P; j += kMaskedThreads) {
        uint32_t acc = 0xFFFFFFFFu;
        if (slot < S1) {
            const uint64_t aj = pa[j], bj = pb[j];
            for (int e = slot; e < total; e += S1) {
                const int64_t nid = e < deg ? (int64_t)nb[e] : x;
                if (e < deg && nid == partner) continue;
                const uint32_t hv = permuted_hash(aj, bj, hash_u64((uint64_t)(nid + 1)));
                acc = hv < acc ? hv : acc;
            }
            if (S1 > 1) part[slot * P + j] = acc;
            else dst[j] = acc;
        }
        if (P <= kMaskedThreads) break;
    }
    // HLL: one register per neighbour, scattered into LDS words (hashing.py:126-137)
    const int M = L.M;
    for (int i = t; i < M; i += kMaskedThreads) L.regs[i] = 0u;
    __syncthreads();
    if (S1 > 1 && t < P) {
        uint32_t r = part[t];
        for (int s = 1; s < S1; ++s) r = part[s * P + t] < r ? part[s * P + t] : r;
        dst[t] = r;
    }
    for (int e = t; e < total; e += kMaskedThreads) {
        const int64_t nid = e < deg ? (int64_t)nb[e] : x;
        if (e < deg && nid == partner) continue;
        const uint64_t hv = hash_u64((uint64_t)(nid + 1));
        atomicMax(&L.regs[hll_register_of(hv, M)], hll_rank_of(hv, p));
    }
    __syncthreads();
    uint32_t *dst_h = reinterpret_cast<uint32_t *>(L.row(side, 0) + L.CM);
    for (int d = t; d < (M >> 2); d += kMaskedThreads)
        dst_h[d] = L.regs[4 * d] | (L.regs[4 * d + 1] << 8) | (L.regs[4 * d + 2] << 16) | (L.regs[4 * d + 3] << 24);
    __syncthreads();
}

template <int H>
__global__ __launch_bounds__(kMaskedThreads) void masked_pairs_kernel(GraphArgs g, const int64_t *__restrict__ links, int64_t N,
                                                                      const int32_t *__restrict__ counter, const int32_t *__restrict__ list,
                                                                      const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb,
                                                                      HopTables tabs, int P, ss_hll_params prm, uint32_t flags,
                                                                      float *__restrict__ out, int32_t *__restrict__ dbg_match,
                                                                      int32_t *__restrict__ dbg_zero, int32_t *__restrict__ dbg_row_zeros)
{
    extern __shared__ u32x4 dyn[];
    __shared__ EstimatorLds lds;
    const int n = *counter;
    if ((int)blockIdx.x >= n) return;  // (workgroup-uniform) a batch without edge links costs one scalar load per workgroup
    const EstimatorTables est = stage_tables(lds, prm);
    constexpr int NF = H * (H + 2);
    constexpr int NC = H * H;
    const int t = threadIdx.x;
    const int p = prm.p;
    MaskedLink L;
    L.rowptr = g.rowptr;
    L.col = g.col;
    L.tabs = tabs;
    L.P = P;
    L.M = 1 << p;
    L.CM = P >> 2;
    const int CH = L.M >> 4;
    L.W4 = L.CM + CH;
    L.S = kMaskedThreads / L.W4;
    L.H = H;
    L.rows = dyn;
    L.partial = dyn + 2 * H * L.W4;
    L.regs = reinterpret_cast<uint32_t *>(L.partial + kMaskedThreads);
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    const int c = t % L.W4, slot = t / L.W4;
    const bool active = slot < L.S;

    for (int i = blockIdx.x; i < n; i += gridDim.x) {  // workgroup-uniform
        const int64_t q = list[i];
        int64_t u, v;
        link_ids(links, q, N, u, v);  // (listed links are in range and have u != v)
        L.u = u;
        L.v = v;
        masked_first_hop(L, 0, pa, pb, p, u < n_self);
        masked_first_hop(L, 1, pa, pb, p, v < n_self);
        if constexpr (H >= 2) {
            for (int side = 0; side < 2; ++side) {
                const int64_t x = side ? v : u, partner = side ? u : v;
                const int64_t rb = g.rowptr[x];
                const int deg = (int)(g.rowptr[x + 1] - rb);
                const int32_t *nb = g.col + rb;
                u32x4 acc = L.identity(c);
                if (active)
                    for (int e = slot; e < deg; e += L.S) {
                        const int64_t w = nb[e];
                        if (w == partner) continue;
                        acc = L.fold(acc, L.h1(w, c), c);
                    }
                L.reduce(acc, active, slot, c, L.row(side, 0), L.row(side, 1));
                if constexpr (H >= 3) {
                    acc = L.identity(c);
                    for (int e = 0; e < deg; ++e) {  // workgroup-uniform: the slots share the walk of every w in N'(x)
                        const int64_t w = nb[e];
                        if (w == partner) continue;
                        const int64_t wb = g.rowptr[w];
                        const int wdeg = (int)(g.rowptr[w + 1] - wb);
                        const int32_t *wnb = g.col + wb;
                        const int64_t wpartner = L.partner_of(w);
                        if (active)
                            for (int s = slot; s <= wdeg; s += L.S) {  // s == wdeg: w itself (a source lies below n_self)
                                const int64_t y = s < wdeg ? (int64_t)wnb[s] : w;
                                if (s < wdeg && y == wpartner) continue;
                                acc = L.fold(acc, L.h1(y, c), c);
                            }
                    }
                    L.reduce(acc, active, slot, c, L.row(side, 1), L.row(side, 2));
                }
            }
        }
        // ---- the pair arithmetic on the masked rows: one 16-lane group, lane l takes chunks l, l + 16, ... (eq4 / union_stats of
        // ss_pair_math.hpp on LDS rows, as pair_features_kernel's run-time-shape path applies them to table rows)
        if (t < kWave) {
            const int l = t & (kRow - 1);
            const int CM = L.CM;
            int mz[NC];
            float hs[NC];
#pragma unroll
            for (int k1 = 0; k1 < H; ++k1)
#pragma unroll
                for (int k2 = 0; k2 < H; ++k2) {
                    const u32x4 *ru = L.row(0, k1), *rv = L.row(1, k2);
                    pair_stats_generic(ru, rv, ru + CM, rv + CM, CM, CH, l, mz[k1 * H + k2], hs[k1 * H + k2]);
                }
            // cardinalities of the masked rows (hll_row16_stats: the statistics of a finished row, as for the stored rows above)
            float c1[H], c2[H];
            int rz[2 * H];
#pragma unroll
            for (int side = 0; side < 2; ++side)
#pragma unroll
                for (int k = 0; k < H; ++k) {
                    int nonzero;
                    float hsum;
                    hll_row16_stats(L.row(side, k) + CM, CH, l, nonzero, hsum);
                    rz[side * H + k] = L.M - nonzero;
                    const float card = hll_estimate(est, L.M - nonzero, hsum);
                    if (side == 0) c1[k] = card;
                    else c2[k] = card;
                }
            // (written out, not a shared function: that moved the VGPRs at h >= 2, a wavefront per SIMD at h = 3 -- DESIGN_EXPERIMENTS "One source for the pair finish")
            const int my_mz = lane_select(mz, l);
            const float my_hs = lane_select(hs, l);
            float my_I = 0.0f;
            const int my_match = (int)((uint32_t)my_mz >> 20), my_zeros = my_mz & 0xFFFFF;
            if (l < NC) my_I = intersection_estimate(est, my_match, my_zeros, my_hs, P);
            const int row_base = t & ~(kRow - 1);
            float I[H][H];
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) I[cc / H][cc % H] = __shfl(my_I, row_base + cc);
            float f[NF];
            assemble_features<H>(I, c1, c2, flags, f);
            const float my_f = lane_select(f, l);
            const int my_rz = lane_select(rz, l);
            if (t < kRow) {
                if (l < NF) out[q * NF + l] = my_f;
                if (l < NC) {
                    if (dbg_match) dbg_match[q * NC + l] = my_match;
                    if (dbg_zero) dbg_zero[q * NC + l] = my_zeros;
                }
                if (l < 2 * H && dbg_row_zeros) dbg_row_zeros[q * (2 * H) + l] = my_rz;
            }
        }
        __syncthreads();  // the rows are the next link's scratch
    }
}

}  // namespace ss

extern "C" size_t ss_masked_workspace_bytes(int64_t B)
{
    if (B < 0 || B >= ((int64_t)1 << 31)) return 0;
    return ss::kMaskedHeaderBytes + (((size_t)B * 4 + 255) & ~(size_t)255);
}

extern "C" int ss_masked_pair_features(const ss_csr_graph *graph, const int64_t *links, int64_t B, int64_t N, int32_t h, const uint64_t *a,
                                       const uint64_t *b, const uint32_t *const *mh, int32_t P, const uint8_t *const *hll, const float *cards,
                                       int64_t cards_stride, const ss_hll_params *prm, uint32_t flags, float *out, int32_t *dbg_match,
                                       int32_t *dbg_zero, int32_t *dbg_row_zeros, uint8_t *dbg_masked, int32_t *err_flag, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    using namespace ss;
    const int rc = check_pair_query_args(h, B >= 0 && N >= 0 && B < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), prm, P, B == 0);
    if (rc != SS_OK || B == 0) return rc;
    if (!graph || !graph->rowptr || !graph->col || graph->num_nodes != N || !a || !b || !mh || !hll || !workspace) return SS_ERR_INVALID_ARG;
    if (graph->row_begin != 0 || graph->row_end != 0) return SS_ERR_INVALID_ARG;
    const int M = 1 << prm->p;
    const int W4 = (P >> 2) + (M >> 4);
    if (W4 > kMaskedThreads) return SS_ERR_UNSUPPORTED;  // a sketch row is walked with one 16-byte chunk per thread
    if (workspace_bytes < ss_masked_workspace_bytes(B)) return SS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // every row from the plain query: links that are not edges keep these bits
    const int rq = ss_pair_features(links, B, N, h, mh, P, hll, cards, cards_stride, prm, flags, out, dbg_match, dbg_zero, nullptr, err_flag,
                                    stream);
    if (rq != SS_OK) return rq;
    HopTables tabs;
    if (!fill_hop_tables(mh, hll, h, tabs)) return SS_ERR_INVALID_ARG;  // (the plain query above has seen every entry)
    int32_t *counter = static_cast<int32_t *>(workspace);
    int32_t *list = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(workspace) + kMaskedHeaderBytes);
    if (hipMemsetAsync(workspace, 0, kMaskedHeaderBytes, s) != hipSuccess) return SS_ERR_LAUNCH;
    const int groups = kMaskedThreads / kRow;
    const unsigned grid16 = (unsigned)((B + groups - 1) / groups < 8192 ? (B + groups - 1) / groups : 8192);
    hipLaunchKernelGGL(masked_classify_kernel, dim3(grid16), dim3(kMaskedThreads), 0, s, graph->rowptr, graph->col, N, links, B, counter, list,
                       dbg_masked);
    SS_LAUNCH_CHECK();
    if (dbg_row_zeros) {
        hipLaunchKernelGGL(masked_row_zeros_kernel, dim3(grid16), dim3(kMaskedThreads), 0, s, links, B, N, (int)h, tabs, M, dbg_row_zeros);
        SS_LAUNCH_CHECK();
    }
    const GraphArgs g = to_args(*graph);
    const size_t dyn = ((size_t)2 * h * W4 + kMaskedThreads) * 16 + (size_t)M * 4;
    const unsigned grid = (unsigned)(B < kMaskedGrid ? B : kMaskedGrid);
    dispatch_h(h, [&](auto H) {
        hipLaunchKernelGGL(masked_pairs_kernel<H()>, dim3(grid), dim3(kMaskedThreads), dyn, s, g, links, N, counter, list, a, b, tabs, (int)P, *prm,
                           flags, out, dbg_match, dbg_zero, dbg_row_zeros);
    });
    SS_LAUNCH_CHECK();
    return SS_OK;
}
