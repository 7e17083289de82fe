// ss_update.hip -- incremental update of the sketch tables: after a few edges were added or removed, only the rows within k hops
// downstream of the touched targets are recomputed at hop k.
//
// The reference has no counterpart: build_hash_tables (hashing.py:139-165) recomputes every row of every hop, and its dataset
// construction (src/data.py:173-176 + datasets/elph.py) does so once per split for graphs that differ by a few per cent of their edges.
//
// Two kernel families:
//   mark + list  update_seed_kernel scatters the seed flags (targets of the changed edges), update_mark_kernel -- one launch per hop --
//                pulls the previous hop's byte map over the in-edge CSR (row i is dirty at hop k if it is a seed, if it was dirty at hop
//                k - 1 and has its implicit self loop, or if one of its in-neighbours was dirty at hop k - 1), writes this hop's byte map
//                and compacts it into an int32 row list with a device-side count.  Flags are plain byte stores of 1 (no atomics on
//                them: the map does not depend on scheduling); the only atomics are one add per workgroup on the list counters, so a
//                list is ascending inside a workgroup's 256 rows and in arrival order between workgroups.  Rows with more in-edges than
//                graph.hub_threshold go to a list of their own, filled from the END of the same array.
//   row hops     persistent workgroups over rows[0 .. *n) -- the count never leaves the device -- that recompute a listed row from
//                scratch by CALLING the row bodies of the build kernels (ss_walks.hpp: minhash_hop_row, hll_hop_row, hll_hop_row16,
//                first_hop_minhash_row, hll_first_hop_row16; ss_hub.hpp: first_hop_hub_walk / first_hop_hub_finish).  The arithmetic,
//                the lane mapping and the order of the statistics are SHARED with ss_propagate.hip / ss_first_hop.hip, not repeated:
//                a recomputed row (and its cardinality) carries the bits a rebuild would give it because it runs the rebuild's code,
//                and a change to a row body changes both.  Only the output side differs (a plain store here, store + peers' tables
//                in the build).  Listed hub rows are walked by one 16-wavefront workgroup each, partials combined through LDS; hub
//                rows that are not dirty are never touched.
#include "ss_hub.hpp"

namespace ss {

constexpr int kUpdHeaderBytes = 256;   // int32 counters: word 0 = seed rows, words 4k .. 4k+2 = hop k: dirty rows, row list, hub list
constexpr int kUpdRowGrid = 2048;      // persistent workgroups of a row launch (eight per CU)
constexpr int kUpdHubGrid = 256;
constexpr int kUpdHubThreads = 1024;
constexpr int kUpdHubWaves = kUpdHubThreads / kWave;
constexpr int kMarkSolo = 32;          // in-edges a single lane walks on its own
constexpr int kMarkWave = 2048;        // ... a wavefront walks; longer rows are walked by the whole workgroup

inline size_t upd_pad(int64_t N) { return (size_t)((N + 255) & ~(int64_t)255); }

struct UpdateWs {
    int32_t *counters;
    uint8_t *flags[SS_MAX_HOPS];
    int32_t *list[SS_MAX_HOPS];
};

inline UpdateWs carve_update_ws(void *ws, int64_t N, int h)
{
    UpdateWs w = {};
    uint8_t *base = static_cast<uint8_t *>(ws);
    const size_t pad = upd_pad(N);
    w.counters = reinterpret_cast<int32_t *>(base);
    for (int k = 0; k < h; ++k) {
        w.flags[k] = base + kUpdHeaderBytes + (size_t)k * pad;
        w.list[k] = reinterpret_cast<int32_t *>(base + kUpdHeaderBytes + (size_t)h * pad + (size_t)k * 4 * pad);
    }
    return w;
}

// ---- mark + list ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void update_seed_kernel(const int64_t *__restrict__ added, int64_t n_added, const int64_t *__restrict__ removed,
                                                          int64_t n_removed, int64_t N, uint8_t *__restrict__ flags, int32_t *err_flag)
{
    const int64_t n = n_added + n_removed;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = t < n_added ? added[t] : removed[t - n_added];
        if ((uint64_t)id >= (uint64_t)N) {
            if (err_flag) *err_flag = SS_CSR_ERR_BOUNDS;  // (a plain store, as the CSR build's: the word may be pinned host memory)
        } else {
            flags[id] = 1;
        }
    }
}

// FIRST: hop 1 (dirty_1 = seed: the scattered flags plus the rows whose implicit self loop appeared or disappeared);
// otherwise hop k from the map of hop k - 1.  `seed` and `out` are the same map for FIRST (a thread reads and writes its own byte).
template <bool FIRST>
__global__ __launch_bounds__(256) void update_mark_kernel(GraphArgs g, const uint8_t *seed, const uint8_t *prev, uint8_t *out,
                                                          const float *__restrict__ cards_old, int64_t cards_stride, int32_t *list,
                                                          int32_t *counters, int32_t *seed_count)
{
    __shared__ int s_big[256];
    __shared__ int s_nbig, s_hit;
    __shared__ int s_wcount[256 / kWave][2];
    __shared__ int s_base[2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t first = (int64_t)blockIdx.x * 256;
    const int64_t i = first + tid;
    const bool ok = i < g.N;
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    int64_t rb = 0;
    int deg = 0;
    if (ok) {
        rb = g.rowptr[i];
        deg = (int)(g.rowptr[i + 1] - rb);
    }
    bool f = false;
    if (ok) {
        // a row had its self loop iff its old hop-1 HLL row was non-zero iff its old hop-1 cardinality is positive
        if (FIRST) f = seed[i] != 0 || ((i < n_self) != (cards_old[i * cards_stride] > 0.0f));
        else f = seed[i] != 0 || (i < n_self && prev[i] != 0);
    }
    if (tid == 0) s_nbig = 0;
    __syncthreads();
    if (!FIRST) {
        // short rows: the lane walks its own in-edges, early exit on the first dirty neighbour
        if (ok && !f && deg <= kMarkSolo) {
            for (int t = 0; t < deg; ++t)
                if (prev[g.col[rb + t]] != 0) {
                    f = true;
                    break;
                }
        }
        // longer rows: one after the other by the whole wavefront, 64 in-edges per step
        unsigned long long pend = __ballot(ok && !f && deg > kMarkSolo && deg <= kMarkWave);
        while (pend) {  // wave-uniform
            const int src = __ffsll((long long)pend) - 1;
            pend &= pend - 1;
            const int64_t rbs = ((int64_t)__shfl((int)((uint64_t)rb >> 32), src) << 32) | (uint32_t)__shfl((int)rb, src);
            const int degs = __shfl(deg, src);
            bool hit = false;
            for (int t0 = 0; t0 < degs && !hit; t0 += kWave) {
                const int t = t0 + lane;
                const bool h = t < degs && prev[g.col[rbs + t]] != 0;
                hit = __any(h) != 0;
            }
            if (lane == src) f = hit;
        }
        // hub rows: by the whole workgroup, four in-edges per thread in flight
        if (ok && !f && deg > kMarkWave) s_big[atomicAdd(&s_nbig, 1)] = tid;
        __syncthreads();
        const int nbig = s_nbig;
        for (int m = 0; m < nbig; ++m) {  // workgroup-uniform
            const int r = s_big[m];
            if (tid == 0) s_hit = 0;
            __syncthreads();
            const int64_t rbb = g.rowptr[first + r];
            const int dd = (int)(g.rowptr[first + r + 1] - rbb);
            for (int t0 = 0; t0 < dd; t0 += 4 * 256) {
                if (*(volatile int *)&s_hit) break;
                int id[4];
                uint8_t fl[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = t0 + u * 256 + tid;
                    id[u] = g.col[rbb + (t < dd ? t : dd - 1)];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) fl[u] = prev[id[u]];
                if (fl[0] | fl[1] | fl[2] | fl[3]) s_hit = 1;  // (a slot past the end repeats the row's last in-edge: harmless)
            }
            __syncthreads();
            if (tid == r) f = s_hit != 0;
            __syncthreads();
        }
    }
    if (ok) out[i] = f ? 1 : 0;

    // compaction: regular rows from the front of `list`, hub rows from its end
    const bool hub = f && deg > g.hub_threshold, reg = f && !hub;
    const unsigned long long br = __ballot(reg), bh = __ballot(hub);
    if (lane == 0) {
        s_wcount[wave][0] = __popcll(br);
        s_wcount[wave][1] = __popcll(bh);
    }
    __syncthreads();
    if (tid == 0) {
        int nr = 0, nh = 0;
        for (int w = 0; w < 256 / kWave; ++w) {
            nr += s_wcount[w][0];
            nh += s_wcount[w][1];
        }
        s_base[0] = nr ? atomicAdd(&counters[1], nr) : 0;
        s_base[1] = nh ? atomicAdd(&counters[2], nh) : 0;
        if (nr + nh) atomicAdd(&counters[0], nr + nh);
        if (FIRST && nr + nh) atomicAdd(seed_count, nr + nh);
    }
    __syncthreads();
    int off_r = s_base[0], off_h = s_base[1];
    for (int w = 0; w < wave; ++w) {
        off_r += s_wcount[w][0];
        off_h += s_wcount[w][1];
    }
    const unsigned long long below = lane ? (~0ull >> (kWave - lane)) : 0ull;
    if (reg) list[off_r + __popcll(br & below)] = (int32_t)i;
    if (hub) list[g.N - 1 - (off_h + __popcll(bh & below))] = (int32_t)i;
}

// ---- row hops over a device-counted list ----------------------------------------------------------------------------------------
__device__ __forceinline__ int uniform_row(const int32_t *__restrict__ list, int64_t q) { return __builtin_amdgcn_readfirstlane(list[q]); }

// Every kernel below keeps the list indexing and the row bounds and CALLS the row bodies of the build kernels (ss_walks.hpp, ss_hub.hpp)
// with a plain store for an output side: there is no second copy of the arithmetic here.

// MinHash table hop, one wavefront per listed row
template <int TP>
__global__ __launch_bounds__(256) void update_minhash_rows_kernel(GraphArgs g, const int32_t *__restrict__ list, const int32_t *__restrict__ n_ptr,
                                                                  const uint32_t *__restrict__ mh_in, uint32_t *__restrict__ mh_out, int P_rt)
{
    const int P = TP ? TP : P_rt;
    const int lane = threadIdx.x & (kWave - 1);
    const int n = *n_ptr;
    const int waves = blockDim.x / kWave;
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    for (int64_t q = (int64_t)blockIdx.x * waves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave)); q < n; q += (int64_t)gridDim.x * waves) {
        const int64_t i = uniform_row(list, q);
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        minhash_hop_row<TP>(mh_in, g.col + rb, deg, total, i, P, lane, 0, 1, [&](int c, bool mine, const u32x4 &acc) {
            if (mine) *reinterpret_cast<u32x4 *>(mh_out + i * P + 4 * c) = acc;
        });
    }
}

// HLL table hop + cardinality, any M, one wavefront per listed row
__global__ __launch_bounds__(256) void update_hll_rows_kernel(GraphArgs g, const int32_t *__restrict__ list, const int32_t *__restrict__ n_ptr,
                                                              const uint8_t *__restrict__ hll_in, uint8_t *__restrict__ hll_out, int M,
                                                              float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm)
{
    __shared__ EstimatorLds lds;
    const EstimatorTables est = stage_tables(lds, prm);
    const int lane = threadIdx.x & (kWave - 1);
    const int n = *n_ptr;
    const int waves = blockDim.x / kWave;
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    for (int64_t q = (int64_t)blockIdx.x * waves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave)); q < n; q += (int64_t)gridDim.x * waves) {
        const int64_t i = uniform_row(list, q);
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        hll_hop_row<0>(
            hll_in, g.col + rb, deg, total, i, M, lane, 0, 1, true, est,
            [&](int c, bool mine, const u32x4 &acc) {
                if (mine) *reinterpret_cast<u32x4 *>(hll_out + i * M + 16 * c) = acc;
                return mine;
            },
            [&](float card) { cards_out[i * cards_stride] = card; });
    }
}

// HLL table hop at M = 256: four listed rows per wavefront, one 16-lane group each (hll_hop_row16, as hll_propagate_row16_kernel)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void update_hll256_rows_kernel(
    GraphArgs g, const int32_t *__restrict__ list, const int32_t *__restrict__ n_ptr, const uint8_t *__restrict__ hll_in,
    uint8_t *__restrict__ hll_out, float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm)
{
    __shared__ EstimatorLds lds;
    const EstimatorTables est = stage_tables(lds, prm);
    const int n = *n_ptr;
    const int grp = threadIdx.x / kRow, groups = blockDim.x / kRow;
    for (int64_t q0 = (int64_t)blockIdx.x * groups; q0 < n; q0 += (int64_t)gridDim.x * groups) {  // workgroup-uniform
        const int64_t q = q0 + grp;
        const int64_t row = q < n ? (int64_t)list[q] : -1;
        hll_hop_row16(g, row, false, hll_in, hll_out, cards_out, cards_stride, est, true, threadIdx.x & (kRow - 1));
    }
}

// MinHash first hop from node ids, one wavefront per listed row
template <int PPL>
__global__ __launch_bounds__(256) void update_first_minhash_rows_kernel(GraphArgs g, const int32_t *__restrict__ list, const int32_t *__restrict__ n_ptr,
                                                                        const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb,
                                                                        uint32_t *__restrict__ mh_out, int p)
{
    constexpr int P = PPL * kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int n = *n_ptr;
    const int waves = blockDim.x / kWave;
    const int64_t q_first = (int64_t)blockIdx.x * waves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (q_first >= n) return;
    uint64_t a[PPL], b[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        a[q] = pa[lane + kWave * q];
        b[q] = pb[lane + kWave * q];
    }
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    for (int64_t qi = q_first; qi < n; qi += (int64_t)gridDim.x * waves) {
        const int64_t i = uniform_row(list, qi);
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        uint32_t acc[PPL];
        first_hop_minhash_row<PPL>(g.col + rb, deg, total, i, p, a, b, acc, lane, true);
#pragma unroll
        for (int q = 0; q < PPL; ++q) mh_out[i * P + lane + kWave * q] = acc[q];
    }
}

// HLL first hop from node ids (p = 8), one 16-lane group per listed row through its LDS row image
__global__ __launch_bounds__(256) void update_first_hll_rows_kernel(GraphArgs g, const int32_t *__restrict__ list, const int32_t *__restrict__ n_ptr,
                                                                    int p, uint8_t *__restrict__ hll_out, float *__restrict__ cards_out,
                                                                    int64_t cards_stride, ss_hll_params prm)
{
    __shared__ LcLds<257> lds;
    __shared__ __attribute__((aligned(16))) uint32_t rows[256 / kRow][256];
    const EstimatorTables est = stage_lc_only(lds, prm);
    const int l = threadIdx.x & (kRow - 1);
    const int grp = threadIdx.x / kRow, groups = blockDim.x / kRow;
    const int n = *n_ptr;
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    const int32_t *always_valid = reinterpret_cast<const int32_t *>(g.rowptr);
    for (int64_t q0 = (int64_t)blockIdx.x * groups; q0 < n; q0 += (int64_t)gridDim.x * groups) {  // workgroup-uniform
        const int64_t q = q0 + grp;
        const bool ok = q < n;
        const int64_t i = ok ? (int64_t)list[q] : 0;
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = ok ? deg + (i < n_self ? 1 : 0) : 0;
        const int32_t *nb = g.col + rb;
        const int nid0 = *(l < deg ? nb + l : always_valid);
        hll_first_hop_row16<false>(rows[grp], nb, deg, total, i, nid0, always_valid, p, ok, hll_out, cards_out, cards_stride, est, true, l, g.mir);
    }
}

// ---- listed hub rows: one 16-wavefront workgroup per row, entries N - 1, N - 2, ... of the list -------------------------------------
// table hop, any P / M: wavefront w is part w of 16 of the row bodies' neighbour walk; the wavefronts' folds of a chunk meet in `part`
// and wavefront 0 stores the row
__global__ __launch_bounds__(kUpdHubThreads) void update_hub_table_kernel(GraphArgs g, const int32_t *__restrict__ list, const int32_t *__restrict__ n_ptr,
                                                                          const uint32_t *__restrict__ mh_in, uint32_t *__restrict__ mh_out, int P,
                                                                          const uint8_t *__restrict__ hll_in, uint8_t *__restrict__ hll_out, int M,
                                                                          float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm)
{
    __shared__ EstimatorLds lds;
    __shared__ u32x4 part[kUpdHubWaves][kWave];
    const int n = *n_ptr;
    if ((int)blockIdx.x >= n) return;  // the common case (no dirty hub row) costs one scalar load per workgroup
    EstimatorTables est = {};
    if (hll_out) est = stage_tables(lds, prm);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    // the chunk's folds of all wavefronts -> wavefront 0 (a lane that holds a chunk is a lane of sub-group 0: lane = chunk lane);
    // called by every thread; true: the lane holds the finished chunk
    auto combine = [&](bool mine, u32x4 &acc, auto fold) {
        if (mine) part[wave][lane] = acc;
        __syncthreads();
        const bool done = wave == 0 && mine;
        if (done)
            for (int w = 1; w < kUpdHubWaves; ++w) acc = fold(acc, part[w][lane]);
        __syncthreads();
        return done;
    };
    for (int q = blockIdx.x; q < n; q += gridDim.x) {  // workgroup-uniform
        const int64_t i = list[g.N - 1 - q];
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        const int32_t *nb = g.col + rb;
        if (mh_out)
            minhash_hop_row<0>(mh_in, nb, deg, total, i, P, lane, wave, kUpdHubWaves, [&](int c, bool mine, u32x4 &acc) {
                if (combine(mine, acc, min4)) *reinterpret_cast<u32x4 *>(mh_out + i * P + 4 * c) = acc;
            });
        if (hll_out)
            hll_hop_row<0>(
                hll_in, nb, deg, total, i, M, lane, wave, kUpdHubWaves, wave == 0, est,
                [&](int c, bool mine, u32x4 &acc) {
                    const bool done = combine(mine, acc, bytemax16);
                    if (done) *reinterpret_cast<u32x4 *>(hll_out + i * M + 16 * c) = acc;
                    return done;
                },
                [&](float card) { cards_out[i * cards_stride] = card; });
    }
}

// first hop from node ids: one whole row per workgroup through the walk and the finish of the build's hub units (ss_hub.hpp)
template <int PPL, bool DO_MH, bool DO_HLL>
__global__ __launch_bounds__(kUpdHubThreads) void update_hub_first_kernel(GraphArgs g, const int32_t *__restrict__ list, const int32_t *__restrict__ n_ptr,
                                                                          const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pb,
                                                                          uint32_t *__restrict__ mh_out, int p, uint8_t *__restrict__ hll_out,
                                                                          float *__restrict__ cards_out, int64_t cards_stride, ss_hll_params prm)
{
    __shared__ EstimatorLds lds;
    __shared__ FirstHopHubLds<PPL> s;
    const int n = *n_ptr;
    if ((int)blockIdx.x >= n) return;
    EstimatorTables est = {};
    if (DO_HLL) est = stage_tables(lds, prm);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    uint64_t a[PPL], b[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        a[q] = DO_MH ? pa[lane + kWave * q] : 0ULL;
        b[q] = DO_MH ? pb[lane + kWave * q] : 0ULL;
    }
    const int64_t n_self = g.n_self_dev ? *g.n_self_dev : g.n_self;
    for (int qi = blockIdx.x; qi < n; qi += gridDim.x) {  // workgroup-uniform
        const int64_t i = list[g.N - 1 - qi];
        const int64_t rb = g.rowptr[i];
        const int deg = (int)(g.rowptr[i + 1] - rb);
        const int total = deg + (i < n_self ? 1 : 0);
        first_hop_hub_walk<PPL, kUpdHubWaves, DO_MH, DO_HLL>(s, i, g.col + rb, deg, 0, total, p, a, b, lane, wave);
        // (the update keeps the all-zero rule for a listed row without any neighbour; the build's hub units have no such rule)
        if (wave == 0) first_hop_hub_finish<PPL, DO_MH, DO_HLL, false>(s, i, total == 0, mh_out, hll_out, cards_out, cards_stride, est, DO_HLL, lane, g.mir);
        __syncthreads();
    }
}

}  // namespace ss

extern "C" size_t ss_update_workspace_bytes(int64_t N, int32_t h)
{
    if (N < 0 || N >= ((int64_t)1 << 31) || h < 1 || h > SS_MAX_HOPS) return 0;
    return ss::kUpdHeaderBytes + (size_t)h * 5 * ss::upd_pad(N);
}

extern "C" int ss_update_mark(const ss_csr_graph *graph, const int64_t *added_dst, int64_t n_added, const int64_t *removed_dst, int64_t n_removed,
                              const float *cards_old, int64_t cards_stride, int32_t h, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                              void *stream)
{
    using namespace ss;
    if (h < 1 || h > SS_MAX_HOPS) return SS_ERR_UNSUPPORTED;
    if (!graph_given(graph) || n_added < 0 || n_removed < 0) return SS_ERR_INVALID_ARG;
    if ((n_added > 0 && !added_dst) || (n_removed > 0 && !removed_dst)) return SS_ERR_INVALID_ARG;
    const int64_t N = graph->num_nodes;
    if (N == 0) return SS_OK;
    // (written out, here and in ss_update_hop: the update lists its own hub rows and asks nothing of hub_rows / hub_count)
    if (N >= ((int64_t)1 << 31) || !cards_old || cards_stride < 1 || !workspace || !graph->col) return SS_ERR_INVALID_ARG;
    if (graph->row_begin != 0 || graph->row_end != 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < ss_update_workspace_bytes(N, h)) return SS_ERR_WORKSPACE;
    const GraphArgs g = to_args(*graph);
    const UpdateWs w = carve_update_ws(workspace, N, h);
    hipStream_t s = (hipStream_t)stream;
    // the counters and the seed map (adjacent in the workspace) start at zero
    if (hipMemsetAsync(workspace, 0, kUpdHeaderBytes + upd_pad(N), s) != hipSuccess) return SS_ERR_LAUNCH;
    const int64_t n = n_added + n_removed;
    if (n > 0) {
        const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        hipLaunchKernelGGL(update_seed_kernel, dim3(blocks), dim3(256), 0, s, added_dst, n_added, removed_dst, n_removed, N, w.flags[0], err_flag);
        SS_LAUNCH_CHECK();
    }
    const unsigned grid = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL((update_mark_kernel<true>), dim3(grid), dim3(256), 0, s, g, (const uint8_t *)w.flags[0], (const uint8_t *)nullptr, w.flags[0],
                       cards_old, cards_stride, w.list[0], w.counters + 4, w.counters);
    SS_LAUNCH_CHECK();
    for (int k = 2; k <= h; ++k) {
        hipLaunchKernelGGL((update_mark_kernel<false>), dim3(grid), dim3(256), 0, s, g, (const uint8_t *)w.flags[0], (const uint8_t *)w.flags[k - 2],
                           w.flags[k - 1], cards_old, cards_stride, w.list[k - 1], w.counters + 4 * k, w.counters);
        SS_LAUNCH_CHECK();
    }
    return SS_OK;
}

extern "C" int ss_update_hop(const ss_csr_graph *graph, int32_t hop, int32_t h, const uint64_t *a, const uint64_t *b, const uint32_t *mh_in,
                             uint32_t *mh_out, int32_t P, const uint8_t *hll_in, uint8_t *hll_out, int32_t p, float *cards_out,
                             int64_t cards_stride, const ss_hll_params *prm, const void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ss;
    if (h < 1 || h > SS_MAX_HOPS) return SS_ERR_UNSUPPORTED;
    if (!graph_given(graph) || hop < 1 || hop > h) return SS_ERR_INVALID_ARG;
    if (P <= 0 || (P & 3) || P > 2048) return SS_ERR_INVALID_ARG;
    if (p < 4 || p > 16) return SS_ERR_UNSUPPORTED;
    if (!mh_in && (hop != 1 || P % kWave || P > 256)) return SS_ERR_UNSUPPORTED;  // MinHash from node ids: the first hop, 64 .. 256 permutations
    if (!hll_in && (hop != 1 || p != 8)) return SS_ERR_UNSUPPORTED;               // HLL from node ids: the first hop at p = 8
    const int64_t N = graph->num_nodes;
    if (N == 0) return SS_OK;
    if (N >= ((int64_t)1 << 31) || !mh_out || !hll_out || !cards_out || !workspace || !graph->col) return SS_ERR_INVALID_ARG;
    if (!mh_in && (!a || !b)) return SS_ERR_INVALID_ARG;
    if (graph->row_begin != 0 || graph->row_end != 0) return SS_ERR_INVALID_ARG;
    HopRequest r;
    r.a = a;
    r.b = b;
    r.P = P;
    r.p = p;
    r.M = 1 << p;
    r.mh_in = mh_in;
    r.mh_out = mh_out;
    r.hll_in = hll_in;
    r.hll_out = hll_out;
    r.cards_out = cards_out;
    r.cards_stride = cards_stride;
    r.stream = (hipStream_t)stream;
    const int rc = take_params(r, prm);
    if (rc != SS_OK) return rc;
    if (workspace_bytes < ss_update_workspace_bytes(N, h)) return SS_ERR_WORKSPACE;
    r.g = to_args(*graph);
    const UpdateWs w = carve_update_ws(const_cast<void *>(workspace), N, h);
    const int32_t *list = w.list[hop - 1];
    const int32_t *n_rows = w.counters + 4 * hop + 1, *n_hubs = w.counters + 4 * hop + 2;
    // launches are sized by N, the bound the host knows; the workgroups stride over the device-side counts
    const unsigned grid4 = (unsigned)((N + 3) / 4 < kUpdRowGrid ? (N + 3) / 4 : kUpdRowGrid);
    const unsigned grid16 = (unsigned)((N + 15) / 16 < kUpdRowGrid ? (N + 15) / 16 : kUpdRowGrid);
    const unsigned hub_grid = (unsigned)(N < kUpdHubGrid ? N : kUpdHubGrid);
    // the listed hub rows of a first hop, one sketch per launch; the other sketch's arguments are nulls and zeros
    const auto hub_first = [&](auto ppl, auto mh, auto hll) {
        constexpr bool MH = decltype(mh)::value, HLL = decltype(hll)::value;
        hipLaunchKernelGGL((update_hub_first_kernel<decltype(ppl)::value, MH, HLL>), dim3(hub_grid), dim3(kUpdHubThreads), 0, r.stream, r.g, list, n_hubs,
                           MH ? r.a : nullptr, MH ? r.b : nullptr, MH ? r.mh_out : nullptr, r.p, HLL ? r.hll_out : nullptr,
                           HLL ? r.cards_out : nullptr, HLL ? r.cards_stride : (int64_t)0, HLL ? r.prm : ss_hll_params{});
    };

    // ---- HLL rows + cardinalities
    if (!r.hll_in) {
        hipLaunchKernelGGL(update_first_hll_rows_kernel, dim3(grid16), dim3(256), 0, r.stream, r.g, list, n_rows, r.p, r.hll_out, r.cards_out,
                           r.cards_stride, r.prm);
        SS_LAUNCH_CHECK();
        hub_first(std::integral_constant<int, 1>{}, std::false_type{}, std::true_type{});
    } else if (r.M == 256) {
        hipLaunchKernelGGL(update_hll256_rows_kernel, dim3(grid16), dim3(256), 0, r.stream, r.g, list, n_rows, r.hll_in, r.hll_out, r.cards_out,
                           r.cards_stride, r.prm);
    } else {
        hipLaunchKernelGGL(update_hll_rows_kernel, dim3(grid4), dim3(256), 0, r.stream, r.g, list, n_rows, r.hll_in, r.hll_out, r.M, r.cards_out,
                           r.cards_stride, r.prm);
    }
    SS_LAUNCH_CHECK();
    // ---- MinHash rows
    if (!r.mh_in) {
        for_ppl(r.P, [&](auto ppl) {
            hipLaunchKernelGGL((update_first_minhash_rows_kernel<decltype(ppl)::value>), dim3(grid4), dim3(256), 0, r.stream, r.g, list, n_rows, r.a, r.b,
                               r.mh_out, r.p);
            hub_first(ppl, std::true_type{}, std::false_type{});
        });
    } else if (r.P == 128) {
        hipLaunchKernelGGL((update_minhash_rows_kernel<128>), dim3(grid4), dim3(256), 0, r.stream, r.g, list, n_rows, r.mh_in, r.mh_out, r.P);
    } else {
        hipLaunchKernelGGL((update_minhash_rows_kernel<0>), dim3(grid4), dim3(256), 0, r.stream, r.g, list, n_rows, r.mh_in, r.mh_out, r.P);
    }
    SS_LAUNCH_CHECK();
    // ---- listed hub rows of the sketches that read a table (one launch serves both when both do)
    if (r.mh_in || r.hll_in) {
        hipLaunchKernelGGL(update_hub_table_kernel, dim3(hub_grid), dim3(kUpdHubThreads), 0, r.stream, r.g, list, n_hubs, r.mh_in,
                           r.mh_in ? r.mh_out : nullptr, r.P, r.hll_in, r.hll_in ? r.hll_out : nullptr, r.M, r.cards_out, r.cards_stride, r.prm);
        SS_LAUNCH_CHECK();
    }
    return SS_OK;
}
