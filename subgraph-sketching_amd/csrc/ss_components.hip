// ss_components.hip -- connected components of an edge_index and the induced subgraph of a node set: what connected_components /
// induced_subgraph / largest_component_subgraph return (components.py).  Replaces, on the host side of the reference,
// get_component (src/lcc.py:34-44: a Python set walk that scans `row` once per visited node), get_largest_connected_component
// (src/lcc.py:7-15), get_node_mapper / remap_edges (src/lcc.py:18-32) and the edge filter of use_lcc (src/data.py:241-249).
//
// Labels: a lock-free union-find over the edges as given (no CSR).  parent[x] <= x always: a hook puts the LARGER root under the
// SMALLER one, a compression replaces a parent by a smaller id of the same tree, so every chain descends strictly and the root of a
// tree is the smallest id of its component -- the labels are a function of the graph, not of the interleaving.
//
//   who decides what   the only operation that joins two trees is atomicCAS(parent[hi], hi, lo): it succeeds only if hi IS a root at
//                      the instant the memory side executes it.  Everything else -- the walks of cc_find, the test ra == rb -- reads
//                      parent with plain (L1-bypassing, possibly another XCD's stale L2) loads.  Every value such a load can return was
//                      once stored in that word, hence is an id <= x of a node that was then, and is still, in x's tree (trees only
//                      merge).  So a stale value can name a node that is no longer x's parent or no longer a root; it cannot name a
//                      node of another tree.  ra == rb is therefore always a true "same tree"; a stale "root" is caught by the CAS,
//                      which returns the word's current value, and the lane goes on FROM THAT VALUE.
//   termination        cc_find moves from x to a loaded parent p and stops when p == x; otherwise p < x.  A failed CAS returns
//                      old < hi and the lane continues with (old, lo): max(ra, rb) or the sum ra + rb strictly decreases with every
//                      retry.  Ids are bounded below by 0, so every loop ends after at most ra + rb steps whatever the other lanes do.
//                      No lane waits for, spins on or polls a value another lane or workgroup has yet to write; there is no flag, no
//                      ticket, no hand-off in this unit.
//   compression        halving: when the parent p of x is not a root as read, parent[x] becomes min(parent[x], parent[p]) by atomicMin
//                      (no return value).  x is a non-root (a value != x was read from its word, and a non-root never becomes a root
//                      again), the new value is smaller and of the same tree: chains still descend and still end in the tree's root.
//
// Sizes: size[label[x]] += 1, aggregated per wavefront: the lanes that share the label of the first remaining lane add their count
// with ONE atomic (kCcPeel rounds, then one atomic per leftover lane).  Inside a giant component a wavefront sends one add instead of
// 64 to the same word.  Roots (label[x] == x), selected nodes and kept edges are compacted IN ORDER by the same two-pass scheme: a count
// pass leaves one count per workgroup (a workgroup owns SS_COMPONENTS_CHUNK consecutive items), the caller's cumulative sum turns them
// into offsets, the fill pass ranks the kept items of a 256-item tile by ballot / mbcnt and a 4-entry LDS scan across the wavefronts.
// Order is never left to an atomic.  The largest component is one 64-bit atomicMax per wavefront of the root fill pass on the key
// (size << 32) | (0xFFFFFFFF - root): the largest size, ties to the smallest root.
#include "ss_common.hpp"

namespace ss {

constexpr int kCcBlock = 256;
constexpr int kCcTiles = SS_COMPONENTS_CHUNK / kCcBlock;
constexpr int kCcPeel = 4;  // labels of a wavefront that get one aggregated add each (sizes kernel)
static_assert(SS_COMPONENTS_CHUNK % kCcBlock == 0, "a workgroup's chunk is a whole number of tiles");

__device__ __forceinline__ int32_t cc_load(const int32_t *p) { return __hip_atomic_load(const_cast<int32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as far as the loaded values say (a stale "root" is caught by the caller's CAS); halves the path on the way
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t x)
{
    int32_t p = cc_load(parent + x);
    while (p != x) {  // p < x
        const int32_t gp = cc_load(parent + p);  // gp <= p
        if (gp != p) (void)__hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

// an id of the input as a node: torch-style negative indexing, then the bounds
__device__ __forceinline__ bool cc_node(int64_t &x, int64_t N)
{
    x = x < 0 ? x + N : x;
    return (uint64_t)x < (uint64_t)N;
}

__global__ __launch_bounds__(kCcBlock) void cc_init_kernel(int32_t *__restrict__ parent, int64_t N)
{
    const int64_t stride = (int64_t)gridDim.x * kCcBlock;
    for (int64_t x = (int64_t)blockIdx.x * kCcBlock + threadIdx.x; x < N; x += stride) parent[x] = (int32_t)x;
}

__global__ __launch_bounds__(kCcBlock) void cc_hook_kernel(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, int64_t E, int64_t N,
                                                           int32_t *parent, int32_t *err)
{
    const int64_t stride = (int64_t)gridDim.x * kCcBlock;
    for (int64_t e = (int64_t)blockIdx.x * kCcBlock + threadIdx.x; e < E; e += stride) {
        int64_t a = src[e], b = dst[e];
        if (!cc_node(a, N) | !cc_node(b, N)) {  // the edge is ignored
            if (err) *err = 1;
            continue;
        }
        int32_t ra = (int32_t)a, rb = (int32_t)b;
        for (;;) {
            ra = cc_find(parent, ra);
            rb = cc_find(parent, rb);
            if (ra == rb) break;  // one tree already (self-loops, repeated edges, edges inside a tree)
            const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
            const int32_t old = atomicCAS(parent + hi, hi, lo);
            if (old == hi) break;  // hi was a root and now hangs under lo
            ra = old;              // hi had been hooked or compressed meanwhile: old < hi, go on from there
            rb = lo;
        }
    }
}

__global__ __launch_bounds__(kCcBlock) void cc_flatten_kernel(int32_t *parent, int32_t *__restrict__ label, int64_t N)
{
    const int64_t stride = (int64_t)gridDim.x * kCcBlock;
    for (int64_t x = (int64_t)blockIdx.x * kCcBlock + threadIdx.x; x < N; x += stride) label[x] = cc_find(parent, (int32_t)x);
}

__device__ __forceinline__ int cc_lane() { return threadIdx.x & (kWave - 1); }

// the sum over the workgroup of one wave-uniform count per wavefront (every thread calls; every thread gets the total)
__device__ __forceinline__ int cc_block_total(int wave_count, int32_t *lds)
{
    __syncthreads();  // (the readers of an earlier use are done)
    if (cc_lane() == 0) lds[threadIdx.x / kWave] = wave_count;
    __syncthreads();
    int total = 0;
    for (int k = 0; k < kCcBlock / kWave; ++k) total += lds[k];
    return total;
}

// the rank of this thread's item among the kept items of the workgroup's tile, in thread order, and their number
__device__ __forceinline__ int cc_tile_rank(bool keep, int32_t *lds, int &total)
{
    const unsigned long long m = __ballot(keep);
    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int w = threadIdx.x / kWave;
    __syncthreads();
    if (cc_lane() == 0) lds[w] = __builtin_popcountll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int k = 0; k < kCcBlock / kWave; ++k) {
        const int c = lds[k];
        before += k < w ? c : 0;
        total += c;
    }
    return before + below;
}

__device__ __forceinline__ int64_t cc_block_offset(const int64_t *__restrict__ block_incl) { return blockIdx.x ? block_incl[blockIdx.x - 1] : 0; }

// size[label[x]] += 1 for the nodes of the workgroup's chunk; block_roots[b] = the roots among them
__global__ __launch_bounds__(kCcBlock) void cc_sizes_kernel(const int32_t *__restrict__ label, int64_t N, int32_t *size, int32_t *__restrict__ block_roots)
{
    __shared__ int32_t lds[kCcBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * SS_COMPONENTS_CHUNK;
    const int lane = cc_lane();
    int roots = 0;
    for (int i = 0; i < kCcTiles; ++i) {
        const int64_t x = base + i * kCcBlock + threadIdx.x;
        const bool live = x < N;
        const int32_t l = live ? label[x] : -1;
        roots += __builtin_popcountll(__ballot(live && l == x));
        unsigned long long rest = __ballot(live);  // wave-uniform: the lanes whose node is not counted yet
        for (int round = 0; round < kCcPeel && rest; ++round) {
            const int leader = __builtin_ctzll(rest);
            const int32_t ll = __shfl(l, leader);
            const unsigned long long same = __ballot(live && l == ll) & rest;
            if (lane == leader) atomicAdd(size + ll, (int32_t)__builtin_popcountll(same));
            rest &= ~same;
        }
        if ((rest >> lane) & 1) atomicAdd(size + l, 1);
    }
    const int total = cc_block_total(roots, lds);
    if (threadIdx.x == 0) block_roots[blockIdx.x] = total;
}

// roots ascending with their sizes, and the largest component's key
__global__ __launch_bounds__(kCcBlock) void cc_roots_kernel(const int32_t *__restrict__ label, const int32_t *__restrict__ size, int64_t N,
                                                            const int64_t *__restrict__ block_incl, int64_t *__restrict__ roots,
                                                            int64_t *__restrict__ sizes, unsigned long long *best)
{
    __shared__ int32_t lds[kCcBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * SS_COMPONENTS_CHUNK;
    int64_t run = cc_block_offset(block_incl);
    unsigned long long key = 0;
    for (int i = 0; i < kCcTiles; ++i) {
        const int64_t x = base + i * kCcBlock + threadIdx.x;
        const bool keep = x < N && label[x] == x;
        int total;
        const int rank = cc_tile_rank(keep, lds, total);
        if (keep) {
            const int32_t s = size[x];
            roots[run + rank] = x;
            sizes[run + rank] = s;
            const unsigned long long k = ((unsigned long long)(uint32_t)s << 32) | (0xFFFFFFFFu - (uint32_t)x);
            key = k > key ? k : key;
        }
        run += total;
    }
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other > key ? other : key;
    }
    if (cc_lane() == 0 && key) atomicMax(best, key);
}

// the nodes of a set, ascending, and their new ids: the set is mask[x] != 0, or (mask == nullptr) label[x] == the root in *best
template <bool FILL>
__global__ __launch_bounds__(kCcBlock) void cc_select_kernel(const uint8_t *__restrict__ mask, const int32_t *__restrict__ label,
                                                             const unsigned long long *__restrict__ best, int64_t N,
                                                             const int64_t *__restrict__ block_incl, int32_t *__restrict__ block_count,
                                                             int64_t *__restrict__ nodes, int64_t *__restrict__ mapper)
{
    __shared__ int32_t lds[kCcBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * SS_COMPONENTS_CHUNK;
    const int32_t root = mask ? 0 : (int32_t)(0xFFFFFFFFu - (uint32_t)*best);
    int64_t run = FILL ? cc_block_offset(block_incl) : 0;
    int kept = 0;
    for (int i = 0; i < kCcTiles; ++i) {
        const int64_t x = base + i * kCcBlock + threadIdx.x;
        const bool keep = x < N && (mask ? mask[x] != 0 : label[x] == root);
        if (FILL) {
            int total;
            const int rank = cc_tile_rank(keep, lds, total);
            if (keep) nodes[run + rank] = x;
            if (x < N) mapper[x] = keep ? run + rank : -1;
            run += total;
        } else {
            kept += __builtin_popcountll(__ballot(keep));
        }
    }
    if (!FILL) {
        const int total = cc_block_total(kept, lds);
        if (threadIdx.x == 0) block_count[blockIdx.x] = total;
    }
}

// mapper[nodes[i]] = i over a mapper preset to -1; a second writer of a word finds it taken: the list repeats a node
__global__ __launch_bounds__(kCcBlock) void cc_scatter_kernel(const int64_t *__restrict__ nodes, int64_t n, int64_t N, int64_t *mapper, int32_t *err,
                                                              int32_t *dup)
{
    const int64_t i = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
    if (i >= n) return;
    int64_t x = nodes[i];
    if (!cc_node(x, N)) {
        if (err) *err = 1;
        return;
    }
    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(mapper + x), ~0ULL, (unsigned long long)i);
    if (old != ~0ULL && dup) *dup = 1;
}

// the edges with both endpoints in the set, in their original order, renumbered, with their positions
template <bool FILL>
__global__ __launch_bounds__(kCcBlock) void cc_edges_kernel(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, int64_t E, int64_t N,
                                                            const int64_t *__restrict__ mapper, const int64_t *__restrict__ block_incl,
                                                            int32_t *__restrict__ block_count, int64_t *__restrict__ out_src,
                                                            int64_t *__restrict__ out_dst, int64_t *__restrict__ edge_ids, int32_t *err)
{
    __shared__ int32_t lds[kCcBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * SS_COMPONENTS_CHUNK;
    int64_t run = FILL ? cc_block_offset(block_incl) : 0;
    int kept = 0;
    for (int i = 0; i < kCcTiles; ++i) {
        const int64_t e = base + i * kCcBlock + threadIdx.x;
        int64_t a = -1, b = -1;
        if (e < E) {
            a = src[e];
            b = dst[e];
            if (cc_node(a, N) & cc_node(b, N)) {
                a = mapper[a];
                b = mapper[b];
            } else {  // the edge is ignored
                if (!FILL && err) *err = 1;
                a = b = -1;
            }
        }
        const bool keep = a >= 0 && b >= 0;
        if (FILL) {
            int total;
            const int rank = cc_tile_rank(keep, lds, total);
            if (keep) {
                out_src[run + rank] = a;
                out_dst[run + rank] = b;
                edge_ids[run + rank] = e;
            }
            run += total;
        } else {
            kept += __builtin_popcountll(__ballot(keep));
        }
    }
    if (!FILL) {
        const int total = cc_block_total(kept, lds);
        if (threadIdx.x == 0) block_count[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kCcBlock) void cc_same_kernel(const int32_t *__restrict__ label, int64_t N, const int64_t *__restrict__ links, int64_t L,
                                                           uint8_t *__restrict__ out, int32_t *err)
{
    const int64_t q = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
    if (q >= L) return;
    int64_t u, v;
    const bool ok = link_ids(links, q, N, u, v);
    if (!ok && err) *err = 1;
    out[q] = ok && label[u] == label[v];
}

constexpr int64_t kCcLimit = (int64_t)1 << 31;  // node ids, edge positions and per-workgroup counts are 32-bit inside the unit

inline unsigned cc_stride_grid(int64_t n)  // grid-stride launches: enough workgroups to fill the part, never more than the work
{
    const int64_t blocks = (n + kCcBlock - 1) / kCcBlock;
    return (unsigned)(blocks < 4096 ? blocks : 4096);
}
inline unsigned cc_chunk_grid(int64_t n) { return (unsigned)((n + SS_COMPONENTS_CHUNK - 1) / SS_COMPONENTS_CHUNK); }

}  // namespace ss

extern "C" int ss_components_labels(const int64_t *src, const int64_t *dst, int64_t E, int64_t N, int32_t *parent, int32_t *label,
                                    int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= kCcLimit || E < 0 || E >= kCcLimit) return SS_ERR_INVALID_ARG;
    if (N == 0) return SS_OK;  // (edges of a graph without nodes are all out of range; the host module rejects them)
    if (!parent || !label || (E > 0 && (!src || !dst))) return SS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_init_kernel, dim3(cc_stride_grid(N)), dim3(kCcBlock), 0, s, parent, N);
    SS_LAUNCH_CHECK();
    if (E > 0) {
        hipLaunchKernelGGL(cc_hook_kernel, dim3(cc_stride_grid(E)), dim3(kCcBlock), 0, s, src, dst, E, N, parent, err_flag);
        SS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_stride_grid(N)), dim3(kCcBlock), 0, s, parent, label, N);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_components_sizes(const int32_t *label, int64_t N, int32_t *size, int32_t *block_roots, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= kCcLimit) return SS_ERR_INVALID_ARG;
    if (N == 0) return SS_OK;
    if (!label || !size || !block_roots) return SS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t)N, s) != hipSuccess) return SS_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(cc_chunk_grid(N)), dim3(kCcBlock), 0, s, label, N, size, block_roots);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_components_roots(const int32_t *label, const int32_t *size, int64_t N, const int64_t *block_incl, int64_t *roots, int64_t *sizes,
                                   uint64_t *best, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= kCcLimit) return SS_ERR_INVALID_ARG;
    if (N == 0) return SS_OK;
    if (!label || !size || !block_incl || !roots || !sizes || !best) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cc_roots_kernel, dim3(cc_chunk_grid(N)), dim3(kCcBlock), 0, (hipStream_t)stream, label, size, N, block_incl, roots, sizes,
                       reinterpret_cast<unsigned long long *>(best));
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_induced_select(const uint8_t *mask, const int32_t *label, const uint64_t *best, int64_t N, const int64_t *block_incl,
                                 int32_t *block_count, int64_t *nodes, int64_t *mapper, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= kCcLimit) return SS_ERR_INVALID_ARG;
    if (N == 0) return SS_OK;
    if ((mask != nullptr) == (label != nullptr) || (label != nullptr) != (best != nullptr)) return SS_ERR_INVALID_ARG;  // one way to say the set
    const auto *key = reinterpret_cast<const unsigned long long *>(best);
    if (!block_incl) {  // count pass
        if (!block_count) return SS_ERR_INVALID_ARG;
        hipLaunchKernelGGL(cc_select_kernel<false>, dim3(cc_chunk_grid(N)), dim3(kCcBlock), 0, (hipStream_t)stream, mask, label, key, N, block_incl,
                           block_count, nodes, mapper);
    } else {
        if (!nodes || !mapper) return SS_ERR_INVALID_ARG;
        hipLaunchKernelGGL(cc_select_kernel<true>, dim3(cc_chunk_grid(N)), dim3(kCcBlock), 0, (hipStream_t)stream, mask, label, key, N, block_incl,
                           block_count, nodes, mapper);
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_induced_mapper(const int64_t *nodes, int64_t n, int64_t N, int64_t *mapper, int32_t *err_flag, int32_t *dup_flag, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= kCcLimit || n < 0 || n >= kCcLimit) return SS_ERR_INVALID_ARG;
    if (N == 0) return SS_OK;
    if (!mapper || (n > 0 && !nodes)) return SS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(mapper, 0xFF, sizeof(int64_t) * (size_t)N, s) != hipSuccess) return SS_ERR_LAUNCH;  // every word -1
    if (n == 0) return SS_OK;
    hipLaunchKernelGGL(cc_scatter_kernel, dim3((unsigned)((n + kCcBlock - 1) / kCcBlock)), dim3(kCcBlock), 0, s, nodes, n, N, mapper, err_flag, dup_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_induced_edges(const int64_t *src, const int64_t *dst, int64_t E, int64_t N, const int64_t *mapper, const int64_t *block_incl,
                                int32_t *block_count, int64_t *out_src, int64_t *out_dst, int64_t *edge_ids, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= kCcLimit || E < 0 || E >= kCcLimit) return SS_ERR_INVALID_ARG;
    if (E == 0) return SS_OK;
    if (!src || !dst || !mapper) return SS_ERR_INVALID_ARG;
    if (!block_incl) {  // count pass
        if (!block_count) return SS_ERR_INVALID_ARG;
        hipLaunchKernelGGL(cc_edges_kernel<false>, dim3(cc_chunk_grid(E)), dim3(kCcBlock), 0, (hipStream_t)stream, src, dst, E, N, mapper, block_incl,
                           block_count, out_src, out_dst, edge_ids, err_flag);
    } else {
        if (!out_src || !out_dst || !edge_ids) return SS_ERR_INVALID_ARG;
        hipLaunchKernelGGL(cc_edges_kernel<true>, dim3(cc_chunk_grid(E)), dim3(kCcBlock), 0, (hipStream_t)stream, src, dst, E, N, mapper, block_incl,
                           block_count, out_src, out_dst, edge_ids, err_flag);
    }
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_components_same(const int32_t *label, int64_t N, const int64_t *links, int64_t L, uint8_t *out, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= kCcLimit || L < 0) return SS_ERR_INVALID_ARG;
    if (L == 0) return SS_OK;
    if (!label || !links || !out) return SS_ERR_INVALID_ARG;
    const int64_t blocks = (L + kCcBlock - 1) / kCcBlock;
    if (blocks >= kCcLimit) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cc_same_kernel, dim3((unsigned)blocks), dim3(kCcBlock), 0, (hipStream_t)stream, label, N, links, L, out, err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
