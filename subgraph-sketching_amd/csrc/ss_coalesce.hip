// ss_coalesce.hip -- the merge of equal (row, col) entries of an edge list: what coalesce / to_undirected / coalesce_graph return
// (graph_prep.py).  Replaces, at the head of every dataset constructor of the reference, torch_sparse.coalesce
// (src/datasets/elph.py:54-66, src/datasets/seal.py:58-60, 111-113) and PyG's to_undirected(..., reduce='add') (src/datasets/elph.py:54-66
// for directed data, src/data.py:137, 174) [both restated: neither package is in this image].
//
// The caller brings the positions of the list sorted by (row, col, position) -- perm, two stable groupings by ss_csr_group_ids +
// ss_csr_sort_rows, least significant key first; row and col are never multiplied together -- and this unit does the rest:
//   mark     position i of the sorted order is a HEAD when i == 0 or its (row, col) differs from position i - 1's; one head count per
//            workgroup of SS_COALESCE_BLOCK positions (the caller's cumulative sum turns the counts into offsets)
//   fill     every head finds its output slot (workgroup offset + ballot rank), writes the pair and where its run starts, and fills the
//            output rowptr over the rows between the previous head's row and its own
//   reduce   one lane per output slot walks its run in list order and applies the op under the chunk rule; runs of more than
//            long_entries entries are listed for
//   long     one wavefront per listed run, lanes summing whole chunks, the chunk results combined in chunk order
//   symmetric one lane per output pair (u, v) looks for (v, u) by binary search of row v
//
// Accumulation order (the contract): a run is cut into chunks of SS_COALESCE_CHUNK entries from its start; a chunk is folded
// sequentially in list order starting from its first entry, the chunk results are folded in chunk order.  Both tiers do exactly that,
// so a value's bits depend on its own run alone.  There is no float atomic in this unit; the only atomics append a run's slot to the
// long list (whose order nothing depends on) and take the maximum run length.
#include "ss_common.hpp"

#define SS_COALESCE_CHUNK 256   // entries per chunk of the accumulation order; ss_coalesce_chunk() tells it to callers
#define SS_COALESCE_BLOCK 2048  // sorted positions per workgroup of the mark / fill passes; ss_coalesce_block()
// the dtype and op codes of the boundary (include/subgraph_sketch.h)
#define SS_COALESCE_INT64 0
#define SS_COALESCE_FLOAT32 1
#define SS_COALESCE_FLOAT64 2
#define SS_COALESCE_ADD 0
#define SS_COALESCE_MEAN 1
#define SS_COALESCE_MIN 2
#define SS_COALESCE_MAX 3

namespace ss {

constexpr int kCoBlock = 256;
constexpr int kCoTiles = SS_COALESCE_BLOCK / kCoBlock;
constexpr int kCoChunk = SS_COALESCE_CHUNK;
constexpr int kCoBatch = 8;       // independent gathers in flight inside a chunk's sequential fold
constexpr int kCoGapLane = 32;    // a rowptr gap of more rows than this is filled by the whole wavefront
constexpr int64_t kCoLimit = (int64_t)1 << 31;  // node ids and positions are 32-bit quantities inside the unit
static_assert(SS_COALESCE_BLOCK % kCoBlock == 0, "a workgroup's positions are a whole number of tiles");

__device__ __forceinline__ int co_lane() { return threadIdx.x & (kWave - 1); }

// position i of the sorted order: its pair (r, c), the row of position i - 1 (pr; -1 at i == 0) and whether it starts a run.  Every
// lane of the wavefront calls (dead lanes: i >= E): the predecessor comes from the lane below, lane 0 gathers its own -- for the first
// wavefront of a workgroup that is the last position of the previous workgroup's range.
__device__ __forceinline__ bool co_head(const int64_t *__restrict__ row, const int64_t *__restrict__ col, const int32_t *__restrict__ perm, int64_t i,
                                        int64_t E, int64_t &r, int64_t &c, int64_t &pr)
{
    const bool live = i < E;
    r = c = -1;
    if (live) {
        const int32_t p = perm[i];
        r = row[p];
        c = col[p];
    }
    pr = __shfl_up(r, 1);
    int64_t pc = __shfl_up(c, 1);
    if (co_lane() == 0 && live && i > 0) {
        const int32_t q = perm[i - 1];
        pr = row[q];
        pc = col[q];
    }
    if (i == 0) pr = -1;
    return live && (i == 0 || r != pr || c != pc);
}

__global__ __launch_bounds__(kCoBlock) void co_mark_kernel(const int64_t *__restrict__ row, const int64_t *__restrict__ col,
                                                           const int32_t *__restrict__ perm, int64_t E, int64_t N, int32_t *__restrict__ block_heads,
                                                           int32_t *err)
{
    __shared__ int32_t lds[kCoBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * SS_COALESCE_BLOCK;
    int heads = 0;
    for (int k = 0; k < kCoTiles; ++k) {
        const int64_t i = base + k * kCoBlock + threadIdx.x;
        int64_t r, c, pr;
        const bool head = co_head(row, col, perm, i, E, r, c, pr);
        if (i < E && (((uint64_t)r >= (uint64_t)N) | ((uint64_t)c >= (uint64_t)N)) && err) *err = 1;
        heads += __builtin_popcountll(__ballot(head));
    }
    if (co_lane() == 0) lds[threadIdx.x / kWave] = heads;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kCoBlock / kWave; ++w) total += lds[w];
        block_heads[blockIdx.x] = total;
    }
}

// rowptr[lo .. hi) = v for every lane that has such a span; the whole wavefront calls.  Short spans are written by their own lane, a
// long one (empty rows by the thousand) by all lanes together.
__device__ __forceinline__ void co_fill_span(int64_t *__restrict__ rowptr, int64_t lo, int64_t hi, int64_t v)
{
    const int64_t len = hi - lo;
    if (len <= kCoGapLane)
        for (int64_t x = lo; x < hi; ++x) rowptr[x] = v;
    unsigned long long big = __ballot(len > kCoGapLane);
    while (big) {
        const int l = __builtin_ctzll(big);
        big &= big - 1;
        const int64_t lo_l = __shfl(lo, l), hi_l = __shfl(hi, l), v_l = __shfl(v, l);
        for (int64_t x = lo_l + co_lane(); x < hi_l; x += kWave) rowptr[x] = v_l;
    }
}

// a row number as an index of rowptr whatever the input holds (ids out of range are reported by the mark pass; here they must only
// not carry a store outside rowptr[0 .. N])
__device__ __forceinline__ int64_t co_clamp_row(int64_t r, int64_t N) { return r < -1 ? -1 : (r > N - 1 ? N - 1 : r); }

__global__ __launch_bounds__(kCoBlock) void co_fill_kernel(const int64_t *__restrict__ row, const int64_t *__restrict__ col,
                                                           const int32_t *__restrict__ perm, int64_t E, int64_t N,
                                                           const int64_t *__restrict__ block_incl, int64_t n_runs, int64_t *__restrict__ out_row,
                                                           int64_t *__restrict__ out_col, int32_t *__restrict__ run_start, int64_t *__restrict__ rowptr)
{
    __shared__ int32_t lds[kCoBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * SS_COALESCE_BLOCK;
    const int w = threadIdx.x / kWave;
    int64_t run = blockIdx.x ? block_incl[blockIdx.x - 1] : 0;
    for (int k = 0; k < kCoTiles; ++k) {
        const int64_t i = base + k * kCoBlock + threadIdx.x;
        int64_t r, c, pr;
        const bool head = co_head(row, col, perm, i, E, r, c, pr);
        const unsigned long long m = __ballot(head);
        const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        __syncthreads();  // (the readers of the previous tile are done)
        if (co_lane() == 0) lds[w] = __builtin_popcountll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int q = 0; q < kCoBlock / kWave; ++q) {
            const int n = lds[q];
            before += q < w ? n : 0;
            total += n;
        }
        const int64_t slot = run + before + below;
        // the rows after the previous head's row up to and including this head's start at this slot (the first head: rows 0 .. r)
        int64_t lo = 0, hi = 0;
        if (head) {
            out_row[slot] = r;
            out_col[slot] = c;
            run_start[slot] = (int32_t)i;
            lo = co_clamp_row(pr, N) + 1;
            hi = co_clamp_row(r, N) + 1;
        }
        co_fill_span(rowptr, lo, hi, slot);
        // the last position closes the list: the rows after its row, and rowptr[N], start at n_runs
        lo = hi = 0;
        if (i == E - 1) {
            run_start[n_runs] = (int32_t)E;
            lo = co_clamp_row(r, N) + 1;
            hi = N + 1;
        }
        co_fill_span(rowptr, lo, hi, n_runs);
        run += total;
    }
}

// ---- the fold of a run ----------------------------------------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ bool co_isnan(T x) { return x != x; }
template <>
__device__ __forceinline__ bool co_isnan<int64_t>(int64_t) { return false; }

template <typename T>
__device__ __forceinline__ T co_nan();
template <>
__device__ __forceinline__ float co_nan<float>() { return __uint_as_float(0x7FC00000u); }
template <>
__device__ __forceinline__ double co_nan<double>() { return __longlong_as_double(0x7FF8000000000000LL); }
template <>
__device__ __forceinline__ int64_t co_nan<int64_t>() { return 0; }

template <typename T>
__device__ __forceinline__ T co_plus(T a, T b) { return a + b; }
template <>
__device__ __forceinline__ int64_t co_plus<int64_t>(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }  // wraps, as torch does

template <typename T>
__device__ __forceinline__ T co_mean(T s, int32_t n) { return s / (T)n; }
template <>
__device__ __forceinline__ int64_t co_mean<int64_t>(int64_t s, int32_t n)  // floor division (n > 0)
{
    const int64_t q = s / n;
    return (s % n != 0 && s < 0) ? q - 1 : q;
}

// the running result of a fold: init with the first entry, step with every further one in list order, merge with the fold of the
// entries that follow.  min / max: a strict comparison, so of equal values (-0.0 and +0.0) the one listed first stays; a NaN anywhere
// makes the result the canonical quiet NaN
template <typename T, int OP>
struct CoFold {
    T v;
    int nan;
    __device__ __forceinline__ void init(T x)
    {
        v = x;
        nan = OP >= SS_COALESCE_MIN && co_isnan(x);
    }
    __device__ __forceinline__ void step(T x)
    {
        if (OP <= SS_COALESCE_MEAN) {
            v = co_plus(v, x);
        } else {
            nan |= co_isnan(x);
            if (OP == SS_COALESCE_MIN ? x < v : x > v) v = x;
        }
    }
    __device__ __forceinline__ void merge(const CoFold &o)
    {
        step(o.v);
        if (OP >= SS_COALESCE_MIN) nan |= o.nan;
    }
    __device__ __forceinline__ T finish(int32_t n) const
    {
        if (OP == SS_COALESCE_ADD) return v;
        if (OP == SS_COALESCE_MEAN) return co_mean(v, n);
        return nan ? co_nan<T>() : v;
    }
};

// the value of the entry at position j of the sorted order: list position p of the (possibly doubled) list reads value[p mod n_values]
template <typename T>
__device__ __forceinline__ T co_entry(const int32_t *__restrict__ perm, const T *__restrict__ value, int64_t n_values, int64_t j)
{
    const int64_t p = perm[j];
    return value[p >= n_values ? p - n_values : p];
}

// one chunk, entries [b, e) of the sorted order, 1 <= e - b <= kCoChunk, folded sequentially; the gathers go kCoBatch at a time
template <typename T, int OP>
__device__ __forceinline__ CoFold<T, OP> co_fold_chunk(const int32_t *__restrict__ perm, const T *__restrict__ value, int64_t n_values, int64_t b,
                                                        int64_t e)
{
    CoFold<T, OP> f;
    f.init(co_entry(perm, value, n_values, b));
    int64_t j = b + 1;
    for (; j + kCoBatch <= e; j += kCoBatch) {
        T x[kCoBatch];
#pragma unroll
        for (int t = 0; t < kCoBatch; ++t) x[t] = co_entry(perm, value, n_values, j + t);
#pragma unroll
        for (int t = 0; t < kCoBatch; ++t) f.step(x[t]);
    }
    for (; j < e; ++j) f.step(co_entry(perm, value, n_values, j));
    return f;
}

// the maximum over the wavefront of a non-negative int, in every lane
__device__ __forceinline__ int32_t co_wave_max(int32_t v)
{
    for (int off = 1; off < kWave; off <<= 1) {
        const int32_t o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// info[0]: the number of listed (long) runs, info[1]: the longest run.  value == nullptr: only the counts
template <typename T, int OP>
__global__ __launch_bounds__(kCoBlock) void co_reduce_kernel(const int32_t *__restrict__ perm, const int32_t *__restrict__ run_start, int64_t n_runs,
                                                             const T *__restrict__ value, int64_t n_values, int32_t long_entries,
                                                             T *__restrict__ out_value, int32_t *__restrict__ out_count,
                                                             int32_t *__restrict__ long_runs, int64_t max_long, int32_t *info)
{
    const int64_t s = (int64_t)blockIdx.x * kCoBlock + threadIdx.x;
    const bool live = s < n_runs;
    const int64_t b = live ? run_start[s] : 0, e = live ? run_start[s + 1] : 0;
    const int32_t len = (int32_t)(e - b);
    if (live) out_count[s] = len;
    const int32_t longest = co_wave_max(len);
    if (co_lane() == 0 && longest > 0) atomicMax(info + 1, longest);
    if (!live || value == nullptr) return;
    if (len > long_entries) {  // the long tier's
        const int32_t at = atomicAdd(info, 1);
        if (at < max_long) long_runs[at] = (int32_t)s;  // (a run of more than long_entries entries: at most E / long_entries of them)
        return;
    }
    CoFold<T, OP> total = co_fold_chunk<T, OP>(perm, value, n_values, b, b + kCoChunk < e ? b + kCoChunk : e);
    for (int64_t c0 = b + kCoChunk; c0 < e; c0 += kCoChunk)
        total.merge(co_fold_chunk<T, OP>(perm, value, n_values, c0, c0 + kCoChunk < e ? c0 + kCoChunk : e));
    out_value[s] = total.finish(len);
}

// one wavefront per listed run: lane l folds chunks l, l + 64, ... of the run; after every round of 64 chunks their results join the
// total in chunk order (every lane computes the same total from the same broadcasts; lane 0 stores it)
template <typename T, int OP>
__global__ __launch_bounds__(kCoBlock) void co_reduce_long_kernel(const int32_t *__restrict__ perm, const int32_t *__restrict__ run_start,
                                                                  const T *__restrict__ value, int64_t n_values, T *__restrict__ out_value,
                                                                  const int32_t *__restrict__ long_runs, const int32_t *__restrict__ info,
                                                                  int64_t max_long)
{
    const int lane = co_lane();
    const int64_t waves = (int64_t)gridDim.x * (kCoBlock / kWave);
    int64_t n_long = info[0];
    n_long = n_long < max_long ? n_long : max_long;
    for (int64_t k = (int64_t)blockIdx.x * (kCoBlock / kWave) + threadIdx.x / kWave; k < n_long; k += waves) {
        const int64_t s = long_runs[k];
        const int64_t b = run_start[s], e = run_start[s + 1];
        CoFold<T, OP> total;
        bool first = true;
        for (int64_t r0 = b; r0 < e; r0 += (int64_t)kWave * kCoChunk) {  // a round: up to 64 chunks
            const int64_t c0 = r0 + (int64_t)lane * kCoChunk;
            CoFold<T, OP> mine;
            mine.init(T(0));
            if (c0 < e) mine = co_fold_chunk<T, OP>(perm, value, n_values, c0, c0 + kCoChunk < e ? c0 + kCoChunk : e);
            const int64_t left = e - r0;
            const int chunks = left >= (int64_t)kWave * kCoChunk ? kWave : (int)((left + kCoChunk - 1) / kCoChunk);
            for (int l = 0; l < chunks; ++l) {
                CoFold<T, OP> other;
                other.v = __shfl(mine.v, l);
                other.nan = __shfl(mine.nan, l);
                if (first) total = other;
                else total.merge(other);
                first = false;
            }
        }
        if (lane == 0) out_value[s] = total.finish((int32_t)(e - b));
    }
}

template <typename T>
__device__ __forceinline__ bool co_same(T a, T b) { return a == b || (a != a && b != b); }

// *asymmetric = 1 if some output pair (u, v) has no pair (v, u), or (value given) has one with another value.  Row v of the output is
// out_col[rowptr[v] .. rowptr[v + 1]), ascending and duplicate-free
template <typename T>
__global__ __launch_bounds__(kCoBlock) void co_symmetric_kernel(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ out_row,
                                                                const int64_t *__restrict__ out_col, int64_t n_runs, const T *__restrict__ value,
                                                                int32_t *asymmetric)
{
    const int64_t s = (int64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (s >= n_runs) return;
    const int64_t u = out_row[s], v = out_col[s];
    if (u == v) return;
    int64_t lo = rowptr[v], hi = rowptr[v + 1];
    while (lo < hi) {  // the first entry of row v that is not below u
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (out_col[mid] < u) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < rowptr[v + 1] && out_col[lo] == u;
    if (!found || (value != nullptr && !co_same(value[s], value[lo]))) *asymmetric = 1;
}

inline unsigned co_grid(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

template <typename T, int OP>
int co_launch_reduce(const int32_t *perm, const int32_t *run_start, int64_t n_runs, const void *value, int64_t n_values, int32_t long_entries,
                     void *out_value, int32_t *out_count, int32_t *long_runs, int64_t max_long, int32_t *info, hipStream_t s)
{
    hipLaunchKernelGGL((co_reduce_kernel<T, OP>), dim3(co_grid(n_runs, kCoBlock)), dim3(kCoBlock), 0, s, perm, run_start, n_runs,
                       static_cast<const T *>(value), n_values, long_entries, static_cast<T *>(out_value), out_count, long_runs, max_long, info);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

template <typename T, int OP>
int co_launch_long(const int32_t *perm, const int32_t *run_start, const void *value, int64_t n_values, void *out_value, const int32_t *long_runs,
                   const int32_t *info, int64_t max_long, hipStream_t s)
{
    const int64_t blocks = (max_long + kCoBlock / kWave - 1) / (kCoBlock / kWave);
    hipLaunchKernelGGL((co_reduce_long_kernel<T, OP>), dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kCoBlock), 0, s, perm, run_start,
                       static_cast<const T *>(value), n_values, static_cast<T *>(out_value), long_runs, info, max_long);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

// the instantiation of F for a (dtype, op) pair; SS_ERR_UNSUPPORTED for any other
#define SS_CO_DISPATCH_OP(T, F, ...)                                        \
    switch (op) {                                                           \
    case SS_COALESCE_ADD: return F<T, SS_COALESCE_ADD>(__VA_ARGS__);        \
    case SS_COALESCE_MEAN: return F<T, SS_COALESCE_MEAN>(__VA_ARGS__);      \
    case SS_COALESCE_MIN: return F<T, SS_COALESCE_MIN>(__VA_ARGS__);        \
    case SS_COALESCE_MAX: return F<T, SS_COALESCE_MAX>(__VA_ARGS__);        \
    default: return SS_ERR_UNSUPPORTED;                                     \
    }
#define SS_CO_DISPATCH(F, ...)                                              \
    switch (dtype) {                                                        \
    case SS_COALESCE_INT64: SS_CO_DISPATCH_OP(int64_t, F, __VA_ARGS__)      \
    case SS_COALESCE_FLOAT32: SS_CO_DISPATCH_OP(float, F, __VA_ARGS__)      \
    case SS_COALESCE_FLOAT64: SS_CO_DISPATCH_OP(double, F, __VA_ARGS__)     \
    default: return SS_ERR_UNSUPPORTED;                                     \
    }

inline bool co_known(int32_t dtype, int32_t op)
{
    return dtype >= SS_COALESCE_INT64 && dtype <= SS_COALESCE_FLOAT64 && op >= SS_COALESCE_ADD && op <= SS_COALESCE_MAX;
}

}  // namespace ss

extern "C" int ss_coalesce_chunk(void) { return SS_COALESCE_CHUNK; }
extern "C" int ss_coalesce_block(void) { return SS_COALESCE_BLOCK; }

extern "C" int ss_coalesce_mark(const int64_t *row, const int64_t *col, const int32_t *perm, int64_t E, int64_t N, int32_t *block_heads,
                                int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (N < 1 || N >= kCoLimit || E < 0 || E >= kCoLimit) return SS_ERR_INVALID_ARG;
    if (E == 0) return SS_OK;
    if (!row || !col || !perm || !block_heads) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(co_mark_kernel, dim3(co_grid(E, SS_COALESCE_BLOCK)), dim3(kCoBlock), 0, (hipStream_t)stream, row, col, perm, E, N, block_heads,
                       err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_coalesce_fill(const int64_t *row, const int64_t *col, const int32_t *perm, int64_t E, int64_t N, const int64_t *block_incl,
                                int64_t n_runs, int64_t *out_row, int64_t *out_col, int32_t *run_start, int64_t *rowptr, void *stream)
{
    using namespace ss;
    if (N < 1 || N >= kCoLimit || E < 0 || E >= kCoLimit || n_runs < 0 || n_runs > E) return SS_ERR_INVALID_ARG;
    if (E == 0) return SS_OK;
    if (!row || !col || !perm || !block_incl || !out_row || !out_col || !run_start || !rowptr || n_runs < 1) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(co_fill_kernel, dim3(co_grid(E, SS_COALESCE_BLOCK)), dim3(kCoBlock), 0, (hipStream_t)stream, row, col, perm, E, N, block_incl,
                       n_runs, out_row, out_col, run_start, rowptr);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_coalesce_reduce(const int32_t *perm, const int32_t *run_start, int64_t n_runs, const void *value, int64_t n_values, int32_t dtype,
                                  int32_t op, int32_t long_entries, void *out_value, int32_t *out_count, int32_t *long_runs, int64_t max_long,
                                  int32_t *info, void *stream)
{
    using namespace ss;
    if (n_runs < 0 || n_runs >= kCoLimit || n_values < 0 || long_entries < 1 || max_long < 0) return SS_ERR_INVALID_ARG;
    if (value != nullptr && !co_known(dtype, op)) return SS_ERR_UNSUPPORTED;
    if (n_runs == 0) return SS_OK;
    if (!perm || !run_start || !out_count || !info) return SS_ERR_INVALID_ARG;
    if (value != nullptr && (!out_value || !long_runs || n_values < 1)) return SS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return SS_ERR_LAUNCH;
    if (value == nullptr) return co_launch_reduce<int64_t, SS_COALESCE_ADD>(perm, run_start, n_runs, nullptr, 1, long_entries, nullptr, out_count,
                                                                             nullptr, 0, info, s);
    SS_CO_DISPATCH(co_launch_reduce, perm, run_start, n_runs, value, n_values, long_entries, out_value, out_count, long_runs, max_long, info, s)
}

extern "C" int ss_coalesce_reduce_long(const int32_t *perm, const int32_t *run_start, int64_t n_runs, const void *value, int64_t n_values,
                                       int32_t dtype, int32_t op, void *out_value, const int32_t *long_runs, const int32_t *info, int64_t max_long,
                                       void *stream)
{
    using namespace ss;
    if (n_runs < 0 || n_runs >= kCoLimit || n_values < 0 || max_long < 0) return SS_ERR_INVALID_ARG;
    if (!co_known(dtype, op)) return SS_ERR_UNSUPPORTED;
    if (n_runs == 0 || max_long == 0) return SS_OK;
    if (!perm || !run_start || !value || !out_value || !long_runs || !info || n_values < 1) return SS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    SS_CO_DISPATCH(co_launch_long, perm, run_start, value, n_values, out_value, long_runs, info, max_long, s)
}

extern "C" int ss_coalesce_symmetric(const int64_t *rowptr, const int64_t *out_row, const int64_t *out_col, int64_t n_runs, int64_t N,
                                     const void *value, int32_t dtype, int32_t *asymmetric, void *stream)
{
    using namespace ss;
    if (N < 1 || N >= kCoLimit || n_runs < 0 || n_runs >= kCoLimit || !asymmetric) return SS_ERR_INVALID_ARG;
    if (value != nullptr && (dtype < SS_COALESCE_INT64 || dtype > SS_COALESCE_FLOAT64)) return SS_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(asymmetric, 0, sizeof(int32_t), s) != hipSuccess) return SS_ERR_LAUNCH;
    if (n_runs == 0) return SS_OK;
    if (!rowptr || !out_row || !out_col) return SS_ERR_INVALID_ARG;
    const dim3 grid(co_grid(n_runs, kCoBlock)), block(kCoBlock);
    if (value == nullptr || dtype == SS_COALESCE_INT64)
        hipLaunchKernelGGL(co_symmetric_kernel<int64_t>, grid, block, 0, s, rowptr, out_row, out_col, n_runs, static_cast<const int64_t *>(value),
                           asymmetric);
    else if (dtype == SS_COALESCE_FLOAT32)
        hipLaunchKernelGGL(co_symmetric_kernel<float>, grid, block, 0, s, rowptr, out_row, out_col, n_runs, static_cast<const float *>(value),
                           asymmetric);
    else
        hipLaunchKernelGGL(co_symmetric_kernel<double>, grid, block, 0, s, rowptr, out_row, out_col, n_runs, static_cast<const double *>(value),
                           asymmetric);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
