// ss_pool.hip -- the graph readouts of the SEAL models over a disjoint-union batch of subgraphs (reference models/seal.py:
// global_sort_pool :245 in SEALDGCNN, global_add_pool / global_mean_pool :42-45, :101-106, :161, centre pooling :88-95, :149-156)
// [PyG semantics restated: the package is not in this image; tests/pooling_restatement.py restates them in numpy].
// Graph q owns the rows rowptr[q] .. rowptr[q + 1] of x [T, F].  Every output element has ONE right value:
//   select   per graph the first k rows in the order "last channel descending, NaN first, -0 == +0, ties by ascending position".
//            The order is an integer order: key(v) (below) in the high word, the position in the low word of a 64-bit word, ascending.
//            All words of a graph are distinct, so neither the tier nor the sorting network can show in the result.
//   gather / scatter   move the selected rows (forward / backward of sort pool): a node is selected at most once -- no atomics.
//   segment pool       one lane owns one output element and adds the graph's rows in ascending order (ss_spmm.hip's loop shape).
// Rows are moved and added as the pieces of ss_feature_rows.hpp (a float4 per lane, or a single float), in its launch shape.
//   centre pool        the product of the two root rows of each link, roots read on the device.
// Offsets are 64-bit everywhere; ids that point outside their graph are not followed and set *err_flag.
#include "ss_feature_rows.hpp"

namespace ss {

constexpr int kPoolCap = 1024;  // C: words the on-chip sort holds (ss_pool_sort_capacity(); pooling.SORT_CAPACITY)
constexpr int kPoolThreads = 256;
constexpr unsigned long long kPoolPad = ~0ull;  // sorts behind every real word (the largest real key is key(-inf) = 0xFF800000)

// ascending key = descending float: NaN (any sign, any payload) -> 0, +inf -> 0x007FFFFF, ..., +-0 -> 0x7FFFFFFF, ..., -inf -> 0xFF800000
__device__ __forceinline__ uint32_t pool_key(float v)
{
    uint32_t b = __float_as_uint(v);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
    if ((b & 0x7FFFFFFFu) == 0u) b = 0u;
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // the monotone image of the float
    return ~m;
}

struct PoolSelectLds {
    unsigned long long keys[kPoolCap];
    int hist[256];
    int wave_a[kPoolThreads / kWave], wave_b[kPoolThreads / kWave];
    uint32_t prefix;
    int remaining;
};

// ascending bitonic sort of keys[0 .. P), P a power of two <= kPoolCap (whole workgroup; starts and ends with a barrier)
__device__ __forceinline__ void pool_sort(unsigned long long *keys, int P)
{
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < (P >> 1); i += kPoolThreads) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == up) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
        }
    __syncthreads();
}

// One workgroup per graph.  n <= kPoolCap: every (key, position) word goes to LDS and is sorted there.  n > kPoolCap (then n > k): the
// k-th smallest key by a radix select over the key column re-read from global memory (four 8-bit passes over the key; the position
// needs no pass -- among equal keys the lowest positions win), an ordered compaction of the k survivors, and the same sort.
// The key column is x[.., F - 1], read with stride F; nothing else of x is read.
__global__ __launch_bounds__(kPoolThreads) void pool_select_kernel(const int64_t *__restrict__ rowptr, int64_t L, const float *__restrict__ x,
                                                                   int64_t T, int F, int k, int32_t *__restrict__ perm,
                                                                   int32_t *__restrict__ err_flag)
{
    __shared__ PoolSelectLds s;
    const int t = threadIdx.x, wave = t / kWave, wl = t & (kWave - 1);
    for (int64_t q = blockIdx.x; q < L; q += gridDim.x) {
        const int64_t r0 = rowptr[q], r1 = rowptr[q + 1];
        const bool ok = r0 >= 0 && r1 >= r0 && r1 <= T && r1 - r0 < ((int64_t)1 << 31);
        if (!ok && t == 0 && err_flag) *err_flag = 1;
        const int n = ok ? (int)(r1 - r0) : 0;
        const float *__restrict__ kc = x + r0 * F + (F - 1);
        int cnt, P;
        if (n <= kPoolCap) {
            cnt = n;
            P = pow2_ceil(n);
            for (int i = t; i < P; i += kPoolThreads)
                s.keys[i] = i < n ? ((unsigned long long)pool_key(kc[(int64_t)i * F]) << 32) | (uint32_t)i : kPoolPad;
        } else {
            uint32_t prefix = 0;
            int remaining = k;
            for (int shift = 24; shift >= 0; shift -= 8) {
                s.hist[t] = 0;
                __syncthreads();
                for (int64_t i = t; i < n; i += kPoolThreads) {
                    const uint64_t key = pool_key(kc[i * F]);
                    if ((key >> (shift + 8)) == ((uint64_t)prefix >> (shift + 8))) atomicAdd(&s.hist[(int)(key >> shift) & 0xFF], 1);
                }
                __syncthreads();
                const int mine = s.hist[t];
                int inc = mine;  // inclusive prefix sum over the bins: within the wave, then across the waves
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) {
                    const int y = __shfl_up(inc, d);
                    if (wl >= d) inc += y;
                }
                if (wl == kWave - 1) s.wave_a[wave] = inc;
                __syncthreads();
                for (int w = 0; w < wave; ++w) inc += s.wave_a[w];
                if (inc - mine < remaining && remaining <= inc) {  // exactly one bin: the counts sum to n > k >= remaining
                    s.prefix = prefix | ((uint32_t)t << shift);
                    s.remaining = remaining - (inc - mine);
                }
                __syncthreads();
                prefix = s.prefix;
                remaining = s.remaining;
            }
            // survivors in position order: every key below the threshold, and the `remaining` first of the keys equal to it
            int run_lt = 0, run_eq = 0;
            for (int64_t base = 0; base < n; base += kPoolThreads) {
                const int64_t i = base + t;
                const uint32_t key = i < n ? pool_key(kc[i * F]) : 0xFFFFFFFFu;
                const bool lt = i < n && key < prefix, eq = i < n && key == prefix;
                const unsigned long long bl = __ballot(lt), be = __ballot(eq);
                if (wl == 0) {
                    s.wave_a[wave] = __popcll(bl);
                    s.wave_b[wave] = __popcll(be);
                }
                __syncthreads();
                int lt_before = run_lt, eq_before = run_eq;
                for (int w = 0; w < kPoolThreads / kWave; ++w) {
                    if (w < wave) {
                        lt_before += s.wave_a[w];
                        eq_before += s.wave_b[w];
                    }
                    run_lt += s.wave_a[w];
                    run_eq += s.wave_b[w];
                }
                const unsigned long long below = ((unsigned long long)1 << wl) - 1;
                lt_before += __popcll(bl & below);
                eq_before += __popcll(be & below);
                // (a survivor's slot is below k: k - remaining keys lie below the threshold; checked all the same, for an x that
                //  another stream rewrites between the passes)
                const int slot = lt_before + (eq_before < remaining ? eq_before : remaining);
                if ((lt || (eq && eq_before < remaining)) && slot < k) s.keys[slot] =((unsigned long long)key << 32) | (uint32_t)i;
                __syncthreads();
                if (run_lt + (run_eq < remaining ? run_eq : remaining) >= k) break;  // (uniform) all k survivors are in
            }
            cnt = k;
            P = pow2_ceil(k);
            for (int i = k + t; i < P; i += kPoolThreads) s.keys[i] = kPoolPad;
        }
        pool_sort(s.keys, P);
        const int kept = cnt < k ? cnt : k;
        int32_t *__restrict__ pq = perm + q * k;
        for (int j = t; j < k; j += kPoolThreads) pq[j] = j < kept ? (int32_t)(uint32_t)s.keys[j] : -1;
        __syncthreads();  // (the words are read before the next graph writes them)
    }
}

// which item (a row of `lanes` lanes) this lane works on, and its lane inside the item
__device__ __forceinline__ int64_t pool_item(int lanes, int &cl)
{
    const int lane = threadIdx.x & (kWave - 1);
    cl = lane % lanes;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    return wave * (kWave / lanes) + lane / lanes;
}

__device__ __forceinline__ bool pool_row_ok(int64_t r0, int64_t r1, int64_t T) { return r0 >= 0 && r1 >= r0 && r1 <= T; }

// out[q, j] = x[rowptr[q] + perm[q, j]], zeros for perm == -1; any other id outside [0, n) is not followed: nothing written, *err_flag set
template <class V>
__global__ __launch_bounds__(256) void pool_gather_kernel(const int64_t *__restrict__ rowptr, int64_t L, const int32_t *__restrict__ perm, int k,
                                                          const float *__restrict__ x, int64_t T, int F, float *__restrict__ out,
                                                          int32_t *__restrict__ err_flag, int lanes)
{
    int cl;
    const int64_t item = pool_item(lanes, cl);
    if (item >= L * k) return;
    const int64_t q = item / k, r0 = rowptr[q], r1 = rowptr[q + 1];
    const int32_t p = perm[item];
    const bool zero = p == -1;
    if (!zero && !(pool_row_ok(r0, r1, T) && p >= 0 && p < r1 - r0)) {
        if (cl == 0 && err_flag) *err_flag = 1;
        return;
    }
    const float *__restrict__ src = x + (zero ? 0 : r0 + p) * F;
    float *__restrict__ dst = out + item * F;
    const int W = piece_width<V>(F);
    for (int c = cl; c < W; c += lanes) piece_store<V>(dst, c, zero ? piece_zero<V>() : piece_load<V>(src, c));
}

// grad_x[rowptr[q] + perm[q, j]] = g[q, j] for perm >= 0 (the entry has cleared grad_x before)
template <class V>
__global__ __launch_bounds__(256) void pool_scatter_kernel(const int64_t *__restrict__ rowptr, int64_t L, const int32_t *__restrict__ perm, int k,
                                                           const float *__restrict__ g, int64_t T, int F, float *__restrict__ grad_x,
                                                           int32_t *__restrict__ err_flag, int lanes)
{
    int cl;
    const int64_t item = pool_item(lanes, cl);
    if (item >= L * k) return;
    const int64_t q = item / k, r0 = rowptr[q], r1 = rowptr[q + 1];
    const int32_t p = perm[item];
    if (p == -1) return;
    if (!(pool_row_ok(r0, r1, T) && p >= 0 && p < r1 - r0)) {
        if (cl == 0 && err_flag) *err_flag = 1;
        return;
    }
    const float *__restrict__ src = g + item * F;
    float *__restrict__ dst = grad_x + (r0 + p) * F;
    const int W = piece_width<V>(F);
    for (int c = cl; c < W; c += lanes) piece_store<V>(dst, c, piece_load<V>(src, c));
}

// out[q] = the rows of graph q added in ascending order from +0.0 by one lane per element (four rows requested before the first is
// used; the adds stay in row order), then for `mean` ONE division by float(max(n, 1))
template <class V>
__global__ __launch_bounds__(256) void pool_segment_kernel(const int64_t *__restrict__ rowptr, int64_t L, const float *__restrict__ x, int64_t T,
                                                           int F, int mean, float *__restrict__ out, int32_t *__restrict__ err_flag, int lanes)
{
    int cl;
    const int64_t q = pool_item(lanes, cl);
    if (q >= L) return;
    const int64_t r0 = rowptr[q], r1 = rowptr[q + 1];
    if (!pool_row_ok(r0, r1, T)) {
        if (cl == 0 && err_flag) *err_flag = 1;
        return;
    }
    const int64_t n = r1 - r0;
    const float d = (float)(n > 1 ? n : 1);
    const int W = piece_width<V>(F);
    for (int c = cl; c < W; c += lanes) {
        V acc = piece_zero<V>();
        int64_t t = r0;
        for (; t + 3 < r1; t += 4) {
            V r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = piece_load<V>(x + (t + j) * F, c);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = piece_add(acc, r[j]);
        }
        for (; t < r1; ++t) acc = piece_add(acc, piece_load<V>(x + t * F, c));
        piece_store<V>(out + q * F, c, mean ? piece_div(acc, d) : acc);
    }
}

// grad_x[t] = g[q(t)] (mean: / float(max(n, 1))): one item per row t of x, its graph found by bisection of rowptr; a row that lies in no
// graph (before rowptr[0], from rowptr[L] on) gets zeros.  Every row of grad_x is written exactly once.
template <class V>
__global__ __launch_bounds__(256) void pool_segment_grad_kernel(const int64_t *__restrict__ rowptr, int64_t L, const float *__restrict__ g,
                                                                int64_t T, int F, int mean, float *__restrict__ grad_x, int lanes)
{
    int cl;
    const int64_t t = pool_item(lanes, cl);
    if (t >= T) return;
    int64_t lo = 0, hi = L + 1;  // the first entry of rowptr[0 .. L] above t
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] <= t) lo = mid + 1; else hi = mid;
    }
    const bool inside = lo >= 1 && lo <= L;
    const int64_t q = inside ? lo - 1 : 0;
    const int64_t n = rowptr[q + 1] - rowptr[q];
    const float d = (float)(n > 1 ? n : 1);
    const int W = piece_width<V>(F);
    for (int c = cl; c < W; c += lanes) {
        V v = piece_zero<V>();
        if (inside) {
            v = piece_load<V>(g + q * F, c);
            if (mean) v = piece_div(v, d);
        }
        piece_store<V>(grad_x + t * F, c, v);
    }
}

// roots of link q: both -1 (a row emptied by max_nodes) -> 1; both inside [0, n) -> 0; anything else -> -1
__device__ __forceinline__ int pool_roots(const int64_t *rowptr, const int32_t *roots, int64_t q, int64_t T, int64_t &ra, int64_t &rb)
{
    const int32_t a = roots[2 * q], b = roots[2 * q + 1];
    if (a == -1 && b == -1) return 1;
    const int64_t r0 = rowptr[q], r1 = rowptr[q + 1];
    if (!(pool_row_ok(r0, r1, T) && a >= 0 && b >= 0 && a < r1 - r0 && b < r1 - r0)) return -1;
    ra = r0 + a;
    rb = r0 + b;
    return 0;
}

template <class V>
__global__ __launch_bounds__(256) void pool_center_kernel(const int64_t *__restrict__ rowptr, int64_t L, const int32_t *__restrict__ roots,
                                                          const float *__restrict__ x, int64_t T, int F, float *__restrict__ out,
                                                          int32_t *__restrict__ err_flag, int lanes)
{
    int cl;
    const int64_t q = pool_item(lanes, cl);
    if (q >= L) return;
    int64_t ra = 0, rb = 0;
    const int kind = pool_roots(rowptr, roots, q, T, ra, rb);
    if (kind < 0) {
        if (cl == 0 && err_flag) *err_flag = 1;
        return;
    }
    const int W = piece_width<V>(F);
    for (int c = cl; c < W; c += lanes)
        piece_store<V>(out + q * F, c, kind ? piece_zero<V>() : piece_mul(piece_load<V>(x + ra * F, c), piece_load<V>(x + rb * F, c)));
}

// grad_x[a] = g * x[b], grad_x[b] = g * x[a]; a == b: the sum of the two (the entry has cleared grad_x before)
template <class V>
__global__ __launch_bounds__(256) void pool_center_grad_kernel(const int64_t *__restrict__ rowptr, int64_t L, const int32_t *__restrict__ roots,
                                                               const float *__restrict__ x, const float *__restrict__ g, int64_t T, int F,
                                                               float *__restrict__ grad_x, int32_t *__restrict__ err_flag, int lanes)
{
    int cl;
    const int64_t q = pool_item(lanes, cl);
    if (q >= L) return;
    int64_t ra = 0, rb = 0;
    const int kind = pool_roots(rowptr, roots, q, T, ra, rb);
    if (kind < 0 && cl == 0 && err_flag) *err_flag = 1;
    if (kind != 0) return;
    const int W = piece_width<V>(F);
    for (int c = cl; c < W; c += lanes) {
        const V gg = piece_load<V>(g + q * F, c);
        const V ga = piece_mul(gg, piece_load<V>(x + rb * F, c)), gb = piece_mul(gg, piece_load<V>(x + ra * F, c));
        if (ra == rb) {
            piece_store<V>(grad_x + ra * F, c, piece_add(ga, gb));
        } else {
            piece_store<V>(grad_x + ra * F, c, ga);
            piece_store<V>(grad_x + rb * F, c, gb);
        }
    }
}

inline bool pool_sizes_ok(int64_t L, int64_t T, int F) { return L >= 0 && T >= 0 && F >= 0 && L < ((int64_t)1 << 31); }

}  // namespace ss

extern "C" int ss_pool_sort_capacity(void) { return ss::kPoolCap; }

extern "C" int ss_pool_select(const int64_t *rowptr, int64_t L, const float *x, int64_t T, int32_t F, int32_t k, int32_t *perm,
                              int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (!pool_sizes_ok(L, T, F) || F < 1 || k < 1 || k > kPoolCap) return SS_ERR_INVALID_ARG;
    if (!rowptr || !perm || (T > 0 && !x)) return SS_ERR_INVALID_ARG;
    if (L == 0) return SS_OK;
    hipLaunchKernelGGL(pool_select_kernel, dim3((unsigned)L), dim3(kPoolThreads), 0, (hipStream_t)stream, rowptr, L, x, T, (int)F, (int)k, perm,
                       err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_pool_gather(const int64_t *rowptr, int64_t L, const int32_t *perm, int32_t k, const float *x, int64_t T, int32_t F,
                              float *out, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (!pool_sizes_ok(L, T, F) || k < 1) return SS_ERR_INVALID_ARG;
    if (!rowptr || !perm || (F > 0 && (!out || (T > 0 && !x)))) return SS_ERR_INVALID_ARG;
    if (L == 0 || F == 0) return SS_OK;
    const RowShape sh = row_shape(L * k, F, (uintptr_t)x | (uintptr_t)out);
    SS_ROWS_LAUNCH(sh, pool_gather_kernel<float4>, pool_gather_kernel<float>, rowptr, L, perm, (int)k, x, T, (int)F, out, err_flag, sh.lanes);
    return SS_OK;
}

extern "C" int ss_pool_scatter(const int64_t *rowptr, int64_t L, const int32_t *perm, int32_t k, const float *g, int64_t T, int32_t F,
                               float *grad_x, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (!pool_sizes_ok(L, T, F) || k < 1) return SS_ERR_INVALID_ARG;
    if (!rowptr || !perm || (F > 0 && ((T > 0 && !grad_x) || (L > 0 && !g)))) return SS_ERR_INVALID_ARG;
    if (T > 0 && F > 0 && hipMemsetAsync(grad_x, 0, (size_t)T * F * sizeof(float), (hipStream_t)stream) != hipSuccess) return SS_ERR_LAUNCH;
    if (L == 0 || F == 0 || T == 0) return SS_OK;
    const RowShape sh = row_shape(L * k, F, (uintptr_t)g | (uintptr_t)grad_x);
    SS_ROWS_LAUNCH(sh, pool_scatter_kernel<float4>, pool_scatter_kernel<float>, rowptr, L, perm, (int)k, g, T, (int)F, grad_x, err_flag, sh.lanes);
    return SS_OK;
}

extern "C" int ss_segment_pool(const int64_t *rowptr, int64_t L, const float *x, int64_t T, int32_t F, int32_t mean, float *out,
                               int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (!pool_sizes_ok(L, T, F)) return SS_ERR_INVALID_ARG;
    if (!rowptr || (F > 0 && ((L > 0 && !out) || (T > 0 && !x)))) return SS_ERR_INVALID_ARG;
    if (L == 0 || F == 0) return SS_OK;
    const RowShape sh = row_shape(L, F, (uintptr_t)x | (uintptr_t)out);
    SS_ROWS_LAUNCH(sh, pool_segment_kernel<float4>, pool_segment_kernel<float>, rowptr, L, x, T, (int)F, (int)(mean != 0), out, err_flag, sh.lanes);
    return SS_OK;
}

extern "C" int ss_segment_pool_grad(const int64_t *rowptr, int64_t L, const float *g, int64_t T, int32_t F, int32_t mean, float *grad_x,
                                    void *stream)
{
    using namespace ss;
    if (!pool_sizes_ok(L, T, F)) return SS_ERR_INVALID_ARG;
    if (!rowptr || (F > 0 && ((T > 0 && !grad_x) || (L > 0 && !g)))) return SS_ERR_INVALID_ARG;
    if (T == 0 || F == 0) return SS_OK;
    if (L == 0) return hipMemsetAsync(grad_x, 0, (size_t)T * F * sizeof(float), (hipStream_t)stream) == hipSuccess ? SS_OK : SS_ERR_LAUNCH;
    const RowShape sh = row_shape(T, F, (uintptr_t)g | (uintptr_t)grad_x);
    SS_ROWS_LAUNCH(sh, pool_segment_grad_kernel<float4>, pool_segment_grad_kernel<float>, rowptr, L, g, T, (int)F, (int)(mean != 0), grad_x, sh.lanes);
    return SS_OK;
}

extern "C" int ss_center_pool(const int64_t *rowptr, int64_t L, const int32_t *roots, const float *x, int64_t T, int32_t F, float *out,
                              int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (!pool_sizes_ok(L, T, F)) return SS_ERR_INVALID_ARG;
    if (!rowptr || (L > 0 && !roots) || (F > 0 && ((L > 0 && !out) || (T > 0 && !x)))) return SS_ERR_INVALID_ARG;
    if (L == 0 || F == 0) return SS_OK;
    const RowShape sh = row_shape(L, F, (uintptr_t)x | (uintptr_t)out);
    SS_ROWS_LAUNCH(sh, pool_center_kernel<float4>, pool_center_kernel<float>, rowptr, L, roots, x, T, (int)F, out, err_flag, sh.lanes);
    return SS_OK;
}

extern "C" int ss_center_pool_grad(const int64_t *rowptr, int64_t L, const int32_t *roots, const float *x, const float *g, int64_t T,
                                   int32_t F, float *grad_x, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (!pool_sizes_ok(L, T, F)) return SS_ERR_INVALID_ARG;
    if (!rowptr || (L > 0 && !roots) || (F > 0 && ((T > 0 && (!grad_x || !x)) || (L > 0 && !g)))) return SS_ERR_INVALID_ARG;
    if (T > 0 && F > 0 && hipMemsetAsync(grad_x, 0, (size_t)T * F * sizeof(float), (hipStream_t)stream) != hipSuccess) return SS_ERR_LAUNCH;
    if (L == 0 || F == 0 || T == 0) return SS_OK;
    const RowShape sh = row_shape(L, F, (uintptr_t)x | (uintptr_t)g | (uintptr_t)grad_x);
    SS_ROWS_LAUNCH(sh, pool_center_grad_kernel<float4>, pool_center_grad_kernel<float>, rowptr, L, roots, x, g, T, (int)F, grad_x, err_flag, sh.lanes);
    return SS_OK;
}
