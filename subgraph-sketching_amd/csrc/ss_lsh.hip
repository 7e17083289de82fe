// ss_lsh.hip -- locality-sensitive hashing by banding over one hop's MinHash table: the index behind ElphHashes.build_lsh_index /
// lsh_candidates / topk_links_lsh (lsh.py).
//
// Band j of node v is the slice M[v][j r : (j + 1) r] of its stored MinHash row (r = rows, b = bands, r b <= P); two nodes are
// candidates of each other when they agree on a whole band, value for value.  The one-vs-all scans (ss_topk.hip, ss_topk_head.hip,
// ss_rank.hip) score all N nodes per source and are bound by their VALU work per pair; here a source only meets the nodes of its b
// buckets.
//
//   lsh_band_keys_kernel   keys[j][v] = a 64-bit mix of band j of v, for every node and band: the table is read once in 16-byte
//                          chunks through an LDS tile of rows, the keys leave as 8-byte stores that are consecutive along v.
//                          torch.sort then orders every band (sorted keys + the permutation as int32): plumbing, not here.
//   lsh_walk_kernel<false> count: one 16-lane DPP row per (source, band): the equal range of the source's key in the band's sorted
//                          keys by binary search, dropped when longer than max_bucket, else every member's r values compared with the
//                          source's own (what makes the result exact under key collisions) and the survivors other than u counted.
//   lsh_walk_kernel<true>  fill: the same walk, writing s * N + v at the offsets an exclusive scan of the counts gives.
//
// The key is only what the bands are sorted by: membership is decided by the r values themselves.  key_bits < 64 keeps the low bits
// of the mix only (a test hook: buckets full of false matches).
#include "ss_common.hpp"

namespace ss {

constexpr int kLshTileWords = 8192;  // MinHash words of one LDS tile of rows (32 KiB)
constexpr int kLshTileRows = 64;     // rows per tile at most: a wavefront of consecutive keys per band

// the mix of one band: x[0 .. r) in LDS (the keys kernel) or global memory (a source's own row in the walk)
__device__ __forceinline__ uint64_t band_key(const uint32_t *x, int r)
{
    uint64_t k = (uint64_t)r;
    for (int i = 0; i < r; ++i) k = hash_u64(k ^ (uint64_t)x[i]) + 0x9E3779B97F4A7C15ULL;
    return k;
}

__host__ __device__ __forceinline__ uint64_t key_mask(int key_bits) { return key_bits >= 64 ? ~0ULL : ((1ULL << key_bits) - 1); }

// T rows per workgroup (T * P <= kLshTileWords); only the chunks that hold the r b words in use are read
__global__ __launch_bounds__(256) void lsh_band_keys_kernel(const uint32_t *__restrict__ mh, int64_t N, int P, int r, int b, uint64_t mask,
                                                             int T, int64_t *__restrict__ keys)
{
    __shared__ uint32_t tile[kLshTileWords + kLshTileRows];
    const int stride = P + 1;  // odd: the rows of a band's 64 readers start in different banks
    const int CW = (r * b + 3) >> 2;
    const int64_t v0 = (int64_t)blockIdx.x * T;
    const int nt = N - v0 < T ? (int)(N - v0) : T;
    for (int i = threadIdx.x; i < nt * CW; i += blockDim.x) {
        const int t = i / CW, c = i % CW;
        const u32x4 x = *reinterpret_cast<const u32x4 *>(mh + (v0 + t) * P + 4 * c);
        uint32_t *d = tile + t * stride + 4 * c;
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt * b; i += blockDim.x) {  // consecutive threads: consecutive nodes of one band
        const int j = i / nt, t = i % nt;
        keys[(int64_t)j * N + v0 + t] = (int64_t)(band_key(tile + t * stride + j * r, r) & mask);
    }
}

// one 16-lane row per item g = s * b + j.  FILL = false: counts[g] = candidates of sources[s] in band j; FILL = true: their entries
// s * N + v at out[offsets[g] ..), offsets = the exclusive scan of those counts
template <bool FILL>
__global__ __launch_bounds__(256) void lsh_walk_kernel(const int64_t *__restrict__ sources, int S, int64_t N, const uint32_t *__restrict__ mh,
                                                        int P, int r, int b, uint64_t mask, const int64_t *__restrict__ keys,
                                                        const int32_t *__restrict__ perm, int max_bucket, int32_t *__restrict__ counts,
                                                        const int64_t *__restrict__ offsets, int64_t *__restrict__ out,
                                                        int32_t *__restrict__ err)
{
    const int64_t g = (int64_t)blockIdx.x * (256 / kRow) + threadIdx.x / kRow;
    if (g >= (int64_t)S * b) return;
    const int l = threadIdx.x & (kRow - 1);
    const int s = (int)(g / b), j = (int)(g % b);
    int64_t u = sources[s];
    u = u < 0 ? u + N : u;  // torch-style negative indexing, as the one-vs-all scans
    if ((uint64_t)u >= (uint64_t)N) {
        if (!FILL && l == 0) {
            if (err && j == 0) *err = 1;
            counts[g] = 0;
        }
        return;
    }
    const uint32_t *su = mh + u * P + j * r;
    const int64_t key = (int64_t)(band_key(su, r) & mask);
    const int64_t *kb = keys + (int64_t)j * N;
    int64_t lo = 0, hi = N;  // first position whose key is not below the source's (u itself is in the range: it exists)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (kb[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int64_t first = lo;
    hi = N - first > (int64_t)max_bucket + 1 ? first + max_bucket + 1 : N;  // a range that reaches past max_bucket is dropped: no need to find its end
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (kb[mid] <= key) lo = mid + 1; else hi = mid;
    }
    const int64_t len = lo - first;
    int n = 0;
    if (len <= max_bucket) {
        const int32_t *pb = perm + (int64_t)j * N + first;
        const int64_t base = FILL ? offsets[g] : 0;
        for (int64_t i0 = 0; i0 < len; i0 += kRow) {  // row-uniform; the rows of a wavefront run different numbers of rounds
            bool ok = false;
            int64_t v = 0;
            if (i0 + l < len) {
                v = pb[i0 + l];
                if (v != u) {
                    const uint32_t *sv = mh + v * P + j * r;
                    ok = true;
                    for (int i = 0; i < r; ++i) ok = ok && sv[i] == su[i];
                }
            }
            const uint32_t mine = (uint32_t)(__ballot(ok) >> (threadIdx.x & (kWave - kRow))) & 0xFFFFu;  // this row's 16 lanes
            if (FILL && ok) out[base + n + __builtin_popcount(mine & ((1u << l) - 1u))] = (int64_t)s * N + v;
            n += __builtin_popcount(mine);
        }
    }
    if (!FILL && l == 0) counts[g] = n;
}

static int check_lsh_shape(int64_t N, int32_t P, int32_t rows, int32_t bands, int32_t key_bits)
{
    if (N < 0 || N >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;  // (the permutation is int32)
    if (P < 4 || P % 4 || P > 2048) return SS_ERR_UNSUPPORTED;
    if (rows < 1 || bands < 1 || (int64_t)rows * bands > P || key_bits < 1 || key_bits > 64) return SS_ERR_INVALID_ARG;
    return SS_OK;
}

template <bool FILL>
static int lsh_walk(const int64_t *sources, int32_t S, int64_t N, const uint32_t *mh, int32_t P, int32_t rows, int32_t bands,
                    int32_t key_bits, const int64_t *keys, const int32_t *perm, int32_t max_bucket, int32_t *counts,
                    const int64_t *offsets, int64_t *out, int32_t *err_flag, void *stream)
{
    const int rc = check_lsh_shape(N, P, rows, bands, key_bits);
    if (rc != SS_OK) return rc;
    if (S < 0 || max_bucket < 1) return SS_ERR_INVALID_ARG;
    if (S == 0) return SS_OK;
    if (N == 0 || !sources || !mh || !keys || !perm || (FILL ? (!offsets || !out) : !counts)) return SS_ERR_INVALID_ARG;
    const int64_t blocks = ((int64_t)S * bands + 256 / kRow - 1) / (256 / kRow);
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(lsh_walk_kernel<FILL>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sources, (int)S, N, mh, (int)P,
                       (int)rows, (int)bands, key_mask(key_bits), keys, perm, (int)max_bucket, counts, offsets, out, err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

}  // namespace ss

extern "C" int ss_lsh_band_keys(const uint32_t *mh, int64_t N, int32_t P, int32_t rows, int32_t bands, int32_t key_bits, int64_t *keys,
                                void *stream)
{
    using namespace ss;
    const int rc = check_lsh_shape(N, P, rows, bands, key_bits);
    if (rc != SS_OK) return rc;
    if (N == 0) return SS_OK;
    if (!mh || !keys) return SS_ERR_INVALID_ARG;
    const int T = kLshTileWords / P < kLshTileRows ? kLshTileWords / P : kLshTileRows;
    hipLaunchKernelGGL(lsh_band_keys_kernel, dim3((unsigned)((N + T - 1) / T)), dim3(256), 0, (hipStream_t)stream, mh, N, (int)P, (int)rows,
                       (int)bands, key_mask(key_bits), T, keys);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_lsh_count(const int64_t *sources, int32_t S, int64_t N, const uint32_t *mh, int32_t P, int32_t rows, int32_t bands,
                            int32_t key_bits, const int64_t *keys, const int32_t *perm, int32_t max_bucket, int32_t *counts,
                            int32_t *err_flag, void *stream)
{
    return ss::lsh_walk<false>(sources, S, N, mh, P, rows, bands, key_bits, keys, perm, max_bucket, counts, nullptr, nullptr, err_flag, stream);
}

extern "C" int ss_lsh_fill(const int64_t *sources, int32_t S, int64_t N, const uint32_t *mh, int32_t P, int32_t rows, int32_t bands,
                           int32_t key_bits, const int64_t *keys, const int32_t *perm, int32_t max_bucket, const int64_t *offsets,
                           int64_t *out, void *stream)
{
    return ss::lsh_walk<true>(sources, S, N, mh, P, rows, bands, key_bits, keys, perm, max_bucket, nullptr, offsets, out, nullptr, stream);
}
