// ss_negatives.hip -- negative links drawn on the device from the CSR the engine already builds: what NegativeSampler.sample /
// sample_negatives return (negatives.py).  Replaces, on the host side of the reference, PyG's negative_sampling
// (src/data.py:199-217), get_same_source_negs (src/utils.py:88-99) and the unfinished sample_hard_negatives (src/data.py:262-304).
//
// Rows: row u of (rowptr, col) = {v : u -> v}, SORTED ascending (ss_csr_sort_rows), duplicates kept.  Slot q makes up to max_tries
// attempts; attempt a draws r0 = draw(seed, q, a, 0), r1 = draw(seed, q, a, 1) (ss_negatives.hpp) and proposes
//   uniform      u = the slot's source, or hi(r0 N) when the call has no sources;  v = hi(r1 N)
//   same_source  u = the slot's source;                                            v = hi(r1 N)
//   wedge        u = the slot's source;  w = row_u[hi(r0 deg u)];                  v = row_w[hi(r1 deg w)]
// and is accepted when v != u and u -> v is neither in the graph's rows nor in the exclude rows (binary searches).  The first accepted
// attempt is the slot's (u, v); none: (u, -1), counted as unsampled.  A slot is a function of (seed, q) and the rows only.
//
//   negatives_kernel<WEDGE>  one lane per slot: the num_neg slots of a positive are neighbouring lanes (their reads of the source and
//                            of rowptr[u] coalesce), everything after that is dependent random loads -- rowptr[w], col[..], then
//                            ~log2(deg) steps per membership search -- so the kernel lives on occupancy (few registers, no LDS).
//                            Lanes of a wavefront leave the attempt loop at different times; the unsampled slots of a wavefront
//                            are counted by one ballot and added by ONE lane's atomic.  The pair leaves as one 16-byte store.
#include "ss_negatives.hpp"

namespace ss {

typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

// is x in the sorted col[b .. e) ?
__device__ __forceinline__ bool row_has(const int32_t *__restrict__ col, int64_t b, int64_t e, int32_t x)
{
    const int64_t lo = bound<false>(col, b, e, x);
    return lo < e && col[lo] == x;
}

template <bool WEDGE>
__global__ __launch_bounds__(256) void negatives_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         const int64_t *__restrict__ xrowptr, const int32_t *__restrict__ xcol, int64_t N,
                                                         const int64_t *__restrict__ sources, int64_t stride, int64_t n_slots,
                                                         int64_t num_neg, uint64_t seed, int max_tries, int64_t first_slot,
                                                         i64x2 *__restrict__ out, int32_t *__restrict__ unsampled,
                                                         int32_t *__restrict__ err)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool missed = false;
    if (t < n_slots) {
        const int64_t q = first_slot + t;
        const uint64_t key = neg_slot_key(seed, (uint64_t)q);
        int64_t u = -1, v = -1, ub = 0, ue = 0;
        bool ok = true;
        if (sources) {  // (sources points at the positive of the launch's first slot)
            u = sources[(q / num_neg - first_slot / num_neg) * stride];
            const int64_t wrapped = u < 0 ? u + N : u;  // torch-style negative indexing, as the link queries
            ok = (uint64_t)wrapped < (uint64_t)N;
            if (ok) {
                u = wrapped;
                ub = rowptr[u];
                ue = rowptr[u + 1];
            } else if (err) {
                *err = 1;  // the slot leaves as (the id as given, -1)
            }
        }
        if (ok && !(WEDGE && ub == ue)) {  // (a wedge source without neighbours has no proposal: unsampled)
            for (int a = 0; a < max_tries; ++a) {
                const uint64_t r0 = neg_draw(key, a, 0), r1 = neg_draw(key, a, 1);
                int64_t c;
                if (WEDGE) {
                    const int64_t w = col[ub + neg_pick(r0, ue - ub)];
                    const int64_t wb = rowptr[w], we = rowptr[w + 1];
                    if (wb == we) continue;  // (only a directed graph has such a w)
                    c = col[wb + neg_pick(r1, we - wb)];
                } else {
                    if (!sources) {
                        u = neg_pick(r0, N);
                        ub = rowptr[u];
                        ue = rowptr[u + 1];
                    }
                    c = neg_pick(r1, N);
                }
                if (c == u || row_has(col, ub, ue, (int32_t)c)) continue;
                if (xrowptr && row_has(xcol, xrowptr[u], xrowptr[u + 1], (int32_t)c)) continue;
                v = c;
                break;
            }
        }
        out[t] = i64x2{u, v};
        missed = v < 0;
    }
    if (unsampled) {
        const unsigned long long m = __ballot(missed);
        if (m && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(unsampled, (int32_t)__builtin_popcountll(m));
    }
}

}  // namespace ss

extern "C" int ss_sample_negatives(const int64_t *rowptr, const int32_t *col, const int64_t *ex_rowptr, const int32_t *ex_col, int64_t N,
                                   const int64_t *sources, int64_t source_stride, int64_t n_slots, int32_t num_neg, int32_t mode,
                                   uint64_t seed, int32_t max_tries, int64_t first_slot, int64_t *out, int32_t *unsampled,
                                   int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (N < 0 || N >= ((int64_t)1 << 31) || n_slots < 0 || num_neg < 1 || first_slot < 0) return SS_ERR_INVALID_ARG;  // (col is int32)
    if (mode != SS_NEG_UNIFORM && mode != SS_NEG_SAME_SOURCE && mode != SS_NEG_WEDGE) return SS_ERR_INVALID_ARG;
    if (max_tries < 1 || max_tries > SS_NEG_MAX_TRIES) return SS_ERR_INVALID_ARG;
    if (mode != SS_NEG_UNIFORM && !sources) return SS_ERR_INVALID_ARG;
    if (sources && source_stride < 1) return SS_ERR_INVALID_ARG;
    if ((ex_rowptr == nullptr) != (ex_col == nullptr)) return SS_ERR_INVALID_ARG;
    if (first_slot > INT64_MAX - n_slots) return SS_ERR_INVALID_ARG;
    if (n_slots == 0) return SS_OK;
    if (!rowptr || !col || !out || ((uintptr_t)out & 15)) return SS_ERR_INVALID_ARG;
    if (N == 0 && !sources) return SS_ERR_INVALID_ARG;  // (no node to draw; with sources every id is out of range and is reported)
    const int64_t blocks = (n_slots + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    auto kernel = mode == SS_NEG_WEDGE ? negatives_kernel<true> : negatives_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, ex_rowptr, ex_col, N, sources,
                       source_stride, n_slots, (int64_t)num_neg, seed, (int)max_tries, first_slot, reinterpret_cast<i64x2 *>(out), unsampled,
                       err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
