// ss_ppr.hip -- batched personalised PageRank, the fourth link heuristic (reference heuristics.py:74-113: PPR, one
// fast_pagerank.pagerank_power call per distinct source node).  S sources run at once as the columns of a row-major fp64
// iterate X[N, Sp] (Sp = S rounded up to even), ping-ponged between two buffers:
//     X_new[v, j] = sum_{u -> v} w_uv * X_old[u, j]  +  [v == src_j] * (n * t_j),      w_uv = (p * A[u, v]) * (1 / r_u)
// a pull over the CSR of A^T built on the host.  t_j = z . x_j is the previous step's dot product with
// z_u = ((1-p)[r_u != 0] + [r_u == 0]) / n.
//
// Layout of one step: a wavefront owns one row; its two 32-lane halves walk the even / odd in-edges of the row, every lane
// holding two columns (one 16-byte load per edge: the 512-byte row of the previous iterate at S = 64), and the two halves are
// added at the end.  Rows with more than SS_PPR_SEGMENT in-edges (hubs) are cut into segments of SS_PPR_SEGMENT edges, each
// walked by its own wavefront into a scratch row; a second kernel adds a hub's segments in segment order.  Every column's sums
// therefore run in an order fixed by the graph alone -- never by S, the column a source sits in, or the other sources -- and the
// per-column reductions (residual, z . x, sum x) go through per-block partials combined in block order: results are
// bit-identical across S and source order.  No atomics, no inter-workgroup waits; two plain launches per iteration, three with hubs.
#include "ss_common.hpp"

namespace ss {

constexpr int kPprRowsPerBlock = 64;  // 4 wavefronts x 16 rows, interleaved
constexpr int kPprWaves = 4;
constexpr int kPprColsPerChunk = 64;  // 32 lanes x 2 columns: one grid.y slice
constexpr int kPprFinalThreads = 256;

struct PprWs {
    double *x[2];     // [N, Sp] iterates; iteration k reads x[(k-1)&1] and writes x[k&1]
    double *part;     // [3][Sp][nbt] per-block partials: sum (x_new - x_old)^2, sum z x_new, sum x_new
    double *segp;     // [n_segments, Sp] hub segment sums
    int64_t *src;     // [S]
    double *t;        // [S] z . x of the last iterate
    double *sum;      // [S] sum of the last iterate
    int32_t *iters;   // [S] steps taken
    int32_t *active;  // [S]
    int64_t nrb, nhb, nbt;
    int32_t Sp;
};

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace carve; returns the bytes needed (0 = unsupported size).  ws may be NULL (size query).
static size_t ppr_layout(int64_t N, int32_t S, int64_t n_hubs, int64_t n_segments, void *ws, PprWs *L)
{
    if (N <= 0 || N >= ((int64_t)1 << 31) || S <= 0 || S > SS_PPR_MAX_COLUMNS || n_hubs < 0 || n_segments < 0) return 0;
    const int32_t Sp = (S + 1) & ~1;
    const int64_t nrb = (N + kPprRowsPerBlock - 1) / kPprRowsPerBlock, nhb = (n_hubs + kPprWaves - 1) / kPprWaves;
    const int64_t nbt = nrb + nhb;
    size_t off = 0;
    size_t o_x0 = off; off += align256((size_t)N * Sp * 8);
    size_t o_x1 = off; off += align256((size_t)N * Sp * 8);
    size_t o_part = off; off += align256((size_t)3 * Sp * nbt * 8);
    size_t o_seg = off; off += align256((size_t)(n_segments > 0 ? n_segments : 1) * Sp * 8);
    size_t o_src = off; off += align256((size_t)S * 8);
    size_t o_t = off; off += align256((size_t)S * 8);
    size_t o_sum = off; off += align256((size_t)S * 8);
    size_t o_it = off; off += align256((size_t)S * 4);
    size_t o_act = off; off += align256((size_t)S * 4);
    if (L) {
        char *b = (char *)ws;
        L->x[0] = (double *)(b + o_x0);
        L->x[1] = (double *)(b + o_x1);
        L->part = (double *)(b + o_part);
        L->segp = (double *)(b + o_seg);
        L->src = (int64_t *)(b + o_src);
        L->t = (double *)(b + o_t);
        L->sum = (double *)(b + o_sum);
        L->iters = (int32_t *)(b + o_it);
        L->active = (int32_t *)(b + o_act);
        L->nrb = nrb;
        L->nhb = nhb;
        L->nbt = nbt;
        L->Sp = Sp;
    }
    return off;
}

__global__ void ppr_begin_kernel(const int64_t *__restrict__ sources, int32_t S, int64_t N, double tol, const double *__restrict__ z,
                                 PprWs W, int32_t *__restrict__ err_flag)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= S) return;
    const int64_t s = sources[j];
    const bool ok = s >= 0 && s < N;
    if (!ok && err_flag) *err_flag = 1;
    const double n = (double)N;
    W.src[j] = ok ? s : -1;
    if (ok) W.x[0][s * W.Sp + j] = n;  // x0 = s = n * e_src (personalize / personalize.sum() * n)
    W.t[j] = ok ? z[s] * n : 0.0;
    W.sum[j] = n;
    W.iters[j] = 0;
    W.active[j] = ok && n > tol;  // the reference's first test: ||x0 - 0|| = n > tol
}

// this lane's share of sum_e w_e * X[col_e, 2pc .. 2pc+1] over edges [e0, e1): the lower half walks e0, e0+2, ..., the upper
// half e0+1, e0+3, ...; each half adds in edge order and the halves are added at the end (the same order for every S)
__device__ inline void ppr_gather(const int32_t *__restrict__ col, const double *__restrict__ w, const double *__restrict__ X, int32_t Sp,
                                  int64_t e0, int64_t e1, int half, int pc, bool live, double &sx, double &sy)
{
    double ax = 0.0, ay = 0.0;
    if (live) {
        const double *xc = X + 2 * pc;
        int64_t e = e0 + half;
        for (; e + 6 < e1; e += 8) {  // four edges of this half in flight
            const int32_t u0 = col[e], u1 = col[e + 2], u2 = col[e + 4], u3 = col[e + 6];
            const double w0 = w[e], w1 = w[e + 2], w2 = w[e + 4], w3 = w[e + 6];
            const double2 x0 = *(const double2 *)(xc + (int64_t)u0 * Sp), x1 = *(const double2 *)(xc + (int64_t)u1 * Sp);
            const double2 x2 = *(const double2 *)(xc + (int64_t)u2 * Sp), x3 = *(const double2 *)(xc + (int64_t)u3 * Sp);
            ax += w0 * x0.x; ay += w0 * x0.y;
            ax += w1 * x1.x; ay += w1 * x1.y;
            ax += w2 * x2.x; ay += w2 * x2.y;
            ax += w3 * x3.x; ay += w3 * x3.y;
        }
        for (; e < e1; e += 2) {
            const double we = w[e];
            const double2 xe = *(const double2 *)(xc + (int64_t)col[e] * Sp);
            ax += we * xe.x; ay += we * xe.y;
        }
    }
    const double ox = __shfl_xor(ax, 32), oy = __shfl_xor(ay, 32);
    sx = ax + ox;  // even + odd (addition commutes exactly: both halves hold the same value)
    sy = ay + oy;
}

// the new value of (v, two columns): store the active ones and add their terms to the lane's running partials
__device__ inline void ppr_emit(double *__restrict__ xn, const double *__restrict__ xo, int32_t Sp, int64_t v, int pc, bool a0, bool a1,
                                double vx, double vy, const PprWs &W, int64_t s0, int64_t s1, const double *__restrict__ z, double n,
                                double acc[3][2])
{
    if (a0 && v == s0) vx = vx + n * W.t[2 * pc];  // + s (z^T x): only the source row holds a non-zero s
    if (a1 && v == s1) vy = vy + n * W.t[2 * pc + 1];
    if (!a0 && !a1) return;
    const int64_t o = v * Sp + 2 * pc;
    const double2 old = *(const double2 *)(xo + o);
    const double zv = z[v];
    if (a0 && a1) {
        *(double2 *)(xn + o) = make_double2(vx, vy);
    } else if (a0) {
        xn[o] = vx;
    } else if (a1) {
        xn[o + 1] = vy;
    }
    if (a0) {
        const double d = vx - old.x;
        acc[0][0] += d * d; acc[1][0] += zv * vx; acc[2][0] += vx;
    }
    if (a1) {
        const double d = vy - old.y;
        acc[0][1] += d * d; acc[1][1] += zv * vy; acc[2][1] += vy;
    }
}

// the four wavefronts' partials of one block, added in wave order, stored as partial `blk` of every column of this chunk
__device__ inline void ppr_block_partials(double acc[3][2], int wv, int lane, int chunk, int64_t blk, const PprWs &W)
{
    __shared__ double sh[kPprWaves][3][kPprColsPerChunk];
    if (lane < 32) {
        for (int q = 0; q < 3; ++q) {
            sh[wv][q][2 * lane] = acc[q][0];
            sh[wv][q][2 * lane + 1] = acc[q][1];
        }
    }
    __syncthreads();
    if (threadIdx.x < kPprColsPerChunk) {
        const int c = chunk * kPprColsPerChunk + threadIdx.x;
        if (c < W.Sp) {
            for (int q = 0; q < 3; ++q) {
                double s = sh[0][q][threadIdx.x];
                for (int k = 1; k < kPprWaves; ++k) s += sh[k][q][threadIdx.x];
                W.part[((int64_t)q * W.Sp + c) * W.nbt + blk] = s;
            }
        }
    }
}

struct PprLane {
    int lane, half, pc;
    bool a0, a1;
    int64_t s0, s1;
};

__device__ inline PprLane ppr_lane(const PprWs &W, int32_t S, int chunk)
{
    PprLane r;
    r.lane = threadIdx.x & 63;
    r.half = r.lane >> 5;
    r.pc = chunk * (kPprColsPerChunk / 2) + (r.lane & 31);
    const int c0 = 2 * r.pc, c1 = c0 + 1;
    r.a0 = c0 < S && W.active[c0];
    r.a1 = c1 < S && W.active[c1];
    r.s0 = r.a0 ? W.src[c0] : -1;
    r.s1 = r.a1 ? W.src[c1] : -1;
    return r;
}

// blocks [0, nrb): 64 rows each (hub rows skipped); blocks [nrb, nrb + ceil(n_segments / 4)): one hub segment per wavefront
__global__ __launch_bounds__(256) void ppr_step_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ w, const double *__restrict__ z, int64_t N,
                                                       const int32_t *__restrict__ hub_rows, const int32_t *__restrict__ hub_seg,
                                                       const int32_t *__restrict__ seg_hub, int64_t n_segments, int32_t S, int32_t k,
                                                       PprWs W)
{
    const int chunk = blockIdx.y, wv = threadIdx.x >> 6;
    const PprLane ln = ppr_lane(W, S, chunk);
    const bool live = ln.a0 || ln.a1;
    if (!__any(live)) {  // every column of this chunk has stopped (wave-uniform: the same flags for every wave of the block)
        return;
    }
    const double *xo = W.x[(k - 1) & 1];
    double *xn = W.x[k & 1];
    const int64_t b = blockIdx.x;
    if (b >= W.nrb) {  // a hub segment: its partial sum goes to the scratch row of the segment
        const int64_t s = (b - W.nrb) * kPprWaves + wv;
        if (s >= n_segments) return;
        const int h = seg_hub[s];
        const int64_t v = hub_rows[h];
        const int64_t e0 = rowptr[v] + (s - hub_seg[h]) * (int64_t)SS_PPR_SEGMENT;
        const int64_t e1 = min(e0 + (int64_t)SS_PPR_SEGMENT, rowptr[v + 1]);
        double vx, vy;
        ppr_gather(col, w, xo, W.Sp, e0, e1, ln.half, ln.pc, live, vx, vy);
        if (ln.half == 0 && live) *(double2 *)(W.segp + s * W.Sp + 2 * ln.pc) = make_double2(vx, vy);
        return;
    }
    const double n = (double)N;
    double acc[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int i = 0; i < kPprRowsPerBlock / kPprWaves; ++i) {
        const int64_t v = b * kPprRowsPerBlock + wv + kPprWaves * i;
        if (v >= N) break;
        const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
        if (e1 - e0 > SS_PPR_SEGMENT) continue;  // hub: ppr_hub_kernel writes it
        double vx, vy;
        ppr_gather(col, w, xo, W.Sp, e0, e1, ln.half, ln.pc, live, vx, vy);
        if (ln.half == 0) ppr_emit(xn, xo, W.Sp, v, ln.pc, ln.a0, ln.a1, vx, vy, W, ln.s0, ln.s1, z, n, acc);
    }
    ppr_block_partials(acc, wv, ln.lane, chunk, b, W);
}

// one hub row per wavefront: its segments' sums added in segment order, then the same emit as an ordinary row
__global__ __launch_bounds__(256) void ppr_hub_kernel(const double *__restrict__ z, int64_t N, const int32_t *__restrict__ hub_rows,
                                                      const int32_t *__restrict__ hub_seg, int64_t n_hubs, int32_t S, int32_t k, PprWs W)
{
    const int chunk = blockIdx.y, wv = threadIdx.x >> 6;
    const PprLane ln = ppr_lane(W, S, chunk);
    if (!__any(ln.a0 || ln.a1)) return;
    const double *xo = W.x[(k - 1) & 1];
    double *xn = W.x[k & 1];
    double acc[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    const int64_t h = (int64_t)blockIdx.x * kPprWaves + wv;
    if (h < n_hubs && ln.half == 0 && (ln.a0 || ln.a1)) {
        const int64_t v = hub_rows[h];
        double vx = 0.0, vy = 0.0;
        for (int s = hub_seg[h]; s < hub_seg[h + 1]; ++s) {
            const double2 p = *(const double2 *)(W.segp + (int64_t)s * W.Sp + 2 * ln.pc);
            vx += p.x; vy += p.y;
        }
        ppr_emit(xn, xo, W.Sp, v, ln.pc, ln.a0, ln.a1, vx, vy, W, ln.s0, ln.s1, z, (double)N, acc);
    }
    ppr_block_partials(acc, wv, ln.lane, chunk, W.nrb + blockIdx.x, W);
}

// one block per column: the block partials reduced in a fixed order, then the reference's stop rule
//     it += 1; stop if not ||x - oldx|| > tol or it >= max_iter
__global__ __launch_bounds__(kPprFinalThreads) void ppr_finalize_kernel(int32_t S, double tol, int32_t max_iter, PprWs W)
{
    const int j = blockIdx.x;
    if (j >= S || !W.active[j]) return;
    __shared__ double sh[3][kPprFinalThreads];
    for (int q = 0; q < 3; ++q) {
        const double *p = W.part + ((int64_t)q * W.Sp + j) * W.nbt;
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < W.nbt; i += kPprFinalThreads) s += p[i];
        sh[q][threadIdx.x] = s;
    }
    __syncthreads();
    for (int off = kPprFinalThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off)
            for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int it = W.iters[j] + 1;
        W.iters[j] = it;
        W.sum[j] = sh[2][0];
        W.t[j] = sh[1][0];
        if (!(sqrt(sh[0][0]) > tol) || it >= max_iter) W.active[j] = 0;
    }
}

// out[l] = (float)(x_col[dst_l] / sum x_col) of the final iterate of column link_col[l]
__global__ void ppr_scores_kernel(const int64_t *__restrict__ dst, const int32_t *__restrict__ link_col, int64_t L, int64_t N, int32_t S,
                                  PprWs W, float *__restrict__ out, int32_t *__restrict__ err_flag)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const int64_t d = dst[l];
    const int c = link_col[l];
    if (d < 0 || d >= N || c < 0 || c >= S) {
        out[l] = 0.0f;
        if (err_flag) *err_flag = 1;
        return;
    }
    out[l] = (float)(W.x[W.iters[c] & 1][d * W.Sp + c] / W.sum[c]);
}

// vectors [S, N] = the normalised final iterates (transposed: one source per row)
__global__ void ppr_vectors_kernel(int64_t N, int32_t S, PprWs W, double *__restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (v >= N) return;
    out[(int64_t)j * N + v] = W.x[W.iters[j] & 1][v * W.Sp + j] / W.sum[j];
}

__global__ void ppr_status_kernel(int32_t S, PprWs W, int32_t *__restrict__ iters, int32_t *__restrict__ n_active)
{
    __shared__ int32_t cnt[256];
    int32_t c = 0;
    for (int j = threadIdx.x; j < S; j += blockDim.x) {
        if (iters) iters[j] = W.iters[j];
        c += W.active[j];
    }
    cnt[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0 && n_active) {
        int32_t s = 0;
        for (int i = 0; i < (int)blockDim.x; ++i) s += cnt[i];
        *n_active = s;
    }
}

static bool ppr_graph_ok(const ss_ppr_graph *g)
{
    return g && g->rowptr && g->z && g->num_nodes > 0 && g->num_nodes < ((int64_t)1 << 31) && g->n_hubs >= 0 && g->n_segments >= 0 &&
           (g->n_hubs == 0 || (g->hub_rows && g->hub_seg && g->seg_hub && g->n_segments > 0)) &&
           (g->nnz == 0 || (g->col && g->w)) && g->nnz >= 0;
}

}  // namespace ss

extern "C" size_t ss_ppr_workspace_bytes(int64_t N, int32_t S, int64_t n_hubs, int64_t n_segments)
{
    return ss::ppr_layout(N, S, n_hubs, n_segments, nullptr, nullptr);
}

extern "C" int ss_ppr_begin(const ss_ppr_graph *g, const int64_t *sources, int32_t S, double tol, void *workspace, size_t workspace_bytes,
                            int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (!ppr_graph_ok(g) || !sources || !workspace) return SS_ERR_INVALID_ARG;
    PprWs W;
    const size_t need = ppr_layout(g->num_nodes, S, g->n_hubs, g->n_segments, workspace, &W);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    if (hipMemsetAsync(W.x[0], 0, (size_t)g->num_nodes * W.Sp * 8, (hipStream_t)stream) != hipSuccess) return SS_ERR_LAUNCH;
    hipLaunchKernelGGL(ppr_begin_kernel, dim3((S + 255) / 256), dim3(256), 0, (hipStream_t)stream, sources, S, g->num_nodes, tol, g->z, W,
                       err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_ppr_iterate(const ss_ppr_graph *g, int32_t S, int32_t iteration, int32_t max_iter, double tol, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    using namespace ss;
    if (!ppr_graph_ok(g) || !workspace || iteration < 1) return SS_ERR_INVALID_ARG;
    PprWs W;
    const size_t need = ppr_layout(g->num_nodes, S, g->n_hubs, g->n_segments, workspace, &W);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    const unsigned chunks = (unsigned)((W.Sp + kPprColsPerChunk - 1) / kPprColsPerChunk);
    const int64_t seg_blocks = (g->n_segments + kPprWaves - 1) / kPprWaves;
    if (W.nrb + seg_blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppr_step_kernel, dim3((unsigned)(W.nrb + seg_blocks), chunks), dim3(256), 0, st, g->rowptr, g->col, g->w, g->z,
                       g->num_nodes, g->hub_rows, g->hub_seg, g->seg_hub, g->n_segments, S, iteration, W);
    SS_LAUNCH_CHECK();
    if (W.nhb > 0) {
        hipLaunchKernelGGL(ppr_hub_kernel, dim3((unsigned)W.nhb, chunks), dim3(256), 0, st, g->z, g->num_nodes, g->hub_rows, g->hub_seg,
                           g->n_hubs, S, iteration, W);
        SS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ppr_finalize_kernel, dim3((unsigned)S), dim3(kPprFinalThreads), 0, st, S, tol, max_iter, W);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_ppr_status(const ss_ppr_graph *g, int32_t S, const void *workspace, size_t workspace_bytes, int32_t *iters,
                             int32_t *n_active, void *stream)
{
    using namespace ss;
    if (!ppr_graph_ok(g) || !workspace) return SS_ERR_INVALID_ARG;
    PprWs W;
    const size_t need = ppr_layout(g->num_nodes, S, g->n_hubs, g->n_segments, (void *)workspace, &W);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    hipLaunchKernelGGL(ppr_status_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, S, W, iters, n_active);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_ppr_vectors(const ss_ppr_graph *g, int32_t S, const void *workspace, size_t workspace_bytes, double *out, void *stream)
{
    using namespace ss;
    if (!ppr_graph_ok(g) || !workspace || !out) return SS_ERR_INVALID_ARG;
    PprWs W;
    const size_t need = ppr_layout(g->num_nodes, S, g->n_hubs, g->n_segments, (void *)workspace, &W);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    hipLaunchKernelGGL(ppr_vectors_kernel, dim3((unsigned)((g->num_nodes + 255) / 256), (unsigned)S), dim3(256), 0, (hipStream_t)stream,
                       g->num_nodes, S, W, out);
    SS_LAUNCH_CHECK();
    return SS_OK;
}

extern "C" int ss_ppr_scores(const ss_ppr_graph *g, int32_t S, const int64_t *dst, const int32_t *link_col, int64_t L, const void *workspace,
                             size_t workspace_bytes, float *out, int32_t *err_flag, void *stream)
{
    using namespace ss;
    if (L < 0) return SS_ERR_INVALID_ARG;
    if (L == 0) return SS_OK;
    if (!ppr_graph_ok(g) || !workspace || !dst || !link_col || !out) return SS_ERR_INVALID_ARG;
    PprWs W;
    const size_t need = ppr_layout(g->num_nodes, S, g->n_hubs, g->n_segments, (void *)workspace, &W);
    if (need == 0) return SS_ERR_INVALID_ARG;
    if (workspace_bytes < need) return SS_ERR_WORKSPACE;
    const int64_t blocks = (L + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return SS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(ppr_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dst, link_col, L, g->num_nodes, S, W,
                       out, err_flag);
    SS_LAUNCH_CHECK();
    return SS_OK;
}
