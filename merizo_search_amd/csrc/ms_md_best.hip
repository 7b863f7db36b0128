// ms_md_best_mappings: the best mapping of every (query chain, target chain) candidate, behind ms_md_chain_scores on the same
// device buffers (the definition is the header's).
//
// One wave (= one workgroup of 64) per candidate.  Cell weights are integers (the cell times 2^32, rounded once), totals are
// int64 sums: "best" carries no rounding, no summation order and no floating-point ties.
//
// Kind 0, any order: the rectangular assignment problem by shortest augmenting paths with row and column potentials, rows
// inserted in order 0..nqd-1.  Lanes stride the columns (column j belongs to lane j & 63); the per-column state -- potential
// v, slack minv, the column a column was reached from (way) and its row (row_of) -- lives in LDS because it is indexed by
// run-time columns; the set of visited columns is one bit per owned column in a register of the owning lane.  One step: every
// lane relaxes its free columns from the row the search stands on, the wave takes the argmin of (slack, column) with a
// butterfly (64-bit compare, the smaller column on equal slack), the potentials move by that slack.  At most nqd steps per
// row; a step is a few LDS passes over nhd / 64 columns per lane.  The row that finds no free column proves that no mapping
// exists (the rows before it are all matched: a maximum matching without an augmenting path).
//
// Kind 1, order-preserving: D[i][j] = w[i][j] + max over j' < j of D[i-1][j'], D in the workspace (one int64 per cell at the
// matrix's own offset).  Per row every lane owns a contiguous chunk of columns: the maximum of its chunk of the row above, an
// exclusive max-scan of the chunk maxima over the wave, then the chunk sequentially.  A lane reads only what it wrote itself
// until the backtrack (smallest argmax below the column chosen after it), which follows a workgroup barrier.
//
// Every D cell the kernel reads it wrote in the same launch: the workspace needs no clean-up.  Vector stores only, no
// atomics, no scratch, no run-time indexed register arrays.
#include "ms_common.h"

#include <limits.h>

#define MS_MD_BEST_MAX_QD 64
#define MS_MD_BEST_INF LLONG_MAX
#define MS_MD_BEST_NEG LLONG_MIN

__device__ __forceinline__ bool ms_best_allowed(float m) { return m != 0.0f && m == m; }             // (-0.0 is zero; NaN is not a cell)
__device__ __forceinline__ long long ms_best_weight(float m) {
    const double x = fmin(fmax((double)m, -1048576.0), 1048576.0);
    return __double2ll_rn(x * 4294967296.0);                                                           // exact product, one rounding
}

__global__ __launch_bounds__(64) void ms_md_best_mappings_kernel(
        const float *__restrict__ scores, int64_t total_cells, const int32_t *__restrict__ cand, const int64_t *__restrict__ mat_off,
        int32_t *__restrict__ out_status, int64_t *__restrict__ out_total, int32_t *__restrict__ out_path,
        float *__restrict__ out_cell, long long *__restrict__ dws) {
    __shared__ long long v[MS_MD_BEST_MAX_HD], minv[MS_MD_BEST_MAX_HD], u[MS_MD_BEST_MAX_QD];
    __shared__ int16_t way[MS_MD_BEST_MAX_HD], row_of[MS_MD_BEST_MAX_HD];
    __shared__ int32_t pathl[MS_MD_BEST_MAX_QD];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int32_t nqd = cand[4 * c + 1], nhd = cand[4 * c + 3];
    const int64_t off = mat_off[c];
    int32_t *path0 = out_path + (2 * c) * MS_MD_BEST_MAX_QD, *path1 = path0 + MS_MD_BEST_MAX_QD;
    float *cell0 = out_cell + (2 * c) * MS_MD_BEST_MAX_QD, *cell1 = cell0 + MS_MD_BEST_MAX_QD;

    int bad = 0;                                                           // descriptors are data: nothing is formed from a bad one
    if (nqd < 1 || nhd < 1) bad = -1;
    else if (nqd > MS_MD_BEST_MAX_QD || nhd > MS_MD_BEST_MAX_HD) bad = -2;
    else if (off < 0 || off > total_cells - (int64_t)nqd * nhd) bad = -1;
    if (bad) {                                                             // (wave-uniform: the whole workgroup leaves)
        if (lane < 2) { out_status[2 * c + lane] = bad; out_total[2 * c + lane] = 0; }
        path0[lane] = -1; path1[lane] = -1;
        cell0[lane] = 0.0f; cell1[lane] = 0.0f;
        return;
    }
    const float *M = scores + off;
    const bool fits = nqd <= nhd;                                          // more query domains than columns: no mapping of either kind

    // ---------------------------------------------------------------- kind 0: any order
    for (int j = lane; j < nhd; j += 64) { v[j] = 0; row_of[j] = -1; }
    u[lane] = 0;
    pathl[lane] = -1;
    __syncthreads();
    bool found = fits;
    for (int i = 0; i < nqd && found; ++i) {
        for (int j = lane; j < nhd; j += 64) { minv[j] = MS_MD_BEST_INF; way[j] = -1; }
        uint32_t used = 0u;                                                // bit k: column lane + 64 k was visited in this insertion
        int j0 = -1;                                                       // the column the search stands on; -1: the new row's start
        while (true) {
            const int i0 = j0 < 0 ? i : (int)row_of[j0];
            const long long ui0 = u[i0];
            const float *Mrow = M + i0 * nhd;
            long long best = MS_MD_BEST_INF;
            int bestj = INT_MAX;
            for (int k = 0, j = lane; j < nhd; ++k, j += 64) {
                if ((used >> k) & 1u) continue;
                const float m = Mrow[j];
                long long mv = minv[j];
                if (ms_best_allowed(m)) {
                    const long long cur = -ms_best_weight(m) - ui0 - v[j];
                    if (cur < mv) { mv = cur; minv[j] = cur; way[j] = (int16_t)j0; }
                }
                if (mv < best) { best = mv; bestj = j; }                   // (ascending j: the lane's smallest column on equal slack)
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long ob = __shfl_xor(best, o);
                const int oj = __shfl_xor(bestj, o);
                if (ob < best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
            }
            if (best == MS_MD_BEST_INF) { found = false; break; }          // (wave-uniform) no free column can be reached
            for (int k = 0, j = lane; j < nhd; ++k, j += 64) {
                if ((used >> k) & 1u) { u[row_of[j]] += best; v[j] -= best; }      // (visited columns hold distinct rows)
                else if (minv[j] != MS_MD_BEST_INF) minv[j] -= best;
            }
            if (lane == 0) u[i] += best;
            j0 = bestj;
            if (lane == (j0 & 63)) used |= 1u << (j0 >> 6);
            __syncthreads();
            if (row_of[j0] < 0) break;                                     // a free column: the augmenting path ends here
        }
        if (found && lane == 0) {                                          // augment along `way` (at most i + 1 columns)
            while (j0 >= 0) {
                const int j1 = way[j0];
                row_of[j0] = j1 < 0 ? (int16_t)i : row_of[j1];
                j0 = j1;
            }
        }
        __syncthreads();
    }
    if (found) {
        for (int j = lane; j < nhd; j += 64)
            if (row_of[j] >= 0) pathl[row_of[j]] = j;
    }
    __syncthreads();
    {
        const int p = pathl[lane];                                         // (-1 at and behind nqd, and everywhere without a mapping)
        const float m = p >= 0 ? M[lane * nhd + p] : 0.0f;
        long long t = p >= 0 ? ms_best_weight(m) : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        path0[lane] = p;
        cell0[lane] = m;
        if (lane == 0) { out_status[2 * c] = found ? 1 : 0; out_total[2 * c] = t; }
    }
    __syncthreads();

    // ---------------------------------------------------------------- kind 1: order-preserving
    pathl[lane] = -1;
    long long *D = dws + off;
    long long total1 = 0;
    bool ordered = fits;
    if (fits) {
        const int chunk = (nhd + 63) >> 6;
        const int ja = min(lane * chunk, nhd), jb = min(ja + chunk, nhd);
        for (int j = ja; j < jb; ++j) {
            const float m = M[j];
            D[j] = ms_best_allowed(m) ? ms_best_weight(m) : MS_MD_BEST_NEG;
        }
        for (int i = 1; i < nqd; ++i) {
            const long long *Dp = D + (i - 1) * nhd;
            long long *Dc = D + i * nhd;
            long long x = MS_MD_BEST_NEG;
            for (int j = ja; j < jb; ++j) x = max(x, Dp[j]);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {                             // inclusive max-scan of the chunk maxima
                const long long y = __shfl_up(x, d);
                if (lane >= d) x = max(x, y);
            }
            long long run = __shfl_up(x, 1);                               // exclusive: the maximum over the chunks before this one
            if (lane == 0) run = MS_MD_BEST_NEG;
            for (int j = ja; j < jb; ++j) {
                const float m = M[i * nhd + j];
                Dc[j] = (ms_best_allowed(m) && run != MS_MD_BEST_NEG) ? ms_best_weight(m) + run : MS_MD_BEST_NEG;
                run = max(run, Dp[j]);
            }
        }
        __threadfence_block();
        __syncthreads();                                                   // the backtrack reads cells other lanes wrote
        int limit = nhd;
        for (int i = nqd - 1; i >= 0; --i) {
            const long long *Dc = D + i * nhd;
            long long best = MS_MD_BEST_NEG;
            int bestj = INT_MAX;
            for (int j = lane; j < limit; j += 64) {
                const long long d = Dc[j];
                if (d > best) { best = d; bestj = j; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long ob = __shfl_xor(best, o);
                const int oj = __shfl_xor(bestj, o);
                if (ob > best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
            }
            if (best == MS_MD_BEST_NEG) { ordered = false; break; }        // (wave-uniform)
            if (i == nqd - 1) total1 = best;
            if (lane == 0) pathl[i] = bestj;
            limit = bestj;
        }
    }
    __syncthreads();
    {
        const int p = ordered ? pathl[lane] : -1;
        path1[lane] = p;
        cell1[lane] = p >= 0 ? M[lane * nhd + p] : 0.0f;
        if (lane == 0) { out_status[2 * c + 1] = ordered ? 1 : 0; out_total[2 * c + 1] = ordered ? total1 : 0; }
    }
}

extern "C" size_t ms_md_best_mappings_workspace_bytes(int ncand, int64_t total_cells) {
    if (ncand < 0 || total_cells < 0 || total_cells > (int64_t)1 << 56) return 0;
    return ms_align_up((size_t)total_cells * sizeof(long long), 16) + 16;                  // (never 0 for good arguments)
}

extern "C" int ms_md_best_mappings(const float *scores, int64_t total_cells, const int32_t *cand, int ncand, const int64_t *mat_off,
                                   int32_t *out_status, int64_t *out_total, int32_t *out_path, float *out_cell, void *workspace,
                                   size_t workspace_bytes, ms_stream_t stream) {
    if (ncand < 0 || total_cells < 0)
        MS_FAIL(MS_ERR_ARG, "ms_md_best_mappings: need ncand >= 0 and total_cells >= 0 (ncand=%d total_cells=%lld)", ncand, (long long)total_cells);
    if (!cand || !mat_off || !out_status || !out_total || !out_path || !out_cell || !workspace || (total_cells > 0 && !scores))
        MS_FAIL(MS_ERR_ARG, "ms_md_best_mappings: NULL pointer");
    if (((uintptr_t)workspace & 15u) != 0) MS_FAIL(MS_ERR_ARG, "ms_md_best_mappings: workspace must be 16-byte aligned");
    const size_t need = ms_md_best_mappings_workspace_bytes(ncand, total_cells);
    if (need == 0) MS_FAIL(MS_ERR_ARG, "ms_md_best_mappings: total_cells %lld is out of range", (long long)total_cells);
    if (workspace_bytes < need) MS_FAIL(MS_ERR_WORKSPACE, "ms_md_best_mappings: workspace %zu < %zu bytes", workspace_bytes, need);
    if (ncand == 0) return MS_OK;
    hipLaunchKernelGGL(ms_md_best_mappings_kernel, dim3((unsigned)ncand), dim3(64), 0, (hipStream_t)stream, scores, total_cells, cand,
                       mat_off, out_status, out_total, out_path, out_cell, (long long *)workspace);
    MS_LAUNCH_CHECK("ms_md_best_mappings_kernel");
    return MS_OK;
}
