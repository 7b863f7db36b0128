// ms_md_chain_scores: the score matrices of the multi-domain search's `exhaustive_cosine` mode.
//
// Candidate c is one (query chain, target chain) pair: nqd query domains (adjacent rows of q) against nhd target domains
// (database rows named by a slice of trows).  Cell (i, j) of its matrix gets exactly what ms_ip_topk returns for that query
// and that row in `mode`, scores below min_score (and NaN) stored as +0.0; out_match[c] counts the rows and the columns
// that keep a non-zero entry -- the two early exits of multidomain.chain_mappings, taken on the device.
//
// Bit-exactness fixes the inner loop: a score is ONE sequential chain of 128 fmaf in the scan's order (s = 0..63: element s,
// then element 64 + s), so the dimension cannot be split over lanes.  One lane owns one cell; one wave (= one workgroup)
// owns one candidate, its cells lane-strided: cell e = lane + 64 i, query row e / nhd, target e % nhd.  Both operands are
// read with 16-byte loads from the two halves of the vector.  The gathers are uncoalesced by nature; neighbouring lanes
// share a query row (nhd of them) or a target row (every nhd-th), and the host orders candidates by query chain and trows
// by row, so the reads are served by the L2.  Row / column occupancy: one bit per row and per column in LDS (ds_or), counted
// at the end.  Vector stores only, no global atomics, no scratch.
// The queries are prepared by the scan's own launch (ms_launch_prepare_queries) into the workspace.
#include "ms_common.h"

#include <math.h>

#define MS_MD_MAX_DOMAINS 4096                       // nqd, nhd <= this (bits of the occupancy maps)
#define MS_MD_WORDS (MS_MD_MAX_DOMAINS / 32)

__global__ __launch_bounds__(64) void ms_md_chain_scores_kernel(
        const float *__restrict__ db, int64_t n, const float *__restrict__ qn, int nq, const float *__restrict__ lengths,
        const float *__restrict__ qlen, float mincov, const int32_t *__restrict__ cand, const int64_t *__restrict__ trows,
        int64_t ntrows, const int64_t *__restrict__ mat_off, float min_score, float *__restrict__ out_scores,
        int32_t *__restrict__ out_match) {
    __shared__ uint32_t rowbits[MS_MD_WORDS], colbits[MS_MD_WORDS];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int32_t q0 = cand[4 * c], nqd = cand[4 * c + 1], t_off = cand[4 * c + 2], nhd = cand[4 * c + 3];
    // a descriptor that leaves the queries or the row list (or the occupancy maps) names nothing: {-1, -1}, nothing else
    if (nqd < 1 || nhd < 1 || nqd > MS_MD_MAX_DOMAINS || nhd > MS_MD_MAX_DOMAINS || q0 < 0 || (int64_t)q0 + nqd > (int64_t)nq ||
        t_off < 0 || (int64_t)t_off + nhd > ntrows) {
        if (lane < 2) out_match[2 * c + lane] = -1;
        return;                                                            // (wave-uniform: the whole workgroup leaves)
    }
    const int rwords = (nqd + 31) >> 5, cwords = (nhd + 31) >> 5;
    for (int w = lane; w < rwords; w += 64) rowbits[w] = 0u;
    for (int w = lane; w < cwords; w += 64) colbits[w] = 0u;
    __syncthreads();

    const int64_t *tr = trows + t_off;
    float *out = out_scores + mat_off[c];
    const uint32_t cells = (uint32_t)nqd * (uint32_t)nhd;                  // <= 2^24
    for (uint32_t e = lane; e < cells; e += 64) {
        const uint32_t i = e / (uint32_t)nhd, j = e - i * (uint32_t)nhd;
        const int64_t row = tr[j];
        float s = 0.0f;
        if (row >= 0 && row < n) {                                         // a row outside the database is never read: its cells are 0
            const f32x4 *a = reinterpret_cast<const f32x4 *>(qn + (size_t)(q0 + (int)i) * MS_DIM);
            const f32x4 *b = reinterpret_cast<const f32x4 *>(db + (size_t)row * MS_DIM);
            float acc = 0.0f;
#pragma unroll 4
            for (int g = 0; g < 16; ++g) {
                const f32x4 a0 = a[g], a1 = a[16 + g], b0 = b[g], b1 = b[16 + g];
                acc = fmaf(a0.x, b0.x, acc); acc = fmaf(a1.x, b1.x, acc);
                acc = fmaf(a0.y, b0.y, acc); acc = fmaf(a1.y, b1.y, acc);
                acc = fmaf(a0.z, b0.z, acc); acc = fmaf(a1.z, b1.z, acc);
                acc = fmaf(a0.w, b0.w, acc); acc = fmaf(a1.w, b1.w, acc);
            }
            s = acc;
            if (lengths != nullptr) {                                      // MS_MODE_COSINE_UNIT's length mask, the scan's operations
                const float mk = (qlen[q0 + (int)i] >= lengths[row] * mincov) ? 1.0f : 0.0f;
                s = s * mk;
            }
            if (!(s >= min_score)) s = 0.0f;                               // below the cut, or NaN
        }
        out[e] = s;
        if (s != 0.0f) {                                                   // (-0.0 is zero, as `tm != 0` has it)
            atomicOr(&rowbits[i >> 5], 1u << (i & 31));
            atomicOr(&colbits[j >> 5], 1u << (j & 31));
        }
    }
    __syncthreads();
    int nr = 0, nc = 0;
    for (int w = lane; w < rwords; w += 64) nr += __popc(rowbits[w]);
    for (int w = lane; w < cwords; w += 64) nc += __popc(colbits[w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { nr += __shfl_xor(nr, off); nc += __shfl_xor(nc, off); }
    if (lane == 0) out_match[2 * c] = nr;
    if (lane == 1) out_match[2 * c + 1] = nc;
}

extern "C" size_t ms_md_chain_scores_workspace_bytes(int nq) {
    if (nq < 1) return 0;
    return (size_t)nq * MS_DIM * sizeof(float);
}

extern "C" int ms_md_chain_scores(const float *db, int64_t n, const float *q, int nq, int mode, const float *lengths,
                                  const float *qlen, float mincov, const int32_t *cand, int ncand, const int64_t *trows,
                                  int64_t ntrows, const int64_t *mat_off, float min_score, float *out_scores,
                                  int32_t *out_match, void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    if (mode != MS_MODE_IP_PRENORM && mode != MS_MODE_IP_NORMQ && mode != MS_MODE_COSINE_UNIT)
        MS_FAIL(MS_ERR_ARG, "ms_md_chain_scores: mode %d is not served (MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ, MS_MODE_COSINE_UNIT)", mode);
    if (nq < 1 || n < 0 || ncand < 0 || ntrows < 0)
        MS_FAIL(MS_ERR_ARG, "ms_md_chain_scores: need nq >= 1, n >= 0, ncand >= 0, ntrows >= 0 (nq=%d n=%lld ncand=%d ntrows=%lld)", nq,
                (long long)n, ncand, (long long)ntrows);
    if (!q || !cand || !mat_off || !out_scores || !out_match || !workspace || (n > 0 && !db) || (ntrows > 0 && !trows))
        MS_FAIL(MS_ERR_ARG, "ms_md_chain_scores: NULL pointer");
    if (mode != MS_MODE_COSINE_UNIT && (lengths || qlen))
        MS_FAIL(MS_ERR_ARG, "ms_md_chain_scores: lengths / qlen are only valid in MS_MODE_COSINE_UNIT");
    if (n > 0 && (lengths == nullptr) != (qlen == nullptr)) MS_FAIL(MS_ERR_ARG, "ms_md_chain_scores: lengths and qlen go together");
    if (min_score != min_score) MS_FAIL(MS_ERR_ARG, "ms_md_chain_scores: min_score is NaN (-inf: no cut)");
    if ((((uintptr_t)db | (uintptr_t)workspace) & 15u) != 0)
        MS_FAIL(MS_ERR_ARG, "ms_md_chain_scores: db and workspace must be 16-byte aligned");
    const size_t need = ms_md_chain_scores_workspace_bytes(nq);
    if (workspace_bytes < need)
        MS_FAIL(MS_ERR_WORKSPACE, "ms_md_chain_scores: workspace %zu < %zu bytes", workspace_bytes, need);
    if (ncand == 0) return MS_OK;
    hipStream_t st = (hipStream_t)stream;
    float *qn = (float *)workspace;
    const int rc = ms_launch_prepare_queries(q, nq, nq, mode, qn, st);
    if (rc) return rc;
    hipLaunchKernelGGL(ms_md_chain_scores_kernel, dim3((unsigned)ncand), dim3(64), 0, st, db, n, qn, nq, lengths, qlen, mincov, cand,
                       trows, ntrows, mat_off, min_score, out_scores, out_match);
    MS_LAUNCH_CHECK("ms_md_chain_scores_kernel");
    return MS_OK;
}
