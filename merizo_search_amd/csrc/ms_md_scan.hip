// ms_md_chain_scan: the pass over ALL rows of the multi-domain search's `database_cosine` mode.
//
// Database rows of one chain are adjacent: target chain c is the run of rows [chain_start[c], chain_start[c + 1]).  For every
// (query chain g, target chain c) the kernel decides what ms_md_chain_scores' out_match decides -- every query domain of g has
// a non-zero cell in the chain's matrix, and at least nqd of the chain's rows have one -- without writing a matrix, and appends
// the pairs that pass to out_pairs.  A cell is ms_md_chain_scores' cell bit for bit: the same prepared queries (the scan's own
// preparation launch), the same sequential chain of 128 fmaf (s = 0..63: element s, then element 64 + s), the same mask and cut.
//
// Route: one lane per target ROW.  A wave stages a tile of up to 64 whole chains' rows (<= 64 rows) in LDS with coalesced 16-byte
// loads (1 KiB per wave instruction), the staged row padded to 33 x 16 bytes so that lane = row reads its own row back with
// ds_read_b128 free of bank conflicts, and keeps that row in 128 registers.  The query elements are wave-uniform (scalar
// operands), so a score costs 128 v_fma per lane and nothing else; the matrix pipe would produce the same bits, but with a
// handful of query domains it would run a 32-query tile nearly empty and needs the ring of ms_scan.h around it.  Per query
// domain ONE ballot says which rows of the tile matched it; lane l owns the l-th chain of the tile and reads its verdict off
// the ballots with its chain's lane mask: no cross-lane reduction, no atomics in LDS.
// Whole chains go to waves: the rows are cut into ranges of MS_MDS_RANGE rows, a wave takes the chains that START in its range
// (ms_md_scan_table_kernel writes the first chain of every range while it validates the table), so a verdict needs no state
// shared between workgroups.  A chain longer than a tile is looped over in pieces of 64 rows by its wave, lane l then keeping the
// matched-domain mask and the column count of query chain l (64 query chains per pass over the chain).
// Vector stores only; one global atomic per wave and query chain that found a pair (the slot counter).  No scratch.
#include "ms_md_scan.h"

// Rows [r0, r0 + nrows) (nrows <= 64, inside the database) -> LDS -> row r0 + lane in `row` (zeros for lane >= nrows).
__device__ __forceinline__ void ms_mds_stage(const float *__restrict__ db, int64_t r0, int nrows, f32x4 *tile, int lane,
                                             float (&row)[MS_DIM]) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(db + (size_t)r0 * MS_DIM);
    const int nf4 = nrows * (MS_DIM / 4);
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();                                                       // the previous tile has been read
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int f = (h * 16 + u) * 64 + lane;
            v[u] = f < nf4 ? src[f] : zero;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int f = (h * 16 + u) * 64 + lane;
            tile[(f >> 5) * MS_MDS_ROW_F4 + (f & 31)] = v[u];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MS_DIM / 4; ++j) {
        const f32x4 t = tile[lane * MS_MDS_ROW_F4 + j];
        row[4 * j] = t.x; row[4 * j + 1] = t.y; row[4 * j + 2] = t.z; row[4 * j + 3] = t.w;
    }
}

// Which rows of the tile keep a non-zero cell for prepared query qv: ms_md_chain_scores' cell, then one ballot.
__device__ __forceinline__ ms_u64 ms_mds_ballot(const float *__restrict__ qv, const float (&row)[MS_DIM], bool has_mask, float qlen_q,
                                                float lim, float min_score, bool valid) {
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < MS_DIM / 2; ++s) {
        acc = fmaf(qv[s], row[s], acc);
        acc = fmaf(qv[MS_DIM / 2 + s], row[MS_DIM / 2 + s], acc);
    }
    const float sc = ms_mds_cut(acc, has_mask, qlen_q, lim, min_score);
    return __ballot(valid && sc != 0.0f);                                  // (-0.0 is zero)
}

__global__ __launch_bounds__(64) void ms_md_chain_scan_kernel(
        const float *__restrict__ db, int64_t n, const int64_t *__restrict__ cs, int64_t nchains, const float *__restrict__ qn, int nq,
        const float *__restrict__ lengths, const float *__restrict__ qlen, float mincov, const int32_t *__restrict__ qchain, int nqc,
        float min_score, int64_t *__restrict__ out_pairs, int64_t cap, const int64_t *__restrict__ first, int64_t nranges,
        ms_u64 *__restrict__ ctl) {
    __shared__ f32x4 tile[MS_MDS_TILE * MS_MDS_ROW_F4];
    if (ctl[1] != 0ull) return;                                            // an invalid table is never followed (uniform)
    const int lane = threadIdx.x;
    const bool has_mask = lengths != nullptr;
    float row[MS_DIM];
    for (int64_t k = blockIdx.x; k < nranges; k += gridDim.x) {
        int64_t c = first[k];
        const int64_t c_hi = k + 1 < nranges ? first[k + 1] : nchains;
        while (c < c_hi) {
            const int64_t r0 = cs[c];
            // ends of the next 64 chains, relative to r0; the ones that still fit into a tile are a prefix (the table ascends)
            const int64_t e = c + 1 + lane <= c_hi ? cs[c + 1 + lane] : (int64_t)-1;
            const bool fits = e > r0 && e - r0 <= MS_MDS_TILE && e <= n;
            const ms_u64 fm = __ballot(fits);
            if (fm & 1ull) {
                // ---- a tile of nch whole chains; lane l < nch owns chain c + l = tile rows [a, b)
                const int nch = ~fm == 0ull ? 64 : __ffsll((long long)~fm) - 1;
                const int b = fits ? (int)(e - r0) : 0;
                int a = __shfl_up(b, 1);
                if (lane == 0) a = 0;
                const bool owner = lane < nch;
                const int nrows = __shfl(b, nch - 1);
                const ms_u64 seg = owner ? (ms_mds_low_bits(b) & ~ms_mds_low_bits(a)) : 0ull;
                int maxlen = owner ? b - a : 0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, off));
                ms_mds_stage(db, r0, nrows, tile, lane, row);
                const bool valid = lane < nrows;
                const float lim = has_mask && valid ? lengths[r0 + lane] * mincov : 0.0f;
                for (int g = 0; g < nqc; ++g) {
                    const int q0 = qchain[2 * g], nqd = qchain[2 * g + 1];
                    if (ms_mds_bad_chain(q0, nqd, nq) || nqd > maxlen) continue;      // (no chain of the tile has nqd rows)
                    ms_u64 rowbits = 0ull, any = 0ull;
                    bool dead = false;
                    for (int i = 0; i < nqd; ++i) {
                        const ms_u64 bal = ms_mds_ballot(qn + (size_t)(q0 + i) * MS_DIM, row, has_mask, has_mask ? qlen[q0 + i] : 0.0f,
                                                         lim, min_score, valid);
                        if (bal == 0ull) { dead = true; break; }                        // no row of the tile matches this domain
                        any |= bal;
                        rowbits |= (ms_u64)((bal & seg) != 0ull) << i;
                    }
                    if (dead) continue;
                    const bool qual = owner && rowbits == ms_mds_low_bits(nqd) && __popcll(any & seg) >= nqd;
                    ms_mds_emit(qual, (int64_t)g, c + lane, out_pairs, cap, ctl, lane);
                }
                c += nch;
            } else {
                // ---- chain c is longer than a tile: pieces of 64 rows, lane l keeps query chain gb + l
                const int64_t e0 = min(max(cs[c + 1], r0), n);
                const int64_t len = e0 - r0;
                for (int gb = 0; gb < nqc; gb += 64) {
                    ms_u64 st_rows = 0ull;
                    int st_cols = 0;
                    const int gn = min(64, nqc - gb);
                    for (int64_t p = r0; p < e0; p += MS_MDS_TILE) {
                        const int nrows = (int)min((int64_t)MS_MDS_TILE, e0 - p);
                        ms_mds_stage(db, p, nrows, tile, lane, row);
                        const bool valid = lane < nrows;
                        const float lim = has_mask && valid ? lengths[p + lane] * mincov : 0.0f;
                        for (int gg = 0; gg < gn; ++gg) {
                            const int q0 = qchain[2 * (gb + gg)], nqd = qchain[2 * (gb + gg) + 1];
                            if (ms_mds_bad_chain(q0, nqd, nq) || (int64_t)nqd > len) continue;
                            ms_u64 rb = 0ull, any = 0ull;
                            for (int i = 0; i < nqd; ++i) {
                                const ms_u64 bal = ms_mds_ballot(qn + (size_t)(q0 + i) * MS_DIM, row, has_mask,
                                                                 has_mask ? qlen[q0 + i] : 0.0f, lim, min_score, valid);
                                any |= bal;
                                rb |= (ms_u64)(bal != 0ull) << i;
                            }
                            if (lane == gg) { st_rows |= rb; st_cols += __popcll(any); }
                        }
                    }
                    bool qual = false;
                    if (lane < gn) {
                        const int q0 = qchain[2 * (gb + lane)], nqd = qchain[2 * (gb + lane) + 1];
                        qual = !ms_mds_bad_chain(q0, nqd, nq) && st_rows == ms_mds_low_bits(nqd) && st_cols >= nqd;
                    }
                    ms_mds_emit(qual, (int64_t)(gb + lane), c, out_pairs, cap, ctl, lane);
                }
                c += 1;
            }
        }
    }
}

extern "C" size_t ms_md_chain_scan_workspace_bytes(int64_t n, int nq) {
    if (nq < 1 || n < 0) return 0;
    return (size_t)nq * MS_DIM * sizeof(float) + (size_t)(ms_mds_ranges(n) + 2) * sizeof(int64_t);
}

extern "C" int ms_md_chain_scan(const float *db, int64_t n, const int64_t *chain_start, int64_t nchains, const float *q, int nq, int mode,
                                const float *lengths, const float *qlen, float mincov, const int32_t *qchain, int nqc, float min_score,
                                int64_t *out_pairs, int64_t cap, int64_t *out_count, int32_t *out_qstatus, void *workspace,
                                size_t workspace_bytes, ms_stream_t stream) {
    MS_MDS_CHECK_ARGS("ms_md_chain_scan");
    const size_t need = ms_md_chain_scan_workspace_bytes(n, nq);
    if (workspace_bytes < need) MS_FAIL(MS_ERR_WORKSPACE, "ms_md_chain_scan: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float *qn = (float *)workspace;
    int64_t *first = (int64_t *)(qn + (size_t)nq * MS_DIM);
    const int64_t nranges = ms_mds_ranges(n);
    ms_u64 *ctl = (ms_u64 *)(first + nranges);
    hipLaunchKernelGGL(ms_md_scan_setup_kernel, dim3((unsigned)((nqc + 255) / 256 > 0 ? (nqc + 255) / 256 : 1)), dim3(256), 0, st, qchain, nqc,
                       nq, out_qstatus, ctl);
    MS_LAUNCH_CHECK("ms_md_scan_setup_kernel");
    if (nqc > 0 && nchains > 0 && n > 0) {
        const int rc = ms_launch_prepare_queries(q, nq, nq, mode, qn, st);
        if (rc) return rc;
        const int64_t ncheck = nchains < n + 1 ? nchains : n + 1;
        hipLaunchKernelGGL(ms_md_scan_table_kernel, dim3((unsigned)((ncheck + 1 + 255) / 256)), dim3(256), 0, st, chain_start, nchains, ncheck,
                           n, nranges, first, ctl);
        MS_LAUNCH_CHECK("ms_md_scan_table_kernel");
        const unsigned grid = (unsigned)(nranges < MS_MDS_MAX_GRID ? nranges : MS_MDS_MAX_GRID);
        hipLaunchKernelGGL(ms_md_chain_scan_kernel, dim3(grid), dim3(64), 0, st, db, n, chain_start, nchains, qn, nq, lengths, qlen, mincov,
                           qchain, nqc, min_score, out_pairs, cap, first, nranges, ctl);
        MS_LAUNCH_CHECK("ms_md_chain_scan_kernel");
    }
    hipLaunchKernelGGL(ms_md_scan_finish_kernel, dim3(1), dim3(1), 0, st, ctl, out_count, (int64_t *)nullptr);
    MS_LAUNCH_CHECK("ms_md_scan_finish_kernel");
    return MS_OK;
}
