// ms_md_chain_scan_mq: ms_md_chain_scan for MANY queries -- the same pairs, count and status, bit for bit
// the same cells, with the 16-bit matrix pipe in front of the exact chain.
//
// The scan has a FIXED threshold: a cell is non-zero only if its exact score s (the chain of 128 fmaf of ms_md_chain_scan) is
// >= min_score.  An approximate score a with |a - s| <= E |row||q| therefore PROVES a cell zero when a < min_score - E B |q|
// (B = row_norm_bound >= |row|); only the other cells are re-scored with the exact chain, mask and cut.  No moving bound, no lists of
// candidates, no proof that can fail: a cell that is not proved zero is simply computed.
//
// Operands and scalings are those of the MS_PF_F16X1 image scan (ms_scan_pf16.h), so E = ms_pf_err_coef(MS_PF_F16X1) = 1.05e-3:
//   row operand    row * 2^sr, sr = 14 - ilogb(B), clamped to +-65504, rounded to nearest even -- converted in the kernel from the
//                  fp32 tile in LDS (the fp32 copy is what the exact chain reads);
//   query operand  the PREPARED query (ms_launch_prepare_queries) * 2^sq, sq = 13 - exponent(max |q_i|) clamped to +-60, clamped to
//                  +-65504, rounded to nearest even -- written once per call next to the prepared queries;
//   a              one accumulator chain of 8 v_mfma_f32_32x32x16_f16 per 32 rows x 32 queries, compared in the accumulators' domain
//                  against thr[q] = (min_score - E B |q|) 2^(sr + sq).
//   Error budget per unit of |row||q| (none of the terms depends on the order of the fp32 accumulation): row rounding 2^-11 =
//   4.883e-4; query rounding 2^-11 more, cross term 2^-22; components below the fp16 normal range after scaling 2 x 8.4e-8; fp32
//   accumulation of 128 products inside the matrix pipe, truncating at worst, 128 x 2^-23 = 1.53e-5; the exact chain's own 128
//   roundings 7.6e-6.  Sum 1.00e-3.  Charged to the margin up to E = 1.05e-3 (5e-5 per unit):
//     * a row is taken as bounded when its fp32 sum of squares (any order: relative error <= 128 x 2^-24 = 7.6e-6) is <=
//       B^2 (1 + 1e-5) -- the slack keeps rows normalised in fp32 on the fast path -- so |row| <= B (1 + 9e-6): 9.5e-9 per unit, and
//       row * 2^sr stays below 2^15 (1 + 9e-6) < 65504: no clamp acts on such a row;
//     * |q| is the fp32 sqrt of the fp32 sum of squares times (1 + 1e-5): an upper bound of the norm;
//     * the threshold's own fp32 arithmetic (one multiply chain, one subtraction) is pushed down by 2^-22 of its magnitude.
//   Everything else goes to the exact chain: a row whose sum of squares is above that or not finite (its operand is NaN: every a
//   of the row is NaN, and the comparison is written so that NaN is never proved), a query with a non-finite element, a zero norm or
//   a norm outside [2^-40, 2^40] (thr = -inf), a threshold that leaves the fp32 normal range in the accumulators' domain, and
//   min_score = -inf (nothing is proved: correct, and as slow as one lane per cell).
// In MS_MODE_COSINE_UNIT the length mask multiplies by 0 or 1: a cell proved zero on the unmasked score is zero with the mask too;
// the mask is applied in the exact chain.
//
// Route.  A workgroup of 4 waves takes the chains that START in a range of 256 rows (the table launch of ms_md_scan.h), tile by tile:
// whole chains, at most 64 rows, staged as fp32 in LDS (coalesced 16-byte loads, rows padded to 33 slots).  Each wave converts the
// tile to its two 32-row A operands in registers (64 VGPRs) and keeps them for all its query tiles: wave w takes query tiles
// w, w + 4, ... of 32 queries, reads their B operands from the workspace (256 B per query, L2-resident), runs 2 x 8 matrix
// instructions and compares.  Unproved cells go to the wave's list in LDS; the wave drains it with one lane per cell: the exact
// chain from the fp32 row in LDS and the prepared query, mask, cut, and an LDS atomic OR of the row's bit into that query's 64-bit
// row mask.  Verdicts are read off the row masks: a query chain whose domains all have a non-empty mask is checked against the
// chains of the tile, lane = chain, as in ms_md_chain_scan.  A chain longer than 64 rows is cut into pieces of 64; across the
// pieces LDS carries one matched bit per query and one (saturating) column count per query chain.
// Queries are served in blocks of MS_MQ_QB = 4160 with a stride of 4096: the block of a query chain is the one its q0 falls into
// by the stride, and as nqd <= 64 the chain ends inside it.  nq and nqc are not limited.
// LDS: 76.6 KB per workgroup (two workgroups share a CU).  Vector stores only; LDS atomics; per wave one global atomic per emission
// and one for the re-score count at its end.  No scratch.
#include "ms_mq.h"                           // the operands, the staged tile, the filter loop (ms_mq_cells), the exact cell and the
                                             // host's parameters, workspace front and operand launches: shared with ms_edges.hip

#define MS_MQ_QSTEP 4096                     // q0 / MS_MQ_QSTEP = the block that serves a query chain
#define MS_MQ_QB (MS_MQ_QSTEP + 64)          // queries per block: 130 tiles of 32
#define MS_MQ_GWIN 4096                      // query chains per pass over a long chain (one byte of column count each)

constexpr size_t MS_MQ_OFF_MASK = 0;
constexpr size_t MS_MQ_OFF_TILE = MS_MQ_OFF_MASK + (size_t)MS_MQ_QB * 8;
constexpr size_t MS_MQ_OFF_LIST = MS_MQ_OFF_TILE + (size_t)MS_MDS_TILE * MS_MDS_ROW_F4 * 16;
constexpr size_t MS_MQ_OFF_LIM = MS_MQ_OFF_LIST + (size_t)4 * MS_MQ_LIST * 4;
constexpr size_t MS_MQ_OFF_FLAG = MS_MQ_OFF_LIM + 64 * 4;
constexpr size_t MS_MQ_OFF_QM = MS_MQ_OFF_FLAG + 64 * 4;
constexpr size_t MS_MQ_OFF_COLS = MS_MQ_OFF_QM + (size_t)(MS_MQ_QB / 64 + 1) * 8;
constexpr size_t MS_MQ_LDS = MS_MQ_OFF_COLS + MS_MQ_GWIN;
static_assert(MS_MQ_QB % 64 == 0 && MS_MQ_LDS <= 80 * 1024, "two workgroups per CU");

__global__ __launch_bounds__(256, 2) void ms_md_chain_scan_mq_kernel(
        const float *__restrict__ db, int64_t n, const int64_t *__restrict__ cs, int64_t nchains, const float *__restrict__ qn,
        const _Float16 *__restrict__ qh, const float *__restrict__ thr, int nq, int nq_pad, const float *__restrict__ lengths,
        const float *__restrict__ qlen, float mincov, const int32_t *__restrict__ qchain, int nqc, float min_score, float b2, float rscale,
        int64_t *__restrict__ out_pairs, int64_t cap, const int64_t *__restrict__ first, int64_t nranges, ms_u64 *__restrict__ ctl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ms_u64 *masks = reinterpret_cast<ms_u64 *>(smem + MS_MQ_OFF_MASK);           // [MS_MQ_QB] rows of the tile with a non-zero cell
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + MS_MQ_OFF_TILE);
    float *lim = reinterpret_cast<float *>(smem + MS_MQ_OFF_LIM);                // [64] lengths[row] * mincov
    uint32_t *rflag = reinterpret_cast<uint32_t *>(smem + MS_MQ_OFF_FLAG);       // [64] the row goes to the exact chain
    ms_u64 *qmatch = reinterpret_cast<ms_u64 *>(smem + MS_MQ_OFF_QM);            // long chain: one bit per query of the block
    uint8_t *cols = reinterpret_cast<uint8_t *>(smem + MS_MQ_OFF_COLS);          // long chain: columns per query chain, saturating
    if (ctl[1] != 0ull) return;                                                  // an invalid table is never followed (uniform)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    uint32_t *list = reinterpret_cast<uint32_t *>(smem + MS_MQ_OFF_LIST) + wave * MS_MQ_LIST;
    const bool has_mask = lengths != nullptr;
    const int nblocks = (nq + MS_MQ_QSTEP - 1) / MS_MQ_QSTEP;
    uint32_t nresc = 0;                                                          // cells this lane re-scored
    f16x8 af[2][8];                                                              // the tile's A operands: [half][k block]

    // the staged tile -> af (every wave for itself), NaN for a flagged row
    auto convert = [&]() __attribute__((always_inline)) { ms_mq_convert(tile, rflag, rscale, r, h, af); };

    // the wave's list -> exact cells -> row masks
    int cnt = 0;                                                                 // entries in the wave's list (uniform)
    int qb0 = 0;                                                                 // first query of the block being served (uniform)
    auto drain = [&]() __attribute__((always_inline)) {
        for (int e0 = 0; e0 < cnt; e0 += 64) {
            const int e = e0 + lane;
            if (e < cnt) {
                const uint32_t ent = list[e];
                const int row = (int)(ent & 63u), ql = (int)(ent >> 6);
                const int q = qb0 + ql;
                const float acc = ms_mq_exact(qn + (size_t)q * MS_DIM, tile + row * MS_MDS_ROW_F4);
                const float sc = ms_mds_cut(acc, has_mask, has_mask ? qlen[q] : 0.0f, lim[row], min_score);
                if (sc != 0.0f) atomicOr(&masks[ql], 1ull << row);
                nresc += 1u;
            }
        }
        cnt = 0;
    };

    // every query tile of the block against the staged tile of nrows rows
    auto cells = [&](int nrows) __attribute__((always_inline)) {
        const int nqt = min(MS_MQ_QB / 32, (nq_pad - qb0) / 32);
        ms_mq_cells(af, qh, thr, qb0, nqt, nrows, nq, wave, lane, cnt,
                    [&](int slot, int ql, int row) __attribute__((always_inline)) { list[slot] = ((uint32_t)ql << 6) | (uint32_t)row; }, drain);
    };

    // (only the masks of queries that exist, to a multiple of 64: a call with a few queries does not clear 33 KB per tile)
    auto block_masks = [&]() __attribute__((always_inline)) { return min(MS_MQ_QB, (nq_pad - qb0 + 63) / 64 * 64); };
    auto zero_masks = [&]() __attribute__((always_inline)) {
        const int nm = block_masks();
        for (int i = tid; i < nm; i += 256) masks[i] = 0ull;
    };

    for (int64_t k = blockIdx.x; k < nranges; k += gridDim.x) {
        int64_t c = first[k];
        const int64_t c_hi = k + 1 < nranges ? first[k + 1] : nchains;
        while (c < c_hi) {
            const int64_t r0 = cs[c];
            // ends of the next 64 chains, relative to r0; the ones that still fit into a tile are a prefix (the table ascends).
            // Every wave computes the same values: lane l of EACH wave owns chain c + l.
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
                ms_mq_stage(db, r0, nrows, lengths, mincov, b2, tile, lim, rflag, tid);
                convert();
                for (int blk = 0; blk < nblocks; ++blk) {
                    qb0 = blk * MS_MQ_QSTEP;
                    __syncthreads();                                             // the previous block's verdicts have been read
                    zero_masks();
                    __syncthreads();
                    cells(nrows);
                    __syncthreads();
                    // verdicts: lane = query chain, 64 per wave and step; a live one (every domain matched some row of the tile)
                    // is then checked by all lanes, lane = chain of the tile
                    for (int gb = 64 * wave; gb < nqc; gb += 256) {
                        const int g = gb + lane;
                        int q0 = 0, nqd = 0;
                        bool live = false;
                        if (g < nqc) {
                            q0 = qchain[2 * g]; nqd = qchain[2 * g + 1];
                            live = !ms_mds_bad_chain(q0, nqd, nq) && q0 / MS_MQ_QSTEP == blk && nqd <= maxlen;
                            for (int i = 0; live && i < nqd; ++i) live = masks[q0 - qb0 + i] != 0ull;
                        }
                        ms_u64 lv = __ballot(live);
                        while (lv != 0ull) {
                            const int l = __ffsll((long long)lv) - 1;
                            lv &= lv - 1ull;
                            const int uq = __builtin_amdgcn_readlane(q0, l) - qb0, un = __builtin_amdgcn_readlane(nqd, l);
                            bool rows_ok = true;
                            ms_u64 any = 0ull;
                            for (int i = 0; i < un; ++i) {
                                const ms_u64 m = masks[uq + i] & seg;
                                rows_ok = rows_ok && m != 0ull;
                                any |= m;
                            }
                            const bool qual = owner && rows_ok && __popcll(any) >= un;
                            ms_mds_emit(qual, (int64_t)(gb + l), c + lane, out_pairs, cap, ctl, lane);
                        }
                    }
                }
                c += nch;
            } else {
                // ---- chain c is longer than a tile: pieces of 64 rows; qmatch and cols carry the verdicts' state
                const int64_t e0 = min(max(cs[c + 1], r0), n);
                const int64_t len = e0 - r0;
                for (int blk = 0; blk < nblocks; ++blk) {
                    qb0 = blk * MS_MQ_QSTEP;
                    for (int gw = 0; gw < nqc; gw += MS_MQ_GWIN) {
                        bool mine = false;                                       // a served query chain of this window in this block?
                        for (int gi = tid; gi < MS_MQ_GWIN && gw + gi < nqc; gi += 256) {
                            const int q0 = qchain[2 * (gw + gi)], nqd = qchain[2 * (gw + gi) + 1];
                            mine = mine || (!ms_mds_bad_chain(q0, nqd, nq) && q0 / MS_MQ_QSTEP == blk && (int64_t)nqd <= len);
                        }
                        if (!__syncthreads_or(mine ? 1 : 0)) continue;
                        for (int i = tid; i < MS_MQ_QB / 64; i += 256) qmatch[i] = 0ull;
                        for (int i = tid; i < MS_MQ_GWIN; i += 256) cols[i] = 0;
                        for (int64_t p = r0; p < e0; p += MS_MDS_TILE) {
                            const int nrows = (int)min((int64_t)MS_MDS_TILE, e0 - p);
                            ms_mq_stage(db, p, nrows, lengths, mincov, b2, tile, lim, rflag, tid);
                            convert();
                            zero_masks();
                            __syncthreads();
                            cells(nrows);
                            __syncthreads();
                            for (int qi = 64 * wave; qi < block_masks(); qi += 256) {
                                const ms_u64 bal = __ballot(masks[qi + lane] != 0ull);
                                if (lane == 0 && bal != 0ull) qmatch[qi >> 6] |= bal;
                            }
                            for (int gi = tid; gi < MS_MQ_GWIN && gw + gi < nqc; gi += 256) {
                                const int q0 = qchain[2 * (gw + gi)], nqd = qchain[2 * (gw + gi) + 1];
                                if (ms_mds_bad_chain(q0, nqd, nq) || q0 / MS_MQ_QSTEP != blk) continue;
                                ms_u64 any = 0ull;
                                for (int i = 0; i < nqd; ++i) any |= masks[q0 - qb0 + i];
                                cols[gi] = (uint8_t)min(255, (int)cols[gi] + __popcll(any));
                            }
                        }
                        __syncthreads();
                        for (int gb = 64 * wave; gb < MS_MQ_GWIN && gw + gb < nqc; gb += 256) {
                            const int gi = gb + lane, g = gw + gi;
                            bool qual = false;
                            if (g < nqc) {
                                const int q0 = qchain[2 * g], nqd = qchain[2 * g + 1];
                                qual = !ms_mds_bad_chain(q0, nqd, nq) && q0 / MS_MQ_QSTEP == blk && (int64_t)nqd <= len && (int)cols[gi] >= nqd;
                                for (int i = 0; qual && i < nqd; ++i) qual = ((qmatch[(q0 - qb0 + i) >> 6] >> ((q0 - qb0 + i) & 63)) & 1ull) != 0ull;
                            }
                            ms_mds_emit(qual, (int64_t)g, c, out_pairs, cap, ctl, lane);
                        }
                        __syncthreads();                                         // (the state is reset by the next window)
                    }
                }
                c += 1;
            }
        }
    }
    ms_mq_count_rescored(nresc, lane, ctl);
}

// workspace: ms_mq_ws (prepared queries | their fp16 operands | thresholds) | first [nranges] | ctl [3]
extern "C" size_t ms_md_chain_scan_mq_workspace_bytes(int64_t n, int nq) {
    if (nq < 1 || n < 0 || nq > 0x7FFFFFE0) return 0;
    return ms_mq_ws_bytes((size_t)ms_mq_pad(nq)) + (size_t)(ms_mds_ranges(n) + 3) * sizeof(int64_t);
}

extern "C" int ms_md_chain_scan_mq(const float *db, int64_t n, const int64_t *chain_start, int64_t nchains, const float *q, int nq, int mode,
                                   const float *lengths, const float *qlen, float mincov, const int32_t *qchain, int nqc, float min_score,
                                   int64_t *out_pairs, int64_t cap, int64_t *out_count, int32_t *out_qstatus, float row_norm_bound,
                                   int64_t *out_stats, void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    MS_MDS_CHECK_ARGS("ms_md_chain_scan_mq");
    MS_MQ_CHECK_BOUND("ms_md_chain_scan_mq");
    const size_t need = ms_md_chain_scan_mq_workspace_bytes(n, nq);
    if (need == 0 || workspace_bytes < need) MS_FAIL(MS_ERR_WORKSPACE, "ms_md_chain_scan_mq: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int nq_pad = ms_mq_pad(nq);
    const ms_mq_params p = ms_mq_derive(row_norm_bound);
    const ms_mq_ws w = ms_mq_carve(workspace, nq_pad);
    int64_t *first = (int64_t *)w.tail;
    const int64_t nranges = ms_mds_ranges(n);
    ms_u64 *ctl = (ms_u64 *)(first + nranges);
    MS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(ms_md_chain_scan_mq_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)MS_MQ_LDS));
    hipLaunchKernelGGL(ms_md_scan_setup_kernel, dim3((unsigned)((nqc + 255) / 256 > 0 ? (nqc + 255) / 256 : 1)), dim3(256), 0, st, qchain, nqc,
                       nq, out_qstatus, ctl);
    MS_LAUNCH_CHECK("ms_md_scan_setup_kernel");
    const bool work = nqc > 0 && nchains > 0 && n > 0;
    const int rc = ms_mq_launch_operands(q, nq, nq_pad, mode, work, min_score, p, w, ctl, st);
    if (rc) return rc;
    if (work) {
        const int64_t ncheck = nchains < n + 1 ? nchains : n + 1;
        hipLaunchKernelGGL(ms_md_scan_table_kernel, dim3((unsigned)((ncheck + 1 + 255) / 256)), dim3(256), 0, st, chain_start, nchains, ncheck,
                           n, nranges, first, ctl);
        MS_LAUNCH_CHECK("ms_md_scan_table_kernel");
        const unsigned grid = (unsigned)(nranges < MS_MDS_MAX_GRID ? nranges : MS_MDS_MAX_GRID);
        hipLaunchKernelGGL(ms_md_chain_scan_mq_kernel, dim3(grid), dim3(256), MS_MQ_LDS, st, db, n, chain_start, nchains, w.qn, w.qh, w.thr, nq,
                           nq_pad, lengths, qlen, mincov, qchain, nqc, min_score, p.b2, p.rscale, out_pairs, cap, first, nranges, ctl);
        MS_LAUNCH_CHECK("ms_md_chain_scan_mq_kernel");
    }
    hipLaunchKernelGGL(ms_md_scan_finish_kernel, dim3(1), dim3(1), 0, st, ctl, out_count, out_stats);
    MS_LAUNCH_CHECK("ms_md_scan_finish_kernel");
    return MS_OK;
}
