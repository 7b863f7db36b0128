// ms_threshold_edges: every (query, row) cell of a block of rows whose exact score is at or above a FIXED threshold, as a list of
// (query, global row, score) -- what `cluster --complete` asks for the rows whose neighbour lists came back full (DESIGN.md
// section 5.8).  The definition is the header's; the score is ms_ip_topk's for that query and row, bit for bit.
//
// Route: ms_md_chain_scan_mq's, without the chain logic (its header comment derives the error bound E and the threshold; the
// filter loop is the one both kernels call, ms_mq_cells of ms_mq.h; this file keeps the list's encoding and the drain).  A
// workgroup of 4 waves takes tiles of 64 rows, grid-stride: the tile is staged as fp32 in LDS (ms_mq_stage), each wave converts
// it to its two 32-row fp16 A operands in registers and keeps them for its query tiles (wave w: tiles w, w + 4, ... of 32
// queries), 2 x 8 v_mfma_f32_32x32x16_f16 per query tile, every accumulator compared with
//   thr[q] = (min_score - E B |q|) 2^(sr + sq).
// A cell that is not proved below min_score goes to the wave's list in LDS ({query, row of the tile}); the wave drains the list
// with one lane per cell: the exact chain of 128 fmaf from the fp32 row in LDS and the prepared query, the cut (NaN never
// passes), the excluded range of the query, and the emission: ONE global atomic per wave and drain reserves the slots of all the
// drain's cells, each lane then writes its three outputs behind the cap check.  Queries are not served in blocks: a list entry
// holds the query's number in 32 bits, so one pass over the rows serves any nq.
// LDS: 42.5 KB per workgroup.  Vector stores and vector atomics only; per wave one more global atomic for the re-score count at
// its end.  No scratch.
#include "ms_mq.h"

constexpr size_t MS_TE_OFF_TILE = 0;
constexpr size_t MS_TE_OFF_LIST = MS_TE_OFF_TILE + (size_t)MS_MDS_TILE * MS_MDS_ROW_F4 * 16;
constexpr size_t MS_TE_OFF_LIM = MS_TE_OFF_LIST + (size_t)4 * MS_MQ_LIST * 8;
constexpr size_t MS_TE_OFF_FLAG = MS_TE_OFF_LIM + 64 * 4;
constexpr size_t MS_TE_LDS = MS_TE_OFF_FLAG + 64 * 4;
static_assert(MS_TE_LDS <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(256, 2) void ms_threshold_edges_kernel(
        const float *__restrict__ db, int64_t n, int64_t row_offset, const float *__restrict__ qn, const _Float16 *__restrict__ qh,
        const float *__restrict__ thr, int nq, int nq_pad, const int64_t *__restrict__ lo, const int64_t *__restrict__ hi, float min_score,
        float b2, float rscale, int64_t *__restrict__ out_src, int64_t *__restrict__ out_dst, float *__restrict__ out_score, int64_t cap,
        ms_u64 *__restrict__ ctl) {
    __shared__ __attribute__((aligned(16))) char smem[MS_TE_LDS];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + MS_TE_OFF_TILE);
    float *lim = reinterpret_cast<float *>(smem + MS_TE_OFF_LIM);                // (ms_mq_stage's mask limits: no mask here)
    uint32_t *rflag = reinterpret_cast<uint32_t *>(smem + MS_TE_OFF_FLAG);       // [64] the row goes to the exact chain
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    uint2 *list = reinterpret_cast<uint2 *>(smem + MS_TE_OFF_LIST) + wave * MS_MQ_LIST;      // {query, row of the tile}
    const bool has_ranges = lo != nullptr;
    const int nqt = nq_pad / 32;
    uint32_t nresc = 0;                                                          // cells this lane re-scored
    f16x8 af[2][8];                                                              // the tile's A operands: [half][k block]
    int cnt = 0;                                                                 // entries in the wave's list (uniform)
    int64_t r0 = 0;                                                              // first row of the staged tile (uniform)

    // the wave's list -> exact cells -> the outputs: at most MS_MQ_LIST = 4 x 64 cells, one slot reservation for all of them
    auto drain = [&]() __attribute__((always_inline)) {
        float sc[MS_MQ_LIST / 64];
        ms_u64 m[MS_MQ_LIST / 64];
        int total = 0;
#pragma unroll
        for (int c = 0; c < MS_MQ_LIST / 64; ++c) {
            const int e = 64 * c + lane;
            bool ok = false;
            sc[c] = 0.0f;
            if (e < cnt) {
                const uint2 ent = list[e];
                const int q = (int)ent.x, row = (int)ent.y;
                const float s = ms_mq_exact(qn + (size_t)q * MS_DIM, tile + row * MS_MDS_ROW_F4);
                ok = s >= min_score;                                             // (NaN fails)
                if (ok && has_ranges) {
                    const int64_t g = row_offset + r0 + row;
                    ok = !(g >= lo[q] && g < hi[q]);
                }
                sc[c] = s;
                nresc += 1u;
            }
            m[c] = __ballot(ok);
            total += __popcll(m[c]);
        }
        cnt = 0;
        if (total == 0) return;
        uint32_t blo = 0u, bhi = 0u;
        if (lane == 0) {
            const ms_u64 base = atomicAdd(&ctl[0], (ms_u64)total);
            blo = (uint32_t)base; bhi = (uint32_t)(base >> 32);
        }
        ms_u64 slot0 = ((ms_u64)ms_readlane_u(bhi, 0) << 32) | (ms_u64)ms_readlane_u(blo, 0);
#pragma unroll
        for (int c = 0; c < MS_MQ_LIST / 64; ++c) {
            const ms_u64 slot = slot0 + (ms_u64)__popcll(m[c] & ms_mds_low_bits(lane));
            if (((m[c] >> lane) & 1ull) != 0ull && slot < (ms_u64)cap) {
                const uint2 ent = list[64 * c + lane];
                out_src[slot] = (int64_t)ent.x;
                out_dst[slot] = row_offset + r0 + (int64_t)ent.y;
                out_score[slot] = sc[c];
            }
            slot0 += (ms_u64)__popcll(m[c]);
        }
    };

    const int64_t ntiles = (n + MS_MDS_TILE - 1) / MS_MDS_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        r0 = t * MS_MDS_TILE;
        const int nrows = (int)min((int64_t)MS_MDS_TILE, n - r0);
        ms_mq_stage(db, r0, nrows, nullptr, 0.0f, b2, tile, lim, rflag, tid);
        ms_mq_convert(tile, rflag, rscale, r, h, af);
        ms_mq_cells(af, qh, thr, 0, nqt, nrows, nq, wave, lane, cnt,
                    [&](int slot, int ql, int row) __attribute__((always_inline)) { list[slot] = make_uint2((uint32_t)ql, (uint32_t)row); }, drain);
    }
    ms_mq_count_rescored(nresc, lane, ctl);
}

// workspace: ms_mq_ws (prepared queries | their fp16 operands | thresholds) | ctl [4]
extern "C" size_t ms_threshold_edges_workspace_bytes(int64_t n, int nq) {
    if (nq < 1 || n < 0 || nq > 0x7FFFFFE0) return 0;
    return ms_mq_ws_bytes((size_t)ms_mq_pad(nq)) + 4 * sizeof(ms_u64);
}

extern "C" int ms_threshold_edges(const float *db, int64_t n, int64_t row_offset, const float *q, int nq, int mode, const int64_t *lo,
                                  const int64_t *hi, float min_score, float row_norm_bound, int64_t *out_src, int64_t *out_dst,
                                  float *out_score, int64_t cap, int64_t *out_count, int64_t *out_stats, void *workspace,
                                  size_t workspace_bytes, ms_stream_t stream) {
    if (mode != MS_MODE_IP_PRENORM && mode != MS_MODE_IP_NORMQ && mode != MS_MODE_COSINE_UNIT)
        MS_FAIL(MS_ERR_ARG, "ms_threshold_edges: mode %d is not served (MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ, MS_MODE_COSINE_UNIT)", mode);
    if (nq < 1 || n < 0 || cap < 0)
        MS_FAIL(MS_ERR_ARG, "ms_threshold_edges: need nq >= 1, n >= 0, cap >= 0 (nq=%d n=%lld cap=%lld)", nq, (long long)n, (long long)cap);
    if (!q || !out_count || !workspace || (n > 0 && !db) || (cap > 0 && (!out_src || !out_dst || !out_score)))
        MS_FAIL(MS_ERR_ARG, "ms_threshold_edges: NULL pointer");
    if ((lo == nullptr) != (hi == nullptr)) MS_FAIL(MS_ERR_ARG, "ms_threshold_edges: lo and hi go together");
    if (min_score != min_score) MS_FAIL(MS_ERR_ARG, "ms_threshold_edges: min_score is NaN (-inf: no cut)");
    if ((((uintptr_t)db | (uintptr_t)workspace) & 15u) != 0) MS_FAIL(MS_ERR_ARG, "ms_threshold_edges: db and workspace must be 16-byte aligned");
    MS_MQ_CHECK_BOUND("ms_threshold_edges");
    if (n > 2147483647LL) MS_FAIL(MS_ERR_RANGE, "ms_threshold_edges: at most 2^31 - 1 rows per call (n=%lld)", (long long)n);
    const size_t need = ms_threshold_edges_workspace_bytes(n, nq);
    if (need == 0 || workspace_bytes < need) MS_FAIL(MS_ERR_WORKSPACE, "ms_threshold_edges: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int nq_pad = ms_mq_pad(nq);
    const ms_mq_params p = ms_mq_derive(row_norm_bound);
    const ms_mq_ws w = ms_mq_carve(workspace, nq_pad);
    ms_u64 *ctl = (ms_u64 *)w.tail;
    // ctl[0] the slot counter, ctl[1] always 0 here (the chain scans' table status), ctl[2] the re-score count: all reset by the call
    hipLaunchKernelGGL(ms_md_scan_setup_kernel, dim3(1), dim3(256), 0, st, (const int32_t *)nullptr, 0, nq, (int32_t *)nullptr, ctl);
    MS_LAUNCH_CHECK("ms_md_scan_setup_kernel");
    const bool work = n > 0;
    const int rc = ms_mq_launch_operands(q, nq, nq_pad, mode, work, min_score, p, w, ctl, st);
    if (rc) return rc;
    if (work) {
        const int64_t ntiles = (n + MS_MDS_TILE - 1) / MS_MDS_TILE;
        const unsigned grid = (unsigned)(ntiles < MS_MDS_MAX_GRID ? ntiles : MS_MDS_MAX_GRID);
        hipLaunchKernelGGL(ms_threshold_edges_kernel, dim3(grid), dim3(256), 0, st, db, n, row_offset, w.qn, w.qh, w.thr, nq, nq_pad, lo, hi,
                           min_score, p.b2, p.rscale, out_src, out_dst, out_score, cap, ctl);
        MS_LAUNCH_CHECK("ms_threshold_edges_kernel");
    }
    hipLaunchKernelGGL(ms_md_scan_finish_kernel, dim3(1), dim3(1), 0, st, ctl, out_count, out_stats);
    MS_LAUNCH_CHECK("ms_md_scan_finish_kernel");
    return MS_OK;
}
