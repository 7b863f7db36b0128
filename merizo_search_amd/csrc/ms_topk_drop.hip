// ms_topk_drop_ranges: exact removal of a row range (and of scores below a cut) from sorted top-k lists.
//
// The step a database searched against itself needs behind the scan: every query finds its own
// row first and the sibling domains of its chain next; the caller over-fetches k' = k + (hi - lo) entries and this kernel
// takes the excluded rows out again.  One wave per query.  The list is read in 64-entry pieces, one entry per lane
// (coalesced: 256 B of scores, 512 B of rows per piece); a ballot of the lanes that keep their entry gives each of them
// its place behind what earlier pieces kept (entries before it in the ballot), so the output is in the input's order by
// construction -- no sort, no LDS, no atomics, no scratch.  The wave stops reading once kout entries are out.
#include "ms_common.h"

#define MS_DROP_WAVES 4      // queries (waves) per workgroup

__global__ __launch_bounds__(64 * MS_DROP_WAVES) void ms_topk_drop_ranges_kernel(
        const float *__restrict__ scores, const int64_t *__restrict__ idx, int nq, int kin, const int64_t *__restrict__ lo,
        const int64_t *__restrict__ hi, float min_score, int kout, float *__restrict__ out_scores,
        int64_t *__restrict__ out_idx, int32_t *__restrict__ out_count) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * MS_DROP_WAVES + (threadIdx.x >> 6);
    if (q >= nq) return;                                        // (whole waves leave: q is wave-uniform)
    const int64_t x_lo = lo[q], x_hi = hi[q];                   // lo >= hi: the range is empty
    const float *s_in = scores + (size_t)q * kin;
    const int64_t *i_in = idx + (size_t)q * kin;
    float *s_out = out_scores + (size_t)q * kout;
    int64_t *i_out = out_idx + (size_t)q * kout;
    const unsigned long long below = (1ull << lane) - 1ull;     // the lanes in front of this one
    int written = 0;                                            // wave-uniform: entries kept so far
    for (int base = 0; base < kin && written < kout; base += 64) {
        const int j = base + lane;
        float s = -INFINITY;
        int64_t r = -1;
        if (j < kin) { s = s_in[j]; r = i_in[j]; }
        const bool keep = r >= 0 && !(r >= x_lo && r < x_hi) && !(s < min_score);      // r < 0: padding
        const unsigned long long kept = __ballot(keep);
        const int pos = written + __popcll(kept & below);
        if (keep && pos < kout) { s_out[pos] = s; i_out[pos] = r; }
        written += __popcll(kept);
    }
    if (written > kout) written = kout;
    for (int j = written + lane; j < kout; j += 64) { s_out[j] = -INFINITY; i_out[j] = -1; }
    if (lane == 0) out_count[q] = written;
}

extern "C" int ms_topk_drop_ranges(const float *scores, const int64_t *idx, int nq, int kin, const int64_t *lo, const int64_t *hi,
                                   float min_score, int kout, float *out_scores, int64_t *out_idx, int32_t *out_count,
                                   ms_stream_t stream) {
    if (!scores || !idx || !lo || !hi || !out_scores || !out_idx || !out_count)
        MS_FAIL(MS_ERR_ARG, "ms_topk_drop_ranges: NULL pointer");
    if (nq < 1 || kout < 1 || kin < kout)
        MS_FAIL(MS_ERR_ARG, "ms_topk_drop_ranges: need nq >= 1 and 1 <= kout <= kin (nq=%d kin=%d kout=%d)", nq, kin, kout);
    if (min_score != min_score) MS_FAIL(MS_ERR_ARG, "ms_topk_drop_ranges: min_score is NaN (-inf: no cut)");
    hipLaunchKernelGGL(ms_topk_drop_ranges_kernel, dim3((nq + MS_DROP_WAVES - 1) / MS_DROP_WAVES), dim3(64 * MS_DROP_WAVES), 0,
                       (hipStream_t)stream, scores, idx, nq, kin, lo, hi, min_score, kout, out_scores, out_idx, out_count);
    MS_LAUNCH_CHECK("ms_topk_drop_ranges_kernel");
    return MS_OK;
}
