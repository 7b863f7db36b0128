// ms_ip_topk_large: the exact top-k of ms_ip_topk for 64 < k <= MS_LARGE_K_MAX from ONE filtered pass over the rows instead of
// ceil(k / 64) fp32 scans.  The definition is the header's; every score is ms_ip_topk's, bit for bit.
//
// Exactness.  For ANY threshold t[q], let the bin of query q receive every row whose exact (masked) score is >= t[q].  If the bin
// holds at least k rows and did not overflow, its best k in the search's total order (score descending, row ascending,
// -0.0 == +0.0) are the best k of the whole database: a row outside the bin scores below t[q], hence below k rows of the bin.
// Nothing else is assumed of t[q]; a threshold that is too high is detected (fewer than k rows) and never answers.
//
// Route, all on the caller's stream:
//   (a) bound    the rows are cut into G = ceil(k / 64) contiguous groups and ms_ip_topk (k = 64, the call's mode and mask) runs on
//                each: one fp32 read of the database in all.  ms_tkl_bound_kernel takes the k-th largest of the 64 G scores of a
//                query: at least k real rows reach it.  (lb_in replaces this step: the second round of an overflowed query.)
//   (b) operands ms_tkl_prep_kernel: ms_md_scan_mq_prep_kernel of ms_mq.h with the cut of each query in place of one min_score.
//   (c) emit     ms_tkl_emit_kernel: the loop of ms_threshold_edges_kernel (ms_mq_stage, ms_mq_convert, ms_mq_cells, a drain with
//                one lane per unproved cell and ms_mq_exact) with the length mask in the exact cell and a bin per query: one global
//                atomic per emitted cell reserves its slot, slots at or behind MS_LARGE_K_CAND are counted and not written.
//   (d) select   ms_tkl_select_kernel: a workgroup per query sorts the bin's keys (bitonic, 64 KB of LDS at MS_LARGE_K_CAND) and
//                writes the first k, the status and out_lb.
// A masked search filters on the UNMASKED score, which is sound only while t[q] > 0 (a masked row scores +-0.0 and a non-positive
// cut would have to emit it): a masked query whose cut is not > 0 is status 2 and emits nothing.
// Vector stores and vector atomics only; no scratch memory.
#include "ms_mq.h"

namespace {

constexpr int MS_TKL_SELECT_THREADS = 1024;
constexpr size_t MS_TKL_ALIGN = 256;
// ctl (ms_u64 [8]): [2] cells sent to the exact chain (ms_mq_count_rescored), [4 + s] queries with status s; reset by the bound launch
constexpr int MS_TKL_CTL_WORDS = 8;

// A score as an unsigned 32-bit key of the same order (-0.0 as +0.0; never NaN here), and back (a zero comes back as +0.0).
__device__ __forceinline__ uint32_t ms_tkl_key32(float s) {
    const uint32_t b = __float_as_uint(s + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ms_tkl_unkey32(uint32_t b) { return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b); }

// Bitonic sort of key[0, m) in LDS, largest first (m a power of two >= 2), by nthreads threads of one workgroup.
template <typename K>
__device__ __forceinline__ void ms_tkl_sort_desc(K *key, int m, int tid, int nthreads) {
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < (m >> 1); i += nthreads) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const K a = key[lo], b = key[hi];
                const bool desc = (lo & size) == 0;
                if ((a < b) == desc && a != b) { key[lo] = b; key[hi] = a; }
            }
        }
    }
    __syncthreads();
}

// (a) One workgroup per query: the cut t[q] -- lb_in[q], or the k-th largest of the query's 64 G group-list scores (gs
// [G][nq][64]; -inf is padding) -- and what the emit and select launches go by: tcut[q] = t[q], or NaN for a query that is not
// served (then pre[q] = 2: the cut is NaN or -inf, or the search is masked and the cut is not > 0).  Resets cnt[q] and ctl.
__global__ __launch_bounds__(256) void ms_tkl_bound_kernel(const float *__restrict__ gs, int G, int nq, int k, const float *__restrict__ lb_in,
                                                           int has_mask, float *__restrict__ t, float *__restrict__ tcut,
                                                           int32_t *__restrict__ pre, uint32_t *__restrict__ cnt, ms_u64 *__restrict__ ctl) {
    __shared__ uint32_t key[MS_LARGE_K_MAX];
    __shared__ int nvalid;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (q == 0 && tid < MS_TKL_CTL_WORDS) ctl[tid] = 0ull;
    float tq;
    if (lb_in != nullptr) {
        tq = lb_in[q];
    } else {
        const int m = 64 * G;
        int mp = 128;
        while (mp < m) mp <<= 1;
        if (tid == 0) nvalid = 0;
        __syncthreads();
        int mine = 0;
        for (int i = tid; i < mp; i += 256) {
            const float v = i < m ? gs[((size_t)(i >> 6) * nq + q) * 64 + (i & 63)] : -INFINITY;
            const bool ok = v > -INFINITY;                                  // (NaN fails; the scan returns neither)
            key[i] = ok ? ms_tkl_key32(v) : 0u;
            mine += ok ? 1 : 0;
        }
        if (mine != 0) atomicAdd(&nvalid, mine);
        ms_tkl_sort_desc(key, mp, tid, 256);
        tq = nvalid >= k ? ms_tkl_unkey32(key[k - 1]) : -INFINITY;
    }
    if (tid == 0) {
        bool ok = tq > -INFINITY;                                           // (NaN fails)
        if (has_mask && !(tq > 0.0f)) ok = false;
        t[q] = tq;
        tcut[q] = ok ? tq : __builtin_nanf("");
        pre[q] = ok ? 0 : 2;
        cnt[q] = 0u;
    }
}

// (b) ms_md_scan_mq_prep_kernel with a cut per query: the fp16 operand, and the threshold in the accumulators' domain (+inf for
// the padding behind nq and for a query that emits nothing: proved below; -inf for a query every cell of which goes to the exact
// chain).  The margin E B |q| (1 + 1e-5), the ulp step-down and the "prove nothing" cases are that kernel's.
__global__ __launch_bounds__(256) void ms_tkl_prep_kernel(const float *__restrict__ qn, int nq, int nq_pad, const float *__restrict__ tcut, float eb,
                                                          int sr, _Float16 *__restrict__ qh, float *__restrict__ thr) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_pad) return;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(qn + (size_t)q * MS_DIM);
    float ss = 0.0f, m = 0.0f;
    for (int j = 0; j < MS_DIM / 4; ++j) {
        const f32x4 v = src[j];
        ss += v.x * v.x; ss += v.y * v.y; ss += v.z * v.z; ss += v.w * v.w;
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    int sq = 0;
    if (m > 0.0f && m < INFINITY) sq = 13 - ((int)((__float_as_uint(m) >> 23) & 0xFFu) - 127);
    sq = sq > 60 ? 60 : (sq < -60 ? -60 : sq);
    const float qs = __uint_as_float((uint32_t)(127 + sq) << 23);
    f16x8 *dst = reinterpret_cast<f16x8 *>(qh + (size_t)q * MS_DIM);
    for (int j = 0; j < MS_DIM / 8; ++j) {
        const f32x4 a0 = src[2 * j] * qs, a1 = src[2 * j + 1] * qs;
        const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (_Float16)fminf(fmaxf(x[e], -65504.0f), 65504.0f);      // round to nearest even
        dst[j] = o;
    }
    float t = INFINITY;
    const float cut = q < nq ? tcut[q] : 0.0f;
    if (q < nq && cut == cut) {
        const float nrm = sqrtf(ss);
        const bool flagged = !(ss > 0.0f && ss < INFINITY) || !(nrm >= MS_MQ_NORM_MIN && nrm <= MS_MQ_NORM_MAX);
        t = cut - eb * (nrm * (1.0f + 1e-5f));
        if (t > -INFINITY && t < INFINITY) t = t - fabsf(t) * 2.3841858e-7f;
        t = ldexpf(t, sr + sq);
        if (flagged || !(fabsf(t) >= 7.888609e-31f)) t = -INFINITY;          // (NaN, zero or below 2^-100: nothing is proved)
    }
    thr[q] = t;
}

constexpr size_t MS_TKL_OFF_TILE = 0;
constexpr size_t MS_TKL_OFF_LIST = MS_TKL_OFF_TILE + (size_t)MS_MDS_TILE * MS_MDS_ROW_F4 * 16;
constexpr size_t MS_TKL_OFF_LIM = MS_TKL_OFF_LIST + (size_t)4 * MS_MQ_LIST * 8;
constexpr size_t MS_TKL_OFF_FLAG = MS_TKL_OFF_LIM + 64 * 4;
constexpr size_t MS_TKL_LDS = MS_TKL_OFF_FLAG + 64 * 4;
static_assert(MS_TKL_LDS <= 64 * 1024, "static LDS");

// (c) ms_threshold_edges_kernel's loop with a cut and a bin per query.  The exact cell: the chain of 128 fmaf, times the length
// mask, then score >= tcut[q] (NaN on either side fails, +inf passes, -0.0 counts as 0.0).  An emitted cell takes slot
// atomicAdd(&cnt[q], 1) and writes {score bits, row of the shard} at bins[q * MS_LARGE_K_CAND + slot] when the slot is inside the bin.
__global__ __launch_bounds__(256, 2) void ms_tkl_emit_kernel(
        const float *__restrict__ db, int64_t n, const float *__restrict__ qn, const _Float16 *__restrict__ qh, const float *__restrict__ thr,
        const float *__restrict__ tcut, int nq, int nq_pad, const float *__restrict__ lengths, const float *__restrict__ qlen, float mincov, float b2,
        float rscale, uint32_t *__restrict__ cnt, uint2 *__restrict__ bins, ms_u64 *__restrict__ ctl) {
    __shared__ __attribute__((aligned(16))) char smem[MS_TKL_LDS];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + MS_TKL_OFF_TILE);
    float *lim = reinterpret_cast<float *>(smem + MS_TKL_OFF_LIM);               // [64] lengths[row] * mincov (0 without a mask)
    uint32_t *rflag = reinterpret_cast<uint32_t *>(smem + MS_TKL_OFF_FLAG);      // [64] the row goes to the exact chain
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    uint2 *list = reinterpret_cast<uint2 *>(smem + MS_TKL_OFF_LIST) + wave * MS_MQ_LIST;     // {query, row of the tile}
    const bool has_mask = lengths != nullptr;
    const int nqt = nq_pad / 32;
    uint32_t nresc = 0;                                                          // cells this lane re-scored
    f16x8 af[2][8];                                                              // the tile's A operands: [half][k block]
    int cnt_l = 0;                                                               // entries in the wave's list (uniform)
    int64_t r0 = 0;                                                              // first row of the staged tile (uniform)

    // the wave's list -> exact cells -> the bins: at most MS_MQ_LIST = 4 x 64 cells, one lane per cell
    auto drain = [&]() __attribute__((always_inline)) {
#pragma unroll 1
        for (int c = 0; c < MS_MQ_LIST / 64; ++c) {
            const int e = 64 * c + lane;
            if (e < cnt_l) {
                const uint2 ent = list[e];
                const int q = (int)ent.x, row = (int)ent.y;
                float s = ms_mq_exact(qn + (size_t)q * MS_DIM, tile + row * MS_MDS_ROW_F4);
                if (has_mask) s = s * ((qlen[q] >= lim[row]) ? 1.0f : 0.0f);     // the scan's operations
                nresc += 1u;
                if (s >= tcut[q]) {
                    const uint32_t slot = atomicAdd(&cnt[q], 1u);
                    if (slot < (uint32_t)MS_LARGE_K_CAND)
                        bins[(size_t)q * MS_LARGE_K_CAND + slot] = make_uint2(__float_as_uint(s), (uint32_t)(r0 + row));
                }
            }
        }
        cnt_l = 0;
    };

    const int64_t ntiles = (n + MS_MDS_TILE - 1) / MS_MDS_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        r0 = t * MS_MDS_TILE;
        const int nrows = (int)min((int64_t)MS_MDS_TILE, n - r0);
        ms_mq_stage(db, r0, nrows, lengths, mincov, b2, tile, lim, rflag, tid);
        ms_mq_convert(tile, rflag, rscale, r, h, af);
        ms_mq_cells(af, qh, thr, 0, nqt, nrows, nq, wave, lane, cnt_l,
                    [&](int slot, int ql, int row) __attribute__((always_inline)) { list[slot] = make_uint2((uint32_t)ql, (uint32_t)row); }, drain);
    }
    ms_mq_count_rescored(nresc, lane, ctl);
}

// The select's sort key: ms_order_key with the row's 31 bits moved up by one and, in bit 0, whether the score is -0.0 (rows of a bin
// are distinct, so the bit never decides a compare): the stored score comes back bit for bit.  0 = an empty slot.
__device__ __forceinline__ ms_u64 ms_tkl_key64(uint2 e) {
    const ms_u64 ok = ms_order_key(e);
    return (ok & 0xFFFFFFFF00000000ull) | ((ok & 0x7FFFFFFFull) << 1) | (e.x == 0x80000000u ? 1ull : 0ull);
}
__device__ __forceinline__ uint2 ms_tkl_unkey64(ms_u64 key) {
    const uint32_t b = (uint32_t)(key >> 32);
    uint32_t s = (b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b;
    if ((key & 1ull) != 0ull) s = 0x80000000u;
    return make_uint2(s, (~(uint32_t)(key >> 1)) & 0x7FFFFFFFu);
}

// (d) One workgroup per query: the best k of the bin, the status and out_lb (the header's rules).
__global__ __launch_bounds__(MS_TKL_SELECT_THREADS) void ms_tkl_select_kernel(
        const uint2 *__restrict__ bins, const uint32_t *__restrict__ cnt, const int32_t *__restrict__ pre, const float *__restrict__ t,
        const float *__restrict__ thr, int k, int64_t row_offset, float *__restrict__ out_scores, int64_t *__restrict__ out_idx,
        int32_t *__restrict__ out_status, float *__restrict__ out_lb, ms_u64 *__restrict__ ctl) {
    __shared__ ms_u64 key[MS_LARGE_K_CAND];
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint32_t c = cnt[q];
    const bool over = c > (uint32_t)MS_LARGE_K_CAND;
    int status = 0;
    if (pre[q] != 0 || c < (uint32_t)k) status = 2;
    else if (over) status = thr[q] == -INFINITY ? 2 : 1;                         // (a query the filter cannot take gets no second round)
    float lb = t[q];
    if (status != 2) {
        const int m = over ? MS_LARGE_K_CAND : (int)c;
        int mp = 64;
        while (mp < m) mp <<= 1;
        for (int i = tid; i < mp; i += MS_TKL_SELECT_THREADS) key[i] = i < m ? ms_tkl_key64(bins[(size_t)q * MS_LARGE_K_CAND + i]) : 0ull;
        ms_tkl_sort_desc(key, mp, tid, MS_TKL_SELECT_THREADS);
        if (status == 1) lb = __uint_as_float(ms_tkl_unkey64(key[k - 1]).x);
    }
    for (int i = tid; i < k; i += MS_TKL_SELECT_THREADS) {
        float s = -INFINITY;
        int64_t row = -1;
        if (status == 0) {
            const uint2 e = ms_tkl_unkey64(key[i]);
            s = __uint_as_float(e.x);
            row = row_offset + (int64_t)e.y;
        }
        out_scores[(size_t)q * k + i] = s;
        out_idx[(size_t)q * k + i] = row;
    }
    if (tid == 0) {
        out_status[q] = status;
        out_lb[q] = lb;
        atomicAdd(&ctl[4 + status], 1ull);
    }
}

__global__ void ms_tkl_finish_kernel(const ms_u64 *__restrict__ ctl, int64_t *__restrict__ out_stats) {
    out_stats[0] = (int64_t)ctl[4];
    out_stats[1] = (int64_t)ctl[5];
    out_stats[2] = (int64_t)ctl[6];
    out_stats[3] = (int64_t)ctl[2];
}

// A shape the route does not take: ms_ip_topk answered, every query is final.
__global__ __launch_bounds__(256) void ms_tkl_forwarded_kernel(int nq, int32_t *__restrict__ out_status, float *__restrict__ out_lb,
                                                               int64_t *__restrict__ out_stats) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < nq) { out_status[q] = 0; out_lb[q] = -INFINITY; }
    if (q == 0 && out_stats != nullptr) { out_stats[0] = nq; out_stats[1] = 0; out_stats[2] = 0; out_stats[3] = -1; }
}

inline int tkl_groups(int k) { return (k + 63) / 64; }
inline bool tkl_takes(int64_t n, int k) { return k > 64 && k <= MS_LARGE_K_MAX && n >= (int64_t)128 * tkl_groups(k); }
// Group g of G: rows [n g / G ...): the first n % G groups hold one row more
inline int64_t tkl_group_start(int64_t n, int G, int g) { return (n / G) * g + (g < n % G ? g : n % G); }

// workspace: ms_mq_ws (prepared queries | fp16 operands | thresholds) | ctl | t | tcut | pre | cnt | group scores [G][nq][64] |
// group rows [nq][64] (written by every group, never read) | bins [nq][MS_LARGE_K_CAND] | ms_ip_topk's own workspace
struct TklWs {
    ms_mq_ws mq;
    ms_u64 *ctl;
    float *t, *tcut, *gs;
    int32_t *pre;
    uint32_t *cnt;
    int64_t *gi;
    uint2 *bins;
    char *sub;
    size_t sub_bytes, total;
};

TklWs tkl_carve(void *workspace, int64_t n, int nq, int k) {
    TklWs w{};
    const bool large = tkl_takes(n, k);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = ms_align_up(off + bytes, MS_TKL_ALIGN); return (char *)workspace + at; };
    if (large) {
        const int nq_pad = ms_mq_pad(nq), G = tkl_groups(k);
        w.mq = ms_mq_carve(workspace, nq_pad);
        take(ms_mq_ws_bytes((size_t)nq_pad));
        w.ctl = (ms_u64 *)take(MS_TKL_CTL_WORDS * sizeof(ms_u64));
        w.t = (float *)take((size_t)nq * sizeof(float));
        w.tcut = (float *)take((size_t)nq * sizeof(float));
        w.pre = (int32_t *)take((size_t)nq * sizeof(int32_t));
        w.cnt = (uint32_t *)take((size_t)nq * sizeof(uint32_t));
        w.gs = (float *)take((size_t)G * nq * 64 * sizeof(float));
        w.gi = (int64_t *)take((size_t)nq * 64 * sizeof(int64_t));
        w.bins = (uint2 *)take((size_t)nq * MS_LARGE_K_CAND * sizeof(uint2));
        w.sub_bytes = ms_ip_topk_workspace_bytes(n / G, nq, 64);
        if (n % G != 0) {
            const size_t b = ms_ip_topk_workspace_bytes(n / G + 1, nq, 64);
            w.sub_bytes = b > w.sub_bytes ? b : w.sub_bytes;
        }
    } else {
        w.sub_bytes = ms_ip_topk_workspace_bytes(n, nq, k);
    }
    w.sub = take(w.sub_bytes);
    w.total = w.sub_bytes == 0 ? 0 : off;
    return w;
}

}  // namespace

extern "C" size_t ms_ip_topk_large_workspace_bytes(int64_t n, int nq, int k) {
    if (nq < 1 || n < 0 || k < 1 || nq > 0x7FFFFFE0 || n >= (int64_t)0x7FFFFFFF) return 0;
    return tkl_carve(nullptr, n, nq, k).total;
}

extern "C" int ms_ip_topk_large(const float *db, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode, const float *lengths,
                                const float *qlen, float mincov, float row_norm_bound, const float *lb_in, float *out_scores, int64_t *out_idx,
                                int32_t *out_status, float *out_lb, int64_t *out_stats, void *workspace, size_t workspace_bytes,
                                ms_stream_t stream) {
    if (mode != MS_MODE_IP_PRENORM && mode != MS_MODE_IP_NORMQ && mode != MS_MODE_COSINE_UNIT)
        MS_FAIL(MS_ERR_ARG, "ms_ip_topk_large: mode %d is not served (MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ, MS_MODE_COSINE_UNIT)", mode);
    if (nq < 1 || n < 0 || k < 1 || nq > 0x7FFFFFE0)
        MS_FAIL(MS_ERR_ARG, "ms_ip_topk_large: need nq >= 1, n >= 0, k >= 1 (nq=%d n=%lld k=%d)", nq, (long long)n, k);
    if (!q || !out_scores || !out_idx || !out_status || !out_lb || !workspace || (n > 0 && !db)) MS_FAIL(MS_ERR_ARG, "ms_ip_topk_large: NULL pointer");
    if (mode != MS_MODE_COSINE_UNIT && (lengths || qlen)) MS_FAIL(MS_ERR_ARG, "ms_ip_topk_large: lengths / qlen are only valid in MS_MODE_COSINE_UNIT");
    if (n > 0 && (lengths == nullptr) != (qlen == nullptr)) MS_FAIL(MS_ERR_ARG, "ms_ip_topk_large: lengths and qlen go together");
    if ((((uintptr_t)db | (uintptr_t)workspace) & 15u) != 0) MS_FAIL(MS_ERR_ARG, "ms_ip_topk_large: db and workspace must be 16-byte aligned");
    MS_MQ_CHECK_BOUND("ms_ip_topk_large");
    if (n >= (int64_t)0x7FFFFFFF) MS_FAIL(MS_ERR_RANGE, "ms_ip_topk_large: n=%lld rows per call must be < 2^31 - 1", (long long)n);
    const TklWs w = tkl_carve(workspace, n, nq, k);
    if (w.total == 0 || workspace_bytes < w.total) MS_FAIL(MS_ERR_WORKSPACE, "ms_ip_topk_large: workspace %zu < %zu bytes", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    if (!tkl_takes(n, k)) {
        const int rc = ms_ip_topk(db, n, row_offset, q, nq, k, mode, nullptr, lengths, qlen, mincov, out_scores, out_idx, w.sub, w.sub_bytes, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(ms_tkl_forwarded_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, nq, out_status, out_lb, out_stats);
        MS_LAUNCH_CHECK("ms_tkl_forwarded_kernel");
        return MS_OK;
    }
    const int G = tkl_groups(k), nq_pad = ms_mq_pad(nq);
    const bool has_mask = lengths != nullptr;
    if (lb_in == nullptr) {
        for (int g = 0; g < G; ++g) {
            const int64_t g0 = tkl_group_start(n, G, g), g1 = tkl_group_start(n, G, g + 1);
            const int rc = ms_ip_topk(db + (size_t)g0 * MS_DIM, g1 - g0, 0, q, nq, 64, mode, nullptr, has_mask ? lengths + g0 : nullptr, qlen, mincov,
                                      w.gs + (size_t)g * nq * 64, w.gi, w.sub, w.sub_bytes, stream);
            if (rc) return rc;
        }
    }
    const ms_mq_params p = ms_mq_derive(row_norm_bound);
    int rc = ms_launch_prepare_queries(q, nq, nq_pad, mode, w.mq.qn, st);
    if (rc) return rc;
    hipLaunchKernelGGL(ms_tkl_bound_kernel, dim3((unsigned)nq), dim3(256), 0, st, w.gs, G, nq, k, lb_in, has_mask ? 1 : 0, w.t, w.tcut, w.pre, w.cnt,
                       w.ctl);
    MS_LAUNCH_CHECK("ms_tkl_bound_kernel");
    hipLaunchKernelGGL(ms_tkl_prep_kernel, dim3((unsigned)((nq_pad + 255) / 256)), dim3(256), 0, st, w.mq.qn, nq, nq_pad, w.tcut, p.eb, p.sr, w.mq.qh,
                       w.mq.thr);
    MS_LAUNCH_CHECK("ms_tkl_prep_kernel");
    const int64_t ntiles = (n + MS_MDS_TILE - 1) / MS_MDS_TILE;
    const unsigned grid = (unsigned)(ntiles < MS_MDS_MAX_GRID ? ntiles : MS_MDS_MAX_GRID);
    hipLaunchKernelGGL(ms_tkl_emit_kernel, dim3(grid), dim3(256), 0, st, db, n, w.mq.qn, w.mq.qh, w.mq.thr, w.tcut, nq, nq_pad, lengths, qlen, mincov,
                       p.b2, p.rscale, w.cnt, w.bins, w.ctl);
    MS_LAUNCH_CHECK("ms_tkl_emit_kernel");
    hipLaunchKernelGGL(ms_tkl_select_kernel, dim3((unsigned)nq), dim3(MS_TKL_SELECT_THREADS), 0, st, w.bins, w.cnt, w.pre, w.t, w.mq.thr, k, row_offset,
                       out_scores, out_idx, out_status, out_lb, w.ctl);
    MS_LAUNCH_CHECK("ms_tkl_select_kernel");
    if (out_stats != nullptr) {
        hipLaunchKernelGGL(ms_tkl_finish_kernel, dim3(1), dim3(1), 0, st, w.ctl, out_stats);
        MS_LAUNCH_CHECK("ms_tkl_finish_kernel");
    }
    return MS_OK;
}
