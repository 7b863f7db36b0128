// What the two chain scans of the multi-domain search share (ms_md_scan.hip: one lane per row; ms_md_scan_mq.hip: the fp16 matrix
// pipe in front of the same exact cell): the ranges and their table, the set-up and finish launches, the cut and the emission.
// The kernels are static: every unit that includes this header gets its own copy.
#pragma once
#include "ms_common.h"

#include <math.h>

#define MS_MDS_RANGE 256                     // rows per range (the chains starting in one range are one work item)
#define MS_MDS_TILE 64                       // rows per tile
#define MS_MDS_ROW_F4 33                     // 16-byte slots per staged row: 32 + 1 of padding
#define MS_MDS_MAX_NQD 64                    // one 64-bit mask of matched query domains per target chain
#define MS_MDS_MAX_GRID 8192

typedef unsigned long long ms_u64;

__device__ __forceinline__ bool ms_mds_bad_chain(int q0, int nqd, int nq) {
    return nqd < 1 || nqd > MS_MDS_MAX_NQD || q0 < 0 || (int64_t)q0 + nqd > (int64_t)nq;
}

// ctl[0]: the slot counter, ctl[1]: non-zero = the chain table broke its rules.  Both reset here, by every call.
// (The matrix route keeps a third word, ctl[2] = cells sent to the exact re-score, and resets it in its own set-up launch.)
static __global__ __launch_bounds__(256) void ms_md_scan_setup_kernel(const int32_t *__restrict__ qchain, int nqc, int nq,
                                                                      int32_t *__restrict__ out_qstatus, ms_u64 *__restrict__ ctl) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g == 0) { ctl[0] = 0ull; ctl[1] = 0ull; }
    if (g < nqc) out_qstatus[g] = ms_mds_bad_chain(qchain[2 * g], qchain[2 * g + 1], nq) ? -1 : 0;
}

// Entry c of the table (c = nchains: the closing n) against its predecessor; the ranges [k R, (k + 1) R) whose first chain
// start at or behind k R is entry c get first[k] = c (every k exactly once when the table is valid).
// (ncheck = min(nchains, n + 1): a table of more than n chains breaks a rule among its first n + 2 entries.)
static __global__ __launch_bounds__(256) void ms_md_scan_table_kernel(const int64_t *__restrict__ cs, int64_t nchains, int64_t ncheck, int64_t n,
                                                                      int64_t nranges, int64_t *__restrict__ first, ms_u64 *__restrict__ ctl) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > ncheck) return;
    const int64_t s = cs[c], prev = c > 0 ? cs[c - 1] : -1;
    const bool ok = (c == 0 ? s == 0 : (prev >= 0 && s > prev)) && s <= n && (c < nchains || s == n);
    if (!ok) { atomicOr(&ctl[1], 1ull); return; }
    for (int64_t k = prev < 0 ? 0 : prev / MS_MDS_RANGE + 1; k < nranges && k * MS_MDS_RANGE <= s; ++k) first[k] = c;
}

// out_stats: NULL, or where the matrix route reports ctl[2].
static __global__ void ms_md_scan_finish_kernel(const ms_u64 *__restrict__ ctl, int64_t *__restrict__ out_count, int64_t *__restrict__ out_stats) {
    *out_count = ctl[1] != 0ull ? (int64_t)-1 : (int64_t)ctl[0];
    if (out_stats != nullptr) out_stats[0] = (int64_t)ctl[2];
}

// The end of ms_md_chain_scores' cell behind its chain of 128 fmaf: MS_MODE_COSINE_UNIT's length mask, then the cut.
__device__ __forceinline__ float ms_mds_cut(float acc, bool has_mask, float qlen_q, float lim, float min_score) {
    float sc = acc;
    if (has_mask) sc = sc * ((qlen_q >= lim) ? 1.0f : 0.0f);               // the scan's operations
    if (!(sc >= min_score)) sc = 0.0f;                                     // below the cut, or NaN
    return sc;                                                             // (-0.0 is zero: callers test sc != 0.0f)
}

__device__ __forceinline__ ms_u64 ms_mds_low_bits(int b) { return b >= 64 ? ~0ull : ((1ull << b) - 1ull); }

// The lanes with `qual` append (g, c): one counter add per wave, slots at or behind cap are counted and not written.
__device__ __forceinline__ void ms_mds_emit(bool qual, int64_t g, int64_t c, int64_t *__restrict__ out_pairs, int64_t cap,
                                            ms_u64 *__restrict__ ctl, int lane) {
    const ms_u64 m = __ballot(qual);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t lo = 0u, hi = 0u;
    if (lane == leader) {
        const ms_u64 base = atomicAdd(&ctl[0], (ms_u64)__popcll(m));
        lo = (uint32_t)base; hi = (uint32_t)(base >> 32);
    }
    const ms_u64 base = ((ms_u64)ms_readlane_u(hi, leader) << 32) | (ms_u64)ms_readlane_u(lo, leader);
    const ms_u64 slot = base + (ms_u64)__popcll(m & ms_mds_low_bits(lane));
    if (qual && slot < (ms_u64)cap) {
        out_pairs[2 * slot] = g;
        out_pairs[2 * slot + 1] = c;
    }
}

static inline int64_t ms_mds_ranges(int64_t n) { return (n + MS_MDS_RANGE - 1) / MS_MDS_RANGE; }

// The argument checks both entry points make, in the same order with the same codes.
#define MS_MDS_CHECK_ARGS(NAME)                                                                                                              \
    do {                                                                                                                                     \
        if (mode != MS_MODE_IP_PRENORM && mode != MS_MODE_IP_NORMQ && mode != MS_MODE_COSINE_UNIT)                                           \
            MS_FAIL(MS_ERR_ARG, NAME ": mode %d is not served (MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ, MS_MODE_COSINE_UNIT)", mode);            \
        if (nq < 1 || n < 0 || nchains < 0 || nqc < 0 || cap < 0)                                                                            \
            MS_FAIL(MS_ERR_ARG, NAME ": need nq >= 1, n >= 0, nchains >= 0, nqc >= 0, cap >= 0 (nq=%d n=%lld nchains=%lld nqc=%d cap=%lld)", \
                    nq, (long long)n, (long long)nchains, nqc, (long long)cap);                                                              \
        if (!q || !out_count || !workspace || (nqc > 0 && (!qchain || !out_qstatus)) || (n > 0 && !db) || (nchains > 0 && !chain_start) ||   \
            (cap > 0 && !out_pairs))                                                                                                         \
            MS_FAIL(MS_ERR_ARG, NAME ": NULL pointer");                                                                                      \
        if (mode != MS_MODE_COSINE_UNIT && (lengths || qlen))                                                                                \
            MS_FAIL(MS_ERR_ARG, NAME ": lengths / qlen are only valid in MS_MODE_COSINE_UNIT");                                              \
        if (n > 0 && (lengths == nullptr) != (qlen == nullptr)) MS_FAIL(MS_ERR_ARG, NAME ": lengths and qlen go together");                  \
        if (min_score != min_score) MS_FAIL(MS_ERR_ARG, NAME ": min_score is NaN (-inf: no cut)");                                           \
        if ((((uintptr_t)db | (uintptr_t)workspace) & 15u) != 0)                                                                             \
            MS_FAIL(MS_ERR_ARG, NAME ": db and workspace must be 16-byte aligned");                                                          \
    } while (0)
