// What a directed entry of the cluster graph IS, for every unit that reads that graph (ms_cluster.hip, ms_cluster_pairs.hip): the
// priority of two rows, the validity rule of an entry, the two entry sources (the [n,k] lists, the m extra entries) and the
// grid-stride pass over them.  One copy: the units cannot disagree on which entries are edges.
#pragma once
#include "ms_common.h"

#define MS_CL_THREADS 256
#define MS_CL_MAX_BLOCKS (1 << 20)     // grid-stride above this many workgroups (2^28 threads: inside HIP's 2^32 per launch)

// Priority: the longer domain, the smaller row on equal length.
__device__ __forceinline__ bool ms_cl_before(int32_t la, int64_t a, int32_t lb, int64_t b) { return la > lb || (la == lb && a < b); }

// A directed entry i->j counts when j is a row other than i, the score is a number at or above min_score and the shorter
// domain covers mincov of the longer one (fp32, this operand order).  lengths[j] is read only behind the range check.
__device__ __forceinline__ bool ms_cl_valid(int64_t i, int64_t j, float s, int64_t n, const int32_t *lengths, int32_t li,
                                            float min_score, float mincov, int32_t *lj_out) {
    if (j < 0 || j >= n || j == i) return false;
    if (!(s >= min_score)) return false;                                  // (NaN fails every comparison)
    const int32_t lj = lengths[j];
    *lj_out = lj;
    const int32_t lmin = li < lj ? li : lj, lmax = li < lj ? lj : li;
    return (float)lmin >= mincov * (float)lmax;
}

// A grid-stride pass over `total` entries: the thread works on entry e = base + thread.
#define MS_CL_FOR_ENTRIES(total)                                                                                   \
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < (total); base += (int64_t)gridDim.x * MS_CL_THREADS)

// The row i of entry base + thread of the [n,k] lists (one 64-bit division per workgroup and pass, a 32-bit one per thread).
__device__ __forceinline__ int64_t ms_cl_entry_row(int64_t base, int k) {
    const int64_t row0 = base / k;
    const uint32_t local = (uint32_t)(base - row0 * k) + threadIdx.x;      // < k + 256
    return row0 + (int64_t)(local / (uint32_t)k);
}

// The two ENTRY SOURCES, passed to the per-entry kernels by value: entry e of total() is i -> dst[e] with score[e], and row(base) is
// the i of the thread's entry e = base + thread, or -1: no such entry, or an i outside [0, n) -- nothing may be looked up with it.
struct ms_cl_lists {                   // the [n,k] lists: i is DERIVED from the entry's place
    const int64_t *__restrict__ dst;
    const float *__restrict__ score;
    int64_t n;
    int k;
    static constexpr bool owns_cut = true;                                 // an entry that is not valid sets cut[i]
    __device__ __forceinline__ int64_t total() const { return n * (int64_t)k; }
    __device__ __forceinline__ int64_t row(int64_t base) const {
        const int64_t i = ms_cl_entry_row(base, k);
        return i < n ? i : -1;
    }
};

struct ms_cl_edges {                   // the m extra entries src[e] -> dst[e]: i is READ, and range-checked before it is used
    const int64_t *__restrict__ src, *__restrict__ dst;
    const float *__restrict__ score;
    int64_t n, m;
    static constexpr bool owns_cut = false;                                // (`cut`, and with it out_saturated, is the lists' alone:
                                                                           // an extra entry that is not valid says nothing about a LIST)
    __device__ __forceinline__ int64_t total() const { return m; }
    __device__ __forceinline__ int64_t row(int64_t base) const {
        const int64_t e = base + threadIdx.x;
        if (e >= m) return -1;
        const int64_t i = src[e];
        return i >= 0 && i < n ? i : -1;
    }
};

static inline unsigned ms_cl_blocks(int64_t items) {
    const int64_t b = (items + MS_CL_THREADS - 1) / MS_CL_THREADS;
    return (unsigned)(b < MS_CL_MAX_BLOCKS ? b : MS_CL_MAX_BLOCKS);
}

