// The host side every ROUND-BASED reading of the cluster graph shares (ms_cluster.hip: the greedy clustering and the connected
// components; ms_cluster_tree.hip: the single-linkage tree): the workspace head with the rounds' words and the counts, the
// order-preserving score key, the argument record and its checks, the launch of one per-entry pass over both entry sources, the host
// loop over the rounds and the read-back behind the finish launch.  One copy: the entry points refuse the same calls in the same words.
#pragma once
#include "ms_cluster_entries.h"

#define MS_CL_GROUP 4                  // rounds enqueued between two looks at the undecided counts
#define MS_CL_HEAD_BYTES 64            // counters in front of the per-row arrays

struct ms_cl_head {                    // the first MS_CL_HEAD_BYTES of the workspace (every clustering)
    uint32_t word[MS_CL_GROUP];        // per round (slot) of the current group, 0 = it was the last: greedy: rows still undecided
                                       // after it; components, tree: it saw an entry between two trees
    unsigned long long n_reps;         // representatives (components, tree: as many as components)
    unsigned long long saturated;
};

static inline size_t ms_cl_rows_bytes(int64_t n) { return ms_align_up((size_t)n, 16); }

// {score, row} as one unsigned key: a larger score wins, then the smaller row; -0.0 ranks as +0.0; never 0 for a real entry.
__device__ __forceinline__ unsigned long long ms_cl_key(float s, int64_t row) {
    uint32_t b = __float_as_uint(s + 0.0f);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | (unsigned long long)(~(uint32_t)row);
}

// The score behind the upper half of ms_cl_key (bits != 0).
__device__ __forceinline__ float ms_cl_key_score(uint32_t b) { return __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b); }

// What all the entry points are handed: the lists ([n,k]; lists_only: k >= 1 and never NULL, else k >= 0), the extra entries
// (m >= 0), the cuts, the outputs and the workspace.  The checks they all make, in one order, `who` in the messages.
struct ms_cl_args {
    ms_cl_lists lists;
    ms_cl_edges edges;
    const int32_t *lengths;
    float min_score, mincov;
    int64_t *out_rep;
    float *out_score;
    int64_t *out_count;
    int32_t *out_rounds;
    int64_t *out_saturated;
    void *workspace;
    size_t workspace_bytes;
};

static int ms_cl_check_args(const char *who, bool lists_only, const ms_cl_args &a, size_t (*ws_bytes)(int64_t), const char *ws_bytes_name) {
    const ms_cl_lists &l = a.lists;
    const ms_cl_edges &e = a.edges;
    if (!lists_only && (l.k < 0 || e.m < 0)) MS_FAIL(MS_ERR_ARG, "%s: need k >= 0 and m >= 0 (k=%d m=%lld)", who, l.k, (long long)e.m);
    if (((lists_only || l.k > 0) && (!l.dst || !l.score)) || (e.m > 0 && (!e.src || !e.dst || !e.score)) || !a.lengths ||
        !a.out_rep || !a.out_score || !a.out_count || !a.out_rounds || !a.out_saturated || !a.workspace)
        MS_FAIL(MS_ERR_ARG, "%s: NULL pointer", who);
    if (l.n < 1 || l.n > 2147483647LL) MS_FAIL(MS_ERR_ARG, "%s: need 1 <= n <= 2^31 - 1 (n=%lld)", who, (long long)l.n);
    if (lists_only && l.k < 1) MS_FAIL(MS_ERR_ARG, "%s: need k >= 1 (k=%d)", who, l.k);
    if (a.min_score != a.min_score) MS_FAIL(MS_ERR_ARG, "%s: min_score is NaN (-inf: no cut)", who);
    if (!(a.mincov >= 0.0f && a.mincov <= 1.0f)) MS_FAIL(MS_ERR_ARG, "%s: mincov must lie in [0, 1]", who);
    const size_t need = ws_bytes(l.n);
    if (a.workspace_bytes < need)
        MS_FAIL(MS_ERR_ARG, "%s: workspace of %zu bytes, %s(%lld) = %zu", who, a.workspace_bytes, ws_bytes_name, (long long)l.n, need);
    if (((uintptr_t)a.workspace & 15u) != 0) MS_FAIL(MS_ERR_ARG, "%s: workspace must be 16-byte aligned", who);
    return MS_OK;
}

// One per-entry pass on stream ST: KERNEL over the lists of ms_cl_args A (k > 0), then over its extra entries (m > 0).  EMPTY_TOO:
// with k == 0 the second launch is made whatever m, with one workgroup when m == 0 (the mark step: it resets the round's count).
#define MS_CL_LAUNCH_ENTRIES(KERNEL, A, EMPTY_TOO, ST, ...)                                                                                \
    do {                                                                                                                                   \
        if ((A).lists.k > 0) {                                                                                                             \
            hipLaunchKernelGGL(KERNEL<ms_cl_lists>, dim3(ms_cl_blocks((A).lists.n * (int64_t)(A).lists.k)), dim3(MS_CL_THREADS), 0, ST,   \
                               (A).lists, __VA_ARGS__);                                                                                    \
            MS_LAUNCH_CHECK(#KERNEL "<ms_cl_lists>");                                                                                     \
        }                                                                                                                                  \
        if ((A).edges.m > 0 || ((EMPTY_TOO) && (A).lists.k == 0)) {                                                                        \
            hipLaunchKernelGGL(KERNEL<ms_cl_edges>, dim3((A).edges.m > 0 ? ms_cl_blocks((A).edges.m) : 1u), dim3(MS_CL_THREADS), 0, ST,   \
                               (A).edges, __VA_ARGS__);                                                                                    \
            MS_LAUNCH_CHECK(#KERNEL "<ms_cl_edges>");                                                                                     \
        }                                                                                                                                  \
    } while (0)

// The rounds of a clustering.  round(g) enqueues one round whose launches leave head->word[g] zero when it was the last one needed;
// MS_CL_GROUP of them go out between two looks at the words (one 16-byte read-back).  The first zero word ends it: `rounds` counts up
// to that round (the rounds behind it in the group changed nothing).  Every clustering needs at most n rounds: stuck(last word,
// rounds) makes the error of a call that is past them -- unreachable on sound memory.
template <typename Round, typename Stuck>
static int ms_cl_rounds(int64_t n, const ms_cl_head *head, hipStream_t st, int64_t &rounds, Round round, Stuck stuck) {
    for (bool done = false; !done;) {
        for (int g = 0; g < MS_CL_GROUP; ++g) {
            const int rc = round(g);
            if (rc) return rc;
        }
        uint32_t word[MS_CL_GROUP];
        MS_HIP_CHECK(hipMemcpyAsync(word, head->word, sizeof(word), hipMemcpyDeviceToHost, st));
        MS_HIP_CHECK(hipStreamSynchronize(st));
        for (int g = 0; g < MS_CL_GROUP && !done; ++g) {
            ++rounds;
            done = word[g] == 0u;
        }
        if (!done && rounds > n) return stuck(word[MS_CL_GROUP - 1], rounds);
    }
    return MS_OK;
}

// Behind the finish launch: the head's counts and the rounds -> the call's scalar outputs.
static int ms_cl_read_head(const ms_cl_head *dev, const ms_cl_args &a, int64_t rounds, hipStream_t st) {
    ms_cl_head head;
    MS_HIP_CHECK(hipMemcpyAsync(&head, dev, sizeof(head), hipMemcpyDeviceToHost, st));
    MS_HIP_CHECK(hipStreamSynchronize(st));
    *a.out_count = (int64_t)head.n_reps;
    *a.out_saturated = a.lists.k > 0 ? (int64_t)head.saturated : 0;        // (no list, no full list)
    *a.out_rounds = (int32_t)rounds;
    return MS_OK;
}
