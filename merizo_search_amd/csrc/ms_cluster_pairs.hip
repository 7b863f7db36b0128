// ms_cluster_pairs / ms_cluster_pairs_apply / ms_cluster_pairs_find: the step between the cluster graph and a per-pair verdict
// from outside (`cluster --mintm`: TM-align on every edge; DESIGN.md section 5.8, "Structure-verified edges").
//
// The graph is the one ms_cluster_greedy_edges reads -- the [n,k] lists plus m extra directed entries, the validity rule and the
// priority of ms_cluster_entries.h -- and most of its pairs appear twice or more: i -> j, j -> i, and again among the extras.
//   ms_cluster_pairs        every valid entry inserts its CANONICAL pair (a = the higher-priority row, b = the other) into an
//                           open-addressing set in the workspace; the entry that claims a position hands the pair an output slot.
//   ms_cluster_pairs_apply  every valid entry looks its pair's slot up and, where keep[slot] == 0, is overwritten by padding.
//   ms_cluster_pairs_find   the slot of given pairs.
//
// The set: npos positions (a power of two >= 2 (n k + m): at most half full, so a probe sequence always meets an empty position),
// a 64-bit key a * 2^32 + b per position (all ones: empty; no pair has it, rows are below 2^31) and an int32 slot per position.
// An insert probes linearly from the key's hash; every probe is ONE 64-bit compare-and-swap (empty -> key) whose return value says
// what happened: it was empty (claimed: this entry is the pair's winner), it held the key already (a duplicate: done) or another
// key (next position).  No lane waits for another, and the loop is bounded by npos.  The winners of a wave take their slots with one
// atomicAdd per wave (ballot, as ms_threshold_edges does) and then write the pair (slot < cap) and the position's slot; slots are
// read by later launches only, so the kernel boundary is the hand-off.  Which entry wins a pair, and with it the slot numbering,
// depends on timing; the SET of pairs, the count and the (pair -> slot) map being a bijection onto [0, count) do not.
// Lists: one wave per row, lane-strided over k (the row's length and its "all k valid" ballot are wave-uniform); extras: one lane
// per entry.  Vector loads, stores and atomics only; no LDS, no scratch, no inline assembly.
#include "ms_cluster_entries.h"

#define MS_CP_HEAD_BYTES 64
#define MS_CP_MAGIC 0x6d73637070616972ull                                  // "mscppair": the workspace holds a set
#define MS_CP_EMPTY 0xFFFFFFFFFFFFFFFFull
#define MS_CP_WAVES (MS_CL_THREADS / MS_WAVE)                              // rows per workgroup and pass of the list kernel

struct ms_cp_head {                    // the first MS_CP_HEAD_BYTES of the workspace
    unsigned long long magic;          // MS_CP_MAGIC once a ms_cluster_pairs call has initialised the set
    unsigned long long npos;           // positions of that set
    long long cap;                     // out_pairs slots of that call: a slot at or behind it has no pair written
    long long n;                       // rows of that call
};

struct ms_cp_set {                     // the workspace, carved
    ms_cp_head *head;
    unsigned long long *key;           // [npos]
    int32_t *slot;                     // [npos]
    unsigned long long npos;
};

// Positions for `entries` directed entries: the power of two at or above max(2 entries, 64).  entries < 2^31: at most 2^32.
static inline unsigned long long ms_cp_positions(int64_t entries) {
    unsigned long long p = 64;
    while (p < 2ull * (unsigned long long)entries) p <<= 1;
    return p;
}

static __host__ __device__ inline ms_cp_set ms_cp_carve(const void *workspace, unsigned long long npos) {
    char *p = (char *)workspace;
    ms_cp_set s;
    s.head = (ms_cp_head *)p;
    s.key = (unsigned long long *)(p + MS_CP_HEAD_BYTES);
    s.slot = (int32_t *)(p + MS_CP_HEAD_BYTES + 8 * (size_t)npos);
    s.npos = npos;
    return s;
}

extern "C" size_t ms_cluster_pairs_workspace_bytes(int64_t n, int k, int64_t m) {
    if (n < 1 || n > 2147483647LL || k < 0 || m < 0 || m >= (1LL << 31) || n * (int64_t)k + m >= (1LL << 31)) return 0;
    return MS_CP_HEAD_BYTES + 12 * (size_t)ms_cp_positions(n * (int64_t)k + m);
}

// Where the probe sequence of a key starts (the finaliser of MurmurHash3: every input bit reaches the low bits).
__device__ __forceinline__ unsigned long long ms_cp_hash(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// The canonical pair of the valid entry i -> j as a key: the higher-priority row in the upper half.
__device__ __forceinline__ unsigned long long ms_cp_key(int64_t i, int32_t li, int64_t j, int32_t lj) {
    const bool first = ms_cl_before(li, i, lj, j);
    return ((unsigned long long)(uint32_t)(first ? i : j) << 32) | (unsigned long long)(uint32_t)(first ? j : i);
}

// Insert: the position the key now lives at; *won: this call put it there.  (npos probes without success cannot happen in a set
// that is at most half full; the bound keeps a call on unsound memory finite: *won false, position -1.)
__device__ __forceinline__ long long ms_cp_insert(const ms_cp_set &set, unsigned long long key, bool *won) {
    const unsigned long long mask = set.npos - 1;
    unsigned long long pos = ms_cp_hash(key) & mask;
    *won = false;
    for (unsigned long long probe = 0; probe < set.npos; ++probe, pos = (pos + 1) & mask) {
        const unsigned long long old = atomicCAS(set.key + pos, MS_CP_EMPTY, key);
        if (old == MS_CP_EMPTY) { *won = true; return (long long)pos; }
        if (old == key) return (long long)pos;
    }
    return -1;
}

// Look-up in a set no one writes during this launch: the key's slot, or -1.
__device__ __forceinline__ long long ms_cp_lookup(const ms_cp_set &set, unsigned long long key) {
    const unsigned long long mask = set.npos - 1;
    unsigned long long pos = ms_cp_hash(key) & mask;
    for (unsigned long long probe = 0; probe < set.npos; ++probe, pos = (pos + 1) & mask) {
        const unsigned long long at = set.key[pos];
        if (at == key) return (long long)set.slot[pos];
        if (at == MS_CP_EMPTY) return -1;
    }
    return -1;
}

// Every lane of the wave calls it: the winners get consecutive slots from ONE atomicAdd on *count, write their pair when the slot
// lies below cap, and leave the slot at their position.
__device__ __forceinline__ void ms_cp_hand_out(const ms_cp_set &set, bool won, long long pos, unsigned long long key,
                                               unsigned long long *count, int32_t *out_pairs, long long cap) {
    const unsigned long long winners = __ballot(won);
    if (winners == 0ull) return;                                           // (wave-uniform)
    const int lane = threadIdx.x & (MS_WAVE - 1), leader = __ffsll((long long)winners) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(winners));
    base = __shfl(base, leader);
    if (!won) return;
    const long long slot = (long long)(base + (unsigned long long)__popcll(winners & ((1ull << lane) - 1ull)));
    if (slot < cap) {
        out_pairs[2 * slot] = (int32_t)(key >> 32);
        out_pairs[2 * slot + 1] = (int32_t)(uint32_t)key;
    }
    set.slot[pos] = (int32_t)slot;                                         // (below 2^31: there are fewer entries than that)
}

// An empty set, its head, and both counts at zero.
__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_pairs_init_kernel(ms_cp_set set, long long cap, long long n,
                                                                              unsigned long long *out_count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        set.head->magic = MS_CP_MAGIC;
        set.head->npos = set.npos;
        set.head->cap = cap;
        set.head->n = n;
        out_count[0] = 0ull;
        out_count[1] = 0ull;
    }
    for (unsigned long long p = (unsigned long long)blockIdx.x * MS_CL_THREADS + threadIdx.x; p < set.npos;
         p += (unsigned long long)gridDim.x * MS_CL_THREADS)
        set.key[p] = MS_CP_EMPTY;
}

// The lists: wave w of a workgroup owns row blockIdx * MS_CP_WAVES + w of a pass, lane l its entries l, l + 64, ...
__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_pairs_lists_kernel(
        const int64_t *__restrict__ nbr_idx, const float *__restrict__ nbr_score, int64_t n, int k, const int32_t *__restrict__ lengths,
        float min_score, float mincov, ms_cp_set set, int32_t *out_pairs, long long cap, unsigned long long *out_count) {
    const int lane = threadIdx.x & (MS_WAVE - 1), wave = threadIdx.x / MS_WAVE;
    for (int64_t i = (int64_t)blockIdx.x * MS_CP_WAVES + wave; i < n; i += (int64_t)gridDim.x * MS_CP_WAVES) {      // (wave-uniform)
        const int32_t li = lengths[i];
        bool all_valid = true;
        for (int c0 = 0; c0 < k; c0 += MS_WAVE) {
            const int c = c0 + lane;
            bool valid = false, won = false;
            long long pos = -1;
            unsigned long long key = 0;
            if (c < k) {
                const int64_t j = nbr_idx[i * k + c];
                int32_t lj;
                valid = ms_cl_valid(i, j, nbr_score[i * k + c], n, lengths, li, min_score, mincov, &lj);
                if (valid) {
                    key = ms_cp_key(i, li, j, lj);
                    pos = ms_cp_insert(set, key, &won);
                }
            }
            all_valid = all_valid && __ballot(valid || c >= k) == ~0ull;
            ms_cp_hand_out(set, won, pos, key, out_count, out_pairs, cap);
        }
        if (all_valid && lane == 0) atomicAdd(out_count + 1, 1ull);
    }
}

// The extras: one lane per entry.
__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_pairs_edges_kernel(
        const ms_cl_edges from, const int32_t *__restrict__ lengths, float min_score, float mincov, ms_cp_set set, int32_t *out_pairs,
        long long cap, unsigned long long *out_count) {
    MS_CL_FOR_ENTRIES(from.total()) {
        const int64_t i = from.row(base), e = base + threadIdx.x;
        bool won = false;
        long long pos = -1;
        unsigned long long key = 0;
        if (i >= 0) {
            const int64_t j = from.dst[e];
            const int32_t li = lengths[i];
            int32_t lj;
            if (ms_cl_valid(i, j, from.score[e], from.n, lengths, li, min_score, mincov, &lj)) {
                key = ms_cp_key(i, li, j, lj);
                pos = ms_cp_insert(set, key, &won);
            }
        }
        ms_cp_hand_out(set, won, pos, key, out_count, out_pairs, cap);     // (every lane of the wave, the ones without an entry too)
    }
}

// The set a later call may trust: built by ms_cluster_pairs for n rows with npos positions.
__device__ __forceinline__ bool ms_cp_sound(const ms_cp_set &set, long long n) {
    return set.head->magic == MS_CP_MAGIC && set.head->npos == set.npos && set.head->n == n;
}

// One thread per entry of source `from`, read and written through dst / score (the source's own pointers are const): a valid entry
// whose pair is not kept becomes padding.
template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_pairs_apply_kernel(
        const Src from, int64_t *dst, float *score, const int32_t *__restrict__ lengths, float min_score, float mincov, ms_cp_set set,
        const uint8_t *__restrict__ keep, long long count, unsigned long long *out_removed) {
    const bool sound = ms_cp_sound(set, from.n);
    const long long slots = sound ? (count < set.head->cap ? count : set.head->cap) : 0;
    MS_CL_FOR_ENTRIES(from.total()) {
        const int64_t i = from.row(base), e = base + threadIdx.x;
        bool removed = false;
        if (i >= 0) {
            const int64_t j = dst[e];
            const int32_t li = lengths[i];
            int32_t lj;
            if (ms_cl_valid(i, j, score[e], from.n, lengths, li, min_score, mincov, &lj)) {
                const long long slot = sound ? ms_cp_lookup(set, ms_cp_key(i, li, j, lj)) : -1;
                removed = slot < 0 || slot >= slots || keep[slot] == 0;    // (fail closed: no verdict, no edge)
                if (removed) {
                    dst[e] = -1;
                    score[e] = -INFINITY;
                }
            }
        }
        const unsigned long long gone = __ballot(removed);
        if ((threadIdx.x & (MS_WAVE - 1)) == 0 && gone) atomicAdd(out_removed, (unsigned long long)__popcll(gone));
    }
}

// The set is located by its own head: a head that does not describe a set of n rows inside the workspace_bytes given finds nothing.
__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_pairs_find_kernel(
        const int64_t *__restrict__ a, const int64_t *__restrict__ b, int64_t cnt, const int32_t *__restrict__ lengths, int64_t n,
        const void *workspace, unsigned long long workspace_bytes, int64_t *out_slot) {
    const ms_cp_head *head = (const ms_cp_head *)workspace;
    const unsigned long long npos = head->npos;
    const bool sound = head->magic == MS_CP_MAGIC && head->n == n && npos >= 64 && npos <= (1ull << 32) && (npos & (npos - 1)) == 0 &&
                       MS_CP_HEAD_BYTES + 12 * npos <= workspace_bytes;
    const ms_cp_set set = ms_cp_carve(workspace, sound ? npos : 64);
    const long long cap = sound ? head->cap : 0;
    MS_CL_FOR_ENTRIES(cnt) {
        const int64_t e = base + threadIdx.x;
        if (e >= cnt) continue;
        const int64_t i = a[e], j = b[e];
        long long slot = -1;
        if (sound && i >= 0 && i < n && j >= 0 && j < n && i != j) {
            slot = ms_cp_lookup(set, ms_cp_key(i, lengths[i], j, lengths[j]));
            if (slot >= cap) slot = -1;                                    // (counted, never written)
        }
        out_slot[e] = slot;
    }
}

// The graph arguments of the three calls and the checks on them: those of ms_cluster_greedy_edges, in its order, then the range
// of n k + m and the workspace.
struct ms_cp_graph {
    const int64_t *nbr_idx;
    const float *nbr_score;
    int64_t n;
    int k;
    const int64_t *edge_src, *edge_dst;
    const float *edge_score;
    int64_t m;
    const int32_t *lengths;
    float min_score, mincov;
};

static int ms_cp_check_workspace(const char *who, int64_t n, int k, int64_t m, const void *workspace, size_t workspace_bytes) {
    const size_t need = ms_cluster_pairs_workspace_bytes(n, k, m);
    if (need == 0) MS_FAIL(MS_ERR_RANGE, "%s: n k + m = %lld directed entries, the set holds fewer than 2^31", who, (long long)(n * (int64_t)k + m));
    if (workspace_bytes < need)
        MS_FAIL(MS_ERR_WORKSPACE, "%s: workspace of %zu bytes, ms_cluster_pairs_workspace_bytes(%lld, %d, %lld) = %zu", who, workspace_bytes,
                (long long)n, k, (long long)m, need);
    if (((uintptr_t)workspace & 15u) != 0) MS_FAIL(MS_ERR_ARG, "%s: workspace must be 16-byte aligned", who);
    return MS_OK;
}

static int ms_cp_check_graph(const char *who, const ms_cp_graph &g, bool others_null, const void *workspace, size_t workspace_bytes) {
    if (g.k < 0 || g.m < 0) MS_FAIL(MS_ERR_ARG, "%s: need k >= 0 and m >= 0 (k=%d m=%lld)", who, g.k, (long long)g.m);
    if ((g.k > 0 && (!g.nbr_idx || !g.nbr_score)) || (g.m > 0 && (!g.edge_src || !g.edge_dst || !g.edge_score)) || !g.lengths || others_null ||
        !workspace)
        MS_FAIL(MS_ERR_ARG, "%s: NULL pointer", who);
    if (g.n < 1 || g.n > 2147483647LL) MS_FAIL(MS_ERR_ARG, "%s: need 1 <= n <= 2^31 - 1 (n=%lld)", who, (long long)g.n);
    if (g.min_score != g.min_score) MS_FAIL(MS_ERR_ARG, "%s: min_score is NaN (-inf: no cut)", who);
    if (!(g.mincov >= 0.0f && g.mincov <= 1.0f)) MS_FAIL(MS_ERR_ARG, "%s: mincov must lie in [0, 1]", who);
    if (g.m >= (1LL << 31) || g.n * (int64_t)g.k + g.m >= (1LL << 31))
        MS_FAIL(MS_ERR_RANGE, "%s: n k + m must stay below 2^31 directed entries (n=%lld k=%d m=%lld)", who, (long long)g.n, g.k, (long long)g.m);
    return ms_cp_check_workspace(who, g.n, g.k, g.m, workspace, workspace_bytes);
}

extern "C" int ms_cluster_pairs(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                                const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths, float min_score,
                                float mincov, int32_t *out_pairs, int64_t cap, int64_t *out_count, void *workspace,
                                size_t workspace_bytes, ms_stream_t stream) {
    const char *who = "ms_cluster_pairs";
    const ms_cp_graph g = {nbr_idx, nbr_score, n, k, edge_src, edge_dst, edge_score, m, lengths, min_score, mincov};
    if (cap < 0) MS_FAIL(MS_ERR_ARG, "%s: need cap >= 0 (cap=%lld)", who, (long long)cap);
    const int rc = ms_cp_check_graph(who, g, (cap > 0 && !out_pairs) || !out_count, workspace, workspace_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ms_cp_set set = ms_cp_carve(workspace, ms_cp_positions(n * (int64_t)k + m));
    unsigned long long *count = (unsigned long long *)out_count;
    hipLaunchKernelGGL(ms_cluster_pairs_init_kernel, dim3(ms_cl_blocks((int64_t)set.npos)), dim3(MS_CL_THREADS), 0, st, set, (long long)cap,
                       (long long)n, count);
    MS_LAUNCH_CHECK("ms_cluster_pairs_init_kernel");
    if (k > 0) {
        hipLaunchKernelGGL(ms_cluster_pairs_lists_kernel, dim3(ms_cl_blocks(n * MS_WAVE)), dim3(MS_CL_THREADS), 0, st, nbr_idx, nbr_score, n, k,
                           lengths, min_score, mincov, set, out_pairs, (long long)cap, count);
        MS_LAUNCH_CHECK("ms_cluster_pairs_lists_kernel");
    }
    if (m > 0) {
        const ms_cl_edges edges = {edge_src, edge_dst, edge_score, n, m};
        hipLaunchKernelGGL(ms_cluster_pairs_edges_kernel, dim3(ms_cl_blocks(m)), dim3(MS_CL_THREADS), 0, st, edges, lengths, min_score, mincov, set,
                           out_pairs, (long long)cap, count);
        MS_LAUNCH_CHECK("ms_cluster_pairs_edges_kernel");
    }
    return MS_OK;
}

extern "C" int ms_cluster_pairs_apply(int64_t *nbr_idx, float *nbr_score, int64_t n, int k, const int64_t *edge_src, int64_t *edge_dst,
                                      float *edge_score, int64_t m, const int32_t *lengths, float min_score, float mincov,
                                      const uint8_t *keep, int64_t count, const void *workspace, size_t workspace_bytes,
                                      int64_t *out_removed, ms_stream_t stream) {
    const char *who = "ms_cluster_pairs_apply";
    const ms_cp_graph g = {nbr_idx, nbr_score, n, k, edge_src, edge_dst, edge_score, m, lengths, min_score, mincov};
    if (count < 0) MS_FAIL(MS_ERR_ARG, "%s: need count >= 0 (count=%lld)", who, (long long)count);
    const int rc = ms_cp_check_graph(who, g, (count > 0 && !keep) || !out_removed, workspace, workspace_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ms_cp_set set = ms_cp_carve(workspace, ms_cp_positions(n * (int64_t)k + m));
    unsigned long long *removed = (unsigned long long *)out_removed;
    MS_HIP_CHECK(hipMemsetAsync(out_removed, 0, sizeof(int64_t), st));
    if (k > 0) {
        const ms_cl_lists lists = {nbr_idx, nbr_score, n, k};
        hipLaunchKernelGGL(ms_cluster_pairs_apply_kernel<ms_cl_lists>, dim3(ms_cl_blocks(n * (int64_t)k)), dim3(MS_CL_THREADS), 0, st, lists,
                           nbr_idx, nbr_score, lengths, min_score, mincov, set, keep, (long long)count, removed);
        MS_LAUNCH_CHECK("ms_cluster_pairs_apply_kernel<ms_cl_lists>");
    }
    if (m > 0) {
        const ms_cl_edges edges = {edge_src, edge_dst, edge_score, n, m};
        hipLaunchKernelGGL(ms_cluster_pairs_apply_kernel<ms_cl_edges>, dim3(ms_cl_blocks(m)), dim3(MS_CL_THREADS), 0, st, edges, edge_dst,
                           edge_score, lengths, min_score, mincov, set, keep, (long long)count, removed);
        MS_LAUNCH_CHECK("ms_cluster_pairs_apply_kernel<ms_cl_edges>");
    }
    return MS_OK;
}

extern "C" int ms_cluster_pairs_find(const int64_t *a, const int64_t *b, int64_t cnt, const int32_t *lengths, int64_t n, const void *workspace,
                                     size_t workspace_bytes, int64_t *out_slot, ms_stream_t stream) {
    const char *who = "ms_cluster_pairs_find";
    if (cnt < 0) MS_FAIL(MS_ERR_ARG, "%s: need cnt >= 0 (cnt=%lld)", who, (long long)cnt);
    if ((cnt > 0 && (!a || !b || !out_slot)) || !lengths || !workspace) MS_FAIL(MS_ERR_ARG, "%s: NULL pointer", who);
    if (n < 1 || n > 2147483647LL) MS_FAIL(MS_ERR_ARG, "%s: need 1 <= n <= 2^31 - 1 (n=%lld)", who, (long long)n);
    const int rc = ms_cp_check_workspace(who, n, 0, 0, workspace, workspace_bytes);        // (the smallest set there is; the head says more)
    if (rc) return rc;
    if (cnt == 0) return MS_OK;
    hipLaunchKernelGGL(ms_cluster_pairs_find_kernel, dim3(ms_cl_blocks(cnt)), dim3(MS_CL_THREADS), 0, (hipStream_t)stream, a, b, cnt, lengths, n,
                       workspace, (unsigned long long)workspace_bytes, out_slot);
    MS_LAUNCH_CHECK("ms_cluster_pairs_find_kernel");
    return MS_OK;
}
