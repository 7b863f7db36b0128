// ms_cluster_tree: the single-linkage tree of the cluster graph -- its maximum spanning forest under a strict edge order -- by
// Boruvka rounds (`cluster --tree / --levels`; DESIGN.md section 5.8, "The single-linkage tree").
//
// Same entries, same validity test (ms_cl_valid), same two entry sources and the same host loop as ms_cluster_components
// (ms_cluster_rounds.h).  The undirected edges are ordered STRICTLY: weight descending (the larger of the valid directed scores, -0.0
// as +0.0: the upper half of ms_cl_key), then (min(i,j), max(i,j)) ascending.  The forest is the one Kruskal builds in that order.
//
// State: parent[n] (32-bit rows, FULLY compressed at a round's start: parent[x] is the root of x), and per ROOT bestw[n] (the largest
// order-preserving weight bits among the entries that leave the tree, 0: none) and bestpair[n] ((min << 32) | max of the first such
// edge in the order, ~0: none).  A round is a sequence of launches; the kernel boundary is the only hand-off, and no launch reads a
// word that another thread writes in the same launch, except through the atomics' own monotone slots:
//   weight   one thread per entry (lists, then extras): a valid entry whose ends have different roots does atomicMax(bestw[root],
//            bits) at both roots and raises this round's `changed` word (ballot, one store per wave).
//   pair     the same pass: an entry whose bits equal bestw[root] does a 64-bit atomicMin(bestpair[root], pair).  After it every tree
//            with an entry to another tree holds its FIRST outgoing edge in the order: an edge of the forest (the cut property; the
//            order is strict, so there is one such forest).
//   hook     one thread per row: a root r with a selection finds the other root r' = parent[the pair's end outside r].  When r'
//            selected the SAME pair, the root with the LARGER row hooks and the smaller one stays a root; otherwise r hooks.  A root
//            that hooks writes next[r] = r' and its own output slot r = {pair, weight}; every other row writes next[x] = parent[x].
//            Selections strictly rise along a chain of hooks r -> r' -> r'' (r' prefers its own selection to r's), so the only cycle
//            is the mutual pair, which the rule breaks: next[] is a forest over the old roots.
//   jump     pointer jumping from one buffer into another: out[x] = the MS_TREE_STEPS-th ancestor of x in in[] (or the root when it
//            is nearer).  A tree that selected has merged in every round so far, so at round r it holds at least 2^(r-1) rows: at
//            most n >> (r-1) trees select, no chain of next[] is longer than that, and ceil(log_STEPS) launches -- a number the host
//            knows without a read-back -- leave every row at its root.  The last of them writes parent[] and resets the row's own
//            bestw / bestpair slot for the next round.
// The same count ends it: a tree that still selects at round r needs a second one beside it, 2^r <= n, so the first round without an
// entry between two trees is at most floor(log2 n) + 1 -- *out_rounds, a function of the entry set alone.  The launches of a round
// behind that one (the rest of its group of MS_CL_GROUP) look at the `changed` words and return at once.
//
// Hot addresses: in late rounds one root receives every entry that leaves a large tree.  (a) Before an atomic a relaxed device-scope
// load of the slot skips it when it cannot win -- the slots only rise (bestw) or only fall (bestpair) within a launch, so a stale
// read errs towards issuing the atomic; (b) a lane whose predecessor in the wave targets the same root with a value at least as good
// leaves the atomic to it: a row's k entries are adjacent and sorted, so of a list's k atomics on the row's own root one is issued.
// Vector loads, stores and atomics only; no LDS, no scratch.
#include "ms_cluster_rounds.h"

#define MS_TREE_STEPS 16               // ancestors one jump launch walks: ceil(log16(chain)) launches per round
#define MS_TREE_NO_PAIR (~0ull)
#define MS_TREE_FINISH_BLOCKS 512u     // workgroups of the finish launch (two per CU): 2,048 waves, two atomics each

struct ms_tree_view {
    ms_cl_head *head;                  // word[]: the rounds' `changed` words; n_reps: the roots left (components)
    unsigned long long *bestpair;      // [n] per root: (min << 32) | max of its first outgoing edge
    uint32_t *parent;                  // [n] the root of the row (compressed between rounds)
    uint32_t *next[2];                 // [n] each: the hook targets, and the buffers the jumps alternate between
    uint32_t *bestw;                   // [n] per root: order-preserving bits of its largest outgoing weight (0: none)
    uint8_t *cut;                      // [n] the row's list holds an entry that is not valid
};

static inline size_t ms_tree_words_bytes(int64_t n) { return ms_align_up(4 * (size_t)n, 16); }

static inline ms_tree_view ms_tree_carve(void *workspace, int64_t n) {
    char *p = (char *)workspace;
    const size_t words = ms_tree_words_bytes(n);
    ms_tree_view v;
    v.head = (ms_cl_head *)p;
    v.bestpair = (unsigned long long *)(p + MS_CL_HEAD_BYTES);
    char *w = p + MS_CL_HEAD_BYTES + ms_align_up(8 * (size_t)n, 16);
    v.parent = (uint32_t *)w;
    v.next[0] = (uint32_t *)(w + words);
    v.next[1] = (uint32_t *)(w + 2 * words);
    v.bestw = (uint32_t *)(w + 3 * words);
    v.cut = (uint8_t *)(w + 4 * words);
    return v;
}

__global__ __launch_bounds__(MS_CL_THREADS) void ms_tree_init_kernel(int64_t n, ms_tree_view v, int32_t *out_pairs, float *out_weight) {
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t x = base + threadIdx.x;
        if (x >= n) continue;
        v.parent[x] = (uint32_t)x;
        v.bestw[x] = 0u;
        v.bestpair[x] = MS_TREE_NO_PAIR;
        v.cut[x] = 0;
        out_pairs[2 * x] = -1;                                             // a row that never hooks keeps these
        out_pairs[2 * x + 1] = -1;
        out_weight[x] = -INFINITY;
    }
}

// One entry of a select pass: valid and between two trees (`cross`), with the roots of its ends, its weight bits and its pair.
struct ms_tree_entry {
    bool cross;
    uint32_t ri, rj, bits;
    unsigned long long pair;
};

template <bool FIRST, typename Src>
__device__ __forceinline__ ms_tree_entry ms_tree_read_entry(const Src &from, int64_t base, const int32_t *__restrict__ lengths, float min_score,
                                                            float mincov, const uint32_t *__restrict__ parent, uint8_t *cut) {
    ms_tree_entry t = {false, 0u, 0u, 0u, MS_TREE_NO_PAIR};
    const int64_t i = from.row(base), e = base + threadIdx.x;
    if (i < 0) return t;
    const int64_t j = from.dst[e];
    const float s = from.score[e];
    int32_t lj;
    if (!ms_cl_valid(i, j, s, from.n, lengths, lengths[i], min_score, mincov, &lj)) {
        if (FIRST && Src::owns_cut) cut[i] = 1;
        return t;
    }
    t.ri = parent[i];
    t.rj = parent[j];
    t.cross = t.ri != t.rj;
    t.bits = (uint32_t)(ms_cl_key(s, 0) >> 32);
    const uint32_t a = (uint32_t)(i < j ? i : j), b = (uint32_t)(i < j ? j : i);
    t.pair = ((unsigned long long)a << 32) | (unsigned long long)b;
    return t;
}

// atomicMax / atomicMin behind a look at the slot: it only rises / only falls within the launch, so a value that cannot win now
// never can (relaxed, device scope: a vector load that does not trust this CU's cached copy).
__device__ __forceinline__ void ms_tree_raise(uint32_t *slot, uint32_t bits) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(slot, bits);
}

__device__ __forceinline__ void ms_tree_lower(unsigned long long *slot, unsigned long long pair) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pair) atomicMin(slot, pair);
}

// The weight step.  prev: the `changed` word of the round before, in the same group (NULL: the group's first round) -- zero: that
// round was the last, nothing is left to do.  FIRST: the call's first round, which also marks the lists that hold an invalid entry.
template <bool FIRST, typename Src>
__device__ __forceinline__ void ms_tree_weight_pass(const Src &from, const int32_t *__restrict__ lengths, float min_score, float mincov,
                                                    const uint32_t *__restrict__ parent, uint32_t *bestw, uint8_t *cut,
                                                    const uint32_t *prev, uint32_t *changed_slot) {
    if (prev && *prev == 0u) return;
    const int lane = threadIdx.x & 63;
    MS_CL_FOR_ENTRIES(from.total()) {
        const ms_tree_entry t = ms_tree_read_entry<FIRST>(from, base, lengths, min_score, mincov, parent, cut);
        // (every lane of the wave is here: the shuffles and the ballot are the whole wave's)
        const uint32_t up_root = __shfl_up(t.ri, 1), up_bits = __shfl_up(t.bits, 1);
        const int up_cross = __shfl_up((int)t.cross, 1);
        const bool left_to_neighbour = lane > 0 && up_cross && up_root == t.ri && up_bits >= t.bits;
        if (t.cross) {
            if (!left_to_neighbour) ms_tree_raise(bestw + t.ri, t.bits);
            ms_tree_raise(bestw + t.rj, t.bits);
        }
        if (__ballot(t.cross) && lane == 0) *changed_slot = 1u;            // (the value 1 from every wave that stores)
    }
}

template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_tree_weight_first_kernel(
        const Src from, const int32_t *__restrict__ lengths, float min_score, float mincov, const uint32_t *__restrict__ parent,
        uint32_t *bestw, uint8_t *cut, const uint32_t *prev, uint32_t *changed_slot) {
    ms_tree_weight_pass<true>(from, lengths, min_score, mincov, parent, bestw, cut, prev, changed_slot);
}

template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_tree_weight_kernel(
        const Src from, const int32_t *__restrict__ lengths, float min_score, float mincov, const uint32_t *__restrict__ parent,
        uint32_t *bestw, uint8_t *cut, const uint32_t *prev, uint32_t *changed_slot) {
    ms_tree_weight_pass<false>(from, lengths, min_score, mincov, parent, bestw, cut, prev, changed_slot);
}

// The pair step: bestw[] is final (the weight launches are behind a kernel boundary) and read-only here.
template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_tree_pair_kernel(
        const Src from, const int32_t *__restrict__ lengths, float min_score, float mincov, const uint32_t *__restrict__ parent,
        const uint32_t *__restrict__ bestw, unsigned long long *bestpair, const uint32_t *changed_slot) {
    if (*changed_slot == 0u) return;                                       // (this round's weight launches saw one forest per component)
    const int lane = threadIdx.x & 63;
    MS_CL_FOR_ENTRIES(from.total()) {
        const ms_tree_entry t = ms_tree_read_entry<false>(from, base, lengths, min_score, mincov, parent, (uint8_t *)nullptr);
        const bool hit_i = t.cross && bestw[t.ri] == t.bits, hit_j = t.cross && bestw[t.rj] == t.bits;
        const uint32_t up_root = __shfl_up(t.ri, 1);
        const unsigned long long up_pair = __shfl_up(t.pair, 1);
        const int up_hit = __shfl_up((int)hit_i, 1);
        const bool left_to_neighbour = lane > 0 && up_hit && up_root == t.ri && up_pair <= t.pair;
        if (hit_i && !left_to_neighbour) ms_tree_lower(bestpair + t.ri, t.pair);
        if (hit_j) ms_tree_lower(bestpair + t.rj, t.pair);
    }
}

// The hook step.  Reads parent[], bestw[], bestpair[] (no thread of this launch writes them); writes next[] and the outputs.
__global__ __launch_bounds__(MS_CL_THREADS) void ms_tree_hook_kernel(int64_t n, const uint32_t *__restrict__ parent,
                                                                     const uint32_t *__restrict__ bestw,
                                                                     const unsigned long long *__restrict__ bestpair, uint32_t *next,
                                                                     int32_t *out_pairs, float *out_weight, const uint32_t *changed_slot) {
    if (*changed_slot == 0u) return;
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t x = base + threadIdx.x;
        if (x >= n) continue;
        const uint32_t p = parent[x];
        uint32_t to = p;
        const uint32_t w = p == (uint32_t)x ? bestw[x] : 0u;
        const unsigned long long pair = w ? bestpair[x] : MS_TREE_NO_PAIR;
        if (pair != MS_TREE_NO_PAIR) {                                     // (a weight without a pair cannot be: no row is read with one)
            const uint32_t a = (uint32_t)(pair >> 32), b = (uint32_t)pair;
            const uint32_t ra = parent[a], rb = parent[b];
            const uint32_t other = ra == (uint32_t)x ? rb : ra;
            const bool stays = bestpair[other] == pair && (uint32_t)x < other;      // the mutual pair: the smaller root stays
            if (!stays) {
                to = other;
                out_pairs[2 * x] = (int32_t)a;
                out_pairs[2 * x + 1] = (int32_t)b;
                out_weight[x] = ms_cl_key_score(w);
            }
        }
        next[x] = to;
    }
}

// One jump launch: out[x] = the MS_TREE_STEPS-th ancestor of x in in[], or its root.  LAST: `out` is parent[], and the row's own
// selection slots are reset for the next round.
template <bool LAST>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_tree_jump_kernel(int64_t n, const uint32_t *__restrict__ in, uint32_t *out, uint32_t *bestw,
                                                                     unsigned long long *bestpair, const uint32_t *changed_slot) {
    if (*changed_slot == 0u) return;
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t x = base + threadIdx.x;
        if (x >= n) continue;
        uint32_t y = in[x];
        for (int s = 1; s < MS_TREE_STEPS; ++s) {
            const uint32_t z = in[y];
            if (z == y) break;
            y = z;
        }
        out[x] = y;
        if (LAST && bestw[x]) {
            bestw[x] = 0u;
            bestpair[x] = MS_TREE_NO_PAIR;
        }
    }
}

__global__ __launch_bounds__(MS_CL_THREADS) void ms_tree_finish_kernel(int64_t n, const uint32_t *__restrict__ parent,
                                                                       const uint8_t *__restrict__ cut, ms_cl_head *head) {
    // (MS_TREE_FINISH_BLOCKS workgroups stride over the rows and every wave adds its two counts ONCE: one wave-atomic per 64 rows on
    // two addresses cost ms_components_finish_kernel 190 us at 1M rows)
    unsigned long long roots = 0, fulls = 0;
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t x = base + threadIdx.x;
        const bool root = x < n && parent[x] == (uint32_t)x, full = x < n && !cut[x];
        roots += (unsigned long long)__popcll(__ballot(root));
        fulls += (unsigned long long)__popcll(__ballot(full));
    }
    if ((threadIdx.x & 63) == 0) {
        if (roots) atomicAdd(&head->n_reps, roots);
        if (fulls) atomicAdd(&head->saturated, fulls);
    }
}

extern "C" size_t ms_cluster_tree_workspace_bytes(int64_t n) {
    if (n < 1 || n > 2147483647LL) return 0;
    return MS_CL_HEAD_BYTES + ms_align_up(8 * (size_t)n, 16) + 4 * ms_tree_words_bytes(n) + ms_cl_rows_bytes(n);
}

// Jump launches of round r (1-based): at most n >> (r - 1) trees select, so no chain of next[] is longer than that.
static inline int ms_tree_jumps(int64_t n, int64_t r) {
    const int64_t chain = r > 32 ? 1 : (n >> (r - 1)) > 1 ? (n >> (r - 1)) : 1;
    int jumps = 1;
    for (int64_t reach = MS_TREE_STEPS; reach < chain; reach *= MS_TREE_STEPS) ++jumps;
    return jumps;
}

extern "C" int ms_cluster_tree(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                               const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths, float min_score,
                               float mincov, int32_t *out_pairs, float *out_weight, int64_t *out_n_edges, int32_t *out_rounds,
                               int64_t *out_saturated, void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    // (out_pairs stands where the other calls have out_rep: the shared checks only compare it with NULL)
    const ms_cl_args a = {{nbr_idx, nbr_score, n, k}, {edge_src, edge_dst, edge_score, n, m}, lengths, min_score, mincov, (int64_t *)out_pairs,
                          out_weight, out_n_edges, out_rounds, out_saturated, workspace, workspace_bytes};
    const int rc = ms_cl_check_args("ms_cluster_tree", false, a, ms_cluster_tree_workspace_bytes, "ms_cluster_tree_workspace_bytes");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ms_tree_view v = ms_tree_carve(workspace, n);
    const unsigned row_blocks = ms_cl_blocks(n);
    MS_HIP_CHECK(hipMemsetAsync(v.head, 0, MS_CL_HEAD_BYTES, st));                                  // words and counters 0
    hipLaunchKernelGGL(ms_tree_init_kernel, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v, out_pairs, out_weight);
    MS_LAUNCH_CHECK("ms_tree_init_kernel");

    int64_t rounds = 0;
    const int rr = ms_cl_rounds(
            n, v.head, st, rounds,
            [&](int g) -> int {
                if (g == 0 && rounds > 0) MS_HIP_CHECK(hipMemsetAsync(v.head->word, 0, sizeof(v.head->word), st));
                uint32_t *changed = v.head->word + g;
                const uint32_t *prev = g > 0 ? changed - 1 : nullptr;
                if (rounds == 0 && g == 0)
                    MS_CL_LAUNCH_ENTRIES(ms_tree_weight_first_kernel, a, false, st, lengths, min_score, mincov, v.parent, v.bestw, v.cut, prev, changed);
                else
                    MS_CL_LAUNCH_ENTRIES(ms_tree_weight_kernel, a, false, st, lengths, min_score, mincov, v.parent, v.bestw, v.cut, prev, changed);
                MS_CL_LAUNCH_ENTRIES(ms_tree_pair_kernel, a, false, st, lengths, min_score, mincov, v.parent, v.bestw, v.bestpair, changed);
                hipLaunchKernelGGL(ms_tree_hook_kernel, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v.parent, v.bestw, v.bestpair,
                                   v.next[0], out_pairs, out_weight, changed);
                MS_LAUNCH_CHECK("ms_tree_hook_kernel");
                const int jumps = ms_tree_jumps(n, rounds + g + 1);
                for (int j = 0; j + 1 < jumps; ++j) {
                    hipLaunchKernelGGL(ms_tree_jump_kernel<false>, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v.next[j & 1],
                                       v.next[(j + 1) & 1], v.bestw, v.bestpair, changed);
                    MS_LAUNCH_CHECK("ms_tree_jump_kernel<false>");
                }
                hipLaunchKernelGGL(ms_tree_jump_kernel<true>, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v.next[(jumps - 1) & 1], v.parent,
                                   v.bestw, v.bestpair, changed);
                MS_LAUNCH_CHECK("ms_tree_jump_kernel<true>");
                return MS_OK;
            },
            [&](uint32_t, int64_t r) -> int {                              // (floor(log2 n) + 1 rounds at the most)
                MS_FAIL(MS_ERR_HIP, "ms_cluster_tree: trees still merging after %lld rounds", (long long)r);
            });
    if (rr) return rr;

    hipLaunchKernelGGL(ms_tree_finish_kernel, dim3(row_blocks < MS_TREE_FINISH_BLOCKS ? row_blocks : MS_TREE_FINISH_BLOCKS), dim3(MS_CL_THREADS),
                       0, st, n, v.parent, v.cut, v.head);
    MS_LAUNCH_CHECK("ms_tree_finish_kernel");
    const int rh = ms_cl_read_head(v.head, a, rounds, st);
    if (rh) return rh;
    *out_n_edges = n - *out_n_edges;                                       // (the head counts the roots left: the components)
    return MS_OK;
}
