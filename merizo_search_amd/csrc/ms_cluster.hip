// ms_cluster_greedy: greedy representative clustering of a database from its k-nearest-neighbour lists.
//
// The step behind a self-search (`db-search db db --exclude_self`) that makes a database non-redundant (DESIGN.md section
// 5.8): the representatives are the lexicographically-first maximal independent set of the undirected neighbour graph under
// the priority "longer domain first, smaller row on equal length" -- what cd-hit's sequential greedy pass yields -- and
// every other row goes to its best-scoring adjacent representative.
//
// The graph is never transposed.  An edge may be held by one endpoint's list only; the other endpoint learns of it by being
// WRITTEN TO.  A round is two launches ordered by the stream (the kernel boundary is the only cross-workgroup hand-off):
//   mark    one thread per list entry i->j, status read-only: an undecided i stores `blocked` into a lower-priority j (push) or
//           into itself when a higher-priority j is still undecided (pull); a new representative stores `covered` into its
//           neighbours, an undecided i into itself next to a representative.  All stores write the value 1: any order, any
//           multiplicity gives the same bytes.
//   decide  one thread per row: undecided + covered -> member; undecided, neither covered nor blocked -> representative;
//           its `blocked` byte is cleared for the next round; the rows still undecided are counted.
// The highest-priority undecided row is never blocked, so every round decides a row.  Decided rows skip their lists (a
// representative reads its list once more, the round after it was chosen, to cover its neighbours).
// Assignment runs once on the final set: 64-bit atomicMax on {order-preserving score bits, ~row}, pushed and pulled in the
// same way, so the result depends on the set alone.  Vector stores and vector atomics only; no LDS, no scratch.
// ms_cluster_greedy_edges adds m directed entries held as three arrays (row i, row j, score) to the lists: the mark and the
// assign step get a second launch over them, with i read instead of derived from the entry's place; ms_cluster_greedy is that
// call with m == 0 -- the launches it always made, in their order.
//
// How the file is laid out: where a directed entry comes from is an ENTRY SOURCE (ms_cl_lists, ms_cl_edges; they, the validity rule and
// the priority live in ms_cluster_entries.h, which ms_cluster_pairs.hip reads the same graph through), and every per-entry
// step -- mark and assign here, hook and link of ms_cluster_components below -- is ONE kernel template over the source, launched
// over the lists and then over the extras by MS_CL_LAUNCH_ENTRIES.  The three entry points share their argument checks
// (ms_cl_check_args), the host loop over the rounds (ms_cl_rounds) and the read-back behind the finish launch (ms_cl_read_head).
// Another way of reading the graph is another per-entry function.  (Those shared pieces, and the head and the score key, live in
// ms_cluster_rounds.h: ms_cluster_tree.hip runs its rounds through them too.)
#include "ms_cluster_rounds.h"

#define MS_CL_UNDECIDED 0
#define MS_CL_MEMBER 1
#define MS_CL_REP_NEW 2                // chosen by the last decide launch: covers its neighbours in the next mark launch
#define MS_CL_REP 3

struct ms_cl_view {                    // the workspace, carved (host and device)
    ms_cl_head *head;
    unsigned long long *best;          // [n] assignment key of a member
    uint8_t *status, *blocked, *covered, *cut;      // [n] each; cut: the row's list holds an entry that is not valid
};

static inline ms_cl_view ms_cl_carve(void *workspace, int64_t n) {
    char *p = (char *)workspace;
    ms_cl_view v;
    v.head = (ms_cl_head *)p;
    v.best = (unsigned long long *)(p + MS_CL_HEAD_BYTES);
    v.status = (uint8_t *)(p + MS_CL_HEAD_BYTES + 8 * (size_t)n);
    v.blocked = v.status + ms_cl_rows_bytes(n);
    v.covered = v.blocked + ms_cl_rows_bytes(n);
    v.cut = v.covered + ms_cl_rows_bytes(n);
    return v;
}

__device__ __forceinline__ bool ms_cl_is_rep(uint8_t st) { return st >= MS_CL_REP_NEW; }

// The mark step of ONE directed entry i -> j with score s (i inside [0, n)): what the header comment calls push, pull and cover.
__device__ __forceinline__ void ms_cl_mark_entry(int64_t i, const int64_t *__restrict__ jp, const float *__restrict__ sp, int64_t n,
                                                 const int32_t *__restrict__ lengths, float min_score, float mincov,
                                                 const uint8_t *__restrict__ status, uint8_t *blocked, uint8_t *covered) {
    const uint8_t st = status[i];
    if (st != MS_CL_UNDECIDED && st != MS_CL_REP_NEW) return;              // decided rows have nothing left to say
    const int64_t j = *jp;
    const float s = *sp;
    const int32_t li = lengths[i];
    int32_t lj;
    if (!ms_cl_valid(i, j, s, n, lengths, li, min_score, mincov, &lj)) return;
    if (st == MS_CL_REP_NEW) { covered[j] = 1; return; }
    const uint8_t sj = status[j];
    if (ms_cl_before(li, i, lj, j)) {
        if (sj == MS_CL_UNDECIDED) blocked[j] = 1;                         // push: j must wait for i
    } else if (sj == MS_CL_UNDECIDED) {
        blocked[i] = 1;                                                    // pull: i must wait for j
    } else if (ms_cl_is_rep(sj)) {
        covered[i] = 1;
    }
}

// (The launch over the extra entries runs between a round's list launch and its decide launch; with k == 0 it is the round's only
// mark launch, so it resets the count too: the same value, whichever launch stores it.)
template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_mark_kernel(
        const Src from, const int32_t *__restrict__ lengths, float min_score, float mincov, const uint8_t *__restrict__ status,
        uint8_t *blocked, uint8_t *covered, uint32_t *remaining_slot) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *remaining_slot = 0u;         // (this round's decide launch counts into it)
    MS_CL_FOR_ENTRIES(from.total()) {
        const int64_t i = from.row(base), e = base + threadIdx.x;
        if (i < 0) continue;
        ms_cl_mark_entry(i, from.dst + e, from.score + e, from.n, lengths, min_score, mincov, status, blocked, covered);
    }
}

__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_decide_kernel(int64_t n, uint8_t *status, uint8_t *blocked,
                                                                          const uint8_t *covered, uint32_t *remaining_slot) {
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t i = base + threadIdx.x;
        bool waits = false;
        if (i < n) {
            const uint8_t st = status[i];
            if (st == MS_CL_REP_NEW) {
                status[i] = MS_CL_REP;                                     // (it covered its neighbours in this round's mark launch)
            } else if (st == MS_CL_UNDECIDED) {
                const uint8_t b = blocked[i];
                if (b) blocked[i] = 0;
                if (covered[i]) status[i] = MS_CL_MEMBER;
                else if (!b) status[i] = MS_CL_REP_NEW;
                else waits = true;
            }
        }
        const unsigned long long m = __ballot(waits);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(remaining_slot, (uint32_t)__popcll(m));
    }
}

// The assignment step of ONE directed entry i -> j (i inside [0, n)); false: the entry is not valid.
__device__ __forceinline__ bool ms_cl_assign_entry(int64_t i, int64_t j, float s, int64_t n, const int32_t *__restrict__ lengths,
                                                   float min_score, float mincov, const uint8_t *__restrict__ status,
                                                   unsigned long long *best) {
    const int32_t li = lengths[i];
    int32_t lj;
    if (!ms_cl_valid(i, j, s, n, lengths, li, min_score, mincov, &lj)) return false;
    const bool rep_i = ms_cl_is_rep(status[i]), rep_j = ms_cl_is_rep(status[j]);
    if (rep_j && !rep_i) atomicMax(best + i, ms_cl_key(s, j));             // pull
    if (rep_i && !rep_j) atomicMax(best + j, ms_cl_key(s, i));             // push
    return true;
}

template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_assign_kernel(
        const Src from, const int32_t *__restrict__ lengths, float min_score, float mincov, const uint8_t *__restrict__ status,
        unsigned long long *best, uint8_t *cut) {
    MS_CL_FOR_ENTRIES(from.total()) {
        const int64_t i = from.row(base), e = base + threadIdx.x;
        if (i < 0) continue;
        if (!ms_cl_assign_entry(i, from.dst[e], from.score[e], from.n, lengths, min_score, mincov, status, best) && Src::owns_cut) cut[i] = 1;
    }
}

__global__ __launch_bounds__(MS_CL_THREADS) void ms_cluster_finish_kernel(int64_t n, const uint8_t *__restrict__ status,
                                                                          const unsigned long long *__restrict__ best,
                                                                          const uint8_t *__restrict__ cut, int64_t *out_rep,
                                                                          float *out_rep_score, ms_cl_head *head) {
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t i = base + threadIdx.x;
        bool rep = false, full = false;
        if (i < n) {
            rep = ms_cl_is_rep(status[i]);
            full = !cut[i];
            int64_t r = i;
            float s = 1.0f;
            if (!rep) {
                const unsigned long long key = best[i];
                const uint32_t b = (uint32_t)(key >> 32);
                r = key ? (int64_t)(~(uint32_t)key) : -1;                  // (a member always has an adjacent representative)
                s = key ? __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b) : -INFINITY;
            }
            out_rep[i] = r;
            out_rep_score[i] = s;
        }
        const unsigned long long mr = __ballot(rep), mf = __ballot(full);
        if ((threadIdx.x & 63) == 0) {
            if (mr) atomicAdd(&head->n_reps, (unsigned long long)__popcll(mr));
            if (mf) atomicAdd(&head->saturated, (unsigned long long)__popcll(mf));
        }
    }
}

extern "C" size_t ms_cluster_workspace_bytes(int64_t n) {
    if (n < 1 || n > 2147483647LL) return 0;
    return MS_CL_HEAD_BYTES + 8 * (size_t)n + 4 * ms_cl_rows_bytes(n);
}

// Both greedy entry points.
static int ms_cl_run(const char *who, bool lists_only, const ms_cl_args &a, ms_stream_t stream) {
    const int rc = ms_cl_check_args(who, lists_only, a, ms_cluster_workspace_bytes, "ms_cluster_workspace_bytes");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = a.lists.n;
    const ms_cl_view v = ms_cl_carve(a.workspace, n);
    const unsigned row_blocks = ms_cl_blocks(n);
    MS_HIP_CHECK(hipMemsetAsync(a.workspace, 0, ms_cluster_workspace_bytes(n), st));      // every row undecided, no flag, no key, counters 0

    int64_t rounds = 0;
    const int rr = ms_cl_rounds(
            n, v.head, st, rounds,
            [&](int g) -> int {
                MS_CL_LAUNCH_ENTRIES(ms_cluster_mark_kernel, a, true, st, a.lengths, a.min_score, a.mincov, v.status, v.blocked, v.covered,
                                     v.head->word + g);
                hipLaunchKernelGGL(ms_cluster_decide_kernel, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v.status, v.blocked, v.covered,
                                   v.head->word + g);
                MS_LAUNCH_CHECK("ms_cluster_decide_kernel");
                return MS_OK;
            },
            [&](uint32_t last, int64_t r) -> int {                         // (every round decides a row)
                MS_FAIL(MS_ERR_HIP, "%s: %lld rows still undecided after %lld rounds", who, (long long)last, (long long)r);
            });
    if (rr) return rr;

    MS_CL_LAUNCH_ENTRIES(ms_cluster_assign_kernel, a, false, st, a.lengths, a.min_score, a.mincov, v.status, v.best, v.cut);
    hipLaunchKernelGGL(ms_cluster_finish_kernel, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v.status, v.best, v.cut, a.out_rep,
                       a.out_score, v.head);
    MS_LAUNCH_CHECK("ms_cluster_finish_kernel");
    return ms_cl_read_head(v.head, a, rounds, st);
}

extern "C" int ms_cluster_greedy(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int32_t *lengths,
                                 float min_score, float mincov, int64_t *out_rep, float *out_rep_score, int64_t *out_n_reps,
                                 int32_t *out_rounds, int64_t *out_saturated, void *workspace, size_t workspace_bytes,
                                 ms_stream_t stream) {
    return ms_cl_run("ms_cluster_greedy", true,
                     {{nbr_idx, nbr_score, n, k}, {nullptr, nullptr, nullptr, n, 0}, lengths, min_score, mincov, out_rep, out_rep_score,
                      out_n_reps, out_rounds, out_saturated, workspace, workspace_bytes},
                     stream);
}

extern "C" int ms_cluster_greedy_edges(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                                       const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths,
                                       float min_score, float mincov, int64_t *out_rep, float *out_rep_score, int64_t *out_n_reps,
                                       int32_t *out_rounds, int64_t *out_saturated, void *workspace, size_t workspace_bytes,
                                       ms_stream_t stream) {
    return ms_cl_run("ms_cluster_greedy_edges", false,
                     {{nbr_idx, nbr_score, n, k}, {edge_src, edge_dst, edge_score, n, m}, lengths, min_score, mincov, out_rep, out_rep_score,
                      out_n_reps, out_rounds, out_saturated, workspace, workspace_bytes},
                     stream);
}

// ---------------------------------------------------------------------------------------------------------------------------
// ms_cluster_components: the connected components of the same graph (`cluster --cluster_mode connected`; DESIGN.md section 5.8,
// "Connected components").  Same entries, same validity test (ms_cl_valid), same two entry sources, same kernel-boundary-only
// hand-off; what differs is what is read off the graph.
//
// Every row has a 64-bit priority key {length, ~row}: the longer domain, then the smaller row, is the larger key (ms_cl_before).
// parent[n] holds the KEY of each row's parent (its own key: a root; the row is the key's low half), a forest in which a parent's key
// is at least its child's and every tree lies inside one component of the graph.  A round is
//   hook      one thread per entry i -> j (lists, then extras): a valid entry looks up the root keys of its endpoints by following
//             parent[]; when they differ it does a 64-bit atomicMax(parent[row of the lower key], higher key) and raises this round's
//             `changed` word.  (Many entries at one root: the highest key wins.)
//   compress  one thread per row: parent[i] = root key of i (no hook runs beside it: roots are fixed for the launch).
// Parents only rise and stay inside the row's component, so every value a racing read returns is the key of a row of the component at
// or above the reader, and following them ends, within n steps, at a row that read as its own parent.  A row that stopped being a
// root never is one again.  A hook whose lower root has meanwhile been hooked by another thread may replace that link by a higher
// one: nothing is lost for good, since every round looks at every entry again.  A round that raised `changed` saw the lower root as
// a root during the launch and left it none: every such round takes a root away, so at most n - 1 of them exist (n rounds in all).
// A round that did not raise it read every valid entry with both ends in one tree, on memory no one wrote: the trees are the
// components.  Their roots are the components' highest-priority rows (such a row is never the lower one) -- the REPRESENTATIVES,
// whatever the timing, and no pass has to pick them; the NUMBER of rounds is not fixed by the inputs (what a racing read returns
// decides how much one launch merges).
// Afterwards, once: a per-entry 32-bit atomicMax of the order-preserving score bits on link[i] and link[j] is the link score (the
// upper half of ms_cl_key); the finish launch writes the outputs and counts.  Vector loads, stores and atomics only; no LDS, no
// scratch.  (A first form kept 32-bit rows in parent[], hooked by row number and picked the representatives afterwards with an
// atomicMax on best[root]: on a 1M-row graph whose largest component has 443k rows that pass alone took 5.0 ms, every row of the
// component on one address; DESIGN.md has the trace.)
struct ms_cc_view {
    ms_cl_head *head;                  // word[]: the rounds' `changed` words
    unsigned long long *parent;        // [n] priority key of the row's parent
    uint32_t *link;                    // [n] order-preserving bits of the row's largest incident weight (0: none)
    uint8_t *cut;                      // [n] the row's list holds an entry that is not valid
};

static inline size_t ms_cc_words_bytes(int64_t n) { return ms_align_up(4 * (size_t)n, 16); }

static inline ms_cc_view ms_cc_carve(void *workspace, int64_t n) {
    char *p = (char *)workspace;
    ms_cc_view v;
    v.head = (ms_cl_head *)p;
    v.parent = (unsigned long long *)(p + MS_CL_HEAD_BYTES);
    v.link = (uint32_t *)(p + MS_CL_HEAD_BYTES + 8 * (size_t)n);
    v.cut = (uint8_t *)v.link + ms_cc_words_bytes(n);
    return v;
}

// {length, row} as one unsigned key: the longer domain wins, then the smaller row (ms_cl_before); distinct rows, distinct keys.
__device__ __forceinline__ unsigned long long ms_cc_priority_key(int32_t length, uint32_t row) {
    return ((unsigned long long)((uint32_t)length ^ 0x80000000u) << 32) | (unsigned long long)(~row);
}

__device__ __forceinline__ uint32_t ms_cc_key_row(unsigned long long key) { return ~(uint32_t)key; }

// A racing read of parent[]: relaxed, device scope (a vector load that does not trust this CU's cached copy).
__device__ __forceinline__ unsigned long long ms_cc_parent(const unsigned long long *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The key of the root above row x as this thread reads it: keys only rise along the way, so the walk ends.
__device__ __forceinline__ unsigned long long ms_cc_root(const unsigned long long *parent, uint32_t x) {
    for (;;) {
        const unsigned long long p = ms_cc_parent(parent, x);
        if (ms_cc_key_row(p) == x) return p;
        x = ms_cc_key_row(p);
    }
}

// The hook step of ONE directed entry i -> j with score s (i inside [0, n)); true: it saw two trees.
__device__ __forceinline__ bool ms_cc_hook_entry(int64_t i, int64_t j, float s, int64_t n, const int32_t *__restrict__ lengths,
                                                 float min_score, float mincov, unsigned long long *parent) {
    int32_t lj;
    if (!ms_cl_valid(i, j, s, n, lengths, lengths[i], min_score, mincov, &lj)) return false;
    const unsigned long long ki = ms_cc_root(parent, (uint32_t)i), kj = ms_cc_root(parent, (uint32_t)j);
    if (ki == kj) return false;
    const unsigned long long low = ki < kj ? ki : kj, high = ki < kj ? kj : ki;
    atomicMax(parent + ms_cc_key_row(low), high);
    return true;
}

__global__ __launch_bounds__(MS_CL_THREADS) void ms_components_init_kernel(int64_t n, const int32_t *__restrict__ lengths,
                                                                           unsigned long long *parent) {
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t i = base + threadIdx.x;
        if (i < n) parent[i] = ms_cc_priority_key(lengths[i], (uint32_t)i);
    }
}

template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_components_hook_kernel(
        const Src from, const int32_t *__restrict__ lengths, float min_score, float mincov, unsigned long long *parent, uint32_t *changed_slot) {
    MS_CL_FOR_ENTRIES(from.total()) {
        const int64_t i = from.row(base), e = base + threadIdx.x;
        const bool saw = i >= 0 && ms_cc_hook_entry(i, from.dst[e], from.score[e], from.n, lengths, min_score, mincov, parent);
        // (the ballot is every lane's, the ones without an entry too; the value 1 from every wave that stores)
        if (__ballot(saw) && (threadIdx.x & 63) == 0) *changed_slot = 1u;
    }
}

__global__ __launch_bounds__(MS_CL_THREADS) void ms_components_compress_kernel(int64_t n, unsigned long long *parent) {
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t i = base + threadIdx.x;
        if (i >= n) continue;
        const unsigned long long p = ms_cc_parent(parent, (uint32_t)i);
        if (ms_cc_key_row(p) == (uint32_t)i) continue;
        const unsigned long long r = ms_cc_root(parent, ms_cc_key_row(p));
        if (r != p) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The link step of ONE directed entry i -> j (i inside [0, n)); false: the entry is not valid.
__device__ __forceinline__ bool ms_cc_link_entry(int64_t i, int64_t j, float s, int64_t n, const int32_t *__restrict__ lengths,
                                                 float min_score, float mincov, uint32_t *link) {
    int32_t lj;
    if (!ms_cl_valid(i, j, s, n, lengths, lengths[i], min_score, mincov, &lj)) return false;
    const uint32_t b = (uint32_t)(ms_cl_key(s, 0) >> 32);
    atomicMax(link + i, b);
    atomicMax(link + j, b);
    return true;
}

template <typename Src>
__global__ __launch_bounds__(MS_CL_THREADS) void ms_components_link_kernel(
        const Src from, const int32_t *__restrict__ lengths, float min_score, float mincov, uint32_t *link, uint8_t *cut) {
    MS_CL_FOR_ENTRIES(from.total()) {
        const int64_t i = from.row(base), e = base + threadIdx.x;
        if (i < 0) continue;
        if (!ms_cc_link_entry(i, from.dst[e], from.score[e], from.n, lengths, min_score, mincov, link) && Src::owns_cut) cut[i] = 1;
    }
}

__global__ __launch_bounds__(MS_CL_THREADS) void ms_components_finish_kernel(int64_t n, const unsigned long long *__restrict__ parent,
                                                                             const uint32_t *__restrict__ link, const uint8_t *__restrict__ cut,
                                                                             int64_t *out_rep, float *out_link_score, ms_cl_head *head) {
    for (int64_t base = (int64_t)blockIdx.x * MS_CL_THREADS; base < n; base += (int64_t)gridDim.x * MS_CL_THREADS) {
        const int64_t i = base + threadIdx.x;
        bool rep = false, full = false;
        if (i < n) {
            const int64_t r = (int64_t)ms_cc_key_row(parent[i]);           // (compressed: its root, the component's highest-priority row)
            rep = r == i;
            full = !cut[i];
            const uint32_t b = link[i];                                    // (a row that is no representative has a valid entry)
            out_rep[i] = r;
            out_link_score[i] = rep ? 1.0f : b ? __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b) : -INFINITY;
        }
        const unsigned long long mr = __ballot(rep), mf = __ballot(full);
        if ((threadIdx.x & 63) == 0) {
            if (mr) atomicAdd(&head->n_reps, (unsigned long long)__popcll(mr));
            if (mf) atomicAdd(&head->saturated, (unsigned long long)__popcll(mf));
        }
    }
}

extern "C" size_t ms_cluster_components_workspace_bytes(int64_t n) {
    if (n < 1 || n > 2147483647LL) return 0;
    return MS_CL_HEAD_BYTES + 8 * (size_t)n + ms_cc_words_bytes(n) + ms_cl_rows_bytes(n);
}

extern "C" int ms_cluster_components(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                                     const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths, float min_score,
                                     float mincov, int64_t *out_rep, float *out_link_score, int64_t *out_n_components, int32_t *out_rounds,
                                     int64_t *out_saturated, void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    const ms_cl_args a = {{nbr_idx, nbr_score, n, k}, {edge_src, edge_dst, edge_score, n, m}, lengths, min_score, mincov, out_rep, out_link_score,
                          out_n_components, out_rounds, out_saturated, workspace, workspace_bytes};
    const int rc = ms_cl_check_args("ms_cluster_components", false, a, ms_cluster_components_workspace_bytes, "ms_cluster_components_workspace_bytes");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ms_cc_view v = ms_cc_carve(workspace, n);
    const unsigned row_blocks = ms_cl_blocks(n);
    MS_HIP_CHECK(hipMemsetAsync(workspace, 0, ms_cluster_components_workspace_bytes(n), st));      // no link, no flag, counters 0
    hipLaunchKernelGGL(ms_components_init_kernel, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, lengths, v.parent);
    MS_LAUNCH_CHECK("ms_components_init_kernel");

    int64_t rounds = 0;
    const int rr = ms_cl_rounds(
            n, v.head, st, rounds,
            [&](int g) -> int {
                // (no launch of a round resets its word, as the greedy mark launch does: a memset per group behind the first)
                if (g == 0 && rounds > 0) MS_HIP_CHECK(hipMemsetAsync(v.head->word, 0, sizeof(v.head->word), st));
                MS_CL_LAUNCH_ENTRIES(ms_components_hook_kernel, a, false, st, lengths, min_score, mincov, v.parent, v.head->word + g);
                hipLaunchKernelGGL(ms_components_compress_kernel, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v.parent);
                MS_LAUNCH_CHECK("ms_components_compress_kernel");
                return MS_OK;
            },
            [&](uint32_t, int64_t r) -> int {                              // (every round that saw two trees took a root away)
                MS_FAIL(MS_ERR_HIP, "ms_cluster_components: trees still merging after %lld rounds", (long long)r);
            });
    if (rr) return rr;

    MS_CL_LAUNCH_ENTRIES(ms_components_link_kernel, a, false, st, lengths, min_score, mincov, v.link, v.cut);
    hipLaunchKernelGGL(ms_components_finish_kernel, dim3(row_blocks), dim3(MS_CL_THREADS), 0, st, n, v.parent, v.link, v.cut, out_rep,
                       out_link_score, v.head);
    MS_LAUNCH_CHECK("ms_components_finish_kernel");
    return ms_cl_read_head(v.head, a, rounds, st);
}
