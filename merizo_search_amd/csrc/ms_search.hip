// Brute-force cosine / inner-product top-k over the 128-d domain-embedding database on gfx950.
//
// Reference arithmetic replaced (programs/Foldclass/dbsearch.py):
//   :75-81   search_query_against_db   cosine_similarity(db, q) * mask -> topk   (`.pt` DB)
//   :213-248 knn_exact_faiss           IndexFlat(IP).search per block + ResultHeap merge
//   :303-304 F.normalize(query_embeddings)
//
// This file: normalisation kernels, the launch plan (row streams x query tiles, workspace carve), the two merges of
// per-stream lists and the C entry points.  The scan kernels themselves live in ms_scan.h (instantiated per list
// length in ms_scan_kl*.hip):
//   ms_scan_loader_kernel<KL,AUXM,SAMPLE>  >= 3 query tiles (MFMA-bound), k <= 64, all modes: 4 compute waves share the rows
//                                          a fifth wave streams into an LDS ring by LDS-DMA; SAMPLE = its sample pass
//   ms_scan_kernel<KL,AUX,UB>              1-2 query tiles (HBM-bound), and passes with an upper bound (k > 64)
//   ms_scan_sample_kernel<KL,AUX>          sample pass of the latter: best scores of the first tiles of every stream
// Common to all of them: one wave = one (32-query tile, row stream) pair; the query tile is the MFMA B
// operand in 64 VGPRs for the whole kernel; 32-row tiles arrive by LDS-DMA in an image whose lane = row ds_read_b128
// A-fragment reads are conflict free; k-step s of the v_mfma_f32_32x32x2_f32 chain multiplies
// elements k = s (lanes 0-31) and k = 64 + s (lanes 32-63), i.e. the accumulation order is s = 0..63: (k = s, k = 64 + s)
// -- restated by oracle/oracle.c:dot_ordered(order = 1), which reproduces the scores bit for bit; the running top-k of a
// query lives in the registers of its two lanes; rows are visited in ascending order, so "strictly greater than the k-th
// best" is the exact (score desc, row asc) order.
//
// Kernels here
//   ms_normalize_rows_kernel / ms_row_inv_norms_kernel / ms_prepare_queries_kernel   one wave per 512-byte row
//   ms_block_merge_kernel     per query, one workgroup: threshold = k-th best list head, the few entries at or above it rank
//                             themselves (ms_common.h: ms_block_merge); the usual final merge
//   ms_sample_bound_kernel    per query: k-th largest of the sample pass's maxima = lower bound of the full pass
//   ms_head_merge_kernel      per query: k rounds of "best list head wins" over the per-stream lists staged in LDS (shapes the
//                             block merge declines, and more than 256 lists)
//   ms_partial_merge_kernel   the same merge for large k * P (does not fit LDS): threshold from the list heads + pool
//   ms_kway_merge_kernel      public merge of S sorted lists (shards after the all-gather, blocks when streaming);
//                             ms_kway_merge_any_kernel beyond 64 lists
#include "ms_common.h"
#include "ms_wsstate.h"

#include <math.h>
#include <stdlib.h>

thread_local char ms_err_buf[512] = "";

// ------------------------------------------------------------------ normalisation ------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(256) void ms_normalize_rows_kernel(const float *x, float *y, int64_t n, float eps) {   // y may be x
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave0; r < n; r += nwaves) {
        float2 v = *(reinterpret_cast<const float2 *>(x + r * MS_DIM) + lane);
        const float ss = wave_sum(v.x * v.x + v.y * v.y);
        const float nrm = fmaxf(sqrtf(ss), eps);
        v.x = v.x / nrm;
        v.y = v.y / nrm;
        *(reinterpret_cast<float2 *>(y + r * MS_DIM) + lane) = v;
    }
}

__global__ __launch_bounds__(256) void ms_row_inv_norms_kernel(const float *x, int64_t n, float eps, float *inv) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave0; r < n; r += nwaves) {
        const float2 v = *(reinterpret_cast<const float2 *>(x + r * MS_DIM) + lane);
        const float ss = wave_sum(v.x * v.x + v.y * v.y);
        if (lane == 0) inv[r] = 1.0f / fmaxf(sqrtf(ss), eps);
    }
}

// Queries -> zero-padded [nq_pad,128] copy, optionally L2-normalised (cosine mode, eps 1e-8).
__global__ __launch_bounds__(256) void ms_prepare_queries_kernel(const float *q, int nq, int nq_pad, int normalize,
                                                                 float eps, float *qn) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq_pad) return;
    float2 v = make_float2(0.0f, 0.0f);
    if (row < nq) {
        v = *(reinterpret_cast<const float2 *>(q + (size_t)row * MS_DIM) + lane);
        if (normalize) {
            const float ss = wave_sum(v.x * v.x + v.y * v.y);
            const float nrm = fmaxf(sqrtf(ss), eps);
            v.x = v.x / nrm;
            v.y = v.y / nrm;
        }
    }
    *(reinterpret_cast<float2 *>(qn + (size_t)row * MS_DIM) + lane) = v;
}

// The one mapping from a search mode to the preparation of its queries (ms_common.h): the scan's own launch, and what
// ms_md_chain_scores (ms_multidom.hip) scores its cells with.
int ms_launch_prepare_queries(const float *q, int nq, int nq_pad, int mode, float *qn, hipStream_t st) {
    hipLaunchKernelGGL(ms_prepare_queries_kernel, dim3((nq_pad + 3) / 4), dim3(256), 0, st, q, nq, nq_pad,
                       mode != MS_MODE_IP_PRENORM ? 1 : 0, mode == MS_MODE_IP_NORMQ ? 1e-12f : 1e-8f, qn);
    MS_LAUNCH_CHECK("ms_prepare_queries_kernel");
    return MS_OK;
}

#include "ms_scan.h"
#include "ms_scan_pf.h"
#include "ms_scan_pf16.h"

// ------------------------------------------------------------------ partial merge ------
// One workgroup per query merges its P partial lists (each sorted best-first, rank-major
// layout [k][P]) into the final top-k:
//   1. the k-th best of the P list HEADS (k rounds of a block-wide arg-max) is a lower bound
//      of the answer in the total order (score desc, row asc);
//   2. only entries at least that good can matter -- a sorted prefix of at most k lists, at
//      most k*k entries in all -- they are appended to an LDS pool;
//   3. one wave inserts the pool into a sorted k-list (ms_wave_insert) and writes float32 /
//      int64 results (+ the exclusive bound of the next pass when k > 64).
constexpr int MERGE_MAX_P = 1024;
__global__ __launch_bounds__(256) void ms_partial_merge_kernel(const float *part_s, const uint32_t *part_i, int P,
                                                              int k, int64_t row_offset, float *out_s, int64_t *out_i,
                                                              int out_stride, int out_col0, float *ub_s, uint32_t *ub_i, const uint32_t *gate, uint32_t gate_epoch) {
    if (ms_gate_closed(gate, gate_epoch)) return;      // (the exact pipeline behind a prefiltered search: only when it is needed)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint2 *pool = reinterpret_cast<uint2 *>(smem);              // [k*k]
    uint2 *list = pool + (size_t)k * k;                         // [k]
    __shared__ float red_s[4];
    __shared__ uint32_t red_i[4];
    __shared__ int red_slot[4];
    __shared__ int pool_count;
    const int q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *ps = part_s + (size_t)q * k * P;
    const uint32_t *pi = part_i + (size_t)q * k * P;
    constexpr int PER = MERGE_MAX_P / 256;
    float hs[PER];
    uint32_t hi[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int pp = tid + u * 256;
        hs[u] = -INFINITY; hi[u] = MS_IDX_NONE;
        if (pp < P) { hs[u] = ps[pp]; hi[u] = pi[pp]; }
    }
    if (tid == 0) pool_count = 0;
    // 1. k-th best head
    float th_s = -INFINITY;
    uint32_t th_i = MS_IDX_NONE;
    for (int round = 0; round < k; ++round) {
        float bs = -INFINITY; uint32_t bi = MS_IDX_NONE; int bslot = -1;
#pragma unroll
        for (int u = 0; u < PER; ++u)
            if (hi[u] != MS_IDX_NONE && (bslot < 0 || ms_better(hs[u], hi[u], bs, bi))) { bs = hs[u]; bi = hi[u]; bslot = tid + u * 256; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(bs, off);
            const uint32_t oi = __shfl_xor(bi, off);
            const int oslot = __shfl_xor(bslot, off);
            if (oslot >= 0 && (bslot < 0 || ms_better(os, oi, bs, bi))) { bs = os; bi = oi; bslot = oslot; }
        }
        if (lane == 0) { red_s[wave] = bs; red_i[wave] = bi; red_slot[wave] = bslot; }
        __syncthreads();
        bs = red_s[0]; bi = red_i[0]; bslot = red_slot[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (red_slot[w] >= 0 && (bslot < 0 || ms_better(red_s[w], red_i[w], bs, bi))) { bs = red_s[w]; bi = red_i[w]; bslot = red_slot[w]; }
        __syncthreads();
        if (bslot < 0) { th_s = -INFINITY; th_i = MS_IDX_NONE; break; }   // fewer than k non-empty lists: keep everything
        th_s = bs; th_i = bi;
#pragma unroll
        for (int u = 0; u < PER; ++u)
            if (bslot == tid + u * 256) hi[u] = MS_IDX_NONE;              // remove the winner
    }
    // 2. pool of entries not worse than the threshold
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int pp = tid + u * 256;
        if (pp >= P) continue;
        for (int j = 0; j < k; ++j) {
            const float s = ps[(size_t)j * P + pp];
            const uint32_t i = pi[(size_t)j * P + pp];
            if (i == MS_IDX_NONE) break;
            if (th_i != MS_IDX_NONE && ms_better(th_s, th_i, s, i)) break;     // strictly worse than the threshold
            const int slot = atomicAdd(&pool_count, 1);
            if (slot < k * k) pool[slot] = make_uint2(__float_as_uint(s), i);
        }
    }
    if (tid < k) list[tid] = make_uint2(__float_as_uint(-INFINITY), MS_IDX_NONE);
    __syncthreads();
    // 3. final selection by one wave
    if (wave == 0) {
        const int count = pool_count < k * k ? pool_count : k * k;
        for (int c0 = 0; c0 < count; c0 += 64) {
            const int idx = c0 + lane;
            const uint2 e = idx < count ? pool[idx] : make_uint2(0u, MS_IDX_NONE);
            const int nn = (count - c0) < 64 ? (count - c0) : 64;
            for (int i = 0; i < nn; ++i)
                ms_wave_insert(list, k, ms_readlane_f(__uint_as_float(e.x), i), ms_readlane_u(e.y, i), lane);
        }
        if (lane < k) {
            const uint2 e = list[lane];
            const size_t o = (size_t)q * out_stride + out_col0 + lane;
            out_s[o] = __uint_as_float(e.x);
            out_i[o] = (e.y == MS_IDX_NONE) ? (int64_t)-1 : row_offset + (int64_t)e.y;
            if (lane == k - 1 && ub_s != nullptr) { ub_s[q] = __uint_as_float(e.x); ub_i[q] = e.y; }
        }
    }
}

// Head-advance form of the same merge for small k * P (the usual case: k = 10, P <= 128 lists):
// one wave per query stages the [k][P] block in LDS, then runs k rounds of "best list head
// wins and its list advances" -- a wave-level arg-max per round, no block barrier, no pool.
template <int PER>      // lists per lane: P <= 64 * PER
__global__ __launch_bounds__(64) void ms_head_merge_kernel(const float *part_s, const uint32_t *part_i, int P, int k,
                                                          int64_t row_offset, float *out_s, int64_t *out_i,
                                                          int out_stride, int out_col0, float *ub_s, uint32_t *ub_i, const uint32_t *gate, uint32_t gate_epoch) {
    if (ms_gate_closed(gate, gate_epoch)) return;      // (the exact pipeline behind a prefiltered search: only when it is needed)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ms_head_merge_wave<PER>(reinterpret_cast<uint2 *>(smem), part_s, part_i, P, k, row_offset, out_s, out_i, out_stride, out_col0,
                            ub_s, ub_i, blockIdx.x, threadIdx.x);
}

// The same merge by a whole workgroup per query (ms_block_merge: threshold = the k-th best list head, then the few entries at
// or above it rank themselves; no serial rounds).  The form launch_merge uses for P <= 256 lists when the [k][P] block
// fits in LDS; shapes ms_block_merge declines (fewer lists than k, ties by the hundred) go through the head-advance merge of
// the workgroup's first wave.
// dp / qmap (the exact pass over the flagged queries of a prefiltered search): the number of queries and of lists comes from the
// device plan, and query q of the compacted batch is row qmap[q] of the outputs.
__device__ __forceinline__ void ms_block_merge_body(char *smem, const float *part_s, const uint32_t *part_i, int P, int k,
                                                    int64_t row_offset, float *out_s, int64_t *out_i,
                                                    int out_stride, int out_col0, float *ub_s, uint32_t *ub_i,
                                                    const ScanDevPlan *dp, const int *qmap, int sparse, size_t sm_stride,
                                                    uint2 *keep = nullptr) {
    // keep (round 6; the fused merge + re-scoring launch): the k merged entries are ALSO left in LDS -- keep[rank] = {score bits, row or
    // MS_IDX_NONE}, keep[64].x = 1 when they are all there -- so that the re-scoring behind the merge does not read back through L2 what
    // this workgroup has just written (one round trip of ~1.5 us per call)
    int q = blockIdx.x;
    if (dp != nullptr) {
        if (q >= dp->nq) return;
        P = dp->P;
    }
    const int q_out = qmap != nullptr ? qmap[q] : q;
    const int tid = threadIdx.x, kP = k * P;
    uint2 *ent = reinterpret_cast<uint2 *>(smem + MS_BLOCK_MERGE_SCRATCH);
    const size_t base = (size_t)q * kP;
    // entry (rank r, list l) of this query: rank-major [k][P] per query, or (sm_stride > 0) stream-major [list][query][rank]
    auto at = [&](int r, int l) -> size_t { return sm_stride != 0 ? (size_t)l * sm_stride + (size_t)q * k + r : base + (size_t)r * P + l; };
    if (sparse) {
        // SPARSE lists (the prefilter's: 256 streams, 20 slots each, ~100 entries in all -- a bound filtered the rest): every thread
        // walks its own list (four ranks in one round trip, further ones only where the fourth is occupied) and appends what it finds
        // to a pool; the pool ranks itself (rows are distinct: an entry's place = how many beat it).  40 KB of mostly empty slots
        // are not staged at all: 28 -> ~5 us at C2.  More than 512 entries (clustered data): the general merge below.
        __shared__ int pool_n;
        unsigned long long *pk = reinterpret_cast<unsigned long long *>(smem);            // [512]  (the scratch area: 8 KiB)
        uint2 *pe = reinterpret_cast<uint2 *>(smem + 4096);                                // [512]
        if (tid == 0) pool_n = 0;
        __syncthreads();
        for (int l = tid; l < P; l += 256) {
            float s4[4];
            uint32_t i4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                i4[r] = MS_IDX_NONE; s4[r] = -INFINITY;
                if (r < k) { s4[r] = part_s[at(r, l)]; i4[r] = part_i[at(r, l)]; }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (i4[r] == MS_IDX_NONE) continue;
                const int pos = atomicAdd(&pool_n, 1);
                if (pos < 512) { const uint2 e = make_uint2(__float_as_uint(s4[r]), i4[r]); pk[pos] = ms_order_key(e); pe[pos] = e; }
            }
            if (k > 4 && i4[3] != MS_IDX_NONE) {
                for (int r = 4; r < k; ++r) {
                    const uint32_t ii = part_i[at(r, l)];
                    if (ii == MS_IDX_NONE) break;
                    const int pos = atomicAdd(&pool_n, 1);
                    if (pos < 512) { const uint2 e = make_uint2(__float_as_uint(part_s[at(r, l)]), ii); pk[pos] = ms_order_key(e); pe[pos] = e; }
                }
            }
        }
        __syncthreads();
        const int n = pool_n;
        if (n <= 512) {
            for (int e = tid; e < n; e += 256) {
                const unsigned long long key = pk[e];
                int rank = 0;
                for (int j = 0; j < n; ++j) rank += pk[j] > key ? 1 : 0;
                if (rank < k) {
                    const uint2 v = pe[e];
                    const size_t o = (size_t)q_out * out_stride + out_col0 + rank;
                    out_s[o] = __uint_as_float(v.x);
                    out_i[o] = row_offset + (int64_t)v.y;
                    if (keep != nullptr) keep[rank] = v;
                }
            }
            if (tid < k && tid >= n) {
                const size_t o = (size_t)q_out * out_stride + out_col0 + tid;
                out_s[o] = -INFINITY;
                out_i[o] = -1;
                if (keep != nullptr) keep[tid] = make_uint2(__float_as_uint(-INFINITY), MS_IDX_NONE);
            }
            if (keep != nullptr && tid == 0) keep[64].x = 1u;
            return;
        }
        __syncthreads();            // (the pool is abandoned: the scratch area is the general merge's from here on)
    }
    if (sm_stride != 0) {           // stream-major: thread l copies its list (k contiguous entries) into the [k][P] staging order
        for (int l = tid; l < P; l += 256)
            for (int r = 0; r < k; ++r) ent[(size_t)r * P + l] = make_uint2(__float_as_uint(part_s[at(r, l)]), part_i[at(r, l)]);
    } else if ((kP & 3) == 0) {
        const float4 *ps4 = reinterpret_cast<const float4 *>(part_s + base);
        const uint4 *pi4 = reinterpret_cast<const uint4 *>(part_i + base);
#pragma unroll 4
        for (int e = tid; e < (kP >> 2); e += 256) {
            const float4 sv = ps4[e];
            const uint4 iv = pi4[e];
            uint2 *dst = ent + 4 * e;
            dst[0] = make_uint2(__float_as_uint(sv.x), iv.x); dst[1] = make_uint2(__float_as_uint(sv.y), iv.y);
            dst[2] = make_uint2(__float_as_uint(sv.z), iv.z); dst[3] = make_uint2(__float_as_uint(sv.w), iv.w);
        }
    } else {
#pragma unroll 4
        for (int e = tid; e < kP; e += 256) ent[e] = make_uint2(__float_as_uint(part_s[base + e]), part_i[base + e]);
    }
    __syncthreads();
    const uint2 *fin = ms_block_merge(ent, smem, P, k, tid);
    if (fin == nullptr) {        // (uniform across the workgroup)
        if (tid < 64)       // (`ent` is staged already: the wave reads nothing at part_s / part_i, and q only names the output row)
            ms_head_merge_wave<4, true>(ent, part_s, part_i, P, k, row_offset, out_s, out_i, out_stride, out_col0, ub_s, ub_i, q_out, tid);
        if (keep != nullptr && tid == 0) keep[64].x = 0u;      // (this rare form writes the global lists only: the re-scoring reads them back)
        return;
    }
    if (keep != nullptr) {
        if (tid < k) keep[tid] = fin[tid];
        if (tid == 0) keep[64].x = 1u;
    }
    if (tid < k) {
        const uint2 v = fin[tid];
        const size_t o = (size_t)q_out * out_stride + out_col0 + tid;
        out_s[o] = __uint_as_float(v.x);
        out_i[o] = v.y == MS_IDX_NONE ? (int64_t)-1 : row_offset + (int64_t)v.y;
        if (tid == k - 1 && ub_s != nullptr) { ub_s[q_out] = __uint_as_float(v.x); ub_i[q_out] = v.y; }
    }
}

__global__ __launch_bounds__(256) void ms_block_merge_kernel(const float *part_s, const uint32_t *part_i, int P, int k,
                                                             int64_t row_offset, float *out_s, int64_t *out_i,
                                                             int out_stride, int out_col0, float *ub_s, uint32_t *ub_i, const uint32_t *gate, uint32_t gate_epoch,
                                                             const ScanDevPlan *dp, const int *qmap, int sparse, size_t sm_stride) {
    if (ms_gate_closed(gate, gate_epoch)) return;      // (the exact pipeline behind a prefiltered search: only when it is needed)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ms_block_merge_body(smem, part_s, part_i, P, k, row_offset, out_s, out_i, out_stride, out_col0, ub_s, ub_i, dp, qmap, sparse, sm_stride);
}

// ------------------------------------------------------------------ sample bound -------
// Lower bound of the full pass from the sample pass's lists: the k-th largest (with multiplicity) of the first
// `ranks` entries of all P lists of a query -- scores of distinct rows, so at least k rows score >= the result.
// Values only (no rows, no sorted output): one wave per query, the values in registers, k rounds of "largest value
// below the previous one + how many lanes hold it".  -inf when there are fewer than k sampled rows.
template <int VPL>      // values per lane: ranks * P <= 64 * VPL
// sm_stride > 0: the lists are STREAM-MAJOR ([stream][query][rank], the image scans of the prefilter: ms_scan_pf.h) -- entry (rank r,
// list l) of query q is at l * sm_stride + q * k + r, sm_stride = nq_pad * k; 0: rank-major per query ([query][rank][stream]).
__global__ __launch_bounds__(64) void ms_sample_bound_kernel(const float *part_s, int P, int k, int ranks, float *lb, uint32_t *hist,
                                                            float *hstep, const uint32_t *gate, uint32_t gate_epoch, size_t sm_stride) {
    if (ms_gate_closed(gate, gate_epoch)) return;      // (the exact pipeline behind a prefiltered search: only when it is needed)
    const int q = blockIdx.x, lane = threadIdx.x;
    const float *ps = part_s + (size_t)q * k * P;              // rank-major [k][P]: the first ranks * P floats
    const int count = ranks * P;
    float v[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int idx = lane + 64 * i;
        if (sm_stride == 0) v[i] = idx < count ? ps[idx] : -INFINITY;
        else v[i] = idx < count ? part_s[(size_t)(idx % P) * sm_stride + (size_t)q * k + idx / P] : -INFINITY;
    }
    float kth = -INFINITY, top = -INFINITY, second = -INFINITY, third = -INFINITY;        // (second, third: with multiplicity)
    // wave maximum: 4 DPP steps inside each row of 16 lanes, then the 4 row results through SGPRs
#define MS_DPP_FMAX(CTRL) m = fmaxf(m, __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(m), CTRL, 0xF, 0xF, false)));
    if constexpr (VPL <= 8) {
        // Round 6: every lane sorts its own <= 8 values once (a network of compare-exchanges), then k rounds of "the largest lane HEAD, and
        // the lowest lane that holds it pops" -- ~30 instructions per round instead of ~60 (the form below scans all VPL values and takes
        // VPL ballots per round): the k-th largest with multiplicity, the same value.  9.6 -> ~7 us for the image scan's 20 rounds.
#define MS_CE(A, B) { const float hi_ = fmaxf(v[A], v[B]), lo_ = fminf(v[A], v[B]); v[A] = hi_; v[B] = lo_; }
        if constexpr (VPL == 4) { MS_CE(0, 1) MS_CE(2, 3) MS_CE(0, 2) MS_CE(1, 3) MS_CE(1, 2) }
        if constexpr (VPL == 8) {
            MS_CE(0, 1) MS_CE(2, 3) MS_CE(4, 5) MS_CE(6, 7) MS_CE(0, 2) MS_CE(1, 3) MS_CE(4, 6) MS_CE(5, 7) MS_CE(1, 2) MS_CE(5, 6)
            MS_CE(0, 4) MS_CE(1, 5) MS_CE(2, 6) MS_CE(3, 7) MS_CE(2, 4) MS_CE(3, 5) MS_CE(1, 2) MS_CE(3, 4) MS_CE(5, 6)
        }
#undef MS_CE
        for (int round = 0; round < k; ++round) {
            float m = v[0];
            MS_DPP_FMAX(0xB1) MS_DPP_FMAX(0x4E) MS_DPP_FMAX(0x141) MS_DPP_FMAX(0x140)
            m = fmaxf(fmaxf(ms_readlane_f(m, 0), ms_readlane_f(m, 16)), fmaxf(ms_readlane_f(m, 32), ms_readlane_f(m, 48)));
            if (!(m > -INFINITY)) { kth = -INFINITY; break; }             // fewer than k values: no bound
            if (round == 0) top = m;
            if (round == 1) second = m;
            if (round == 2) third = m;
            kth = m;
            const int win = __builtin_ctzll(__ballot(v[0] == m));        // (some lane's head IS the maximum)
            if (lane == win) {
#pragma unroll
                for (int i = 0; i + 1 < VPL; ++i) v[i] = v[i + 1];
                v[VPL - 1] = -INFINITY;
            }
        }
    } else {
    float cur = INFINITY;
    int remaining = k;
    for (int round = 0; round < k; ++round) {
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < VPL; ++i) m = (v[i] < cur) ? fmaxf(m, v[i]) : m;
        MS_DPP_FMAX(0xB1) MS_DPP_FMAX(0x4E) MS_DPP_FMAX(0x141) MS_DPP_FMAX(0x140)
        m = fmaxf(fmaxf(ms_readlane_f(m, 0), ms_readlane_f(m, 16)), fmaxf(ms_readlane_f(m, 32), ms_readlane_f(m, 48)));
        if (!(m > -INFINITY)) break;                              // fewer than k values: no bound
        if (round == 0) top = m;
        int c = 0;
#pragma unroll
        for (int i = 0; i < VPL; ++i) c += __popcll(__ballot(v[i] == m));
        const int seen = k - remaining;                               // values above m so far
        if (seen < 2 && seen + c >= 2) second = m;
        if (seen < 3 && seen + c >= 3) third = m;
        if (c >= remaining) { kth = m; break; }
        remaining -= c;
        cur = m;
    }
    }
#undef MS_DPP_FMAX
    if (lane == 0) lb[q] = kth;
    // Score buckets of the full pass's shared bound (ScanHist): the k-th best of the whole shard sits near the sample's BEST
    // score (the sample is a few percent of the rows), so 16 buckets of (best - k-th) / 12 from the k-th up cover the range
    // the bound moves through; the last bucket is open-ended.  No usable spread: step 0 = no histogram for this query.
    // Round 6: "best - k-th" is taken from the SLOPE of the sample's tail, not from its single best score.  Scores of rank r in a tail fall
    // like kth + b ln(k / r); b from rank 1, 2 and 3 each, the MEDIAN of the three.  On a smooth tail the three agree and the buckets are
    // the ones above; a sampled row that is no part of the tail -- a near-duplicate of the query, a close homologue: cosine 0.97 over a
    // tail that ends at 0.35 -- used to stretch the 16 buckets over the whole gap, the bound of that query then never rose, and its ~1,200
    // rows above the sample bound (not ~60) all went through the rare path, the merge and the re-scoring: the bench's database plants three
    // such rows per query, ~6 of 256 queries caught one in the sample, and the C2 step cost 141 us instead of 130
    // (profiles/r06_hist_step_ab.log).
    if (hist != nullptr) {
        if (lane < 16) hist[(size_t)q * 16 + lane] = 0u;
        if (lane == 0) {
            float spread = (kth > -INFINITY && top > kth) ? top - kth : 0.0f;
            if (spread > 0.0f && k >= 4) {
                const float lk = __logf((float)k);
                const float b1 = (top - kth) / lk, b2 = (second - kth) / (lk - 0.6931472f), b3 = (third - kth) / (lk - 1.0986123f);
                const float bm = fmaxf(fminf(b1, b2), fminf(fmaxf(b1, b2), b3));                 // median
                if (bm > 0.0f && bm < INFINITY) spread = bm * lk;
            }
            float step = spread * (1.0f / 12.0f);
            if (!(step > 0.0f) || !(step < INFINITY) || !(1.0f / step < INFINITY)) step = 0.0f;
            hstep[q] = step;
        }
    }
}

// ------------------------------------------------------------------ prefilter: exact re-scoring ---
// ms_ip_topk_prefiltered: the scan ran on APPROXIMATE scores a(row) (split-bf16 matrix instructions, |a - s| <= E =
// MS_PF_ERR |row| |q|) and kept the kp > k best rows per query by a.  One wave per query re-scores those rows with the exact
// fp32 chain (the k order of the fp32 scan: s = 0..63: (k = s, k = 64 + s), one fmaf each -- the same bits), takes the
// best k under the total order, and proves the answer: every row that is NOT a candidate has a <= a_last (the kp-th
// approximate score), hence s <= a_last + E; if the k-th best exact score is above that, no other row can be in the
// answer or tie with it (the candidate list must be full for that argument: a list with empty slots raises the gate too).  Otherwise (near-ties by the dozen around the k-th best) the query raises the gate and the exact
// pipeline, queued behind this kernel, runs after all.
// The flagged queries are gathered for the exact pass right here (round 4b; a separate one-workgroup kernel before): a flagged
// query takes the next slot of the compacted batch (an atomic counter in library-owned memory: the order of the batch varies from
// run to run, the results do not -- every query's exact pass is its own) and copies its vector, bound and length there; the LAST
// workgroup to finish (a ticket) writes the launch plan of the exact pass for that many queries, raises the gate and resets both
// counters.
struct PfCompact {
    float *qn_c, *lb_c, *qlen_c;
    int *qmap;
    ScanDevPlan *dp;
    uint32_t *gate;          // [0] gate, [1] epoch, [2] flagged count (diagnostics), [4] slot counter, [5] ticket (never reset: counts on)
    uint32_t epoch;
    uint32_t ticket_base;    // value of the ticket counter when this call's first workgroup arrives (the host keeps the running total)
    int64_t n;
    int cus, nq;
};
// The two counters of the compaction (slot counter, ticket) are plain atomic adds -- 256 workgroups arrive within a few
// microseconds, and a compare-and-swap loop per arrival (tried: counters tagged with the call's epoch) serialises them into
// O(n^2) retries: +250 us at C2.  Round 6: the TICKET is never reset -- it counts on from call to call, the host keeps the running
// total per workspace (ms_wsstate.h) and hands every call the value its first arrival will see (ticket_base): the last
// workgroup is the one that draws ticket_base + nq - 1.  A counter that is not where the host expects it (a launch that was
// aborted half way, a second stream sharing the workspace against the header's rule, memory poisoned through
// ms_debug_prefilter_poison) never produces that ticket, gate[1] keeps the previous call's epoch, and the gated launches queued
// behind (ms_gate_closed) TRAP instead of leaving the flagged queries with an unproven answer.  The slot counter is still zeroed by
// the last workgroup (its final value is data-dependent).
struct PfRescore {
    const float *db, *qn, *as;
    const int64_t *ai;
    const float *lengths, *qlen;
    float *out_s;
    int64_t *out_i;
    uint32_t *flag;
    int64_t row_offset;
    float err_coef, mincov;
    float q_eps;             // > 0: qn is the caller's RAW query array -- the workgroup normalises its query itself, exactly (round 6)
    int k, kp, fp16_range;
    PfCompact cp;
};
// Every thread of the workgroup calls it (barriers inside); the first wave does the work.  `coherent`: the candidate lists were
// written by THIS workgroup a moment ago (the fused merge + re-scoring launch): read them past the L1.
// The query of a re-scoring workgroup, requested early (round 6: the fused launch asks for it BEFORE it merges the candidate lists, so that its
// round trip runs under the merge's own loads): this lane's float2 of the raw query, or its two floats of the prepared one
struct PfQueryPre { float x, y; };
__device__ __forceinline__ PfQueryPre ms_rescore_query_load(const PfRescore &a, int q, int tid) {
    PfQueryPre r{0.0f, 0.0f};
    if (tid < 64) {
        if (a.q_eps > 0.0f) { const float2 v = *(reinterpret_cast<const float2 *>(a.qn + (size_t)q * MS_DIM) + tid); r.x = v.x; r.y = v.y; }
        else { r.x = a.qn[(size_t)q * MS_DIM + tid]; r.y = a.qn[(size_t)q * MS_DIM + 64 + tid]; }
    }
    return r;
}
__device__ __forceinline__ void ms_rescore_body(const PfRescore &a, int q, int tid, bool coherent, const uint2 *keep = nullptr,
                                                const PfQueryPre *pre = nullptr) {
    __shared__ float qs[128];
    __shared__ float cs[64];
    __shared__ uint32_t ci[64];
    __shared__ float kth;
    __shared__ int slot_s;
    const bool act = tid < 64;
    const int lane = tid & 63;
    const int k = a.k, kp = a.kp;
    const PfCompact &cp = a.cp;
    if (act) {
        if (a.q_eps > 0.0f) {
            // raw query: F.normalize (dbsearch.py:303-304, eps 1e-12) / cosine_similarity's own normalisation (dbsearch.py:78, eps 1e-8) in the
            // arithmetic of ms_normalize_rows_kernel -- float2 per lane, the same butterfly sum, sqrt, max, divide: the same bits -- which
            // is what the exact scores below (and the exact pass's copy of the query) are made of; the image scan in front of this launch
            // normalised the same query approximately, which is all its error bound asks for (ms_scan_pf16.h)
            const PfQueryPre ld = pre != nullptr ? *pre : ms_rescore_query_load(a, q, tid);
            float2 v = make_float2(ld.x, ld.y);
            const float ss = wave_sum(v.x * v.x + v.y * v.y);
            const float nrm = fmaxf(sqrtf(ss), a.q_eps);
            v.x = v.x / nrm;
            v.y = v.y / nrm;
            qs[2 * lane] = v.x;
            qs[2 * lane + 1] = v.y;
        } else {
            const PfQueryPre ld = pre != nullptr ? *pre : ms_rescore_query_load(a, q, tid);
            qs[lane] = ld.x;
            qs[64 + lane] = ld.y;
        }
        if (lane == 0) kth = -INFINITY;
    }
    __syncthreads();
    float qnorm = 0.0f, a_last = 0.0f, s = -INFINITY;
    int64_t row = -1;
    bool full = false;
    if (act) {
        float qq = qs[lane] * qs[lane] + qs[64 + lane] * qs[64 + lane];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) qq += __shfl_xor(qq, off);
        qnorm = sqrtf(qq) * 1.001f;
        const int64_t *aq = a.ai + (size_t)q * kp;
        const float *sq = a.as + (size_t)q * kp;
        if (keep != nullptr && keep[64].x != 0u) {          // (uniform) the candidates are still in LDS
            const uint2 mine = keep[lane < kp ? lane : 0], last = keep[kp - 1];
            row = (lane < kp && mine.y != MS_IDX_NONE) ? (int64_t)mine.y : -1;
            full = last.y != MS_IDX_NONE;
            a_last = __uint_as_float(last.x);
        } else if (coherent) {
            row = lane < kp ? __hip_atomic_load(aq + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
            full = __hip_atomic_load(aq + kp - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0;
            a_last = __hip_atomic_load(sq + kp - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            row = lane < kp ? aq[lane] : -1;
            full = aq[kp - 1] >= 0;
            a_last = sq[kp - 1];
        }
        if (row >= 0) {
            const float4 *x = reinterpret_cast<const float4 *>(a.db + (size_t)row * MS_DIM);
            float acc = 0.0f;
            // (the whole row requested before the chain starts: four batches of eight loads, each a round trip to a row nobody has
            //  touched, were most of this kernel's 14 us)
            float4 xl[16], xh[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) { xl[t] = x[t]; xh[t] = x[16 + t]; }
            __builtin_amdgcn_sched_barrier(0);          // (or hipcc pulls the loads back next to their uses, eight at a time)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float4 lo = xl[t], hi = xh[t];
                acc = fmaf(lo.x, qs[4 * t + 0], acc); acc = fmaf(hi.x, qs[64 + 4 * t + 0], acc);
                acc = fmaf(lo.y, qs[4 * t + 1], acc); acc = fmaf(hi.y, qs[64 + 4 * t + 1], acc);
                acc = fmaf(lo.z, qs[4 * t + 2], acc); acc = fmaf(hi.z, qs[64 + 4 * t + 2], acc);
                acc = fmaf(lo.w, qs[4 * t + 3], acc); acc = fmaf(hi.w, qs[64 + 4 * t + 3], acc);
            }
            s = acc;
            if (a.lengths != nullptr) {       // MS_MODE_COSINE_UNIT: the fp32 scan's own two multiplications (unit rows: scale 1; dbsearch.py:76,78)
                float sv = s * 1.0f;
                const float mk = (a.qlen[q] >= a.lengths[row] * a.mincov) ? 1.0f : 0.0f;
                sv = sv * mk;
                s = sv;
            }
        }
        cs[lane] = s;
        ci[lane] = row >= 0 ? (uint32_t)row : MS_IDX_NONE;
    }
    __syncthreads();
    if (act) {
        const int nvalid = __popcll(__ballot(row >= 0));
        int rank = 0;
        for (int j = 0; j < kp; ++j) rank += (ci[j] != MS_IDX_NONE && ms_better(cs[j], ci[j], s, ci[lane])) ? 1 : 0;
        const size_t o0 = (size_t)q * k;
        if (row >= 0 && rank < k) { a.out_s[o0 + rank] = s; a.out_i[o0 + rank] = a.row_offset + row; }
        if (lane < k && lane >= nvalid) { a.out_s[o0 + lane] = -INFINITY; a.out_i[o0 + lane] = -1; }
        if (row >= 0 && rank == k - 1) kth = s;
    }
    __syncthreads();
    if (tid == 0) {
        // (kth: k rows score at least this -- the bound the exact scan starts from, should it have to run (-inf: none): lb_c below)
        // (a list that is not full cannot happen on a database of >= 65,536 rows unless rows were lost to a bound: no proof then either)
        // (fp16 formats: the scan scales every query into the fp16 range by a power of two it clamps at 2^+-60 -- a query whose norm is
        //  outside [2^-40, 2^40] is not covered by the error bound: no proof)
        const bool in_range = !a.fp16_range || (qnorm >= 9.094947e-13f && qnorm <= 1.0995116e12f);
        const bool flagged = !full || !in_range || !(kth > a_last + a.err_coef * qnorm);
        a.flag[q] = flagged ? 1u : 0u;
        int slot = -1;
        if (flagged) {
            slot = (int)atomicAdd(cp.gate + 4, 1u);
            cp.qmap[slot] = q;
            cp.lb_c[slot] = kth;
            cp.qlen_c[slot] = a.qlen != nullptr ? a.qlen[q] : 0.0f;
        }
        slot_s = slot;
    }
    __syncthreads();
    const int slot = slot_s;
    if (act && slot >= 0) {
        cp.qn_c[(size_t)slot * MS_DIM + lane] = qs[lane];
        cp.qn_c[(size_t)slot * MS_DIM + 64 + lane] = qs[64 + lane];
    }
    if (tid == 0) {
        __threadfence();                                         // (this workgroup's slot is taken before its ticket)
        const uint32_t done = atomicAdd(cp.gate + 5, 1u);
        // this call's nq tickets are ticket_base .. ticket_base + nq - 1: any other value means the counter was not where the host's
        // running total says (behind: the first arrival sees it; ahead by less than nq: the "last" ticket would be drawn EARLY, by a
        // workgroup that is not the last, and the late arrivals see it here) -- trap, never an unproven answer
        if (done - cp.ticket_base >= (uint32_t)cp.nq) __builtin_trap();
        if (done == cp.ticket_base + (uint32_t)cp.nq - 1u) {    // the last workgroup of THIS call: every flagged query has its slot
            __threadfence();
            const int cnt = (int)atomicAdd(cp.gate + 4, 0u);
            ScanDevPlan d;
            ms_plan_core(cp.n, cnt > 0 ? cnt : 1, cp.cus, &d);
            if (cnt == 0) { d.nq = 0; d.grid = 0; }
            *cp.dp = d;
            cp.gate[0] = cnt > 0 ? cp.epoch : 0u;
            cp.gate[1] = cp.epoch;
            cp.gate[2] = (uint32_t)cnt;
            cp.gate[4] = 0u;                                     // (for the next call on this workspace: stream order; the ticket counts on)
        }
    }
}
// ONE launch for the prefilter's candidate merge and the exact re-scoring behind it (round 5; two launches and a clearing memset
// before): a workgroup merges the per-stream lists of its query into the kp candidates (ms_block_merge_body: the sparse pool, or
// the general merge), then its first wave re-scores them, ranks them, proves the answer or takes a slot of the exact pass.
__global__ __launch_bounds__(256) void ms_merge_rescore_kernel(const float *part_s, const uint32_t *part_i, int P, float *as, int64_t *ai,
                                                               size_t sm_stride, const PfRescore a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint2 keep[65];          // the kp <= 64 merged candidates + [64].x: are they all here?
    const PfQueryPre pre = ms_rescore_query_load(a, (int)blockIdx.x, (int)threadIdx.x);
    ms_block_merge_body(smem, part_s, part_i, P, a.kp, 0, as, ai, a.kp, 0, nullptr, nullptr, nullptr, nullptr, 1, sm_stride, keep);
    __threadfence_block();
    __syncthreads();
    ms_rescore_body(a, (int)blockIdx.x, (int)threadIdx.x, true, keep, &pre);
}

// ------------------------------------------------------------------ public k-way merge -
// One thread per query: classic k-way merge of S lists that are each sorted best-first.
__global__ __launch_bounds__(64) void ms_kway_merge_kernel(const float *scores0, const int64_t *idx0, int64_t score_stride,
                                                           int64_t idx_stride, int S, int nq, int k, float *out_s,
                                                           int64_t *out_i) {
    // list s lives at byte offset s * stride of each array (dense [S,nq,k] arrays: stride = nq*k elements)
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    constexpr int MAXS = 64;
    int head[MAXS];
    for (int s = 0; s < S; ++s) head[s] = 0;
    for (int j = 0; j < k; ++j) {
        int best = -1;
        float bs = 0.0f;
        int64_t bi = 0;
        for (int s = 0; s < S; ++s) {
            if (head[s] >= k) continue;
            const size_t o = (size_t)q * k + head[s];
            const int64_t ci = reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(idx0) + (size_t)s * idx_stride)[o];
            if (ci < 0) { head[s] = k; continue; }   // padding: list exhausted
            const float cs = reinterpret_cast<const float *>(reinterpret_cast<const char *>(scores0) + (size_t)s * score_stride)[o];
            if (best < 0 || cs > bs || (cs == bs && ci < bi)) { best = s; bs = cs; bi = ci; }
        }
        const size_t oo = (size_t)q * k + j;
        if (best < 0) { out_s[oo] = -INFINITY; out_i[oo] = -1; }
        else { out_s[oo] = bs; out_i[oo] = bi; ++head[best]; }
    }
}

// The same merge for any number of lists (S > 64: no per-thread head array): output j is the best entry that comes
// strictly after output j-1 in the total order (score desc, index asc; indices are unique across the lists), found
// by a linear walk of every sorted list.  O(k * S * k) per query: only used beyond 64 lists.
__global__ __launch_bounds__(64) void ms_kway_merge_any_kernel(const float *scores0, const int64_t *idx0, int64_t score_stride,
                                                               int64_t idx_stride, int S, int nq, int k, float *out_s,
                                                               int64_t *out_i) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    bool have_prev = false;
    float ps = 0.0f;
    int64_t pi = 0;
    for (int j = 0; j < k; ++j) {
        bool found = false;
        float bs = 0.0f;
        int64_t bi = 0;
        for (int s = 0; s < S; ++s) {
            const float *ls = reinterpret_cast<const float *>(reinterpret_cast<const char *>(scores0) + (size_t)s * score_stride) + (size_t)q * k;
            const int64_t *li = reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(idx0) + (size_t)s * idx_stride) + (size_t)q * k;
            for (int e = 0; e < k; ++e) {
                const int64_t ci = li[e];
                if (ci < 0) break;                                   // padding: list exhausted
                const float cs = ls[e];
                if (have_prev && !(cs < ps || (cs == ps && ci > pi))) continue;   // not after the previous output
                if (!found || cs > bs || (cs == bs && ci < bi)) { found = true; bs = cs; bi = ci; }
                break;                                               // sorted list: its first entry after prev is its best one
            }
        }
        const size_t oo = (size_t)q * k + j;
        if (!found) { for (int r = j; r < k; ++r) { out_s[(size_t)q * k + r] = -INFINITY; out_i[(size_t)q * k + r] = -1; } return; }
        out_s[oo] = bs; out_i[oo] = bi;
        have_prev = true; ps = bs; pi = bi;
    }
}

// ------------------------------------------------------------------ host side ----------
// (the switches, the launch plan, the workspace carve and the rules shared below: ms_plan.h)
// The device behind the per-workspace records (ms_wsstate.h: everything the host remembers about a workspace between calls)
int ms_wsstate::current_device() { int dev = 0; return hipGetDevice(&dev) == hipSuccess ? dev : -1; }
// Both zero the block on the null stream and WAIT for it: the search that asked launches next on the caller's stream, which may be a
// non-blocking one that the null stream does not order itself with (a memset of device memory need not have finished when it returns)
static bool zero_now(void *block, size_t bytes) { return hipMemset(block, 0, bytes) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess; }
void *ms_wsstate::alloc_zeroed(size_t bytes) {
    void *mem = nullptr;
    if (hipMalloc(&mem, bytes) == hipSuccess && !zero_now(mem, bytes)) { (void)hipFree(mem); mem = nullptr; }
    return mem;
}
bool ms_wsstate::drain_and_zero(void *block, size_t bytes) { return hipDeviceSynchronize() == hipSuccess && zero_now(block, bytes); }
namespace {

// CU count of HIP's current device (the device the caller's tensors live on: the Python front end
// makes it current for every call), cached per device ordinal.
int cu_count_cached() {
    constexpr int MAX_DEV = 64;
    static int cus[MAX_DEV] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return 256;
    if (cus[dev] == 0) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cus[dev] = c;
    }
    return cus[dev];
}

int check_search_args(const float *db, int64_t n, const float *q, int nq, int k, int mode, const float *inv_norm,
                      const float *lengths, const float *qlen) {
    if (n < 0 || nq < 1 || k < 1) MS_FAIL(MS_ERR_ARG, "ms_ip_topk: need n >= 0, nq >= 1, k >= 1 (n=%lld nq=%d k=%d)",
                                          (long long)n, nq, k);
    if (n >= (int64_t)0x7FFFFFFF) MS_FAIL(MS_ERR_RANGE, "ms_ip_topk: n=%lld rows per call must be < 2^31; shard the database",
                                          (long long)n);
    if ((n > 0 && db == nullptr) || q == nullptr) MS_FAIL(MS_ERR_ARG, "ms_ip_topk: NULL db / q");
    if (mode != MS_MODE_IP_PRENORM && mode != MS_MODE_COSINE_RAW && mode != MS_MODE_COSINE_UNIT && mode != MS_MODE_IP_NORMQ)
        MS_FAIL(MS_ERR_ARG, "ms_ip_topk: unknown mode %d", mode);
    if ((mode == MS_MODE_IP_PRENORM || mode == MS_MODE_IP_NORMQ) && (inv_norm || lengths || qlen))
        MS_FAIL(MS_ERR_ARG, "ms_ip_topk: inv_norm / lengths / qlen are only valid in the cosine modes");
    if (mode == MS_MODE_COSINE_UNIT && inv_norm)
        MS_FAIL(MS_ERR_ARG, "ms_ip_topk: MS_MODE_COSINE_UNIT takes rows that are normalised already, not an inv_norm array");
    // (an empty shard -- a rank of a sharded search with no rows -- has NULL row arrays)
    if (n > 0 && (lengths == nullptr) != (qlen == nullptr)) MS_FAIL(MS_ERR_ARG, "ms_ip_topk: lengths and qlen go together");
    return MS_OK;
}

// The opening of the four fp32 entry points: argument check, the plan of the call, workspace check.  out_scores / out_idx are
// looked at where the stage writes results (ms_ip_topk, ms_ip_topk_finish -- which takes no rows or queries and checks its own few)
// Stage: the values are bits (pf_run tests them).  PREPARE = queries + sample pass + bound, SCAN = the scan launch, FINISH = the merge
// (prefiltered: + exact re-scoring + the exact pass over the queries whose proof failed)
enum Stage { PREPARE = 1, SCAN = 2, FINISH = 4, WHOLE = 7 };
int open_search(Stage stage, const float *db, int64_t n, const float *q, int nq, int k, int mode, const float *inv_norm, const float *lengths,
                const float *qlen, const float *out_scores, const int64_t *out_idx, const void *workspace, size_t workspace_bytes, ScanPlan *pl) {
    const char *who = stage == WHOLE ? "ms_ip_topk" : stage == PREPARE ? "ms_ip_topk_prepare" : stage == SCAN ? "ms_ip_topk_scan" : "ms_ip_topk_finish";
    if (stage == FINISH) {
        if (k < 1 || k > 64 || nq < 1 || out_scores == nullptr || out_idx == nullptr) MS_FAIL(MS_ERR_ARG, "%s: bad arguments", who);
    } else {
        const int rc = check_search_args(db, n, q, nq, k, mode, inv_norm, lengths, qlen);
        if (rc) return rc;
        if (stage == WHOLE && (out_scores == nullptr || out_idx == nullptr)) MS_FAIL(MS_ERR_ARG, "%s: NULL outputs", who);
        if (stage != WHOLE && k > 64) MS_FAIL(MS_ERR_ARG, "%s: k <= 64 only (use ms_ip_topk)", who);
    }
    *pl = make_plan(ms_settings(), cu_count_cached(), n, nq, k);
    if (workspace == nullptr || workspace_bytes < pl->total) MS_FAIL(MS_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, pl->total);
    return MS_OK;
}

int launch_scan(const ScanPlan &pl, const ScanParams &sp, hipStream_t st) {
    typedef int (*Launch)(const ScanPlan &, const ScanParams &, hipStream_t);
    // one row per kernel family -- the fp32 scan, the prefilter's scan over the split-bf16 image, the one over the fp16 image --
    // one column per list length (MS_KL)
    static const Launch table[3][4] = {
        {ms_launch_scan_kl5, ms_launch_scan_kl10, ms_launch_scan_kl16, ms_launch_scan_kl32},
        {ms_launch_scan_pf2_kl5, ms_launch_scan_pf2_kl10, ms_launch_scan_pf2_kl16, ms_launch_scan_pf2_kl32},
        {ms_launch_scan_pf16_kl5, ms_launch_scan_pf16_kl10, ms_launch_scan_pf16_kl16, ms_launch_scan_pf16_kl32}};
    const bool image = sp.prefilter && sp.pf_image != nullptr;
    if (!image && sp.ub_s != nullptr) return ms_launch_scan_kl32ub(pl, sp, st);
    return table[!image ? 0 : (is_f16_image(sp.pf_image, sp.pf_format) ? 2 : 1)][pick_kl_index(sp.k)](pl, sp, st);
}

// dp / qmap: the merge behind the exact pass over a prefiltered search's flagged queries -- the list count comes from the device
// plan (pl.d.P is then its upper bound), query q of the compacted batch is output row qmap[q]
int launch_merge(const ScanPlan &pl, const ScanParams &sp, int nq, int kp, int64_t row_offset, float *out_s,
                 int64_t *out_i, int out_stride, int col0, float *ub_s, uint32_t *ub_i, hipStream_t st,
                 const ScanDevPlan *dp = nullptr, const int *qmap = nullptr, int sparse = 0, size_t sm_stride = 0) {
    const uint32_t *gate = sp.gate;
    const uint32_t gate_epoch = sp.gate_epoch;
    const int P = pl.d.P;
    if (P > MERGE_MAX_P) MS_FAIL(MS_ERR_RANGE, "internal: %d partial lists exceed the merge limit", P);
    const size_t head_lds = (size_t)kp * P * sizeof(uint2);
    if (block_merge_takes(kp, P) && (ms_settings().block_merge || dp != nullptr || sm_stride != 0)) {     // the usual case: a workgroup per query
        const size_t block_lds = block_merge_lds(kp, P);
        if (block_lds > 48 * 1024)
            MS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(ms_block_merge_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)block_lds));
        hipLaunchKernelGGL(ms_block_merge_kernel, dim3(nq), dim3(256), block_lds, st, sp.part_s, sp.part_i, P, kp, row_offset, out_s,
                           out_i, out_stride, col0, ub_s, ub_i, gate, gate_epoch, dp, qmap, (ub_s == nullptr) ? sparse : 0, sm_stride);
        MS_LAUNCH_CHECK("ms_block_merge_kernel");
        return MS_OK;
    }
    if (dp != nullptr) MS_FAIL(MS_ERR_RANGE, "internal: the exact pass behind the prefilter needs the block merge (P = %d, k = %d)", P, kp);
    if (sm_stride != 0) MS_FAIL(MS_ERR_RANGE, "internal: stream-major lists need the block merge (P = %d, k = %d)", P, kp);
    if (head_lds <= 128 * 1024 && ms_settings().head_merge) {       // k * P entries fit in LDS: one wave per query, k arg-max rounds
        const int per = (P + 63) / 64;
#define MS_HEAD_MERGE(PER)                                                                                             \
    if (head_lds > 48 * 1024)                                                                                          \
        MS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(ms_head_merge_kernel<PER>),                    \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)head_lds));                  \
    hipLaunchKernelGGL(ms_head_merge_kernel<PER>, dim3(nq), dim3(64), head_lds, st, sp.part_s, sp.part_i, P, kp,       \
                       row_offset, out_s, out_i, out_stride, col0, ub_s, ub_i, gate, gate_epoch)
        if (per <= 1) { MS_HEAD_MERGE(1); }
        else if (per <= 2) { MS_HEAD_MERGE(2); }
        else if (per <= 4) { MS_HEAD_MERGE(4); }
        else if (per <= 8) { MS_HEAD_MERGE(8); }
        else { MS_HEAD_MERGE(16); }
#undef MS_HEAD_MERGE
        MS_LAUNCH_CHECK("ms_head_merge_kernel");
        return MS_OK;
    }
    const size_t lds = ((size_t)kp * kp + kp) * sizeof(uint2);
    hipLaunchKernelGGL(ms_partial_merge_kernel, dim3(nq), dim3(256), lds, st, sp.part_s, sp.part_i, P, kp, row_offset,
                       out_s, out_i, out_stride, col0, ub_s, ub_i, gate, gate_epoch);
    MS_LAUNCH_CHECK("ms_partial_merge_kernel");
    return MS_OK;
}

#ifdef MS_STAMP
constexpr size_t MS_STAMP_WORDS = 4 * 4 * 65536;
unsigned long long *ms_stamp_buffer() {
    static unsigned long long *buf = nullptr;
    if (buf == nullptr) {
        if (hipMalloc(reinterpret_cast<void **>(&buf), MS_STAMP_WORDS * 8) != hipSuccess) return nullptr;
        (void)hipMemset(buf, 0, MS_STAMP_WORDS * 8);
    }
    return buf;
}
extern "C" int ms_debug_stamps(unsigned long long *host, int words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpy(host, ms_stamp_buffer(), (size_t)words * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

// Inner-product mode uses the queries as given: the scan kernels read the caller's array directly
// (no padded copy, one launch less per batch) when it is 16-byte aligned.
// ... and so does MS_MODE_IP_NORMQ when the batch runs in the kernels for 1-2 query tiles, whose waves normalise their
// own query tile (ScanParams::qnorm_eps); larger batches get the prepared copy (ms_prepare_queries_kernel, eps 1e-12).
bool queries_used_in_place(const float *q, int mode, const ScanPlan &pl) {
    if (mode == MS_MODE_IP_PRENORM) return ((uintptr_t)q & 15) == 0;
    if (mode == MS_MODE_IP_NORMQ) return pl.d.qwb < 4 && pl.d.nq <= ms_settings().inkernel_norm_max_nq && ((uintptr_t)q & 7) == 0;
    return false;
}

// ScanParams of the full pass from the workspace layout (queries prepared, inverse norms in the
// workspace when the caller gave none); everything not named here keeps its default: off
ScanParams fill_scan_params(const ScanPlan &pl, const float *db, int64_t n, const float *q, int nq, const float *inv_norm, const float *lengths,
                            const float *qlen, float mincov, char *ws, int mode) {
    ScanParams sp{};
    const ScanDevPlan &d = pl.d;
    const bool in_place = queries_used_in_place(q, mode, pl);
    sp.db = db; sp.n = n; sp.nq = nq; sp.nq_pad = d.nq_pad;
    sp.qn = in_place ? q : pl.qn(ws);
    sp.qnorm_eps = (mode == MS_MODE_IP_NORMQ && in_place) ? 1e-12f : 0.0f;
    sp.k = pl.k_pass;
    sp.inv_norm = (mode == MS_MODE_COSINE_RAW && inv_norm == nullptr && n > 0) ? pl.inv(ws) : inv_norm;
    sp.lengths = lengths; sp.qlen = qlen; sp.mincov = mincov;
    sp.unit_rows = mode == MS_MODE_COSINE_UNIT ? 1 : 0;
    sp.qpw = pl.qpw; sp.list_sm = pl.list_sm;
    sp.part_s = pl.part_s(ws); sp.part_i = pl.part_i(ws);
    sp.rows_per_stream = d.rows_per_stream; sp.n_streams = d.n_streams; sp.n_qtiles = d.n_qtiles;
    sp.qwb = d.qwb; sp.n_qgroups = d.n_qgroups; sp.n_sgroups = d.n_sgroups; sp.P = d.P;
#ifdef MS_STAMP
    sp.stamps = ms_stamp_buffer();
#endif
    return sp;
}

// What a sample pass left in the workspace for the scan behind it: the lower bound of every query and, with `hist`, the
// shared bound's histogram (counters zeroed by ms_sample_bound_kernel, and the bucket width it chose)
void attach_prepass_results(const ScanPlan &pl, char *ws, ScanParams *sp, bool hist) {
    sp->lb_s = pl.lb_s(ws);
    if (hist) { sp->hist = pl.hist(ws); sp->hstep = pl.hstep(ws); }
}

// The counters must start at zero for EVERY scan (a second scan after one prepare would otherwise count rows twice): a staged scan
// that does not directly follow its prepare zeroes them itself
int zero_hist_unless_clean(const ScanPlan &pl, const ScanParams &sp, const void *workspace, int64_t n, int nq, int k, hipStream_t st) {
    if (sp.hist != nullptr && !ms_wsstate::take_clean(workspace, n, nq, k))
        MS_HIP_CHECK(hipMemsetAsync(sp.hist, 0, (size_t)pl.d.nq_pad * 16 * sizeof(uint32_t), st));
    return MS_OK;
}

// The bound selection over ranks * P <= 2048 values per query: the kernel whose lanes hold them all (run_prepass, and the test
// hook ms_debug_sample_bound)
int launch_sample_bound(const float *part_s, int P, int nq, int k, int ranks, float *lb, uint32_t *hist, float *hstep, const uint32_t *gate,
                        uint32_t gate_epoch, size_t sm_stride, hipStream_t st) {
    const int vpl = (ranks * P + 63) / 64;
#define MS_BOUND(V) hipLaunchKernelGGL(ms_sample_bound_kernel<V>, dim3(nq), dim3(64), 0, st, part_s, P, k, ranks, lb, hist, hstep, gate, gate_epoch, sm_stride)
    if (vpl <= 4) { MS_BOUND(4); }
    else if (vpl <= 8) { MS_BOUND(8); }
    else if (vpl <= 16) { MS_BOUND(16); }
    else { MS_BOUND(32); }
#undef MS_BOUND
    MS_LAUNCH_CHECK("ms_sample_bound_kernel");
    return MS_OK;
}

// Sample pass: scan the first prepass_tiles tiles of every stream, merge, and leave the k-th
// best score per query in the workspace as the lower bound of the full pass (attach_prepass_results).
int run_prepass(const ScanPlan &pl, ScanParams *sp, int nq, char *ws, hipStream_t st) {
    if (pl.prepass_tiles <= 0) return MS_OK;
    const MsSettings &set = ms_settings();
    const int P = pl.d.P, qwb = pl.d.qwb;
    ScanParams s0 = *sp;
    s0.max_tiles = pl.prepass_tiles;
    s0.lb_s = nullptr;
    int rc = (s0.prefilter && s0.pf_image != nullptr) ? (is_f16_image(s0.pf_image, s0.pf_format) ? ms_launch_sample_pf16(pl, s0, st) : ms_launch_sample_pf2(pl, s0, st))
             : ((qwb == 4 && set.loader_wave) ? ms_launch_sample_loader(pl, s0, st) : launch_scan(pl, s0, st));
    if (rc) return rc;
    // the sample kernel leaves at most 2 entries per (query, stream) and merges the 4 / qwb streams of a workgroup: only the
    // first `ranks` entries of a list can be valid.  Their k-th largest value is the bound: no rows, no sorted list needed.
    int ranks = (2 * (4 / qwb) < s0.k) ? 2 * (4 / qwb) : s0.k;
    // (few query tiles: a workgroup's list holds the maxima of 4 / qwb streams; the best two or so per list bound nearly as
    //  well as all eight, and the selection below reads a quarter of the values: 12 -> 5 us)
    {
        const int enough = (s0.k + P - 1) / P;                 // ranks * P >= k values are needed for a bound at all
        const int cap = 512 / P > enough ? 512 / P : enough;
        if (ranks > cap) ranks = cap > 1 ? cap : 1;
    }
    // diagnostics / tuning: MS_BOUND_RANKS caps how many entries per sample list the bound selection reads (fewer = a cheaper, weaker bound)
    if (set.bound_ranks > 0 && set.bound_ranks < ranks && (int64_t)set.bound_ranks * P >= 4 * (int64_t)s0.k) ranks = set.bound_ranks;
    const int vpl = (ranks * P + 63) / 64;
    const size_t sm_stride = s0.list_sm ? (size_t)pl.d.nq_pad * s0.k : 0;       // (the image scans, and the loader-wave kernel where its merge allows, write stream-major lists)
    if (vpl > 32 && sm_stride != 0) MS_FAIL(MS_ERR_RANGE, "internal: %d sample lists of the image scan exceed the bound selection", P);
    if (vpl > 32) {      // too many values for one wave's selection: a merge, its outputs to scratch (no histogram: nothing zeroes its counters)
        rc = launch_merge(pl, s0, nq, s0.k, 0, pl.scr_s(ws), pl.scr_i(ws), s0.k, 0, pl.lb_s(ws), pl.lb_i(ws), st);
        if (rc) return rc;
        attach_prepass_results(pl, ws, sp, false);
        return MS_OK;
    }
    uint32_t *hist = pl.hist_on ? pl.hist(ws) : nullptr;
    rc = launch_sample_bound(s0.part_s, P, nq, s0.k, ranks, pl.lb_s(ws), hist, pl.hstep(ws), s0.gate, s0.gate_epoch, sm_stride, st);
    if (rc) return rc;
    attach_prepass_results(pl, ws, sp, pl.hist_on);
    return MS_OK;
}

// 4 rows per 256-thread workgroup, grid-stride beyond 65536 workgroups: the row-norm kernels
dim3 row_grid(int64_t n) {
    const int64_t blocks = (n + 3) / 4;
    return dim3((unsigned)(blocks < 65536 ? blocks : 65536));
}

// Prepare queries (+ inverse norms if absent) and fill ScanParams for the first pass.
int prepare_scan(const ScanPlan &pl, const float *db, int64_t n, const float *q, int nq, int mode,
                 const float *inv_norm, const float *lengths, const float *qlen, float mincov, char *ws,
                 hipStream_t st, ScanParams *sp) {
    if (!queries_used_in_place(q, mode, pl)) {
        const int rc = ms_launch_prepare_queries(q, nq, pl.d.nq_pad, mode, pl.qn(ws), st);
        if (rc) return rc;
    }
    if (mode == MS_MODE_COSINE_RAW && inv_norm == nullptr && n > 0) {
        hipLaunchKernelGGL(ms_row_inv_norms_kernel, row_grid(n), dim3(256), 0, st, db, n, 1e-8f, pl.inv(ws));
        MS_LAUNCH_CHECK("ms_row_inv_norms_kernel");
    }
    *sp = fill_scan_params(pl, db, n, q, nq, inv_norm, lengths, qlen, mincov, ws, mode);
    return MS_OK;
}

}  // namespace

extern "C" {

int ms_version(void) { return 210; }      // 200: pf_format in the prefilter entry points (round 5); 210: ms_device_pci_bus_id, ms_debug_prefilter_poison (round 6)
const char *ms_last_error(void) { return ms_err_buf; }

int ms_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

int ms_device_cu_count(void) { return cu_count_cached(); }

int ms_device_pci_bus_id(char *buf, int len) {
    if (buf == nullptr || len < 16) MS_FAIL(MS_ERR_ARG, "ms_device_pci_bus_id: need a buffer of >= 16 bytes");
    int dev = 0;
    MS_HIP_CHECK(hipGetDevice(&dev));
    MS_HIP_CHECK(hipDeviceGetPCIBusId(buf, len, dev));
    return MS_OK;
}

void ms_small_batch_thresholds(int *fused_merge_max_nq, int *inkernel_norm_max_nq) {
    if (fused_merge_max_nq != nullptr) *fused_merge_max_nq = ms_settings().fused_merge_max_nq;
    if (inkernel_norm_max_nq != nullptr) *inkernel_norm_max_nq = ms_settings().inkernel_norm_max_nq;
}
int ms_prefilter_max_k(void) { return MS_PREFILTER_MAX_K; }
int64_t ms_pf_few_min_rows(int nq) { return pf_few_min_rows(ms_settings(), nq); }

int ms_l2_normalize_rows(float *x, int64_t n, int d, float eps, ms_stream_t stream) {
    if (d != MS_DIM) MS_FAIL(MS_ERR_ARG, "ms_l2_normalize_rows: d must be %d (got %d)", MS_DIM, d);
    if (n < 0 || (n > 0 && x == nullptr)) MS_FAIL(MS_ERR_ARG, "ms_l2_normalize_rows: bad arguments");
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(ms_normalize_rows_kernel, row_grid(n), dim3(256), 0, (hipStream_t)stream, x, x, n, eps);
    MS_LAUNCH_CHECK("ms_normalize_rows_kernel");
    return MS_OK;
}

int ms_l2_normalize_rows_to(const float *x, float *y, int64_t n, int d, float eps, ms_stream_t stream) {
    if (d != MS_DIM) MS_FAIL(MS_ERR_ARG, "ms_l2_normalize_rows_to: d must be %d (got %d)", MS_DIM, d);
    if (n < 0 || (n > 0 && (x == nullptr || y == nullptr))) MS_FAIL(MS_ERR_ARG, "ms_l2_normalize_rows_to: bad arguments");
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(ms_normalize_rows_kernel, row_grid(n), dim3(256), 0, (hipStream_t)stream, x, y, n, eps);
    MS_LAUNCH_CHECK("ms_normalize_rows_kernel");
    return MS_OK;
}

int ms_row_inv_norms(const float *x, int64_t n, int d, float eps, float *inv_norm, ms_stream_t stream) {
    if (d != MS_DIM) MS_FAIL(MS_ERR_ARG, "ms_row_inv_norms: d must be %d (got %d)", MS_DIM, d);
    if (n < 0 || (n > 0 && (x == nullptr || inv_norm == nullptr))) MS_FAIL(MS_ERR_ARG, "ms_row_inv_norms: bad arguments");
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(ms_row_inv_norms_kernel, row_grid(n), dim3(256), 0, (hipStream_t)stream, x, n, eps, inv_norm);
    MS_LAUNCH_CHECK("ms_row_inv_norms_kernel");
    return MS_OK;
}

size_t ms_ip_topk_workspace_bytes(int64_t n, int nq, int k) {
    if (n < 0 || nq < 1 || k < 1) return 0;
    return make_plan(ms_settings(), cu_count_cached(), n, nq, k).total;
}

int ms_ip_topk_prepare(const float *db, int64_t n, const float *q, int nq, int k, int mode, const float *inv_norm,
                       const float *lengths, const float *qlen, float mincov, void *workspace, size_t workspace_bytes,
                       ms_stream_t stream) {
    ScanPlan pl;
    int rc = open_search(PREPARE, db, n, q, nq, k, mode, inv_norm, lengths, qlen, nullptr, nullptr, workspace, workspace_bytes, &pl);
    if (rc) return rc;
    ScanParams sp;
    rc = prepare_scan(pl, db, n, q, nq, mode, inv_norm, lengths, qlen, mincov, (char *)workspace, (hipStream_t)stream, &sp);
    if (rc) return rc;
    rc = run_prepass(pl, &sp, nq, (char *)workspace, (hipStream_t)stream);
    if (rc == MS_OK && sp.hist != nullptr) ms_wsstate::mark_clean(workspace, n, nq, k);      // (ms_sample_bound_kernel zeroed the counters)
    return rc;
}

int ms_ip_topk_scan(const float *db, int64_t n, const float *q, int nq, int k, int mode, const float *inv_norm,
                    const float *lengths, const float *qlen, float mincov, void *workspace, size_t workspace_bytes,
                    ms_stream_t stream) {
    ScanPlan pl;
    int rc = open_search(SCAN, db, n, q, nq, k, mode, inv_norm, lengths, qlen, nullptr, nullptr, workspace, workspace_bytes, &pl);
    if (rc) return rc;
    char *ws = (char *)workspace;
    // same parameters as ms_ip_topk_prepare left in the workspace (queries, inverse norms, lower bound, histogram)
    ScanParams sp = fill_scan_params(pl, db, n, q, nq, inv_norm, lengths, qlen, mincov, ws, mode);
    if (pl.prepass_tiles > 0) attach_prepass_results(pl, ws, &sp, pl.hist_on);
    rc = zero_hist_unless_clean(pl, sp, workspace, n, nq, k, (hipStream_t)stream);
    if (rc) return rc;
    return launch_scan(pl, sp, (hipStream_t)stream);
}

int ms_ip_topk_finish(int64_t n, int64_t row_offset, int nq, int k, float *out_scores, int64_t *out_idx,
                      void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    ScanPlan pl;
    const int rc = open_search(FINISH, nullptr, n, nullptr, nq, k, 0, nullptr, nullptr, nullptr, out_scores, out_idx, workspace, workspace_bytes, &pl);
    if (rc) return rc;
    ScanParams sp{};
    sp.part_s = pl.part_s(workspace);
    sp.part_i = pl.part_i(workspace);
    return launch_merge(pl, sp, nq, pl.k_pass, row_offset, out_scores, out_idx, k, 0, nullptr, nullptr, (hipStream_t)stream, nullptr, nullptr, 0,
                        pl.list_sm ? (size_t)pl.d.nq_pad * pl.k_pass : 0);
}

int ms_ip_topk(const float *db, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode,
               const float *inv_norm, const float *lengths, const float *qlen, float mincov, float *out_scores,
               int64_t *out_idx, void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    ScanPlan pl;
    int rc = open_search(WHOLE, db, n, q, nq, k, mode, inv_norm, lengths, qlen, out_scores, out_idx, workspace, workspace_bytes, &pl);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    ScanParams sp;
    rc = prepare_scan(pl, db, n, q, nq, mode, inv_norm, lengths, qlen, mincov, ws, st, &sp);
    if (rc) return rc;
    rc = run_prepass(pl, &sp, nq, ws, st);
    if (rc) return rc;
    ms_wsstate::invalidate(workspace);     // (a staged ms_ip_topk_scan on this workspace must not take the counters for clean afterwards)
    // a handful of queries, one pass: the scan launch merges its own lists (ms_scan_body, last workgroup of a query group)
    char *blk = (k <= 64 && pl.d.qwb < 4 && nq <= ms_settings().fused_merge_max_nq && merge_fits_scan_launch(pl.k_pass, pl.d.P))
                    ? ms_wsstate::block(ws) : nullptr;
    if (blk != nullptr) {
        sp.fin_s = out_scores; sp.fin_i = out_idx; sp.fin_row_offset = row_offset; sp.fin_stride = k;
        sp.ticket = reinterpret_cast<uint32_t *>(blk);
        return launch_scan(pl, sp, st);
    }
    // ceil(k / 64) passes; pass p returns ranks [64p, 64p + kp) using the last entry of pass
    // p-1 as an exclusive upper bound in the total order.
    for (int col0 = 0; col0 < k; col0 += 64) {
        const int kp = (k - col0) < 64 ? (k - col0) : 64;
        sp.k = kp;
        // the list stride inside the workspace is the pass's own k
        rc = launch_scan(pl, sp, st);
        if (rc) return rc;
        const bool more = col0 + 64 < k;
        rc = launch_merge(pl, sp, nq, kp, row_offset, out_scores, out_idx, k, col0, more ? pl.ub_s(ws) : nullptr,
                          more ? pl.ub_i(ws) : nullptr, st, nullptr, nullptr, 0, sp.list_sm ? (size_t)pl.d.nq_pad * kp : 0);
        if (rc) return rc;
        sp.ub_s = pl.ub_s(ws);
        sp.ub_i = pl.ub_i(ws);
    }
    return MS_OK;
}

// ---- prefiltered search (>= 3 query tiles, k <= 48) -------------------------------------------------------------------
namespace {
// Stage `stage` of the fp32 path: what a prefiltered call runs for shapes the prefilter does not serve
int fp32_stage(Stage stage, const float *db, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode, const float *lengths, const float *qlen,
               float mincov, float *out_scores, int64_t *out_idx, void *workspace, size_t workspace_bytes, hipStream_t st) {
    if (stage == PREPARE) return ms_ip_topk_prepare(db, n, q, nq, k, mode, nullptr, lengths, qlen, mincov, workspace, workspace_bytes, st);
    if (stage == SCAN) return ms_ip_topk_scan(db, n, q, nq, k, mode, nullptr, lengths, qlen, mincov, workspace, workspace_bytes, st);
    if (stage == FINISH) return ms_ip_topk_finish(n, row_offset, nq, k, out_scores, out_idx, workspace, workspace_bytes, st);
    return ms_ip_topk(db, n, row_offset, q, nq, k, mode, nullptr, lengths, qlen, mincov, out_scores, out_idx, workspace, workspace_bytes, st);
}
bool pf_format_ok(int f) { return f == MS_PF_BF16X3 || f == MS_PF_F16X2 || f == MS_PF_F16X1; }
float pf_err_coef(bool image, int format) {
    if (!is_f16_image(image, format)) return MS_PF_ERR;
    return format == MS_PF_F16X2 ? MS_PF_ERR_F16X2 : MS_PF_ERR_F16X1;
}
// A staged scan or finish (no stage 1 in the call) attaches the histogram wherever the shared bound is on.  That is NOT
// ScanPlan::hist_on, which stage 1 goes by: the two differ over an image with MS_LOADER_WAVE=0 (diagnostics), as they always have.
bool pf_staged_hist(const MsSettings &set) { return set.shared_bound != 0; }

int pf_run(Stage stages, const float *db, const void *image, int format, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode,
           const float *lengths, const float *qlen, float mincov, float row_norm_bound, float *out_scores, int64_t *out_idx,
           void *workspace, size_t workspace_bytes, hipStream_t st) {
    int rc = check_search_args(db, n, q, nq, k, mode, nullptr, lengths, qlen);
    if (rc) return rc;
    if (mode == MS_MODE_COSINE_RAW) MS_FAIL(MS_ERR_ARG, "ms_ip_topk_prefiltered: MS_MODE_COSINE_RAW is not served (normalise the rows once: MS_MODE_COSINE_UNIT)");
    if (image != nullptr && !pf_format_ok(format)) MS_FAIL(MS_ERR_ARG, "ms_ip_topk_prefiltered: unknown pf_format %d", format);
    const MsSettings &set = ms_settings();
    const PfLayout L = pf_layout(set, cu_count_cached(), n, nq, k, mode, image != nullptr, format);
    if (workspace == nullptr || workspace_bytes < L.total)
        MS_FAIL(MS_ERR_WORKSPACE, "ms_ip_topk_prefiltered: workspace %zu < %zu bytes", workspace_bytes, L.total);
    char *blk = L.ok && row_norm_bound > 0.0f && row_norm_bound < INFINITY ? ms_wsstate::block(workspace) : nullptr;
    if (blk == nullptr)            // shapes the prefilter does not serve: the fp32 path, same stages
        return fp32_stage(stages, db, n, row_offset, q, nq, k, mode, lengths, qlen, mincov, out_scores, out_idx, workspace, workspace_bytes, st);
    char *ws = (char *)workspace;
    const ScanPlan &pl = L.pf;
    const bool f16 = is_f16_image(image, format);
    // Raw queries over the fp16 image (MS_MODE_IP_NORMQ, MS_MODE_COSINE_UNIT; round 6): no query-preparation launch -- the sample pass and the
    // scan read the caller's array and normalise approximately in their set-up, the re-scoring launch normalises exactly (MS_PF_RAWQ=0: the
    // prepared copy as before)
    const float rawq_eps = (f16 && (mode == MS_MODE_IP_NORMQ || mode == MS_MODE_COSINE_UNIT) && ((uintptr_t)q & 15) == 0 && set.pf_rawq)
                               ? (mode == MS_MODE_IP_NORMQ ? 1e-12f : 1e-8f) : 0.0f;
    ScanParams sp;
    if ((stages & PREPARE) && rawq_eps == 0.0f) rc = prepare_scan(pl, db, n, q, nq, mode, nullptr, lengths, qlen, mincov, ws, st, &sp);
    else sp = fill_scan_params(pl, db, n, q, nq, nullptr, lengths, qlen, mincov, ws, mode);
    if (rc) return rc;
    if (rawq_eps > 0.0f) { sp.qn = q; sp.qnorm_eps = 0.0f; sp.qraw_eps = rawq_eps; }
    sp.prefilter = 1; sp.pf_image = image; sp.pf_format = format;
    if (stages & PREPARE) {
        rc = run_prepass(pl, &sp, nq, ws, st);
        if (rc) return rc;
        if (sp.hist != nullptr && (stages & SCAN)) ms_wsstate::invalidate(workspace);            // (the sample pass zeroed the counters: this call's scan uses
        else if (sp.hist != nullptr) ms_wsstate::mark_clean(workspace, n, nq, L.kp);             //  them up, or they are clean for a staged one)
    } else {
        if (pl.prepass_tiles > 0) attach_prepass_results(pl, ws, &sp, pf_staged_hist(set));
        if (stages & SCAN) rc = zero_hist_unless_clean(pl, sp, workspace, n, nq, L.kp, st);
        if (rc) return rc;
    }
    sp.debug_flags = set.pf_debug;
    if (stages & SCAN) {
        if (f16 && pl.d.n_qgroups >= 2 && pl.d.n_qgroups <= 16 && set.pf_pace) {
            // several query groups walk every row stream: they pace each other through progress words (ms_scan_pf16.h) so that a tile
            // one of them fetched is still in the XCD's L2 when the others want it
            sp.prog = pl.prog(ws);
            sp.prog_epoch = ms_wsstate::next_pace_epoch(workspace);
        }
        rc = launch_scan(pl, sp, st);
        if (rc) return rc;
    }
    if (stages & FINISH) {
        if (out_scores == nullptr || out_idx == nullptr) MS_FAIL(MS_ERR_ARG, "ms_ip_topk_prefiltered: NULL outputs");
        uint32_t *gate = reinterpret_cast<uint32_t *>(blk + ms_wsstate::GATE_OFFSET);
        const uint32_t epoch = ms_wsstate::next_gate_epoch(workspace);
        const ScanPlan &px = L.exact;
        PfCompact cp;
        cp.qn_c = L.qn_c(ws); cp.lb_c = L.lb_c(ws); cp.qlen_c = L.qlen_c(ws); cp.qmap = L.qmap(ws); cp.dp = L.dp(ws); cp.gate = gate; cp.epoch = epoch; cp.n = n;
        cp.cus = cu_count_cached(); cp.nq = nq; cp.ticket_base = ms_wsstate::peek_tickets(workspace);
        // ONE launch: merge of the per-stream candidate lists (sparse; stream-major behind the image scans) + exact re-scoring + proof + compaction
        PfRescore ra;
        ra.db = db; ra.qn = sp.qn; ra.as = L.as(ws); ra.ai = L.ai(ws); ra.lengths = lengths; ra.qlen = qlen; ra.out_s = out_scores; ra.out_i = out_idx; ra.flag = L.flag(ws);
        ra.row_offset = row_offset; ra.err_coef = pf_err_coef(image != nullptr, format) * row_norm_bound; ra.mincov = mincov;
        ra.q_eps = rawq_eps;
        ra.k = k; ra.kp = L.kp; ra.fp16_range = f16 ? 1 : 0; ra.cp = cp;
        if (!block_merge_takes(L.kp, pl.d.P)) MS_FAIL(MS_ERR_RANGE, "internal: %d candidate lists of %d entries exceed the merge", pl.d.P, L.kp);
        const size_t block_lds = block_merge_lds(L.kp, pl.d.P);
        if (block_lds > 48 * 1024)
            MS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(ms_merge_rescore_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)block_lds));
        hipLaunchKernelGGL(ms_merge_rescore_kernel, dim3(nq), dim3(256), block_lds, st, sp.part_s, sp.part_i, pl.d.P, L.as(ws), L.ai(ws),
                           sp.list_sm ? (size_t)pl.d.nq_pad * L.kp : (size_t)0, ra);
        MS_LAUNCH_CHECK("ms_merge_rescore_kernel");
        ms_wsstate::commit_tickets(workspace, (uint32_t)nq);       // (only now: a failing return above leaves the host's total where the device word is)
        // The exact pass, for the flagged queries ONLY (the reference's semantics are per query: dbsearch.py:234-242): an fp32 scan
        // and a merge over the compacted batch, decomposed on the device (ScanDevPlan), both returning at once when no query was
        // flagged.  No sample pass: the k-th best exact score among a query's candidates is already a lower bound on its k-th
        // best (k rows score at least that), and a tight one.  Always the kernels for any number of query tiles (ms_scan_kernel).
        ScanParams sx = fill_scan_params(px, db, n, q, nq, nullptr, lengths, lengths != nullptr ? cp.qlen_c : nullptr, mincov, ws, mode);
        sx.qn = cp.qn_c;                     // (prepared -- normalised where the mode asks for it -- by the prefilter's stage 1)
        sx.qnorm_eps = 0.0f;
        sx.gate = gate; sx.gate_epoch = epoch;
        sx.lb_s = cp.lb_c;
        sx.dev_plan = cp.dp;
        sx.part_s = L.xs(ws);
        sx.part_i = L.xi(ws);
        ScanPlan pg = px;
        pg.d.grid = L.exact_grid_max; pg.d.P = L.exact_P_max; pg.d.qwb = 1;     // (qwb = 1: routes to ms_scan_kernel, whose decomposition is the device plan's)
        sx.qwb = 1;
        sx.list_sm = 0;                      // (ms_scan_kernel writes rank-major lists)
        // A handful of queries (the reference's own CLI regime over the fp16 image of a large database; round 6): the exact pass merges
        // inside its own launch -- the last workgroup of the query group, as ms_ip_topk does for such batches -- so that ONE gated launch
        // follows the re-scoring instead of two (each costs ~5 us even when it returns at once).  More queries: the last workgroup would
        // merge them one after the other (4.4 us each) while 255 others have finished; the merge launch stays.
        // (up to 8 queries whatever ms_ip_topk's own threshold is: the serial merge only runs for queries that were flagged -- rare -- while the
        //  second launch costs every call; MS_PF_FUSE_EXACT_MAX_NQ overrides)
        const bool fuse_exact = nq <= set.pf_fuse_exact_max_nq && merge_fits_scan_launch(px.k_pass, L.exact_P_max);
        if (fuse_exact) {
            sx.fin_s = out_scores; sx.fin_i = out_idx; sx.fin_row_offset = row_offset; sx.fin_stride = k; sx.fin_qmap = cp.qmap;
            sx.ticket = reinterpret_cast<uint32_t *>(blk);
        }
        rc = launch_scan(pg, sx, st);
        if (rc) return rc;
        if (!fuse_exact) {
            rc = launch_merge(pg, sx, nq, px.k_pass, row_offset, out_scores, out_idx, k, 0, nullptr, nullptr, st, cp.dp, cp.qmap);
            if (rc) return rc;
        }
    }
    return MS_OK;
}
}  // namespace

size_t ms_pf_image_bytes(int64_t n, int pf_format) {
    if (n < 0 || !pf_format_ok(pf_format)) return 0;
    if (pf_format == MS_PF_BF16X3) return (size_t)((n + 31) / 32) * 16384;
    return (size_t)((n + 63) / 64) * 16384 + 256;          // (+ the trailer the scan checks: magic, scale exponent, n)
}
float ms_pf_err_coef(int pf_format) { return pf_format_ok(pf_format) ? pf_err_coef(true, pf_format) : -1.0f; }

int ms_pf_build_image(const float *db, int64_t n, int pf_format, float row_norm_bound, void *image, ms_stream_t stream) {
    if (!pf_format_ok(pf_format)) MS_FAIL(MS_ERR_ARG, "ms_pf_build_image: unknown pf_format %d", pf_format);
    if (n < 0 || (n > 0 && db == nullptr) || image == nullptr) MS_FAIL(MS_ERR_ARG, "ms_pf_build_image: bad arguments");
    if (((uintptr_t)image & 15) != 0 || ((uintptr_t)db & 15) != 0) MS_FAIL(MS_ERR_ARG, "ms_pf_build_image: db and image must be 16-byte aligned");
    if (pf_format == MS_PF_BF16X3) {
        if (n == 0) return MS_OK;
        return ms_launch_pf_build_image(db, n, image, (hipStream_t)stream);
    }
    // fp16: every component of row * 2^sr must sit below 2^15 -- sr from the bound on the rows' norms
    if (!(row_norm_bound >= 9.094947e-13f && row_norm_bound <= 1.0995116e12f))
        MS_FAIL(MS_ERR_RANGE, "ms_pf_build_image: the fp16 image needs a row-norm bound in [2^-40, 2^40] (got %g): use MS_PF_BF16X3", (double)row_norm_bound);
    const int sr = 14 - ilogbf(row_norm_bound);
    return ms_launch_pf16_build_image(db, n, sr, image, (hipStream_t)stream);
}

size_t ms_ip_topk_prefiltered_workspace_bytes(int64_t n, int nq, int k) {
    if (n < 0 || nq < 1 || k < 1) return 0;
    return pf_workspace_bytes(ms_settings(), cu_count_cached(), n, nq, k);
}

int ms_ip_topk_prefiltered(const float *db, const void *pf_image, int pf_format, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode,
                           const float *lengths, const float *qlen, float mincov, float row_norm_bound, float *out_scores,
                           int64_t *out_idx, void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    if (k > 64) return ms_ip_topk(db, n, row_offset, q, nq, k, mode, nullptr, lengths, qlen, mincov, out_scores, out_idx, workspace, workspace_bytes, stream);
    return pf_run(WHOLE, db, pf_image, pf_format, n, row_offset, q, nq, k, mode, lengths, qlen, mincov, row_norm_bound, out_scores, out_idx, workspace,
                  workspace_bytes, (hipStream_t)stream);
}
int ms_ip_topk_prefiltered_prepare(const float *db, const void *pf_image, int pf_format, int64_t n, const float *q, int nq, int k, int mode,
                                   const float *lengths, const float *qlen, float mincov, float row_norm_bound, void *workspace,
                                   size_t workspace_bytes, ms_stream_t stream) {
    return pf_run(PREPARE, db, pf_image, pf_format, n, 0, q, nq, k, mode, lengths, qlen, mincov, row_norm_bound, nullptr, nullptr, workspace, workspace_bytes,
                  (hipStream_t)stream);
}
int ms_ip_topk_prefiltered_scan(const float *db, const void *pf_image, int pf_format, int64_t n, const float *q, int nq, int k, int mode,
                                const float *lengths, const float *qlen, float mincov, float row_norm_bound, void *workspace,
                                size_t workspace_bytes, ms_stream_t stream) {
    return pf_run(SCAN, db, pf_image, pf_format, n, 0, q, nq, k, mode, lengths, qlen, mincov, row_norm_bound, nullptr, nullptr, workspace, workspace_bytes,
                  (hipStream_t)stream);
}
int ms_ip_topk_prefiltered_finish(const float *db, const void *pf_image, int pf_format, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode,
                                  const float *lengths, const float *qlen, float mincov, float row_norm_bound, float *out_scores,
                                  int64_t *out_idx, void *workspace, size_t workspace_bytes, ms_stream_t stream) {
    return pf_run(FINISH, db, pf_image, pf_format, n, row_offset, q, nq, k, mode, lengths, qlen, mincov, row_norm_bound, out_scores, out_idx, workspace,
                  workspace_bytes, (hipStream_t)stream);
}
// Diagnostics for the tests (synchronises the device): the state the last prefiltered search on this workspace left behind --
// *flagged = how many of its queries needed the exact pass (0: the prefilter proved every answer).
int ms_debug_prefilter_state(void *workspace, unsigned int *gate_value, unsigned int *last_epoch, unsigned int *flagged) {
    char *blk = ms_wsstate::block(workspace);
    if (blk == nullptr || hipDeviceSynchronize() != hipSuccess) return -1;
    unsigned int w[3] = {0, 0, 0};
    if (hipMemcpy(w, blk + ms_wsstate::GATE_OFFSET, 12, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    *gate_value = w[0]; *last_epoch = w[1]; *flagged = w[2];
    return 0;
}

// Diagnostics for the tests (synchronises the device): overwrite the two counters of the compaction in the library-owned block of
// this workspace -- what an aborted launch, or a second stream on the same workspace, would leave behind.  The next prefiltered
// search on the workspace must then fail loudly (the gated launch traps: ms_gate_closed), never answer.
int ms_debug_prefilter_poison(void *workspace, unsigned int slot_counter, unsigned int ticket) {
    char *blk = ms_wsstate::block(workspace);
    if (blk == nullptr || hipDeviceSynchronize() != hipSuccess) return -1;
    const unsigned int w[2] = {slot_counter, ticket};
    if (hipMemcpy(blk + ms_wsstate::GATE_OFFSET + 16, w, 8, hipMemcpyHostToDevice) != hipSuccess) return -1;
    return 0;
}

// Diagnostics (tools/pf_try.py): the candidate lists (approximate scores, rows) the last prefiltered search left in the workspace.
int ms_debug_prefilter_lists(void *workspace, int64_t n, int nq, int k, int image, float *as_host, int64_t *ai_host, int *kp_out) {
    // image: 0 = none, 1 = split-bf16 image, 2 = fp16 image (the layouts differ in their tile size only)
    const PfLayout L = pf_layout(ms_settings(), cu_count_cached(), n, nq, k, MS_MODE_IP_PRENORM, image != 0, image == 2 ? MS_PF_F16X2 : MS_PF_BF16X3);
    if (!L.ok || hipDeviceSynchronize() != hipSuccess) return -1;
    *kp_out = L.kp;
    if (hipMemcpy(as_host, L.as(workspace), (size_t)nq * L.kp * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(ai_host, L.ai(workspace), (size_t)nq * L.kp * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

// Test hook: launch_merge on lists the caller wrote (include/merizo_search_amd.h; tests/merge_case.py).  The plan and the parameters
// carry what launch_merge reads of them -- the list count, the lists, no gate -- so the form launched is the one a search of that
// (P, k) gets.
int ms_debug_merge_lists(const float *part_s, const unsigned int *part_i, int P, int nq, int k, int sm_nq_pad, int sparse, int64_t row_offset,
                         float *out_s, int64_t *out_i, int out_stride, int col0, float *ub_s, unsigned int *ub_i, int dp_nq, int dp_P,
                         const int *qmap, void *dp_scratch, ms_stream_t stream) {
    if (part_s == nullptr || part_i == nullptr || out_s == nullptr || out_i == nullptr || (ub_s == nullptr) != (ub_i == nullptr))
        MS_FAIL(MS_ERR_ARG, "ms_debug_merge_lists: NULL lists or outputs, or only one of ub_s / ub_i");
    if ((((uintptr_t)part_s | (uintptr_t)part_i) & 15) != 0) MS_FAIL(MS_ERR_ARG, "ms_debug_merge_lists: the lists must be 16-byte aligned");
    if (k < 1 || k > 64 || nq < 1 || P < 1 || col0 < 0 || out_stride < col0 + k || sm_nq_pad < 0 || (sm_nq_pad > 0 && sm_nq_pad < nq))
        MS_FAIL(MS_ERR_ARG, "ms_debug_merge_lists: need 1 <= k <= 64, nq >= 1, P >= 1, out_stride >= col0 + k, sm_nq_pad 0 or >= nq (P=%d nq=%d k=%d)", P, nq, k);
    if (dp_scratch == nullptr ? qmap != nullptr : (dp_nq < 1 || dp_nq > nq || dp_P < 1 || dp_P > P || sm_nq_pad != 0))
        MS_FAIL(MS_ERR_ARG, "ms_debug_merge_lists: qmap without a device plan, or a plan outside its launch (dp_nq=%d nq=%d dp_P=%d P=%d)", dp_nq, nq, dp_P, P);
    const hipStream_t st = (hipStream_t)stream;
    ScanPlan pl{};
    ScanParams sp{};
    pl.d.P = P;
    sp.part_s = const_cast<float *>(part_s); sp.part_i = const_cast<uint32_t *>(part_i);      // (the merges only read them)
    if (dp_scratch != nullptr) {
        if (!block_merge_takes(k, P))       // (what launch_merge answers: nothing is written to the scratch for a launch that does not happen)
            return launch_merge(pl, sp, nq, k, row_offset, out_s, out_i, out_stride, col0, ub_s, ub_i, st, static_cast<const ScanDevPlan *>(dp_scratch), qmap);
        static_assert(sizeof(ScanDevPlan) == 64, "the hook's scratch is 64 bytes");
        char *d = static_cast<char *>(dp_scratch);
        MS_HIP_CHECK(hipMemsetAsync(d, 0, sizeof(ScanDevPlan), st));
        MS_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d + offsetof(ScanDevPlan, nq)), dp_nq, 1, st));
        MS_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d + offsetof(ScanDevPlan, P)), dp_P, 1, st));
    }
    return launch_merge(pl, sp, nq, k, row_offset, out_s, out_i, out_stride, col0, ub_s, ub_i, st, static_cast<const ScanDevPlan *>(dp_scratch), qmap,
                        sparse != 0 ? 1 : 0, sm_nq_pad > 0 ? (size_t)sm_nq_pad * k : 0);
}

// Test hook: the bound selection of a sample pass on lists the caller wrote (run_prepass launches the same function)
int ms_debug_sample_bound(const float *part_s, int P, int nq, int k, int ranks, int sm_nq_pad, float *lb, unsigned int *hist, float *hstep,
                          ms_stream_t stream) {
    if (part_s == nullptr || lb == nullptr || (hist == nullptr) != (hstep == nullptr))
        MS_FAIL(MS_ERR_ARG, "ms_debug_sample_bound: NULL lists or bound, or only one of hist / hstep");
    if (k < 1 || k > 64 || nq < 1 || P < 1 || sm_nq_pad < 0 || (sm_nq_pad > 0 && sm_nq_pad < nq))
        MS_FAIL(MS_ERR_ARG, "ms_debug_sample_bound: need 1 <= k <= 64, nq >= 1, P >= 1, sm_nq_pad 0 or >= nq (P=%d nq=%d k=%d)", P, nq, k);
    if (ranks < 1 || ranks > k || (int64_t)ranks * P > 2048)
        MS_FAIL(MS_ERR_RANGE, "ms_debug_sample_bound: need 1 <= ranks <= k and ranks * P <= 2048 (ranks=%d P=%d k=%d)", ranks, P, k);
    return launch_sample_bound(part_s, P, nq, k, ranks, lb, hist, hstep, nullptr, 0u, sm_nq_pad > 0 ? (size_t)sm_nq_pad * k : 0, (hipStream_t)stream);
}

// S sorted lists per query, list s of each array s * stride BYTES behind list 0 -> the best k (both merge entry points)
static int kway_merge(const char *who, bool strided, const float *scores, const int64_t *idx, int64_t score_stride_bytes, int64_t idx_stride_bytes,
                      int S, int nq, int k, float *out_scores, int64_t *out_idx, ms_stream_t stream) {
    if (S < 1 || nq < 1 || k < 1 || !scores || !idx || !out_scores || !out_idx)
        MS_FAIL(MS_ERR_ARG, "%s: need S >= 1, nq >= 1, k >= 1 and non-NULL buffers (S=%d)", who, S);
    if (strided && (score_stride_bytes % 4 != 0 || idx_stride_bytes % 8 != 0 || ((uintptr_t)idx & 7) != 0))
        MS_FAIL(MS_ERR_ARG, "%s: strides / index pointer must keep float32 and int64 alignment", who);
    if (S <= 64)
        hipLaunchKernelGGL(ms_kway_merge_kernel, dim3((nq + 63) / 64), dim3(64), 0, (hipStream_t)stream, scores, idx,
                           score_stride_bytes, idx_stride_bytes, S, nq, k, out_scores, out_idx);
    else
        hipLaunchKernelGGL(ms_kway_merge_any_kernel, dim3((nq + 63) / 64), dim3(64), 0, (hipStream_t)stream, scores, idx,
                           score_stride_bytes, idx_stride_bytes, S, nq, k, out_scores, out_idx);
    MS_LAUNCH_CHECK("ms_kway_merge_kernel");
    return MS_OK;
}

int ms_topk_merge(const float *scores, const int64_t *idx, int S, int nq, int k, float *out_scores,
                  int64_t *out_idx, ms_stream_t stream) {
    return kway_merge("ms_topk_merge", false, scores, idx, (int64_t)nq * k * 4, (int64_t)nq * k * 8, S, nq, k, out_scores, out_idx, stream);
}

int ms_topk_merge_strided(const float *scores, const int64_t *idx, int64_t score_stride_bytes, int64_t idx_stride_bytes,
                          int S, int nq, int k, float *out_scores, int64_t *out_idx, ms_stream_t stream) {
    return kway_merge("ms_topk_merge_strided", true, scores, idx, score_stride_bytes, idx_stride_bytes, S, nq, k, out_scores, out_idx, stream);
}

}  // extern "C"
