// What the units that put the 16-bit matrix pipe in front of the exact cell share (ms_md_scan_mq.hip: chain verdicts;
// ms_edges.hip: the cells themselves): the query operands and thresholds, the staged fp32 tile and its A operands, the filter
// loop over a wave's query tiles (ms_mq_cells), the exact cell and the pick of one accumulator register; on the host what a call
// derives from its row-norm bound, the front of the workspace and the launches that fill it.  The error bound behind the
// threshold is derived in ms_md_scan_mq.hip.
// The kernel is static: every unit that includes this header gets its own copy.
#pragma once
#include "ms_md_scan.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define MS_MQ_LIST 256                       // unproved cells per wave between two drains
#define MS_MQ_NORM_MIN 9.094947e-13f         // 2^-40 and
#define MS_MQ_NORM_MAX 1.0995116e12f         // 2^40: a row-norm bound or a query norm outside them proves nothing

// Per prepared query: the fp16 operand, and the threshold in the accumulators' domain (+inf for the padding behind nq: proved zero;
// -inf for a query every cell of which goes to the exact chain).  eb = E * B.  Thread 0 resets the re-score count.
static __global__ __launch_bounds__(256) void ms_md_scan_mq_prep_kernel(const float *__restrict__ qn, int nq, int nq_pad, float min_score, float eb,
                                                                        int sr, _Float16 *__restrict__ qh, float *__restrict__ thr,
                                                                        ms_u64 *__restrict__ ctl) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q == 0) ctl[2] = 0ull;
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
    if (q < nq) {
        const float nrm = sqrtf(ss);
        const bool flagged = !(ss > 0.0f && ss < INFINITY) || !(nrm >= MS_MQ_NORM_MIN && nrm <= MS_MQ_NORM_MAX);
        t = min_score - eb * (nrm * (1.0f + 1e-5f));
        if (t > -INFINITY && t < INFINITY) t = t - fabsf(t) * 2.3841858e-7f;
        t = ldexpf(t, sr + sq);
        if (flagged || !(fabsf(t) >= 7.888609e-31f)) t = -INFINITY;          // (NaN, zero or below 2^-100: nothing is proved)
    }
    thr[q] = t;
}

// Rows [r0, r0 + nrows) (nrows <= 64) -> the fp32 tile (zero rows behind nrows), their mask limits and their flags.
__device__ __forceinline__ void ms_mq_stage(const float *__restrict__ db, int64_t r0, int nrows, const float *__restrict__ lengths, float mincov,
                                            float b2, f32x4 *tile, float *lim, uint32_t *rflag, int tid) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(db + (size_t)r0 * MS_DIM);
    const int nf4 = nrows * (MS_DIM / 4);
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();                                                       // the previous tile has been read
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int f = u * 256 + tid;
        v[u] = f < nf4 ? src[f] : zero;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int f = u * 256 + tid;
        tile[(f >> 5) * MS_MDS_ROW_F4 + (f & 31)] = v[u];
    }
    if (tid < MS_MDS_TILE) lim[tid] = (lengths != nullptr && tid < nrows) ? lengths[r0 + tid] * mincov : 0.0f;
    __syncthreads();
    // four threads per row: a quarter of the sum of squares each
    const int row = tid >> 2, part = tid & 3;
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x4 t = tile[row * MS_MDS_ROW_F4 + 8 * part + j];
        ss += t.x * t.x; ss += t.y * t.y; ss += t.z * t.z; ss += t.w * t.w;
    }
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
    if (part == 0) rflag[row] = (ss <= b2) ? 0u : 1u;                       // (NaN and inf are flagged)
    __syncthreads();
}

// The staged tile -> a wave's two 32-row A operands [half][k block] (r = lane & 31: the row of the half, h = lane >> 5: the half
// of each k block), scaled by rscale = 2^sr, clamped, rounded to nearest even; NaN for a flagged row.
__device__ __forceinline__ void ms_mq_convert(const f32x4 *tile, const uint32_t *rflag, float rscale, int r, int h, f16x8 (&af)[2][8]) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const int row = 32 * hf + r;
        const bool fl = rflag[row] != 0u;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const f32x4 a0 = tile[row * MS_MDS_ROW_F4 + 16 * h + 2 * b] * rscale, a1 = tile[row * MS_MDS_ROW_F4 + 16 * h + 2 * b + 1] * rscale;
            const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const _Float16 v = (_Float16)fminf(fmaxf(x[e], -65504.0f), 65504.0f);      // round to nearest even
                af[hf][b][e] = fl ? (_Float16)__builtin_nanf("") : v;
            }
        }
    }
}

// The exact cell of ms_md_chain_scan for (prepared query qv, staged row): the chain s = 0..63: element s, then element 64 + s.
__device__ __forceinline__ float ms_mq_exact(const float *__restrict__ qv, const f32x4 *row) {
    const f32x4 *q4 = reinterpret_cast<const f32x4 *>(qv);
    float acc = 0.0f;
#pragma unroll 2
    for (int j = 0; j < 16; ++j) {                                         // (two steps in flight: the drain runs inside the cells' registers)
        const f32x4 qa = q4[j], qb = q4[16 + j], ra = row[j], rb = row[16 + j];
        acc = fmaf(qa.x, ra.x, acc); acc = fmaf(qb.x, rb.x, acc);
        acc = fmaf(qa.y, ra.y, acc); acc = fmaf(qb.y, rb.y, acc);
        acc = fmaf(qa.z, ra.z, acc); acc = fmaf(qb.z, rb.z, acc);
        acc = fmaf(qa.w, ra.w, acc); acc = fmaf(qb.w, rb.w, acc);
    }
    return acc;
}

// Register i (uniform) of two accumulators: a select tree under scalar masks (a dynamic index would go through scratch memory).
__device__ __forceinline__ float ms_mq_select(const f32x16 &lo, const f32x16 &hi, int i) {
    const uint64_t m0 = (i & 1) ? ~0ull : 0ull, m1 = (i & 2) ? ~0ull : 0ull, m2 = (i & 4) ? ~0ull : 0ull, m3 = (i & 8) ? ~0ull : 0ull,
                   m4 = (i & 16) ? ~0ull : 0ull;
    float l0[16], l1[8], l2[4], l3[2], out;
#define MS_SEL(D, A, B, M) asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(D) : "v"(A), "v"(B), "s"(M))
#pragma unroll
    for (int j = 0; j < 16; ++j) l0[j] = m4 ? hi[j] : lo[j];          // (the accumulators may live in AGPRs: no asm operand)
#pragma unroll
    for (int j = 0; j < 8; ++j) MS_SEL(l1[j], l0[2 * j], l0[2 * j + 1], m0);
#pragma unroll
    for (int j = 0; j < 4; ++j) MS_SEL(l2[j], l1[2 * j], l1[2 * j + 1], m1);
    MS_SEL(l3[0], l2[0], l2[1], m2); MS_SEL(l3[1], l2[2], l2[3], m2);
    MS_SEL(out, l3[0], l3[1], m3);
#undef MS_SEL
    return out;
}

// Every query tile a wave owns (tiles wave, wave + 4, ... of the nqt tiles of 32 queries that begin at query q0) against the wave's A
// operands of a staged tile of nrows rows: 2 x 8 v_mfma_f32_32x32x16_f16 per query tile, every accumulator compared with thr[q].
// A cell that is not proved below the cut is appended to the wave's list -- entry(slot, ql, row) writes it in the unit's own
// encoding, ql = q - q0 -- and drain() empties the list (it sets cnt = 0) when fewer than 64 slots are left, and once at the end.
template <typename Entry, typename Drain>
__device__ __forceinline__ void ms_mq_cells(const f16x8 (&af)[2][8], const _Float16 *__restrict__ qh, const float *__restrict__ thr, int q0,
                                            int nqt, int nrows, int nq, int wave, int lane, int &cnt, Entry entry, Drain drain) {
    const int r = lane & 31, h = lane >> 5;
    // the B operand and threshold of query tile t: requested one tile ahead (an L2 round trip per tile otherwise)
    f16x8 bn[8];
    float thn = INFINITY;
    auto request = [&](int t) __attribute__((always_inline)) {
        const int q = q0 + 32 * t + r;
        const f16x8 *bsrc = reinterpret_cast<const f16x8 *>(qh + (size_t)q * MS_DIM + 64 * h);
#pragma unroll
        for (int b = 0; b < 8; ++b) bn[b] = bsrc[b];
        thn = thr[q];
    };
    if (wave < nqt) request(wave);
    for (int qt = wave; qt < nqt; qt += 4) {
        const int ql = 32 * qt + r, q = q0 + ql;
        f16x8 bq[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) bq[b] = bn[b];
        const float th = thn;
        if (qt + 4 < nqt) request(qt + 4);
        f32x16 o0 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, o1 = o0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0][b], bq[b], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1][b], bq[b], o1, 0, 0, 0);
        }
        // register 4 g + j of half hf: row 32 hf + 8 g + 4 h + j, query r.  PROVED BELOW THE CUT iff a < th (never for a NaN a).
        bool open = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) open = open || !(o0[i] < th) || !(o1[i] < th);
        if (__ballot(open) == 0ull) continue;
        uint32_t regs = 0u;                                                      // registers with an unproved cell (uniform)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            regs |= (__ballot(!(o0[i] < th)) != 0ull ? 1u : 0u) << i;
            regs |= (__ballot(!(o1[i] < th)) != 0ull ? 1u : 0u) << (16 + i);
        }
#pragma unroll 1
        while (regs != 0u) {
            const int i = __builtin_ctz(regs);
            regs &= regs - 1u;
            const float a = ms_mq_select(o0, o1, i);
            const int row = 32 * (i >> 4) + 8 * ((i & 15) >> 2) + 4 * h + (i & 3);
            const bool pass = !(a < th) && row < nrows && q < nq;
            const ms_u64 pm = __ballot(pass);
            if (pass) entry(cnt + __popcll(pm & ms_mds_low_bits(lane)), ql, row);
            cnt += __popcll(pm);
            if (cnt > MS_MQ_LIST - 64) drain();
        }
    }
    drain();
}

// The re-score count of a kernel (nresc: the cells this lane sent to the exact chain): one add per wave.
__device__ __forceinline__ void ms_mq_count_rescored(uint32_t nresc, int lane, ms_u64 *__restrict__ ctl) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nresc += __shfl_xor(nresc, off);
    if (lane == 0 && nresc != 0u) atomicAdd(&ctl[2], (ms_u64)nresc);
}

static inline int ms_mq_pad(int nq) { return (int)(((int64_t)nq + 31) / 32 * 32); }

// What the host hands the prep launch and the scan for a row-norm bound B in [2^-40, 2^40]: the row scaling's exponent sr and the
// scaling rscale = 2^sr itself, the margin per unit of |q| eb = E * B with E = ms_pf_err_coef(MS_PF_F16X1), and the sum of squares
// b2 up to which a row counts as bounded.
struct ms_mq_params {
    int sr;
    float eb, b2, rscale;
};

static inline bool ms_mq_bound_ok(float row_norm_bound) { return row_norm_bound >= MS_MQ_NORM_MIN && row_norm_bound <= MS_MQ_NORM_MAX; }

static inline ms_mq_params ms_mq_derive(float row_norm_bound) {
    ms_mq_params p;
    p.sr = 14 - ilogbf(row_norm_bound);
    p.eb = ms_pf_err_coef(MS_PF_F16X1) * row_norm_bound;
    p.b2 = row_norm_bound * row_norm_bound * (1.0f + 1e-5f);
    p.rscale = ldexpf(1.0f, p.sr);
    return p;
}

#define MS_MQ_CHECK_BOUND(NAME)                                                                                                   \
    do {                                                                                                                          \
        if (!ms_mq_bound_ok(row_norm_bound))                                                                                      \
            MS_FAIL(MS_ERR_RANGE, NAME ": the fp16 operands need a row-norm bound in [2^-40, 2^40] (got %g)", (double)row_norm_bound); \
    } while (0)

// The front of both units' workspaces: prepared queries [nq_pad][128] fp32 | their fp16 operands [nq_pad][128] | thresholds
// [nq_pad], padded to 16 bytes; `tail` is the first byte behind them (the unit's own words).
struct ms_mq_ws {
    float *qn;
    _Float16 *qh;
    float *thr;
    char *tail;
};

static inline size_t ms_mq_ws_bytes(size_t nq_pad) {
    return nq_pad * MS_DIM * (sizeof(float) + sizeof(_Float16)) + ms_align_up(nq_pad * sizeof(float), 16);
}

static inline ms_mq_ws ms_mq_carve(void *workspace, int nq_pad) {
    ms_mq_ws w;
    w.qn = (float *)workspace;
    w.qh = (_Float16 *)(w.qn + (size_t)nq_pad * MS_DIM);
    w.thr = (float *)(w.qh + (size_t)nq_pad * MS_DIM);
    w.tail = (char *)workspace + ms_mq_ws_bytes((size_t)nq_pad);
    return w;
}

// The launches that fill that front: the prepared queries (only when the call has work), then their operands and thresholds.
// (The second launch runs in every call, over no query when there is no work: it resets the re-score count ctl[2].)
static inline int ms_mq_launch_operands(const float *q, int nq, int nq_pad, int mode, bool work, float min_score, const ms_mq_params &p,
                                        const ms_mq_ws &w, ms_u64 *ctl, hipStream_t st) {
    if (work) {
        const int rc = ms_launch_prepare_queries(q, nq, nq_pad, mode, w.qn, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ms_md_scan_mq_prep_kernel, dim3((unsigned)(work ? (nq_pad + 255) / 256 : 1)), dim3(256), 0, st, w.qn, nq,
                       work ? nq_pad : 0, min_score, p.eb, p.sr, w.qh, w.thr, ctl);
    MS_LAUNCH_CHECK("ms_md_scan_mq_prep_kernel");
    return MS_OK;
}
