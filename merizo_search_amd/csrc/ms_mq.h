// What the units that put the 16-bit matrix pipe in front of the exact cell share (ms_md_scan_mq.hip: chain verdicts;
// ms_edges.hip: the cells themselves): the query operands and thresholds, the staged fp32 tile and its A operands, the exact
// cell and the pick of one accumulator register.  The error bound behind the threshold is derived in ms_md_scan_mq.hip.
// The kernel is static: every unit that includes this header gets its own copy.
#pragma once
#include "ms_md_scan.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define MS_MQ_LIST 256                       // unproved cells per wave between two drains

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
        const bool flagged = !(ss > 0.0f && ss < INFINITY) || !(nrm >= 9.094947e-13f && nrm <= 1.0995116e12f);
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

static inline int ms_mq_pad(int nq) { return (int)(((int64_t)nq + 31) / 32 * 32); }

// What the host hands the prep launch and the scan for a row-norm bound B in [2^-40, 2^40]: the row scaling's exponent sr, the
// margin per unit of |q| eb = E * B with E = ms_pf_err_coef(MS_PF_F16X1), and the sum of squares up to which a row counts as bounded.
static inline bool ms_mq_bound_ok(float row_norm_bound) { return row_norm_bound >= 9.094947e-13f && row_norm_bound <= 1.0995116e12f; }
static inline int ms_mq_sr(float row_norm_bound) { return 14 - ilogbf(row_norm_bound); }
static inline float ms_mq_eb(float row_norm_bound) { return ms_pf_err_coef(MS_PF_F16X1) * row_norm_bound; }
static inline float ms_mq_b2(float row_norm_bound) { return row_norm_bound * row_norm_bound * (1.0f + 1e-5f); }
