/* The cell score of ms_md_chain_scores as a true fmaf chain -- TEST INFRASTRUCTURE (tests/multidom_case.py builds and binds it).
 * A float64 emulation of fma would round twice (53 bits, then 24) and disagree in rare bits; fmaf rounds once. */
#include <math.h>
#include <stdint.h>

/* the scan's accumulation order: s = 0..63: element s, then element 64 + s */
static float md_dot(const float *a, const float *b) {
    float acc = 0.0f;
    for (int s = 0; s < 64; ++s) {
        acc = fmaf(a[s], b[s], acc);
        acc = fmaf(a[64 + s], b[64 + s], acc);
    }
    return acc;
}

/* out[i][j] = <q[i], t[j]> for nq prepared queries and nt rows, both [.,128] */
void md_dot_matrix(const float *q, int nq, const float *t, int nt, float *out) {
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < nt; ++j) out[(int64_t)i * nt + j] = md_dot(q + (int64_t)i * 128, t + (int64_t)j * 128);
}
