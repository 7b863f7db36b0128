/*
 * tmalign_ref.c -- CPU restatement of TM-align (Zhang & Skolnick, NAR 2005) for the parity tests of
 * merizo_search_amd/csrc/ms_tmalign.hip (TEST INFRASTRUCTURE; the product never loads it).
 *
 * The routine sequence and every constant follow the public TMalign.cpp as DESIGN.md section 4 tabulates them
 * (the version is UNPINNED: no TM-align source or binary is part of this project).  Each routine below names the
 * TMalign.cpp routine it restates; the kernel names the same routines in the same order.
 *
 * Two reduction orders, chosen per call:
 *   order 0 ("seq")    every sum is a plain left-to-right loop, as in TMalign.cpp;
 *   order 1 ("kernel") every sum is the kernel's: 64 lane-strided partials (lane l adds terms l, l+64, ... from 0.0)
 *                      combined by the xor butterfly p[l] = p[l] + p[l ^ off], off = 32, 16, ..., 1.
 * The superposition is Horn's quaternion form of the Kabsch problem, solved by cyclic Jacobi rotations on the 4x4
 * key matrix with + - * / sqrt only (TMalign.cpp's own Kabsch solves a cubic with acos / cos): with order 1 the
 * kernel reproduces every value of this file bit for bit.  Build: gcc -O2 -ffp-contract=off (tests/tmalign_ref.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TM_MIN_LEN 6      /* TMalign.cpp get_initial: "Sequence is too short <=5!" */
#define TM_MAX_INC 64     /* find_max_frag: cap on the relaxations of the CA-CA cut (1.1^64 * 4.25 A: every chain passes) */

typedef struct {
    const double *x, *y;          /* [xlen][3], [ylen][3] */
    const uint8_t *seqx, *seqy;
    int xlen, ylen, fast, order;
    /* parameter_set4search */
    double D0_MIN, Lnorm, score_d8, d0, d0_search, dcu0;
    /* scratch */
    double *r1, *r2, *dis, *terms;   /* [minlen][3] x2, [minlen], [max(xlen,ylen)] */
    int *ax, *ay;                    /* aligned pairs (xtm / ytm of TMalign.cpp): x index, y index */
    int *i_ali, *k_ali;
    char *secx, *secy;
    unsigned char *dir;              /* NW directions [(xlen+1)][(ylen+1)]: 0 diagonal, 1 from (i,j-1), 2 from (i-1,j) */
    double *val;                     /* two rows of the NW value matrix */
    int *invmap, *invmap0, *invmap_dp, *y2x_, *ifr;
} ctx_t;

/* ------------------------------------------------------------------ sums ------------------------------------------ */
static double rsum(const double *t, int n, int order)
{
    if (order == 0) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s += t[i];
        return s;
    }
    double p[64], q[64];
    for (int l = 0; l < 64; l++) p[l] = 0.0;
    for (int i = 0; i < n; i++) p[i & 63] += t[i];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; l++) q[l] = p[l] + p[l ^ off];
        memcpy(p, q, sizeof p);
    }
    return p[0];
}

static double dist2(const double *a, const double *b)
{
    double d1 = a[0] - b[0], d2 = a[1] - b[1], d3 = a[2] - b[2];
    return d1 * d1 + d2 * d2 + d3 * d3;
}

/* TMalign.cpp transform / do_rotation: xx = t + u x */
static void transform(const double t[3], const double u[3][3], const double *x, double *xx)
{
    for (int c = 0; c < 3; c++) xx[c] = t[c] + u[c][0] * x[0] + u[c][1] * x[1] + u[c][2] * x[2];
}

/* ------------------------------------------------------------------ Kabsch ---------------------------------------- */
/* Cyclic Jacobi on the symmetric 4x4 a; v collects the eigenvectors (columns).  Shared op for op with the kernel. */
static void jacobi4(double a[4][4], double v[4][4])
{
    double scale = 0.0;
    for (int p = 0; p < 4; p++)
        for (int q = 0; q < 4; q++) {
            v[p][q] = (p == q) ? 1.0 : 0.0;
            scale += a[p][q] * a[p][q];
        }
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) off += a[p][q] * a[p][q];
        if (!(off > 1e-30 * scale)) break;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double apq = a[p][q];
                if (apq == 0.0) continue;
                double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; k++) {
                    double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; k++) {
                    double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 4; k++) {
                    double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

/* The rotation u and translation t from the 3x3 covariance s[a][b] = sum (x_a - cx_a)(y_b - cy_b) and the centroids:
 * y ~ u x + t.  Horn's key matrix, its leading eigenvector (first of equal maxima), the rotation of that quaternion. */
static void kabsch_solve(const double s[3][3], const double cx[3], const double cy[3], double t[3], double u[3][3])
{
    double n[4][4], v[4][4];
    n[0][0] = s[0][0] + s[1][1] + s[2][2];
    n[0][1] = s[1][2] - s[2][1];
    n[0][2] = s[2][0] - s[0][2];
    n[0][3] = s[0][1] - s[1][0];
    n[1][1] = s[0][0] - s[1][1] - s[2][2];
    n[1][2] = s[0][1] + s[1][0];
    n[1][3] = s[2][0] + s[0][2];
    n[2][2] = s[1][1] - s[0][0] - s[2][2];
    n[2][3] = s[1][2] + s[2][1];
    n[3][3] = s[2][2] - s[0][0] - s[1][1];
    for (int p = 0; p < 4; p++)
        for (int q = 0; q < p; q++) n[p][q] = n[q][p];
    jacobi4(n, v);
    int best = 0;
    for (int k = 1; k < 4; k++)
        if (n[k][k] > n[best][best]) best = k;
    double a = v[0][best], b = v[1][best], c = v[2][best], d = v[3][best];
    double nn = a * a + b * b + c * c + d * d;
    u[0][0] = (a * a + b * b - c * c - d * d) / nn;
    u[0][1] = 2.0 * (b * c - a * d) / nn;
    u[0][2] = 2.0 * (b * d + a * c) / nn;
    u[1][0] = 2.0 * (b * c + a * d) / nn;
    u[1][1] = (a * a - b * b + c * c - d * d) / nn;
    u[1][2] = 2.0 * (c * d - a * b) / nn;
    u[2][0] = 2.0 * (b * d - a * c) / nn;
    u[2][1] = 2.0 * (c * d + a * b) / nn;
    u[2][2] = (a * a - b * b - c * c + d * d) / nn;
    for (int k = 0; k < 3; k++) t[k] = cy[k] - (u[k][0] * cx[0] + u[k][1] * cx[1] + u[k][2] * cx[2]);
}

/* TMalign.cpp Kabsch (mode 1): superpose r1 (n points) onto r2 */
static void kabsch(ctx_t *c, const double *r1, const double *r2, int n, double t[3], double u[3][3])
{
    if (n == 0) {
        for (int a = 0; a < 3; a++) {
            t[a] = 0.0;
            for (int b = 0; b < 3; b++) u[a][b] = (a == b) ? 1.0 : 0.0;
        }
        return;
    }
    double cx[3], cy[3], s[3][3];
    for (int a = 0; a < 3; a++) {
        for (int k = 0; k < n; k++) c->terms[k] = r1[3 * k + a];
        cx[a] = rsum(c->terms, n, c->order) / n;
        for (int k = 0; k < n; k++) c->terms[k] = r2[3 * k + a];
        cy[a] = rsum(c->terms, n, c->order) / n;
    }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            for (int k = 0; k < n; k++) c->terms[k] = (r1[3 * k + a] - cx[a]) * (r2[3 * k + b] - cy[b]);
            s[a][b] = rsum(c->terms, n, c->order);
        }
    kabsch_solve(s, cx, cy, t, u);
}

/* ------------------------------------------------------------------ parameters ------------------------------------ */
/* TMalign.cpp parameter_set4search */
static void parameter_set4search(ctx_t *c)
{
    c->D0_MIN = 0.5;
    c->dcu0 = 4.25;
    c->Lnorm = c->xlen < c->ylen ? c->xlen : c->ylen;
    if (c->Lnorm <= 19) c->d0 = 0.168;
    else c->d0 = 1.24 * pow(c->Lnorm * 1.0 - 15, 1.0 / 3) - 1.8;
    c->D0_MIN = c->d0 + 0.8;
    c->d0 = c->D0_MIN;
    c->d0_search = c->d0;
    if (c->d0_search > 8) c->d0_search = 8;
    if (c->d0_search < 4.5) c->d0_search = 4.5;
    c->score_d8 = 1.5 * pow(c->Lnorm * 1.0, 0.3) + 3.5;
}

/* TMalign.cpp parameter_set4final: -> d0, d0_search for normalisation length len */
static void parameter_set4final(double len, double *d0, double *d0_search)
{
    if (len <= 21) *d0 = 0.5;
    else *d0 = 1.24 * pow(len * 1.0 - 15, 1.0 / 3) - 1.8;
    if (*d0 < 0.5) *d0 = 0.5;
    *d0_search = *d0;
    if (*d0_search > 8) *d0_search = 8;
    if (*d0_search < 4.5) *d0_search = 4.5;
}

/* ------------------------------------------------------------------ scoring --------------------------------------- */
/* pairs ax/ay [0,lali) -> r1/r2 rows of the subset sel[0,n) (sel NULL: the contiguous range [start, start+n)) */
static void gather(ctx_t *c, const int *sel, int start, int n)
{
    for (int k = 0; k < n; k++) {
        int m = sel ? sel[k] : start + k;
        memcpy(c->r1 + 3 * k, c->x + 3 * c->ax[m], 3 * sizeof(double));
        memcpy(c->r2 + 3 * k, c->y + 3 * c->ay[m], 3 * sizeof(double));
    }
}

/* TMalign.cpp score_fun8: distances of the rotated pairs, the ordered list of pairs within d (relaxed by 0.5 A while
 * fewer than 3 survive and a pair outside the cut has a finite distance), the score sum / Lnorm */
static int score_fun8(ctx_t *c, int lali, const double t[3], const double u[3][3], double d, int *i_ali, double *score,
                      int score_sum_method, double Lnorm, double score_d8, double d0)
{
    double d_tmp = d * d, d02 = d0 * d0, score_d8_cut = score_d8 * score_d8, xx[3];
    int n_cut, inc = 0;
    for (int i = 0; i < lali; i++) {
        transform(t, u, c->x + 3 * c->ax[i], xx);
        c->dis[i] = dist2(xx, c->y + 3 * c->ay[i]);
    }
    for (;;) {
        int out_finite = 0;     /* NaN / inf distances never enter the cut: relaxing for them would not end */
        n_cut = 0;
        for (int i = 0; i < lali; i++) {
            double di = c->dis[i];
            if (di < d_tmp) i_ali[n_cut++] = i;
            else out_finite |= isfinite(di) != 0;
            c->terms[i] = (score_sum_method != 8 || di <= score_d8_cut) ? 1 / (1 + di / d02) : 0.0;
        }
        if (n_cut < 3 && lali > 3 && out_finite) {
            inc++;
            double dinc = d + inc * 0.5;
            d_tmp = dinc * dinc;
        } else
            break;
    }
    *score = rsum(c->terms, lali, c->order) / Lnorm;
    return n_cut;
}

/* TMalign.cpp TMscore8_search over the aligned pairs ax/ay [0,lali): the best superposition (t0,u0) by fragment
 * superposition + iterative extension; returns the best score */
static double TMscore8_search(ctx_t *c, int lali, double t0[3], double u0[3][3], int simplify_step, int score_sum_method,
                              double local_d0_search, double Lnorm, double score_d8, double d0)
{
    int L_ini[6], n_init = 0, i;
    int L_ini_min = 4;
    if (lali < L_ini_min) L_ini_min = lali;
    for (i = 0; i < 5; i++) {
        n_init++;
        L_ini[i] = lali >> i;
        if (L_ini[i] <= L_ini_min) {
            L_ini[i] = L_ini_min;
            break;
        }
    }
    if (i == 5) {
        n_init++;
        L_ini[i] = L_ini_min;
    }
    double score_max = -1, score, t[3], u[3][3];
    int *i_ali = c->i_ali, *k_ali = c->k_ali;
    for (int i_init = 0; i_init < n_init; i_init++) {
        int L_frag = L_ini[i_init], iL_max = lali - L_frag;
        i = 0;
        for (;;) {
            gather(c, NULL, i, L_frag);
            kabsch(c, c->r1, c->r2, L_frag, t, u);
            int n_cut = score_fun8(c, lali, t, u, local_d0_search - 1, i_ali, &score, score_sum_method, Lnorm, score_d8, d0);
            if (score > score_max) {
                score_max = score;
                memcpy(t0, t, sizeof t);
                memcpy(u0, u, sizeof u);
            }
            double d = local_d0_search + 1;
            for (int it = 0; it < 20; it++) {
                int ka = n_cut;
                int *tmp = k_ali; k_ali = i_ali; i_ali = tmp;      /* k_ali = the list the superposition is fitted to */
                gather(c, k_ali, 0, ka);
                kabsch(c, c->r1, c->r2, ka, t, u);
                n_cut = score_fun8(c, lali, t, u, d, i_ali, &score, score_sum_method, Lnorm, score_d8, d0);
                if (score > score_max) {
                    score_max = score;
                    memcpy(t0, t, sizeof t);
                    memcpy(u0, u, sizeof u);
                }
                if (n_cut == ka) {
                    int k;
                    for (k = 0; k < n_cut; k++)
                        if (i_ali[k] != k_ali[k]) break;
                    if (k == n_cut) break;
                }
            }
            if (i < iL_max) {
                i = i + simplify_step;
                if (i > iL_max) i = iL_max;
            } else
                break;
        }
    }
    return score_max;
}

/* the aligned pairs of a map y2x: ax/ay in order of y; returns their number */
static int pairs_of(ctx_t *c, const int *y2x)
{
    int k = 0;
    for (int j = 0; j < c->ylen; j++)
        if (y2x[j] >= 0) {
            c->ax[k] = y2x[j];
            c->ay[k] = j;
            k++;
        }
    return k;
}

/* TMalign.cpp detailed_search (and detailed_search_standard for the final step) */
static double detailed_search(ctx_t *c, const int *y2x, double t[3], double u[3][3], int simplify_step)
{
    int k = pairs_of(c, y2x);
    return TMscore8_search(c, k, t, u, simplify_step, 8, c->d0_search, c->Lnorm, c->score_d8, c->d0);
}

/* the ordered list of the pairs [0, n_ali) with dis <= cut -> c->i_ali; returns their number, *out_finite: whether a pair
 * outside the cut has a finite distance (get_score_fast relaxes the cut by 0.5 while fewer than 3 are within and one is) */
static int within(ctx_t *c, int n_ali, double cut, int *out_finite)
{
    int j = 0;
    *out_finite = 0;
    for (int k = 0; k < n_ali; k++)
        if (c->dis[k] <= cut) c->i_ali[j++] = k;
        else *out_finite |= isfinite(c->dis[k]) != 0;
    return j;
}

/* TMalign.cpp get_score_fast: three superpositions of the pairs of y2x */
static double get_score_fast(ctx_t *c, const int *y2x, double t[3], double u[3][3])
{
    int n_ali = pairs_of(c, y2x), j, out_finite;
    double d002 = c->d0_search * c->d0_search, d02 = c->d0 * c->d0, xx[3], tmscore, tmscore1, tmscore2;
    gather(c, NULL, 0, n_ali);
    kabsch(c, c->r1, c->r2, n_ali, t, u);
    for (int k = 0; k < n_ali; k++) {
        transform(t, u, c->x + 3 * c->ax[k], xx);
        c->dis[k] = dist2(xx, c->y + 3 * c->ay[k]);
        c->terms[k] = 1 / (1 + c->dis[k] / d02);
    }
    tmscore = rsum(c->terms, n_ali, c->order);
    double d002t = d002;
    for (;;) {
        j = within(c, n_ali, d002t, &out_finite);
        if (j < 3 && n_ali > 3 && out_finite) d002t += 0.5;
        else break;
    }
    if (n_ali != j) {
        gather(c, c->i_ali, 0, j);
        kabsch(c, c->r1, c->r2, j, t, u);
        for (int k = 0; k < n_ali; k++) {
            transform(t, u, c->x + 3 * c->ax[k], xx);
            c->dis[k] = dist2(xx, c->y + 3 * c->ay[k]);
            c->terms[k] = 1 / (1 + c->dis[k] / d02);
        }
        tmscore1 = rsum(c->terms, n_ali, c->order);
        d002t = d002 + 1;
        for (;;) {
            j = within(c, n_ali, d002t, &out_finite);
            if (j < 3 && n_ali > 3 && out_finite) d002t += 0.5;
            else break;
        }
        gather(c, c->i_ali, 0, j);
        kabsch(c, c->r1, c->r2, j, t, u);
        for (int k = 0; k < n_ali; k++) {
            transform(t, u, c->x + 3 * c->ax[k], xx);
            c->terms[k] = 1 / (1 + dist2(xx, c->y + 3 * c->ay[k]) / d02);
        }
        tmscore2 = rsum(c->terms, n_ali, c->order);
    } else {
        tmscore1 = tmscore;
        tmscore2 = tmscore;
    }
    if (tmscore1 >= tmscore) tmscore = tmscore1;
    if (tmscore2 >= tmscore) tmscore = tmscore2;
    return tmscore;
}

/* ------------------------------------------------------------------ dynamic programming --------------------------- */
/* TMalign.cpp NWDP_TM, its three scorings: kind 0 = 1/(1+d^2/d02) after (t,u); kind 1 = secondary structure equal;
 * kind 2 = kind 0 + 0.5 where the secondary structures are equal (score_matrix_rmsd_sec).  The gap applies only when
 * the neighbour cell came from the diagonal; ties go diagonal, then v >= h.  Writes y2x [ylen]. */
static void NWDP_TM(ctx_t *c, int kind, const double t[3], const double u[3][3], double d02, double gap_open, int *y2x)
{
    int len1 = c->xlen, len2 = c->ylen, W = len2 + 1;
    double *prev = c->val, *cur = c->val + W, xx[3];
    unsigned char *dir = c->dir;
    for (int j = 0; j <= len2; j++) {
        prev[j] = 0;
        dir[j] = 1;                /* row 0 and column 0: path false (not from the diagonal) */
        y2x[j] = -1;
    }
    for (int i = 1; i <= len1; i++) {
        if (kind != 1) transform(t, u, c->x + 3 * (i - 1), xx);
        cur[0] = 0;
        dir[i * W] = 1;
        for (int j = 1; j <= len2; j++) {
            double sc;
            if (kind == 1) sc = (c->secx[i - 1] == c->secy[j - 1]) ? 1.0 : 0.0;
            else {
                sc = 1.0 / (1 + dist2(xx, c->y + 3 * (j - 1)) / d02);
                if (kind == 2 && c->secx[i - 1] == c->secy[j - 1]) sc = sc + 0.5;
            }
            double d = prev[j - 1] + sc;
            double h = prev[j];
            if (dir[(i - 1) * W + j] == 0) h += gap_open;
            double v = cur[j - 1];
            if (dir[i * W + j - 1] == 0) v += gap_open;
            if (d >= h && d >= v) {
                dir[i * W + j] = 0;
                cur[j] = d;
            } else if (v >= h) {
                dir[i * W + j] = 1;
                cur[j] = v;
            } else {
                dir[i * W + j] = 2;
                cur[j] = h;
            }
        }
        double *tmp = prev; prev = cur; cur = tmp;
    }
    int i = len1, j = len2;
    while (i > 0 && j > 0) {
        unsigned char e = dir[i * W + j];
        if (e == 0) {
            y2x[j - 1] = i - 1;
            i--;
            j--;
        } else if (e == 1) j--;
        else i--;
    }
}

/* TMalign.cpp DP_iter: writes the best map into y2x_best; (t,u) in: the start superposition */
static double DP_iter(ctx_t *c, double t[3], double u[3][3], int *y2x_best, int g1, int g2, int iteration_max)
{
    double gap_open[2] = {-0.6, 0}, tmscore, tmscore_max = -1, tmscore_old = 0, d02 = c->d0 * c->d0;
    int *invmap = c->invmap_dp;
    for (int g = g1; g < g2; g++)
        for (int iteration = 0; iteration < iteration_max; iteration++) {
            NWDP_TM(c, 0, t, u, d02, gap_open[g], invmap);
            int k = pairs_of(c, invmap);
            tmscore = TMscore8_search(c, k, t, u, 40, 8, c->d0_search, c->Lnorm, c->score_d8, c->d0);
            if (tmscore > tmscore_max) {
                tmscore_max = tmscore;
                memcpy(y2x_best, invmap, c->ylen * sizeof(int));
            }
            if (iteration > 0 && fabs(tmscore_old - tmscore) < 0.000001) break;
            tmscore_old = tmscore;
        }
    return tmscore_max;
}

/* ------------------------------------------------------------------ initial alignments ---------------------------- */
/* TMalign.cpp get_initial: gapless threading, the LAST best shift */
static void get_initial(ctx_t *c, int *y2x, double t[3], double u[3][3])
{
    int xlen = c->xlen, ylen = c->ylen, min_len = xlen < ylen ? xlen : ylen;
    int min_ali = min_len / 2;
    if (min_ali <= 5) min_ali = 5;
    int n1 = -ylen + min_ali, n2 = xlen - min_ali, k_best = n1;
    double tmscore_max = -1;
    for (int k = n1; k <= n2; k += c->fast ? 5 : 1) {
        for (int j = 0; j < ylen; j++) y2x[j] = (j + k >= 0 && j + k < xlen) ? j + k : -1;
        double tmscore = get_score_fast(c, y2x, t, u);
        if (tmscore >= tmscore_max) {
            tmscore_max = tmscore;
            k_best = k;
        }
    }
    for (int j = 0; j < ylen; j++) y2x[j] = (j + k_best >= 0 && j + k_best < xlen) ? j + k_best : -1;
}

/* TMalign.cpp sec_str / make_sec: secondary structure from CA distances i-2..i+2 */
static char sec_str(double dis13, double dis14, double dis15, double dis24, double dis25, double dis35)
{
    double delta = 2.1;
    if (fabs(dis15 - 6.37) < delta && fabs(dis14 - 5.18) < delta && fabs(dis25 - 5.18) < delta && fabs(dis13 - 5.45) < delta &&
        fabs(dis24 - 5.45) < delta && fabs(dis35 - 5.45) < delta)
        return 'H';
    delta = 1.42;
    if (fabs(dis15 - 13) < delta && fabs(dis14 - 10.4) < delta && fabs(dis25 - 10.4) < delta && fabs(dis13 - 6.1) < delta &&
        fabs(dis24 - 6.1) < delta && fabs(dis35 - 6.1) < delta)
        return 'E';
    if (dis15 < 8) return 'T';
    return 'C';
}

static void make_sec(const double *x, int len, char *sec)
{
    for (int i = 0; i < len; i++) {
        sec[i] = 'C';
        if (i - 2 >= 0 && i + 2 < len) {
            const double *a = x + 3 * (i - 2), *b = x + 3 * (i - 1), *m = x + 3 * i, *d = x + 3 * (i + 1), *e = x + 3 * (i + 2);
            sec[i] = sec_str(sqrt(dist2(a, m)), sqrt(dist2(a, d)), sqrt(dist2(a, e)), sqrt(dist2(b, d)), sqrt(dist2(b, e)),
                             sqrt(dist2(m, e)));
        }
    }
}

/* TMalign.cpp get_initial5: local superposition of fragments of 20 and 100, FIRST best */
static int get_initial5(ctx_t *c, int *y2x)
{
    int xlen = c->xlen, ylen = c->ylen, aL = xlen < ylen ? xlen : ylen;
    double d01 = c->d0 + 1.5, t[3], u[3][3];
    if (d01 < c->D0_MIN) d01 = c->D0_MIN;
    double d02 = d01 * d01, GLmax = 0;
    int n_jump1 = xlen > 250 ? 45 : xlen > 200 ? 35 : xlen > 150 ? 25 : 15;
    if (n_jump1 > xlen / 3) n_jump1 = xlen / 3;
    int n_jump2 = ylen > 250 ? 45 : ylen > 200 ? 35 : ylen > 150 ? 25 : 15;
    if (n_jump2 > ylen / 3) n_jump2 = ylen / 3;
    int n_frag[2] = {20, 100};
    if (n_frag[0] > aL / 3) n_frag[0] = aL / 3;
    if (n_frag[1] > aL / 2) n_frag[1] = aL / 2;
    if (c->fast) {
        n_jump1 *= 5;
        n_jump2 *= 5;
    }
    int flag = 0, *invmap = c->y2x_;
    for (int i_frag = 0; i_frag < 2; i_frag++) {
        int m1 = xlen - n_frag[i_frag] + 1, m2 = ylen - n_frag[i_frag] + 1;
        for (int i = 0; i < m1; i += n_jump1)
            for (int j = 0; j < m2; j += n_jump2) {
                for (int k = 0; k < n_frag[i_frag]; k++) {
                    memcpy(c->r1 + 3 * k, c->x + 3 * (k + i), 3 * sizeof(double));
                    memcpy(c->r2 + 3 * k, c->y + 3 * (k + j), 3 * sizeof(double));
                }
                kabsch(c, c->r1, c->r2, n_frag[i_frag], t, u);
                NWDP_TM(c, 0, t, u, d02, 0.0, invmap);
                double GL = get_score_fast(c, invmap, t, u);
                if (GL > GLmax) {
                    GLmax = GL;
                    memcpy(y2x, invmap, ylen * sizeof(int));
                    flag = 1;
                }
            }
    }
    return flag;
}

/* TMalign.cpp get_initial_ssplus (score_matrix_rmsd_sec + NWDP_TM): superposition of the pairs of y2x0, DP on
 * distance + secondary-structure scores */
static void get_initial_ssplus(ctx_t *c, const int *y2x0, int *y2x)
{
    double d01 = c->d0 + 1.5, t[3], u[3][3];
    if (d01 < c->D0_MIN) d01 = c->D0_MIN;
    int k = pairs_of(c, y2x0);
    gather(c, NULL, 0, k);
    kabsch(c, c->r1, c->r2, k, t, u);
    NWDP_TM(c, 2, t, u, d01 * d01, -1.0, y2x);
}

/* TMalign.cpp find_max_frag: the longest run of CA-CA steps below dcu0 (relaxed by 1.1^inc) */
static void find_max_frag(ctx_t *c, const double *x, int len, int *start_max, int *end_max)
{
    int fra_min = c->fast ? 8 : 4, Lfr_max = 0, inc = 0;
    int r_min = (int)(len * 1.0 / 3.0);
    if (r_min > fra_min) r_min = fra_min;
    double dcu_cut = c->dcu0 * c->dcu0;
    while (Lfr_max < r_min) {
        Lfr_max = 0;
        int j = 1, start = 0;
        for (int i = 1; i < len; i++) {
            if (dist2(x + 3 * (i - 1), x + 3 * i) < dcu_cut) {
                j++;
                if (i == len - 1) {
                    if (j > Lfr_max) {
                        Lfr_max = j;
                        *start_max = start;
                        *end_max = i;
                    }
                    j = 1;
                }
            } else {
                if (j > Lfr_max) {
                    Lfr_max = j;
                    *start_max = start;
                    *end_max = i - 1;
                }
                j = 1;
                start = i;
            }
        }
        if (Lfr_max < r_min) {
            inc++;
            if (inc > TM_MAX_INC) break;
            double dinc = pow(1.1, (double)inc) * c->dcu0;
            dcu_cut = dinc * dinc;
        }
    }
}

/* TMalign.cpp get_initial_fgt: gapless threading of the longest continuous fragment, the LAST best shift */
static void get_initial_fgt(ctx_t *c, int *y2x, double t[3], double u[3][3])
{
    int xlen = c->xlen, ylen = c->ylen, fra_min1 = (c->fast ? 8 : 4) - 1;
    int xstart = 0, ystart = 0, xend = 0, yend = 0;
    find_max_frag(c, c->x, xlen, &xstart, &xend);
    find_max_frag(c, c->y, ylen, &ystart, &yend);
    int Lx = xend - xstart + 1, Ly = yend - ystart + 1, *ifr = c->ifr, *y2x_ = c->y2x_;
    int L_fr = Lx < Ly ? Lx : Ly;
    int on_x = Lx < Ly || (Lx == Ly && xlen <= ylen);
    for (int i = 0; i < L_fr; i++) ifr[i] = (on_x ? xstart : ystart) + i;
    int L0 = xlen < ylen ? xlen : ylen;
    if (L_fr == L0) {
        int n1 = (int)(L0 * 0.1), n2 = (int)(L0 * 0.89), j = 0;
        for (int i = n1; i <= n2; i++) ifr[j++] = ifr[i];
        L_fr = j;
    }
    double tmscore, tmscore_max = -1;
    if (on_x) {
        int L1 = L_fr, min_len = L1 < ylen ? L1 : ylen;
        int min_ali = (int)(min_len / 2.5);
        if (min_ali <= fra_min1) min_ali = fra_min1;
        for (int k = -ylen + min_ali; k <= L1 - min_ali; k += c->fast ? 3 : 1) {
            for (int j = 0; j < ylen; j++) y2x_[j] = (j + k >= 0 && j + k < L1) ? ifr[j + k] : -1;
            tmscore = get_score_fast(c, y2x_, t, u);
            if (tmscore >= tmscore_max) {
                tmscore_max = tmscore;
                memcpy(y2x, y2x_, ylen * sizeof(int));
            }
        }
    } else {
        int L2 = L_fr, min_len = xlen < L2 ? xlen : L2;
        int min_ali = (int)(min_len / 2.5);
        if (min_ali <= fra_min1) min_ali = fra_min1;
        for (int k = -L2 + min_ali; k <= xlen - min_ali; k++) {
            for (int j = 0; j < ylen; j++) y2x_[j] = -1;
            for (int j = 0; j < L2; j++)
                if (j + k >= 0 && j + k < xlen) y2x_[ifr[j]] = j + k;
            tmscore = get_score_fast(c, y2x_, t, u);
            if (tmscore >= tmscore_max) {
                tmscore_max = tmscore;
                memcpy(y2x, y2x_, ylen * sizeof(int));
            }
        }
    }
}

/* ------------------------------------------------------------------ TMalign_main ---------------------------------- */
/* Test hook: the superposition of the n point pairs r1 -> r2 (r2 ~ u r1 + t; u row-major [3][3]) that kabsch computes in
 * order=kernel, for checking the solver against an independent SVD.  Returns 0, or -1 for n < 0. */
int tm_kabsch(const double *r1, const double *r2, int n, double *t, double *u)
{
    if (n < 0) return -1;
    ctx_t C;
    memset(&C, 0, sizeof C);
    C.order = 1;
    C.terms = malloc(sizeof(double) * (n > 0 ? n : 1));
    double uu[3][3];
    kabsch(&C, r1, r2, n, t, uu);
    memcpy(u, uu, sizeof uu);
    free(C.terms);
    return 0;
}

/* x: chain 1 (query) [xlen][3], y: chain 2 [ylen][3].  out_f: qtm (normalised by xlen), ttm (by ylen), rmsd;
 * out_i: n_ali8, n_identical; invmap_out [ylen] (NULL: not wanted): the final alignment y -> x (-1 = gap).
 * Returns 0, or -1 for a chain of <= 5 residues. */
int tm_align(const double *x, int xlen, const uint8_t *seqx, const double *y, int ylen, const uint8_t *seqy, int fast, int order,
             double *out_f, int *out_i, int *invmap_out)
{
    if (xlen < TM_MIN_LEN || ylen < TM_MIN_LEN) return -1;
    ctx_t C, *c = &C;
    memset(c, 0, sizeof C);
    c->x = x; c->y = y; c->seqx = seqx; c->seqy = seqy; c->xlen = xlen; c->ylen = ylen; c->fast = fast; c->order = order;
    int mx = xlen > ylen ? xlen : ylen;
    c->r1 = malloc(3 * sizeof(double) * mx);
    c->r2 = malloc(3 * sizeof(double) * mx);
    c->dis = malloc(sizeof(double) * mx);
    c->terms = malloc(sizeof(double) * mx);
    c->ax = malloc(sizeof(int) * mx);
    c->ay = malloc(sizeof(int) * mx);
    c->i_ali = malloc(sizeof(int) * mx);
    c->k_ali = malloc(sizeof(int) * mx);
    c->secx = malloc(xlen + 1);
    c->secy = malloc(ylen + 1);
    c->dir = malloc((size_t)(xlen + 1) * (ylen + 1));
    c->val = malloc(2 * sizeof(double) * (ylen + 1));
    c->invmap = malloc(sizeof(int) * (ylen + 1));
    c->invmap0 = malloc(sizeof(int) * (ylen + 1));
    c->invmap_dp = malloc(sizeof(int) * (ylen + 1));
    c->y2x_ = malloc(sizeof(int) * (ylen + 1));
    c->ifr = malloc(sizeof(int) * mx);

    parameter_set4search(c);
    make_sec(x, xlen, c->secx);
    make_sec(y, ylen, c->secy);
    double t[3], u[3][3], TM, TMmax = -1;
    int *invmap0 = c->invmap0, *invmap = c->invmap;
    double ddcc = c->Lnorm <= 40 ? 0.1 : 0.4;
#define KEEP_IF_BETTER() do { if (TM > TMmax) { TMmax = TM; memcpy(invmap0, invmap, ylen * sizeof(int)); } } while (0)

    /* get_initial + detailed_search + DP_iter */
    get_initial(c, invmap0, t, u);
    TM = detailed_search(c, invmap0, t, u, 40);
    if (TM > TMmax) TMmax = TM;
    TM = DP_iter(c, t, u, invmap, 0, 2, fast ? 2 : 30);
    KEEP_IF_BETTER();

    /* get_initial_ss */
    NWDP_TM(c, 1, t, u, 0.0, -1.0, invmap);
    TM = detailed_search(c, invmap, t, u, 40);
    KEEP_IF_BETTER();
    if (TM > TMmax * 0.2) {
        TM = DP_iter(c, t, u, invmap, 0, 2, fast ? 2 : 30);
        KEEP_IF_BETTER();
    }

    /* get_initial5 */
    if (get_initial5(c, invmap)) {
        TM = detailed_search(c, invmap, t, u, 40);
        KEEP_IF_BETTER();
        if (TM > TMmax * ddcc) {
            TM = DP_iter(c, t, u, invmap, 0, 2, 2);
            KEEP_IF_BETTER();
        }
    }

    /* get_initial_ssplus */
    get_initial_ssplus(c, invmap0, invmap);
    TM = detailed_search(c, invmap, t, u, 40);
    KEEP_IF_BETTER();
    if (TM > TMmax * ddcc) {
        TM = DP_iter(c, t, u, invmap, 0, 2, fast ? 2 : 30);
        KEEP_IF_BETTER();
    }

    /* get_initial_fgt */
    get_initial_fgt(c, invmap, t, u);
    TM = detailed_search(c, invmap, t, u, 40);
    KEEP_IF_BETTER();
    if (TM > TMmax * ddcc) {
        TM = DP_iter(c, t, u, invmap, 1, 2, 2);
        KEEP_IF_BETTER();
    }
#undef KEEP_IF_BETTER

    /* final: detailed_search_standard, the pairs within score_d8, TM-scores by both lengths (parameter_set4final) */
    detailed_search(c, invmap0, t, u, fast ? 40 : 1);
    double score_d8_cut = c->score_d8 * c->score_d8, xx[3];
    int n_ali8 = 0, n_ident = 0, lali = pairs_of(c, invmap0);
    for (int k = 0; k < lali; k++) {
        transform(t, u, x + 3 * c->ax[k], xx);
        if (sqrt(dist2(xx, y + 3 * c->ay[k])) <= c->score_d8) {
            c->ax[n_ali8] = c->ax[k];
            c->ay[n_ali8] = c->ay[k];
            n_ali8++;
        }
    }
    (void)score_d8_cut;
    for (int k = 0; k < n_ali8; k++) n_ident += seqx[c->ax[k]] == seqy[c->ay[k]];
    /* RMSD of the n_ali8 pairs after their own optimal superposition */
    double rmsd = 0.0;
    if (n_ali8 > 0) {
        gather(c, NULL, 0, n_ali8);
        kabsch(c, c->r1, c->r2, n_ali8, t, u);
        for (int k = 0; k < n_ali8; k++) {
            transform(t, u, c->r1 + 3 * k, xx);
            c->terms[k] = dist2(xx, c->r2 + 3 * k);
        }
        rmsd = sqrt(rsum(c->terms, n_ali8, order) / n_ali8);
    }
    double d0, d0s, tf[3], uf[3][3];
    parameter_set4final(xlen, &d0, &d0s);
    out_f[0] = n_ali8 > 0 ? TMscore8_search(c, n_ali8, tf, uf, 1, 0, d0s, xlen, c->score_d8, d0) : 0.0;
    parameter_set4final(ylen, &d0, &d0s);
    out_f[1] = n_ali8 > 0 ? TMscore8_search(c, n_ali8, tf, uf, 1, 0, d0s, ylen, c->score_d8, d0) : 0.0;
    out_f[2] = rmsd;
    out_i[0] = n_ali8;
    out_i[1] = n_ident;
    if (invmap_out) memcpy(invmap_out, invmap0, ylen * sizeof(int));

    free(c->r1); free(c->r2); free(c->dis); free(c->terms); free(c->ax); free(c->ay); free(c->i_ali); free(c->k_ali);
    free(c->secx); free(c->secy); free(c->dir); free(c->val); free(c->invmap); free(c->invmap0); free(c->invmap_dp);
    free(c->y2x_); free(c->ifr);
    return 0;
}
