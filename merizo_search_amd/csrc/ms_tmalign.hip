// ms_tmalign.hip -- batched TM-align (Zhang & Skolnick, NAR 2005) on gfx950: ms_tmalign_workspace_bytes, ms_tmalign_batch.
//
// Replaces the TM-align subprocess the reference starts for every hit (programs/Foldclass/utils.py:75-109) and for every
// query-domain x target-domain pair of the multi-domain search (dbsearch_fulllength.py:55-92).  The routine sequence and
// every constant are those of the public TMalign.cpp (DESIGN.md section 4 tabulates them; the version is unpinned); each
// device routine below names the TMalign.cpp routine it restates, in the order tests/tmalign_ref.c (the CPU restatement
// the tests compare against) restates them.
//
// Layout: ONE WAVE PER PAIR (a workgroup of 64 lanes).  Workgroup w takes pairs w, w + grid, ... of the list in the order
// given (the host passes it longest first).  Control flow is uniform: every lane runs the sequential logic of TM-align on
// the same values, and the loops over residues / aligned pairs are lane-strided.  Every sum is 64 lane-strided partials
// (lane l adds terms l, l+64, ... from 0.0) combined by an xor butterfly, which leaves the same bits on every lane; the
// restatement's order=kernel computes the same expression.  Lists (aligned pairs, pairs within a cut) are compacted in
// order with a ballot.  The Needleman-Wunsch DP runs as a skewed wavefront: in a block of 64 rows lane l owns row
// i0 + l and at step s computes column s - l + 1; the cell above comes from lane l-1 by a cross-lane shift, the last
// row of a block is handed to the next block through LDS.  The traceback reads a direction byte per cell (0 diagonal,
// 1 left, 2 up), stored step-major (64 consecutive bytes per step) in the pair's slot of the workspace; the forward
// pass's own decisions are stored, so the traceback is exact.  Geometry is fp64 throughout.  Superposition: Horn's
// quaternion form of the Kabsch problem, solved by cyclic Jacobi rotations of the 4x4 key matrix with + - * / sqrt
// only, so the CPU restatement reproduces it bit for bit.  Length-dependent parameters (pow / cbrt in TMalign.cpp) come
// from a host-computed table copied into the workspace with every call.
#include "ms_common.h"

#include <math.h>
#include <mutex>

namespace {

constexpr int kMaxInc = 64;             // find_max_frag: relaxations of the CA-CA cut (tests/tmalign_ref.c TM_MAX_INC)
constexpr int kMinLen = 6;              // TM-align refuses chains of <= 5 residues
constexpr int kMaxLen = MS_TMALIGN_MAX_LEN;

// parameter table: per length L in [0, kMaxLen]
struct TmParams {
    double s_d0[kMaxLen + 1];           // parameter_set4search: d0 (= D0_MIN) for Lnorm = L
    double s_d0_search[kMaxLen + 1];
    double s_score_d8[kMaxLen + 1];
    double f_d0[kMaxLen + 1];           // parameter_set4final(L)
    double f_d0_search[kMaxLen + 1];
    double pow11[kMaxInc + 1];          // find_max_frag: pow(1.1, inc)
};

const TmParams *host_params() {
    static TmParams p;
    static std::once_flag once;
    std::call_once(once, [] {
        for (int L = 0; L <= kMaxLen; ++L) {
            double Lnorm = L, d0;
            if (Lnorm <= 19) d0 = 0.168;
            else d0 = 1.24 * pow(Lnorm * 1.0 - 15, 1.0 / 3) - 1.8;
            double D0_MIN = d0 + 0.8;
            d0 = D0_MIN;
            double ds = d0;
            if (ds > 8) ds = 8;
            if (ds < 4.5) ds = 4.5;
            p.s_d0[L] = d0;
            p.s_d0_search[L] = ds;
            p.s_score_d8[L] = 1.5 * pow(Lnorm * 1.0, 0.3) + 3.5;
            double f;
            if (Lnorm <= 21) f = 0.5;
            else f = 1.24 * pow(Lnorm * 1.0 - 15, 1.0 / 3) - 1.8;
            if (f < 0.5) f = 0.5;
            double fs = f;
            if (fs > 8) fs = 8;
            if (fs < 4.5) fs = 4.5;
            p.f_d0[L] = f;
            p.f_d0_search[L] = fs;
        }
        p.pow11[0] = 1.0;
        for (int i = 1; i <= kMaxInc; ++i) p.pow11[i] = pow(1.1, (double)i);
    });
    return &p;
}

// per-pair slot of the workspace, for chains up to X x Y residues
struct SlotLayout {
    size_t dir, ax, ay, ia, ka, dis, secx, secy, invmap, invmap0, invmap_dp, y2x_, total;
};

__host__ __device__ inline size_t take(size_t &o, size_t bytes) {
    const size_t at = o;
    o = (o + bytes + 255) / 256 * 256;
    return at;
}

__host__ __device__ inline SlotLayout slot_layout(int X, int Y) {
    SlotLayout s;
    const size_t M = (size_t)(X > Y ? X : Y) + 1, nb = (size_t)(X + 63) / 64;
    size_t o = 0;
    s.dir = take(o, nb * (size_t)(Y + 63) * 64);
    s.ax = take(o, M * 4); s.ay = take(o, M * 4); s.ia = take(o, M * 4); s.ka = take(o, M * 4);
    s.dis = take(o, M * 8);
    s.secx = take(o, (size_t)X + 1); s.secy = take(o, (size_t)Y + 1);
    s.invmap = take(o, (size_t)(Y + 1) * 4); s.invmap0 = take(o, (size_t)(Y + 1) * 4);
    s.invmap_dp = take(o, (size_t)(Y + 1) * 4); s.y2x_ = take(o, (size_t)(Y + 1) * 4);
    s.total = o;
    return s;
}

constexpr size_t kParamBytes = (sizeof(TmParams) + 255) / 256 * 256;
constexpr int kMaxSlots = 2048;
constexpr size_t kSlotBudget = (size_t)2 << 30;      // slots beyond one per CU-wave pay off only while they stay this small

int slot_count(int X, int Y, int npairs) {
    const size_t per = slot_layout(X, Y).total;
    size_t fit = kSlotBudget / per;
    if (fit < 1) fit = 1;
    size_t n = (size_t)npairs;
    if (n > fit) n = fit;
    if (n > (size_t)kMaxSlots) n = kMaxSlots;
    return (int)n;
}

// ---------------------------------------------------------------- device ----------------------------------------------
struct Ctx {
    const double *x, *y;
    const uint8_t *seqx, *seqy;
    int xlen, ylen, fast, lane, X, Y;
    double D0_MIN, Lnorm, score_d8, d0, d0_search, dcu0;
    const TmParams *prm;
    uint8_t *dir, *secx, *secy;
    int *ax, *ay, *ia, *ka, *invmap, *invmap0, *invmap_dp, *y2x_;
    double *dis;
    double *rowval;                 // LDS [kMaxLen + 1]
    uint8_t *rowdir;                // LDS [kMaxLen + 1]
};

__device__ __forceinline__ void wave_sync() { __syncthreads(); }      // one wave per workgroup: orders the lanes' memory

__device__ __forceinline__ double wave_sum(double p) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    return p;
}

__device__ __forceinline__ int prefix_before(unsigned long long mask, int lane) {
    return __popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ double dist2(const double *a, const double *b) {
    double d1 = a[0] - b[0], d2 = a[1] - b[1], d3 = a[2] - b[2];
    return d1 * d1 + d2 * d2 + d3 * d3;
}

__device__ __forceinline__ void load3(const double *p, double *v) { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; }

// TMalign.cpp transform / do_rotation
__device__ __forceinline__ void transform(const double t[3], const double u[3][3], const double *x, double *xx) {
#pragma unroll
    for (int c = 0; c < 3; c++) xx[c] = t[c] + u[c][0] * x[0] + u[c][1] * x[1] + u[c][2] * x[2];
}

// ---- Kabsch: Horn's key matrix, cyclic Jacobi (op for op as tests/tmalign_ref.c jacobi4 / kabsch_solve) ----
__device__ void jacobi4(double a[4][4], double v[4][4]) {
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

__device__ void kabsch_solve(const double s[3][3], const double cx[3], const double cy[3], double t[3], double u[3][3]) {
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

// TMalign.cpp Kabsch (mode 1): superpose the n point pairs g(k) -> (a from x, b from y)
template <class G>
__device__ void kabsch(const Ctx &c, const G &g, int n, double t[3], double u[3][3]) {
    if (n == 0) {
        for (int a = 0; a < 3; a++) {
            t[a] = 0.0;
            for (int b = 0; b < 3; b++) u[a][b] = (a == b) ? 1.0 : 0.0;
        }
        return;
    }
    double px[3] = {0.0, 0.0, 0.0}, py[3] = {0.0, 0.0, 0.0}, cx[3], cy[3], s[3][3];
    for (int k = c.lane; k < n; k += 64) {
        double a[3], b[3];
        g(k, a, b);
        for (int i = 0; i < 3; i++) {
            px[i] += a[i];
            py[i] += b[i];
        }
    }
    for (int i = 0; i < 3; i++) {
        cx[i] = wave_sum(px[i]) / n;
        cy[i] = wave_sum(py[i]) / n;
    }
    double ps[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) ps[i][j] = 0.0;
    for (int k = c.lane; k < n; k += 64) {
        double a[3], b[3];
        g(k, a, b);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) ps[i][j] += (a[i] - cx[i]) * (b[j] - cy[j]);
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) s[i][j] = wave_sum(ps[i][j]);
    kabsch_solve(s, cx, cy, t, u);
}

// point pairs: aligned pairs [start, start+n) or the subset sel[0,n) of them; contiguous fragments of x and y
struct PairSel {
    const Ctx &c;
    const int *sel;
    int start;
    __device__ void operator()(int k, double *a, double *b) const {
        int m = sel ? sel[k] : start + k;
        load3(c.x + 3 * c.ax[m], a);
        load3(c.y + 3 * c.ay[m], b);
    }
};
struct FragSel {
    const Ctx &c;
    int i0, j0;
    __device__ void operator()(int k, double *a, double *b) const {
        load3(c.x + 3 * (i0 + k), a);
        load3(c.y + 3 * (j0 + k), b);
    }
};

// ---- scoring ----
// TMalign.cpp score_fun8 over the aligned pairs [0, lali) rotated by (t,u): ordered list of pairs within d (relaxed by
// 0.5 A while fewer than 3 survive and a pair outside the cut has a finite distance) -> i_ali, score sum / Lnorm
__device__ int score_fun8(Ctx &c, int lali, const double t[3], const double u[3][3], double d, int *i_ali, double *score,
                          int score_sum_method, double Lnorm, double score_d8, double d0) {
    const double d02 = d0 * d0, score_d8_cut = score_d8 * score_d8;
    double d_tmp = d * d;
    for (int k = c.lane; k < lali; k += 64) {
        double xx[3], yy[3], xk[3];
        load3(c.x + 3 * c.ax[k], xk);
        transform(t, u, xk, xx);
        load3(c.y + 3 * c.ay[k], yy);
        c.dis[k] = dist2(xx, yy);
    }
    int n_cut, inc = 0;
    double p;
    for (;;) {
        n_cut = 0;
        p = 0.0;
        bool out_finite = false;            // NaN / inf distances never enter the cut: relaxing for them would not end
        for (int base = 0; base < lali; base += 64) {
            const int k = base + c.lane;
            bool in = false;
            if (k < lali) {
                const double di = c.dis[k];
                in = di < d_tmp;
                out_finite |= !in && isfinite(di);
                p += (score_sum_method != 8 || di <= score_d8_cut) ? 1 / (1 + di / d02) : 0.0;
            }
            const unsigned long long m = __ballot(in);
            if (in) i_ali[n_cut + prefix_before(m, c.lane)] = k;
            n_cut += __popcll(m);
        }
        if (n_cut < 3 && lali > 3 && __any(out_finite)) {
            inc++;
            double dinc = d + inc * 0.5;
            d_tmp = dinc * dinc;
        } else
            break;
    }
    *score = wave_sum(p) / Lnorm;
    wave_sync();
    return n_cut;
}

// TMalign.cpp TMscore8_search over the aligned pairs [0, lali): fragments Lali, Lali/2, ... >= 4 (at most 6), 20
// extension iterations per start; the FIRST best superposition (strict >) -> (t0,u0)
__device__ double TMscore8_search(Ctx &c, int lali, double t0[3], double u0[3][3], int simplify_step, int score_sum_method,
                                  double local_d0_search, double Lnorm, double score_d8, double d0) {
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
    int *i_ali = c.ia, *k_ali = c.ka;
    for (int i_init = 0; i_init < n_init; i_init++) {
        const int L_frag = L_ini[i_init], iL_max = lali - L_frag;
        i = 0;
        for (;;) {
            kabsch(c, PairSel{c, nullptr, i}, L_frag, t, u);
            int n_cut = score_fun8(c, lali, t, u, local_d0_search - 1, i_ali, &score, score_sum_method, Lnorm, score_d8, d0);
            if (score > score_max) {
                score_max = score;
                for (int a = 0; a < 3; a++) {
                    t0[a] = t[a];
                    for (int b = 0; b < 3; b++) u0[a][b] = u[a][b];
                }
            }
            const double d = local_d0_search + 1;
            for (int it = 0; it < 20; it++) {
                const int ka = n_cut;
                int *tmp = k_ali; k_ali = i_ali; i_ali = tmp;
                kabsch(c, PairSel{c, k_ali, 0}, ka, t, u);
                n_cut = score_fun8(c, lali, t, u, d, i_ali, &score, score_sum_method, Lnorm, score_d8, d0);
                if (score > score_max) {
                    score_max = score;
                    for (int a = 0; a < 3; a++) {
                        t0[a] = t[a];
                        for (int b = 0; b < 3; b++) u0[a][b] = u[a][b];
                    }
                }
                if (n_cut == ka) {
                    bool diff = false;
                    for (int k = c.lane; k < n_cut; k += 64) diff |= i_ali[k] != k_ali[k];
                    if (!__any(diff)) break;
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

// the aligned pairs of a map y2x, in order of y -> ax / ay; returns their number
__device__ int pairs_of(Ctx &c, const int *y2x) {
    int k = 0;
    for (int base = 0; base < c.ylen; base += 64) {
        const int j = base + c.lane;
        const int i = j < c.ylen ? y2x[j] : -1;
        const unsigned long long m = __ballot(i >= 0);
        if (i >= 0) {
            const int at = k + prefix_before(m, c.lane);
            c.ax[at] = i;
            c.ay[at] = j;
        }
        k += __popcll(m);
    }
    wave_sync();
    return k;
}

// TMalign.cpp detailed_search / detailed_search_standard
__device__ double detailed_search(Ctx &c, const int *y2x, double t[3], double u[3][3], int simplify_step) {
    const int k = pairs_of(c, y2x);
    return TMscore8_search(c, k, t, u, simplify_step, 8, c.d0_search, c.Lnorm, c.score_d8, c.d0);
}

// ordered list of the pairs [0, n_ali) with dis <= cut (relaxed by 0.5 while fewer than 3 and a pair outside the cut has
// a finite distance) -> c.ia; returns the count
__device__ int select_within(Ctx &c, int n_ali, double cut) {
    int j;
    for (;;) {
        j = 0;
        bool out_finite = false;
        for (int base = 0; base < n_ali; base += 64) {
            const int k = base + c.lane;
            bool in = false;
            if (k < n_ali) {
                const double di = c.dis[k];
                in = di <= cut;
                out_finite |= !in && isfinite(di);
            }
            const unsigned long long m = __ballot(in);
            if (in) c.ia[j + prefix_before(m, c.lane)] = k;
            j += __popcll(m);
        }
        if (j < 3 && n_ali > 3 && __any(out_finite)) cut += 0.5;
        else break;
    }
    wave_sync();
    return j;
}

// sum over the pairs [0, n_ali) of 1/(1+d^2/d02) after (t,u); keep_dis: store d^2 in c.dis
__device__ double score_pairs(Ctx &c, int n_ali, const double t[3], const double u[3][3], double d02, bool keep_dis) {
    double p = 0.0;
    for (int k = c.lane; k < n_ali; k += 64) {
        double xk[3], xx[3], yy[3];
        load3(c.x + 3 * c.ax[k], xk);
        transform(t, u, xk, xx);
        load3(c.y + 3 * c.ay[k], yy);
        const double di = dist2(xx, yy);
        if (keep_dis) c.dis[k] = di;
        p += 1 / (1 + di / d02);
    }
    return wave_sum(p);
}

// TMalign.cpp get_score_fast: three superpositions of the pairs of y2x
__device__ double get_score_fast(Ctx &c, const int *y2x, double t[3], double u[3][3]) {
    const int n_ali = pairs_of(c, y2x);
    const double d002 = c.d0_search * c.d0_search, d02 = c.d0 * c.d0;
    kabsch(c, PairSel{c, nullptr, 0}, n_ali, t, u);
    double tmscore = score_pairs(c, n_ali, t, u, d02, true), tmscore1, tmscore2;
    int j = select_within(c, n_ali, d002);
    if (n_ali != j) {
        kabsch(c, PairSel{c, c.ia, 0}, j, t, u);
        tmscore1 = score_pairs(c, n_ali, t, u, d02, true);
        j = select_within(c, n_ali, d002 + 1);
        kabsch(c, PairSel{c, c.ia, 0}, j, t, u);
        tmscore2 = score_pairs(c, n_ali, t, u, d02, false);
    } else {
        tmscore1 = tmscore;
        tmscore2 = tmscore;
    }
    if (tmscore1 >= tmscore) tmscore = tmscore1;
    if (tmscore2 >= tmscore) tmscore = tmscore2;
    return tmscore;
}

// ---- dynamic programming ----
// TMalign.cpp NWDP_TM, skewed over the lanes.  kind 0: 1/(1+d^2/d02) after (t,u); 1: secondary structures equal;
// 2: kind 0 + 0.5 where the secondary structures are equal.  The gap applies only when the neighbour came from the
// diagonal; ties go diagonal, then v >= h.  -> y2x [ylen]
__device__ void NWDP_TM(Ctx &c, int kind, const double t[3], const double u[3][3], double d02, double gap_open, int *y2x) {
    const int len1 = c.xlen, len2 = c.ylen, lane = c.lane, steps = len2 + 63;
    for (int j = lane; j <= len2; j += 64) {
        c.rowval[j] = 0.0;
        c.rowdir[j] = 1;
        if (j < len2) y2x[j] = -1;
    }
    wave_sync();
    for (int b = 0; b * 64 < len1; b++) {
        const int i = b * 64 + lane + 1;
        const bool active = i <= len1;
        double xx[3] = {0.0, 0.0, 0.0};
        uint8_t sxi = 0;
        if (active) {
            if (kind != 1) {
                double xi[3];
                load3(c.x + 3 * (i - 1), xi);
                transform(t, u, xi, xx);
            }
            sxi = c.secx[i - 1];
        }
        const bool hand_on = lane == 63 && (b + 1) * 64 < len1;      // last row of a block that has a successor
        uint8_t *dirb = c.dir + (size_t)b * steps * 64 + lane;
        double left_val = 0.0, diag_val = 0.0, out_val = 0.0;
        int left_dir = 1, out_dir = 1;
        for (int s = 0; s < steps; s++) {
            const int j = s - lane + 1;
            double up_val = __shfl_up(out_val, 1, 64);
            int up_dir = __shfl_up(out_dir, 1, 64);
            const bool in = active && j >= 1 && j <= len2;
            if (lane == 0 && in) {
                up_val = c.rowval[j];
                up_dir = c.rowdir[j];
            }
            if (in) {
                double sc;
                if (kind == 1) sc = (sxi == c.secy[j - 1]) ? 1.0 : 0.0;
                else {
                    double yj[3];
                    load3(c.y + 3 * (j - 1), yj);
                    sc = 1.0 / (1 + dist2(xx, yj) / d02);
                    if (kind == 2 && sxi == c.secy[j - 1]) sc = sc + 0.5;
                }
                const double d = diag_val + sc;
                double h = up_val;
                if (up_dir == 0) h += gap_open;
                double v = left_val;
                if (left_dir == 0) v += gap_open;
                int e;
                double val;
                if (d >= h && d >= v) {
                    e = 0;
                    val = d;
                } else if (v >= h) {
                    e = 1;
                    val = v;
                } else {
                    e = 2;
                    val = h;
                }
                dirb[(size_t)s * 64] = (uint8_t)e;
                left_val = out_val = val;
                left_dir = out_dir = e;
                diag_val = up_val;
                if (hand_on) {
                    c.rowval[j] = val;
                    c.rowdir[j] = (uint8_t)e;
                }
            }
        }
    }
    wave_sync();
    if (lane == 0) {
        int i = len1, j = len2;
        while (i > 0 && j > 0) {
            const int b = (i - 1) >> 6, l = (i - 1) & 63;
            const uint8_t e = c.dir[((size_t)b * steps + (j - 1 + l)) * 64 + l];
            if (e == 0) {
                y2x[j - 1] = i - 1;
                i--;
                j--;
            } else if (e == 1)
                j--;
            else
                i--;
        }
    }
    wave_sync();
}

__device__ void copy_map(Ctx &c, int *dst, const int *src) {
    for (int j = c.lane; j < c.ylen; j += 64) dst[j] = src[j];
    wave_sync();
}

// TMalign.cpp DP_iter: best map -> y2x_best; (t,u): the start superposition, updated
__device__ double DP_iter(Ctx &c, double t[3], double u[3][3], int *y2x_best, int g1, int g2, int iteration_max) {
    const double gap_open[2] = {-0.6, 0}, d02 = c.d0 * c.d0;
    double tmscore, tmscore_max = -1, tmscore_old = 0;
    for (int g = g1; g < g2; g++)
        for (int iteration = 0; iteration < iteration_max; iteration++) {
            NWDP_TM(c, 0, t, u, d02, gap_open[g], c.invmap_dp);
            const int k = pairs_of(c, c.invmap_dp);
            tmscore = TMscore8_search(c, k, t, u, 40, 8, c.d0_search, c.Lnorm, c.score_d8, c.d0);
            if (tmscore > tmscore_max) {
                tmscore_max = tmscore;
                copy_map(c, y2x_best, c.invmap_dp);
            }
            if (iteration > 0 && fabs(tmscore_old - tmscore) < 0.000001) break;
            tmscore_old = tmscore;
        }
    return tmscore_max;
}

// ---- initial alignments ----
__device__ void shift_map(Ctx &c, int *y2x, int k, int lim, int base) {     // y2x[j] = base + j + k where 0 <= j + k < lim
    for (int j = c.lane; j < c.ylen; j += 64) y2x[j] = (j + k >= 0 && j + k < lim) ? base + j + k : -1;
    wave_sync();
}

// TMalign.cpp get_initial: gapless threading, the LAST best shift (>=)
__device__ void get_initial(Ctx &c, int *y2x, double t[3], double u[3][3]) {
    const int min_len = c.xlen < c.ylen ? c.xlen : c.ylen;
    int min_ali = min_len / 2;
    if (min_ali <= 5) min_ali = 5;
    const int n1 = -c.ylen + min_ali, n2 = c.xlen - min_ali;
    int k_best = n1;
    double tmscore_max = -1;
    for (int k = n1; k <= n2; k += c.fast ? 5 : 1) {
        shift_map(c, y2x, k, c.xlen, 0);
        const double tmscore = get_score_fast(c, y2x, t, u);
        if (tmscore >= tmscore_max) {
            tmscore_max = tmscore;
            k_best = k;
        }
    }
    shift_map(c, y2x, k_best, c.xlen, 0);
}

// TMalign.cpp sec_str / make_sec
__device__ uint8_t sec_str(double dis13, double dis14, double dis15, double dis24, double dis25, double dis35) {
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

__device__ void make_sec(const Ctx &c, const double *x, int len, uint8_t *sec) {
    for (int i = c.lane; i < len; i += 64) {
        uint8_t s = 'C';
        if (i - 2 >= 0 && i + 2 < len) {
            double a[3], b[3], m[3], d[3], e[3];
            load3(x + 3 * (i - 2), a); load3(x + 3 * (i - 1), b); load3(x + 3 * i, m);
            load3(x + 3 * (i + 1), d); load3(x + 3 * (i + 2), e);
            s = sec_str(sqrt(dist2(a, m)), sqrt(dist2(a, d)), sqrt(dist2(a, e)), sqrt(dist2(b, d)), sqrt(dist2(b, e)),
                        sqrt(dist2(m, e)));
        }
        sec[i] = s;
    }
}

// TMalign.cpp get_initial5: local superposition of fragments of 20 and 100, the FIRST best (>)
__device__ bool get_initial5(Ctx &c, int *y2x) {
    const int xlen = c.xlen, ylen = c.ylen, aL = xlen < ylen ? xlen : ylen;
    double d01 = c.d0 + 1.5, t[3], u[3][3];
    if (d01 < c.D0_MIN) d01 = c.D0_MIN;
    const double d02 = d01 * d01;
    double GLmax = 0;
    int n_jump1 = xlen > 250 ? 45 : xlen > 200 ? 35 : xlen > 150 ? 25 : 15;
    if (n_jump1 > xlen / 3) n_jump1 = xlen / 3;
    int n_jump2 = ylen > 250 ? 45 : ylen > 200 ? 35 : ylen > 150 ? 25 : 15;
    if (n_jump2 > ylen / 3) n_jump2 = ylen / 3;
    int n_frag[2] = {20, 100};
    if (n_frag[0] > aL / 3) n_frag[0] = aL / 3;
    if (n_frag[1] > aL / 2) n_frag[1] = aL / 2;
    if (c.fast) {
        n_jump1 *= 5;
        n_jump2 *= 5;
    }
    bool flag = false;
    int *invmap = c.y2x_;
    for (int i_frag = 0; i_frag < 2; i_frag++) {
        const int m1 = xlen - n_frag[i_frag] + 1, m2 = ylen - n_frag[i_frag] + 1;
        for (int i = 0; i < m1; i += n_jump1)
            for (int j = 0; j < m2; j += n_jump2) {
                kabsch(c, FragSel{c, i, j}, n_frag[i_frag], t, u);
                NWDP_TM(c, 0, t, u, d02, 0.0, invmap);
                const double GL = get_score_fast(c, invmap, t, u);
                if (GL > GLmax) {
                    GLmax = GL;
                    copy_map(c, y2x, invmap);
                    flag = true;
                }
            }
    }
    return flag;
}

// TMalign.cpp get_initial_ssplus (score_matrix_rmsd_sec + NWDP_TM)
__device__ void get_initial_ssplus(Ctx &c, const int *y2x0, int *y2x) {
    double d01 = c.d0 + 1.5, t[3], u[3][3];
    if (d01 < c.D0_MIN) d01 = c.D0_MIN;
    const int k = pairs_of(c, y2x0);
    kabsch(c, PairSel{c, nullptr, 0}, k, t, u);
    NWDP_TM(c, 2, t, u, d01 * d01, -1.0, y2x);
}

// TMalign.cpp find_max_frag (every lane walks the chain: a short sequential scan)
__device__ void find_max_frag(const Ctx &c, const double *x, int len, int *start_max, int *end_max) {
    const int fra_min = c.fast ? 8 : 4;
    int Lfr_max = 0, inc = 0;
    int r_min = (int)(len * 1.0 / 3.0);
    if (r_min > fra_min) r_min = fra_min;
    double dcu_cut = c.dcu0 * c.dcu0;
    while (Lfr_max < r_min) {
        Lfr_max = 0;
        int j = 1, start = 0;
        double prev[3], cur[3];
        load3(x, prev);
        for (int i = 1; i < len; i++) {
            load3(x + 3 * i, cur);
            if (dist2(prev, cur) < dcu_cut) {
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
            prev[0] = cur[0]; prev[1] = cur[1]; prev[2] = cur[2];
        }
        if (Lfr_max < r_min) {
            inc++;
            if (inc > kMaxInc) break;
            const double dinc = c.prm->pow11[inc] * c.dcu0;
            dcu_cut = dinc * dinc;
        }
    }
}

// TMalign.cpp get_initial_fgt: gapless threading of the longest continuous fragment, the LAST best shift (>=).
// The fragment is a contiguous run of residues: ifr[i] = ifr0 + i.
__device__ void get_initial_fgt(Ctx &c, int *y2x, double t[3], double u[3][3]) {
    const int xlen = c.xlen, ylen = c.ylen, fra_min1 = (c.fast ? 8 : 4) - 1;
    int xstart = 0, ystart = 0, xend = 0, yend = 0;
    find_max_frag(c, c.x, xlen, &xstart, &xend);
    find_max_frag(c, c.y, ylen, &ystart, &yend);
    const int Lx = xend - xstart + 1, Ly = yend - ystart + 1;
    int L_fr = Lx < Ly ? Lx : Ly;
    const bool on_x = Lx < Ly || (Lx == Ly && xlen <= ylen);
    int ifr0 = on_x ? xstart : ystart;
    const int L0 = xlen < ylen ? xlen : ylen;
    if (L_fr == L0) {
        const int n1 = (int)(L0 * 0.1), n2 = (int)(L0 * 0.89);
        ifr0 += n1;
        L_fr = n2 - n1 + 1;
    }
    double tmscore, tmscore_max = -1;
    int *y2x_ = c.y2x_;
    if (on_x) {
        const int L1 = L_fr, min_len = L1 < ylen ? L1 : ylen;
        int min_ali = (int)(min_len / 2.5);
        if (min_ali <= fra_min1) min_ali = fra_min1;
        for (int k = -ylen + min_ali; k <= L1 - min_ali; k += c.fast ? 3 : 1) {
            shift_map(c, y2x_, k, L1, ifr0);
            tmscore = get_score_fast(c, y2x_, t, u);
            if (tmscore >= tmscore_max) {
                tmscore_max = tmscore;
                copy_map(c, y2x, y2x_);
            }
        }
    } else {
        const int L2 = L_fr, min_len = xlen < L2 ? xlen : L2;
        int min_ali = (int)(min_len / 2.5);
        if (min_ali <= fra_min1) min_ali = fra_min1;
        for (int k = -L2 + min_ali; k <= xlen - min_ali; k++) {
            // y2x_[ifr0 + j] = j + k for 0 <= j < L2 with 0 <= j + k < xlen, else -1
            for (int jj = c.lane; jj < ylen; jj += 64) {
                const int j = jj - ifr0;
                y2x_[jj] = (j >= 0 && j < L2 && j + k >= 0 && j + k < xlen) ? j + k : -1;
            }
            wave_sync();
            tmscore = get_score_fast(c, y2x_, t, u);
            if (tmscore >= tmscore_max) {
                tmscore_max = tmscore;
                copy_map(c, y2x, y2x_);
            }
        }
    }
}

// ---- TMalign_main ----
__device__ void tm_align_pair(Ctx &c, double *out_f, int *out_i, int *invmap_out) {
    const int xlen = c.xlen, ylen = c.ylen;
    make_sec(c, c.x, xlen, c.secx);
    make_sec(c, c.y, ylen, c.secy);
    wave_sync();
    double t[3], u[3][3], TM, TMmax = -1;
    int *invmap0 = c.invmap0, *invmap = c.invmap;
    const double ddcc = c.Lnorm <= 40 ? 0.1 : 0.4;
#define KEEP_IF_BETTER()                  \
    do {                                  \
        if (TM > TMmax) {                 \
            TMmax = TM;                   \
            copy_map(c, invmap0, invmap); \
        }                                 \
    } while (0)

    get_initial(c, invmap0, t, u);                                   // get_initial + detailed_search + DP_iter
    TM = detailed_search(c, invmap0, t, u, 40);
    if (TM > TMmax) TMmax = TM;
    TM = DP_iter(c, t, u, invmap, 0, 2, c.fast ? 2 : 30);
    KEEP_IF_BETTER();

    NWDP_TM(c, 1, t, u, 0.0, -1.0, invmap);                          // get_initial_ss
    TM = detailed_search(c, invmap, t, u, 40);
    KEEP_IF_BETTER();
    if (TM > TMmax * 0.2) {
        TM = DP_iter(c, t, u, invmap, 0, 2, c.fast ? 2 : 30);
        KEEP_IF_BETTER();
    }

    if (get_initial5(c, invmap)) {                                   // get_initial5
        TM = detailed_search(c, invmap, t, u, 40);
        KEEP_IF_BETTER();
        if (TM > TMmax * ddcc) {
            TM = DP_iter(c, t, u, invmap, 0, 2, 2);
            KEEP_IF_BETTER();
        }
    }

    get_initial_ssplus(c, invmap0, invmap);                          // get_initial_ssplus
    TM = detailed_search(c, invmap, t, u, 40);
    KEEP_IF_BETTER();
    if (TM > TMmax * ddcc) {
        TM = DP_iter(c, t, u, invmap, 0, 2, c.fast ? 2 : 30);
        KEEP_IF_BETTER();
    }

    get_initial_fgt(c, invmap, t, u);                                // get_initial_fgt
    TM = detailed_search(c, invmap, t, u, 40);
    KEEP_IF_BETTER();
    if (TM > TMmax * ddcc) {
        TM = DP_iter(c, t, u, invmap, 1, 2, 2);
        KEEP_IF_BETTER();
    }
#undef KEEP_IF_BETTER

    // final: detailed_search_standard, the pairs within score_d8 (n_ali8), RMSD, TM-scores by both lengths
    detailed_search(c, invmap0, t, u, c.fast ? 40 : 1);
    const int lali = pairs_of(c, invmap0);
    int n_ali8 = 0, n_ident = 0;
    for (int base = 0; base < lali; base += 64) {                    // in-place ordered compaction (writes land at <= k)
        const int k = base + c.lane;
        bool keep = false;
        int ix = 0, iy = 0;
        if (k < lali) {
            ix = c.ax[k];
            iy = c.ay[k];
            double xk[3], xx[3], yy[3];
            load3(c.x + 3 * ix, xk);
            transform(t, u, xk, xx);
            load3(c.y + 3 * iy, yy);
            keep = sqrt(dist2(xx, yy)) <= c.score_d8;
        }
        const unsigned long long m = __ballot(keep);
        const unsigned long long same = __ballot(keep && c.seqx[ix] == c.seqy[iy]);
        if (keep) {
            const int at = n_ali8 + prefix_before(m, c.lane);
            c.ax[at] = ix;
            c.ay[at] = iy;
        }
        n_ali8 += __popcll(m);
        n_ident += __popcll(same);
    }
    wave_sync();
    double rmsd = 0.0, qtm = 0.0, ttm = 0.0;
    if (n_ali8 > 0) {
        kabsch(c, PairSel{c, nullptr, 0}, n_ali8, t, u);
        double p = 0.0;
        for (int k = c.lane; k < n_ali8; k += 64) {
            double xk[3], xx[3], yy[3];
            load3(c.x + 3 * c.ax[k], xk);
            transform(t, u, xk, xx);
            load3(c.y + 3 * c.ay[k], yy);
            p += dist2(xx, yy);
        }
        rmsd = sqrt(wave_sum(p) / n_ali8);
        double tf[3], uf[3][3];
        qtm = TMscore8_search(c, n_ali8, tf, uf, 1, 0, c.prm->f_d0_search[xlen], xlen, c.score_d8, c.prm->f_d0[xlen]);
        ttm = TMscore8_search(c, n_ali8, tf, uf, 1, 0, c.prm->f_d0_search[ylen], ylen, c.score_d8, c.prm->f_d0[ylen]);
    }
    if (c.lane == 0) {
        out_f[0] = qtm;
        out_f[1] = ttm;
        out_f[2] = rmsd;
        out_i[0] = n_ali8;
        out_i[1] = n_ident;
        out_i[2] = MS_TM_OK;
    }
    if (invmap_out)
        for (int j = c.lane; j < ylen; j += 64) invmap_out[j] = invmap0[j];
}

__global__ void __launch_bounds__(64) ms_tmalign_kernel(const double *__restrict__ xyz, const uint8_t *__restrict__ seq,
                                                        const int64_t *__restrict__ offsets, int nstruct,
                                                        const int32_t *__restrict__ pairs, int npairs, int X, int Y, int fast,
                                                        char *__restrict__ workspace, size_t slot_bytes, double *out_f,
                                                        int32_t *out_i, int32_t *out_invmap) {
    __shared__ double rowval[kMaxLen + 1];
    __shared__ uint8_t rowdir[kMaxLen + 1];
    const SlotLayout L = slot_layout(X, Y);
    const TmParams *prm = reinterpret_cast<const TmParams *>(workspace);
    char *slot = workspace + kParamBytes + (size_t)blockIdx.x * slot_bytes;
    const int lane = threadIdx.x;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int s1 = pairs[2 * p], s2 = pairs[2 * p + 1];
        double *of = out_f + 3 * (size_t)p;
        int32_t *oi = out_i + 3 * (size_t)p;
        int status = MS_TM_OK;
        int64_t o1 = 0, o2 = 0, l1 = 0, l2 = 0;
        if (s1 < 0 || s1 >= nstruct || s2 < 0 || s2 >= nstruct) status = MS_TM_ERR_INDEX;
        else {
            o1 = offsets[s1]; l1 = offsets[s1 + 1] - o1;
            o2 = offsets[s2]; l2 = offsets[s2 + 1] - o2;
            if (l1 > X || l2 > Y || l1 > kMaxLen || l2 > kMaxLen) status = MS_TM_ERR_LONG;
            else if (l1 < kMinLen || l2 < kMinLen) status = MS_TM_ERR_SHORT;
        }
        if (status != MS_TM_OK) {
            if (lane == 0) {
                of[0] = of[1] = of[2] = 0.0;
                oi[0] = oi[1] = 0;
                oi[2] = status;
            }
            continue;
        }
        Ctx c;
        c.x = xyz + 3 * o1; c.y = xyz + 3 * o2;
        c.seqx = seq + o1; c.seqy = seq + o2;
        c.xlen = (int)l1; c.ylen = (int)l2;
        c.fast = fast; c.lane = lane; c.X = X; c.Y = Y;
        c.prm = prm;
        const int Lmin = c.xlen < c.ylen ? c.xlen : c.ylen;
        c.Lnorm = Lmin;                                              // parameter_set4search
        c.d0 = prm->s_d0[Lmin];
        c.D0_MIN = c.d0;
        c.d0_search = prm->s_d0_search[Lmin];
        c.score_d8 = prm->s_score_d8[Lmin];
        c.dcu0 = 4.25;
        c.dir = (uint8_t *)(slot + L.dir);
        c.ax = (int *)(slot + L.ax); c.ay = (int *)(slot + L.ay);
        c.ia = (int *)(slot + L.ia); c.ka = (int *)(slot + L.ka);
        c.dis = (double *)(slot + L.dis);
        c.secx = (uint8_t *)(slot + L.secx); c.secy = (uint8_t *)(slot + L.secy);
        c.invmap = (int *)(slot + L.invmap); c.invmap0 = (int *)(slot + L.invmap0);
        c.invmap_dp = (int *)(slot + L.invmap_dp); c.y2x_ = (int *)(slot + L.y2x_);
        c.rowval = rowval; c.rowdir = rowdir;
        tm_align_pair(c, of, oi, out_invmap ? out_invmap + (size_t)p * Y : nullptr);
        wave_sync();
    }
}

}  // namespace

extern "C" {

size_t ms_tmalign_workspace_bytes(int max_len1, int max_len2, int npairs) {
    if (max_len1 < 1 || max_len2 < 1 || npairs < 1 || max_len1 > kMaxLen || max_len2 > kMaxLen) return 0;
    return kParamBytes + (size_t)slot_count(max_len1, max_len2, npairs) * slot_layout(max_len1, max_len2).total;
}

int ms_tmalign_max_len(void) { return kMaxLen; }

int ms_tmalign_batch(const double *xyz, const uint8_t *seq, const int64_t *offsets, int nstruct, const int32_t *pairs, int npairs,
                     int max_len1, int max_len2, int flags, void *workspace, size_t workspace_bytes, double *out_f, int32_t *out_i,
                     int32_t *out_invmap, ms_stream_t stream) {
    if (!xyz || !seq || !offsets || !pairs || !workspace || !out_f || !out_i || nstruct < 1 || npairs < 1)
        MS_FAIL(MS_ERR_ARG, "ms_tmalign_batch: NULL argument, nstruct < 1 or npairs < 1");
    if (max_len1 < 1 || max_len2 < 1) MS_FAIL(MS_ERR_ARG, "ms_tmalign_batch: max_len1 / max_len2 must be >= 1");
    if (max_len1 > kMaxLen || max_len2 > kMaxLen)
        MS_FAIL(MS_ERR_RANGE, "ms_tmalign_batch: structures of up to %d residues are supported, asked for %d x %d", kMaxLen,
                max_len1, max_len2);
    if (flags & ~MS_TM_FAST) MS_FAIL(MS_ERR_ARG, "ms_tmalign_batch: unknown flags 0x%x", flags);
    const size_t per = slot_layout(max_len1, max_len2).total;
    if (workspace_bytes < kParamBytes + per) MS_FAIL(MS_ERR_WORKSPACE, "ms_tmalign_batch: workspace of %zu bytes, need at least %zu",
                                                     workspace_bytes, kParamBytes + per);
    int slots = slot_count(max_len1, max_len2, npairs);
    const size_t fit = (workspace_bytes - kParamBytes) / per;
    if ((size_t)slots > fit) slots = (int)fit;
    MS_HIP_CHECK(hipMemcpyAsync(workspace, host_params(), sizeof(TmParams), hipMemcpyHostToDevice, (hipStream_t)stream));
    hipLaunchKernelGGL(ms_tmalign_kernel, dim3(slots), dim3(64), 0, (hipStream_t)stream, xyz, seq, offsets, nstruct, pairs, npairs,
                       max_len1, max_len2, (flags & MS_TM_FAST) ? 1 : 0, (char *)workspace, per, out_f, out_i, out_invmap);
    MS_LAUNCH_CHECK("ms_tmalign_kernel");
    return MS_OK;
}

}  // extern "C"
