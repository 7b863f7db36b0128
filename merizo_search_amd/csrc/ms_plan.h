// Host-side planning of the search path: the library's switches, the decomposition of a scan launch, the carve of the caller's
// workspace and the rules the drivers in ms_search.hip share.  Plain C++17: it compiles without HIP (tests/c_abi/plan_fingerprint.cpp
// runs it on a CPU); under hipcc ms_plan_core is also device code (the exact pass behind a prefiltered search plans itself there).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/merizo_search_amd.h"

#ifdef __HIPCC__
#define MS_HOST_DEVICE __host__ __device__
#else
#define MS_HOST_DEVICE
#endif

// The decomposition of one scan launch: query tiles x row streams.  Computed on the host for an ordinary search (make_plan) and ON
// THE DEVICE for the exact pass behind a prefiltered search, whose batch -- the queries whose proof failed -- is only known there
// (the last workgroup of ms_rescore_kernel writes a ScanDevPlan, the gated scan and merge read it).
struct ScanDevPlan {
    int nq, nq_pad, n_qtiles, qwb, n_qgroups, n_sgroups, n_streams, rows_per_stream, P, grid;
    int pad_[6];
};
MS_HOST_DEVICE inline void ms_plan_core(int64_t n, int nq, int cus, ScanDevPlan *d) {
    d->nq = nq;
    d->n_qtiles = (nq + 31) / 32;
    d->qwb = d->n_qtiles >= 3 ? 4 : (d->n_qtiles == 2 ? 2 : 1);
    d->n_qgroups = (d->n_qtiles + d->qwb - 1) / d->qwb;
    d->nq_pad = d->n_qgroups * d->qwb * 32;
    const int64_t tiles = (n + 31) / 32;
    // one wave per (query tile, stream): one wave on each of the 4 * cus SIMDs
    int64_t want = ((int64_t)4 * cus) / ((int64_t)d->n_qgroups * d->qwb);
    if (want < 1) want = 1;
    if (want > tiles) want = tiles > 0 ? tiles : 1;
    const int64_t tiles_per_stream = (tiles + want - 1) / want;
    d->rows_per_stream = (int)((tiles_per_stream > 0 ? tiles_per_stream : 1) * 32);
    d->n_streams = (int)((n + d->rows_per_stream - 1) / d->rows_per_stream);
    if (d->n_streams < 1) d->n_streams = 1;
    const int spb = 4 / d->qwb;
    d->n_sgroups = (d->n_streams + spb - 1) / spb;
    d->P = d->qwb == 4 ? d->n_streams : d->n_sgroups;
    d->grid = ((d->n_sgroups + 7) / 8) * 8 * d->n_qgroups;
}

// ------------------------------------------------------------------ switches ----------
// Every environment variable of the search path: member, name, default (DESIGN.md "Switches of the search path" says what each one
// does and which test uses it).  All are diagnostics or tuning; each is read once per process, on first use.
#define MS_SETTINGS_TABLE(X)                                                       \
    X(int, loader_wave, "MS_LOADER_WAVE", 1)                                       \
    X(int, head_merge, "MS_HEAD_MERGE", 1)                                         \
    X(int, block_merge, "MS_BLOCK_MERGE", 1)                                       \
    X(int, list_sm, "MS_LIST_SM", 1)                                               \
    X(int, shared_bound, "MS_SHARED_BOUND", 1)                                     \
    X(int, prepass_tiles, "MS_PREPASS_TILES", -1)                                  \
    X(int, sample_min_nq, "MS_SAMPLE_MIN_NQ", 8)                                   \
    X(double, sample_coef, "MS_SAMPLE_COEF", 0.05)                                 \
    X(double, pf_sample_coef, "MS_PF_SAMPLE_COEF", 1.2)                            \
    X(int, bound_ranks, "MS_BOUND_RANKS", 0)                                       \
    X(int, fused_merge_max_nq, "MS_FUSED_MERGE_MAX_NQ", 2)                         \
    X(int, inkernel_norm_max_nq, "MS_INKERNEL_NORM_MAX_NQ", 4)                     \
    X(int, prefilter, "MS_PREFILTER", 1)                                           \
    X(int64_t, pf_few_min_rows, "MS_PF_FEW_MIN_ROWS", MS_PF_FEW_MIN_ROWS)          \
    X(int64_t, pf_few2_min_rows, "MS_PF_FEW2_MIN_ROWS", MS_PF_FEW2_MIN_ROWS)       \
    X(int, pf_pace, "MS_PF_PACE", 1)                                               \
    X(int, pf_rawq, "MS_PF_RAWQ", 1)                                               \
    X(int, pf_fuse_exact_max_nq, "MS_PF_FUSE_EXACT_MAX_NQ", 8)                     \
    X(int, pf_debug, "MS_PF_DEBUG", 0)

struct MsSettings {
#define MS_X(type, member, name, dflt) type member = dflt;
    MS_SETTINGS_TABLE(MS_X)
#undef MS_X
};

inline int ms_setting_value(const char *text, int) { return atoi(text); }
inline int64_t ms_setting_value(const char *text, int64_t) { return atoll(text); }
inline double ms_setting_value(const char *text, double) { return atof(text); }

// lookup(name) -> the variable's text or NULL (the process environment, or a test's own table)
template <class Lookup>
MsSettings ms_parse_settings(Lookup lookup) {
    MsSettings s;
#define MS_X(type, member, name, dflt) \
    if (const char *text = lookup(name)) s.member = ms_setting_value(text, s.member);
    MS_SETTINGS_TABLE(MS_X)
#undef MS_X
    if (s.prepass_tiles < -1) s.prepass_tiles = -1;      // (-1: the sample-size rule decides)
    return s;
}

inline const MsSettings &ms_settings() { static const MsSettings s = ms_parse_settings(getenv); return s; }

// <= 64 queries take the fp16-image scan from this many rows: 1..32 queries (one query tile, HBM-bound) / 33..64 (two tiles)
inline int64_t pf_few_min_rows(const MsSettings &s, int nq) { return nq > 32 && s.pf_few2_min_rows < s.pf_few_min_rows ? s.pf_few2_min_rows : s.pf_few_min_rows; }

// ------------------------------------------------------------------ rules -------------
// LDS scratch of ms_block_merge (ms_common.h) in front of the [k][P] entries it merges
constexpr int MS_BLOCK_MERGE_SCRATCH = 8192;
inline size_t block_merge_lds(int k, int P) { return (size_t)MS_BLOCK_MERGE_SCRATCH + (((size_t)k * P + 3) & ~(size_t)3) * 8; }
// the workgroup-per-query merge stages <= 256 lists per query whose entries fit the LDS of a CU next to its scratch
inline bool block_merge_takes(int k, int P) { return block_merge_lds(k, P) <= 156 * 1024 && P <= 256; }
// the last workgroup of a scan launch can merge the lists itself (ms_scan_body): they fit the LDS the scan has left
inline bool merge_fits_scan_launch(int k_pass, int P) { return P <= 256 && (size_t)k_pass * P <= 4224; }
// the fp16 image (64-row tiles; MS_PF_F16X2 / MS_PF_F16X1) as opposed to the split-bf16 image or none (`image`: a pointer will do)
inline bool is_f16_image(bool image, int format) { return image && format != MS_PF_BF16X3; }

// list entries per lane and pass, as an index into {5, 10, 16, 32}: 5 for k <= 10, 10 for k <= 20, 16 for k <= 32, else 32 (k <= 64)
constexpr int MS_KL[4] = {5, 10, 16, 32};
inline int pick_kl_index(int k_pass) {
    for (int i = 0; i < 3; ++i)
        if (2 * MS_KL[i] >= k_pass) return i;
    return 3;
}
inline int pick_kl(int k_pass) { return MS_KL[pick_kl_index(k_pass)]; }

// candidates kept per query: twice k for short lists, at least 8-16 spare entries for long ones (the proof needs the rows within the
// error bound of the k-th best to fit; more spare entries = fewer queries for the exact pass on clustered data)
inline int pf_list_len(int k) { return k <= 5 ? 10 : (k <= 10 ? 20 : (k <= 24 ? 32 : (k <= MS_PREFILTER_MAX_K ? 64 : 0))); }

// ------------------------------------------------------------------ workspace carve ---
// Regions are handed out front to back, each 256-byte aligned; a region is its byte offset plus a typed accessor.
struct MsCarve {
    size_t off = 0;
    template <class T> size_t take(size_t count) { const size_t at = off; off += (count * sizeof(T) + 255) / 256 * 256; return at; }
};
#define MS_REGION(T, name) size_t off_##name = 0; T *name(void *ws) const { return reinterpret_cast<T *>(static_cast<char *>(ws) + off_##name); }

struct ScanPlan {
    ScanDevPlan d;         // the launch (d.nq: the real queries)
    int k_pass;            // ranks per pass (<= 64)
    int kl;                // list entries per lane: smallest of {5,10,16,32} with 2*kl >= k_pass
    int prepass_tiles;     // tiles per stream scanned by the sample pass (0 = no sample pass)
    int qpw;               // split-image prefilter scan (ms_scan_pf.h): query tiles per wave (0: any other kernel)
    int list_sm;           // the scan of this plan writes stream-major lists (the image scans; the loader-wave kernel when the block merge takes them)
    bool hist_on;          // the sample pass starts the shared bound's histogram (ScanParams::hist) and the scan follows it
    size_t lds_bytes;
    MS_REGION(float, qn)          // [nq_pad][128] prepared queries
    MS_REGION(float, inv)         // [n] inverse row norms when the caller gave none
    MS_REGION(float, part_s) MS_REGION(uint32_t, part_i)      // [P][nq_pad][k_pass] partial lists: scores, rows
    MS_REGION(float, ub_s) MS_REGION(uint32_t, ub_i)          // [nq_pad] upper bound of the next pass (k > 64)
    MS_REGION(float, lb_s) MS_REGION(uint32_t, lb_i)          // [nq_pad] lower bound from the sample pass
    MS_REGION(float, scr_s) MS_REGION(int64_t, scr_i)         // [nq_pad][k_pass] the sample merge's own outputs
    MS_REGION(uint32_t, hist) MS_REGION(float, hstep)         // [nq_pad][16] counters of the shared bound, [nq_pad] bucket widths
    MS_REGION(uint32_t, prog)     // [n_streams][16] progress words of the image scan's workgroups
    size_t total = 0;
};

// qpw > 0: the plan of the split-image prefilter scan (ms_scan_pf.h): 4 waves x qpw query tiles per workgroup, one workgroup per CU
// tile_rows: rows per tile of that kernel's image (32: split-bf16, 64: fp16); streams are whole tiles
inline ScanPlan make_plan(const MsSettings &s, int cus, int64_t n, int nq, int k, int qpw = 0, int tile_rows = 32) {
    ScanPlan pl{};
    ScanDevPlan &d = pl.d;
    pl.qpw = qpw;
    pl.k_pass = k < 64 ? k : 64;
    pl.kl = pick_kl(pl.k_pass);
    int64_t tiles_per_stream;
    if (qpw == 0) {
        ms_plan_core(n, nq, cus, &d);      // (the same arithmetic the device runs for the exact pass behind a prefiltered search)
        tiles_per_stream = d.rows_per_stream / 32;
    } else {
        d.nq = nq;
        d.n_qtiles = (nq + 31) / 32;
        d.qwb = 4;                         // (one list per (stream, query), as in the loader-wave form)
        const int group_tiles = 4 * qpw;   // query tiles per workgroup
        d.n_qgroups = (d.n_qtiles + group_tiles - 1) / group_tiles;
        d.nq_pad = d.n_qgroups * group_tiles * 32;
        const int64_t big_tiles = (n + tile_rows - 1) / tile_rows;
        int64_t want = (int64_t)cus / d.n_qgroups;
        if (want < 1) want = 1;
        if (want > big_tiles) want = big_tiles > 0 ? big_tiles : 1;
        const int64_t big_per_stream = (big_tiles + want - 1) / want;
        tiles_per_stream = big_per_stream * (tile_rows / 32);           // (in 32-row units: the sample-size rule below)
        d.rows_per_stream = (int)((big_per_stream > 0 ? big_per_stream : 1) * tile_rows);
        d.n_streams = (int)((n + d.rows_per_stream - 1) / d.rows_per_stream);
        if (d.n_streams < 1) d.n_streams = 1;
        d.n_sgroups = d.n_streams;
        d.P = d.n_streams;
        d.grid = ((d.n_sgroups + 7) / 8) * 8 * d.n_qgroups;
    }
    pl.lds_bytes = 4 * 32768 + 4 * 1024;        // tile slots, cosine side data, in-launch bound
    pl.hist_on = d.qwb == 4 && s.loader_wave && s.shared_bound;
    // stream-major lists: the image scans always; the loader-wave kernel (>= 3 query tiles, one pass) when the workgroup-per-query merge
    // reads them -- MS_LIST_SM=0: rank-major as in rounds 1-4
    pl.list_sm = (qpw > 0 || (s.list_sm && d.qwb == 4 && s.loader_wave && k <= 64 && block_merge_takes(pl.k_pass, d.P))) ? 1 : 0;
    // sample pass: the k-th best score of the first few tiles of every stream bounds the answer
    // from below and prunes almost every insertion of the full pass; worth it for long streams
    // Size of the sample: T0 tiles per stream cost T0 tile times; the insertion steps they save in the
    // full pass fall as 1/T0 (candidates per tile = 1024 k / (streams * 32 * T0) while the sample's bound is
    // tighter than a stream's own list).  Minimum at T0 = sqrt(c * tiles_per_stream * k / streams), c from
    // the measured cost of a tile (2.2 us) and of a candidate (0.27 us): 3 tiles at 31 tiles per stream,
    // 9 at 244, 17 at 977 for k = 10 and 128 streams (sweeps at 125k-16M rows x 256 queries agree).
    // (... without the shared bound.  With it -- the loader-wave form of the fp32 scan -- the threshold follows the scan and
    //  the sample only has to start it: the optimum moves to ~0.4 of that, 3-4 tiles at C2 instead of 9 (0.518 against 0.526 ms per
    //  step) and 9 instead of 22 at k = 64 (0.665 against 0.719); profiles/r04_sample_size_sweep.log.  Below k = 5 the sample's best and
    //  k-th best scores are too close for the histogram to have buckets: the old rule)
    // MS_PF_SAMPLE_COEF, the constant for the image scans with more than 64 queries: twice the sample of the fp32 rule's 0.3 -- a visit of
    // the rare path costs these kernels ~900 cycles per half tile and a sample tile next to nothing (the sample launch is mostly fixed
    // cost): C2 0.145 -> 0.137 ms per call, every other shape within 1 % (profiles/r05_pf_sample_coef_sweep.log); few-query plans keep
    // 0.3.  (The split-image scan only appends between flushes: its thresholds move with the shared bound alone.)
    pl.prepass_tiles = s.prepass_tiles;
    if (pl.prepass_tiles < 0) {
        const double c = (qpw == 0 && pl.hist_on && pl.k_pass >= 5) ? s.sample_coef : (qpw > 0 && nq > 64 ? s.pf_sample_coef : 0.3);
        const double t0 = sqrt(c * (double)tiles_per_stream * ((double)pl.k_pass / 10.0) * (128.0 / (double)d.n_streams));
        pl.prepass_tiles = t0 < 1.0 ? 1 : (t0 > 32.0 ? 32 : (int)(t0 + 0.5));
    }
    if (tiles_per_stream < 8 * (int64_t)pl.prepass_tiles) pl.prepass_tiles = (int)(tiles_per_stream / 8);
    // short streams / few queries: few insertions anyway -- except in the image scans of the prefilter, whose lists only take candidates at
    // a flush and whose thresholds come from the sample and the shared bound alone: without a sample every tile visits the rare path
    // until the first flush (one query over 1M rows: 158 us against 62 with a sample)
    if (tiles_per_stream < 12 || k > 64 || (qpw == 0 && nq < s.sample_min_nq)) pl.prepass_tiles = 0;
    if (qpw > 0 && tile_rows == 64) pl.prepass_tiles = (pl.prepass_tiles + 1) / 2;                     // (counted in the kernel's own tiles)
    MsCarve c;
    const size_t lists = (size_t)d.P * d.nq_pad * pl.k_pass;
    pl.off_qn = c.take<float>((size_t)d.nq_pad * MS_DIM);
    pl.off_inv = c.take<float>((size_t)(n > 0 ? n : 1));
    pl.off_part_s = c.take<float>(lists);
    pl.off_part_i = c.take<uint32_t>(lists);
    pl.off_ub_s = c.take<float>(d.nq_pad);
    pl.off_ub_i = c.take<uint32_t>(d.nq_pad);
    pl.off_lb_s = c.take<float>(d.nq_pad);
    pl.off_lb_i = c.take<uint32_t>(d.nq_pad);
    pl.off_scr_s = c.take<float>((size_t)d.nq_pad * pl.k_pass);
    pl.off_scr_i = c.take<int64_t>((size_t)d.nq_pad * pl.k_pass);
    pl.off_hist = c.take<uint32_t>((size_t)d.nq_pad * 16);
    pl.off_hstep = c.take<float>(d.nq_pad);
    pl.off_prog = c.take<uint32_t>(qpw > 0 ? (size_t)d.n_streams * 16 : 0);
    pl.total = c.off;
    return pl;
}

// Workspace of a prefiltered search: [the larger of the prefilter scan's and the exact scan's plans | candidate lists (approximate
// scores, rows) | per-query flags | the compacted batch of the exact pass: queries, bounds, lengths, map | its device plan | its lists]
struct PfLayout {
    ScanPlan pf, exact;
    MS_REGION(float, as) MS_REGION(int64_t, ai) MS_REGION(uint32_t, flag)
    MS_REGION(float, qn_c) MS_REGION(float, lb_c) MS_REGION(float, qlen_c) MS_REGION(int, qmap)
    MS_REGION(ScanDevPlan, dp) MS_REGION(float, xs) MS_REGION(uint32_t, xi)
    size_t total = 0;
    int kp = 0, exact_grid_max = 0, exact_P_max = 0;
    bool ok = false;       // false: the prefilter does not serve the shape; the workspace is the fp32 search's (exact), every offset 0
};
inline PfLayout pf_layout(const MsSettings &s, int cus, int64_t n, int nq, int k, int mode, bool image, int format = MS_PF_BF16X3) {
    PfLayout L{};
    L.kp = pf_list_len(k);
    L.exact = make_plan(s, cus, n, nq, k);
    L.total = L.exact.total;
    L.exact_grid_max = L.exact.d.grid; L.exact_P_max = L.exact.d.P;
    const bool ip = mode == MS_MODE_IP_PRENORM || mode == MS_MODE_IP_NORMQ;
    const bool f16 = is_f16_image(image, format);
    // without an image the rows are split in registers (round 3's kernel: inner-product modes only, the loader-wave form)
    // (one or two query tiles -- the reference's own CLI regime -- are HBM-bound: over the fp16 image the scan reads half the bytes of
    //  the fp32 rows; worth the fixed cost of the pipeline around it from a few million rows: pf_few_min_rows)
    const bool few_ok = f16 && n >= pf_few_min_rows(s, nq);
    if (!(s.prefilter && L.kp > 0 && n >= 65536 && (L.exact.d.qwb == 4 || few_ok) &&
          (image ? (ip || mode == MS_MODE_COSINE_UNIT) : (ip && s.loader_wave != 0))))
        return L;
    // two query tiles per wave (8 per workgroup) from 5 query tiles, while the lists leave room for it
    const int qpw = image ? ((L.exact.d.n_qtiles >= 5 && L.kp <= 32) ? 2 : 1) : 0;
    L.pf = make_plan(s, cus, n, nq, L.kp, qpw, f16 ? 64 : 32);
    // the exact pass runs over 1 .. nq queries, decomposed on the device: the launch grid and the merge's LDS cover every case
    size_t lists_max = 0;        // (its partial lists: nq_pad * P entries per rank, whichever decomposition the device picks)
    for (int qt = 1; qt <= L.exact.d.n_qtiles; ++qt) {
        ScanDevPlan d;
        ms_plan_core(n, qt * 32 < nq ? qt * 32 : nq, cus, &d);
        if (d.grid > L.exact_grid_max) L.exact_grid_max = d.grid;
        if (d.P > L.exact_P_max) L.exact_P_max = d.P;
        if ((size_t)d.nq_pad * d.P > lists_max) lists_max = (size_t)d.nq_pad * d.P;
    }
    // the merges behind the image scan and the exact pass stage <= 256 lists per query (a device with more than 256 CUs): ms_ip_topk
    if (L.exact_P_max > 256 || L.pf.d.P > 256 || nq >= (1 << 20)) return L;
    L.ok = true;
    MsCarve c{L.pf.total > L.exact.total ? L.pf.total : L.exact.total};
    const size_t nq_pad = L.pf.d.nq_pad > L.exact.d.nq_pad ? L.pf.d.nq_pad : L.exact.d.nq_pad;
    L.off_as = c.take<float>(nq_pad * L.kp);
    L.off_ai = c.take<int64_t>(nq_pad * L.kp);
    L.off_flag = c.take<uint32_t>(nq_pad);
    L.off_qn_c = c.take<float>(nq_pad * MS_DIM);
    L.off_lb_c = c.take<float>(nq_pad);
    L.off_qlen_c = c.take<float>(nq_pad);
    L.off_qmap = c.take<int>(nq_pad);
    L.off_dp = c.take<ScanDevPlan>(1);
    L.off_xs = c.take<float>(lists_max * L.exact.k_pass);
    L.off_xi = c.take<uint32_t>(lists_max * L.exact.k_pass);
    L.total = c.off;
    return L;
}
// what ms_ip_topk_prefiltered_workspace_bytes answers: the largest layout of no image, the split-bf16 image (32-row tiles) and the
// fp16 image (64-row tiles)
inline size_t pf_workspace_bytes(const MsSettings &s, int cus, int64_t n, int nq, int k) {
    size_t m = make_plan(s, cus, n, nq, k).total;
    for (int image = 0; image < 3; ++image) {
        const size_t a = pf_layout(s, cus, n, nq, k, image ? MS_MODE_COSINE_UNIT : MS_MODE_IP_PRENORM, image != 0, image == 2 ? MS_PF_F16X2 : MS_PF_BF16X3).total;
        if (a > m) m = a;
    }
    return m;
}
