/*
 * merizo_search_amd.h -- C ABI of the MI355X (gfx950) Foldclass embed-and-search library.
 *
 * The reference (psipred/merizo_search) has no FFI: its hot path is Python calling torch /
 * faiss.  Each entry point below replaces one of those call sites; the citation names the
 * reference lines whose arithmetic the entry point performs.  All pointers are DEVICE
 * pointers owned by the caller unless a parameter says "host"; `stream` is a hipStream_t
 * (0 = the null stream).  Functions are asynchronous on `stream`, never allocate, never
 * synchronise.  Return 0 on success, a negative MS_ERR_* otherwise; ms_last_error() gives
 * the message of the calling thread's last failure.  Embedding width is fixed at 128
 * (FoldClassNet(128), reference programs/Foldclass/dbsearch.py:40).
 * Threading: entry points may be called from any host thread; a WORKSPACE serves one stream at a time (calls that share a workspace
 * must be ordered on one stream: the searches keep lists, counters and the exact pass's launch plan in it between their launches) --
 * concurrent searches take one workspace each.  One exception to "never allocate, never synchronise": the FIRST search on a workspace
 * (and the first after its record was handed on, ms_wsstate.h) allocates the library's own 512-byte block of counters for it and
 * waits until the null stream has zeroed it, once, before anything is launched on `stream`.  A prefiltered search whose bookkeeping was disturbed all the same (a second stream on
 * its workspace, a launch aborted half way) does not answer: the exact pass queued behind it finds the re-scoring's verdict missing
 * and TRAPS (round 6; ms_debug_prefilter_poison is the test's way in).  For the same reason the prefiltered entry points
 * (ms_ip_topk_prefiltered and its _prepare / _scan / _finish stages) CANNOT BE CAPTURED INTO A GRAPH: the base of the compaction's ticket
 * and the epochs of the call are kernel arguments, counted on by the host from call to call, so a replay would carry stale ones and trap.
 *
 * Environment: the search path has a handful of diagnostic and tuning switches (MS_LOADER_WAVE, MS_PREPASS_TILES, ...), each read once
 * per process; DESIGN.md, "Switches of the search path", is the one table of their names, defaults and meanings.
 *
 * Paths below are relative to /root/reference/merizo_search/programs/Foldclass/.
 */
#ifndef MERIZO_SEARCH_AMD_H
#define MERIZO_SEARCH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS_DIM 128
#define MS_OK 0
#define MS_ERR_ARG (-1)       /* bad argument (NULL pointer, k < 1, d != 128, ...) */
#define MS_ERR_WORKSPACE (-2) /* workspace too small */
#define MS_ERR_HIP (-3)       /* a HIP call / kernel launch failed */
#define MS_ERR_RANGE (-4)     /* structure longer than the positional table, n >= 2^31, ... */

typedef void *ms_stream_t;

/* Library / device introspection. */
int ms_version(void);
const char *ms_last_error(void);
int ms_device_count(void);
int ms_device_cu_count(void);
/* PCI bus id ("0000:c1:00.0") of HIP's current device into buf (len >= 16): lets the ranks of a multi-GPU run prove that they sit
 * on DISTINCT devices (bench.py gathers it into every N > 1 line; the reference's own multi-GPU call, faiss.index_cpu_to_all_gpus,
 * dbsearch.py:228-230, has no such check). */
int ms_device_pci_bus_id(char *buf, int len);
/* The few-query shortcuts of ms_ip_topk as this build applies them (defaults 2 and 4; the environment variables
 * MS_FUSED_MERGE_MAX_NQ / MS_INKERNEL_NORM_MAX_NQ override them): up to *fused_merge_max_nq queries the scan launch merges its own
 * lists (one launch per search), up to *inkernel_norm_max_nq queries MS_MODE_IP_NORMQ normalises inside the scan launch. */
void ms_small_batch_thresholds(int *fused_merge_max_nq, int *inkernel_norm_max_nq);
int ms_prefilter_max_k(void); /* MS_PREFILTER_MAX_K */

/* ------------------------------------------------------------------ search ---------- */

/* Score semantics of ms_ip_topk. */
#define MS_MODE_IP_PRENORM 0 /* faiss path: database rows and queries used as given (inner product);
                                 knn_exact_faiss, dbsearch.py:213-248 */
#define MS_MODE_COSINE_RAW 1 /* `.pt` path: F.cosine_similarity(db, q) * mask over a RAW database;
                                 search_query_against_db, dbsearch.py:75-81 */
#define MS_MODE_COSINE_UNIT 2 /* the same `.pt` search over rows the caller has L2-normalised once with
                                 ms_l2_normalize_rows(db, eps = 1e-8) -- cosine_similarity's own normalise-then-dot
                                 (dbsearch.py:78) with the row half done ahead of time: no inv_norm array, the
                                 scores leave the matrix pipe final and the scan runs at the inner-product rate;
                                 queries are still given raw, lengths / qlen / mincov mask as in COSINE_RAW */
#define MS_MODE_IP_NORMQ 3   /* the faiss path with its query normalisation fused in: q is RAW, F.normalize(q) (eps 1e-12,
                                 dbsearch.py:303-304) is applied inside the call -- by the scan launch's own waves for a handful
                                 of queries (ms_small_batch_thresholds: 4 by default), by one small preparation launch in front
                                 of it otherwise -- then knn_exact_faiss as in MS_MODE_IP_PRENORM.  Bit-identical to
                                 ms_l2_normalize_rows_to + MS_MODE_IP_PRENORM */

/* F.normalize(x) in place: x[r,:] /= max(||x[r,:]||_2, eps).  dbsearch.py:303-304 (eps 1e-12);
 * also the per-operand normalisation inside F.cosine_similarity (eps 1e-8), dbsearch.py:78. */
int ms_l2_normalize_rows(float *x, int64_t n, int d, float eps, ms_stream_t stream);
/* The same, out of place (what F.normalize itself does): y[r,:] = x[r,:] / max(||x[r,:]||_2, eps); x is not
 * modified, y may not overlap x.  Bit-identical to ms_l2_normalize_rows on a copy. */
int ms_l2_normalize_rows_to(const float *x, float *y, int64_t n, int d, float eps, ms_stream_t stream);

/* inv_norm[r] = 1 / max(||x[r,:]||_2, eps): the database half of F.cosine_similarity
 * (dbsearch.py:78), computed once per database instead of once per query. */
int ms_row_inv_norms(const float *x, int64_t n, int d, float eps, float *inv_norm, ms_stream_t stream);

/* Bytes of scratch ms_ip_topk needs for a database shard of n rows, nq queries, top k. */
size_t ms_ip_topk_workspace_bytes(int64_t n, int nq, int k);

/* Exact top-k of nq queries against n database rows (row-major float32 [n,128], resident in HBM).
 *   mode MS_MODE_IP_PRENORM: score = <db[r], q>; replaces IndexFlat.add/search + `I += i0`
 *        for one block or shard (dbsearch.py:234-242).  inv_norm/lengths/qlen must be NULL.
 *   mode MS_MODE_COSINE_RAW: score = cos(db[r], q) * mask, mask = (qlen[q] >= lengths[r]*mincov)
 *        (dbsearch.py:76-79); masked rows score (+-)0.0 and stay candidates, as in the
 *        reference.  q is raw (normalised internally, eps 1e-8); inv_norm = ms_row_inv_norms(db,
 *        1e-8) or NULL (then computed into the workspace on every call, as the reference does).
 *        lengths/qlen NULL = no mask.
 * Output: out_scores float32 [nq,k], out_idx int64 [nq,k] = row_offset + row, sorted by score
 * descending, ties by ascending row (torch.topk / faiss leave tie order unspecified).  If
 * n < k the tail is (-inf, -1), like faiss.  Any k >= 1 is accepted (k > 64 costs
 * ceil(k/64) scans; ms_ip_topk_large below returns the same lists from one filtered pass).
 * n must be < 2^31. */
int ms_ip_topk(const float *db, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode,
               const float *inv_norm, const float *lengths, const float *qlen, float mincov, float *out_scores,
               int64_t *out_idx, void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* The three stages of ms_ip_topk for k <= 64, exposed so that a profiler / bench can time the
 * scan kernel alone.  Call them in order with identical arguments:
 *   ms_ip_topk_prepare  cosine mode: queries -> normalised padded copy (inner-product mode reads the
 *                       caller's 16-byte aligned array in place), inverse row norms if absent,
 *                       and the sample pass (best rows of the first tiles of every row stream -> a
 *                       lower bound on each query's k-th best score);
 *   ms_ip_topk_scan     ONE launch of the fused score + top-k scan over all remaining rows
 *                       (ms_scan_loader_kernel for batches of >= 3 query tiles, else ms_scan_kernel);
 *   ms_ip_topk_finish   merge of the per-stream lists into the outputs. */
int ms_ip_topk_prepare(const float *db, int64_t n, const float *q, int nq, int k, int mode, const float *inv_norm,
                       const float *lengths, const float *qlen, float mincov, void *workspace,
                       size_t workspace_bytes, ms_stream_t stream);
int ms_ip_topk_scan(const float *db, int64_t n, const float *q, int nq, int k, int mode, const float *inv_norm,
                    const float *lengths, const float *qlen, float mincov, void *workspace, size_t workspace_bytes,
                    ms_stream_t stream);
int ms_ip_topk_finish(int64_t n, int64_t row_offset, int nq, int k, float *out_scores, int64_t *out_idx,
                      void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* ---- large k: the lists of ms_ip_topk for 64 < k <= MS_LARGE_K_MAX from ONE filtered pass over the rows ----
 *
 * ms_ip_topk serves k > 64 with ceil(k/64) fp32 scans.  This entry point returns the same [nq,k] lists, bit for bit, from one
 * fp32 read (the bound) and one read behind the 16-bit matrix pipe (the emission), for the queries it can serve; it says per
 * query whether it did.
 * EXACTNESS.  For query q take ANY threshold t[q] and put every row whose exact score is >= t[q] into a bin of
 * MS_LARGE_K_CAND slots.  If the bin received at least k rows and did not overflow, the best k of the bin in the search's total
 * order (score descending, row ascending, -0.0 == +0.0) are the best k of the whole database: every row outside the bin scores
 * below t[q], hence below k rows of the bin.  Nothing else is assumed of t[q].  The call's own t[q]: the rows are cut into
 * G = ceil(k/64) contiguous groups, ms_ip_topk (k = 64, the call's mode and mask) runs on each -- one read of the database in
 * all -- and t[q] is the k-th largest of those 64 G scores: at least k real rows reach it.  The emission is ms_threshold_edges'
 * with a cut per query: a cell whose fp16 score is below t[q] - E * row_norm_bound * |q| is proved below the cut, every other
 * cell is scored with the exact chain of 128 fmaf (ms_ip_topk's score, bit for bit), masked, and emitted iff score >= t[q]
 * (NaN fails, +inf passes, -0.0 counts as 0.0).  A masked search filters on the UNMASKED score; that is sound only while
 * t[q] > 0 (a masked row scores +-0.0, which a non-positive cut would have to emit): a masked query whose t[q] is not > 0 is
 * status 2 and emits nothing.
 *   mode             MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ, or MS_MODE_COSINE_UNIT with or without the length mask (lengths float32
 *                    [n] and qlen float32 [nq] go together, NULL NULL = no mask; NULL in the other modes).  MS_MODE_COSINE_RAW:
 *                    MS_ERR_ARG, as in the prefiltered search.
 *   row_norm_bound   as in ms_threshold_edges: NaN, <= 0 or outside [2^-40, 2^40] is MS_ERR_RANGE; it need not hold (a row above it,
 *                    or a query the fp16 filter cannot take, has all its cells scored exactly).
 *   out_scores / out_idx   ms_ip_topk's contract exactly: float32 / int64 [nq,k], row_offset + row, (-inf, -1) padding, +inf scores
 *                    first, NaN and -inf never returned.
 *   out_status       int32 [nq]: 0 = row q of the outputs is final.  1 = the bin overflowed: row q of the outputs is (-inf, -1)
 *                    throughout and out_lb[q] is the k-th best of the MS_LARGE_K_CAND buffered entries -- real rows with exact
 *                    scores, so a valid and tighter threshold for a second call.  2 = not served, the caller must use ms_ip_topk
 *                    for this query (row q is (-inf, -1) throughout): t[q] is NaN or -inf (fewer than k returnable rows); the
 *                    bin overflowed for a query the fp16 filter cannot take; a masked search whose t[q] is not > 0; a given
 *                    threshold that left the bin below k entries.
 *   out_lb           float32 [nq]: status 0 or 2: the threshold that was used; status 1: see above.
 *   lb_in            NULL, or float32 [nq] thresholds that replace the call's own (the second round: lb_in = the out_lb of the
 *                    first).  A NaN or -inf entry is status 2; one that is too high (fewer than k rows reach it) is status 2,
 *                    never a wrong answer.
 *   out_stats        int64 [4], may be NULL: [0] [1] [2] the queries with status 0, 1, 2, [3] the cells sent to the exact chain;
 *                    written by the call's last launch, the counters reset by the call.
 * Shapes the route does not take -- k <= 64, k > MS_LARGE_K_MAX, n < 128 G (n = 0 included) -- are answered by ms_ip_topk inside
 * the call: status 0 for every query, out_lb = -inf, out_stats[3] = -1 (lb_in is ignored).  The workspace covers that route too:
 * ms_ip_topk_large_workspace_bytes(n, nq, k) bytes, 16-byte aligned (0 for nq < 1, n < 0, k < 1 or n >= 2^31 - 1).
 * MS_ERR_ARG: another mode, nq < 1, n < 0, k < 1, NULL pointers, lengths / qlen outside MS_MODE_COSINE_UNIT or only one of them,
 * db or workspace not 16-byte aligned; MS_ERR_RANGE: the bound, n >= 2^31 - 1; MS_ERR_WORKSPACE: a short workspace.  Nothing is
 * launched on an error.
 * Asynchronous on `stream`, never allocates, never synchronises.  Every counter lives in the workspace and is reset by the
 * call: a workspace serves the next call, with another nq or k, without clean-up.  Vector stores and vector atomics only (one
 * global atomic per emitted cell, one per wave for out_stats[3], one per query for the status counts); no scratch memory.
 * MS_LARGE_K_CAND = 8192: one 64 KB sort of 8-byte keys in LDS per query.
 * Backward compatible additions: ms_version() stays 210. */
#define MS_LARGE_K_MAX 2048   /* 64 G <= 2048 group-list scores per query */
#define MS_LARGE_K_CAND 8192  /* candidates a query's bin holds */
size_t ms_ip_topk_large_workspace_bytes(int64_t n, int nq, int k);
int ms_ip_topk_large(const float *db, int64_t n, int64_t row_offset, const float *q, int nq, int k, int mode,
                     const float *lengths, const float *qlen, float mincov, float row_norm_bound,
                     const float *lb_in, float *out_scores, int64_t *out_idx,
                     int32_t *out_status, float *out_lb, int64_t *out_stats,
                     void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* ---- the prefiltered search: the same results as ms_ip_topk bit for bit, several times faster for large batches ----
 *
 * Replaces index.search of dbsearch.py:234-242 (MS_MODE_IP_PRENORM / MS_MODE_IP_NORMQ) and, on rows normalised once,
 * search_query_against_db of dbsearch.py:75-81 (MS_MODE_COSINE_UNIT) for batches of more than 64 queries, k <= MS_PREFILTER_MAX_K and
 * databases of >= 65,536 rows.  The rows are scanned once with 16-bit matrix instructions on an image of the database (fp16 rows
 * against split fp16 queries, or bf16 hi + lo halves of both), which gives every score to within E |row| |q| (E = 2.5e-4 .. 1.05e-3
 * by format, below); the 2k-4k best rows per query by that score are re-scored
 * with the exact fp32 chain (ms_ip_topk's own arithmetic, from the fp32 rows) and the best k of them are returned -- after a
 * PER-QUERY proof that no other row can belong to the answer (the k-th exact score exceeds the last kept approximate score by
 * more than the error bound).  Queries whose proof fails (dozens of rows within the error bound of their k-th best: families of
 * near-duplicates) are gathered into a dense batch on the device and an exact fp32 scan, queued behind on the same stream, runs
 * for THOSE queries only: always exact, never an approximation, and a clustered query costs only itself.
 *
 *   pf_image / pf_format   an MFMA-ready image of db made once, when the database becomes resident (ms_pf_build_image), next to the
 *                    fp32 rows -- which stay: the re-scoring and the exact pass read them.  The scan then streams operands and
 *                    converts nothing.  Three arithmetics, all with the same exact results (E = the bound on |approximate - exact|
 *                    the proof uses, in units of |row| |q|; ms_pf_err_coef):
 *                      MS_PF_BF16X3  rows AND queries split into bf16 hi + lo, 3 matrix instructions per 16 dimensions, 512 B per
 *                                    row, E = 2.5e-4 (round 4);
 *                      MS_PF_F16X2   rows rounded to fp16, queries split into fp16 hi + lo, 2 matrix instructions per 16
 *                                    dimensions, 256 B per row, E = 5.5e-4 (round 5; the default of the Python driver);
 *                      MS_PF_F16X1   the SAME image as MS_PF_F16X2, the query's hi part only: 1 matrix instruction per 16
 *                                    dimensions, E = 1.05e-3 (more queries fail their proof on clustered data).
 *                    pf_format of a search must be the arithmetic the image was built for (F16X2 and F16X1 share one image; the
 *                    fp16 image carries a trailer the scan checks: a mismatch traps instead of answering).
 *                    pf_image NULL: the rows are split in registers instead (bf16 x 3; no second copy of anything; about 2.5x
 *                    slower; inner-product modes only -- MS_MODE_COSINE_UNIT without an image is ms_ip_topk); pf_format is ignored.
 *   lengths / qlen / mincov   MS_MODE_COSINE_UNIT: the length mask of dbsearch.py:76 (NULL, NULL: none); NULL in the other modes.
 *   row_norm_bound   an upper bound on the L2 norm of every row of db (1.0 + 1e-6 for unit rows, as dbfname_IP and
 *                    MS_MODE_COSINE_UNIT hold; 1 / min(ms_row_inv_norms) otherwise); <= 0, not finite (a database with non-finite
 *                    rows has no bound) or shapes outside the above: the call is ms_ip_topk.  Queries with non-finite elements
 *                    (fp16 formats: or a norm outside [2^-40, 2^40]) fail their proof and get the exact pass.
 *                    ms_pf_build_image takes it too: the fp16 image stores row * 2^sr with sr chosen from it (components below
 *                    2^15; outside [2^-40, 2^40] the fp16 formats are declined with MS_ERR_RANGE); MS_PF_BF16X3 ignores it.
 * Workspace: ms_ip_topk_prefiltered_workspace_bytes.  _prepare / _scan / _finish: its three stages as for ms_ip_topk
 * (queries + sample pass; the one scan launch; merge + exact re-scoring + the exact pass over the flagged queries).
 * ABI note: ms_version() == 210 (round 6: + ms_device_pci_bus_id, ms_debug_prefilter_poison; signatures of 200 unchanged); >= 200 (round 5) -- ms_pf_image_bytes / ms_pf_build_image gained `pf_format` (+ row_norm_bound), the four
 * search entry points gained `pf_format` behind `pf_image`; version 100 callers must be rebuilt (merizo_search_amd/_lib.py checks). */
#define MS_PREFILTER_MAX_K 48
/* <= 64 queries (the reference's own CLI regime, dbsearch.py:531-546) are HBM-bound up to 32 queries and two query tiles of fp32
 * matrix work from 33: over the fp16 image (MS_PF_F16X2 / F16X1) the scan reads 256 B per row instead of 512 and multiplies in fp16,
 * and from a row count on that outweighs the fixed cost of the pipeline around it -- ms_ip_topk_prefiltered then serves ANY number
 * of queries (below it, and over a split-bf16 image or none, <= 64 queries are ms_ip_topk as before).  The row count: 1M rows for 1..32
 * queries, 200k rows for 33..64 (measured: profiles/r05_few_query_image_sweep.log); ms_pf_few_min_rows(nq): the value in force
 * (the environment variables MS_PF_FEW_MIN_ROWS / MS_PF_FEW2_MIN_ROWS override). */
#define MS_PF_FEW_MIN_ROWS 1000000
#define MS_PF_FEW2_MIN_ROWS 200000
int64_t ms_pf_few_min_rows(int nq);
#define MS_PF_BF16X3 0
#define MS_PF_F16X2 1
#define MS_PF_F16X1 2
size_t ms_pf_image_bytes(int64_t n, int pf_format);
int ms_pf_build_image(const float *db, int64_t n, int pf_format, float row_norm_bound, void *pf_image, ms_stream_t stream);
float ms_pf_err_coef(int pf_format);      /* E of the format, per unit of |row| |q|; < 0: unknown format */
size_t ms_ip_topk_prefiltered_workspace_bytes(int64_t n, int nq, int k);
int ms_ip_topk_prefiltered(const float *db, const void *pf_image, int pf_format, int64_t n, int64_t row_offset, const float *q, int nq,
                           int k, int mode, const float *lengths, const float *qlen, float mincov, float row_norm_bound,
                           float *out_scores, int64_t *out_idx, void *workspace, size_t workspace_bytes, ms_stream_t stream);
int ms_ip_topk_prefiltered_prepare(const float *db, const void *pf_image, int pf_format, int64_t n, const float *q, int nq, int k, int mode,
                                   const float *lengths, const float *qlen, float mincov, float row_norm_bound, void *workspace,
                                   size_t workspace_bytes, ms_stream_t stream);
int ms_ip_topk_prefiltered_scan(const float *db, const void *pf_image, int pf_format, int64_t n, const float *q, int nq, int k, int mode,
                                const float *lengths, const float *qlen, float mincov, float row_norm_bound, void *workspace,
                                size_t workspace_bytes, ms_stream_t stream);
int ms_ip_topk_prefiltered_finish(const float *db, const void *pf_image, int pf_format, int64_t n, int64_t row_offset, const float *q,
                                  int nq, int k, int mode, const float *lengths, const float *qlen, float mincov,
                                  float row_norm_bound, float *out_scores, int64_t *out_idx, void *workspace,
                                  size_t workspace_bytes, ms_stream_t stream);
/* Diagnostics (tests; synchronises the device): what the last prefiltered search on this workspace left behind -- *flagged =
 * how many of its queries needed the exact pass (0: every answer was proved), *gate_value == *last_epoch iff any did. */
int ms_debug_prefilter_state(void *workspace, unsigned int *gate_value, unsigned int *last_epoch, unsigned int *flagged);
/* Diagnostics (tests; synchronises the device): overwrite the slot counter and the ticket of this workspace's compaction -- the state
 * an aborted launch or a second stream would leave.  The next prefiltered search on the workspace must fail loudly. */
int ms_debug_prefilter_poison(void *workspace, unsigned int slot_counter, unsigned int ticket);
/* Diagnostics (tools/pf_debug.py): the candidate lists of the last prefiltered search on this workspace, copied to the host
 * (approximate scores float32 [nq][kp], rows int64 [nq][kp]); image: 0 = no image, 1 = the split-bf16 image, 2 = the fp16 image; -1 when the shape is
 * not served by the prefilter. */
int ms_debug_prefilter_lists(void *workspace, int64_t n, int nq, int k, int image, float *as_host, int64_t *ai_host, int *kp_out);
/* Test hook (tests/merge_case.py): the final merge of a search on lists the CALLER wrote -- P lists of k slots for each of nq queries,
 * every list sorted best first (score descending, row ascending), empty slots (-inf, 0xFFFFFFFF) last, rows distinct across the lists
 * of a query.  The launch is the one a search makes for this (P, k): the workgroup merge for P <= 256, the head-advance merge or the
 * pool merge beyond (MS_BLOCK_MERGE / MS_HEAD_MERGE as in a search).  All pointers are device memory, 16-byte aligned lists.
 *   part_s / part_i  sm_nq_pad == 0: rank-major, entry (rank r, list l) of query q at (q * k + r) * P + l;
 *                    sm_nq_pad >= nq: stream-major, at (l * sm_nq_pad + q) * k + r
 *   sparse           != 0: the pool form the prefiltered search uses on its mostly empty lists (ignored when ub_s is given)
 *   out_s / out_i    rank r of query q at q * out_stride + col0 + r: float32 score, int64 row + row_offset, (-inf, -1) padding
 *   ub_s / ub_i      both NULL, or [nq]: the k-th entry (score, row without the offset; (-inf, 0xFFFFFFFF) when there are fewer)
 *   dp_scratch       NULL, or 64 bytes the hook fills on `stream` with a device plan of dp_nq <= nq queries and dp_P <= P lists (the
 *                    exact pass behind a prefiltered search): the lists are then laid out rank-major with dp_P, only the first dp_nq
 *                    queries are merged and query q is written to output row qmap[q] (qmap: NULL or int32 [dp_nq]; only with a plan)
 * MS_ERR_ARG: NULL or misaligned lists, k outside 1..64, nq < 1, P < 1, out_stride < col0 + k, a plan outside its launch;
 * MS_ERR_RANGE: what the search's own merge launch declines (more than 1024 lists; a plan or stream-major lists that the workgroup
 * merge does not take).  Nothing is launched on an error. */
int ms_debug_merge_lists(const float *part_s, const unsigned int *part_i, int P, int nq, int k, int sm_nq_pad, int sparse, int64_t row_offset,
                         float *out_s, int64_t *out_i, int out_stride, int col0, float *ub_s, unsigned int *ub_i, int dp_nq, int dp_P,
                         const int *qmap, void *dp_scratch, ms_stream_t stream);
/* Test hook: the lower bound a sampled search takes from its sample pass -- lb[q] = the k-th largest (with multiplicity) of the first
 * `ranks` entries of the P lists of query q (part_s laid out as above; -inf = an empty slot), -inf when there are fewer than k.
 * hist / hstep: both NULL, or uint32 [nq][16] counters (zeroed) and float [nq] bucket widths of the shared bound.
 * MS_ERR_ARG: NULL pointers, k outside 1..64, nq < 1, P < 1, only one of hist / hstep; MS_ERR_RANGE: ranks < 1, ranks > k,
 * ranks * P > 2048 (a search merges such lists instead). */
int ms_debug_sample_bound(const float *part_s, int P, int nq, int k, int ranks, int sm_nq_pad, float *lb, unsigned int *hist, float *hstep,
                          ms_stream_t stream);

/* Merge S sorted result lists per query into the best k: faiss.ResultHeap(nq,k).add_result /
 * finalize (dbsearch.py:224,240,245) and the cross-shard merge after the RCCL all-gather.
 * scores float32 [S,nq,k], idx int64 [S,nq,k] (idx < 0 = padding), each list sorted best-first
 * (score descending, index ascending); an index appears in at most one list (shards / blocks are
 * disjoint row ranges).  Any S >= 1. */
int ms_topk_merge(const float *scores, const int64_t *idx, int S, int nq, int k, float *out_scores,
                  int64_t *out_idx, ms_stream_t stream);

/* The same merge when list s of each array starts s * stride BYTES after list 0 -- e.g. straight out of
 * the all-gather buffer, where every rank contributed one packed block [scores f32 nq*k | rows i64 nq*k]
 * (no unpack copy between the collective and the merge). */
int ms_topk_merge_strided(const float *scores, const int64_t *idx, int64_t score_stride_bytes, int64_t idx_stride_bytes,
                          int S, int nq, int k, float *out_scores, int64_t *out_idx, ms_stream_t stream);

/* Exact removal of excluded rows from top-k lists: the step behind the scan when a database is searched against itself
 * (every query finds its own row first, the sibling domains of its chain next; the reference has no such search -- its
 * callers filter hit tables by hand).  Per query q, from a list of kin entries sorted as ms_ip_topk leaves it (score
 * descending, row ascending, (-inf, -1) padding last):
 *   - entries whose row lies in [lo[q], hi[q]) are dropped (global row numbers; lo[q] >= hi[q]: nothing is excluded);
 *   - entries whose score is below min_score are dropped (-inf: no cut; NaN is refused);
 *   - what remains keeps its order, the first kout entries are written, the tail is padded with (-inf, -1);
 *   - out_count[q] = the number of real entries written.
 * scores float32 [nq,kin], idx int64 [nq,kin], lo / hi int64 [nq], out_scores float32 [nq,kout], out_idx int64 [nq,kout],
 * out_count int32 [nq]; the outputs may not overlap the inputs.  NULL pointers, nq < 1, kout < 1 and kin < kout: MS_ERR_ARG.
 * One wave per query, the list read in 64-entry pieces (any kin), order preserved by a ballot compaction.
 * EXACTNESS: a database with the rows [lo, hi) removed has its best kout rows among the best kout + (hi - lo) rows of the
 * whole database (at most hi - lo of those are excluded, and removing rows does not reorder the others).  So if the input is
 * the exact top-kin of the whole database and kin >= kout + (hi[q] - lo[q]) for every query, the output is the exact
 * top-kout of the database without those rows -- scores and order included -- as long as min_score cuts nothing; with a
 * cut it is that list's entries at or above min_score.  Backward compatible addition: ms_version() stays 210. */
int ms_topk_drop_ranges(const float *scores, const int64_t *idx, int nq, int kin, const int64_t *lo, const int64_t *hi,
                        float min_score, int kout, float *out_scores, int64_t *out_idx, int32_t *out_count,
                        ms_stream_t stream);

/* Greedy representative clustering of a database of n rows from its neighbour lists: what `cluster` runs behind the
 * self-search (the reference has no clustering; its users cluster hit tables in other programs).
 *   nbr_idx int64 [n,k], nbr_score float32 [n,k]: per row k entries (row j, score s) in the layout ms_topk_drop_ranges writes
 *   ((-inf, -1) padding); lengths int32 [n]: the domain lengths.  The order of a list's entries does not matter.
 * A directed entry i -> j is VALID when 0 <= j < n, j != i, s is not NaN, s >= min_score and
 * (float)min(L_i, L_j) >= mincov * (float)max(L_i, L_j) in fp32; every other entry is ignored (rows outside [0, n) are never
 * dereferenced).  i ~ j when either direction is valid, with the larger of the directed scores as weight (-0.0 counts as +0.0).
 * Priority: the longer domain, the smaller row on equal length.  The representatives are the lexicographically-first
 * maximal independent set under that priority (a row is one exactly when none of its higher-priority neighbours is: the
 * result of cd-hit's sequential greedy pass).  Then, on the final set: out_rep[i] = i, out_rep_score[i] = 1.0f for a
 * representative; every other row gets the adjacent representative of largest weight, the smaller row on equal weights,
 * and that weight.  The result is a function of the inputs alone: no run-to-run or launch-order dependence.
 * out_rep int64 [n], out_rep_score float32 [n]: device.  HOST pointers: *out_n_reps = representatives, *out_rounds = rounds
 * of the mark / decide launch pair it took (1..n), *out_saturated = rows whose k entries are ALL valid (such a list may
 * have been cut short by k: neighbours beyond it are unknown to the clustering).
 * Unlike the entry points above this one SYNCHRONISES: it reads the count of undecided rows back every few rounds, and it
 * returns after all its work on `stream` has finished.  workspace: ms_cluster_workspace_bytes(n) bytes (0 for n outside
 * [1, 2^31 - 1]), 16-byte aligned, initialised by the call.
 * MS_ERR_ARG: NULL pointers, n < 1, n > 2^31 - 1, k < 1, NaN min_score (-inf: no cut), mincov outside [0, 1] or NaN, a
 * workspace that is too small.  Backward compatible additions: ms_version() stays 210. */
size_t ms_cluster_workspace_bytes(int64_t n);
int ms_cluster_greedy(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int32_t *lengths,
                      float min_score, float mincov, int64_t *out_rep, float *out_rep_score,
                      int64_t *out_n_reps, int32_t *out_rounds, int64_t *out_saturated,
                      void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* ms_cluster_greedy over the UNION of the lists' entries and m extra directed entries edge_src[e] -> edge_dst[e] with score
 * edge_score[e] (int64 [m], int64 [m], float32 [m], device): what `cluster --complete` runs on the lists plus the output of
 * ms_threshold_edges.  An extra entry is valid under the rule above with i = edge_src[e]; an edge_src outside [0, n) makes it
 * invalid, and such a row is never dereferenced (nor is an edge_dst outside [0, n)).  Duplicates -- of list entries or of each
 * other -- change nothing: the weight of i ~ j is the larger of the directed scores.  Every output is defined as above on that
 * union; the same entries split in any way between lists and extras give identical outputs, *out_rounds included.
 * k == 0 with NULL lists is allowed (extra entries only), m == 0 with NULL edge arrays is allowed.  *out_saturated counts over
 * the lists only (0 when k == 0).  The workspace is ms_cluster_workspace_bytes(n), unchanged.
 * ms_cluster_greedy is this call with m == 0.  MS_ERR_ARG: k < 0, m < 0, a NULL pointer that the counts make necessary, and
 * what ms_cluster_greedy refuses.  Synchronises like ms_cluster_greedy.  Backward compatible addition: ms_version() stays 210. */
int ms_cluster_greedy_edges(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                            const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths, float min_score,
                            float mincov, int64_t *out_rep, float *out_rep_score, int64_t *out_n_reps, int32_t *out_rounds,
                            int64_t *out_saturated, void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* Connected components (single linkage) of the SAME graph: what `cluster --cluster_mode connected` runs.  The inputs are those
 * of ms_cluster_greedy_edges -- lists [n,k] (k == 0 with NULL lists: none), m extra directed entries (m == 0 with NULL arrays:
 * none), lengths, min_score, mincov -- and a directed entry is valid under exactly the rule of ms_cluster_greedy (row inside
 * [0, n), no self-loop, score not NaN and >= min_score, the fp32 coverage inequality; an edge_src or a row outside [0, n) is never
 * dereferenced).  i ~ j when either direction is valid, with the larger of the directed scores as weight (-0.0 counts as +0.0).
 * A component is a connected component of ~.  Its representative is its highest-priority row: the longest domain, the smaller
 * row on equal length (the priority of ms_cluster_greedy).  out_rep[i] = the representative of i's component.
 * out_link_score[i] = 1.0f for a representative (a row without a valid entry is one: a singleton); for every other row the
 * largest weight among the row's OWN valid incident edges, in either direction: the strongest link that ties the row to its
 * cluster.  (A member need not be adjacent to its representative: the graph holds no "score to the representative".)
 * HOST pointers: *out_n_components = components, *out_saturated = rows whose k list entries are ALL valid (over the lists only, 0
 * when k == 0), *out_rounds = hook / compress rounds it took (1..n), for information.
 * out_rep, out_link_score and *out_n_components are functions of the set of entries alone: identical however the same entries
 * are split between lists and extras, in whatever order, with whatever duplicates, run after run; *out_saturated is one of the
 * lists alone.  *out_rounds is NOT promised: how many trees one round merges depends on what concurrent reads of the parent
 * array return.
 * workspace: ms_cluster_components_workspace_bytes(n) bytes (0 for n outside [1, 2^31 - 1]), 16-byte aligned, initialised by the
 * call.  MS_ERR_ARG: what ms_cluster_greedy_edges refuses.  Synchronises like ms_cluster_greedy_edges: it reads the rounds'
 * "changed" words back every few rounds and returns after all its work on `stream` has finished.
 * Backward compatible addition: ms_version() stays 210. */
size_t ms_cluster_components_workspace_bytes(int64_t n);
int ms_cluster_components(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                          const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths, float min_score,
                          float mincov, int64_t *out_rep, float *out_link_score, int64_t *out_n_components, int32_t *out_rounds,
                          int64_t *out_saturated, void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* The single-linkage tree of the SAME graph: what `cluster --tree` and `cluster --levels` run.  The inputs are those of
 * ms_cluster_components, entry for entry: the same validity rule, an edge_src or a row outside [0, n) never dereferenced, i ~ j when
 * either direction is valid, the larger of the valid directed scores as weight (-0.0 counts as +0.0), k == 0 with NULL lists and
 * m == 0 with NULL edge arrays allowed.
 * Order the undirected edges STRICTLY: weight descending, then (min(i,j), max(i,j)) ascending.  The FOREST is the spanning forest
 * Kruskal's algorithm builds in that order (the maximum spanning forest; the order makes it unique).  Cutting it at any T >=
 * min_score -- keeping its edges of weight >= T -- gives exactly the connected components of the graph cut at T, and the largest
 * weight among a row's own forest edges >= T is the largest among its own graph edges >= T (every row's best edge is in the forest):
 * ms_cluster_components on the forest's edges as extra entries (k == 0) returns, at every such T, what it returns on the graph.
 * The forest is a function of the SET of valid entries alone: not of how they are split between lists and extras, of their order,
 * of duplicates, of timing or of the run.
 * Outputs (device): out_pairs int32 [n][2], out_weight float32 [n], all n slots written by the call.  A row stops being the root of
 * its tree at most once; the edge it hooked by is stored in the row's OWN slot r: out_pairs[r] = {a, b} with a < b, out_weight[r]
 * its weight.  {-1, -1} and -inf mark a row that never hooked (one per component).  Which row holds which edge: in a round every
 * tree selects its first outgoing edge in the order and its root hooks by it; when two trees select the same edge, the root with
 * the LARGER row hooks and the smaller stays a root.  (So the slots, too, are a function of the entry set.)
 * HOST pointers: *out_n_edges = filled slots = n - components; *out_saturated as in ms_cluster_components; *out_rounds = rounds up
 * to and including the first that found no entry between two trees.  Every tree with such an entry merges in every round, so
 * *out_rounds <= floor(log2 n) + 1, and it is a function of the entry set: PROMISED, unlike ms_cluster_components' count.
 * workspace: ms_cluster_tree_workspace_bytes(n) bytes (0 for n outside [1, 2^31 - 1]), 16-byte aligned, initialised by the call; a
 * used one serves the next call with another n.  MS_ERR_ARG: what ms_cluster_greedy_edges refuses; nothing is launched on an error.
 * Synchronises like ms_cluster_components: one 16-byte read-back per group of rounds, and it returns after all its work on
 * `stream` has finished.  Backward compatible addition: ms_version() stays 210. */
size_t ms_cluster_tree_workspace_bytes(int64_t n);
int ms_cluster_tree(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                    const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths, float min_score,
                    float mincov, int32_t *out_pairs, float *out_weight, int64_t *out_n_edges, int32_t *out_rounds,
                    int64_t *out_saturated, void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* The distinct unordered pairs of the SAME graph, and a verdict per pair written back onto it: what `cluster --mintm` runs around
 * its TM-align stage.  The graph arguments are those of ms_cluster_greedy_edges -- lists [n,k] (k == 0 with NULL lists: none), m
 * extra directed entries (m == 0 with NULL arrays: none), lengths, min_score, mincov -- a directed entry is VALID under exactly
 * the rule of ms_cluster_greedy (an edge_src or a row outside [0, n) is never dereferenced), and the priority is its priority.
 * The CANONICAL pair of a valid entry i -> j is (a, b): a the higher-priority row of {i, j}, b the other one.
 *
 * ms_cluster_pairs: out_count int64 [2] (device): out_count[0] = the number of distinct canonical pairs over all valid entries,
 * exact whatever cap is; out_count[1] = the list rows whose k entries are ALL valid (*out_saturated of the cluster calls, 0 when
 * k == 0: reported here because the lists are about to be edited).  out_pairs int32 [cap][2] (device): its first min(count, cap)
 * slots hold distinct canonical pairs {a, b}, in unspecified order; nothing is written at or behind slot cap; cap == 0 only
 * counts (out_pairs may then be NULL).  The pair SET is a function of the inputs alone: it does not depend on how the same
 * entries are split between lists and extras, on their order or on duplicates; slot numbers are not promised.  The workspace is
 * left holding the set (pair -> slot) for the two calls below.  Asynchronous on `stream`; never allocates; the workspace --
 * ms_cluster_pairs_workspace_bytes(n, k, m) bytes (0 for n outside [1, 2^31 - 1], k < 0, m < 0 or n k + m >= 2^31), 16-byte
 * aligned -- is initialised by the call itself and serves the next ms_cluster_pairs call without clean-up.
 *
 * ms_cluster_pairs_apply: the same graph arguments (n, k and m as in the building call), written in place; keep uint8 [count]
 * (device), indexed by slot; the workspace as ms_cluster_pairs left it.  Every VALID directed entry whose pair has
 * keep[slot] == 0 is overwritten: a list entry becomes (-inf, -1), an extra edge_dst = -1, edge_score = -inf.  A valid entry is
 * removed as well (fail closed) when its pair is not in the set, when its slot is >= count, or >= the cap of the building call.
 * Invalid entries are left bit for bit as they were.  *out_removed (int64 [1], device) = the directed entries removed.  After
 * it the cluster calls above see exactly the graph without the rejected pairs, in both directions.  Asynchronous.
 *
 * ms_cluster_pairs_find: a / b int64 [cnt] (device); out_slot[e] (int64 [cnt], device) = the slot of the unordered pair
 * {a[e], b[e]}, in either order; -1 when the pair is not in the set (or was counted behind cap), when a row is outside [0, n)
 * and when a[e] == b[e].  n as in the building call; the set is found through the workspace's own head.  Asynchronous.
 *
 * MS_ERR_ARG: what ms_cluster_greedy_edges refuses, a negative cap / count / cnt, a workspace that is not 16-byte aligned;
 * MS_ERR_RANGE: n k + m >= 2^31; MS_ERR_WORKSPACE: a workspace that is too small.
 * Backward compatible additions: ms_version() stays 210. */
size_t ms_cluster_pairs_workspace_bytes(int64_t n, int k, int64_t m);
int ms_cluster_pairs(const int64_t *nbr_idx, const float *nbr_score, int64_t n, int k, const int64_t *edge_src,
                     const int64_t *edge_dst, const float *edge_score, int64_t m, const int32_t *lengths, float min_score,
                     float mincov, int32_t *out_pairs, int64_t cap, int64_t *out_count, void *workspace, size_t workspace_bytes,
                     ms_stream_t stream);
int ms_cluster_pairs_apply(int64_t *nbr_idx, float *nbr_score, int64_t n, int k, const int64_t *edge_src, int64_t *edge_dst,
                           float *edge_score, int64_t m, const int32_t *lengths, float min_score, float mincov,
                           const uint8_t *keep, int64_t count, const void *workspace, size_t workspace_bytes,
                           int64_t *out_removed, ms_stream_t stream);
int ms_cluster_pairs_find(const int64_t *a, const int64_t *b, int64_t cnt, const int32_t *lengths, int64_t n,
                          const void *workspace, size_t workspace_bytes, int64_t *out_slot, ms_stream_t stream);

/* The score matrices of the multi-domain search's `exhaustive_cosine` mode: step 3 of dbsearch_fulllength.py (:468-483) with
 * the search's own score in place of TM-align -- the "embscore mode" that file leaves as a TODO (:202-203, :558-571).
 * Candidate c = cand[c] = {q0, nqd, t_off, nhd} is one (query chain, target chain) pair: its query domains are rows
 * [q0, q0 + nqd) of q [nq,128], its target domains the nhd rows db[trows[t_off + j]] of db [n,128] (trows int64 [ntrows], a
 * ragged list; rows may repeat).  Its matrix is written row-major [nqd,nhd] at out_scores + mat_off[c] (mat_off int64
 * [ncand], in floats; the caller lays the matrices out, gaps are left alone).
 *   cell (i, j) = EXACTLY the score ms_ip_topk reports for query q0 + i and row trows[t_off + j] in `mode`, bit for bit:
 *        MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ or MS_MODE_COSINE_UNIT (others: MS_ERR_ARG); the queries are prepared by the
 *        scan's own preparation launch into the workspace, the dot is the scan's chain (s = 0..63: element s, then element
 *        64 + s, one fmaf each), MS_MODE_COSINE_UNIT multiplies by the length mask (qlen[q] >= lengths[row] * mincov;
 *        lengths float32 [n] and qlen float32 [nq] go together, NULL NULL = no mask; NULL in the other modes);
 *   cut: a score that is NaN or < min_score is stored as +0.0f; a score equal to min_score stays; -inf cuts nothing;
 *   out_match int32 [ncand][2] = {rows of the matrix with a non-zero entry, columns with a non-zero entry} after the cut
 *        (-0.0 is zero): the caller keeps a candidate only if [0] == nqd and [1] >= nqd.
 * Descriptors are data, not trusted: a trows entry outside [0, n) is never dereferenced, its cells are +0.0f; a candidate
 * with nqd < 1, nhd < 1, nqd or nhd > 4096, [q0, q0 + nqd) outside [0, nq] or [t_off, t_off + nhd) outside [0, ntrows]
 * gets out_match = {-1, -1} and nothing else is written for it.
 * ncand == 0 succeeds without a launch.  MS_ERR_ARG: NULL pointers, nq < 1, ncand < 0, another mode, a NaN min_score, db or
 * workspace not 16-byte aligned; MS_ERR_WORKSPACE: fewer than ms_md_chain_scores_workspace_bytes(nq) bytes (0 for nq < 1).
 * One wave per candidate, one lane per cell (the chain is sequential); vector stores only.  Backward compatible
 * additions: ms_version() stays 210. */
size_t ms_md_chain_scores_workspace_bytes(int nq);
int ms_md_chain_scores(const float *db, int64_t n, const float *q, int nq, int mode, const float *lengths, const float *qlen,
                       float mincov, const int32_t *cand, int ncand, const int64_t *trows, int64_t ntrows,
                       const int64_t *mat_off, float min_score, float *out_scores, int32_t *out_match, void *workspace,
                       size_t workspace_bytes, ms_stream_t stream);

/* The pass over ALL rows of the multi-domain search's `database_cosine` mode: which (query chain, target chain) pairs of a
 * whole database pass the two early exits of the mapping step -- the pairs ms_md_chain_scores would report with
 * out_match == {nqd, >= nqd} if it were given every pair as a candidate -- found in one read of the rows, without matrices.
 * Target chain c is the run of rows [chain_start[c], chain_start[c + 1]) of db [n,128] (chain_start int64 [nchains + 1],
 * device; database rows of one chain are adjacent).  Rules: chain_start[0] == 0, chain_start[nchains] == n, strictly
 * increasing.  The table is data, not trusted: it is VALIDATED by a small launch of its own before any row is read; a table
 * that breaks a rule gives *out_count = -1 and no pair, and no address outside db [0, n) is ever formed from it.
 * Query chain g is rows [q0, q0 + nqd) of q [nq,128], with qchain int32 [nqc][2] = {q0, nqd} (device).
 *   cell (i, j) of the pair (g, c) = EXACTLY the cell ms_md_chain_scores writes for query q0 + i and row chain_start[c] + j in
 *        `mode` (MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ or MS_MODE_COSINE_UNIT): the queries prepared by the scan's own
 *        preparation launch into the workspace, the same chain of 128 fmaf, the length mask of MS_MODE_COSINE_UNIT (lengths
 *        float32 [n], qlen float32 [nq], mincov; NULL NULL = no mask; NULL in the other modes), and the same cut: NaN or
 *        < min_score counts as +0.0f, a score equal to min_score stays, -0.0 is zero, -inf cuts nothing;
 *   (g, c) QUALIFIES iff every one of the nqd rows of that matrix has a non-zero cell and at least nqd columns have one.
 * *out_count (int64, device) = the number of qualifying pairs over all (g, c); the first min(count, cap) slots of out_pairs
 * (int64 [cap][2] = {query chain, target chain}, device) hold distinct qualifying pairs in unspecified order; nothing is
 * written at or behind slot cap; cap == 0 only counts (out_pairs may then be NULL).
 * out_qstatus int32 [nqc] (device) = 0, or -1 for a descriptor with nqd < 1, nqd > 64 or [q0, q0 + nqd) outside [0, nq]: such a
 * query chain reports no pair.  64 query domains per query chain is the limit of this entry point (one 64-bit mask of matched
 * query domains per target chain).  A target chain may have ANY number of rows: one longer than a wave's tile of 64 rows is
 * looped over (there is no 4096 limit here).
 * nqc == 0, nchains == 0 or n == 0 succeed with *out_count = 0.  MS_ERR_ARG: NULL pointers, nq < 1, n, nchains, nqc or cap < 0,
 * another mode, a NaN min_score, db or workspace not 16-byte aligned; MS_ERR_WORKSPACE: fewer than
 * ms_md_chain_scan_workspace_bytes(n, nq) bytes (0 for nq < 1 or n < 0).
 * Asynchronous on `stream`, never allocates, vector stores only.  The slot counter and the table's status word live in the
 * workspace and are reset by the call itself: a workspace serves the next call without any clean-up by the host.
 * One lane per target row, whole chains per wave.  Backward compatible additions: ms_version() stays 210. */
size_t ms_md_chain_scan_workspace_bytes(int64_t n, int nq);
int ms_md_chain_scan(const float *db, int64_t n, const int64_t *chain_start, int64_t nchains, const float *q, int nq, int mode,
                     const float *lengths, const float *qlen, float mincov, const int32_t *qchain, int nqc, float min_score,
                     int64_t *out_pairs, int64_t cap, int64_t *out_count, int32_t *out_qstatus, void *workspace,
                     size_t workspace_bytes, ms_stream_t stream);

/* ms_md_chain_scan for MANY queries: the same definition, served by the 16-bit matrix pipe in front of the exact cell.
 * For every input ms_md_chain_scan accepts, the qualifying pairs are the same SET (their order in out_pairs is unspecified in
 * both), *out_count is the same and out_qstatus is the same; the table is validated the same way (*out_count = -1, no row
 * read); the cap rule is the same (counted, never written at or behind cap; cap == 0 only counts); the return codes are the
 * same; nqd > 64 is still status -1; a target chain may have any number of rows; nq and nqc are not limited.
 * How: an approximate score a from fp16 operands (the operands and scalings of MS_PF_F16X1: row * 2^sr and query * 2^sq
 * rounded to nearest even, fp32 accumulation) obeys |a - s| <= E |row| |q| with E = ms_pf_err_coef(MS_PF_F16X1), s the exact
 * cell's chain of 128 fmaf.  The scan's threshold is FIXED, so a cell with a < min_score - E * row_norm_bound * |q| is proved
 * zero; every other cell is re-scored with the exact chain, mask and cut.  Nothing can fail to be proved: the verdicts are
 * those of ms_md_chain_scan bit for bit.  In MS_MODE_COSINE_UNIT the filter works on the unmasked score (the mask multiplies
 * by 0 or 1) and the mask is applied in the exact cell.
 *   row_norm_bound   as in ms_pf_build_image: an upper bound on the L2 norm of the rows (1.0 + 1e-6 for unit rows).  NaN, <= 0
 *                    or outside [2^-40, 2^40]: MS_ERR_RANGE.  It need not hold: a row whose fp32 sum of squares exceeds
 *                    row_norm_bound^2 (1 + 1e-5) or is not finite has ALL its cells re-scored exactly, as has a query with a
 *                    non-finite element, a zero norm or a norm outside [2^-40, 2^40].  min_score = -inf proves nothing and is
 *                    served correctly at the speed of one lane per cell.
 *   out_stats        int64 [1], device, may be NULL: out_stats[0] = the number of (query, row) cells this call sent to the exact
 *                    re-score; written by the call's last launch, its counter reset by the call itself.
 * Asynchronous on `stream`, never allocates; the workspace (ms_md_chain_scan_mq_workspace_bytes(n, nq) bytes; 0 for nq < 1 or
 * n < 0; MS_ERR_WORKSPACE below that) serves the next call without clean-up.  Vector stores only (LDS atomics; at most one
 * global atomic per wave and emission, one per wave for out_stats); no scratch memory.
 * Backward compatible additions: ms_version() stays 210. */
size_t ms_md_chain_scan_mq_workspace_bytes(int64_t n, int nq);
int ms_md_chain_scan_mq(const float *db, int64_t n, const int64_t *chain_start, int64_t nchains, const float *q, int nq, int mode,
                        const float *lengths, const float *qlen, float mincov, const int32_t *qchain, int nqc, float min_score,
                        int64_t *out_pairs, int64_t cap, int64_t *out_count, int32_t *out_qstatus, float row_norm_bound,
                        int64_t *out_stats, void *workspace, size_t workspace_bytes, ms_stream_t stream);

/* Every (query, row) cell of db [n,128] x q [nq,128] whose score is at or above a fixed threshold, as a list: the range search
 * behind `cluster --complete` (the rows whose neighbour lists came back full get ALL their neighbours from it).
 *   Cell (qi, r), qi in [0, nq), r in [0, n), has score s = EXACTLY the score ms_ip_topk reports for that query and row in
 *        `mode` (MS_MODE_IP_PRENORM, MS_MODE_IP_NORMQ or MS_MODE_COSINE_UNIT with no length mask; others: MS_ERR_ARG): the
 *        queries prepared by the scan's own preparation launch into the workspace, the dot the chain of 128 fmaf that
 *        ms_md_chain_scores documents (s = 0..63: element s, then element 64 + s).
 *   The cell is EMITTED iff s >= min_score and the global row row_offset + r lies outside [lo[qi], hi[qi]).  NaN is never
 *        emitted; -inf as min_score cuts nothing.  lo / hi: int64 [nq], device, they go together; NULL NULL = nothing excluded.
 *        An emitted cell writes out_src = qi, out_dst = row_offset + r, out_score = s as computed (-0.0 stays -0.0).
 *   *out_count (int64, device) = the number of emitted cells, exact even when it exceeds cap; the first min(count, cap) slots
 *        of out_src / out_dst / out_score (int64, int64, float32 [cap], device) hold distinct emitted cells in unspecified
 *        order; nothing is written at or behind slot cap; cap == 0 only counts (the three arrays may then be NULL).
 *   row_norm_bound, out_stats: as in ms_md_chain_scan_mq -- the fp16 matrix pipe proves a cell below min_score when its
 *        approximate score is below min_score - E * row_norm_bound * |q|, every other cell is computed exactly.  The bound need
 *        not hold: a row above it, or a query the filter cannot serve, has all its cells scored exactly.  out_stats[0] = the
 *        number of cells sent to the exact chain (NULL: not reported).
 * n == 0 succeeds with *out_count = 0.  Error codes as ms_md_chain_scan_mq's, in its order: MS_ERR_ARG for another mode, nq < 1,
 * n < 0, cap < 0, NULL pointers, only one of lo / hi, a NaN min_score, db or workspace not 16-byte aligned; MS_ERR_RANGE for a
 * row_norm_bound that is NaN, <= 0 or outside [2^-40, 2^40] and for n >= 2^31; MS_ERR_WORKSPACE below
 * ms_threshold_edges_workspace_bytes(n, nq) bytes (0 for nq < 1 or n < 0).
 * Asynchronous on `stream`, never allocates; the slot counter lives in the workspace and is reset by the call: the workspace
 * serves the next call without clean-up.  Vector stores and vector atomics only (one global atomic per wave and drain of its
 * list of unproved cells, one per wave for out_stats); no scratch memory.  One route serves any nq >= 1 (padded to the 32-query
 * tile; the results do not depend on it).  Backward compatible additions: ms_version() stays 210. */
size_t ms_threshold_edges_workspace_bytes(int64_t n, int nq);
int ms_threshold_edges(const float *db, int64_t n, int64_t row_offset, const float *q, int nq, int mode, const int64_t *lo,
                       const int64_t *hi, float min_score, float row_norm_bound, int64_t *out_src, int64_t *out_dst,
                       float *out_score, int64_t cap, int64_t *out_count, int64_t *out_stats, void *workspace,
                       size_t workspace_bytes, ms_stream_t stream);

/* The best mapping of every (query chain, target chain) candidate: the step behind ms_md_chain_scores, on its buffers.
 * Candidate c has a matrix M [nqd,nhd], row-major, at scores + mat_off[c] (scores float32 [total_cells]) -- what
 * ms_md_chain_scores wrote: cut cells are +0.0f.  cand is the [ncand][4] array that call takes; only nqd = cand[c][1] and
 * nhd = cand[c][3] are read.
 *   cell (i, j) is ALLOWED iff M[i][j] != 0 and it is not NaN (-0.0 is zero).  Its weight is the integer
 *        w = llrint(clamp((double) M[i][j], -2^20, 2^20) * 2^32), rounded to nearest even: exact for 2^-9 <= |M[i][j]| <= 2^20.
 *        Totals are int64 sums of w: "maximum" carries no rounding, no summation order and no floating-point ties.
 *   kind 0, any order: a mapping gives every query domain i a distinct column path[i] with every cell (i, path[i]) allowed;
 *        one mapping of maximum total is reported.  Which one: rows are inserted in order 0..nqd-1 by shortest augmenting
 *        path with row and column potentials on the costs -w (the classic O(nqd^2 nhd) form: the search stands on a column,
 *        relaxes the slack of every unvisited column from that column's row, moves to the unvisited column of smallest
 *        slack, shifts the potentials by that slack, until it reaches an unmatched column); every argmin over columns
 *        takes the smallest column.
 *   kind 1, order-preserving: the same with path strictly increasing.  D[0][j] = w[0][j]; D[i][j] = w[i][j] + max over
 *        j' < j of D[i-1][j'], over allowed cells with a finite prefix.  The last column is the smallest argmax of D[nqd-1];
 *        each earlier column is the smallest argmax of D[i] over the columns below the one chosen after it.
 * Outputs (device); EVERY entry of every candidate is written, so the result is a function of the inputs alone:
 *   out_status int32 [ncand][2], per kind: 1 = mapping found, 0 = none exists, -1 = bad descriptor (nqd < 1, nhd < 1,
 *        mat_off[c] < 0 or mat_off[c] + nqd * nhd > total_cells), -2 = beyond this entry point's limits (nqd > 64 or
 *        nhd > MS_MD_BEST_MAX_HD; tested before the offset);
 *   out_total  int64 [ncand][2]: the sum of w over the path; 0 unless the status is 1;
 *   out_path   int32 [ncand][2][64]: path[i] for i < nqd when the status is 1; -1 everywhere else;
 *   out_cell   float32 [ncand][2][64]: M[i][path[i]], bit for bit; +0.0f everywhere else.
 * Descriptors are data, not trusted: no address outside scores [0, total_cells), the outputs and the workspace is formed.
 * Limits: nqd <= 64 as in ms_md_chain_scan; nhd <= MS_MD_BEST_MAX_HD.
 * workspace: ms_md_best_mappings_workspace_bytes(ncand, total_cells) bytes (0 for a negative argument; never 0 otherwise),
 * 16-byte aligned: kind 1's table D, one int64 per cell at the matrix's offset.  Every cell read was written by the same
 * call: a workspace serves the next call without clean-up.  (Matrices that overlap share their D cells: lay them out apart.)
 * ncand == 0 succeeds without a launch.  MS_ERR_ARG: NULL pointers, negative counts, a workspace that is not 16-byte
 * aligned; MS_ERR_WORKSPACE: a workspace below the size the function reports.
 * Asynchronous on `stream`, never allocates.  One wave per candidate; vector stores only, no atomics, no scratch memory.
 * Backward compatible additions: ms_version() stays 210. */
#define MS_MD_BEST_MAX_HD 1024
size_t ms_md_best_mappings_workspace_bytes(int ncand, int64_t total_cells);
int ms_md_best_mappings(const float *scores, int64_t total_cells, const int32_t *cand, int ncand, const int64_t *mat_off,
                        int32_t *out_status, int64_t *out_total, int32_t *out_path, float *out_cell, void *workspace,
                        size_t workspace_bytes, ms_stream_t stream);

/* ------------------------------------------------------------------ encoder --------- */

/* Floats in the canonical weight blob of the whole encoder (2 EGNN layers, state_dict order:
 * edge_mlp.0.{weight,bias}, edge_mlp.2.{weight,bias}, edge_gate.0.{weight,bias},
 * node_mlp.0.{weight,bias}, node_mlp.2.{weight,bias}; my_egnn_nocoords.py:18-34). */
size_t ms_egnn_weight_floats(void);
/* Bytes of the prepared (kernel-layout) weights produced by ms_egnn_prepare_weights. */
size_t ms_egnn_prepared_bytes(void);
/* Re-lay the canonical blob for the kernels (W1 split per node / distance column, W2 transposed
 * in K-chunks, ...).  weights, prepared: device.  Replaces network_setup's load_state_dict +
 * .to(device), dbsearch.py:35-45. */
int ms_egnn_prepare_weights(const float *weights, void *prepared, ms_stream_t stream);

/* Scratch bytes for embedding a ragged batch of nb structures with total_residues residues and
 * sum_sq = sum over structures of N^2. */
size_t ms_egnn_workspace_bytes(int nb, int64_t total_residues, int64_t sum_sq);

/* FoldClassNet.forward for a ragged batch (nndef_fold_egnn_embed.py:50-62 with
 * my_egnn_nocoords.py:44-74): node features = pe[:N] (the positional table is data,
 * float32 [pe_len,128]), 2 EGNN layers over all N^2 residue pairs, mean over residues.
 *   coords  float32 [total,3] CA coordinates, structures concatenated
 *   offsets int32 [nb+1] (device), offsets[b]..offsets[b+1] = residues of structure b
 *   offsets_host: the same array in host memory (used to size the launch; no device sync)
 *   out     float32 [nb,128]
 * Replaces network(x) at dbsearch.py:97-98, :299-301 and makedb.py:75-79 (there batch = 1). */
int ms_egnn_embed(const void *prepared, const float *pe, int pe_len, const float *coords, const int32_t *offsets,
                  const int32_t *offsets_host, int nb, float *out, void *workspace, size_t workspace_bytes,
                  ms_stream_t stream);
/* Diagnostics (tests; synchronises the device): the per-residue node features float32 [total,128] that the last ms_egnn_embed on
 * this workspace left behind, copied to the host -- layer 0: the output of the first EGNN layer, layer 1: of the second (what the
 * mean-pool reads).  nb, total (residues) and sum_sq (sum of N^2) must be those of that call: they fix where the blocks lie.
 * MS_ERR_ARG on NULL pointers, a layer other than 0 / 1, or counts no batch can have (nb < 1, total < nb, sum_sq outside
 * [total, total^2]).  Backward compatible addition: ms_version() stays 210. */
int ms_debug_egnn_node_features(const void *workspace, int nb, int64_t total, int64_t sum_sq, int layer, float *host_out);

/* ------------------------------------------------------------------ TM-align -------- */

/* Batched TM-align (Zhang & Skolnick, NAR 2005), the check the reference runs as one subprocess per hit
 * (utils.py:75-109) and per query-domain x target-domain pair of the multi-domain search (dbsearch_fulllength.py:55-92).
 * The routine sequence and constants of the public TMalign.cpp (the version is unpinned), fp64
 * geometry, one wave per pair.  Backward compatible additions: ms_version() stays 210. */
#define MS_TMALIGN_MAX_LEN 2000   /* longest chain accepted (createdb's parser cap) */
#define MS_TM_FAST 1              /* flags: TM-align -fast */
/* out_i[3*p + 2], the status of pair p */
#define MS_TM_OK 0
#define MS_TM_ERR_SHORT 1         /* a chain of <= 5 residues: TM-align refuses it */
#define MS_TM_ERR_LONG 2          /* a chain longer than max_len1 / max_len2 (or MS_TMALIGN_MAX_LEN) */
#define MS_TM_ERR_INDEX 3         /* a structure index outside [0, nstruct) */

/* Bytes of scratch for npairs pairs whose chain 1 has <= max_len1 and chain 2 <= max_len2 residues (0: bad argument).
 * Pairs share slots of the workspace when there are many long ones (at most 2 GiB of slots are asked for). */
size_t ms_tmalign_workspace_bytes(int max_len1, int max_len2, int npairs);
int ms_tmalign_max_len(void); /* MS_TMALIGN_MAX_LEN */

/* TM-align pair p: chain 1 = structure pairs[2p] (the query), chain 2 = structure pairs[2p+1].
 *   xyz      fp64 [total][3], the CA coordinates of nstruct structures packed back to back (the values TM-align would
 *            parse from the %8.3f PDB text: the caller rounds them to 3 decimals).  Every coordinate must be finite: the
 *            library does not check them, and NaN / inf give meaningless results;
 *   seq      uint8 [total], the one-letter residue codes (Seq_ID counts equal bytes);
 *   offsets  int64 [nstruct + 1], structure s = rows [offsets[s], offsets[s+1]);
 *   pairs    int32 [npairs][2]: worked on in the order given, one wave per pair -- give them longest first (L1 * L2);
 *   flags    MS_TM_FAST or 0;
 * Outputs: out_f fp64 [npairs][3] = TM-score normalised by chain 1, by chain 2, RMSD of the n_ali8 pairs;
 *          out_i int32 [npairs][3] = n_ali8 ("Aligned length": aligned pairs within score_d8), identical residues among
 *          them, status (MS_TM_*; values 0 unless MS_TM_OK);
 *          out_invmap int32 [npairs][max_len2] or NULL: the final alignment, chain-2 residue j -> chain-1 residue or -1;
 *          only entries j < the chain-2 length of pairs with status MS_TM_OK are written (fill it with -1 first).
 * All arrays are device memory; max_len1 / max_len2 bound every chain of the batch (longer ones get MS_TM_ERR_LONG). */
int ms_tmalign_batch(const double *xyz, const uint8_t *seq, const int64_t *offsets, int nstruct, const int32_t *pairs, int npairs,
                     int max_len1, int max_len2, int flags, void *workspace, size_t workspace_bytes, double *out_f, int32_t *out_i,
                     int32_t *out_invmap, ms_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MERIZO_SEARCH_AMD_H */
