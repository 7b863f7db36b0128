"""Helpers of the `cluster --complete` tests (TEST INFRASTRUCTURE): the restatements of ms_threshold_edges and
ms_cluster_greedy_edges, the oracle-engine hooks for the CPU runs of the driver, the garbage mix of extra entries, the second
planted database (lengths 50 / 100, where coverage rejects half of the pairs) and what the driver must report on both."""
import os

import numpy as np

import cluster_case as cc

NINF = np.float32(-np.inf)
MODES = ("ip_prenorm", "ip", "cosine")                                    # the engine's names of the three modes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ ms_threshold_edges, restated ----
def edge_set(src, dst, score):
    """{(src, dst, score bits)} of three arrays of one length."""
    return set(zip(np.asarray(src, np.int64).tolist(), np.asarray(dst, np.int64).tolist(), bits(score).tolist()))


def edges_of_lists(scores, idx, min_score, lo=None, hi=None):
    """Top-k lists of a search at k = n (rows idx are global; (-inf, -1) or NaN where the search has nothing) -> the set
    ms_threshold_edges must emit: every entry with a row, a score >= min_score (NaN fails) and a row outside [lo[q], hi[q])."""
    scores, idx = np.asarray(scores, np.float32), np.asarray(idx, np.int64)
    with np.errstate(invalid="ignore"):
        keep = (idx >= 0) & (scores >= np.float32(min_score))
    if lo is not None:
        lo, hi = np.asarray(lo, np.int64)[:, None], np.asarray(hi, np.int64)[:, None]
        keep &= ~((idx >= lo) & (idx < hi))
    qi, c = np.nonzero(keep)
    return edge_set(qi, idx[qi, c], scores[qi, c])


def oracle_edges(mode, rows, q, min_score, lo=None, hi=None, row_offset=0):
    """The oracle's search of `mode` (multidom_case.oracle_scores: its top-k at k = all rows, scattered back by row), filtered by
    >= min_score and the ranges -> (src, dst, score) arrays, by (src, dst)."""
    import multidom_case as mc
    s = mc.oracle_scores(mode, rows, q)
    with np.errstate(invalid="ignore"):
        keep = s >= np.float32(min_score)
    if lo is not None:
        g = row_offset + np.arange(s.shape[1], dtype=np.int64)[None, :]
        keep &= ~((g >= np.asarray(lo, np.int64)[:, None]) & (g < np.asarray(hi, np.int64)[:, None]))
    qi, r = np.nonzero(keep)
    return qi.astype(np.int64), (row_offset + r).astype(np.int64), s[qi, r].astype(np.float32)


# ------------------------------------------------------------------ ms_cluster_greedy_edges, restated ----
def cluster_greedy_edges_np(idx, score, src, dst, escore, lengths, min_score, mincov):
    """cluster_case.cluster_greedy_np on lists widened by the extra entries (an entry whose src is no row is dropped: it can name
    no list; the order inside a list does not matter).  'saturated' is that of the lists alone (0 without lists)."""
    lengths = np.asarray(lengths, np.int32)
    n = lengths.shape[0]
    if idx is None:
        idx, score = np.empty((n, 0), np.int64), np.empty((n, 0), np.float32)
    src, dst, escore = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(escore, np.float32)
    ok = (src >= 0) & (src < n)
    src, dst, escore = src[ok], dst[ok], escore[ok]
    order = np.argsort(src, kind="stable")
    src, dst, escore = src[order], dst[order], escore[order]
    per_row = np.bincount(src, minlength=n)
    width = int(per_row.max()) if src.size else 0
    w_idx, w_score = cc.empty_lists(n, idx.shape[1] + max(width, 1))
    w_idx[:, :idx.shape[1]], w_score[:, :idx.shape[1]] = idx, score
    col = idx.shape[1] + np.arange(src.size) - np.repeat(np.cumsum(per_row) - per_row, per_row)
    w_idx[src, col], w_score[src, col] = dst, escore
    rep, rep_score, info = cc.cluster_greedy_np(w_idx, w_score, lengths, min_score, mincov)
    saturated = cc.cluster_greedy_np(idx, score, lengths, min_score, mincov)[2]["saturated"] if idx.shape[1] else 0
    return rep, rep_score, {"n_reps": info["n_reps"], "saturated": saturated}


def random_extras(n, m, idx, score, seed):
    """m extra directed entries with cluster_case.random_lists' garbage mix: src and dst out of range (just past the end, far beyond
    2^32) and negative, self-loops, NaN and -inf scores, and duplicates of list entries with another score."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=m, dtype=np.int64)
    dst = rng.integers(0, n, size=m, dtype=np.int64)
    sc = rng.choice(cc.SCORE_VALUES, size=m).astype(np.float32)
    kind = rng.integers(0, 24, size=m)
    dst = np.where(kind == 0, src, dst)                                    # self-loops
    dst = np.where(kind == 1, n + rng.integers(0, 3, size=m), dst)
    dst = np.where(kind == 2, (1 << 40) + src, dst)
    dst = np.where(kind == 3, -2 - src, dst)
    sc = np.where(kind == 4, np.float32(np.nan), sc)
    sc = np.where(kind == 5, NINF, sc)
    src = np.where(kind == 6, n + rng.integers(0, 3, size=m), src)         # a src that is no row: never dereferenced
    src = np.where(kind == 7, (1 << 40) + dst, src)
    src = np.where(kind == 8, -1 - rng.integers(0, n, size=m), src)
    dup = np.nonzero(kind == 9)[0]                                         # a list entry again, with another score
    if idx.shape[1]:
        r, c = rng.integers(0, n, size=dup.size), rng.integers(0, idx.shape[1], size=dup.size)
        src[dup], dst[dup] = r, idx[r, c]
        sc[dup] = np.float32(0.9)
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), np.ascontiguousarray(sc.astype(np.float32))


# ------------------------------------------------------------------ the oracle engine ----
def install_oracle_complete():
    """cluster_case.install_oracle_cluster plus OracleEngine.threshold_edges (the oracle's search in the same mode at k = n,
    filtered) and OracleEngine.cluster_greedy_edges (cluster_greedy_edges_np): the CPU runs of `cluster --complete`."""
    import torch
    Engine = cc.install_oracle_cluster()

    def threshold_edges(self, db, q, mode, min_score, lo=None, hi=None, row_offset=0, row_norm_bound=None, out=None, stats=None):
        src, dst, score = oracle_edges(mode, db.numpy(), q.numpy(), min_score, None if lo is None else lo.numpy(),
                                       None if hi is None else hi.numpy(), int(row_offset))
        count = int(src.shape[0])
        if stats is not None:
            stats["rescored"] = count
        got = (torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(score))
        if out is None:
            return got + (count,)
        kept = min(count, int(out[0].numel()))                             # (the cap rule: count is exact, the rest is not written)
        for o, g in zip(out, got):
            o[:kept] = g[:kept]
        return out[0][:kept], out[1][:kept], out[2][:kept], count

    def cluster_greedy_edges(self, nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score, mincov=0.0):
        none = np.empty(0, np.int64)
        rep, score, info = cluster_greedy_edges_np(
            None if nbr_idx is None else nbr_idx.numpy(), None if nbr_score is None else nbr_score.numpy(),
            none if edge_src is None else edge_src.numpy(), none if edge_dst is None else edge_dst.numpy(),
            np.empty(0, np.float32) if edge_score is None else edge_score.numpy(), np.asarray(lengths), min_score, mincov)
        return torch.from_numpy(rep), torch.from_numpy(score), dict(info, rounds=0)

    Engine.threshold_edges = threshold_edges
    Engine.cluster_greedy_edges = cluster_greedy_edges
    return Engine


# ------------------------------------------------------------------ the two planted databases ----
SPLIT_MINCOV = 0.7


def split_lengths(n=500):
    """Lengths from {50, 100}: 50 / 100 fails coverage 0.7, so about half of the pairs above the cosine threshold are no edges."""
    return np.where(np.random.default_rng(0).random(n) < 0.5, 50, 100).astype(np.int32)


def write_split(work, n=500, seed=3):
    """cluster_case.planted_rows' rows with split_lengths as a database in both layouts under `work` ('fa2', 'pt2').
    -> (names, lengths, family)."""
    from merizo_search_amd.foldclass import dbutil, synthetic as syn
    os.makedirs(work, exist_ok=True)
    rows, _lengths, family = cc.planted_rows(n, seed)
    lengths = split_lengths(n)
    rng = np.random.default_rng(seed + 1)
    names = ["fam%03d_r%04d" % (family[r], r) for r in range(n)]
    seqs = ["".join(rng.choice(list("ACDEFGHIKL"), size=int(l))) for l in lengths]
    coords = [syn.random_walk(int(l), seed * 7919 + r) for r, l in enumerate(lengths)]
    dbutil.write_faiss_db(os.path.join(work, "fa2"), rows, names, seqs, coords)
    raw = (rows * rng.uniform(0.5, 4.0, size=(n, 1))).astype(np.float32)
    dbutil.write_pt_db(os.path.join(work, "pt2"), raw, ["/x/" + nm + ".pdb" for nm in names], coords, seqs)
    return names, lengths, family


def expected_counts(lengths, family, k, mincov, n=500, seed=3):
    """What the driver must report at -k `k` on planted rows with these lengths: the margins cluster_case.planted_rows asserts make
    a row's neighbours at the threshold exactly the other members of its family, whichever search path scored them.
    -> dict(full_lists, edges, saturated): rows with >= k neighbours; the directed entries the edge pass finds for them (ALL
    their neighbours); rows whose k best neighbours all pass coverage -- from the restatement on the oracle's own lists."""
    from oracle import oracle as orc
    rows, _l, fam = cc.planted_rows(n, seed)
    assert np.array_equal(fam, family)
    s, i = orc.ip_topk(rows, rows, k + 1, order=1)
    idx, score = cc.empty_lists(n, k)
    for r in range(n):
        keep = [(float(sv), int(iv)) for sv, iv in zip(s[r], i[r]) if iv != r and sv >= np.float32(cc.PLANTED_MINCOS)][:k]
        for c, (sv, iv) in enumerate(keep):
            idx[r, c], score[r, c] = iv, sv
    size = np.bincount(family)[family]
    full = size - 1 >= k
    assert np.array_equal((idx >= 0).sum(axis=1) == k, full)
    saturated = cc.cluster_greedy_np(idx, score, lengths, cc.PLANTED_MINCOS, mincov)[2]["saturated"]
    return {"full_lists": int(full.sum()), "edges": int((size - 1)[full].sum()), "saturated": int(saturated)}
