"""Helpers of the db-search tests (TEST INFRASTRUCTURE): the numpy restatement of ms_topk_drop_ranges -- the definition the
kernel is compared with, bit for bit -- an oracle-engine hook for the CPU runs, and small databases in both layouts."""
import os

import numpy as np


def drop_ranges_np(scores, idx, lo, hi, min_score, kout):
    """include/merizo_search_amd.h, ms_topk_drop_ranges, entry by entry: from each sorted list drop the padding (row < 0), the
    rows in [lo[q], hi[q]) and the scores below min_score; the first kout of what remains in its order, (-inf, -1) behind;
    count = real entries written.  -> (float32 [nq,kout], int64 [nq,kout], int32 [nq])."""
    scores, idx = np.asarray(scores, np.float32), np.asarray(idx, np.int64)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    nq, kin = scores.shape
    assert idx.shape == (nq, kin) and lo.shape == (nq,) and hi.shape == (nq,) and 1 <= kout <= kin
    out_s = np.full((nq, kout), -np.inf, np.float32)
    out_i = np.full((nq, kout), -1, np.int64)
    count = np.zeros(nq, np.int32)
    cut = np.float32(min_score)
    for q in range(nq):
        w = 0
        for j in range(kin):
            r, s = idx[q, j], scores[q, j]
            if r < 0 or lo[q] <= r < hi[q] or s < cut:
                continue
            if w < kout:
                out_s[q, w], out_i[q, w] = s, r
                w += 1
        count[q] = w
    return out_s, out_i, count


def install_oracle_drop():
    """OracleEngine.topk_drop_ranges = the numpy restatement (the CPU runs of the driver)."""
    import torch
    from oracle_engine import OracleEngine

    def topk_drop_ranges(self, scores, idx, lo, hi, kout, min_score=float("-inf")):
        s, i, c = drop_ranges_np(scores.numpy(), idx.numpy(), np.asarray(lo), np.asarray(hi), min_score, kout)
        return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(c)

    OracleEngine.topk_drop_ranges = topk_drop_ranges
    return OracleEngine


def chain_names(n, seed, max_run=7):
    """n domain names forming chains of 1..max_run adjacent domains ('c00012_TED03'-style: multidomain.domid2chainid gives
    'c00012') -> (names, first row of each row's chain, one past its last row)."""
    rng = np.random.default_rng(seed)
    names, first, last = [], np.empty(n, np.int64), np.empty(n, np.int64)
    row = chain = 0
    while row < n:
        run = min(int(rng.integers(1, max_run + 1)), n - row)
        for d in range(run):
            names.append("c%05d_TED%02d" % (chain, d + 1))
        first[row:row + run], last[row:row + run] = row, row + run
        row += run
        chain += 1
    return names, first, last


def write_case(work, n=600, seed=5, dup=True):
    """A database of n rows in BOTH layouts under `work` ('fa': faiss layout with metadata, 'pt': the `.pt` layout) whose names
    form multi-domain chains; the faiss rows are the normalised `.pt` rows.  With exact duplicates across the 2-rank shard
    boundary (ties resolve to the lower row).  -> (names, first, last)."""
    from merizo_search_amd.foldclass import dbutil, synthetic as syn
    os.makedirs(work, exist_ok=True)
    raw, lengths = syn.raw_database(n, seed=seed)
    lengths = np.clip(lengths, 20, 60)
    if dup and n > 40:
        raw[5] = raw[n - 3]
        raw[n // 2 - 1] = raw[n // 2 + 4]
        raw[7] = raw[8]
    names, first, last = chain_names(n, seed + 1)
    rng = np.random.default_rng(seed + 2)
    seqs = ["".join(rng.choice(list("ACDEFGHIKL"), size=int(l))) for l in lengths]
    coords = [syn.random_walk(int(l), seed * 7919 + i) for i, l in enumerate(lengths)]
    norm = (raw / np.linalg.norm(raw, axis=1, keepdims=True)).astype(np.float32)
    dbutil.write_faiss_db(os.path.join(work, "fa"), norm, names, seqs, coords, metadata=['{ "row": %d }' % i for i in range(n)])
    dbutil.write_pt_db(os.path.join(work, "pt"), raw, ["/x/" + nm + ".pdb" for nm in names], coords, seqs)
    return names, first, last


def read_tsv(path):
    with open(path) as handle:
        return [line.rstrip("\n").split("\t") for line in handle]
