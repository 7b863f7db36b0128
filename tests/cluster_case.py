"""Helpers of the cluster tests (TEST INFRASTRUCTURE): the sequential numpy restatement of ms_cluster_greedy -- the
definition the kernels are compared with, bit for bit -- an oracle-engine hook for the CPU runs of the driver, hand-built
and random neighbour lists, and a small database of planted families in both layouts."""
import os

import numpy as np

NINF = np.float32(-np.inf)


def cluster_greedy_np(nbr_idx, nbr_score, lengths, min_score, mincov):
    """include/merizo_search_amd.h, ms_cluster_greedy, restated SEQUENTIALLY (no rounds, no flags): the undirected weighted
    adjacency from the valid directed entries, one visit per row in priority order (a row is a representative unless a
    neighbour visited before it is one), assignment afterwards.  -> (rep int64 [n], rep_score float32 [n], info) with
    info = {'n_reps', 'saturated'}."""
    idx, score = np.asarray(nbr_idx, np.int64), np.asarray(nbr_score, np.float32)
    L = np.asarray(lengths, np.int32)
    n, k = idx.shape
    assert score.shape == (n, k) and L.shape == (n,)
    rows = np.arange(n, dtype=np.int64)[:, None]
    inside = (idx >= 0) & (idx < n) & (idx != rows)
    j = np.where(inside, idx, 0)                                           # (rows outside [0, n) are never looked up)
    l_min = np.minimum(L[:, None], L[j]).astype(np.float32)
    l_max = np.maximum(L[:, None], L[j]).astype(np.float32)
    covers = l_min >= np.float32(mincov) * l_max                           # fp32 product, this operand order
    with np.errstate(invalid="ignore"):
        valid = inside & covers & (score >= np.float32(min_score))         # (NaN compares false)
    adj = [dict() for _ in range(n)]
    for i, c in zip(*np.nonzero(valid)):
        i, t = int(i), int(idx[i, c])
        w = score[i, c] + np.float32(0.0)                                  # -0.0 counts as +0.0
        for a, b in ((i, t), (t, i)):
            if b not in adj[a] or w > adj[a][b]:
                adj[a][b] = w                                              # the larger of the directed scores
    is_rep = np.zeros(n, bool)
    for r in sorted(range(n), key=lambda r: (-int(L[r]), r)):              # the longer domain first, the smaller row on a tie
        is_rep[r] = not any(is_rep[x] for x in adj[r])
    rep = np.arange(n, dtype=np.int64)
    rep_score = np.ones(n, np.float32)
    for r in np.nonzero(~is_rep)[0]:
        w, neg = max((w, -x) for x, w in adj[r].items() if is_rep[x])      # largest weight, the smaller row on a tie
        rep[r], rep_score[r] = -neg, w
    return rep, rep_score, {"n_reps": int(is_rep.sum()), "saturated": int(valid.all(axis=1).sum())}


def install_oracle_cluster():
    """OracleEngine.topk_drop_ranges (with the `out=` the cluster driver uses) and OracleEngine.cluster_greedy = the numpy
    restatements (the CPU runs of the driver)."""
    import torch
    import dbquery_case as dq
    from oracle_engine import OracleEngine

    def topk_drop_ranges(self, scores, idx, lo, hi, kout, min_score=float("-inf"), out=None):
        got = [torch.from_numpy(a) for a in dq.drop_ranges_np(scores.numpy(), idx.numpy(), np.asarray(lo), np.asarray(hi), min_score, kout)]
        if out is None:
            return tuple(got)
        for dst, src in zip(out, got):
            assert dst.shape == src.shape and dst.dtype == src.dtype
            dst.copy_(src)
        return out

    def cluster_greedy(self, nbr_idx, nbr_score, lengths, min_score, mincov=0.0):
        rep, score, info = cluster_greedy_np(nbr_idx.numpy(), nbr_score.numpy(), np.asarray(lengths), min_score, mincov)
        return torch.from_numpy(rep), torch.from_numpy(score), dict(info, rounds=0)

    OracleEngine.topk_drop_ranges = topk_drop_ranges
    OracleEngine.cluster_greedy = cluster_greedy
    return OracleEngine


def empty_lists(n, k):
    """[n,k] lists of padding: (-1, -inf)."""
    return np.full((n, k), -1, np.int64), np.full((n, k), NINF, np.float32)


def lists_from_edges(n, k, edges):
    """Directed entries (i, j, s) appended to row i's list in the order given."""
    idx, score = empty_lists(n, k)
    fill = np.zeros(n, np.int64)
    for i, j, s in edges:
        idx[i, fill[i]], score[i, fill[i]] = j, s
        fill[i] += 1
    return idx, score


LENGTH_VALUES = np.array([40, 70, 71, 100, 130], np.int32)                # five values: many priority ties; 70 / 100 sits on mincov 0.7
CUT = np.float32(0.6)                                                     # the tests' min_score; one ulp below it is a value too
SCORE_VALUES = np.array([0.5, np.nextafter(CUT, np.float32(0.0)), CUT, CUT, 0.75, 0.75, 0.9, -0.0, 0.0], np.float32)


def random_lists(n, k, seed):
    """Random lists with many ties in priority and weight, and with everything a list may hold that is not an edge: padding,
    self-loops, duplicate rows, rows >= n (just past the end and far beyond 2^32), negative rows, NaN and -inf scores.
    -> (idx, score, lengths); meant for min_score 0.6, mincov 0.7."""
    rng = np.random.default_rng(seed)
    lengths = rng.choice(LENGTH_VALUES, size=n)
    idx = rng.integers(0, n, size=(n, k), dtype=np.int64)
    score = rng.choice(SCORE_VALUES, size=(n, k))
    kind = rng.integers(0, 20, size=(n, k))
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], (n, k))
    idx = np.where(kind == 0, rows, idx)                                   # self-loops
    idx = np.where(kind == 1, n + rng.integers(0, 3, size=(n, k)), idx)    # just past the end
    idx = np.where(kind == 2, (1 << 40) + rows, idx)                       # far past it (the low 32 bits name a real row)
    idx = np.where(kind == 3, -2 - rows, idx)                              # negative, not the padding value
    score = np.where(kind == 4, np.float32(np.nan), score)
    pad = kind == 5
    idx, score = np.where(pad, -1, idx), np.where(pad, NINF, score)
    if k > 1:
        idx[:, 1] = np.where(kind[:, 1] == 6, idx[:, 0], idx[:, 1])        # duplicate rows, with another score
    if n > 2:
        full = rng.random(n) < 0.1                                         # some rows whose k entries are all edges ('saturated')
        for r in np.nonzero(full)[0]:
            same = np.nonzero((lengths == lengths[r]) & (np.arange(n) != r))[0]
            if same.size:
                idx[r], score[r] = rng.choice(same, size=k), np.float32(0.75)
    return np.ascontiguousarray(idx), np.ascontiguousarray(score.astype(np.float32)), lengths.astype(np.int32)


def family_lists(n, k, seed):
    """Planted families as neighbour lists: rows in random order, families of 2..12 and singletons; a row lists the other members
    of its family (the best k when there are more) with a pair score that differs by one ulp between the two directions for
    some pairs.  -> (idx, score, lengths, family of each row)."""
    rng = np.random.default_rng(seed)
    family, f = np.empty(n, np.int64), 0
    r = 0
    while r < n:
        size = min(int(rng.choice([1, 1, 2, 3, 5, 8, 12])), n - r)
        family[r:r + size] = f
        r, f = r + size, f + 1
    family = family[rng.permutation(n)]
    lengths = (60 + 10 * (family % 7) + rng.integers(0, 4, size=n)).astype(np.int32)     # ties inside families; coverage >= 0.9
    idx, score = empty_lists(n, k)
    order = np.argsort(family, kind="stable")
    bounds = np.nonzero(np.diff(family[order], prepend=-1, append=f))[0]
    for a, b in zip(bounds[:-1], bounds[1:]):
        members = order[a:b]
        for i in members:
            others = members[members != i]
            s = (0.7 + 0.05 * ((i * others + i + others) % 5)).astype(np.float32)        # symmetric in (i, other), few values
            s = np.where((i < others) & ((i + others) % 3 == 0), np.nextafter(s, np.float32(2.0)), s).astype(np.float32)
            keep = np.lexsort((others, -s))[:k]
            idx[i, :keep.size], score[i, :keep.size] = others[keep], s[keep]
    return idx, score, lengths, family


# ------------------------------------------------------------------ a database of planted families ----
PLANTED_MINCOS = 0.7
PLANTED_SIGMA = 0.3


def planted_rows(n=500, seed=3):
    """Unit rows of planted families: members are normalize(c + sigma * g / sqrt(128)) around a random unit centre c, families of
    2..12 members and singletons, rows shuffled; lengths such that coverage 0.7 holds inside families, with ties.
    ASSERTS the margin the tests rely on, on the CPU oracle's own scores: every intra-family cosine clears PLANTED_MINCOS by
    0.02, every inter-family cosine misses it by 0.02 (rounding differences between search paths are ~1e-7).
    -> (rows float32 [n,128], lengths int32 [n], family int64 [n])."""
    from oracle import oracle as orc
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.choice([1, 1, 1, 2, 3, 4, 6, 9, 12])), n - sum(sizes)))
    family = np.repeat(np.arange(len(sizes)), sizes)
    centres = rng.standard_normal((len(sizes), 128))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows = centres[family] + PLANTED_SIGMA * rng.standard_normal((n, 128)) / np.sqrt(128.0)
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    lengths = (50 + 20 * (family % 5) + rng.integers(0, 5, size=n)).astype(np.int32)     # inside a family: >= 50 / 54 > 0.7
    perm = rng.permutation(n)
    rows, lengths, family = np.ascontiguousarray(rows[perm]), lengths[perm], family[perm]
    s, i = orc.ip_topk(rows, rows, n, order=1)                             # every cosine, as the oracle computes it
    cos = np.empty((n, n), np.float32)
    np.put_along_axis(cos, i, s, axis=1)
    same = family[:, None] == family[None, :]
    off = ~np.eye(n, dtype=bool)
    intra, inter = cos[same & off], cos[~same]
    assert intra.size and intra.min() >= PLANTED_MINCOS + 0.02, ("planted families: intra-family cosine too low", float(intra.min()))
    assert inter.max() <= PLANTED_MINCOS - 0.02, ("planted families: inter-family cosine too high", float(inter.max()))
    assert max(sizes) == 12 and min(sizes) == 1
    return rows, lengths, family


def write_planted(work, n=500, seed=3):
    """The planted families as a database in BOTH layouts under `work` ('fa', 'pt'; the `.pt` rows are the unit rows scaled
    per row, so its cosine path has something to normalise).  -> (names, lengths, family)."""
    from merizo_search_amd.foldclass import dbutil, synthetic as syn
    os.makedirs(work, exist_ok=True)
    rows, lengths, family = planted_rows(n, seed)
    rng = np.random.default_rng(seed + 1)
    names = ["fam%03d_r%04d" % (family[r], r) for r in range(n)]
    seqs = ["".join(rng.choice(list("ACDEFGHIKL"), size=int(l))) for l in lengths]
    coords = [syn.random_walk(int(l), seed * 7919 + r) for r, l in enumerate(lengths)]
    dbutil.write_faiss_db(os.path.join(work, "fa"), rows, names, seqs, coords)
    raw = (rows * rng.uniform(0.5, 4.0, size=(n, 1))).astype(np.float32)
    dbutil.write_pt_db(os.path.join(work, "pt"), raw, ["/x/" + nm + ".pdb" for nm in names], coords, seqs)
    return names, lengths, family


def planted_clusters(lengths, family):
    """rep int64 [n] the planted families must come back as: the longest member, the smaller row on a tie."""
    n = len(family)
    rep = np.empty(n, np.int64)
    for f in np.unique(family):
        members = np.nonzero(family == f)[0]
        rep[members] = min(members, key=lambda r: (-int(lengths[r]), r))
    return rep


def read_tsv(path):
    with open(path) as handle:
        return [line.rstrip("\n").split("\t") for line in handle]
