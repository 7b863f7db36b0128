"""Helpers of the `cluster --mintm` tests (TEST INFRASTRUCTURE): the sequential restatements of ms_cluster_pairs,
ms_cluster_pairs_apply and ms_cluster_pairs_find -- the definition the kernels are compared with -- their oracle-engine hooks and
an aligner backed by the CPU restatement of TM-align for the CPU runs of the driver, the whole `--mintm` pipeline in numpy, and a
database of planted STRUCTURE families in both layouts: embedding families whose members superpose, impostors whose embedding
belongs to a family and whose coordinates do not, and one embedding family that is really two structure families."""
import os

import numpy as np

import cluster_case as cc
import cluster_components_case as cpc

NINF = np.float32(-np.inf)


# ------------------------------------------------------------------ the three calls, restated ----
def _entries(idx, score, src, dst, escore, n):
    """Lists ([n,k] or None) and extras ([m] or None) as one run of directed entries (i, j, s): the lists row by row, then the extras."""
    if idx is None:
        idx, score = np.empty((n, 0), np.int64), np.empty((n, 0), np.float32)
    idx, score = np.asarray(idx, np.int64), np.asarray(score, np.float32)
    k = idx.shape[1]
    none = src is None
    src = np.empty(0, np.int64) if none else np.asarray(src, np.int64)
    dst = np.empty(0, np.int64) if none else np.asarray(dst, np.int64)
    escore = np.empty(0, np.float32) if none else np.asarray(escore, np.float32)
    i = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), k), src])
    return i, np.concatenate([idx.ravel(), dst]), np.concatenate([score.ravel(), escore]), k


def canonical(i, j, lengths):
    """(a, b) of the rows i, j: a the higher-priority one -- the longer domain, the smaller row on equal length."""
    i, j = int(i), int(j)
    return (i, j) if (-int(lengths[i]), i) < (-int(lengths[j]), j) else (j, i)


def cluster_pairs_np(idx, score, src, dst, escore, lengths, min_score, mincov):
    """include/merizo_search_amd.h, ms_cluster_pairs, restated SEQUENTIALLY on cluster_components_case.valid_entries: the canonical
    pairs of the valid entries in the order of their first appearance.  -> (pairs int32 [count,2], saturated)."""
    L = np.asarray(lengths, np.int32)
    n = L.shape[0]
    i, j, s, k = _entries(idx, score, src, dst, escore, n)
    valid = cpc.valid_entries(i, j, s, L, min_score, mincov)
    saturated = int(valid[:n * k].reshape(n, k).all(axis=1).sum()) if k else 0
    seen = {}
    for a, b in zip(i[valid].tolist(), j[valid].tolist()):
        seen.setdefault(canonical(a, b, L), len(seen))
    return np.asarray(list(seen), np.int32).reshape(-1, 2), saturated


def pairs_apply_np(idx, score, src, dst, escore, lengths, min_score, mincov, pairs, keep):
    """ms_cluster_pairs_apply restated: pairs [slots,2] is the set (slot = position), keep uint8 [count].  Every valid entry whose
    pair has no slot below min(slots, count) or has keep 0 there becomes padding; everything else keeps its bits.
    -> (idx, score, dst, escore, removed): edited copies (None where the input was None)."""
    L = np.asarray(lengths, np.int32)
    n = L.shape[0]
    i, j, s, k = _entries(idx, score, src, dst, escore, n)
    valid = cpc.valid_entries(i, j, s, L, min_score, mincov)
    slot_of = {(int(a), int(b)): t for t, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist())}
    keep = np.asarray(keep, np.uint8)
    gone = np.zeros(i.shape[0], bool)
    for e in np.nonzero(valid)[0]:
        t = slot_of.get(canonical(i[e], j[e], L), -1)
        gone[e] = t < 0 or t >= keep.shape[0] or keep[t] == 0
    j, s = j.copy(), s.copy()
    j[gone], s[gone] = -1, NINF
    cut = n * k
    return (None if idx is None else j[:cut].reshape(n, k), None if idx is None else s[:cut].reshape(n, k),
            None if src is None else j[cut:], None if src is None else s[cut:], int(gone.sum()))


def pairs_find_np(a, b, lengths, pairs):
    """ms_cluster_pairs_find restated -> slot int64 [cnt] (-1: not in the set, a row outside [0, n), a == b)."""
    L = np.asarray(lengths, np.int32)
    n = L.shape[0]
    slot_of = {(int(x), int(y)): t for t, (x, y) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist())}
    out = np.full(len(a), -1, np.int64)
    for e, (x, y) in enumerate(zip(np.asarray(a, np.int64).tolist(), np.asarray(b, np.int64).tolist())):
        if 0 <= x < n and 0 <= y < n and x != y:
            out[e] = slot_of.get(canonical(x, y, L), -1)
    return out


# ------------------------------------------------------------------ TM-align on the CPU restatement ----
_tm_memo = {}


def tm_pair(x, y, sx, sy, fast):
    """tmalign_ref.tm_align (order=kernel: the kernel's own order of operations) of chain 1 = x, chain 2 = y, coordinates as given
    -> (qtm, ttm, rmsd, n_ali8, n_identical), or None for a chain of <= 5 residues.  Memoised: the runs of one test module align
    the same few hundred pairs again and again."""
    import tmalign_ref as R
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    key = (x.tobytes(), y.tobytes(), str(sx), str(sy), bool(fast))
    if key not in _tm_memo:
        try:
            r = R.tm_align(x, y, sx, sy, fast=fast, order="kernel", quantize=False)
            _tm_memo[key] = (r["qtm"], r["ttm"], r["rmsd"], r["n_ali8"], r["n_identical"])
        except ValueError:
            _tm_memo[key] = None
    return _tm_memo[key]


def tmalign_batch_ref(coords_list, seqs, pairs, fast=False):
    """ops.tmalign_batch's dict from the CPU restatement (status 1 = TM_ERR_SHORT where it refuses)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = {"qtm": np.zeros(len(pairs)), "ttm": np.zeros(len(pairs)), "rmsd": np.zeros(len(pairs)), "n_ali8": np.zeros(len(pairs), np.int32),
           "n_identical": np.zeros(len(pairs), np.int32), "status": np.zeros(len(pairs), np.int32)}
    for p, (a, b) in enumerate(pairs.tolist()):
        assert np.isfinite(coords_list[a]).all() and np.isfinite(coords_list[b]).all(), "the driver filters non-finite chains"
        r = tm_pair(coords_list[a], coords_list[b], seqs[a], seqs[b], fast)
        if r is None:
            out["status"][p] = 1
        else:
            out["qtm"][p], out["ttm"][p], out["rmsd"][p], out["n_ali8"][p], out["n_identical"][p] = r
    return out


def printed_max_tm(coords_a, seq_a, coords_b, seq_b, fast):
    """What the driver compares with --mintm for chain 1 = a, chain 2 = b (stored float32 coordinates): max(qtm, ttm) of the
    5-decimal values; None where TM-align refuses the pair or a coordinate is not finite."""
    from merizo_search_amd.foldclass import tmalign
    for c in (coords_a, coords_b):
        if len(c) <= 5 or not np.isfinite(np.asarray(c, np.float32)).all():
            return None
    r = tm_pair(tmalign.pdb_values(coords_a), tmalign.pdb_values(coords_b), seq_a, seq_b, fast)
    if r is None:
        return None
    v = tmalign.printed_values(*r)
    return max(v["qtm"], v["ttm"])


# ------------------------------------------------------------------ the oracle engine ----
class _PairSet:
    """What the oracle engine keeps where the library keeps its workspace: the pairs by slot."""

    def __init__(self, pairs):
        self.pairs = pairs


def install_oracle_cluster_tm():
    """cluster_components_case.install_oracle_components plus OracleEngine.cluster_pairs / cluster_pairs_apply / cluster_pairs_find
    (the restatements above; apply edits the driver's tensors in place, as the library does) and OracleEngine.tmalign_batch
    (tmalign_batch_ref): the CPU runs of `cluster --mintm`."""
    import torch
    Engine = cpc.install_oracle_components()
    host = lambda t: None if t is None else t.numpy()

    def cluster_pairs(self, nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score, mincov=0.0, cap=None):
        pairs, saturated = cluster_pairs_np(host(nbr_idx), host(nbr_score), host(edge_src), host(edge_dst), host(edge_score),
                                            np.asarray(lengths), min_score, mincov)
        assert cap is None
        return torch.from_numpy(pairs), torch.tensor([pairs.shape[0], saturated], dtype=torch.int64), _PairSet(pairs)

    def cluster_pairs_apply(self, nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score, mincov, keep, workspace):
        idx, score, dst, escore, removed = pairs_apply_np(host(nbr_idx), host(nbr_score), host(edge_src), host(edge_dst), host(edge_score),
                                                          np.asarray(lengths), min_score, mincov, workspace.pairs, keep.numpy())
        for t, new in ((nbr_idx, idx), (nbr_score, score), (edge_dst, dst), (edge_score, escore)):
            if t is not None:
                t.copy_(torch.from_numpy(np.ascontiguousarray(new)))
        return torch.tensor([removed], dtype=torch.int64)

    def cluster_pairs_find(self, a, b, lengths, workspace):
        return torch.from_numpy(pairs_find_np(np.asarray(a), np.asarray(b), np.asarray(lengths), workspace.pairs))

    def tmalign_batch(self, coords_list, seqs, pairs, fast=False):
        return tmalign_batch_ref(coords_list, seqs, pairs, fast)

    Engine.cluster_pairs = cluster_pairs
    Engine.cluster_pairs_apply = cluster_pairs_apply
    Engine.cluster_pairs_find = cluster_pairs_find
    Engine.tmalign_batch = tmalign_batch
    return Engine


# ------------------------------------------------------------------ a database of planted structure families ----
MINCOS, MINCOV, MINTM = cc.PLANTED_MINCOS, 0.7, 0.5
TM_SAME, TM_OTHER = 0.55, 0.45                                            # the margins write_structured asserts around MINTM
FAMILY_SIZES = (4, 5, 6) * 6                                              # 18 plain families: embedding family = structure family
DOUBLE = 4                                                                # one embedding family of 2 x DOUBLE rows: two structure families
IMPOSTORS = 4                                                             # embedding of families 0..3, coordinates of a fresh walk;
LONGEST_IMPOSTORS = 2                                                     # the first two are the longest row of their embedding family
K_ALL = 8                                                                 # an embedding family has at most 8 rows: -k 8 holds every neighbour
NOISE, SEED = 0.6, 17


def _member(base, rng, seed):
    """A rigidly moved copy of `base` with NOISE A of noise and up to L/12 residues trimmed per end."""
    import tm_case
    L = len(base)
    t1, t2 = (int(t) for t in rng.integers(0, L // 12 + 1, size=2))
    return tm_case.rigid(tm_case.noisy(base[t1:L - t2], NOISE, seed), seed + 1).astype(np.float32)


def structured_rows(seed=SEED):
    """-> (rows float32 [n,128], coords list of float32 [L,3], seqs, efam int64 [n], sfam int64 [n]): efam the embedding family
    (planted as cluster_case.planted_rows plants them), sfam the STRUCTURE family (-1 - t for impostor t: a family of its own), rows
    shuffled.  ASSERTS on the CPU oracle's scores that every intra-efam cosine clears MINCOS by 0.02 and every other misses it by
    0.02, and that coverage >= 5/6 holds inside a structure family and >= 3/4 inside an embedding family."""
    import tm_case
    from oracle import oracle as orc
    rng = np.random.default_rng(seed)
    coords, efam, sfam = [], [], []
    bases = []
    for f, size in enumerate(FAMILY_SIZES + (DOUBLE, DOUBLE)):
        if f == len(FAMILY_SIZES) + 1:                                     # the double family's second structure: a length coverage keeps
            L = len(bases[-1]) + int(rng.integers(-2, 3))
        else:
            L = int(rng.integers(44, 80))
        base = tm_case.walk(L, seed * 1000 + f)
        bases.append(base)
        for t in range(size):
            coords.append(_member(base, rng, seed * 100000 + 100 * f + 2 * t))
            efam.append(min(f, len(FAMILY_SIZES)))
            sfam.append(f)
    for t in range(IMPOSTORS):
        members = [len(c) for c, e in zip(coords, efam) if e == t]
        L = max(members) + 1 + t if t < LONGEST_IMPOSTORS else int(rng.integers(min(members), max(members) + 1))
        coords.append(tm_case.walk(L, seed * 1000 + 500 + t).astype(np.float32))
        efam.append(t)
        sfam.append(-1 - t)
    efam, sfam = np.asarray(efam, np.int64), np.asarray(sfam, np.int64)
    n = efam.shape[0]
    centres = rng.standard_normal((int(efam.max()) + 1, 128))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows = centres[efam] + cc.PLANTED_SIGMA * rng.standard_normal((n, 128)) / np.sqrt(128.0)
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    perm = rng.permutation(n)
    rows, efam, sfam, coords = np.ascontiguousarray(rows[perm]), efam[perm], sfam[perm], [coords[p] for p in perm]
    seqs = [tm_case.seq_of(len(c), seed * 31 + r) for r, c in enumerate(coords)]
    lengths = np.asarray([len(c) for c in coords], np.int32)
    s, i = orc.ip_topk(rows, rows, n, order=1)
    cos = np.empty((n, n), np.float32)
    np.put_along_axis(cos, i, s, axis=1)
    same, off = efam[:, None] == efam[None, :], ~np.eye(n, dtype=bool)
    assert cos[same & off].min() >= MINCOS + 0.02 and cos[~same].max() <= MINCOS - 0.02
    lo, hi = np.minimum(lengths[:, None], lengths[None, :]), np.maximum(lengths[:, None], lengths[None, :])
    assert (6 * lo >= 5 * hi)[sfam[:, None] == sfam[None, :]].all() and (4 * lo[same] >= 3 * hi[same]).all() and lengths.min() > 5
    assert np.bincount(efam).max() == K_ALL == 2 * DOUBLE
    return rows, coords, seqs, efam, sfam


_built = {}


def structured(seed=SEED):
    """structured_rows plus what the tests expect of it, built once per process -> dict(rows, coords, seqs, lengths, efam, sfam,
    tm = {fast: {(a, b) canonical: printed max(qtm, ttm)}} over all neighbour pairs, rep: the representative every row must get at
    MINTM).  ASSERTS the margins in normal and fast mode: same-structure neighbour pairs >= TM_SAME, all others <= TM_OTHER."""
    if seed in _built:
        return _built[seed]
    rows, coords, seqs, efam, sfam = structured_rows(seed)
    lengths = np.asarray([len(c) for c in coords], np.int32)
    n = lengths.shape[0]
    tm = {False: {}, True: {}}
    for a in range(n):
        for b in range(a + 1, n):
            if efam[a] != efam[b]:
                continue
            x, y = canonical(a, b, lengths)
            for fast in (False, True):
                v = printed_max_tm(coords[x], seqs[x], coords[y], seqs[y], fast)
                tm[fast][(x, y)] = v
                if sfam[a] == sfam[b]:
                    assert v >= TM_SAME, ("same structure, low TM-score", x, y, fast, v)
                else:
                    assert v <= TM_OTHER, ("different structures, high TM-score", x, y, fast, v)
    rep = cc.planted_clusters(lengths, sfam)                              # (impostors: families of one)
    _built[seed] = dict(rows=rows, coords=coords, seqs=seqs, lengths=lengths, efam=efam, sfam=sfam, tm=tm, rep=rep)
    return _built[seed]


def write_structured(work, seed=SEED, edit=None):
    """The planted structure families as a database in BOTH layouts under `work` ('sfa', 'spt'; the `.pt` rows are the unit rows
    scaled per row).  edit: a function (coords list, seqs list, built dict) -> None that changes chains before they are written (the
    tests of chains TM-align cannot score).  -> (names, built dict of structured())."""
    from merizo_search_amd.foldclass import dbutil
    os.makedirs(work, exist_ok=True)
    built = structured(seed)
    n = built["rows"].shape[0]
    coords, seqs = [c.copy() for c in built["coords"]], list(built["seqs"])
    if edit is not None:
        edit(coords, seqs, built)
    names = ["s%03d_r%04d" % (built["sfam"][r] % 1000, r) for r in range(n)]
    dbutil.write_faiss_db(os.path.join(work, "sfa"), built["rows"], names, seqs, coords)
    raw = (built["rows"] * np.random.default_rng(seed + 1).uniform(0.5, 4.0, size=(n, 1))).astype(np.float32)
    dbutil.write_pt_db(os.path.join(work, "spt"), raw, ["/x/" + nm + ".pdb" for nm in names], coords, seqs)
    return names, built


def oracle_lists(rows, k, mincos=MINCOS):
    """The neighbour lists the self-search keeps at -k `k` on unit rows, from the oracle's own scores."""
    from oracle import oracle as orc
    n = rows.shape[0]
    s, i = orc.ip_topk(rows, rows, k + 1, order=1)
    idx, score = cc.empty_lists(n, k)
    for r in range(n):
        keep = [(sv, iv) for sv, iv in zip(s[r], i[r]) if iv != r and sv >= np.float32(mincos)][:k]
        for c, (sv, iv) in enumerate(keep):
            idx[r, c], score[r, c] = iv, sv
    return idx, score


def pipeline_graph_np(idx, score, src, dst, escore, lengths, tm_of, mode="greedy", mintm=MINTM, min_score=MINCOS, mincov=MINCOV):
    """`cluster --mintm` in numpy on a graph given as lists and extras (either may be None): cluster_pairs_np, the keep vector from
    tm_of(a, b) -> printed max(qtm, ttm) of the canonical pair, or None where TM-align cannot score it, pairs_apply_np, the cluster
    restatement of `mode`, and the fourth column through pairs_find_np.  -> (rep, rep_score, tm_score float64 [n] or None
    (connected), info: saturated, tm_pairs, tm_rejected_pairs, tm_unaligned_pairs, tm_removed_entries)."""
    import cluster_complete_case as ccc
    n = lengths.shape[0]
    pairs, saturated = cluster_pairs_np(idx, score, src, dst, escore, lengths, min_score, mincov)
    verdicts = [tm_of(int(a), int(b)) for a, b in pairs]
    tm = np.asarray([-1.0 if v is None else v for v in verdicts], np.float64)
    keep = (tm >= mintm).astype(np.uint8)
    idx2, score2, dst2, escore2, removed = pairs_apply_np(idx, score, src, dst, escore, lengths, min_score, mincov, pairs, keep)
    if mode == "connected":
        rep, rep_score, _info = cpc.cluster_components_np(idx2, score2, src, dst2, escore2, lengths, min_score, mincov)
        tm_score = None
    else:
        if src is None:
            rep, rep_score, _info = cc.cluster_greedy_np(idx2, score2, lengths, min_score, mincov)
        else:
            rep, rep_score, _info = ccc.cluster_greedy_edges_np(idx2, score2, src, dst2, escore2, lengths, min_score, mincov)
        members = np.nonzero(rep != np.arange(n))[0]
        tm_score = np.ones(n)
        tm_score[members] = tm[pairs_find_np(rep[members], members, lengths, pairs)]
    return rep, rep_score, tm_score, {"saturated": saturated, "tm_pairs": int(pairs.shape[0]), "tm_rejected_pairs": int((keep == 0).sum()),
                                      "tm_unaligned_pairs": sum(v is None for v in verdicts), "tm_removed_entries": removed}


def pipeline_np(built, k=K_ALL, mode="greedy", fast=False, mintm=MINTM):
    """pipeline_graph_np on the faiss layout's rows: the oracle's lists at -k k, the verdicts from the fixture's TM table."""
    idx, score = oracle_lists(built["rows"], k)
    return pipeline_graph_np(idx, score, None, None, None, built["lengths"], lambda a, b: built["tm"][fast][(a, b)], mode, mintm)
