"""Helpers of the `cluster --cluster_mode connected` tests (TEST INFRASTRUCTURE): the sequential restatement of
ms_cluster_components -- the definition the kernels are compared with, bit for bit -- its oracle-engine hook for the CPU runs of
the driver, the entry layouts of the GPU tests (paths, stars, the same entries split between lists and extras) and a database of
planted chains and dumbbells in both layouts: groups that single linkage keeps together and the greedy mode cuts up."""
import os

import numpy as np

import cluster_case as cc
import cluster_complete_case as ccc

NINF = np.float32(-np.inf)


# ------------------------------------------------------------------ ms_cluster_components, restated ----
def valid_entries(i, j, s, lengths, min_score, mincov):
    """The validity rule of include/merizo_search_amd.h (ms_cluster_greedy) on directed entries i[e] -> j[e] with score s[e], computed
    as cluster_case.cluster_greedy_np computes it; an i outside [0, n) makes an entry invalid too.  -> bool [len(i)]."""
    i, j, s = np.asarray(i, np.int64), np.asarray(j, np.int64), np.asarray(s, np.float32)
    L = np.asarray(lengths, np.int32)
    n = L.shape[0]
    inside = (i >= 0) & (i < n) & (j >= 0) & (j < n) & (i != j)
    a, b = np.where(inside, i, 0), np.where(inside, j, 0)                  # (rows outside [0, n) are never looked up)
    l_min = np.minimum(L[a], L[b]).astype(np.float32)
    l_max = np.maximum(L[a], L[b]).astype(np.float32)
    covers = l_min >= np.float32(mincov) * l_max                           # fp32 product, this operand order
    with np.errstate(invalid="ignore"):
        return inside & covers & (s >= np.float32(min_score))              # (NaN compares false)


def cluster_components_np(idx, score, src, dst, escore, lengths, min_score, mincov):
    """include/merizo_search_amd.h, ms_cluster_components, restated SEQUENTIALLY: a union-find over the valid entries of the lists
    (idx, score: [n,k] or None) and of the extras (src, dst, escore: [m] or None), then the representative and the link score by
    plain loops.  -> (rep int64 [n], link_score float32 [n], info) with info = {'n_components', 'saturated'}."""
    L = np.asarray(lengths, np.int32)
    n = L.shape[0]
    if idx is None:
        idx, score = np.empty((n, 0), np.int64), np.empty((n, 0), np.float32)
    idx, score = np.asarray(idx, np.int64), np.asarray(score, np.float32)
    k = idx.shape[1]
    assert idx.shape == score.shape == (n, k)
    none = src is None
    src = np.empty(0, np.int64) if none else np.asarray(src, np.int64)
    dst = np.empty(0, np.int64) if none else np.asarray(dst, np.int64)
    escore = np.empty(0, np.float32) if none else np.asarray(escore, np.float32)
    i = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), k), src])
    j = np.concatenate([idx.ravel(), dst])
    s = np.concatenate([score.ravel(), escore])
    valid = valid_entries(i, j, s, L, min_score, mincov)
    saturated = int(valid[:n * k].reshape(n, k).all(axis=1).sum()) if k else 0

    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    best = np.full(n, NINF, np.float32)                                    # the largest weight among the row's own valid edges
    for a, b, w in zip(i[valid].tolist(), j[valid].tolist(), (s[valid] + np.float32(0.0)).tolist()):    # -0.0 counts as +0.0
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
        w = np.float32(w)
        for x in (a, b):
            if w > best[x]:
                best[x] = w
    root = np.array([find(x) for x in range(n)], np.int64)
    rep = np.empty(n, np.int64)
    for r in np.unique(root):
        members = np.nonzero(root == r)[0]
        rep[members] = min(members.tolist(), key=lambda x: (-int(L[x]), x))   # the longest domain, the smaller row on a tie
    link = np.where(rep == np.arange(n), np.float32(1.0), best).astype(np.float32)
    return rep, link, {"n_components": int(np.unique(root).size), "saturated": saturated}


def install_oracle_components():
    """cluster_complete_case.install_oracle_complete plus OracleEngine.cluster_components = cluster_components_np: the CPU runs of
    `cluster --cluster_mode connected`."""
    import torch
    Engine = ccc.install_oracle_complete()

    def cluster_components(self, nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score, mincov=0.0):
        host = lambda t: None if t is None else t.numpy()
        rep, link, info = cluster_components_np(host(nbr_idx), host(nbr_score), host(edge_src), host(edge_dst), host(edge_score),
                                                np.asarray(lengths), min_score, mincov)
        return torch.from_numpy(rep), torch.from_numpy(link), dict(info, rounds=0)

    Engine.cluster_components = cluster_components
    return Engine


# ------------------------------------------------------------------ entry layouts of the GPU tests ----
def path_lists(order, lengths_along=None):
    """One path through the rows in `order` (a permutation of 0..n-1): row order[t] holds the entry to order[t + 1] with score 0.8 in
    lists of k = 1.  lengths_along: the length of the t-th row of the path (default: all 100).  -> (idx, score, lengths)."""
    order = np.asarray(order, np.int64)
    n = order.shape[0]
    idx, score = cc.empty_lists(n, 1)
    idx[order[:-1], 0], score[order[:-1], 0] = order[1:], np.float32(0.8)
    lengths = np.full(n, 100, np.int32)
    if lengths_along is not None:
        lengths[order] = np.asarray(lengths_along, np.int32)
    return idx, score, lengths


def lists_as_extras(idx, score, columns, seed):
    """The entries of the list columns `columns` as extra entries (src = the row), in a seeded random order.  -> (src, dst, score)."""
    n = idx.shape[0]
    src = np.repeat(np.arange(n, dtype=np.int64), len(columns))
    dst, sc = idx[:, columns].ravel(), score[:, columns].ravel()
    order = np.random.default_rng(seed).permutation(src.shape[0])
    return np.ascontiguousarray(src[order]), np.ascontiguousarray(dst[order]), np.ascontiguousarray(sc[order])


# ------------------------------------------------------------------ a database of planted chains and dumbbells ----
CHAIN_SIZES = (1, 1, 2, 3, 4, 5, 7, 9, 16, 33)                            # members per chain; four chains of each
CHAIN_STEP = 0.75                                                         # cosine of adjacent members; second neighbours: 0.5625
DUMBBELLS, CLIQUE, CENTRE_COS, CLIQUE_SIGMA = 10, 6, 0.80, 0.1
MINCOS = 0.7
ROWS, GROUPS, LARGEST = 444, 50, 33
SPLIT_AT_K4 = GROUPS + DUMBBELLS                                          # -k 4 keeps only a clique's own members: every dumbbell in two
DOMAIN_LENGTH = 60


def _fresh_direction(rng, basis):
    """A unit vector orthogonal to every (orthonormal) vector of `basis`; it joins the basis."""
    u = rng.standard_normal(128)
    for b in basis:
        u -= (u @ b) * b
    for b in basis:                                                        # (a second sweep: the first leaves ~1e-16 behind)
        u -= (u @ b) * b
    u /= np.linalg.norm(u)
    basis.append(u)
    return u


def chain_rows(seed=5):
    """Unit rows of the planted groups, shuffled.  Chains: member t+1 = 0.75 m_t + sqrt(1 - 0.75^2) u_t with u_t a fresh unit
    direction orthogonal to all earlier ones of its chain.  Dumbbells: two centres at cosine 0.80, six members each at
    normalize(c + 0.1 g / sqrt(128)).  ASSERTS, on the CPU oracle's own scores, that no off-diagonal cosine lies within 0.02 of
    MINCOS and that the threshold graph has exactly the planted groups as components.  -> (rows float32 [444,128], group int64 [444])."""
    from oracle import oracle as orc
    rng = np.random.default_rng(seed)
    rows, group = [], []
    g = 0
    for size in CHAIN_SIZES * 4:
        basis = []
        m = _fresh_direction(rng, basis)
        for _t in range(size):
            rows.append(m)
            group.append(g)
            m = CHAIN_STEP * m + np.sqrt(1.0 - CHAIN_STEP ** 2) * _fresh_direction(rng, basis)
        g += 1
    for _d in range(DUMBBELLS):
        basis = []
        c1 = _fresh_direction(rng, basis)
        c2 = CENTRE_COS * c1 + np.sqrt(1.0 - CENTRE_COS ** 2) * _fresh_direction(rng, basis)
        for c in (c1, c2):
            members = c + CLIQUE_SIGMA * rng.standard_normal((CLIQUE, 128)) / np.sqrt(128.0)
            rows.extend(members / np.linalg.norm(members, axis=1, keepdims=True))
            group.extend([g] * CLIQUE)
        g += 1
    rows, group = np.asarray(rows, np.float32), np.asarray(group, np.int64)
    n = rows.shape[0]
    assert n == ROWS and g == GROUPS and np.bincount(group).max() == LARGEST
    perm = rng.permutation(n)
    rows, group = np.ascontiguousarray(rows[perm]), group[perm]
    s, i = orc.ip_topk(rows, rows, n, order=1)                             # every cosine, as the oracle computes it
    cos = np.empty((n, n), np.float32)
    np.put_along_axis(cos, i, s, axis=1)
    off = ~np.eye(n, dtype=bool)
    margin = np.abs(cos[off] - np.float32(MINCOS)).min()
    assert margin >= 0.02, ("planted chains: a cosine within 0.02 of the threshold", float(margin))
    assert cos[group[:, None] != group[None, :]].max() <= MINCOS - 0.02
    a, b = np.nonzero((cos >= MINCOS) & off)
    _rep, _link, info = cluster_components_np(None, None, a, b, cos[a, b], np.full(n, DOMAIN_LENGTH, np.int32), MINCOS, 0.0)
    assert info["n_components"] == GROUPS
    return rows, group


def write_chains(work, seed=5):
    """The planted chains and dumbbells as a database in BOTH layouts under `work` ('cfa', 'cpt'; the `.pt` rows are the unit rows
    scaled per row), every domain DOMAIN_LENGTH long.  -> (names, lengths, group)."""
    from merizo_search_amd.foldclass import dbutil, synthetic as syn
    os.makedirs(work, exist_ok=True)
    rows, group = chain_rows(seed)
    n = rows.shape[0]
    lengths = np.full(n, DOMAIN_LENGTH, np.int32)
    rng = np.random.default_rng(seed + 1)
    names = ["grp%02d_r%04d" % (group[r], r) for r in range(n)]
    seqs = ["".join(rng.choice(list("ACDEFGHIKL"), size=int(l))) for l in lengths]
    coords = [syn.random_walk(int(l), seed * 7919 + r) for r, l in enumerate(lengths)]
    dbutil.write_faiss_db(os.path.join(work, "cfa"), rows, names, seqs, coords)
    raw = (rows * rng.uniform(0.5, 4.0, size=(n, 1))).astype(np.float32)
    dbutil.write_pt_db(os.path.join(work, "cpt"), raw, ["/x/" + nm + ".pdb" for nm in names], coords, seqs)
    return names, lengths, group
