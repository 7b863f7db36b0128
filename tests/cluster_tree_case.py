"""Helpers of the `cluster --tree / --levels` tests (TEST INFRASTRUCTURE): the sequential restatement of ms_cluster_tree -- Kruskal's
algorithm over the valid entries in the header's strict order, the definition the kernels are compared with -- its oracle-engine
hook for the CPU runs of the driver, and the entry layouts of the GPU tests (rings, a star, two cliques with a bridge)."""
import numpy as np

import cluster_case as cc
import cluster_complete_case as ccc
import cluster_components_case as cpc

NINF = np.float32(-np.inf)


# ------------------------------------------------------------------ ms_cluster_tree, restated ----
def all_entries(idx, score, src, dst, escore, n):
    """The directed entries of the lists (idx, score: [n,k] or None) and the extras (src, dst, escore: [m] or None) as three arrays
    i, j, s, lists first; k of the lists."""
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


def cluster_tree_np(idx, score, src, dst, escore, lengths, min_score, mincov):
    """include/merizo_search_amd.h, ms_cluster_tree, restated SEQUENTIALLY: the undirected edges of the valid entries
    (cluster_components_case.valid_entries), each with the larger of its valid directed scores (-0.0 as +0.0), sorted by weight
    descending, then (min row, max row) ascending; Kruskal's algorithm with a union-find keeps the edges that join two trees.
    -> (a int64 [e], b int64 [e], w float32 [e], info): the forest IN THAT ORDER, a < b; info = {'n_edges', 'saturated'}."""
    L = np.asarray(lengths, np.int32)
    n = L.shape[0]
    i, j, s, k = all_entries(idx, score, src, dst, escore, n)
    valid = cpc.valid_entries(i, j, s, L, min_score, mincov)
    saturated = int(valid[:n * k].reshape(n, k).all(axis=1).sum()) if k else 0
    weight = {}
    for x, y, w in zip(i[valid].tolist(), j[valid].tolist(), (s[valid] + np.float32(0.0)).tolist()):
        key = (min(x, y), max(x, y))
        if key not in weight or w > weight[key]:
            weight[key] = w
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    forest = []
    for (x, y), w in sorted(weight.items(), key=lambda item: (-item[1], item[0])):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
            forest.append((x, y, w))
    a = np.array([e[0] for e in forest], np.int64)
    b = np.array([e[1] for e in forest], np.int64)
    w = np.array([e[2] for e in forest], np.float32)
    return a, b, w, {"n_edges": len(forest), "saturated": saturated}


def forest_set(a, b, w):
    """{(a, b, weight bits)} of a forest."""
    return set(zip(np.asarray(a, np.int64).tolist(), np.asarray(b, np.int64).tolist(), ccc.bits(w).tolist()))


def slots_as_forest(pairs, weight):
    """The outputs of ms_cluster_tree (pairs int32 [n,2], weight float32 [n]) -> (a, b, w) of the filled slots; ASSERTS the slot
    layout: a < b in a filled slot, (-1, -1) with -inf in an empty one."""
    pairs, weight = np.asarray(pairs), np.asarray(weight, np.float32)
    filled = pairs[:, 0] >= 0
    assert np.all(pairs[filled, 0] < pairs[filled, 1])
    assert np.all(pairs[~filled] == -1) and np.all(weight[~filled] == NINF) and not np.isnan(weight[filled]).any()
    return pairs[filled, 0].astype(np.int64), pairs[filled, 1].astype(np.int64), weight[filled]


def install_oracle_tree():
    """cluster_components_case.install_oracle_components plus OracleEngine.cluster_tree = cluster_tree_np: the CPU runs of `cluster
    --tree / --levels`.  (The forest fills slots 0 .. e-1: the driver reads the filled slots, not which row holds which edge.)"""
    import torch
    Engine = cpc.install_oracle_components()

    def cluster_tree(self, nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score, mincov=0.0):
        host = lambda t: None if t is None else t.numpy()
        lengths = np.asarray(lengths)
        n = lengths.shape[0]
        a, b, w, info = cluster_tree_np(host(nbr_idx), host(nbr_score), host(edge_src), host(edge_dst), host(edge_score), lengths, min_score, mincov)
        pairs, weight = np.full((n, 2), -1, np.int32), np.full(n, NINF, np.float32)
        pairs[:a.shape[0], 0], pairs[:a.shape[0], 1], weight[:a.shape[0]] = a, b, w
        return torch.from_numpy(pairs), torch.from_numpy(weight), dict(info, rounds=0)

    Engine.cluster_tree = cluster_tree
    return Engine


# ------------------------------------------------------------------ entry layouts of the GPU tests ----
def ring_lists(n, weight=0.8):
    """A ring of n rows, every edge of one weight: row t holds the entry to (t + 1) % n in lists of k = 1.  -> (idx, score, lengths)."""
    idx, score = cc.empty_lists(n, 1)
    idx[:, 0], score[:, 0] = (np.arange(n) + 1) % n, np.float32(weight)
    return idx, score, np.full(n, 100, np.int32)


def star_lists(leaves, seed=0):
    """`leaves` leaves around row 0, each edge held by its leaf (k = 1), weights from 7 values.  -> (idx, score, lengths)."""
    n = leaves + 1
    idx, score = cc.empty_lists(n, 1)
    idx[1:, 0] = 0
    score[1:, 0] = (0.6 + 0.05 * np.random.default_rng(seed).integers(0, 7, size=leaves)).astype(np.float32)
    return idx, score, np.full(n, 80, np.int32)


TREE_CUT = np.float32(0.6)
TREE_SCORES = np.linspace(0.55, 0.9, 8).astype(np.float32)                # 8 values, one below the cut: heavy ties


def random_graph(n, k, m, seed):
    """Random lists [n,k] and m extras with scores quantised to TREE_SCORES, lengths from cluster_case.LENGTH_VALUES (meant for min_score
    TREE_CUT, mincov 0.7), seeded with everything that is no edge: self-loops, j = -1, j = n, j = 2^40, NaN, -inf padding, scores below
    the cut, and among the extras an edge_src that is no row (-1, n, 2^40).  -> (idx, score, (src, dst, escore), lengths)."""
    rng = np.random.default_rng(seed)
    lengths = rng.choice(cc.LENGTH_VALUES, size=n).astype(np.int32)
    idx = rng.integers(0, n, size=(n, k)).astype(np.int64)
    score = TREE_SCORES[rng.integers(0, 8, size=(n, k))]
    src, dst = rng.integers(0, n, size=m).astype(np.int64), rng.integers(0, n, size=m).astype(np.int64)
    escore = TREE_SCORES[rng.integers(0, 8, size=m)]
    for rows, scores in ((idx.reshape(-1), score.reshape(-1)), (dst, escore)):
        what = rng.random(rows.shape[0])
        own = np.repeat(np.arange(n), k) if rows.shape[0] == n * k else src
        rows[what < 0.02] = own[what < 0.02]                               # self-loops
        rows[(what >= 0.02) & (what < 0.04)] = -1
        rows[(what >= 0.04) & (what < 0.05)] = n
        rows[(what >= 0.05) & (what < 0.06)] = 1 << 40
        scores[(what >= 0.06) & (what < 0.08)] = np.nan
        scores[(what >= 0.08) & (what < 0.12)] = NINF
        scores[(what >= 0.12) & (what < 0.13)] = np.nextafter(TREE_CUT, np.float32(0.0))
    bad = rng.random(m)
    src[bad < 0.01] = -1
    src[(bad >= 0.01) & (bad < 0.02)] = n
    src[(bad >= 0.02) & (bad < 0.03)] = 1 << 40
    return idx.reshape(n, k), score.reshape(n, k), (src, dst, escore), lengths


def two_cliques(size=40, inside=0.9, bridge=0.7):
    """Two cliques of `size` rows (rows [0, size) and [size, 2 size), every pair at `inside`, each row listing the others) and one
    weaker bridge, held as an extra entry from the last row of the first to the first row of the second.
    -> (idx, score, (src, dst, escore), lengths)."""
    n = 2 * size
    idx, score = cc.empty_lists(n, size - 1)
    for r in range(n):
        lo = 0 if r < size else size
        idx[r] = [c for c in range(lo, lo + size) if c != r]
        score[r] = np.float32(inside)
    extras = (np.array([size - 1], np.int64), np.array([size], np.int64), np.array([bridge], np.float32))
    return idx, score, extras, np.full(n, 100, np.int32)
