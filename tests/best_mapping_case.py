"""ms_md_best_mappings restated on the CPU in numpy int64 -- TEST INFRASTRUCTURE (include/merizo_search_amd.h holds the definition).

    quantise        cell -> (allowed, integer weight)
    best_any        kind 0: rows inserted 0..nqd-1 by shortest augmenting path with potentials, every argmin the smallest column
    best_ordered    kind 1: the prefix-max dynamic programme and its backtrack (smallest argmax)
    best_mappings   the entry point, candidate by candidate, on descriptors: status, total, path, cell
    brute_force     the maximum of the integer totals over chain_mappings' own enumeration (small matrices only)
"""
from __future__ import annotations

import itertools

import numpy as np

MAX_QD, MAX_HD = 64, 1024
INF = np.iinfo(np.int64).max
NEG = np.iinfo(np.int64).min


def quantise(m):
    """(allowed bool, w int64) of float32 cells: allowed iff non-zero and not NaN (-0.0 is zero);
    w = llrint(clamp((double) cell, -2^20, 2^20) * 2^32), nearest even; 0 where the cell is not allowed."""
    m = np.asarray(m, dtype=np.float32)
    allowed = (m != 0) & ~np.isnan(m)
    x = np.where(allowed, m, np.float32(0)).astype(np.float64)
    w = np.rint(np.clip(x, -2.0 ** 20, 2.0 ** 20) * 2.0 ** 32).astype(np.int64)
    return allowed, w


def best_any(m):
    """-> (status, total, path list) of the best any-order mapping of a [nqd,nhd] matrix."""
    allowed, w = quantise(m)
    nqd, nhd = allowed.shape
    cost = -w
    cols = np.arange(nhd)
    u = np.zeros(nqd, np.int64)
    v = np.zeros(nhd, np.int64)
    row_of = np.full(nhd, -1, np.int64)
    for i in range(nqd):
        minv = np.full(nhd, INF, np.int64)
        way = np.full(nhd, -1, np.int64)            # the column a column was reached from; -1 = from the new row
        used = np.zeros(nhd, bool)
        j0 = -1                                     # the column the search stands on; -1 = the new row's own start
        while True:
            i0 = i if j0 < 0 else int(row_of[j0])
            free = ~used
            upd = free & allowed[i0]
            cur = np.where(upd, cost[i0] - u[i0] - v, INF)
            better = upd & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            cand = np.where(free, minv, INF)
            j1 = int(np.argmin(cand))               # (numpy: the first = smallest column among equals)
            delta = cand[j1]
            if delta == INF:
                return 0, 0, []
            # potentials: the rows of the used columns and the new row, the used columns; the others' slack
            u[row_of[used]] += delta
            u[i] += delta
            v[used] -= delta
            dec = free & (minv != INF)
            minv[dec] -= delta
            j0 = j1
            used[j0] = True
            if row_of[j0] < 0:
                break
        while j0 >= 0:                              # augment along `way`
            j1 = int(way[j0])
            row_of[j0] = i if j1 < 0 else row_of[j1]
            j0 = j1
    path = [-1] * nqd
    for j in cols[row_of >= 0]:
        path[int(row_of[j])] = int(j)
    return 1, int(sum(int(w[i, path[i]]) for i in range(nqd))), path


def best_ordered(m):
    """-> (status, total, path list) of the best order-preserving mapping of a [nqd,nhd] matrix."""
    allowed, w = quantise(m)
    nqd, nhd = allowed.shape
    D = np.full((nqd, nhd), NEG, np.int64)
    D[0][allowed[0]] = w[0][allowed[0]]
    for i in range(1, nqd):
        pm = np.full(nhd, NEG, np.int64)            # max over j' < j of D[i - 1][j']
        pm[1:] = np.maximum.accumulate(D[i - 1])[:-1]
        ok = allowed[i] & (pm != NEG)
        D[i][ok] = w[i][ok] + pm[ok]
    path, limit = [0] * nqd, nhd
    for i in range(nqd - 1, -1, -1):
        row = D[i][:limit]
        if row.size == 0 or row.max() == NEG:
            return 0, 0, []
        path[i] = limit = int(np.argmax(row))       # (the first = smallest column among equals)
    return 1, int(D[nqd - 1][path[-1]]), path


def best_mappings(scores, cand, mat_off, total_cells=None):
    """The entry point on host arrays: scores float32 [total_cells], cand [ncand,4] (only nqd = [1] and nhd = [3] are read), mat_off
    [ncand] -> (status int32 [ncand,2], total int64 [ncand,2], path int32 [ncand,2,64], cell float32 [ncand,2,64])."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    total_cells = scores.size if total_cells is None else int(total_cells)
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 4)
    mat_off = np.asarray(mat_off, dtype=np.int64).reshape(-1)
    n = len(cand)
    status = np.zeros((n, 2), np.int32)
    total = np.zeros((n, 2), np.int64)
    path = np.full((n, 2, MAX_QD), -1, np.int32)
    cell = np.zeros((n, 2, MAX_QD), np.float32)
    for c in range(n):
        nqd, nhd, off = int(cand[c, 1]), int(cand[c, 3]), int(mat_off[c])
        if nqd < 1 or nhd < 1:
            status[c] = -1
        elif nqd > MAX_QD or nhd > MAX_HD:
            status[c] = -2
        elif off < 0 or off + nqd * nhd > total_cells:
            status[c] = -1
        else:
            m = scores[off: off + nqd * nhd].reshape(nqd, nhd)
            for kind, solve in enumerate((best_any, best_ordered)):
                st, tot, p = solve(m)
                status[c, kind] = st
                if st == 1:
                    total[c, kind] = tot
                    path[c, kind, :nqd] = p
                    cell[c, kind, :nqd] = m[np.arange(nqd), p]
    return status, total, path, cell


def brute_force(m):
    """(best any-order integer total or None, best order-preserving integer total or None) over the enumeration chain_mappings runs:
    the product of the rows' non-zero columns, one-to-one paths only."""
    allowed, w = quantise(m)
    nqd = allowed.shape[0]
    best = [None, None]
    for p in itertools.product(*[np.flatnonzero(allowed[r]).tolist() for r in range(nqd)]):
        if len(set(p)) != nqd:
            continue
        t = sum(int(w[i, j]) for i, j in enumerate(p))
        kinds = (0, 1) if all(b > a for a, b in zip(p, p[1:])) else (0,)
        for k in kinds:
            if best[k] is None or t > best[k]:
                best[k] = t
    return best
