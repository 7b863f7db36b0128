"""Helpers of the `database_cosine` multi-domain tests (TEST INFRASTRUCTURE; the product never imports this).

    scan_ref       ms_md_chain_scan restated from multidom_case.dot_matrix, cut and match_counts: one matrix per (query chain,
                   target chain), kept when every row and at least nqd columns hold a non-zero cell.  It takes PREPARED queries.
    fixed_layout   the 697-row layout of test_md_scan_gpu.py with its planted relatives
    random_case    one seeded random shape with planted relatives
"""
import numpy as np

import multidom_case as mc

MAX_NQD = 64                  # include/merizo_search_amd.h: query domains per query chain ms_md_chain_scan serves
MINCOS = np.float32(0.5)


def table_of(lengths) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


def unit(x) -> np.ndarray:
    x = np.asarray(x, np.float32)
    return (x / np.linalg.norm(x.astype(np.float64), axis=-1, keepdims=True)).astype(np.float32)


def noisy(v, rng) -> np.ndarray:
    """A copy of v with cosine about 0.98 to it."""
    v = np.asarray(v, np.float32)
    return (v + 0.2 * np.linalg.norm(v) / np.sqrt(128.0) * rng.standard_normal(128)).astype(np.float32)


def bad_chain(q0, nqd, nq) -> bool:
    return nqd < 1 or nqd > MAX_NQD or q0 < 0 or q0 + nqd > nq


def scan_ref(db, qprep, table, qchain, min_score, lengths=None, qlen=None, mincov=0.0, tally=None):
    """-> (sorted list of (g, c), qstatus list).  tally: a dict that receives how the served pairs with nhd >= nqd came out:
    'qualify', 'rows' (fails on the row condition alone), 'cols' (on the column condition alone), 'both'."""
    db = np.asarray(db, np.float32).reshape(-1, 128)
    qprep = np.asarray(qprep, np.float32).reshape(-1, 128)
    table = np.asarray(table, np.int64)
    nq = qprep.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = mc.dot_matrix(qprep, db)
        if lengths is not None:
            lim = (np.asarray(lengths, np.float32) * np.float32(mincov)).astype(np.float32)
            s = (s * (np.asarray(qlen, np.float32)[:, None] >= lim[None, :]).astype(np.float32)).astype(np.float32)
    s = mc.cut(s, min_score)
    pairs, status = [], []
    for g, (q0, nqd) in enumerate(np.asarray(qchain, np.int64).reshape(-1, 2)):
        status.append(-1 if bad_chain(q0, nqd, nq) else 0)
        if status[-1]:
            continue
        for c in range(len(table) - 1):
            a, b = int(table[c]), int(table[c + 1])
            nr, nc = mc.match_counts(s[q0: q0 + nqd, a:b])
            ok_r, ok_c = nr == nqd, nc >= nqd
            if ok_r and ok_c:
                pairs.append((g, c))
            if tally is not None and b - a >= nqd:
                key = "qualify" if ok_r and ok_c else "rows" if ok_c else "cols" if ok_r else "both"
                tally[key] = tally.get(key, 0) + 1
    return sorted(pairs), status


# ------------------------------------------------------------------ the fixed layout
FIXED_LENGTHS = [1, 2, 3, 63, 64, 65, 130, 1, 5, 8, 3, 2, 64, 130, 66, 9, 4, 70, 7]        # 697 rows = 10 * 64 + 57
FIXED_NQD = [2, 3, 5, 8, 64, 2, 131]          # g2 and g5: domains 0 and 1 are twins (noisy copies of one vector); g6: not served


def fixed_layout(seed=5):
    """-> dict(db [697,128] unit rows, table, q [nq,128] unit queries, qchain, expect {(g, c): qualifies?} of the planted pairs,
    masked = (row, g, c): the planted match a length of 100 at `row` masks away in MS_MODE_COSINE_UNIT).
    Planted: per query chain target chains that qualify, chains that miss exactly one query domain, chains where the twin domains
    match only ONE target domain (rows all non-zero, columns nqd - 1), and in the 130-row chains copies on both sides of a 64-row
    piece boundary (offsets 63 | 64, and 0, 127 | 129)."""
    rng = np.random.default_rng(seed)
    table = table_of(FIXED_LENGTHS)
    n = int(table[-1])
    db = rng.standard_normal((n, 128)).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum(FIXED_NQD)])
    q = rng.standard_normal((int(starts[-1]), 128)).astype(np.float32)
    for g in (2, 5):
        q[starts[g] + 1] = noisy(q[starts[g]], rng)
    expect = {}

    def plant(g, c, where, ok):
        """where: {offset in chain c: query domain of g}"""
        for off, d in where.items():
            assert 0 <= off < FIXED_LENGTHS[c]
            db[table[c] + off] = noisy(q[starts[g] + d], rng)
        expect[(g, c)] = ok

    plant(0, 1, {0: 0, 1: 1}, True)
    plant(0, 6, {63: 0, 64: 1}, True)                       # each side of the first piece boundary of a 130-row chain
    plant(0, 11, {0: 0}, False)                             # one query domain missing
    plant(0, 14, {0: 0, 65: 1}, True)                       # a 66-row chain: the last row is a piece of its own
    plant(1, 2, {0: 2, 1: 1, 2: 0}, True)
    plant(1, 13, {0: 0, 127: 1, 129: 2}, True)
    plant(1, 10, {0: 0, 1: 1}, False)
    plant(2, 8, {0: 0, 2: 2, 3: 3, 4: 4}, False)            # the twins share row 0: 5 rows matched, 4 columns
    plant(2, 3, {5: 0, 40: 1, 41: 2, 42: 3, 62: 4}, True)
    plant(3, 9, {i: i for i in range(8)}, True)
    plant(3, 15, {i: i for i in range(7)}, False)
    plant(4, 4, {i: i for i in range(64)}, True)            # nqd = 64: the full mask
    plant(4, 5, {i + 1: i for i in range(64)}, True)
    plant(4, 12, {i: i for i in range(63)}, False)
    plant(5, 16, {1: 0}, False)                             # two query domains on the same single target domain
    plant(5, 18, {2: 0, 6: 1}, True)
    qchain = np.asarray([(int(starts[g]), nqd) for g, nqd in enumerate(FIXED_NQD)], np.int32)
    return dict(db=unit(db), table=table, q=unit(q), qchain=qchain, expect=expect, masked=(int(table[1]) + 1, 0, 1), n=n)


# ------------------------------------------------------------------ seeded random shapes
RANDOM_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 129, 200)


def random_case(seed):
    """n in [1, 3000], chain lengths from RANDOM_LENGTHS (the last chain cut to fit), 1..6 query chains of 1..8 domains (every
    second one with twin domains 0 and 1), and per query chain planted target chains: all domains copied; one domain missing and
    another copied twice (nqd columns, nqd - 1 rows: fails on the row condition alone); the twins on one row and the others copied
    (fails on the column condition alone).  -> dict(db, table, q, qchain)."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 3001))
    lengths, left = [], n
    while left > 0:
        run = min(int(rng.choice(RANDOM_LENGTHS)), left)
        lengths.append(run)
        left -= run
    table = table_of(lengths)
    nqc = int(rng.integers(1, 7))
    nqds = [int(rng.integers(1, 9)) for _ in range(nqc)]
    starts = np.concatenate([[0], np.cumsum(nqds)])
    db = rng.standard_normal((n, 128)).astype(np.float32)
    q = rng.standard_normal((int(starts[-1]), 128)).astype(np.float32)
    twins = [nqd >= 2 and g % 2 == 1 for g, nqd in enumerate(nqds)]
    for g in range(nqc):
        if twins[g]:
            q[starts[g] + 1] = noisy(q[starts[g]], rng)
    free = list(rng.permutation(len(lengths)))
    for g, nqd in enumerate(nqds):
        for kind in ("all", "dup", "twin", "all"):
            fit = [c for c in free if lengths[c] >= (nqd - 1 if kind == "twin" else nqd)]
            if not fit or (kind == "twin" and not twins[g]) or (kind == "dup" and nqd < 2):
                continue
            c = fit[0]
            free.remove(c)
            doms = list(range(nqd))
            if kind == "dup":
                doms.remove(int(rng.integers(0, nqd)))
                doms.append(int(rng.choice(doms)))
            if kind == "twin":
                doms.remove(1)
            offs = np.sort(rng.choice(lengths[c], size=len(doms), replace=False))
            for off, d in zip(offs, rng.permutation(doms)):
                db[table[c] + off] = noisy(q[starts[g] + d], rng)
    qchain = np.asarray([(int(starts[g]), nqd) for g, nqd in enumerate(nqds)], np.int32)
    return dict(db=unit(db), table=table, q=unit(q), qchain=qchain, n=n)
