"""Cases for the fp16 cell filter of ms_threshold_edges and ms_md_chain_scan_mq (csrc/ms_mq.h) away from B = 1: row-norm bounds from
2^-40 to 2^40, query norms from 2^-36 to 2^36, cuts on, next to and around the scores of worst-case cells, and the references
(TEST INFRASTRUCTURE, no GPU; the product never imports this).

    the filter   a cell is proved below min_score when its fp16 score a is below
                     thr[q] = (min_score - E B |q| (1 + 1e-5)) 2^(sr + sq),  sr = 14 - ilogb(B),  sq = 13 - exponent(max |q_i|)
                 (pushed down by 2^-22 of its magnitude; -inf for a flagged query or a threshold below 2^-100 in that domain); a row
                 whose sum of squares is above B^2 (1 + 1e-5) and a query whose norm is outside [2^-40, 2^40] are scored exactly.
    one case     (B, f, mode): pf_adversarial's families (rows that round down, rows that round up, the query's own rounding, the
                 query's components that underflow) times 2^ilogb(B), their queries times 2^f, each family with a query of its own,
                 among filler rows and queries at the same scales.  Scaling by powers of two is exact in the fmaf chain and in the
                 fp16 operands, so the rounding pattern that pa.a_model puts on the wrong side of a cut at B ~ 1 sits there at every
                 scale (tests/test_mq_filter_case.py checks that through the model alone).
    two layouts  "edges": 150 rows x 40 queries, the family rows at rows 0, 63, 64, 127 (both ends of both whole 64-row tiles), 1,
                 62, 65, 126 and in the last, partial tile; the family queries at 0, 31, 32, 39 (both sides of the 32-query tile edge).
                 "chains": 75 chains of 2 rows x 20 query chains of 2 domains; a family row is the first row of its chain and a family
                 query the first domain of its query chain, the second row and the second domain are one unrelated unit vector, so the
                 pair stands and falls with the family cell.  The scan packs 32 such chains into a tile: the family chains are chains
                 0, 31, 32, 63 (tile rows 0 and 62 of both whole tiles), 1, 30, 33, 62 and four of the partial tile.
    the filler   Rows and queries are built on an orthonormal basis of the complement of the families' span.  Filler rows are
                 orthogonal to the second domains, have cosine -0.02 to every family query (a definite score: a rounding residue
                 would leave the fp32 normal range at 2^-76), lean by -0.05 on one filler query (LEAN: every cell of it is proved
                 at a positive cut, at any norm the filter serves) and by -0.67 ... 0.014 on two others (scores on both sides of
                 the negative cut): at the cut of any family cell little more than the 12 family rows is left to the exact chain,
                 under 10 % of the cells -- what lets `rescored` tell a working filter from one that proves nothing.  The cells
                 of family rows and second rows against filler queries are rounding residues around 0: the cuts 0.0 and -0.0 run
                 through them.
    references   scores = multidom_case.dot_matrix (the scan's fmaf chain) over the PREPARED queries; edges_ref and pairs_ref are the
                 exact sets at a cut; rescored_bounds bounds out_stats[0] from both sides.
"""
import functools

import numpy as np

import multidom_case as mc
import pf_adversarial as pa

E = 1.05e-3                            # ms_pf_err_coef(MS_PF_F16X1)
MODES = ("prenorm", "normq", "unit")
BOUNDS = (2.0 ** -40, 1.5 * 2.0 ** -20, 1.0 + 1e-6, 1.9999, 3.0, 2.0 ** 40)      # the smallest and the largest accepted at the ends
QUERY_SCALES = {"prenorm": (-36, 0, 36), "normq": (0,), "unit": (0,)}           # f: the modes that normalise take the queries at 2^0
M = 3                                  # rows per family
N, NQ = 150, 40
ROW_POS = (0, 63, 64, 127, 128, 149, 1, 62, 65, 126, 130, 140)      # "edges": row of family cell 4 j + k (family k, its row j)
QUERY_POS = (0, 31, 32, 39)                                         # "edges": query of family k
CHAIN_POS = (0, 31, 32, 63, 64, 74, 1, 30, 33, 62, 65, 70)          # "chains": chain of family cell 4 j + k
QCHAIN_POS = (0, 15, 16, 19)                                        # "chains": query chain of family k (queries 0, 30, 32, 38)
LEAN = 1                               # the filler query every filler row leans away from (both layouts)
LEAN_COS = -0.05
FAMILY_COS = -0.02                     # every filler row against every family query: a definite score, not a rounding residue


def all_cases():
    """(B, f, mode) of every case."""
    return [(b, f, mode) for b in BOUNDS for mode in MODES for f in QUERY_SCALES[mode]]


def case_id(case):
    b, f, mode = case
    return "B%s-f%d-%s" % (("2^%d" % pa.ilogb(b)) if np.frexp(b)[0] == 0.5 else ("%.7g" % b), f, mode)


# ---- the helpers every mq test shares -------------------------------------------------------------------------------------------
def mode_code(mode):
    from merizo_search_amd import _lib
    return {"prenorm": _lib.MODE_IP_PRENORM, "normq": _lib.MODE_IP_NORMQ, "unit": _lib.MODE_COSINE_UNIT}[mode]


def to_gpu(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def prepared(q, mode):
    """The queries as the scan of `mode` multiplies with them (the GPU's own normalisation launch)."""
    from merizo_search_amd import ops
    if mode == "prenorm":
        return np.array(q, np.float32)
    return ops.l2_normalize_rows(to_gpu(q, np.float32), 1e-12 if mode == "normq" else 1e-8).cpu().numpy()


# ---- the case at B in [1, 2), f = 0 ---------------------------------------------------------------------------------------------
def families():
    """[(query, rows [M,128])] at the scale of B in [1, 2): |row| <= 0.998 (the fourth: 0.75, and |q| = 2^-3)."""
    return [pa.f16_row_rounding(21, M, side=-1), pa.f16_row_rounding(22, M, side=+1), pa.f16x1_query_rounding(23, M),
            pa.query_underflow(24, M)]


@functools.lru_cache(maxsize=None)
def _unit_layouts():
    """Both layouts at e = f = 0 -> dict(layout -> dict(db, q, cells, and for "chains" table, qchain, pairs))."""
    fams = families()
    rng = np.random.default_rng(77)
    span = np.concatenate([np.stack([fq for fq, _r in fams]), np.concatenate([r for _q, r in fams])]).astype(np.float64)
    basis, _ = np.linalg.qr(np.concatenate([span, rng.standard_normal((pa.DIM - len(span), pa.DIM))]).T)
    free = basis[:, len(span):].T                                   # 112 orthonormal vectors, orthogonal to every family vector
    second, fq_dirs, row_dirs = free[:4], free[4:NQ], free[NQ:]
    fam_dirs = span[:4] / np.linalg.norm(span[:4], axis=1, keepdims=True)

    def f32_below_one(v):                                           # |v| <= 1 after the rounding to fp32
        v = (np.asarray(v, np.float64) * 0.999).astype(np.float32)
        assert np.linalg.norm(v.astype(np.float64), axis=-1).max() <= 1.0
        return v

    def filler_rows(count, nfq):
        """Unit rows orthogonal to the second domains; cosine FAMILY_COS to the family queries, LEAN_COS to filler query LEAN and
        -0.67 ... 0.014 to two more of the nfq filler queries in use."""
        out = []
        for _ in range(count):
            w = row_dirs.T @ rng.standard_normal(len(row_dirs))
            w /= np.linalg.norm(w)
            j = rng.choice(np.setdiff1d(np.arange(nfq), [LEAN]), size=2, replace=False)
            c = rng.uniform(-0.95, 0.02, size=2) / np.sqrt(2.0)
            lean = np.concatenate([[LEAN_COS], c])
            v = fq_dirs[LEAN] * lean[0] + fq_dirs[j[0]] * c[0] + fq_dirs[j[1]] * c[1] + w * np.sqrt(1.0 - (lean ** 2).sum())
            v = (v + FAMILY_COS * fam_dirs.sum(axis=0)) / np.sqrt(1.0 + 4 * FAMILY_COS ** 2 + 0.01)
            out.append(v)
        return f32_below_one(np.stack(out))

    # "edges": filler query i is the i-th query that is not a family's
    db, q = filler_rows(N, NQ - 4), np.zeros((NQ, pa.DIM), np.float32)
    others = [i for i in range(NQ) if i not in QUERY_POS]
    q[others] = f32_below_one(fq_dirs[: len(others)])
    cells = []
    for k, (fq, rows) in enumerate(fams):
        q[QUERY_POS[k]] = fq
        for j in range(M):
            db[ROW_POS[4 * j + k]] = rows[j]
            cells.append((QUERY_POS[k], ROW_POS[4 * j + k]))
    edges = dict(db=db, q=q, cells=cells, lean=others[LEAN])

    # "chains": 2-row chains and 2-domain query chains
    nch, nqc = N // 2, NQ // 2
    cdb, cq = filler_rows(N, NQ - 8), np.zeros((NQ, pa.DIM), np.float32)
    cothers = [i for i in range(NQ) if i // 2 not in QCHAIN_POS]
    cq[cothers] = f32_below_one(fq_dirs[: len(cothers)])
    sec = f32_below_one(second)
    ccells, pairs = [], []
    for k, (fq, rows) in enumerate(fams):
        g = QCHAIN_POS[k]
        cq[2 * g], cq[2 * g + 1] = fq, sec[k]
        for j in range(M):
            c = CHAIN_POS[4 * j + k]
            cdb[2 * c], cdb[2 * c + 1] = rows[j], sec[k]
            ccells.append((2 * g, 2 * c))
            pairs.append((g, c))
    chains = dict(db=cdb, q=cq, cells=ccells, pairs=pairs, lean=cothers[LEAN], table=np.arange(0, N + 1, 2, dtype=np.int64),
                  qchain=np.stack([np.arange(0, NQ, 2), np.full(nqc, 2)], axis=1).astype(np.int32))
    return dict(edges=edges, chains=chains)


def pow2(a, k):
    """a * 2^k in fp32, refusing a result that is not exact (overflow, or bits lost below the normal range)."""
    a = np.asarray(a, np.float32)
    out = np.ldexp(a, k).astype(np.float32)
    assert np.array_equal(np.ldexp(out.astype(np.float64), -k), a.astype(np.float64)), "scaling by 2^%d is not exact" % k
    return out


def build(case, layout):
    """The inputs of `case` = (B, f, mode) in `layout` ("edges" or "chains"): dict(B, e, f, mode, db, q (raw), cells [(query, row)]:
    the family cells, lean: the query of LEAN, and for "chains" table, qchain, pairs [(g, c)]: the pair of each family cell).
    Arrays are fresh copies."""
    b, f, mode = case
    assert f in QUERY_SCALES[mode]
    b = float(np.float32(b))
    e = pa.ilogb(b)
    u = _unit_layouts()[layout]
    out = dict(u, B=b, e=e, f=f, mode=mode, layout=layout, db=pow2(u["db"], e), q=pow2(u["q"], f))
    for key in ("table", "qchain"):
        if key in out:
            out[key] = out[key].copy()
    return out


# ---- the references -------------------------------------------------------------------------------------------------------------
def exact_scores(case, qprep):
    """float32 [nq, n]: the scan's fmaf chain of every PREPARED query with every row."""
    return mc.dot_matrix(qprep, case["db"])


def query_norms(qprep):
    return np.linalg.norm(np.asarray(qprep, np.float64), axis=1)


def cuts(case, scores, qprep):
    """The values of min_score for one case, as fp32: per family cell with exact score s: s, its two fp32 neighbours, s +- E B |q| / 2
    and s +- 2 E B |q|; the global cuts 0.0, -0.0, -0.5 B |q| (the first family query's norm) and +inf; and the value at which the
    first family query's threshold comes out as zero (min_score = E B |q| (1 + 1e-5) in the prep kernel's fp32 arithmetic: below 2^-100 in
    the accumulators' domain, so nothing is proved for that query)."""
    qn = query_norms(qprep)
    out = []
    for qi, ri in case["cells"]:
        s = np.float32(scores[qi, ri])
        m = E * case["B"] * qn[qi]
        out += [s, np.nextafter(s, np.float32(np.inf)), np.nextafter(s, np.float32(-np.inf))]
        out += [np.float32(float(s) + d * m) for d in (0.5, -0.5, 2.0, -2.0)]
    q0 = case["cells"][0][0]
    out += [np.float32(0.0), np.float32(-0.0), np.float32(-0.5 * case["B"] * qn[q0]), np.float32(np.inf)]
    v = np.asarray(qprep[q0], np.float32)
    ss = np.float32(0.0)
    for x in v:                                                     # (the prep kernel's order; any order serves: see rescored_bounds)
        ss = np.float32(ss + np.float32(x * x))
    eb = np.float32(np.float32(E) * np.float32(case["B"]))
    out.append(np.float32(eb * np.float32(np.sqrt(ss) * np.float32(1.0 + 1e-5))))
    assert all(np.isfinite(c) or c == np.inf for c in out)
    return out


def edges_ref(scores, min_score):
    """{(query, row, score bits)} with score >= min_score: what ms_threshold_edges must emit (row_offset 0, no ranges)."""
    qi, ri = np.nonzero(scores >= np.float32(min_score))
    return set(zip(qi.tolist(), ri.tolist(), np.ascontiguousarray(scores[qi, ri]).view(np.uint32).tolist()))


def pairs_ref(scores, min_score):
    """Sorted [(g, c)] of the "chains" layout (query chain g = queries 2 g, 2 g + 1; chain c = rows 2 c, 2 c + 1): the cells below
    min_score and the cells that are zero count for nothing; a pair stays when both domains have a cell and the cells lie in both rows
    -- md_scan_case.scan_ref for 2 x 2 matrices, all pairs at once."""
    nz = mc.cut(scores, min_score) != 0
    nq, n = nz.shape
    nz = nz.reshape(nq // 2, 2, n // 2, 2)
    ok = nz.any(axis=3).all(axis=1) & (nz.any(axis=1).sum(axis=2) >= 2)
    return sorted(zip(*(x.tolist() for x in np.nonzero(ok))))


def served_threshold_is_zero(case, qn, min_score):
    """Queries whose threshold (min_score - E B |q| (1 + 1e-5)) may vanish: the kernel proves nothing for them (generous: 1e-4 of the margin)."""
    m = E * case["B"] * qn
    return np.abs(float(min_score) - m * (1.0 + 1e-5)) <= 1e-4 * m


def rescored_bounds(case, scores, qprep, min_score, flagged_rows=(), flagged_queries=()):
    """(lower, upper) of out_stats[0], the cells that went to the exact chain.
    lower: the cells with s >= min_score -- the filter never proves one of them (ms_threshold_edges re-scores every cell it emits; the
    chain scan is held to the upper bound alone).
    upper: an unflagged cell is left unproved only if a >= thr, i.e. (|a - s| <= E |row||q|, |row| <= B (1 + 9e-6), |q| taken 1e-5 high,
    the threshold pushed down by 2^-22 of its magnitude, fp32 roundings of the threshold's three operations) only if
        s >= min_score - 2.001 E B |q| - 2^-20 |min_score|;
    every cell of a flagged row or query is re-scored.  Derived from the prep kernel, not from what the scan returns."""
    s = scores.astype(np.float64)
    qn = query_norms(qprep)
    ms = float(min_score)
    lower = int((scores >= np.float32(min_score)).sum())
    fq = np.zeros(s.shape[0], bool)
    fq[list(flagged_queries)] = True
    fr = np.zeros(s.shape[1], bool)
    fr[list(flagged_rows)] = True
    if np.isfinite(ms):
        fq |= served_threshold_is_zero(case, qn, ms)
        open_ = s >= (ms - 2.001 * E * case["B"] * qn - 2.0 ** -20 * abs(ms))[:, None]
    else:
        open_ = np.full(s.shape, ms < 0)                            # -inf: nothing is proved; +inf: everything is
    open_ = open_ | fq[:, None] | fr[None, :]
    return lower, int(open_.sum())


def model_scores(case, qprep):
    """float64 [nq, n]: pa.a_model of every prepared query -- the approximate score with an exact matrix pipe."""
    return np.stack([pa.a_model(case["db"], qv, pa.PF_F16X1, row_norm_bound=case["B"]) for qv in np.asarray(qprep, np.float32)])


def model_rescored(case, model, qprep, min_score):
    """Cells the filter leaves to the exact chain if its scores are the model's (no flagged rows or queries)."""
    qn = query_norms(qprep)
    t = float(min_score) - E * case["B"] * qn * (1.0 + 1e-5)
    t = np.where(np.isfinite(t), t - np.abs(np.where(np.isfinite(t), t, 0.0)) * 2.0 ** -22, t)
    return int((~(model < t[:, None])).sum())


# ---- rows and queries at the flags' edges ------------------------------------------------------------------------------------
def with_row_of_norm(case, row, factor):
    """A copy of the case whose filler row `row` has norm B * factor (its direction is kept)."""
    out = dict(case, db=case["db"].copy())
    v = case["db"][row].astype(np.float64)
    out["db"][row] = (v / np.linalg.norm(v) * case["B"] * factor).astype(np.float32)
    return out


def with_lean_query_of_norm(case, exponent):
    """A copy of the (prenorm, f = 0) case whose LEAN query has norm 2^exponent (times 0.999)."""
    assert case["mode"] == "prenorm" and case["f"] == 0
    out = dict(case, q=case["q"].copy())
    out["q"][case["lean"]] = pow2(case["q"][case["lean"]], exponent)
    return out
