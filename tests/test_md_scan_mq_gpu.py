"""ms_md_chain_scan_mq (route "matrix" of ops.md_chain_scan: the fp16 matrix pipe in front of the exact cell) on the
GPU against the restatement md_scan_case.scan_ref and against route "lane" (ms_md_chain_scan).  Sets of pairs, counts and statuses
are compared exactly: the prefilter only ever proves a cell zero, so there is no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import md_scan_case as sc
import multidom_case as mc
import pf_adversarial as pa
from mq_filter_case import mode_code as _mode_code, prepared as _prepared, to_gpu as _t

pytestmark = pytest.mark.gpu
NINF = -np.inf
MODES = ("prenorm", "normq", "unit")
CANARY = -7777
TAIL = 16
BOUND = 1.0 + 1e-6                     # the row-norm bound the drivers give for unit rows
E = 1.05e-3                            # ms_pf_err_coef(MS_PF_F16X1)


def _gpu(db, table, q, mode, qchain, min_score, cap=8192, lengths=None, qlen=None, mincov=0.0, workspace=None, route="matrix", bound=BOUND):
    """One call with `cap` slots and TAIL canary pairs behind them -> dict(count, pairs, status, rescored, ws)."""
    import torch
    from merizo_search_amd import ops
    qchain = np.asarray(qchain, np.int32).reshape(-1, 2)
    pairs = torch.full((cap + TAIL, 2), CANARY, dtype=torch.int64, device="cuda")
    count = torch.full((1,), CANARY, dtype=torch.int64, device="cuda")
    stats = torch.full((1,), CANARY, dtype=torch.int64, device="cuda")
    status = torch.full((max(len(qchain), 1),), CANARY, dtype=torch.int32, device="cuda")
    kw = dict(route="matrix", row_norm_bound=bound, out_stats=stats) if route == "matrix" else {}
    ws = ops.md_chain_scan_launch(_t(db, np.float32), _t(table, np.int64), _t(q, np.float32), _mode_code(mode), _t(qchain, np.int32),
                                  float(min_score), pairs, count, status, cap=cap, lengths=None if lengths is None else _t(lengths, np.float32),
                                  qlen=None if qlen is None else _t(qlen, np.float32), mincov=mincov, workspace=workspace, **kw)
    torch.cuda.synchronize()
    found, p = int(count.item()), pairs.cpu().numpy()
    written = max(0, min(found, cap))
    assert (p[written:] == CANARY).all(), "a slot at or behind min(count, cap) was written"
    return dict(count=found, pairs=[tuple(int(x) for x in r) for r in p[:written]], status=status.cpu().numpy()[: len(qchain)].tolist(),
                rescored=int(stats.item()), ws=ws)


def _check(db, table, q, mode, qchain, min_score, lengths=None, qlen=None, mincov=0.0, bound=BOUND, lane=True):
    """Route "matrix" == the restatement == route "lane".  -> (the pairs, the matrix route's result)."""
    kw = dict(lengths=lengths, qlen=qlen, mincov=mincov)
    got = _gpu(db, table, q, mode, qchain, min_score, bound=bound, **kw)
    want, want_status = sc.scan_ref(db, _prepared(q, mode), table, qchain, min_score, lengths, qlen, mincov)
    assert got["status"] == want_status
    assert got["count"] == len(want) and len(set(got["pairs"])) == len(got["pairs"])
    assert sorted(got["pairs"]) == want, (sorted(set(got["pairs"]) - set(want))[:5], sorted(set(want) - set(got["pairs"]))[:5])
    if lane:
        ref = _gpu(db, table, q, mode, qchain, min_score, route="lane", **kw)
        assert ref["count"] == got["count"] and sorted(ref["pairs"]) == want and ref["status"] == got["status"]
    return want, got


@pytest.fixture(scope="module")
def fixed():
    return sc.fixed_layout()


# ------------------------------------------------------------------ 1. the fixed layout ---
@pytest.mark.parametrize("mode", MODES)
def test_fixed_layout_equals_the_restatement_and_the_lane_route(fixed, mode):
    """md_scan_case.fixed_layout: 215 queries are 7 query tiles of 32 and the 64-domain chain spans three of them; the 130-row
    chains carry plants on both sides of a 64-row piece boundary; the twin domains fail on the column condition alone; one
    descriptor is not served.  MS_MODE_COSINE_UNIT: with the length that masks a planted match away."""
    db, table, q, qchain = fixed["db"], fixed["table"], fixed["q"], fixed["qchain"]
    assert len(q) == 215
    extra = {}
    if mode == "unit":
        lengths = np.full(fixed["n"], 40, np.float32)
        lengths[fixed["masked"][0]] = 100
        extra = dict(lengths=lengths, qlen=np.full(len(q), 40, np.float32), mincov=0.7)
    want, _got = _check(db, table, q, mode, qchain, sc.MINCOS, **extra)
    masked = fixed["masked"][1:]
    for pair, ok in fixed["expect"].items():
        assert (pair in want) == (ok and not (mode == "unit" and pair == masked)), pair
    assert not any(g == 6 for g, _c in want)


# ------------------------------------------------------------------ 2. the cut ---
def test_cut_edges_nan_rows_negative_zero_and_no_cut_on_the_matrix_route():
    """The case of test_md_scan_gpu.py's cut test: min_score equal to the cell a pair depends on, one ulp above and below; a NaN
    row (flagged: exact) counts for nothing; a masked negative cosine is -0.0; min_score = -inf proves nothing and is right."""
    from merizo_search_amd import ops
    rng = np.random.default_rng(3)
    q = sc.unit(rng.standard_normal((2, 128)))
    db = sc.unit(np.stack([q[0], sc.noisy(q[1], rng),
                           sc.noisy(q[0], rng), np.full(128, np.nan), sc.noisy(q[1], rng),
                           sc.noisy(q[0], rng), np.full(128, np.nan),
                           sc.noisy(q[0], rng), -q[1]]))
    table, qchain = [0, 2, 5, 7, 9], [(0, 2)]
    cand, off = np.asarray([(0, 2, 0, 2)], np.int32), np.zeros(1, np.int64)
    s, _m = ops.md_chain_scores(_t(db, np.float32), _t(q, np.float32), _mode_code("prenorm"), cand, np.arange(2), off, NINF)
    cell = np.float32(s.cpu().numpy().reshape(2, 2)[1, 1])
    assert 0.9 < cell < 1.0
    assert _check(db, table, q, "prenorm", qchain, cell)[0] == [(0, 0), (0, 1)]
    assert _check(db, table, q, "prenorm", qchain, np.nextafter(cell, np.float32(2)))[0] == [(0, 1)]
    assert _check(db, table, q, "prenorm", qchain, np.nextafter(cell, np.float32(0)))[0] == [(0, 0), (0, 1)]
    assert _check(db, table, q, "prenorm", qchain, sc.MINCOS)[0] == [(0, 0), (0, 1)]
    want, got = _check(db, table, q, "prenorm", qchain, NINF)
    assert want == [(0, 0), (0, 1), (0, 3)] and got["rescored"] == 2 * 9          # no cut: every cell is re-scored
    lengths, qlen = np.full(9, 10, np.float32), np.full(2, 10, np.float32)
    assert _check(db, table, q, "unit", qchain, NINF, lengths=lengths, qlen=qlen, mincov=0.7)[0] == [(0, 0), (0, 1), (0, 3)]
    lengths[8] = 100
    assert _check(db, table, q, "unit", qchain, NINF, lengths=lengths, qlen=qlen, mincov=0.7)[0] == [(0, 0), (0, 1)]


# ------------------------------------------------------------------ 3. near the threshold ---
def test_cells_whose_approximate_score_is_on_the_wrong_side_of_the_threshold():
    """Where a prefilter goes wrong.  pf_adversarial's rows and queries for the F16X1 terms (rows that round down, rows that round
    up, the query's own rounding) as the first domain of 2-domain query chains and the first row of 2-row target chains; the second
    domain is an unrelated unit vector and its own copy, so a pair qualifies iff the cell (first domain, first row) with exact
    score s stays.  min_score runs over s, its two neighbours, s +- E / 2 and s +- 2 E for every such cell.  The numpy model of the
    approximate score (pa.a_model) puts at least a dozen of the cells on the other side of min_score from s (107 as the seeds stand)."""
    rng = np.random.default_rng(11)
    m = 3
    fams = [pa.f16_row_rounding(21, m, side=-1), pa.f16_row_rounding(22, m, side=+1), pa.f16x1_query_rounding(23, m)]
    second = sc.unit(rng.standard_normal((len(fams), 128)))
    q = np.concatenate([np.stack([fq, second[f]]) for f, (fq, _rows) in enumerate(fams)]).astype(np.float32)
    qchain = [(2 * f, 2) for f in range(len(fams))]
    rows, owner = [], []
    for f, (_fq, frows) in enumerate(fams):
        for row in frows:
            rows += [row, second[f]]
            owner.append(f)
    db = np.asarray(rows, np.float32)
    table = sc.table_of([2] * len(owner))
    exact = mc.dot_matrix(q, db)
    model = np.stack([pa.a_model(db, qv, pa.PF_F16X1, row_norm_bound=BOUND) for qv in q])
    assert np.abs(model - exact.astype(np.float64)).max() < E * 1.001                # (the model obeys the bound on these rows)
    wrong_side = 0
    for c, f in enumerate(owner):
        s = exact[2 * f, 2 * c]
        assert 0.9 < s < 1.0
        e32 = np.float32(E)
        for ms in (s, np.nextafter(s, np.float32(2)), np.nextafter(s, np.float32(0)), s + e32 / 2, s - e32 / 2, s + 2 * e32, s - 2 * e32):
            ms = np.float32(ms)
            want, _got = _check(db, table, q, "prenorm", qchain, ms, lane=False)
            assert ((f, c) in want) == bool(s >= ms)
            first_rows = exact[0::2, 0::2], model[0::2, 0::2]
            wrong_side += int(((first_rows[0] >= ms) != (first_rows[1] >= ms)).sum())
    assert wrong_side >= 12, wrong_side


# ------------------------------------------------------------------ 4. flagged inputs ---
@pytest.mark.parametrize("bad_row", ["norm3", "inf", "nan"])
@pytest.mark.parametrize("partner_matches", [True, False])
def test_flagged_rows_take_the_exact_path(bad_row, partner_matches):
    """A row of norm 3 under a bound of 1 + 1e-6 (its scores are three times a unit row's), a row with an inf element, a NaN row:
    every cell of such a row is re-scored exactly, in a chain that qualifies or fails on its partner."""
    rng = np.random.default_rng(5)
    q = sc.unit(rng.standard_normal((4, 128)))
    db = sc.unit(rng.standard_normal((70, 128)))
    table = sc.table_of([2] * 35)
    qchain = [(0, 2), (2, 2)]
    special = 3.0 * sc.unit(sc.noisy(q[0], rng)) if bad_row == "norm3" else sc.unit(sc.noisy(q[0], rng)).copy()
    if bad_row == "inf":
        special[0] = np.copysign(np.float32(np.inf), q[0, 0])               # the product is +inf: so is the score
    if bad_row == "nan":
        special[5] = np.nan
    db[40] = special
    db[41] = sc.unit(sc.noisy(q[1], rng)) if partner_matches else db[41]
    db[10], db[11] = 0.2 * q[2], sc.unit(sc.noisy(q[3], rng))               # a SHORT row: 0.2 < 0.5, no match whatever the bound
    want, got = _check(db, table, q, "prenorm", qchain, sc.MINCOS)
    assert ((0, 20) in want) == (partner_matches and bad_row != "nan")
    assert (1, 5) not in want
    assert got["rescored"] >= 4                                             # the flagged row against all four queries


@pytest.mark.parametrize("bad_query", ["inf", "zero", "huge"])
def test_flagged_queries_take_the_exact_path(bad_query):
    """A query with an inf element (prenorm: used as given), a zero query, a query of norm 2^50: every cell of such a query is
    re-scored exactly; the other query chain is filtered as usual."""
    rng = np.random.default_rng(6)
    q = sc.unit(rng.standard_normal((4, 128)))
    db = sc.unit(rng.standard_normal((130, 128)))
    table = sc.table_of([2] * 65)
    db[20], db[21] = sc.noisy(q[0], rng), sc.noisy(q[1], rng)
    db[100], db[101] = sc.noisy(q[2], rng), sc.noisy(q[3], rng)
    db = sc.unit(db)
    if bad_query == "inf":
        q[0, 3] = np.inf
    elif bad_query == "zero":
        q[0] = 0.0
    else:
        q[0] *= np.float32(2.0 ** 50)
    want, got = _check(db, table, q, "prenorm", [(0, 2), (2, 2)], sc.MINCOS)
    assert (1, 50) in want
    assert bad_query == "inf" or ((0, 10) in want) == (bad_query == "huge")
    assert 130 <= got["rescored"] < 130 + 3 * 130 // 10


# ------------------------------------------------------------------ 5. out_stats ---
def test_rescored_lies_between_its_two_bounds(fixed):
    """3,000 random unit rows in chains of 1-5 with the fixed layout's planted rows against its 215 queries at 0.5: the cells
    re-scored are at least the non-zero cells inside qualifying pairs and at most the cells whose exact score is >= min_score -
    2 E B |q| plus the cells of flagged rows and queries (none here); that is a small fraction of all cells."""
    rng = np.random.default_rng(8)
    lens = []
    while sum(lens) < 3000:
        lens.append(min(int(rng.integers(1, 6)), 3000 - sum(lens)))
    table = sc.table_of(lens)
    db = sc.unit(rng.standard_normal((3000, 128)))
    q, qchain = fixed["q"], fixed["qchain"]
    starts = table[:-1]
    for g, (q0, nqd) in enumerate(qchain[:4]):                               # plant every domain of four query chains somewhere
        c = int(np.flatnonzero(np.diff(table) >= min(nqd, 5))[10 + 20 * g])
        for i in range(min(nqd, int(table[c + 1] - table[c]))):
            db[starts[c] + i] = sc.unit(sc.noisy(q[q0 + i], rng))
    want, got = _check(db, table, q, "prenorm", qchain, sc.MINCOS)
    s = mc.dot_matrix(q, db)
    qn = np.linalg.norm(q.astype(np.float64), axis=1)
    lower = 0
    for g, c in want:
        q0, nqd = qchain[g]
        lower += int((mc.cut(s[q0: q0 + nqd, table[c]: table[c + 1]], sc.MINCOS) != 0).sum())
    upper = int((s.astype(np.float64) >= float(sc.MINCOS) - 2 * E * BOUND * qn[:, None]).sum())
    assert len(want) >= 2 and 0 < lower <= got["rescored"] <= upper, (lower, got["rescored"], upper)
    assert upper < s.size // 1000


# ------------------------------------------------------------------ 6. row-count edges ---
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_row_count_edges(n):
    rng = np.random.default_rng(n)
    q = sc.unit(rng.standard_normal((40, 128)))
    qchain = [(0, 1), (1, 2), (3, 3), (6, 34)]
    db = sc.unit(rng.standard_normal((n, 128)))
    lens = [1] * n if n < 63 else [2] * (n // 2) + [1] * (n % 2)
    table = sc.table_of(lens)
    db[0] = sc.noisy(q[0], rng)
    if n >= 63:
        db[n - 2 - n % 2], db[n - 1 - n % 2] = sc.noisy(q[1], rng), sc.noisy(q[2], rng)
    want, _got = _check(sc.unit(db), table, q, "normq", qchain, sc.MINCOS)
    assert (0, 0) in want and ((1, n // 2 - 1) in want) == (n >= 63)


def test_a_chain_that_starts_at_row_255_and_runs_into_the_next_range():
    rng = np.random.default_rng(1)
    q = sc.unit(rng.standard_normal((5, 128)))
    db = sc.unit(rng.standard_normal((600, 128)))
    table = sc.table_of([255, 70, 3, 272])
    db[255], db[324] = sc.noisy(q[0], rng), sc.noisy(q[1], rng)             # first and last row of the chain that crosses row 256
    db[100], db[254] = sc.noisy(q[2], rng), sc.noisy(q[3], rng)
    db[326], db[327] = sc.noisy(q[0], rng), sc.noisy(q[1], rng)
    want, _got = _check(sc.unit(db), table, q, "prenorm", [(0, 2), (2, 2), (3, 2)], sc.MINCOS)
    assert want == [(0, 1), (0, 2), (1, 0)]


def test_one_chain_of_200_rows_with_more_than_64_query_chains():
    rng = np.random.default_rng(2)
    q = sc.unit(rng.standard_normal((160, 128)))
    qchain = [(2 * g, 2) for g in range(80)]
    db = sc.unit(rng.standard_normal((200, 128)))
    for g, (a, b) in {0: (0, 199), 65: (63, 64), 70: (128, 5), 79: (100, 100)}.items():      # 79: both domains on one row
        db[a] = sc.noisy(q[2 * g], rng)
        if b != a:
            db[b] = sc.noisy(q[2 * g + 1], rng)
    q[159] = sc.noisy(q[158], rng)
    want, _got = _check(sc.unit(db), [0, 200], sc.unit(q), "prenorm", qchain, sc.MINCOS)
    assert want == [(0, 0), (65, 0), (70, 0)]


# ------------------------------------------------------------------ 7. parity shapes ---
@pytest.mark.parametrize("seed", range(12))
def test_random_cases_as_they_are(seed):
    case = sc.random_case(seed)
    mode = MODES[seed % 3]
    extra = {}
    if mode == "unit":
        rng = np.random.default_rng(seed)
        extra = dict(lengths=rng.choice([40, 57, 58, 80], case["n"]).astype(np.float32),
                     qlen=rng.choice([40, 56], len(case["q"])).astype(np.float32), mincov=0.7)
    _check(case["db"], case["table"], case["q"], mode, case["qchain"], sc.MINCOS, **extra)


@pytest.mark.parametrize("seed", range(4))
def test_many_query_chains(seed):
    """33-200 queries in up to 80 query chains of 1-5 domains over chains of 1-5, 64, 65 and 130 rows, with planted relatives."""
    rng = np.random.default_rng(500 + seed)
    nqds = []
    target = int(rng.integers(33, 201))
    while sum(nqds) < target and len(nqds) < 80:
        nqds.append(min(int(rng.integers(1, 6)), target - sum(nqds)))
    starts = np.concatenate([[0], np.cumsum(nqds)])
    q = sc.unit(rng.standard_normal((int(starts[-1]), 128)))
    lens = [int(x) for x in rng.choice([1, 2, 3, 4, 5, 64, 65, 130], size=120, p=[.2, .2, .2, .15, .15, .04, .03, .03])]
    table = sc.table_of(lens)
    db = rng.standard_normal((int(table[-1]), 128)).astype(np.float32)
    for g, nqd in enumerate(nqds):
        fit = [c for c in range(len(lens)) if lens[c] >= nqd]
        for c in rng.choice(fit, size=2, replace=False):
            doms = list(range(nqd)) if rng.random() < 0.7 else list(range(nqd - 1))
            offs = rng.choice(lens[c], size=len(doms), replace=False)
            for off, d in zip(offs, doms):
                db[table[c] + off] = sc.noisy(q[starts[g] + d], rng)
    qchain = [(int(starts[g]), nqd) for g, nqd in enumerate(nqds)]
    want, _got = _check(sc.unit(db), table, q, MODES[seed % 2], qchain, sc.MINCOS)
    assert len(want) >= 5


def test_more_queries_than_a_block_and_more_query_chains_than_a_window():
    """4,300 queries are two query blocks of the kernel (a query chain belongs to the block its first row falls into and may end
    behind the block's 4,096th query); 4,200 descriptors are two windows of a long chain's state.  The descriptors point at a few
    planted query rows, out of order and more than once."""
    rng = np.random.default_rng(9)
    nq = 4300
    q = sc.unit(rng.standard_normal((nq, 128)))
    lens = [3, 150, 2, 64, 5, 70]
    table = sc.table_of(lens)
    db = sc.unit(rng.standard_normal((int(table[-1]), 128)))
    planted = {4090: (1, [0, 149, 75, 64, 63, 3, 2, 140, 9, 10]),            # 10 domains across the block boundary, in the 150-row chain
               4200: (0, [0, 1, 2]), 4296: (5, [69, 0, 64, 1]), 10: (3, [5, 6]), 4000: (4, [0, 1, 2, 3, 4])}
    for q0, (c, offs) in planted.items():
        for i, off in enumerate(offs):
            db[table[c] + off] = sc.noisy(q[q0 + i], rng)
    db = sc.unit(db)
    served = [(4090, 10), (4200, 3), (4296, 4), (10, 2), (4000, 5), (4095, 1), (4096, 2), (4298, 3), (4299, 1)]
    qchain = np.zeros((4200, 2), np.int32)
    qchain[:] = (7, 2)                                                    # filler: an unplanted pair of domains
    where = [0, 1, 4095, 4096, 4097, 4199, 2000, 3000, 100]
    for g, d in zip(where, served):
        qchain[g] = d
    got = _gpu(db, table, q, "prenorm", qchain, sc.MINCOS)
    ref = _gpu(db, table, q, "prenorm", qchain, sc.MINCOS, route="lane")
    sub, _st = sc.scan_ref(db, q, table, [qchain[g] for g in where], sc.MINCOS)
    want = sorted((where[g], c) for g, c in sub)
    assert sorted(got["pairs"]) == sorted(ref["pairs"]) == want and got["count"] == ref["count"] == len(want)
    assert got["status"] == ref["status"] and got["status"][100] == 0 and got["status"][3000] == -1      # (4298, 3) ends behind nq
    assert {(0, 1), (1, 0), (4095, 5), (4096, 3), (4097, 4)} <= set(want)


# ------------------------------------------------------------------ 8. capacity ---
def test_capacity_counts_everything_and_writes_nothing_behind_cap(fixed):
    db, table, q, qchain = fixed["db"], fixed["table"], fixed["q"], fixed["qchain"]
    want, _st = sc.scan_ref(db, _prepared(q, "normq"), table, qchain, sc.MINCOS)
    count = len(want)
    assert count >= 8
    ws = None
    for cap in (0, 1, count - 1, count, count + 7, count):
        got = _gpu(db, table, q, "normq", qchain, sc.MINCOS, cap=cap, workspace=ws)
        ws = got["ws"]
        assert got["count"] == count and len(got["pairs"]) == min(count, cap) and set(got["pairs"]) <= set(want), cap
        assert len(set(got["pairs"])) == len(got["pairs"])
        if cap >= count:
            assert sorted(got["pairs"]) == want


# ------------------------------------------------------------------ 9. arguments ---
def test_query_chain_descriptors(fixed):
    db, table, q = fixed["db"], fixed["table"], fixed["q"]
    nq = len(q)
    qchain = [(0, 0), (0, 65), (nq - 1, 2), (-1, 2), (0, -3), (2147483647, 2), tuple(fixed["qchain"][4]), (0, 2), (nq - 2, 2)]
    want, got = _check(db, table, q, "prenorm", qchain, sc.MINCOS)
    assert got["status"] == [-1, -1, -1, -1, -1, -1, 0, 0, 0]
    assert {g for g, _c in want} == {6, 7} and (6, 4) in want and (6, 5) in want


def test_a_chain_table_that_breaks_its_rules_is_refused_without_reading_rows(fixed):
    from merizo_search_amd import _lib, ops
    db, q, qchain = fixed["db"][:100], fixed["q"], fixed["qchain"][:2]
    for table in ([1, 50, 100], [0, 50, 99], [0, 50, 101], [0, 50, 50, 100], [0, 60, 50, 100], [0, 1 << 40, 100], [0, -(1 << 40), 100],
                  [0, 50, 1 << 62], list(range(0, 202))):
        got = _gpu(db, table, q, "prenorm", qchain, sc.MINCOS)
        assert got["count"] == -1 and got["pairs"] == [] and got["rescored"] == 0, table
    with pytest.raises(_lib.MerizoHipError):
        ops.md_chain_scan(_t(db, np.float32), [0, 50, 50, 100], _t(q, np.float32), _lib.MODE_IP_PRENORM, qchain, 0.5, route="matrix",
                          row_norm_bound=BOUND)
    _check(db, [0, 50, 100], q, "prenorm", qchain, sc.MINCOS)


def test_return_codes_and_empty_inputs():
    import torch
    from merizo_search_amd import _lib
    lib = _lib.load()
    assert lib.ms_version() == 210
    d, q = torch.zeros((20, 128), device="cuda"), torch.ones((4, 128), device="cuda")
    table, qchain = _t([0, 10, 20], np.int64), _t([(0, 2)], np.int32)
    pairs = torch.full((8, 2), CANARY, dtype=torch.int64, device="cuda")
    count, status = torch.full((1,), CANARY, dtype=torch.int64, device="cuda"), torch.full((1,), CANARY, dtype=torch.int32, device="cuda")
    stats = torch.full((1,), CANARY, dtype=torch.int64, device="cuda")
    need = int(lib.ms_md_chain_scan_mq_workspace_bytes(20, 4))
    assert need >= 4 * 768 and int(lib.ms_md_chain_scan_mq_workspace_bytes(20, 0)) == 0 and int(lib.ms_md_chain_scan_mq_workspace_bytes(-1, 4)) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")

    def call(**kw):
        a = dict(db=d.data_ptr(), n=20, table=table.data_ptr(), nchains=2, q=q.data_ptr(), nq=4, mode=_lib.MODE_IP_PRENORM, lengths=None,
                 qlen=None, qchain=qchain.data_ptr(), nqc=1, min_score=0.5, pairs=pairs.data_ptr(), cap=8, count=count.data_ptr(),
                 status=status.data_ptr(), bound=BOUND, stats=stats.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
        a.update(kw)
        rc = lib.ms_md_chain_scan_mq(a["db"], a["n"], a["table"], a["nchains"], a["q"], a["nq"], a["mode"], a["lengths"], a["qlen"],
                                     ctypes.c_float(0.0), a["qchain"], a["nqc"], ctypes.c_float(a["min_score"]), a["pairs"], a["cap"],
                                     a["count"], a["status"], ctypes.c_float(a["bound"]), a["stats"], a["ws"], a["ws_bytes"], None)
        torch.cuda.synchronize()
        return rc

    assert call() == 0 and int(count.item()) == 0 and int(status.item()) == 0 and int(stats.item()) == 0
    assert call(stats=None) == 0
    for kw in (dict(q=None), dict(count=None), dict(ws=None), dict(db=None), dict(table=None), dict(qchain=None), dict(status=None),
               dict(pairs=None), dict(nq=0), dict(min_score=float("nan")), dict(mode=_lib.MODE_COSINE_RAW), dict(mode=17),
               dict(db=d.data_ptr() + 4), dict(ws=ws.data_ptr() + 8), dict(lengths=d.data_ptr()), dict(n=-1), dict(cap=-1)):
        assert call(**kw) == -1 and b"ms_md_chain_scan_mq" in lib.ms_last_error(), kw
    for bound in (float("nan"), 0.0, -1.0, 2.0 ** -41, 2.0 ** 41, float("inf")):
        assert call(bound=bound) == -4 and b"row-norm bound" in lib.ms_last_error(), bound
    assert call(bound=2.0 ** -40) == 0 and call(bound=2.0 ** 40) == 0
    assert call(ws_bytes=need - 1) == -2 and b"workspace" in lib.ms_last_error()
    assert call(pairs=None, cap=0) == 0
    for kw in (dict(nqc=0), dict(nchains=0), dict(nqc=0, qchain=None, status=None), dict(nchains=0, table=None), dict(n=0, db=None)):
        count.fill_(CANARY)
        stats.fill_(CANARY)
        assert call(**kw) == 0 and int(count.item()) == 0 and int(stats.item()) == 0, kw
    assert (pairs.cpu().numpy() == CANARY).all()


# ------------------------------------------------------------------ 10. workspace ---
def test_one_workspace_serves_two_different_calls_and_twenty_repeats_agree(fixed):
    from merizo_search_amd import _lib, ops
    big, small = sc.random_case(7), sc.random_case(3)
    import torch
    lib = _lib.load()
    need = max(int(lib.ms_md_chain_scan_mq_workspace_bytes(c["n"], len(c["q"]))) for c in (big, small, fixed))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for case in (fixed, small, big, fixed):
        got = _gpu(case["db"], case["table"], case["q"], "normq", case["qchain"], sc.MINCOS, workspace=ws)
        want, _st = sc.scan_ref(case["db"], _prepared(case["q"], "normq"), case["table"], case["qchain"], sc.MINCOS)
        assert sorted(got["pairs"]) == want and got["count"] == len(want)
    db, q = _t(big["db"], np.float32), _t(big["q"], np.float32)
    runs = [ops.md_chain_scan(db, big["table"], q, _lib.MODE_IP_NORMQ, big["qchain"], float(sc.MINCOS), cap=c, route="matrix",
                              row_norm_bound=BOUND) for c in [4096, 1] * 10]
    assert len(runs[0][0]) > 0
    for pairs, status in runs[1:]:
        assert np.array_equal(pairs, runs[0][0]) and np.array_equal(status, runs[0][1])
