"""ms_md_chain_scan on the GPU against its restatement (md_scan_case.scan_ref: multidom_case.dot_matrix, cut and match_counts on
one matrix per (query chain, target chain)) and against ms_md_chain_scores given every pair as a candidate.  The queries of the
restatement are prepared by the scan's normalisation (ops.l2_normalize_rows with the mode's eps), which
test_multidom_gpu.py::test_cells_equal_the_scores_of_ip_topk_bit_for_bit anchors to the product's own scan."""
import ctypes

import numpy as np
import pytest

import md_scan_case as sc
import multidom_case as mc

pytestmark = pytest.mark.gpu
NINF = -np.inf
MODES = ("prenorm", "normq", "unit")
CANARY = -7777
TAIL = 16                              # canary pairs behind slot cap


def _mode_code(mode):
    from merizo_search_amd import _lib
    return {"prenorm": _lib.MODE_IP_PRENORM, "normq": _lib.MODE_IP_NORMQ, "unit": _lib.MODE_COSINE_UNIT}[mode]


def _prepared(q, mode):
    """The queries as the scan of the mode multiplies them."""
    import torch
    from merizo_search_amd import ops
    if mode == "prenorm":
        return np.array(q, np.float32)
    return ops.l2_normalize_rows(torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda(), 1e-12 if mode == "normq" else 1e-8).cpu().numpy()


def _t(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _gpu(db, table, q, mode, qchain, min_score, cap=4096, lengths=None, qlen=None, mincov=0.0, workspace=None, want_ws=False):
    """One call with `cap` slots and TAIL canary pairs behind them -> (count, the written pairs as a list of tuples, qstatus),
    after checking the canaries."""
    import torch
    from merizo_search_amd import ops
    qchain = np.asarray(qchain, np.int32).reshape(-1, 2)
    pairs = torch.full((cap + TAIL, 2), CANARY, dtype=torch.int64, device="cuda")
    count = torch.full((1,), CANARY, dtype=torch.int64, device="cuda")
    status = torch.full((max(len(qchain), 1),), CANARY, dtype=torch.int32, device="cuda")
    ws = ops.md_chain_scan_launch(_t(db, np.float32), _t(table, np.int64), _t(q, np.float32), _mode_code(mode), _t(qchain, np.int32),
                                  float(min_score), pairs, count, status, cap=cap, lengths=None if lengths is None else _t(lengths, np.float32),
                                  qlen=None if qlen is None else _t(qlen, np.float32), mincov=mincov, workspace=workspace)
    torch.cuda.synchronize()
    found, p = int(count.item()), pairs.cpu().numpy()
    written = max(0, min(found, cap))
    assert (p[written:] == CANARY).all(), "a slot at or behind min(count, cap) was written"
    out = (found, [tuple(int(x) for x in r) for r in p[:written]], status.cpu().numpy()[: len(qchain)].tolist())
    return out + (ws,) if want_ws else out


def _check(db, table, q, mode, qchain, min_score, lengths=None, qlen=None, mincov=0.0, tally=None):
    found, got, status = _gpu(db, table, q, mode, qchain, min_score, lengths=lengths, qlen=qlen, mincov=mincov)
    want, want_status = sc.scan_ref(db, _prepared(q, mode), table, qchain, min_score, lengths, qlen, mincov, tally=tally)
    assert status == want_status
    assert found == len(want) and len(set(got)) == len(got)
    assert sorted(got) == want, (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    return want


@pytest.fixture(scope="module")
def fixed():
    return sc.fixed_layout()


# ------------------------------------------------------------------ 1. the fixed layout ---
@pytest.mark.parametrize("mode", MODES)
def test_fixed_layout_equals_the_restatement_and_the_score_matrices(fixed, mode):
    """697 rows in chains of 1, 2, 3, 63, 64, 65, 130, 1, ... (md_scan_case.fixed_layout), query chains of 2, 3, 5, 8 and 64
    domains and one of 131 (more domains than any target chain has rows, and more than the entry point serves: status -1, no
    pair).  The set of pairs equals the restatement's and the pairs ms_md_chain_scores keeps (out_match == {nqd, >= nqd}) when
    it is given every (query chain, target chain) pair as a candidate.  MS_MODE_COSINE_UNIT: one length masks a planted match."""
    import torch
    from merizo_search_amd import ops
    db, table, q, qchain = fixed["db"], fixed["table"], fixed["q"], fixed["qchain"]
    extra = {}
    if mode == "unit":
        lengths = np.full(fixed["n"], 40, np.float32)
        lengths[fixed["masked"][0]] = 100
        extra = dict(lengths=lengths, qlen=np.full(len(q), 40, np.float32), mincov=0.7)
    want = _check(db, table, q, mode, qchain, sc.MINCOS, **extra)
    masked = fixed["masked"][1:]
    for pair, ok in fixed["expect"].items():
        assert (pair in want) == (ok and not (mode == "unit" and pair == masked)), pair
    assert not any(g == 6 for g, _c in want)
    # every served pair as a candidate of ms_md_chain_scores
    nchains = len(table) - 1
    cand, keys = [], []
    for g, (q0, nqd) in enumerate(qchain[:6]):
        for c in range(nchains):
            cand.append((q0, nqd, int(table[c]), int(table[c + 1] - table[c])))
            keys.append((g, c))
    cand = np.asarray(cand, np.int32)
    off = np.concatenate([[0], np.cumsum(cand[:, 1].astype(np.int64) * cand[:, 3])])[:-1]
    kw = {k: (_t(v, np.float32) if k != "mincov" else v) for k, v in extra.items()}
    _s, match = ops.md_chain_scores(_t(db, np.float32), _t(q, np.float32), _mode_code(mode), cand, np.arange(fixed["n"]), off, float(sc.MINCOS), **kw)
    match = match.cpu().numpy()
    kept = sorted(k for k, m, cd in zip(keys, match, cand) if m[0] == cd[1] and m[1] >= cd[1])
    assert kept == want


# ------------------------------------------------------------------ 2. the cut ---
def test_cut_edges_nan_rows_negative_zero_and_no_cut():
    """min_score equal to the float32 score of the one cell a pair depends on keeps the pair, one ulp above loses it.  A NaN row
    counts for nothing, a masked negative cosine is -0.0 and counts as zero, min_score = -inf cuts nothing."""
    import torch
    from merizo_search_amd import ops
    rng = np.random.default_rng(3)
    q = sc.unit(rng.standard_normal((2, 128)))
    db = sc.unit(np.stack([q[0], sc.noisy(q[1], rng),                                  # chain 0: depends on cell (1, 1)
                           sc.noisy(q[0], rng), np.full(128, np.nan), sc.noisy(q[1], rng),   # chain 1: a NaN row between two copies
                           sc.noisy(q[0], rng), np.full(128, np.nan),                  # chain 2: the NaN row is the only partner
                           sc.noisy(q[0], rng), -q[1]]))                               # chain 3: the second domain scores -1
    table, qchain = [0, 2, 5, 7, 9], [(0, 2)]
    cand, off = np.asarray([(0, 2, 0, 2)], np.int32), np.zeros(1, np.int64)
    s, _m = ops.md_chain_scores(_t(db, np.float32), _t(q, np.float32), _mode_code("prenorm"), cand, np.arange(2), off, NINF)
    cell = np.float32(s.cpu().numpy().reshape(2, 2)[1, 1])
    assert 0.9 < cell < 1.0
    assert _check(db, table, q, "prenorm", qchain, cell) == [(0, 0), (0, 1)]
    assert _check(db, table, q, "prenorm", qchain, np.nextafter(cell, np.float32(2))) == [(0, 1)]
    assert _check(db, table, q, "prenorm", qchain, np.nextafter(cell, np.float32(0))) == [(0, 0), (0, 1)]
    assert _check(db, table, q, "prenorm", qchain, sc.MINCOS) == [(0, 0), (0, 1)]
    # no cut: every non-zero cell counts, the NaN row still counts for nothing (chain 2 has one usable column)
    assert _check(db, table, q, "prenorm", qchain, NINF) == [(0, 0), (0, 1), (0, 3)]
    # MS_MODE_COSINE_UNIT: the -1 of chain 3 masked (qlen 10 < 100 * 0.7) is -0.0: zero even without a cut; unmasked it counts
    lengths, qlen = np.full(9, 10, np.float32), np.full(2, 10, np.float32)
    assert _check(db, table, q, "unit", qchain, NINF, lengths=lengths, qlen=qlen, mincov=0.7) == [(0, 0), (0, 1), (0, 3)]
    lengths[8] = 100
    assert _check(db, table, q, "unit", qchain, NINF, lengths=lengths, qlen=qlen, mincov=0.7) == [(0, 0), (0, 1)]


# ------------------------------------------------------------------ 3. capacity ---
def test_capacity_counts_everything_and_writes_nothing_behind_cap(fixed):
    """cap = 0, 1, count - 1, count, count + 7: out_count is the same, the first min(count, cap) slots hold distinct qualifying
    pairs, the canaries behind them stay.  Two calls in a row on ONE workspace both come out right."""
    db, table, q, qchain = fixed["db"], fixed["table"], fixed["q"], fixed["qchain"]
    want, _st = sc.scan_ref(db, _prepared(q, "normq"), table, qchain, sc.MINCOS)
    count = len(want)
    assert count >= 8
    ws = None
    for cap in (0, 1, count - 1, count, count + 7, count):
        found, got, _status, ws = _gpu(db, table, q, "normq", qchain, sc.MINCOS, cap=cap, workspace=ws, want_ws=True)
        assert found == count and len(got) == min(count, cap) and len(set(got)) == len(got) and set(got) <= set(want), cap
        if cap >= count:
            assert sorted(got) == want


# ------------------------------------------------------------------ 4. descriptors, arguments ---
def test_query_chain_descriptors(fixed):
    """nqd = 0, 65, and q0 + nqd > nq (also negative values) give status -1 and no pair; nqd = 64 is served."""
    db, table, q = fixed["db"], fixed["table"], fixed["q"]
    nq = len(q)
    qchain = [(0, 0), (0, 65), (nq - 1, 2), (-1, 2), (0, -3), (2147483647, 2), tuple(fixed["qchain"][4]), (0, 2), (nq - 2, 2)]
    found, got, status = _gpu(db, table, q, "prenorm", qchain, sc.MINCOS)
    assert status == [-1, -1, -1, -1, -1, -1, 0, 0, 0]
    want, want_status = sc.scan_ref(db, q, table, qchain, sc.MINCOS)
    assert status == want_status and sorted(got) == want and found == len(want)
    assert {g for g, _c in got} == {6, 7} and (6, 4) in got and (6, 5) in got


def test_a_chain_table_that_breaks_its_rules_is_refused_without_reading_rows(fixed):
    """The table is validated on the device: count -1, no pair, for a table that does not start at 0, does not end at n, repeats
    a start, descends, or names rows far outside the matrix.  The wrapper raises."""
    from merizo_search_amd import _lib, ops
    db, q, qchain = fixed["db"][:100], fixed["q"], fixed["qchain"][:2]
    for table in ([1, 50, 100], [0, 50, 99], [0, 50, 101], [0, 50, 50, 100], [0, 60, 50, 100], [0, 1 << 40, 100], [0, -(1 << 40), 100],
                  [0, 50, 1 << 62], list(range(0, 202))):
        found, got, _status = _gpu(db, table, q, "prenorm", qchain, sc.MINCOS)
        assert found == -1 and got == [], table
    with pytest.raises(_lib.MerizoHipError):
        ops.md_chain_scan(_t(db, np.float32), [0, 50, 50, 100], _t(q, np.float32), _lib.MODE_IP_PRENORM, qchain, 0.5)
    _check(db, [0, 50, 100], q, "prenorm", qchain, sc.MINCOS)            # the workspace's status word does not outlive a call


def test_return_codes_and_empty_inputs():
    import torch
    from merizo_search_amd import _lib
    lib = _lib.load()
    d, q = torch.zeros((20, 128), device="cuda"), torch.ones((4, 128), device="cuda")
    table, qchain = _t([0, 10, 20], np.int64), _t([(0, 2)], np.int32)
    pairs = torch.full((8, 2), CANARY, dtype=torch.int64, device="cuda")
    count, status = torch.full((1,), CANARY, dtype=torch.int64, device="cuda"), torch.full((1,), CANARY, dtype=torch.int32, device="cuda")
    need = int(lib.ms_md_chain_scan_workspace_bytes(20, 4))
    assert need >= 4 * 512 and int(lib.ms_md_chain_scan_workspace_bytes(20, 0)) == 0 and int(lib.ms_md_chain_scan_workspace_bytes(-1, 4)) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")

    def call(**kw):
        a = dict(db=d.data_ptr(), n=20, table=table.data_ptr(), nchains=2, q=q.data_ptr(), nq=4, mode=_lib.MODE_IP_PRENORM, lengths=None,
                 qlen=None, qchain=qchain.data_ptr(), nqc=1, min_score=0.5, pairs=pairs.data_ptr(), cap=8, count=count.data_ptr(),
                 status=status.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
        a.update(kw)
        rc = lib.ms_md_chain_scan(a["db"], a["n"], a["table"], a["nchains"], a["q"], a["nq"], a["mode"], a["lengths"], a["qlen"],
                                  ctypes.c_float(0.0), a["qchain"], a["nqc"], ctypes.c_float(a["min_score"]), a["pairs"], a["cap"],
                                  a["count"], a["status"], a["ws"], a["ws_bytes"], None)
        torch.cuda.synchronize()
        return rc

    assert call() == 0 and int(count.item()) == 0 and int(status.item()) == 0
    for kw in (dict(q=None), dict(count=None), dict(ws=None), dict(db=None), dict(table=None), dict(qchain=None), dict(status=None),
               dict(pairs=None), dict(nq=0), dict(min_score=float("nan")), dict(mode=_lib.MODE_COSINE_RAW), dict(mode=17),
               dict(db=d.data_ptr() + 4), dict(ws=ws.data_ptr() + 8), dict(lengths=d.data_ptr()), dict(n=-1), dict(cap=-1)):
        assert call(**kw) == -1 and b"ms_md_chain_scan" in lib.ms_last_error(), kw
    assert call(ws_bytes=need - 1) == -2 and b"workspace" in lib.ms_last_error()
    assert call(pairs=None, cap=0) == 0                                   # cap = 0 only counts: no slot array needed
    for kw in (dict(nqc=0), dict(nchains=0), dict(nqc=0, qchain=None, status=None), dict(nchains=0, table=None), dict(n=0, db=None)):
        count.fill_(CANARY)
        assert call(**kw) == 0 and int(count.item()) == 0, kw
    assert (pairs.cpu().numpy() == CANARY).all()


# ------------------------------------------------------------------ 5. seeded random shapes ---
def test_seeded_random_shapes_equal_the_restatement():
    """150 shapes (md_scan_case.random_case): n in [1, 3000], chain lengths from {1..5, 63, 64, 65, 129, 200}, 1..6 query chains of
    1..8 domains, planted copies; the mode cycles.  Over the run at least 50 pairs qualify, 50 fail on the row condition alone
    and 20 on the column condition alone (on the CPU the restatement counts 955, 306 and 92)."""
    tally = {}
    for seed in range(150):
        case = sc.random_case(seed)
        mode = MODES[seed % 3]
        extra = {}
        if mode == "unit":
            rng = np.random.default_rng(seed)
            extra = dict(lengths=rng.choice([40, 57, 58, 80], case["n"]).astype(np.float32),
                         qlen=rng.choice([40, 56], len(case["q"])).astype(np.float32), mincov=0.7)
        _check(case["db"], case["table"], case["q"], mode, case["qchain"], sc.MINCOS, tally=tally, **extra)
    assert tally.get("qualify", 0) >= 50 and tally.get("rows", 0) >= 50 and tally.get("cols", 0) >= 20, tally


# ------------------------------------------------------------------ 6. repeatability ---
def test_twenty_repeats_give_identical_sorted_output():
    from merizo_search_amd import _lib, ops
    case = sc.random_case(7)
    db, q = _t(case["db"], np.float32), _t(case["q"], np.float32)
    runs = [ops.md_chain_scan(db, case["table"], q, _lib.MODE_IP_NORMQ, case["qchain"], float(sc.MINCOS), cap=c) for c in [4096, 1] * 10]
    assert len(runs[0][0]) > 0
    for pairs, status in runs[1:]:
        assert np.array_equal(pairs, runs[0][0]) and np.array_equal(status, runs[0][1])
    want, _st = sc.scan_ref(case["db"], _prepared(case["q"], "normq"), case["table"], case["qchain"], sc.MINCOS)
    assert [tuple(p) for p in runs[0][0].tolist()] == want
