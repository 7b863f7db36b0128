"""ms_ip_topk_large on the GPU: the lists of ms_ip_topk for 64 < k <= MS_LARGE_K_MAX from one filtered pass -- bits against the
oracle and against ops.ip_topk, ties, overflow and the second round, the modes and the length mask, the NaN / inf policy, shapes
the route forwards, workspace reuse, given thresholds, refusals, and the drivers with the route on and off."""
import os
import shutil

import numpy as np
import pytest

import dbquery_case as dq

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
BOUND = 1.0 + 1e-5                # |row| of rows normalised in fp32 (the engine's UNIT_ROW_BOUND)
NEVER = 1 << 62


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    from merizo_search_amd import _lib
    _lib.require_gpu()
    return torch


@pytest.fixture(autouse=True)
def _route_from_zero_rows(monkeypatch):
    from merizo_search_amd import ops
    monkeypatch.setattr(ops, "LARGE_K_MIN_ROWS", 0)
    monkeypatch.setattr(ops, "LARGE_K_TWO_SCAN_MIN_NQ", 1)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _norm_db(n, seed):
    from merizo_search_amd.foldclass import synthetic as syn
    return syn.normalized_database(n, seed)


def _same(torch, a, b):
    """(scores, idx) pairs equal bit for bit."""
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def _large(ops, db, q, k, bound=BOUND, **kw):
    st = {}
    s, i = ops.ip_topk_large(db, q, k, bound, stats=st, **kw)
    assert st["first_round"] + st["second_round"] + st["fallback"] == q.shape[0], st
    return (s, i), st


def _raw(torch, db, q, k, bound=BOUND, mode=0, lb_in=None, ws=None, row_offset=0, db_ptr=None, ws_bytes=None):
    """ONE call of the C entry -> (rc, scores, idx, status, lb, stats); the outputs are prefilled so that a refusal shows."""
    from merizo_search_amd import _lib
    from merizo_search_amd._lib import ptr
    lib = _lib.load()
    n, nq = db.shape[0], q.shape[0]
    if ws is None:
        ws = torch.empty(max(int(lib.ms_ip_topk_large_workspace_bytes(n, nq, k)), 16), dtype=torch.uint8, device="cuda")
    s = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    i = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    status = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    lb = torch.full((nq,), 7.0, dtype=torch.float32, device="cuda")
    st = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    rc = lib.ms_ip_topk_large(ptr(db) if db_ptr is None else db_ptr, n, row_offset, ptr(q), nq, k, mode, 0, 0, 0.0, float(bound), ptr(lb_in),
                              ptr(s), ptr(i), ptr(status), ptr(lb), ptr(st), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, s, i, status.cpu().numpy(), lb, st.cpu().numpy()


# ------------------------------------------------------------------ arithmetic and order --------
@pytest.mark.parametrize("n,nq,k", [(3000, 37, 65), (3000, 37, 200), (5000, 70, 130), (40000, 70, 1024), (40000, 33, 2048)])
def test_bits_equal_the_oracle_and_ip_topk_in_the_first_round(n, nq, k, torch_gpu):
    """Partial row tiles, nq off the 32-query tile, G = 2..32, k = MS_LARGE_K_MAX.  Every query is final in the FIRST round (the
    largest bin of these inputs holds 2762 of 8192 candidates: counted on the CPU), so nothing passes through the fallback."""
    torch = torch_gpu
    from merizo_search_amd import _lib, ops
    from oracle import oracle as orc
    assert k <= _lib.LARGE_K_MAX and 2762 < _lib.LARGE_K_CAND
    db, q = _norm_db(n, seed=9), _norm_db(nq, seed=10)
    d, dq_ = _dev(torch, db), _dev(torch, q)
    got, st = _large(ops, d, dq_, k, row_offset=1000)
    assert st["first_round"] == nq and not st["forwarded"] and st["rescored"] >= 0, st
    s_ref, i_ref = orc.ip_topk(db, q, k, row_offset=1000, order=1)
    assert np.array_equal(got[1].cpu().numpy(), i_ref)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), s_ref.view(np.uint32))
    assert _same(torch, got, ops.ip_topk(d, dq_, k, row_offset=1000))


# ------------------------------------------------------------------ ties ------------------------
def test_duplicate_rows_resolve_to_the_lowest_row(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    db, q = _norm_db(2048, seed=21), _norm_db(40, seed=22)
    rng = np.random.default_rng(0)
    for src in rng.choice(2048, 64, replace=False):       # copies of strong rows at scattered places
        for dst in rng.choice(2048, 6, replace=False):
            db[dst] = db[src]
    db[5] = q[3]; db[1] = q[3]; db[4] = q[3]; db[36] = q[3]; db[37] = q[3]   # same-tile ties at the top
    d, dq_ = _dev(torch, db), _dev(torch, q)
    got, st = _large(ops, d, dq_, 100)
    assert st["first_round"] == 40, st
    assert _same(torch, got, ops.ip_topk(d, dq_, 100))
    assert got[1].cpu().numpy()[3, :5].tolist() == [1, 4, 5, 36, 37]


@pytest.mark.parametrize("copy_below", [False, True])
def test_a_tie_across_ranks_k_and_k_plus_1_goes_to_the_lower_row(copy_below, torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    k = 100
    db, q = _norm_db(3000, seed=5), _norm_db(3, seed=6)
    d, dq_ = _dev(torch, db), _dev(torch, q)
    top = ops.ip_topk(d, dq_[:1], k + 1)[1].cpu().numpy()[0]
    kth = int(top[k - 1])
    outside = np.setdiff1d(np.arange(3000), top)
    twin = int(outside[outside < kth][0] if copy_below else outside[outside > kth][-1])
    db[twin] = db[kth]                                     # rows kth and twin now tie for ranks k and k + 1 of query 0
    d = _dev(torch, db)
    got, st = _large(ops, d, dq_, k)
    assert st["first_round"] == 3, st
    assert _same(torch, got, ops.ip_topk(d, dq_, k))
    row = got[1].cpu().numpy()[0]
    assert row[k - 1] == min(kth, twin) and max(kth, twin) not in row


def test_identical_rows_inside_the_bin_are_served(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    one = _norm_db(1, seed=1)
    d, dq_ = _dev(torch, np.repeat(one, 5000, axis=0)), _dev(torch, _norm_db(5, seed=2))
    got, st = _large(ops, d, dq_, 100)
    assert st["first_round"] == 5, st
    assert np.array_equal(got[1].cpu().numpy(), np.tile(np.arange(100), (5, 1)))
    assert _same(torch, got, ops.ip_topk(d, dq_, 100))


def test_identical_rows_beyond_the_bin_overflow_twice_and_fall_back(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import _lib, ops
    n = _lib.LARGE_K_CAND + 500
    d, dq_ = _dev(torch, np.repeat(_norm_db(1, seed=1), n, axis=0)), _dev(torch, _norm_db(5, seed=2))
    rc, _, i, status, lb, stats = _raw(torch, d, dq_, 100)
    assert rc == 0 and (status == 1).all() and stats.tolist()[:3] == [0, 5, 0] and (i.cpu().numpy() == -1).all()
    rc, _, _, status2, _, _ = _raw(torch, d, dq_, 100, lb_in=lb)
    assert rc == 0 and (status2 == 1).all()
    got, st = _large(ops, d, dq_, 100)
    assert (st["first_round"], st["second_round"], st["fallback"]) == (0, 0, 5), st
    assert np.array_equal(got[1].cpu().numpy(), np.tile(np.arange(100), (5, 1)))
    assert _same(torch, got, ops.ip_topk(d, dq_, 100))


# ------------------------------------------------------------------ overflow and the second round
def test_family_sorted_database_overflows_and_is_still_exact(torch_gpu):
    """Rows ordered by family (synthetic.family_sorted_database): the groups of far families pull the bound far below what the
    near families score, the bins overflow, and the second round and the fallback complete the answer."""
    torch = torch_gpu
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import synthetic as syn
    db, q = syn.family_sorted_database(40000, 70, seed=7)
    d, dq_ = _dev(torch, db), _dev(torch, q)
    got, st = _large(ops, d, dq_, 1024)
    assert st["first_round"] < 70 and st["first_round"] + st["second_round"] + st["fallback"] == 70, st
    assert _same(torch, got, ops.ip_topk(d, dq_, 1024))


# ------------------------------------------------------------------ modes -----------------------
def test_ip_normq_on_raw_queries(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import synthetic as syn
    d = _dev(torch, _norm_db(5000, seed=13))
    q = _dev(torch, syn.raw_queries(70, seed=14)[0] * np.float32(3.0))
    got, st = _large(ops, d, q, 130, mode=ops.MODE_IP_NORMQ)
    assert st["first_round"] == 70, st
    assert _same(torch, got, ops.ip_topk(d, q, 130, mode=ops.MODE_IP_NORMQ))


@pytest.mark.parametrize("k", [130, 300])
def test_cosine_unit_with_the_length_mask(k, torch_gpu):
    """Query 0 masks all but 3 rows (fewer than k unmasked rows: its cut is a zero, status 2, the list ends in zero-score ties by
    row); query 1 scores every row below zero (every row has a positive first component, the query a negative one)."""
    torch = torch_gpu
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import synthetic as syn
    n, nq, mincov = 5000, 40, 0.7
    raw, lengths = syn.raw_database(n, seed=95)
    raw[:, 0] = np.abs(raw[:, 0]) + 3.0
    lengths = lengths.copy()
    lengths[[11, 2000, 4999]] = 20.0
    q, qlen = syn.raw_queries(nq, seed=96)
    qlen = qlen.copy()
    qlen[0] = 15.0                                         # 15 >= len * 0.7 only for len <= 21.4: the three rows above
    assert int((qlen[0] >= lengths * np.float32(mincov)).sum()) < k
    q[1] = 0.0
    q[1, 0] = -5.0
    rows = ops.l2_normalize_rows_(_dev(torch, raw), 1e-8)
    dq_, dl, dql = _dev(torch, q), _dev(torch, lengths), _dev(torch, qlen)
    want = ops.ip_topk(rows, dq_, k, mode=ops.MODE_COSINE_UNIT, lengths=dl, qlen=dql, mincov=mincov)
    assert float(want[0][1].max()) <= 0.0 and float(want[0][0, k - 1]) == 0.0
    got, st = _large(ops, rows, dq_, k, mode=ops.MODE_COSINE_UNIT, lengths=dl, qlen=dql, mincov=mincov)
    assert st["fallback"] >= 2 and st["first_round"] > 0, st
    assert _same(torch, got, want)
    plain, st = _large(ops, rows, dq_, k, mode=ops.MODE_COSINE_UNIT)      # no mask: a negative cut is served
    assert st["first_round"] == nq, st
    assert _same(torch, plain, ops.ip_topk(rows, dq_, k, mode=ops.MODE_COSINE_UNIT))


# ------------------------------------------------------------------ policy inputs ---------------
def test_nan_and_inf_rows_are_never_returned_and_plus_inf_comes_first(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    n, k = 5000, 100
    db, q = _norm_db(n, seed=31), _norm_db(3, seed=32)
    bad = np.array([0, 17, 33, n // 2, n - 1])
    db[bad[:3], 5] = np.nan
    db[bad[3]] = -np.inf                                   # -inf * (mixed signs) = NaN / -inf
    db[bad[4], :] = np.nan
    db[1234, 7] = np.inf                                   # +inf for the queries with q[7] > 0, -inf for the others
    q[0, 7], q[1, 7] = abs(q[0, 7]) + np.float32(0.1), -abs(q[1, 7]) - np.float32(0.1)
    d, dq_ = _dev(torch, db), _dev(torch, q)
    got, st = _large(ops, d, dq_, k)
    assert st["first_round"] == 3, st
    s, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert not np.isnan(s).any() and not np.isneginf(s).any() and not np.isin(i, bad).any()
    up = q[:, 7] > 0
    assert up.any() and (i[up, 0] == 1234).all() and np.isposinf(s[up, 0]).all() and not np.isin(i[~up], [1234]).any()
    assert _same(torch, got, ops.ip_topk(d, dq_, k))


@pytest.mark.parametrize("n,k", [(50, 100), (0, 100), (255, 100), (128 * 4 - 1, 200), (5000, 64), (5000, 10)])
def test_shapes_the_route_does_not_take_are_forwarded(n, k, torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    d = _dev(torch, _norm_db(n, seed=3)) if n else torch.empty((0, 128), dtype=torch.float32, device="cuda")
    dq_ = _dev(torch, _norm_db(5, seed=4))
    got, st = _large(ops, d, dq_, k, row_offset=77)
    assert st["forwarded"] and st["first_round"] == 5, st
    assert _same(torch, got, ops.ip_topk(d, dq_, k, row_offset=77))
    rc, _, _, status, lb, stats = _raw(torch, d, dq_, k)
    assert rc == 0 and (status == 0).all() and stats.tolist() == [5, 0, 0, -1] and np.isneginf(lb.cpu().numpy()).all()


def test_the_smallest_database_the_route_takes(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    d, dq_ = _dev(torch, _norm_db(256, seed=3)), _dev(torch, _norm_db(5, seed=4))
    got, st = _large(ops, d, dq_, 100)
    assert not st["forwarded"] and st["first_round"] == 5, st
    assert _same(torch, got, ops.ip_topk(d, dq_, 100))


def test_a_row_above_the_row_norm_bound_is_scored_exactly(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    db, q = _norm_db(5000, seed=41), _norm_db(37, seed=42)
    db[77] = q[5] * np.float32(3.0)                        # three times the bound: the best row of query 5 by far
    db[4100] *= np.float32(1.5)
    d, dq_ = _dev(torch, db), _dev(torch, q)
    got, st = _large(ops, d, dq_, 130)
    assert st["first_round"] == 37 and st["rescored"] >= 2 * 37, st
    assert int(got[1][5, 0]) == 77
    assert _same(torch, got, ops.ip_topk(d, dq_, 130))


# ------------------------------------------------------------------ state -----------------------
def test_one_workspace_serves_calls_of_other_shapes_without_clean_up(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import _lib
    d = _dev(torch, _norm_db(5000, seed=51))
    qa, qb = _dev(torch, _norm_db(37, seed=52)), _dev(torch, _norm_db(70, seed=53))
    need = max(int(_lib.load().ms_ip_topk_large_workspace_bytes(5000, nq, k)) for nq, k in ((37, 200), (70, 130)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    first = _raw(torch, d, qa, 200, ws=ws)
    other = _raw(torch, d, qb, 130, ws=ws)
    again = _raw(torch, d, qa, 200, ws=ws)
    for rc, _, _, status, _, stats in (first, other, again):
        assert rc == 0 and (status == 0).all() and stats[1] == 0 and stats[2] == 0 and stats[3] >= 0
    assert first[5].tolist() == again[5].tolist() and first[5][0] == 37 and other[5][0] == 70
    assert _same(torch, first[1:3], again[1:3]) and torch.equal(first[4].view(torch.int32), again[4].view(torch.int32))


def test_given_thresholds(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    k = 130
    d, dq_ = _dev(torch, _norm_db(5000, seed=61)), _dev(torch, _norm_db(37, seed=62))
    want = ops.ip_topk(d, dq_, k)
    rc, s, i, status, lb, stats = _raw(torch, d, dq_, k, lb_in=want[0][:, k - 1].contiguous())      # the k-th best itself: valid and tight
    assert rc == 0 and (status == 0).all() and _same(torch, (s, i), want) and torch.equal(lb, want[0][:, k - 1])
    high = want[0][:, k // 2].contiguous()                 # too high: fewer than k rows reach it
    high[0] = float("nan")
    high[1] = float("-inf")
    rc, s, i, status, lb, stats = _raw(torch, d, dq_, k, lb_in=high)
    assert rc == 0 and (status == 2).all() and stats.tolist()[:3] == [0, 0, 37]
    assert (i.cpu().numpy() == -1).all() and np.isneginf(s.cpu().numpy()).all()


# ------------------------------------------------------------------ refusals --------------------
def test_refusals_return_the_documented_codes_and_launch_nothing(torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import _lib, ops
    d, dq_ = _dev(torch, _norm_db(5000, seed=71)), _dev(torch, _norm_db(8, seed=72))
    need = int(_lib.load().ms_ip_topk_large_workspace_bytes(5000, 8, 100))
    assert need > 0 and int(_lib.load().ms_ip_topk_large_workspace_bytes(-1, 8, 100)) == 0
    cases = [(dict(mode=ops.MODE_COSINE_RAW), -1), (dict(bound=float("nan")), -4), (dict(bound=0.0), -4), (dict(bound=2.0 ** 41), -4),
             (dict(db_ptr=d.data_ptr() + 4), -1), (dict(ws_bytes=need - 1), -2)]
    for kw, code in cases:
        rc, s, i, status, lb, stats = _raw(torch, d, dq_, 100, **kw)
        assert rc == code, (kw, rc)
        assert (status == 77).all() and (stats == 77).all() and (i == 7).all() and (s == 7.0).all() and (lb == 7.0).all(), kw
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    rc = _raw(torch, d, dq_, 100, ws=ws[1:])[0]            # a misaligned workspace
    assert rc == -1
    with pytest.raises(_lib.MerizoHipError):
        ops.ip_topk_large(d, dq_, 100, BOUND, mode=ops.MODE_COSINE_RAW)
    with pytest.raises(_lib.MerizoHipError):
        ops.ip_topk_large(d, dq_, 100, BOUND, workspace=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------ routing and the drivers -----
def test_engine_and_topk_excluding_route_by_the_predicate(torch_gpu, monkeypatch):
    torch = torch_gpu
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import dbsearch as ds
    engine = ds.engine_setup("cuda:0")
    d, dq_ = _dev(torch, _norm_db(5000, seed=81)), _dev(torch, _norm_db(9, seed=82))
    calls = []
    real = ops.ip_topk_large
    monkeypatch.setattr(ops, "ip_topk_large", lambda *a, **kw: (calls.append(a[2]), real(*a, **kw))[1])
    lo = np.arange(9, dtype=np.int64) * 10
    runs = {}
    for rows in (0, NEVER):
        monkeypatch.setattr(ops, "LARGE_K_MIN_ROWS", rows)
        runs[rows] = (engine.ip_topk(d, dq_, 100, row_norm_bound=BOUND), engine.cosine_topk(d, dq_, 100),
                      ops.topk_excluding(d, dq_, 95, lo, lo + 5, row_norm_bound=BOUND)[:2], engine.ip_topk(d, dq_, 100))
        assert calls == [100, 100, 100]                    # (without a row-norm bound Engine.ip_topk stays on ms_ip_topk)
    assert all(_same(torch, a, b) for a, b in zip(runs[0], runs[NEVER]))


EMB_FMT = "query,emb_rank,target,emb_score,q_len,t_len,metadata"


def test_db_search_writes_the_same_file_with_the_route_on_and_off(torch_gpu, tmp_path, monkeypatch):
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import dbsearch as ds
    work = str(tmp_path / "case")
    os.makedirs(work)
    dq.write_case(work, n=5000, seed=8)
    engine = ds.engine_setup("cuda:0")
    calls = []
    real = ops.ip_topk_large
    monkeypatch.setattr(ops, "ip_topk_large", lambda *a, **kw: (calls.append(a[2]), real(*a, **kw))[1])
    files = {}
    for layout in ("fa", "pt"):
        for rows in (0, NEVER):
            monkeypatch.setattr(ops, "LARGE_K_MIN_ROWS", rows)
            out = tmp_path / f"{layout}_{rows}"
            ds.run_dbsearch_db(os.path.join(work, layout), os.path.join(work, layout), str(out), str(tmp_path / "t"), "cuda:0", topk=100,
                               mincos=-2.0, skip_tmalign=True, format_list=EMB_FMT.split(","), header=True, engine=engine,
                               query_rows="100:400", query_batchsize=128, mincov=0.0)
            files[layout, rows] = open(str(out) + "_search.tsv", "rb").read()
        assert files[layout, 0] == files[layout, NEVER] and files[layout, 0].count(b"\n") == 1 + 100 * 300
    assert len(calls) >= 2 and set(calls) == {100}


def test_search_writes_the_same_file_with_the_route_on_and_off(torch_gpu, tmp_path, monkeypatch):
    from merizo_search_amd import cli, ops
    from merizo_search_amd.foldclass import pdbio, synthetic as syn
    monkeypatch.setenv("MERIZO_ALLOW_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("MERIZO_TMALIGN", raising=False)
    pdbs = tmp_path / "pdbs"
    pdbs.mkdir()
    for f in ("M0_ca.pdb", "3w5h_ca.pdb"):
        shutil.copy(os.path.join(GOLDEN, f), pdbs / f)
    names, coords, seqs = syn.synthetic_structures(300, seed=17, min_len=20, max_len=120)
    for n, c, s in zip(names, coords, seqs):
        path = pdbio.write_pdb(str(pdbs), np.round(c.astype(np.float64), 3).astype(np.float32), s, name=os.path.basename(n).replace(".pdb", ""))
        with open(path) as handle:                         # `search` reads column 22 of every line: no short END line
            atoms = [line for line in handle if line.startswith("ATOM")]
        with open(path, "w") as handle:
            handle.writelines(atoms)
    queries = sorted(str(pdbs / f) for f in os.listdir(pdbs))[:6]
    calls = []
    real = ops.ip_topk_large
    monkeypatch.setattr(ops, "ip_topk_large", lambda *a, **kw: (calls.append(a[2]), real(*a, **kw))[1])
    for layout in ("pt", "faiss"):
        db = str(tmp_path / ("db_" + layout))
        cli.createdb([str(pdbs), db, "--layout", layout])
        files = {}
        for rows in (0, NEVER):
            monkeypatch.setattr(ops, "LARGE_K_MIN_ROWS", rows)
            out = str(tmp_path / f"search_{layout}_{rows}")
            cli.search(queries + [db, out, str(tmp_path / "t"), "-k", "100", "--output_headers", "--report_insignificant_hits", "--skip_tmalign"])
            files[rows] = [open(out + suffix, "rb").read() for suffix in ("_search.tsv", "_search_insignificant.tsv")]
        assert files[0] == files[NEVER] and sum(f.count(b"\n") for f in files[0]) > 100
    assert len(calls) >= 2 and set(calls) == {100}
