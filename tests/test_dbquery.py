"""db-search without a GPU: the semantics of the drop step (the numpy restatement the kernel is compared with), the host-side
refusals of ms_topk_drop_ranges and of the command, the query-side database reader, and the driver on one and two gloo ranks with the
oracle engine (the drop step = the numpy restatement)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dbquery_case as dq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


# ------------------------------------------------------------------ the drop step's semantics ----
def test_drop_restatement_on_hand_built_lists():
    s = np.array([[0.9, 0.8, 0.8, 0.5, 0.1, NINF],                      # a run of equal scores, one padding entry
                  [0.7, 0.6, 0.5, 0.4, 0.3, 0.2],
                  [0.7, 0.6, NINF, NINF, NINF, NINF]], np.float32)
    i = np.array([[10, 3, 4, 11, 12, -1],
                  [20, 21, 22, 23, 24, 25],
                  [5, 6, -1, -1, -1, -1]], np.int64)
    # query 0: its own chain [10, 13) at the head, inside and at the tail; query 1: nothing excluded (lo >= hi); query 2: everything
    os_, oi, oc = dq.drop_ranges_np(s, i, [10, 7, 0], [13, 7, 100], NINF, 3)
    assert oi.tolist() == [[3, 4, -1], [20, 21, 22], [-1, -1, -1]] and oc.tolist() == [2, 3, 0]
    assert os_[0].tolist() == [np.float32(0.8), np.float32(0.8), NINF] and os_[2].tolist() == [NINF] * 3
    assert os_.dtype == np.float32 and oi.dtype == np.int64 and oc.dtype == np.int32
    # a score cut inside the list: entries below it go, whatever their row; equal to it stays
    os_, oi, oc = dq.drop_ranges_np(s, i, [0, 0, 0], [0, 0, 0], np.float32(0.5), 4)
    assert oi.tolist() == [[10, 3, 4, 11], [20, 21, 22, -1], [5, 6, -1, -1]] and oc.tolist() == [4, 3, 2]
    # the cut and the range together, kout = kin
    os_, oi, oc = dq.drop_ranges_np(s, i, [3, 21, 6], [5, 24, 7], np.float32(0.25), 6)
    assert oi.tolist() == [[10, 11, -1, -1, -1, -1], [20, 24, -1, -1, -1, -1], [5, -1, -1, -1, -1, -1]] and oc.tolist() == [2, 2, 1]
    assert os_[1, :2].tolist() == [np.float32(0.7), np.float32(0.3)]


def test_drop_after_overfetch_is_the_topk_of_the_database_without_the_rows():
    """The exactness argument of the header on the oracle: top-(k + run) of the whole database, then the drop == top-k of the
    database with the run physically removed (indices mapped back), in indices and score bits."""
    from oracle import oracle as orc
    from merizo_search_amd.foldclass import synthetic as syn
    n, nq, k = 900, 40, 10
    db = syn.normalized_database(n, seed=2)
    db[17] = db[400]; db[401] = db[400]                                # ties next to and inside excluded runs
    _names, first, last = dq.chain_names(n, seed=9)
    rows = np.arange(3, n, 23)[:nq]
    q = np.ascontiguousarray(db[rows])
    kk = k + int((last - first).max())
    s, i = orc.ip_topk(db, q, kk, order=1)
    got_s, got_i, got_c = dq.drop_ranges_np(s, i, first[rows], last[rows], NINF, k)
    for j, r in enumerate(rows):
        keep = np.r_[0:first[r], last[r]:n]
        ref_s, ref_i = orc.ip_topk(np.ascontiguousarray(db[keep]), q[j:j + 1], k, order=1)
        assert np.array_equal(got_i[j], keep[ref_i[0]]) and np.array_equal(got_s[j].view(np.uint32), ref_s[0].view(np.uint32)), r
    assert (got_c == k).all()


# ------------------------------------------------------------------ host-side refusals -----------
def test_ms_topk_drop_ranges_refuses_bad_arguments_without_a_gpu():
    from merizo_search_amd import _lib
    _lib.build()
    lib = _lib.load()
    p = 0x1000                                                          # never dereferenced: the host checks come first
    ok = dict(scores=p, idx=p, nq=4, kin=8, lo=p, hi=p, min_score=-float("inf"), kout=8, out_scores=p, out_idx=p, out_count=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ms_topk_drop_ranges(a["scores"], a["idx"], a["nq"], a["kin"], a["lo"], a["hi"], ctypes.c_float(a["min_score"]),
                                       a["kout"], a["out_scores"], a["out_idx"], a["out_count"], a["stream"])

    for name in ("scores", "idx", "lo", "hi", "out_scores", "out_idx", "out_count"):
        assert call(**{name: None}) == -1, name
        assert b"NULL" in lib.ms_last_error()
    for bad in (dict(kout=0), dict(kout=-3), dict(kin=7, kout=8), dict(nq=0), dict(nq=-1), dict(min_score=float("nan"))):
        assert call(**bad) == -1, bad
        assert b"ms_topk_drop_ranges" in lib.ms_last_error()
    assert lib.ms_version() == 210


@pytest.fixture(scope="module")
def small_case(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("dbq"))
    names, first, last = dq.write_case(work, n=120, seed=5)
    dq.write_case(os.path.join(work, "other"), n=50, seed=6)
    return work, names, first, last


def _refused(argv, caplog):
    from merizo_search_amd import cli
    caplog.clear()
    with pytest.raises(SystemExit) as exc:
        cli.main(["db-search"] + argv)
    assert exc.value.code == 1
    return caplog.text


def test_db_search_refusals_come_before_any_gpu_work(small_case, tmp_path, caplog):
    """Each of them ends with the drivers' error line and exit status 1 on a box without a GPU: nothing was asked of a device."""
    work, _names, _first, _last = small_case
    fa, pt, other = os.path.join(work, "fa"), os.path.join(work, "pt"), os.path.join(work, "other", "fa")
    out, tmp = str(tmp_path / "o"), str(tmp_path / "t")
    assert "not supported by merizo_search_amd" in _refused([fa, fa, out, tmp, "-d", "cpu"], caplog)
    for flag in ("--exclude_self", "--exclude_same_chain"):
        assert "need the query database and the target database to be the same" in _refused([fa, other, out, tmp, flag], caplog)
        assert "need the query database" in _refused([fa, pt, out, tmp, flag], caplog)      # same rows, another layout: another database
    assert "exceed the 120 rows of the target" in _refused([fa, fa, out, tmp, "--exclude_self", "-k", "120"], caplog)
    assert "exceed the 120 rows of the target" in _refused([pt, pt, out, tmp, "--exclude_same_chain", "-k", "120"], caplog)
    assert "exceed the 50 rows of the target" in _refused([fa, other[:-2] + "pt", out, tmp, "-k", "51"], caplog)
    for rows in ("7:7", "9:3", "120:", ":0", "0:121", "-1:4", "abc", "1:2:3"):
        assert "--query_rows" in _refused([fa, fa, out, tmp, "--query_rows=" + rows], caplog), rows
    assert "neither" in _refused([fa + "_missing", fa, out, tmp], caplog)
    assert not os.path.exists(out + "_search.tsv")


# ------------------------------------------------------------------ the query-side reader --------
def test_querydb_reads_both_layouts_alike(small_case):
    from merizo_search_amd.foldclass import dbquery
    from merizo_search_amd.foldclass.dbrecords import Records
    work, names, first, last = small_case
    fa, pt = dbquery.QueryDB(os.path.join(work, "fa")), dbquery.QueryDB(os.path.join(work, "pt"))
    assert fa.n == pt.n == 120 and fa.normalized and not pt.normalized
    for lo, hi in ((0, 120), (37, 38), (5, 64)):
        assert fa.names(lo, hi) == pt.names(lo, hi) == names[lo:hi]
        assert fa.seqs(lo, hi) == pt.seqs(lo, hi)
        assert all(np.array_equal(a, b) for a, b in zip(fa.coords(lo, hi), pt.coords(lo, hi)))
        raw = pt.embeddings(lo, hi)
        assert raw.dtype == np.float32 and raw.flags.c_contiguous and raw.shape == (hi - lo, 128)
        np.testing.assert_allclose(fa.embeddings(lo, hi), raw / np.linalg.norm(raw, axis=1, keepdims=True), rtol=0, atol=1e-6)
        for same_chain in (False, True):                                # runs that reach beyond the slice included
            for db in (fa, pt):
                a, b = db.exclusion_ranges(lo, hi, same_chain)
                assert np.array_equal(a, first[lo:hi] if same_chain else np.arange(lo, hi))
                assert np.array_equal(b, last[lo:hi] if same_chain else np.arange(lo, hi) + 1)
    store = Records(os.path.join(work, "pt"))                           # the `query` column: the name as Records.entry gives it
    rec = pt.records(3, 6)
    assert [r["name"] for r in rec] == [store.entry(r)[0] for r in range(3, 6)] and rec[0]["coords"] is not None
    assert fa.records(3, 6, with_coords=False)[1]["coords"] is None
    store.close(); fa.close(); pt.close()
    assert dbquery.same_database(os.path.join(work, "fa"), os.path.join(work, "other", "..", "fa"))
    assert not dbquery.same_database(os.path.join(work, "fa"), os.path.join(work, "pt"))


# ------------------------------------------------------------------ the driver, oracle engine ----
_SHIM = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import dbquery_case as dq
from merizo_search_amd import cli
from merizo_search_amd.foldclass import dbsearch as ds, sharded
Engine = dq.install_oracle_drop()
work, tag = sys.argv[2], sys.argv[3]


def engine_setup(device, budget=None):
    eng = Engine()
    if budget is not None:
        eng.budget = budget
    return eng


fa, pt = os.path.join(work, "fa"), os.path.join(work, "pt")
fmt = ["--format", "query,emb_rank,target,emb_score,q_len,t_len,metadata", "--output_headers", "--skip_tmalign"]
runs = [("self_chain", None, [fa, fa, "-k", "5", "-s", "-2", "--exclude_same_chain", "--query_batchsize", "64"]),
        ("self_stream", 0, [fa, fa, "-k", "3", "-s", "0.05", "--exclude_self", "--query_batchsize", "50", "--search_batchsize", "97",
                            "--query_rows", "13:150"]),
        ("pt_self", None, [pt, pt, "-k", "4", "-s", "-2", "-c", "0.7", "--exclude_same_chain", "--query_batchsize", "33",
                           "--report_insignificant_hits"]),
        ("pt_to_fa", None, [pt, fa, "-k", "3", "-s", "0.1", "--query_rows", "300:"]),
        ("fa_to_pt", None, [fa, pt, "-k", "2", "-s", "-2", "-c", "0.0", "--query_rows", ":77", "--query_batchsize", "76"])]
for name, budget, argv in runs:
    ds.engine_setup = lambda device, budget=budget: engine_setup(device, budget)
    cli.db_search(argv[:2] + [os.path.join(work, "%s_%s" % (name, tag)), os.path.join(work, "tmp_" + tag)] + argv[2:] + fmt)
sharded.finalize_distributed()
'''
_RUNS = ("self_chain", "self_stream", "pt_self", "pt_to_fa", "fa_to_pt")


@pytest.fixture(scope="module")
def oracle_runs(tmp_path_factory):
    """The five db-search runs of _SHIM in one process, and again on two gloo ranks (one launch each)."""
    from conftest import free_port
    work = str(tmp_path_factory.mktemp("dbq_ranks"))
    names, first, last = dq.write_case(work, n=600, seed=5)
    shim = os.path.join(work, "shim.py")
    with open(shim, "w") as handle:
        handle.write(_SHIM)
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
    for nproc, tag in ((1, "one"), (2, "two")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), shim, REPO, work, tag]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return work, names, first, last


def test_db_search_two_gloo_ranks_equal_one_rank_byte_for_byte(oracle_runs):
    work = oracle_runs[0]
    for name in _RUNS:
        for suffix in ("_search.tsv",) + (("_search_insignificant.tsv",) if name == "pt_self" else ()):
            one = open(os.path.join(work, name + "_one" + suffix), "rb").read()
            two = open(os.path.join(work, name + "_two" + suffix), "rb").read()
            assert one == two and (one.count(b"\n") > 1 or "insignificant" in suffix), (name, suffix)


def test_db_search_self_search_reports_no_row_of_the_querys_chain(oracle_runs):
    """Every query row present, in row order, k hits each, none of its own chain; the streamed slice run: no query is its own hit,
    and its lists equal an unfiltered oracle search with the self row removed."""
    from oracle import oracle as orc
    from merizo_search_amd.foldclass import dbquery
    from merizo_search_amd.foldclass.multidomain import domid2chainid
    work, names, first, last = oracle_runs
    row_of = {n: r for r, n in enumerate(names)}
    for run, k in (("self_chain", 5), ("pt_self", 4)):
        rows = dq.read_tsv(os.path.join(work, run + "_one_search.tsv"))
        assert rows[0][:4] == ["query", "emb_rank", "target", "emb_score"]
        body = rows[1:]
        assert [r[0] for r in body] == [n for n in names for _ in range(k)]               # ordered by query row, k hits each
        assert all(domid2chainid(r[0]) != domid2chainid(r[2]) for r in body)
        assert [int(r[1]) for r in body] == list(range(k)) * len(names)
    fa = dbquery.QueryDB(os.path.join(work, "fa"))
    db = fa.embeddings(0, fa.n)
    fa.close()
    body = dq.read_tsv(os.path.join(work, "self_stream_one_search.tsv"))[1:]
    assert all(r[0] != r[2] for r in body) and {r[0] for r in body} <= set(names[13:150])
    s, i = orc.ip_topk(db, np.ascontiguousarray(db[13:150]), 4, order=1)
    want = []
    for j, q in enumerate(range(13, 150)):
        kept = [(sc, r) for sc, r in zip(s[j], i[j]) if r != q][:3]
        want += [(names[q], names[r], "%.4f" % sc) for sc, r in kept if sc >= np.float32(0.05)]
    assert [(r[0], r[2], r[3]) for r in body] == want
    # metadata of the hit's row, lengths of both sides
    assert all(r[6] == '{ "row": %d }' % row_of[r[2]] for r in body)


def test_db_search_metadata_json_and_the_path_it_reports(small_case, tmp_path):
    """--metadata_json: `<output>_search.tsv.hit_metadata.json` holds the metadata of the written hits, in their order, as
    results.write_search_results leaves it for `search`; only the files of this run get one.  `timings` says which path ran:
    queries in place for a faiss-layout self-search on one rank, a streamed target under a small budget."""
    import ast
    import json
    from merizo_search_amd.foldclass import dbsearch as ds, results
    Engine = dq.install_oracle_drop()
    work = small_case[0]
    fa, pt = os.path.join(work, "fa"), os.path.join(work, "pt")
    fmt = "query,emb_rank,target,emb_score,q_len,t_len,metadata".split(",")
    kw = dict(topk=3, mincos=-2.0, skip_tmalign=True, format_list=fmt, exclude_self=True, query_batchsize=50, metadata_json=True)
    times = {}
    out = str(tmp_path / "md")
    assert ds.run_dbsearch_db(fa, fa, out, str(tmp_path / "t"), "cuda", engine=Engine(), timings=times, **kw) == 120
    assert times["in_place"] is True and times["streamed"] is False
    rows = dq.read_tsv(out + "_search.tsv")
    assert len(rows) == 360
    with open(out + "_search.tsv.hit_metadata.json") as handle:
        assert json.load(handle) == [ast.literal_eval(r[6]) for r in rows]
    assert not os.path.exists(out + "_search_insignificant.tsv") and not os.path.exists(out + "_search_insignificant.tsv.hit_metadata.json")
    # the same hits through results.write_search_results' own metadata file: one call, as `search` makes it
    hits = [{j: {"query": r[0], "target": r[2], "score": float(r[3]), "q_len": r[4], "t_len": r[5], "metadata": r[6]}
             for j, r in enumerate(rows[3 * q: 3 * q + 3])} for q in range(120)]
    results.write_search_results(hits, str(tmp_path / "ref.tsv"), fmt, header=False, metadata_json=True)
    assert open(str(tmp_path / "ref.tsv.hit_metadata.json")).read() == open(out + "_search.tsv.hit_metadata.json").read()
    # a streamed target; with the insignificant file asked for, it gets its (empty) metadata file too
    small = Engine()
    small.budget = 0
    out2 = str(tmp_path / "md2")
    ds.run_dbsearch_db(fa, fa, out2, str(tmp_path / "t"), "cuda", engine=small, timings=times, search_batchsize=37,
                       report_insignificant_hits=True, **kw)
    assert times["in_place"] is False and times["streamed"] is True
    assert open(out2 + "_search.tsv").read() == open(out + "_search.tsv").read()
    assert json.load(open(out2 + "_search_insignificant.tsv.hit_metadata.json")) == []
    # the `.pt` layout against itself: never in place (its resident rows are normalised), index and tensor loaded once
    loads = []
    real_load = ds.pickle.load
    ds.pickle.load = lambda handle: loads.append(1) or real_load(handle)
    try:
        ds.run_dbsearch_db(pt, pt, str(tmp_path / "md3"), str(tmp_path / "t"), "cuda", engine=Engine(), timings=times, mincov=0.0, **kw)
    finally:
        ds.pickle.load = real_load
    assert times["in_place"] is False and times["streamed"] is False and len(loads) == 1
    assert len(dq.read_tsv(str(tmp_path / "md3") + "_search.tsv")) == 360
