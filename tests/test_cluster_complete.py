"""`cluster --complete` without a GPU: the restatement of ms_cluster_greedy_edges on hand-built cases, the host-side refusals of
the two new entry points and of the command, and the driver with the oracle engine on one and two gloo ranks -- both layouts,
batches of 37, a streamed target, both planted databases -- every TSV at -k 4 --complete byte-equal to the one-process -k 20 TSV."""
import ctypes
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_case as cc
import cluster_complete_case as ccc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement ----
def test_restatement_extras_are_list_entries_by_another_road():
    """The same directed entries as lists, as extras, and split between the two: one answer; an extra whose src is no row says nothing."""
    edges = [(0, 1, 0.8), (1, 2, 0.9), (2, 3, 0.7), (3, 4, 0.6)]
    lengths = np.array([50, 40, 30, 20, 10], np.int32)
    idx, score = cc.lists_from_edges(5, 1, edges)
    want = cc.cluster_greedy_np(idx, score, lengths, 0.5, 0.0)
    assert want[0].tolist() == [0, 2, 2, 2, 4]
    src, dst, sc = (np.array(x) for x in zip(*edges))
    got = ccc.cluster_greedy_edges_np(None, None, src, dst, sc.astype(np.float32), lengths, 0.5, 0.0)
    assert got[0].tolist() == want[0].tolist() and np.array_equal(ccc.bits(got[1]), ccc.bits(want[1])) and got[2] == {"n_reps": 3, "saturated": 0}
    idx2, score2 = cc.lists_from_edges(5, 1, edges[:2])
    got = ccc.cluster_greedy_edges_np(idx2, score2, np.append(src[2:], [7, -1]), np.append(dst[2:], [0, 0]),
                                      np.append(sc[2:], [0.9, 0.9]).astype(np.float32), lengths, 0.5, 0.0)
    assert got[0].tolist() == want[0].tolist() and got[2] == {"n_reps": 3, "saturated": 2}
    # a duplicate with a larger score raises the weight, one with a smaller score changes nothing
    got = ccc.cluster_greedy_edges_np(idx, score, np.array([1, 1]), np.array([0, 2]), np.array([0.95, 0.1], np.float32), lengths, 0.5, 0.0)
    assert got[0].tolist() == [0, 0, 2, 2, 4] and got[1][1] == np.float32(0.95)


# ------------------------------------------------------------------ host-side refusals of the C entries ----
def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from merizo_search_amd import _lib
    _lib.build()
    lib = _lib.load()
    p = 0x1000                                                          # never dereferenced: the host checks come first
    f = ctypes.c_float
    ok = dict(db=p, n=100, row_offset=0, q=p, nq=5, mode=_lib.MODE_IP_PRENORM, lo=p, hi=p, min_score=0.5, bound=1.0, src=p, dst=p, score=p,
              cap=10, count=p, stats=p, ws=p, ws_bytes=1 << 20)

    def edges(**kw):
        a = dict(ok, **kw)
        return lib.ms_threshold_edges(a["db"], a["n"], a["row_offset"], a["q"], a["nq"], a["mode"], a["lo"], a["hi"], f(a["min_score"]),
                                      f(a["bound"]), a["src"], a["dst"], a["score"], a["cap"], a["count"], a["stats"], a["ws"], a["ws_bytes"], None)

    need = int(lib.ms_threshold_edges_workspace_bytes(100, 5))
    assert need >= 32 * 128 * 6 and int(lib.ms_threshold_edges_workspace_bytes(0, 5)) > 0
    assert [int(lib.ms_threshold_edges_workspace_bytes(n, nq)) for n, nq in ((-1, 5), (100, 0), (100, -3))] == [0, 0, 0]
    arg = [dict(mode=_lib.MODE_COSINE_RAW), dict(mode=17), dict(nq=0), dict(n=-1), dict(cap=-1), dict(q=None), dict(count=None), dict(ws=None),
           dict(db=None), dict(src=None), dict(dst=None), dict(score=None), dict(lo=None), dict(hi=None), dict(min_score=float("nan")),
           dict(db=p + 4), dict(ws=p + 8)]
    for bad in arg:
        assert edges(**bad) == -1, bad
        assert b"ms_threshold_edges" in lib.ms_last_error(), bad
    for bad in (dict(bound=float("nan")), dict(bound=0.0), dict(bound=-1.0), dict(bound=1e-13), dict(bound=2e12), dict(n=1 << 31)):
        assert edges(**bad) == -4, bad
    for bad in (dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert edges(**bad) == -2, bad
    # the order of ms_md_chain_scan_mq: mode, counts, NULL, NaN, alignment, bound, workspace
    assert edges(mode=17, nq=0) == -1 and b"mode" in lib.ms_last_error()
    assert edges(nq=0, q=None) == -1 and b"nq >= 1" in lib.ms_last_error()
    assert edges(q=None, min_score=float("nan")) == -1 and b"NULL" in lib.ms_last_error()
    assert edges(min_score=float("nan"), bound=0.0) == -1 and edges(bound=0.0, ws_bytes=0) == -4
    # what is allowed: no ranges, only counting without outputs
    # (these would launch: only their checks are compared through a NaN min_score behind them)
    assert edges(lo=None, hi=None, min_score=float("nan")) == -1 and b"NaN" in lib.ms_last_error()
    assert edges(cap=0, src=None, dst=None, score=None, min_score=float("nan")) == -1 and b"NaN" in lib.ms_last_error()
    assert edges(n=0, db=None, min_score=float("nan")) == -1 and b"NaN" in lib.ms_last_error()

    okc = dict(idx=p, sc=p, n=100, k=5, src=p, dst=p, esc=p, m=7, lengths=p, min_score=0.5, mincov=0.7, rep=p, rep_score=p, n_reps=p, rounds=p,
               saturated=p, ws=p, ws_bytes=1 << 20)

    def greedy(**kw):
        a = dict(okc, **kw)
        return lib.ms_cluster_greedy_edges(a["idx"], a["sc"], a["n"], a["k"], a["src"], a["dst"], a["esc"], a["m"], a["lengths"], f(a["min_score"]),
                                           f(a["mincov"]), a["rep"], a["rep_score"], a["n_reps"], a["rounds"], a["saturated"], a["ws"],
                                           a["ws_bytes"], None)

    needc = int(lib.ms_cluster_workspace_bytes(100))
    for name in ("idx", "sc", "src", "dst", "esc", "lengths", "rep", "rep_score", "n_reps", "rounds", "saturated", "ws"):
        assert greedy(**{name: None}) == -1, name
        assert b"NULL" in lib.ms_last_error() and b"ms_cluster_greedy_edges" in lib.ms_last_error()
    for bad in (dict(n=0), dict(n=-5), dict(n=1 << 31), dict(k=-1), dict(m=-1), dict(min_score=float("nan")), dict(mincov=-0.01), dict(mincov=1.01),
                dict(mincov=float("nan")), dict(ws_bytes=needc - 1), dict(ws_bytes=0), dict(ws=p + 8)):
        assert greedy(**bad) == -1, bad
        assert b"ms_cluster_greedy_edges" in lib.ms_last_error(), bad
    # k == 0 with NULL lists and m == 0 with NULL edge arrays pass the pointer check (a short workspace stops them before any launch)
    assert greedy(k=0, idx=None, sc=None, ws_bytes=0) == -1 and b"workspace" in lib.ms_last_error()
    assert greedy(m=0, src=None, dst=None, esc=None, ws_bytes=0) == -1 and b"workspace" in lib.ms_last_error()
    assert lib.ms_version() == 210


# ------------------------------------------------------------------ the command's refusals ----
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_complete"))
    names, lengths, family = cc.write_planted(work)
    names2, lengths2, family2 = ccc.write_split(work)
    assert names2 == names and np.array_equal(family2, family)
    return work, names, lengths, family, lengths2


def test_max_edges_below_one_is_refused_before_any_gpu_work(planted, tmp_path, caplog):
    """On a box without a GPU: the error line and exit status 1, nothing asked of a device, no file."""
    from merizo_search_amd import cli
    fa, out = os.path.join(planted[0], "fa"), str(tmp_path / "o")
    for value in ("0", "-5"):
        caplog.clear()
        with pytest.raises(SystemExit) as exc:
            cli.main(["cluster", fa, out, str(tmp_path / "t"), "-s", "0.7", "--complete", "--max_edges", value])
        assert exc.value.code == 1 and "--max_edges must be >= 1" in caplog.text
    assert not os.path.exists(out + "_cluster.tsv")


def test_expected_counts_of_the_two_databases(planted):
    """What the issue measured on the CPU: at -k 4 the lists of 327 rows are full; on the {50, 100} lengths at coverage 0.7 only
    20 of them count as saturated -- the old warning under-counts -- and on the planted lengths all of them do."""
    _work, _names, lengths, family, lengths2 = planted
    one = ccc.expected_counts(lengths, family, 4, 0.7)
    two = ccc.expected_counts(lengths2, family, 4, ccc.SPLIT_MINCOV)
    assert one["full_lists"] == two["full_lists"] == 327 and one["edges"] == two["edges"] > 327 * 4
    assert one["saturated"] == one["full_lists"] and two["saturated"] == 20 < two["full_lists"]
    assert ccc.expected_counts(lengths, family, 20, 0.7) == {"full_lists": 0, "edges": 0, "saturated": 0}


# ------------------------------------------------------------------ the driver, oracle engine ----
_SHIM = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import cluster_case as cc
import cluster_complete_case as ccc
from merizo_search_amd.foldclass import cluster, dbsearch as ds, sharded
Engine = ccc.install_oracle_complete()
work, tag = sys.argv[2], sys.argv[3]
rank = sharded.init_distributed()[0]                                   # (what cli.cluster does first under torchrun)


def engine(budget):
    eng = Engine()
    if budget is not None:
        eng.budget = budget
    return eng


def run(name, db, budget=None, k=4, mincov=0.7, **kw):
    rep, score, info = cluster.run_cluster(os.path.join(work, db), os.path.join(work, "%s_%s" % (name, tag)), os.path.join(work, "tmp_" + tag),
                                           "cuda", topk=k, mincos=cc.PLANTED_MINCOS, mincov=mincov, header=True, engine=engine(budget), **kw)
    if rank == 0:
        with open(os.path.join(work, "%s_%s.json" % (name, tag)), "w") as handle:
            json.dump(info, handle)


if tag == "one":
    for db in ("fa", "pt", "fa2", "pt2"):
        run("k20_" + db, db, k=20)
for db in ("fa", "pt", "fa2", "pt2"):
    run(db, db, complete=True)
    run(db + "_37", db, complete=True, query_batchsize=37)
for db in ("fa", "fa2"):
    run(db + "_stream", db, budget=0, complete=True, query_batchsize=120, search_batchsize=97)
    run(db + "_room", db, complete=True, edge_room=64)
sharded.finalize_distributed()
'''
_RUNS = ("%s", "%s_37")
_FA_RUNS = ("%s_stream", "%s_room")


@pytest.fixture(scope="module")
def oracle_runs(planted):
    """The runs of _SHIM in one process, and again on two gloo ranks (one launch each)."""
    from conftest import free_port
    work = planted[0]
    shim = os.path.join(work, "shim_complete.py")
    with open(shim, "w") as handle:
        handle.write(_SHIM)
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
    for nproc, tag in ((1, "one"), (2, "two")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), shim, REPO, work, tag]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return planted


def _names_of(which):
    runs = []
    for layout in ("fa", "pt"):
        db = layout + which
        runs += [pattern % db for pattern in _RUNS] + ([pattern % db for pattern in _FA_RUNS] if layout == "fa" else [])
    return runs


@pytest.mark.parametrize("which", ["", "2"])
def test_complete_tsv_equals_the_k20_tsv_across_ranks_layouts_batches_streaming_and_growth(oracle_runs, which):
    """Byte for byte the one-process -k 20 TSV of the same database files.  (The two layouts of one database hold different numbers
    -- the `.pt` rows are the unit rows scaled per row, its cosines are computed from those -- so a cosine may differ in its last
    printed digit between them: across layouts the representative and member columns are compared.)"""
    work = oracle_runs[0]
    want = {layout: open(os.path.join(work, "k20_%s%s_one_cluster.tsv" % (layout, which)), "rb").read() for layout in ("fa", "pt")}
    assert want["fa"].count(b"\n") == 501
    pairs = lambda text: [line.split(b"\t")[:2] for line in text.splitlines()]
    assert pairs(want["fa"]) == pairs(want["pt"])
    for name in _names_of(which):
        for tag in ("one", "two"):
            assert open(os.path.join(work, "%s_%s_cluster.tsv" % (name, tag)), "rb").read() == want[name[:2]], (name, tag)


@pytest.mark.parametrize("which", ["", "2"])
def test_complete_runs_report_full_lists_edges_and_saturated(oracle_runs, which):
    work, _names, lengths, family, lengths2 = oracle_runs
    want = ccc.expected_counts(lengths2 if which else lengths, family, 4, 0.7)
    for name in _names_of(which):
        for tag in ("one", "two"):
            info = json.load(open(os.path.join(work, "%s_%s.json" % (name, tag))))
            assert {key: info[key] for key in want} == want, (name, tag, info)
            assert info["complete"] is True and info["n"] == 500 and info["k"] == 4
    info = json.load(open(os.path.join(work, "k20_fa%s_one.json" % which)))
    assert info["complete"] is False and info["full_lists"] == 0 and "edges" not in info


def test_complete_differs_from_the_truncated_run_and_the_log_says_what_happened(planted, tmp_path, caplog):
    """-k 4 without --complete gives another TSV and both warnings on the {50, 100} database (the old text verbatim, the new one
    naming --complete); with --complete neither, and one INFO line with the three numbers."""
    from merizo_search_amd.foldclass import cluster
    Engine = ccc.install_oracle_complete()
    work, _names, _lengths, family, lengths2 = planted
    want = ccc.expected_counts(lengths2, family, 4, 0.7)
    run = lambda out, **kw: cluster.run_cluster(os.path.join(work, "fa2"), str(tmp_path / out), str(tmp_path / "t"), "cuda", topk=4,
                                                mincos=cc.PLANTED_MINCOS, mincov=0.7, engine=Engine(), **kw)
    with caplog.at_level(logging.INFO):
        _rep, _score, info = run("cut")
    assert info["full_lists"] == want["full_lists"] and info["saturated"] == want["saturated"] and info["complete"] is False
    assert ("%d rows have all 4 kept neighbours above the thresholds: their lists may have been cut short and neighbours beyond them are "
            "unknown to the clustering. Raise -k." % want["saturated"]) in caplog.text
    assert "%d lists are full" % want["full_lists"] in caplog.text and "--complete" in caplog.text and "--mincov" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO):
        rep, _score, info = run("full", complete=True)
    assert "Raise -k" not in caplog.text and "lists are full" not in caplog.text
    assert "%d rows had a full list of 4" % want["full_lists"] in caplog.text and "%d directed entries" % want["edges"] in caplog.text
    assert "(%d cells re-scored" % info["rescored"] in caplog.text
    assert open(str(tmp_path / "full_cluster.tsv"), "rb").read() != open(str(tmp_path / "cut_cluster.tsv"), "rb").read()
    # the complete clustering never puts two representatives within the threshold of each other: here, one per family and length class
    assert info["n_reps"] < json.loads(json.dumps(run("cut2")[2]))["n_reps"]
    # on the first database at -k 4 every full list is saturated: the old warning alone
    caplog.clear()
    with caplog.at_level(logging.INFO):
        cluster.run_cluster(os.path.join(work, "fa"), str(tmp_path / "one"), str(tmp_path / "t"), "cuda", topk=4, mincos=cc.PLANTED_MINCOS,
                            mincov=0.7, engine=Engine())
    assert "Raise -k" in caplog.text and "lists are full" not in caplog.text


def test_max_edges_too_small_is_refused_with_the_count_and_no_tsv(planted, tmp_path, caplog):
    from merizo_search_amd.foldclass import cluster
    Engine = ccc.install_oracle_complete()
    work, _names, lengths, family, _lengths2 = planted
    want = ccc.expected_counts(lengths, family, 4, 0.7)
    out = str(tmp_path / "refused")
    for extra in (dict(), dict(edge_room=16), dict(query_batchsize=37)):
        caplog.clear()
        with pytest.raises(SystemExit) as exc:
            cluster.run_cluster(os.path.join(work, "fa"), out, str(tmp_path / "t"), "cuda", topk=4, mincos=cc.PLANTED_MINCOS, mincov=0.7,
                                engine=Engine(), complete=True, max_edges=100, **extra)
        assert exc.value.code == 1
        assert "have %d neighbours" % want["edges"] in caplog.text and "--max_edges 100" in caplog.text and "-s/--mincos" in caplog.text
        assert str(cc.PLANTED_MINCOS) in caplog.text
        assert not os.path.exists(out + "_cluster.tsv")
    # exactly enough room is no refusal
    _rep, _score, info = cluster.run_cluster(os.path.join(work, "fa"), out, str(tmp_path / "t"), "cuda", topk=4, mincos=cc.PLANTED_MINCOS,
                                             mincov=0.7, engine=Engine(), complete=True, max_edges=want["edges"], edge_room=64)
    assert info["edges"] == want["edges"] and os.path.exists(out + "_cluster.tsv")
