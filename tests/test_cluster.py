"""`cluster` without a GPU: the definition (the sequential numpy restatement the kernels are compared with) on hand-built
graphs, the host-side refusals of ms_cluster_greedy and of the command, and the driver on one and two gloo ranks with the
oracle engine: both layouts, a batch size that does not divide n, a streamed target -- one TSV, the planted families."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_case as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def _cluster(n, k, edges, lengths, min_score=0.5, mincov=0.0):
    idx, score = cc.lists_from_edges(n, k, edges)
    return cc.cluster_greedy_np(idx, score, np.asarray(lengths, np.int32), min_score, mincov)


# ------------------------------------------------------------------ the definition ---------------
def test_restatement_on_a_path():
    """0 - 1 - 2 - 3 - 4, every edge in the lower row's list only (expectations worked out by hand).
    Decreasing lengths: visit 0 (rep), 1 (next to 0: member), 2 (1 is no rep, 3 not visited: rep), 3 (member), 4 (rep)."""
    edges = [(0, 1, 0.8), (1, 2, 0.9), (2, 3, 0.7), (3, 4, 0.6)]
    rep, score, info = _cluster(5, 1, edges, [50, 40, 30, 20, 10])
    assert rep.tolist() == [0, 2, 2, 2, 4] and info == {"n_reps": 3, "saturated": 4}      # 1 -> 2 (0.9 beats 0.8), 3 -> 2 (0.7 beats 0.6)
    assert score.tolist() == [1.0, np.float32(0.9), 1.0, np.float32(0.7), 1.0] and score.dtype == np.float32 and rep.dtype == np.int64
    # increasing lengths: visit 4 (rep), 3 (member), 2 (rep), 1 (member), 0 (rep): the same set from the other end
    assert _cluster(5, 1, edges, [10, 20, 30, 40, 50])[0].tolist() == [0, 2, 2, 2, 4]
    # equal lengths: the smaller row first -- 0, 1, 2, 3, 4 -- the same set again
    assert _cluster(5, 1, edges, [7] * 5)[0].tolist() == [0, 2, 2, 2, 4]
    # rows 1 and 4 longest: visit 1 (rep), 4 (rep: 3 is not visited yet), 0 (member), 2 (member of 1), 3 (2 is a member, 4 a rep)
    rep, score, info = _cluster(5, 1, edges, [10, 50, 10, 10, 50])
    assert rep.tolist() == [1, 1, 1, 4, 4] and info["n_reps"] == 2
    assert score.tolist() == [np.float32(0.8), 1.0, np.float32(0.9), np.float32(0.6), 1.0]
    # a threshold between the scores cuts the path in two: 0 - 1 - 2   3   4
    rep, _score, info = _cluster(5, 1, edges, [50, 40, 30, 20, 10], min_score=0.75)
    assert rep.tolist() == [0, 2, 2, 3, 4] and info == {"n_reps": 4, "saturated": 2}


def test_restatement_on_the_two_stars():
    n = 6
    leaves = range(1, n)
    # edges only in the leaves' lists, the hub longest: one cluster; each leaf keeps its own score
    rep, score, info = _cluster(n, 1, [(l, 0, 0.5 + 0.05 * l) for l in leaves], [90] + [50] * 5)
    assert rep.tolist() == [0] * n and info["n_reps"] == 1
    assert score.tolist() == [1.0] + [np.float32(0.5 + 0.05 * l) for l in leaves]
    # the mirror: the hub shortest, only its own list has entries: every leaf is a representative, the hub goes to the
    # best-scoring leaf -- the smaller row on a tie
    rep, score, info = _cluster(n, 5, [(0, 1, 0.6), (0, 2, 0.8), (0, 3, 0.7), (0, 4, 0.8), (0, 5, 0.5)], [10] + [50] * 5)
    assert rep.tolist() == [2, 1, 2, 3, 4, 5] and info == {"n_reps": 5, "saturated": 1} and score[0] == np.float32(0.8)


def test_restatement_asymmetric_scores_threshold_and_coverage():
    up = np.nextafter(np.float32(0.8), np.float32(2.0))
    # the two directions of one pair differ in the last bit: the larger one is the weight
    rep, score, _ = _cluster(2, 1, [(0, 1, np.float32(0.8)), (1, 0, up)], [50, 40])
    assert rep.tolist() == [0, 0] and score[1].view(np.uint32) == up.view(np.uint32)
    # only ONE direction clears the threshold: the edge exists all the same
    rep, score, _ = _cluster(2, 1, [(0, 1, 0.3), (1, 0, 0.6)], [50, 40])
    assert rep.tolist() == [0, 0] and score[1] == np.float32(0.6)
    # the threshold itself: equal to it is kept, one ulp below is dropped, NaN is dropped
    cut = np.float32(0.5)
    below = np.nextafter(cut, np.float32(0.0))
    assert _cluster(2, 1, [(1, 0, cut)], [50, 40], min_score=cut)[0].tolist() == [0, 0]
    assert _cluster(2, 1, [(1, 0, below)], [50, 40], min_score=cut)[0].tolist() == [0, 1]
    assert _cluster(2, 1, [(1, 0, np.nan)], [50, 40], min_score=NINF)[0].tolist() == [0, 1]
    assert _cluster(2, 1, [(1, 0, -0.25)], [50, 40], min_score=NINF)[0].tolist() == [0, 0]
    # lengths 70 against 100 at mincov 0.7: in fp32, 0.7f * 100.0f rounds to 70.0f, so the pair is covered; 69 is not
    assert np.float32(0.7) * np.float32(100.0) == np.float32(70.0) and float(np.float32(0.7)) * 100.0 < 70.0
    assert _cluster(2, 1, [(1, 0, 0.9)], [100, 70], mincov=0.7)[0].tolist() == [0, 0]
    assert _cluster(2, 1, [(1, 0, 0.9)], [100, 69], mincov=0.7)[0].tolist() == [0, 1]
    # what is no edge: padding, the row itself, rows outside [0, n) -- never looked up
    idx = np.array([[-1, 0, 2, 1 << 40], [-7, 1, 5, 0]], np.int64)
    score = np.array([[NINF, 0.9, 0.9, 0.9], [0.9, 0.9, 0.9, 0.2]], np.float32)
    rep, _s, info = cc.cluster_greedy_np(idx, score, np.array([5, 5], np.int32), 0.5, 0.0)
    assert rep.tolist() == [0, 1] and info == {"n_reps": 2, "saturated": 0}


def test_restatement_is_independent_of_the_order_inside_a_list():
    rng = np.random.default_rng(4)
    for n, k in ((65, 5), (257, 20)):
        idx, score, lengths = cc.random_lists(n, k, seed=n)
        want = cc.cluster_greedy_np(idx, score, lengths, cc.CUT, 0.7)
        assert 1 < want[2]["n_reps"] < n and want[2]["saturated"] > 0
        perm = np.argsort(rng.random((n, k)), axis=1)
        got = cc.cluster_greedy_np(np.take_along_axis(idx, perm, 1), np.take_along_axis(score, perm, 1), lengths, cc.CUT, 0.7)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and got[2] == want[2]
        # a representative has no representative among its neighbours, a member has one: the set is independent and maximal
        rep = want[0]
        assert (rep[rep] == rep).all()


# ------------------------------------------------------------------ host-side refusals -----------
def test_ms_cluster_greedy_refuses_bad_arguments_without_a_gpu():
    from merizo_search_amd import _lib
    _lib.build()
    lib = _lib.load()
    p = 0x1000                                                          # never dereferenced: the host checks come first
    ok = dict(nbr_idx=p, nbr_score=p, n=100, k=5, lengths=p, min_score=0.5, mincov=0.7, out_rep=p, out_rep_score=p, out_n_reps=p,
              out_rounds=p, out_saturated=p, workspace=p, workspace_bytes=1 << 20, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ms_cluster_greedy(a["nbr_idx"], a["nbr_score"], a["n"], a["k"], a["lengths"], ctypes.c_float(a["min_score"]),
                                     ctypes.c_float(a["mincov"]), a["out_rep"], a["out_rep_score"], a["out_n_reps"], a["out_rounds"],
                                     a["out_saturated"], a["workspace"], a["workspace_bytes"], a["stream"])

    for name in ("nbr_idx", "nbr_score", "lengths", "out_rep", "out_rep_score", "out_n_reps", "out_rounds", "out_saturated", "workspace"):
        assert call(**{name: None}) == -1, name
        assert b"NULL" in lib.ms_last_error() and b"ms_cluster_greedy" in lib.ms_last_error()
    need = int(lib.ms_cluster_workspace_bytes(100))
    assert need >= 12 * 100
    for bad in (dict(n=0), dict(n=-5), dict(n=1 << 31), dict(k=0), dict(k=-1), dict(min_score=float("nan")), dict(mincov=-0.01),
                dict(mincov=1.01), dict(mincov=float("nan")), dict(workspace_bytes=need - 1), dict(workspace_bytes=0)):
        assert call(**bad) == -1, bad
        assert b"ms_cluster_greedy" in lib.ms_last_error(), bad
    assert [int(lib.ms_cluster_workspace_bytes(n)) for n in (0, -1)] == [0, 0]
    assert 0 < int(lib.ms_cluster_workspace_bytes(1)) <= int(lib.ms_cluster_workspace_bytes(2 ** 31 - 1))
    assert lib.ms_version() == 210


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster"))
    names, lengths, family = cc.write_planted(work)
    return work, names, lengths, family


def test_cluster_refusals_come_before_any_gpu_work(planted, tmp_path, caplog):
    """Each ends with the drivers' error line and exit status 1 on a box without a GPU: nothing was asked of a device."""
    from merizo_search_amd import cli
    work = planted[0]
    fa, pt = os.path.join(work, "fa"), os.path.join(work, "pt")
    out, tmp = str(tmp_path / "o"), str(tmp_path / "t")

    def refused(argv, code=1):
        caplog.clear()
        with pytest.raises(SystemExit) as exc:
            cli.main(["cluster"] + argv)
        assert exc.value.code == code, argv
        return caplog.text

    assert "not supported by merizo_search_amd" in refused([fa, out, tmp, "-s", "0.7", "-d", "cpu"])
    assert "neither" in refused([fa + "_missing", out, tmp, "-s", "0.7"])
    for db in (fa, pt):
        assert "exceed the 500 rows of the database" in refused([db, out, tmp, "-s", "0.7", "-k", "500"])
    for cov in ("-0.1", "1.5", "nan"):
        assert "--mincov must lie in [0, 1]" in refused([fa, out, tmp, "-s", "0.7", "-c", cov])
    assert "--mincos" in refused([fa, out, tmp, "-s", "nan"])
    refused([fa, out, tmp], code=2)                                     # -s has no default: argparse refuses the command line
    assert not os.path.exists(out + "_cluster.tsv")
    caplog.clear()
    with pytest.raises(SystemExit) as exc:
        cli.main(["no-such-mode"])
    assert exc.value.code == 2


def test_database_lengths_of_both_layouts(planted):
    from merizo_search_amd.foldclass import dbquery, dbsearch as ds
    work, _names, lengths, _family = planted
    for layout in ("fa", "pt"):
        prefix = os.path.join(work, layout)
        db = ds.read_database(prefix)
        qdb = dbquery.QueryDB(prefix, loaded=None if db["faiss"] else db)
        got = qdb.lengths()
        qdb.close()
        assert got.dtype == np.int32 and np.array_equal(got, lengths), layout


# ------------------------------------------------------------------ the driver, oracle engine ----
_SHIM = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import cluster_case as cc
from merizo_search_amd import cli
from merizo_search_amd.foldclass import dbsearch as ds, sharded
Engine = cc.install_oracle_cluster()
work, tag = sys.argv[2], sys.argv[3]


def engine_setup(device, budget=None):
    eng = Engine()
    if budget is not None:
        eng.budget = budget
    return eng


fa, pt = os.path.join(work, "fa"), os.path.join(work, "pt")
runs = [("fa", None, [fa]), ("pt", None, [pt]), ("fa_37", None, [fa, "--query_batchsize", "37"]), ("pt_37", None, [pt, "--query_batchsize", "37"]),
        ("fa_stream", 0, [fa, "--query_batchsize", "120", "--search_batchsize", "97"])]
for name, budget, argv in runs:
    ds.engine_setup = lambda device, budget=budget: engine_setup(device, budget)
    cli.cluster(argv[:1] + [os.path.join(work, "%s_%s" % (name, tag)), os.path.join(work, "tmp_" + tag)] + argv[1:]
                + ["-s", str(cc.PLANTED_MINCOS), "-k", "20", "--output_headers"])
sharded.finalize_distributed()
'''
_RUNS = ("fa", "pt", "fa_37", "pt_37", "fa_stream")


@pytest.fixture(scope="module")
def oracle_runs(planted):
    """The five cluster runs of _SHIM in one process, and again on two gloo ranks (one launch each)."""
    from conftest import free_port
    work = planted[0]
    shim = os.path.join(work, "shim.py")
    with open(shim, "w") as handle:
        handle.write(_SHIM)
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
    for nproc, tag in ((1, "one"), (2, "two")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), shim, REPO, work, tag]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return planted


def test_cluster_tsv_is_one_file_across_ranks_layouts_batches_and_streaming(oracle_runs):
    work = oracle_runs[0]
    first = open(os.path.join(work, "fa_one_cluster.tsv"), "rb").read()
    assert first.count(b"\n") == 501
    for name in _RUNS:
        for tag in ("one", "two"):
            assert open(os.path.join(work, "%s_%s_cluster.tsv" % (name, tag)), "rb").read() == first, (name, tag)


def test_cluster_returns_the_planted_families(oracle_runs):
    """One cluster per family, its representative the longest member (the smaller row on a tie), singletons alone; clusters
    by the representative's row, its own line first (cosine 1.0000), members by row with their cosine to it."""
    from oracle import oracle as orc
    work, names, lengths, family = oracle_runs
    rows = cc.read_tsv(os.path.join(work, "fa_one_cluster.tsv"))
    assert rows[0] == ["representative", "member", "emb_score"]
    body = rows[1:]
    row_of = {nm: r for r, nm in enumerate(names)}
    want_rep = cc.planted_clusters(lengths, family)
    assert len(body) == len(names) and sorted(row_of[r[1]] for r in body) == list(range(len(names)))
    assert all(want_rep[row_of[member]] == row_of[rep] for rep, member, _ in body)
    key = [(row_of[rep], row_of[member] != row_of[rep], row_of[member]) for rep, member, _ in body]
    assert key == sorted(key)
    assert len({r[0] for r in body}) == len(np.unique(family))
    assert sum(1 for f in np.unique(family) if (family == f).sum() == 1) > 20 and np.bincount(family).max() == 12
    db = np.fromfile(os.path.join(work, "fa_raw_128d_norm.db"), np.float32).reshape(-1, 128)
    for rep, member, text in body:
        if rep == member:
            assert text == "1.0000"
        else:
            s, _i = orc.ip_topk(db[row_of[rep]:row_of[rep] + 1], db[row_of[member]:row_of[member] + 1], 1, order=1)
            assert abs(float(text) - float(s[0, 0])) <= 1e-4, (rep, member)


def test_run_cluster_reports_what_it_found(planted, tmp_path, caplog):
    """The return value and the log: clusters, singletons, rounds -- and the warning once -k cuts lists short."""
    import logging
    from merizo_search_amd.foldclass import cluster
    Engine = cc.install_oracle_cluster()
    work, _names, lengths, family = planted
    times = {}
    with caplog.at_level(logging.INFO):
        rep, score, info = cluster.run_cluster(os.path.join(work, "fa"), str(tmp_path / "a"), str(tmp_path / "t"), "cuda", topk=20,
                                               mincos=cc.PLANTED_MINCOS, mincov=0.7, engine=Engine(), timings=times)
    sizes = np.bincount(family)
    assert np.array_equal(rep, cc.planted_clusters(lengths, family)) and score.dtype == np.float32
    assert info["n"] == 500 and info["n_reps"] == len(sizes) and info["singletons"] == int((sizes == 1).sum()) and info["saturated"] == 0
    assert times["in_place"] is True and times["streamed"] is False
    assert "%d clusters (%d singletons)" % (info["n_reps"], info["singletons"]) in caplog.text and "Raise -k" not in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO):
        _rep, _score, info = cluster.run_cluster(os.path.join(work, "pt"), str(tmp_path / "b"), str(tmp_path / "t"), "cuda", topk=4,
                                                 mincos=cc.PLANTED_MINCOS, mincov=0.7, engine=Engine())
    assert info["saturated"] == int(sizes[family][sizes[family] > 4].size) and info["saturated"] > 0
    assert "%d rows have all 4 kept neighbours" % info["saturated"] in caplog.text and "Raise -k" in caplog.text
