"""`cluster --cluster_mode connected` without a GPU: the restatement of ms_cluster_components on hand-built cases, the host-side
refusals of the new entry point, and the driver with the oracle engine on the planted chains and dumbbells -- one and two gloo
ranks, both layouts, batches of 37, a streamed target: 50 components where the greedy mode makes more, 60 when -k 4 cuts the lists,
and -k 4 --complete byte-equal to -k 40.  The default mode writes what it wrote."""
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
import cluster_components_case as cpc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------ the restatement ----
def _components(edges, lengths, k=1, extras=(), min_score=0.5, mincov=0.0):
    n = len(lengths)
    idx, score = cc.lists_from_edges(n, k, edges) if k else (None, None)
    ext = [np.array(x) for x in zip(*extras)] if extras else [None] * 3
    rep, link, info = cpc.cluster_components_np(idx, score, ext[0], ext[1], None if ext[2] is None else ext[2].astype(F),
                                                np.asarray(lengths, np.int32), min_score, mincov)
    return rep.tolist(), link.tolist(), info


def test_restatement_single_row():
    assert _components([], [7]) == ([0], [1.0], {"n_components": 1, "saturated": 0})


def test_restatement_edge_held_by_the_higher_row_only():
    """Row 1 lists row 0; row 0 lists nothing: one component, the smaller row represents it on equal lengths, the longer one otherwise."""
    assert _components([(1, 0, 0.8)], [5, 5]) == ([0, 0], [1.0, F(0.8)], {"n_components": 1, "saturated": 1})
    assert _components([(1, 0, 0.8)], [5, 6]) == ([1, 1], [F(0.8), 1.0], {"n_components": 1, "saturated": 1})


def test_restatement_extras_only_and_lists_only_agree():
    edges = [(0, 1, 0.9), (1, 2, 0.6), (4, 3, 0.7)]
    lengths = [10, 30, 20, 5, 5, 9]
    want_rep, want_link = [1, 1, 1, 3, 3, 5], [F(0.9), 1.0, F(0.6), 1.0, F(0.7), 1.0]
    assert _components(edges, lengths) == (want_rep, want_link, {"n_components": 3, "saturated": 3})       # m = 0
    assert _components([], lengths, k=0, extras=edges) == (want_rep, want_link, {"n_components": 3, "saturated": 0})   # k = 0
    # the link score is the row's own strongest edge, in either direction, whatever leads to the representative
    rep, link, _info = _components(edges + [(2, 0, 0.95)], lengths, k=2)
    assert rep == want_rep and link == [F(0.95), 1.0, F(0.95), 1.0, F(0.7), 1.0]


def test_restatement_bridge_that_only_an_extra_entry_holds():
    edges = [(0, 1, 0.9), (2, 3, 0.9)]
    lengths = [4, 4, 4, 8]
    assert _components(edges, lengths)[0] == [0, 0, 3, 3]
    rep, link, info = _components(edges, lengths, extras=[(1, 2, 0.55)])
    assert rep == [3, 3, 3, 3] and link == [F(0.9), F(0.9), F(0.9), 1.0] and info == {"n_components": 1, "saturated": 2}
    # an extra below the cut, with a NaN, or from or to no row is no bridge
    for bad in [(1, 2, 0.45), (1, 2, float("nan")), (7, 2, 0.9), (-1, 2, 0.9), (1, 4, 0.9), (1 << 40, 2, 0.9), (1, 1, 0.9)]:
        assert _components(edges, lengths, extras=[bad])[2]["n_components"] == 2, bad


def test_restatement_bridge_that_fails_coverage_leaves_two_components():
    edges = [(0, 1, 0.9), (2, 3, 0.9), (1, 2, 0.9)]
    assert _components(edges, [100, 100, 69, 69], mincov=0.7)[0] == [0, 0, 2, 2]                  # 69 < 0.7 * 100
    assert _components(edges, [100, 100, 70, 70], mincov=0.7)[0] == [0, 0, 0, 0]
    assert _components(edges, [100, 100, 69, 69], mincov=0.7)[2] == {"n_components": 2, "saturated": 2}     # (rows 0 and 2)


def test_restatement_agrees_with_the_greedy_restatement_on_what_an_edge_is():
    """On random lists with the garbage mix: a greedy cluster lies inside one component (a member is adjacent to its representative),
    a member's link score is at least its score to that representative, and `saturated` is the same number."""
    idx, score, lengths = cc.random_lists(300, 6, 11)
    rep, link, info = cpc.cluster_components_np(idx, score, None, None, None, lengths, cc.CUT, 0.7)
    g_rep, g_score, g_info = cc.cluster_greedy_np(idx, score, lengths, cc.CUT, 0.7)
    assert info["saturated"] == g_info["saturated"] and info["n_components"] < g_info["n_reps"]
    assert np.array_equal(rep[g_rep], rep)
    member = (g_rep != np.arange(300)) & (rep != np.arange(300))
    assert member.any() and np.all(link[member] >= g_score[member])
    assert np.array_equal(lengths[rep], np.maximum.reduceat(lengths[np.argsort(rep, kind="stable")],
                                                            np.nonzero(np.diff(np.sort(rep), prepend=-1))[0])[np.searchsorted(np.unique(rep), rep)])


# ------------------------------------------------------------------ host-side refusals of the C entry ----
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from merizo_search_amd import _lib
    _lib.build()
    lib = _lib.load()
    p = 0x1000                                                          # never dereferenced: the host checks come first
    f = ctypes.c_float
    ok = dict(idx=p, sc=p, n=100, k=5, src=p, dst=p, esc=p, m=7, lengths=p, min_score=0.5, mincov=0.7, rep=p, link=p, n_components=p, rounds=p,
              saturated=p, ws=p, ws_bytes=1 << 20)

    def components(**kw):
        a = dict(ok, **kw)
        return lib.ms_cluster_components(a["idx"], a["sc"], a["n"], a["k"], a["src"], a["dst"], a["esc"], a["m"], a["lengths"], f(a["min_score"]),
                                         f(a["mincov"]), a["rep"], a["link"], a["n_components"], a["rounds"], a["saturated"], a["ws"],
                                         a["ws_bytes"], None)

    need = int(lib.ms_cluster_components_workspace_bytes(100))
    assert need >= 100 * (8 + 4 + 1) and need % 16 == 0
    assert [int(lib.ms_cluster_components_workspace_bytes(n)) for n in (0, -1, 1 << 31)] == [0, 0, 0]
    assert int(lib.ms_cluster_components_workspace_bytes((1 << 31) - 1)) > 13 * ((1 << 31) - 1)
    for name in ("idx", "sc", "src", "dst", "esc", "lengths", "rep", "link", "n_components", "rounds", "saturated", "ws"):
        assert components(**{name: None}) == -1, name
        assert b"NULL" in lib.ms_last_error() and b"ms_cluster_components" in lib.ms_last_error()
    for bad in (dict(n=0), dict(n=-5), dict(n=1 << 31), dict(k=-1), dict(m=-1), dict(min_score=float("nan")), dict(mincov=-0.01), dict(mincov=1.01),
                dict(mincov=float("nan")), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=p + 8)):
        assert components(**bad) == -1, bad
        assert b"ms_cluster_components" in lib.ms_last_error(), bad
    # k == 0 with NULL lists and m == 0 with NULL edge arrays pass the pointer check (a short workspace stops them before any launch)
    assert components(k=0, idx=None, sc=None, ws_bytes=0) == -1 and b"workspace" in lib.ms_last_error()
    assert components(m=0, src=None, dst=None, esc=None, ws_bytes=0) == -1 and b"workspace" in lib.ms_last_error()
    assert lib.ms_version() == 210


def test_cli_refuses_an_unknown_cluster_mode_before_any_gpu_work(tmp_path, capsys):
    from merizo_search_amd import cli
    with pytest.raises(SystemExit) as exc:
        cli.main(["cluster", str(tmp_path / "nodb"), str(tmp_path / "o"), str(tmp_path / "t"), "-s", "0.7", "--cluster_mode", "average"])
    assert exc.value.code == 2 and "--cluster_mode" in capsys.readouterr().err


# ------------------------------------------------------------------ the driver, oracle engine ----
@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_components"))
    names, lengths, group = cpc.write_chains(work)
    return work, names, lengths, group


_SHIM = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import cluster_components_case as cpc
from merizo_search_amd.foldclass import cluster, sharded
Engine = cpc.install_oracle_components()
work, tag = sys.argv[2], sys.argv[3]
rank = sharded.init_distributed()[0]                                   # (what cli.cluster does first under torchrun)


def run(name, db, budget=None, k=4, mode="connected", **kw):
    eng = Engine()
    if budget is not None:
        eng.budget = budget
    rep, score, info = cluster.run_cluster(os.path.join(work, db), os.path.join(work, "%s_%s" % (name, tag)), os.path.join(work, "tmp_" + tag),
                                           "cuda", topk=k, mincos=cpc.MINCOS, mincov=0.7, header=True, engine=eng, mode=mode, **kw)
    if rank == 0:
        with open(os.path.join(work, "%s_%s.json" % (name, tag)), "w") as handle:
            json.dump(info, handle)


for db in ("cfa", "cpt"):
    if tag == "one":
        run("k40_" + db, db, k=40)
        run("greedy_" + db, db, k=40, mode="greedy")
    run("cut_" + db, db)
    run("full_" + db, db, complete=True)
    run("full37_" + db, db, complete=True, query_batchsize=37)
run("stream_cfa", "cfa", budget=0, complete=True, query_batchsize=120, search_batchsize=97)
sharded.finalize_distributed()
'''


@pytest.fixture(scope="module")
def oracle_runs(chains):
    """The runs of _SHIM in one process, and again on two gloo ranks (one launch each)."""
    from conftest import free_port
    work = chains[0]
    shim = os.path.join(work, "shim_components.py")
    with open(shim, "w") as handle:
        handle.write(_SHIM)
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
    for nproc, tag in ((1, "one"), (2, "two")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), shim, REPO, work, tag]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return chains


def _tsv(work, name, tag):
    return open(os.path.join(work, "%s_%s_cluster.tsv" % (name, tag)), "rb").read()


def _info(work, name, tag):
    return json.load(open(os.path.join(work, "%s_%s.json" % (name, tag))))


def _groups_of(text, names):
    """{frozenset of member rows} of a cluster TSV with a header line."""
    row = {nm: r for r, nm in enumerate(names)}
    groups = {}
    for rep, member, _score in (line.split("\t") for line in text.decode().splitlines()[1:]):
        groups.setdefault(rep, set()).add(row[member])
    return {frozenset(g) for g in groups.values()}


@pytest.mark.parametrize("layout", ["cfa", "cpt"])
def test_connected_mode_returns_the_planted_groups_and_the_greedy_mode_more_clusters(oracle_runs, layout):
    work, names, _lengths, group = oracle_runs
    info = _info(work, "k40_" + layout, "one")
    assert info["mode"] == "connected" and info["n_components"] == cpc.GROUPS == 50 and info["largest"] == cpc.LARGEST == 33
    assert info["full_lists"] == 0 and info["complete"] is False and info["singletons"] == 8 and "n_reps" not in info
    text = _tsv(work, "k40_" + layout, "one")
    assert text.splitlines()[0] == b"representative\tmember\tlink_score" and text.count(b"\n") == cpc.ROWS + 1
    assert _groups_of(text, names) == {frozenset(np.nonzero(group == g)[0].tolist()) for g in range(cpc.GROUPS)}
    # every domain is equally long: the smallest row of a group represents it, with 1.0000; a chain's members link at ~0.75
    lines = [line.split("\t") for line in text.decode().splitlines()[1:]]
    row = {nm: r for r, nm in enumerate(names)}
    for rep, member, score in lines:
        assert row[rep] == np.nonzero(group == group[row[member]])[0].min()
        assert (score == "1.0000") == (rep == member)
    greedy = _info(work, "greedy_" + layout, "one")
    assert greedy["mode"] == "greedy" and greedy["n_reps"] > info["n_components"] and "largest" not in greedy
    assert _tsv(work, "greedy_" + layout, "one").splitlines()[0] == b"representative\tmember\temb_score"


def test_k4_without_complete_splits_the_dumbbells_and_complete_writes_the_k40_tsv(oracle_runs):
    """-k 4 keeps four of a clique member's five clique mates and none of the six across: 60 components.  -k 4 --complete is the
    -k 40 file byte for byte -- ranks, batches of 37, a streamed target.  (The two layouts hold different numbers -- the `.pt` rows
    are scaled per row -- so a cosine may differ in its last printed digit between them: across layouts the names are compared.)"""
    work = oracle_runs[0]
    want = {layout: _tsv(work, "k40_" + layout, "one") for layout in ("cfa", "cpt")}
    pairs = lambda text: [line.split(b"\t")[:2] for line in text.splitlines()]
    assert pairs(want["cfa"]) == pairs(want["cpt"])
    for tag in ("one", "two"):
        for layout in ("cfa", "cpt"):
            cut = _info(work, "cut_" + layout, tag)
            assert cut["n_components"] == cpc.SPLIT_AT_K4 == 60 and cut["full_lists"] == cpc.DUMBBELLS * 2 * cpc.CLIQUE and cut["largest"] == 33
            assert _tsv(work, "cut_" + layout, tag) != want[layout]
            for name in ("full_", "full37_"):
                assert _tsv(work, name + layout, tag) == want[layout], (name, layout, tag)
                info = _info(work, name + layout, tag)
                assert info["n_components"] == 50 and info["largest"] == 33 and info["complete"] is True and info["mode"] == "connected"
                assert info["full_lists"] == 120 and info["edges"] == 120 * 11
        assert _tsv(work, "stream_cfa", tag) == want["cfa"], tag
        assert _tsv(work, "cut_cfa", tag) == _tsv(work, "cut_cfa", "one")


def test_the_log_warns_of_split_components_only_without_complete(chains, tmp_path, caplog):
    from merizo_search_amd.foldclass import cluster
    Engine = cpc.install_oracle_components()
    work = chains[0]
    run = lambda out, **kw: cluster.run_cluster(os.path.join(work, "cfa"), str(tmp_path / out), str(tmp_path / "t"), "cuda", mincos=cpc.MINCOS,
                                                mincov=0.7, engine=Engine(), mode="connected", **kw)
    with caplog.at_level(logging.INFO):
        _rep, link, info = run("cut", topk=4)
    assert info["n_components"] == 60
    assert "120 lists are full" in caplog.text and "split in two" in caplog.text and "--complete gives the true components" in caplog.text
    assert "60 components (8 singletons, the largest of 33 rows) of 444 rows" in caplog.text and "Raise -k" not in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO):
        rep, link, info = run("full", topk=4, complete=True)
    assert info["n_components"] == 50 and "lists are full" not in caplog.text and "split in two" not in caplog.text
    assert "120 rows had a full list of 4" in caplog.text and "components are those of the full threshold graph" in caplog.text
    assert link.dtype == np.float32 and np.array_equal(link == 1.0, rep == np.arange(444))
    caplog.clear()
    with caplog.at_level(logging.INFO):
        run("wide", topk=40)
    assert "lists are full" not in caplog.text and "50 components" in caplog.text
    with pytest.raises(SystemExit):
        cluster.run_cluster(os.path.join(work, "cfa"), str(tmp_path / "bad"), str(tmp_path / "t"), "cuda", topk=4, mincos=cpc.MINCOS,
                            engine=Engine(), mode="average")
    assert "must be 'greedy' or 'connected'" in caplog.text and not os.path.exists(str(tmp_path / "bad_cluster.tsv"))


def test_default_mode_writes_what_it_wrote(tmp_path, caplog):
    """cluster_case's planted database: run_cluster without the new argument, with mode='greedy', and the command without the flag
    write one file, headed emb_score, with the log lines of the greedy mode; write_cluster_tsv's header column has a name."""
    from merizo_search_amd.foldclass import cluster
    Engine = ccc.install_oracle_complete()                                 # (no cluster_components on this engine: it is never asked)
    work = str(tmp_path / "db")
    names, lengths, family = cc.write_planted(work)
    run = lambda out, **kw: cluster.run_cluster(os.path.join(work, "fa"), str(tmp_path / out), str(tmp_path / "t"), "cuda", topk=4,
                                                mincos=cc.PLANTED_MINCOS, mincov=0.7, header=True, engine=Engine(), **kw)
    with caplog.at_level(logging.INFO):
        rep, score, info = run("plain")
    assert info["mode"] == "greedy" and "n_reps" in info and "largest" not in info and "n_components" not in info
    assert "clusters (" in caplog.text and "Raise -k" in caplog.text and "components" not in caplog.text
    plain = open(str(tmp_path / "plain_cluster.tsv"), "rb").read()
    assert plain.splitlines()[0] == b"representative\tmember\temb_score"
    want_rep, want_score, _info2 = cc.cluster_greedy_np(*_lists_at_k4(names, lengths), lengths, cc.PLANTED_MINCOS, 0.7)
    assert np.array_equal(rep, want_rep) and np.array_equal(ccc.bits(score), ccc.bits(want_score))
    run("named", mode="greedy")
    assert open(str(tmp_path / "named_cluster.tsv"), "rb").read() == plain
    for complete in ((), (dict(complete=True),)):
        kw = complete[0] if complete else {}
        run("a", **kw)
        run("b", mode="greedy", **kw)
        assert open(str(tmp_path / "a_cluster.tsv"), "rb").read() == open(str(tmp_path / "b_cluster.tsv"), "rb").read()
    cluster.write_cluster_tsv(str(tmp_path / "w.tsv"), ["x", "y"], np.array([0, 0]), np.array([1.0, 0.5], np.float32), True)
    assert open(str(tmp_path / "w.tsv")).read() == "representative\tmember\temb_score\nx\tx\t1.0000\nx\ty\t0.5000\n"
    cluster.write_cluster_tsv(str(tmp_path / "w.tsv"), ["x", "y"], np.array([0, 0]), np.array([1.0, 0.5], np.float32), True, "link_score")
    assert open(str(tmp_path / "w.tsv")).read() == "representative\tmember\tlink_score\nx\tx\t1.0000\nx\ty\t0.5000\n"


def _lists_at_k4(names, lengths):
    """The neighbour lists the self-search of cluster_case's planted database keeps at -k 4, from the oracle's own scores."""
    from oracle import oracle as orc
    rows, _l, _family = cc.planted_rows()
    n, k = rows.shape[0], 4
    s, i = orc.ip_topk(rows, rows, k + 1, order=1)
    idx, score = cc.empty_lists(n, k)
    for r in range(n):
        keep = [(sv, iv) for sv, iv in zip(s[r], i[r]) if iv != r and sv >= np.float32(cc.PLANTED_MINCOS)][:k]
        for c, (sv, iv) in enumerate(keep):
            idx[r, c], score[r, c] = iv, sv
    return idx, score
