"""`cluster --tree / --levels` without a GPU: the restatement of ms_cluster_tree (cluster_tree_case.cluster_tree_np) against the
restatement of ms_cluster_components on random multigraphs with heavy ties -- the forest cut at T is the graph cut at T -- the
host-side refusals of the new entry point and of the new flags, and the driver with the oracle engine on the planted chains and
dumbbells in both layouts: every level file is the file of a separate run at that --mincos."""
import ctypes
import os

import numpy as np
import pytest

import cluster_complete_case as ccc
import cluster_components_case as cpc
import cluster_tree_case as ctc

F = np.float32
LEVELS = ("0.76", "0.8", "0.85")


# ------------------------------------------------------------------ the restatement ----
def _random_multigraph(seed):
    """n in [1, 40] rows, up to 4 n directed entries between random rows (self-loops and duplicates in both directions among them)
    with weights from FOUR values, lengths from three values of which 60 / 100 fails coverage 0.7; a third of the entries sit in
    lists of k = 2, the rest are extras."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 41))
    m = int(rng.integers(0, 4 * n + 1))
    values = np.array([0.5, 0.6, 0.7, 0.8], F)
    lengths = rng.choice(np.array([60, 70, 100], np.int32), size=n)
    idx = rng.integers(0, n, size=(n, 2)).astype(np.int64)
    score = values[rng.integers(0, 4, size=(n, 2))]
    idx[rng.random((n, 2)) < 0.5] = -1
    src, dst = rng.integers(0, n, size=m).astype(np.int64), rng.integers(0, n, size=m).astype(np.int64)
    return idx, score, src, dst, values[rng.integers(0, 4, size=m)], lengths


def test_the_forest_cut_at_any_threshold_is_the_graph_cut_at_that_threshold():
    """200 seeded multigraphs, 5 thresholds each: ms_cluster_components restated on the forest's edges alone equals it on the full
    entries -- `rep`, the link score bit for bit, the count; and the forest has n - components edges."""
    many = 0
    for seed in range(200):
        idx, score, src, dst, esc, lengths = _random_multigraph(seed)
        n = lengths.shape[0]
        a, b, w, info = ctc.cluster_tree_np(idx, score, src, dst, esc, lengths, 0.5, 0.7)
        full = cpc.cluster_components_np(idx, score, src, dst, esc, lengths, 0.5, 0.7)
        assert len(a) == info["n_edges"] == n - full[2]["n_components"] and info["saturated"] == full[2]["saturated"], seed
        assert np.all(a < b) and len(ctc.forest_set(a, b, w)) == len(a)
        order = sorted(zip((-w.astype(np.float64)).tolist(), a.tolist(), b.tolist()))
        assert order == list(zip((-w.astype(np.float64)).tolist(), a.tolist(), b.tolist())), seed        # the forest's own order
        for level in (0.5, 0.55, 0.6, 0.7, 0.8):
            want = cpc.cluster_components_np(idx, score, src, dst, esc, lengths, level, 0.7)
            got = cpc.cluster_components_np(None, None, a, b, w, lengths, level, 0.7)
            assert np.array_equal(got[0], want[0]), (seed, level)
            assert np.array_equal(ccc.bits(got[1]), ccc.bits(want[1])), (seed, level)
            assert got[2]["n_components"] == want[2]["n_components"], (seed, level)
        many += len(a) > 3
    assert many > 100                                                      # (most graphs have a forest worth cutting)


def test_restatement_order_ties_and_directions():
    lengths = np.full(4, 10, np.int32)
    # a ring of four equal weights: the dropped edge is the last in the order, (2, 3)
    ring = (np.array([0, 1, 2, 3]), np.array([1, 2, 3, 0]), np.full(4, 0.8, F))
    a, b, w, info = ctc.cluster_tree_np(None, None, *ring, lengths, 0.5, 0.0)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1), (0, 3), (1, 2)] and info == {"n_edges": 3, "saturated": 0}
    # the weight of an edge is the larger of its directions; -0.0 counts as +0.0; an entry below the cut is none
    two = (np.array([0, 1, 2, 3]), np.array([1, 0, 3, 2]), np.array([0.6, 0.9, -0.0, -1.0], F))
    a, b, w, _info = ctc.cluster_tree_np(None, None, *two, lengths, -0.5, 0.0)
    assert ctc.forest_set(a, b, w) == {(0, 1, int(ccc.bits(F(0.9))[0])), (2, 3, 0)}


# ------------------------------------------------------------------ host-side refusals ----
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from merizo_search_amd import _lib
    _lib.build()
    lib = _lib.load()
    p = 0x1000                                                          # never dereferenced: the host checks come first
    f = ctypes.c_float
    ok = dict(idx=p, sc=p, n=100, k=5, src=p, dst=p, esc=p, m=7, lengths=p, min_score=0.5, mincov=0.7, pairs=p, weight=p, n_edges=p, rounds=p,
              saturated=p, ws=p, ws_bytes=1 << 20)

    def tree(**kw):
        a = dict(ok, **kw)
        return lib.ms_cluster_tree(a["idx"], a["sc"], a["n"], a["k"], a["src"], a["dst"], a["esc"], a["m"], a["lengths"], f(a["min_score"]),
                                   f(a["mincov"]), a["pairs"], a["weight"], a["n_edges"], a["rounds"], a["saturated"], a["ws"], a["ws_bytes"], None)

    need = int(lib.ms_cluster_tree_workspace_bytes(100))
    assert need >= 100 * (8 + 4 * 4 + 1) and need % 16 == 0
    assert [int(lib.ms_cluster_tree_workspace_bytes(n)) for n in (0, -1, 1 << 31)] == [0, 0, 0]
    assert int(lib.ms_cluster_tree_workspace_bytes((1 << 31) - 1)) > 25 * ((1 << 31) - 1)
    for name in ("idx", "sc", "src", "dst", "esc", "lengths", "pairs", "weight", "n_edges", "rounds", "saturated", "ws"):
        assert tree(**{name: None}) == -1, name
        assert b"NULL" in lib.ms_last_error() and b"ms_cluster_tree" in lib.ms_last_error()
    for bad in (dict(n=0), dict(n=-5), dict(n=1 << 31), dict(k=-1), dict(m=-1), dict(min_score=float("nan")), dict(mincov=-0.01), dict(mincov=1.01),
                dict(mincov=float("nan")), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=p + 8)):
        assert tree(**bad) == -1, bad
        assert b"ms_cluster_tree" in lib.ms_last_error(), bad
    # k == 0 with NULL lists and m == 0 with NULL edge arrays pass the pointer check (a short workspace stops them before any launch)
    assert tree(k=0, idx=None, sc=None, ws_bytes=0) == -1 and b"workspace" in lib.ms_last_error()
    assert tree(m=0, src=None, dst=None, esc=None, ws_bytes=0) == -1 and b"workspace" in lib.ms_last_error()
    assert lib.ms_version() == 210


@pytest.mark.parametrize("flags,words", [
    (["--cluster_mode", "connected", "--levels", "0.8,0.69"], "below -s/--mincos"),
    (["--cluster_mode", "connected", "--levels", "0.8,nan"], "NaN"),
    (["--cluster_mode", "connected", "--levels", "0.8,0.80"], "given twice"),
    (["--cluster_mode", "connected", "--levels", "0.8,high"], "not a number"),
    (["--tree"], "--cluster_mode connected"),
    (["--cluster_mode", "greedy", "--levels", "0.8"], "--cluster_mode connected"),
])
def test_cli_refuses_bad_levels_and_the_greedy_mode_before_any_database_is_opened(tmp_path, caplog, flags, words):
    """The database does not exist: a run that got as far as opening it would complain about THAT."""
    from merizo_search_amd import cli
    with pytest.raises(SystemExit) as exc:
        cli.main(["cluster", str(tmp_path / "nodb"), str(tmp_path / "o"), str(tmp_path / "t"), "-s", "0.7"] + flags)
    assert exc.value.code == 1 and words in caplog.text and "is not a valid db" not in caplog.text
    assert not os.path.exists(str(tmp_path / "o_cluster.tsv"))


# ------------------------------------------------------------------ the driver, oracle engine ----
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Per layout: the run with --levels at -k 40 and at -k 4 --complete, the run without --tree, and one separate run per level."""
    from merizo_search_amd.foldclass import cluster
    Engine = ctc.install_oracle_tree()
    work = str(tmp_path_factory.mktemp("cluster_tree"))
    names, _lengths, _group = cpc.write_chains(work)
    info = {}

    def run(name, db, mincos=cpc.MINCOS, **kw):
        info[name] = cluster.run_cluster(os.path.join(work, db), os.path.join(work, name), os.path.join(work, "tmp"), "cuda", mincos=mincos,
                                         mincov=0.7, header=True, engine=Engine(), mode="connected", **kw)[2]

    for db in ("cfa", "cpt"):
        run("tree_" + db, db, topk=40, levels=list(LEVELS))
        run("tree4_" + db, db, topk=4, complete=True, levels=list(LEVELS))
        run("plain_" + db, db, topk=40)
        for level in LEVELS:
            run("at%s_%s" % (level, db), db, mincos=float(level), topk=40)
    return work, names, info


def _read(work, name, suffix="_cluster.tsv"):
    return open(os.path.join(work, name + suffix), "rb").read()


def test_the_planting_fixes_the_counts_at_070_and_085():
    """With the generator's own arithmetic (float64 dot products of its rows): no cosine within 0.03 of 0.70 or of 0.85, so the
    components there are the planted ones whichever search path scores them -- 50 groups at 0.70; at 0.85 every chain link (0.75)
    is cut and every dumbbell bridge (0.80) too: 324 chain rows + 20 cliques = 344."""
    rows, group = cpc.chain_rows()
    cos = rows.astype(np.float64) @ rows.astype(np.float64).T
    off = cos[~np.eye(rows.shape[0], dtype=bool)]
    assert np.abs(off - 0.70).min() > 0.03 and np.abs(off - 0.85).min() > 0.03
    n = rows.shape[0]
    lengths = np.full(n, cpc.DOMAIN_LENGTH, np.int32)
    for level, want in ((0.70, 50), (0.85, 344)):
        a, b = np.nonzero((cos >= level) & ~np.eye(n, dtype=bool))
        assert cpc.cluster_components_np(None, None, a, b, cos[a, b].astype(F), lengths, level, 0.0)[2]["n_components"] == want
    assert 4 * sum(cpc.CHAIN_SIZES) + 2 * cpc.DUMBBELLS == 344


@pytest.mark.parametrize("layout", ["cfa", "cpt"])
def test_every_level_file_is_the_file_of_a_separate_run_at_that_mincos(runs, layout):
    work, _names, info = runs
    for name in ("tree_", "tree4_"):
        got = info[name + layout]
        assert got["n_components"] == 50 and got["levels"]["0.85"] == 344 and got["tree_edges"] == cpc.ROWS - 50
        assert list(got["levels"]) == list(LEVELS) and got["tree_rounds"] == 0          # (the oracle engine has no rounds)
        counts = [got["n_components"]] + [got["levels"][level] for level in LEVELS]
        assert counts == sorted(counts)
        for level in LEVELS:
            want = _read(work, "at%s_%s" % (level, layout))
            assert _read(work, name + layout, "_cluster_%s.tsv" % level) == want, (name, level)
            assert got["levels"][level] == info["at%s_%s" % (level, layout)]["n_components"]
            assert want.splitlines()[0] == b"representative\tmember\tlink_score" and want.count(b"\n") == cpc.ROWS + 1
        # the default file is the one a run without --tree writes
        assert _read(work, name + layout) == _read(work, "plain_" + layout)
    plain = info["plain_" + layout]
    assert "tree_edges" not in plain and "levels" not in plain and not os.path.exists(os.path.join(work, "plain_%s_cluster_tree.tsv" % layout))


@pytest.mark.parametrize("layout", ["cfa", "cpt"])
def test_the_tree_file_holds_the_forest_in_its_own_order(runs, layout):
    work, names, _info = runs
    row = {nm: r for r, nm in enumerate(names)}
    for name in ("tree_", "tree4_"):
        lines = _read(work, name + layout, "_cluster_tree.tsv").decode().splitlines()
        assert lines[0] == "member_a\tmember_b\tlink_score" and len(lines) == 1 + cpc.ROWS - 50
        edges = [(F(w), row[a], row[b]) for a, b, w in (line.split("\t") for line in lines[1:])]
        assert all(a < b for _w, a, b in edges) and all(w >= F(cpc.MINCOS) for w, _a, _b in edges)
        assert edges == sorted(edges, key=lambda e: (-float(e[0]), e[1], e[2]))
        assert all("%.9g" % w == text.split("\t")[2] for (w, _a, _b), text in zip(edges, lines[1:]))       # a float32 round-trips
        # cutting the FILE at 0.85 gives the 344 components
        a = np.array([e[1] for e in edges], np.int64)
        b = np.array([e[2] for e in edges], np.int64)
        w = np.array([e[0] for e in edges], F)
        cut = cpc.cluster_components_np(None, None, a, b, w, np.full(cpc.ROWS, cpc.DOMAIN_LENGTH, np.int32), 0.85, 0.7)
        assert cut[2]["n_components"] == 344
    assert _read(work, "tree_" + layout, "_cluster_tree.tsv") == _read(work, "tree4_" + layout, "_cluster_tree.tsv")


def test_tree_without_levels_and_numbers_as_levels(runs, tmp_path):
    from merizo_search_amd.foldclass import cluster
    Engine = ctc.install_oracle_tree()
    work = runs[0]
    run = lambda out, **kw: cluster.run_cluster(os.path.join(work, "cfa"), str(tmp_path / out), str(tmp_path / "t"), "cuda", topk=40,
                                                mincos=cpc.MINCOS, mincov=0.7, engine=Engine(), mode="connected", **kw)[2]
    info = run("only", tree=True)
    assert info["tree_edges"] == cpc.ROWS - 50 and info["levels"] == {}
    assert open(str(tmp_path / "only_cluster_tree.tsv")).read().count("\n") == cpc.ROWS - 50     # no header line
    info = run("num", levels=[0.85])
    assert info["levels"] == {"0.85": 344} and os.path.exists(str(tmp_path / "num_cluster_0.85.tsv"))
    for bad in (dict(levels=[0.5]), dict(levels=[float("nan")]), dict(levels=[0.8, 0.8])):
        with pytest.raises(SystemExit):
            run("bad", **bad)
    with pytest.raises(SystemExit):
        cluster.run_cluster(os.path.join(work, "cfa"), str(tmp_path / "bad"), str(tmp_path / "t"), "cuda", topk=40, mincos=cpc.MINCOS,
                            engine=Engine(), tree=True)
    assert not os.path.exists(str(tmp_path / "bad_cluster.tsv"))
