"""`cluster --mintm` without a GPU: the restatements of the three pair calls on hand-built cases, the host-side refusals of the new
entry points, and the driver with the oracle engine (the aligner: the CPU restatement of TM-align) on the planted structure
families -- both layouts, greedy and connected, -k 3 --complete against -k 8, fast mode: every row goes to the longest member of its
STRUCTURE family, impostors stay alone, the embedding family of eight comes out as two clusters.  Without --mintm the command
writes what it wrote."""
import ctypes
import logging
import os

import numpy as np
import pytest

import cluster_case as cc
import cluster_tm_case as ct

F = np.float32


# ------------------------------------------------------------------ the restatements ----
def test_restatement_pairs_are_canonical_distinct_and_independent_of_the_layout():
    lengths = np.array([10, 30, 20, 20, 5], np.int32)
    edges = [(0, 1, 0.9), (1, 0, 0.8), (2, 3, 0.7), (3, 2, 0.7), (4, 4, 0.9), (0, 9, 0.9), (2, 1, float("nan")), (1, 2, 0.2)]
    idx, score = cc.lists_from_edges(5, 2, edges)
    pairs, saturated = ct.cluster_pairs_np(idx, score, None, None, None, lengths, 0.5, 0.0)
    assert pairs.tolist() == [[1, 0], [2, 3]] and saturated == 0         # (the longer row first; the smaller row on equal length)
    src, dst, sc = (np.array(x) for x in zip(*edges))
    extras, zero = ct.cluster_pairs_np(None, None, src, dst, sc.astype(F), lengths, 0.5, 0.0)
    assert {tuple(p) for p in extras.tolist()} == {(1, 0), (2, 3)} and zero == 0
    assert ct.cluster_pairs_np(idx, score, None, None, None, lengths, 0.5, 0.7)[0].tolist() == [[2, 3]]      # 10 < 0.7 * 30
    assert ct.pairs_find_np([0, 1, 3, 2, 0, 7, 1], [1, 0, 2, 3, 0, 1, 2], lengths, pairs).tolist() == [0, 0, 1, 1, -1, -1, -1]


def test_restatement_apply_removes_both_directions_and_leaves_invalid_bits():
    lengths = np.array([10, 30, 20, 20, 5], np.int32)
    nan = np.array([0x7fc01234], np.uint32).view(F)[0]                   # a NaN with a payload
    edges = [(0, 1, 0.9), (1, 0, 0.8), (2, 3, 0.7), (3, 2, 0.7), (4, 4, 0.9), (0, 9, 0.9), (2, 1, nan)]
    idx, score = cc.lists_from_edges(5, 2, edges)
    pairs, _sat = ct.cluster_pairs_np(idx, score, None, None, None, lengths, 0.5, 0.0)
    new_idx, new_score, _d, _e, removed = ct.pairs_apply_np(idx, score, None, None, None, lengths, 0.5, 0.0, pairs, [0, 1])
    assert removed == 2 and new_idx[0, 0] == -1 and new_idx[1, 0] == -1 and new_score[0, 0] == -np.inf
    untouched = np.ones_like(idx, bool)
    untouched[0, 0] = untouched[1, 0] = False
    assert np.array_equal(new_idx[untouched], idx[untouched]) and np.array_equal(new_score.view(np.uint32)[untouched], score.view(np.uint32)[untouched])
    # fail closed: a keep vector shorter than the set, and a set that lacks the pair
    assert ct.pairs_apply_np(idx, score, None, None, None, lengths, 0.5, 0.0, pairs, [1])[4] == 2
    assert ct.pairs_apply_np(idx, score, None, None, None, lengths, 0.5, 0.0, pairs[:1], [1, 1])[4] == 2
    assert ct.pairs_apply_np(idx, score, None, None, None, lengths, 0.5, 0.0, pairs, [1, 1])[4] == 0


# ------------------------------------------------------------------ host-side refusals of the C entries ----
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from merizo_search_amd import _lib
    _lib.build()
    lib = _lib.load()
    p, f = 0x1000, ctypes.c_float                                         # never dereferenced: the host checks come first
    size = lambda n, k, m: int(lib.ms_cluster_pairs_workspace_bytes(n, k, m))
    assert size(100, 5, 7) == 64 + 12 * 1024 and size(1, 0, 0) == 64 + 12 * 64 and size(100, 5, 7) % 16 == 0
    assert [size(0, 1, 0), size(-1, 1, 0), size(1 << 31, 1, 0), size(5, -1, 0), size(5, 1, -1), size(1 << 30, 2, 0), size(5, 0, 1 << 31),
            size((1 << 30) - 1, 2, 2)] == [0] * 8
    assert size((1 << 30) - 1, 2, 1) == 64 + 12 * (1 << 32)
    ok = dict(idx=p, sc=p, n=100, k=5, src=p, dst=p, esc=p, m=7, lengths=p, min_score=0.5, mincov=0.7, pairs=p, cap=10, count=p, ws=p,
              ws_bytes=1 << 20, keep=p, removed=p)

    def pairs(**kw):
        a = dict(ok, **kw)
        return lib.ms_cluster_pairs(a["idx"], a["sc"], a["n"], a["k"], a["src"], a["dst"], a["esc"], a["m"], a["lengths"], f(a["min_score"]),
                                    f(a["mincov"]), a["pairs"], a["cap"], a["count"], a["ws"], a["ws_bytes"], None)

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.ms_cluster_pairs_apply(a["idx"], a["sc"], a["n"], a["k"], a["src"], a["dst"], a["esc"], a["m"], a["lengths"], f(a["min_score"]),
                                          f(a["mincov"]), a["keep"], a["cap"], a["ws"], a["ws_bytes"], a["removed"], None)

    for call, who, own in ((pairs, b"ms_cluster_pairs", ("pairs", "count")), (apply, b"ms_cluster_pairs_apply", ("keep", "removed"))):
        for name in ("idx", "sc", "src", "dst", "esc", "lengths", "ws") + own:
            assert call(**{name: None}) == -1 and b"NULL" in lib.ms_last_error() and who in lib.ms_last_error(), name
        for bad in (dict(n=0), dict(n=-5), dict(n=1 << 31), dict(k=-1), dict(m=-1), dict(min_score=float("nan")), dict(mincov=-0.01),
                    dict(mincov=1.01), dict(mincov=float("nan")), dict(cap=-1), dict(ws=p + 8)):
            assert call(**bad) == -1 and who in lib.ms_last_error(), bad
        assert call(ws_bytes=size(100, 5, 7) - 1) == -2 and b"workspace" in lib.ms_last_error()
        assert call(n=1 << 30, k=2) == -4 and call(m=1 << 31) == -4 and b"2^31" in lib.ms_last_error()
        # k == 0 with NULL lists and m == 0 with NULL edge arrays pass the pointer check (a short workspace stops them before any launch)
        assert call(k=0, idx=None, sc=None, ws_bytes=0) == -2 and call(m=0, src=None, dst=None, esc=None, ws_bytes=0) == -2
    assert pairs(cap=0, pairs=None, ws_bytes=0) == -2                     # (cap == 0 only counts: no pair buffer needed)
    find = lambda a=p, b=p, cnt=3, lengths=p, n=100, ws=p, ws_bytes=1 << 20, out=p: lib.ms_cluster_pairs_find(a, b, cnt, lengths, n, ws,
                                                                                                              ws_bytes, out, None)
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(lengths=None), dict(ws=None), dict(cnt=-1), dict(n=0), dict(n=1 << 31),
               dict(ws=p + 8)):
        assert find(**kw) == -1 and b"ms_cluster_pairs_find" in lib.ms_last_error(), kw
    assert find(ws_bytes=size(1, 0, 0) - 1) == -2
    assert find(cnt=0, a=None, b=None, out=None) == 0                     # (nothing to find: no launch)
    assert lib.ms_version() == 210


# ------------------------------------------------------------------ the driver, oracle engine ----
@pytest.fixture(scope="module")
def families(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_tm"))
    names, built = ct.write_structured(work)
    return work, names, built


def _run(work, db, out, caplog=None, **kw):
    from merizo_search_amd.foldclass import cluster
    Engine = ct.install_oracle_cluster_tm()
    kw.setdefault("topk", ct.K_ALL)
    kw.setdefault("mincov", ct.MINCOV)
    return cluster.run_cluster(os.path.join(work, db), os.path.join(work, out), os.path.join(work, "tmp"), "cuda", mincos=ct.MINCOS,
                               header=True, engine=Engine(), **kw)


def _tsv(work, out):
    return open(os.path.join(work, out + "_cluster.tsv"), "rb").read()


def _expected_tsv(names, rep, rep_score, tm_score, score_name="emb_score"):
    rows = np.arange(rep.shape[0])
    lines = ["representative\tmember\t%s%s" % (score_name, "" if tm_score is None else "\ttm_score")]
    for r in np.lexsort((rows, rows != rep, rep)):
        lines.append("\t".join([names[rep[r]], names[r], "{:.4f}".format(rep_score[r])] + ([] if tm_score is None else ["{:.4f}".format(tm_score[r])])))
    return ("\n".join(lines) + "\n").encode()


def test_the_fixture_has_its_twists(families):
    _work, _names, built = families
    efam, sfam, lengths, rep = built["efam"], built["sfam"], built["lengths"], built["rep"]
    n = lengths.shape[0]
    assert 95 <= n <= 110 and (sfam < 0).sum() == ct.IMPOSTORS
    for t in range(ct.IMPOSTORS):
        r = int(np.nonzero(sfam == -1 - t)[0][0])
        others = lengths[(efam == efam[r]) & (np.arange(n) != r)]
        assert (lengths[r] > others.max()) == (t < ct.LONGEST_IMPOSTORS) and rep[r] == r
    double = np.nonzero(efam == len(ct.FAMILY_SIZES))[0]
    assert double.shape[0] == 8 and np.unique(sfam[double]).shape[0] == 2 and np.unique(rep[double]).shape[0] == 2
    sizes = np.bincount(sfam[sfam >= 0])
    assert sizes.min() == 4 and sizes.max() == 6


@pytest.mark.parametrize("layout", ["sfa", "spt"])
def test_mintm_clusters_by_structure_family_in_both_modes(families, layout, caplog):
    work, names, built = families
    n = built["lengths"].shape[0]
    want_rep, want_score, want_tm, want_info = ct.pipeline_np(built)
    assert np.array_equal(want_rep, built["rep"])                         # the numpy pipeline finds the planted structure families
    with caplog.at_level(logging.INFO):
        rep, score, info = _run(work, layout, "greedy_" + layout, mintm=ct.MINTM)
    assert np.array_equal(rep, built["rep"]) and info["n_reps"] == np.unique(built["sfam"]).shape[0] and info["mode"] == "greedy"
    assert info["singletons"] == ct.IMPOSTORS
    for key in ("tm_pairs", "tm_rejected_pairs", "tm_removed_entries", "saturated"):
        assert info[key] == want_info[key], key
    assert info["tm_unaligned_pairs"] == 0 and info["tm_removed_entries"] == 2 * info["tm_rejected_pairs"] > 0
    assert "TM-align on %d distinct pairs" % info["tm_pairs"] in caplog.text and "residues or fewer" not in caplog.text
    text = _tsv(work, "greedy_" + layout)
    assert text.splitlines()[0] == b"representative\tmember\temb_score\ttm_score" and text.count(b"\n") == n + 1
    if layout == "sfa":                                                   # (the `.pt` layout's cosines may differ in the last printed digit)
        assert np.array_equal(score.view(np.uint32), want_score.view(np.uint32))
        assert text == _expected_tsv(names, want_rep, want_score, want_tm)
    column = {line.split("\t")[1]: line.split("\t")[3] for line in text.decode().splitlines()[1:]}
    assert [column[nm] for nm in names] == ["{:.4f}".format(v) for v in want_tm]
    assert all((column[names[r]] == "1.0000") == (rep[r] == r) for r in range(n))
    assert min(float(column[names[r]]) for r in range(n)) >= ct.TM_SAME
    # connected: the same partition (every structure family is a clique of verified edges), three columns
    c_rep, c_link, c_info = _run(work, layout, "connected_" + layout, mintm=ct.MINTM, mode="connected")
    assert np.array_equal(c_rep, built["rep"]) and c_info["n_components"] == info["n_reps"] and c_info["tm_pairs"] == info["tm_pairs"]
    c_want = ct.pipeline_np(built, mode="connected")
    assert np.array_equal(c_rep, c_want[0])
    c_text = _tsv(work, "connected_" + layout)
    assert c_text.splitlines()[0] == b"representative\tmember\tlink_score"
    if layout == "sfa":
        assert c_text == _expected_tsv(names, c_want[0], c_want[1], None, "link_score")


def test_without_mintm_the_impostors_join_and_the_double_family_is_one_cluster(families):
    work, _names, built = families
    rep, _score, info = _run(work, "sfa", "cosine_only")
    assert info["n_reps"] == len(ct.FAMILY_SIZES) + 1 and "tm_pairs" not in info
    assert _tsv(work, "cosine_only").splitlines()[0] == b"representative\tmember\temb_score"
    assert not np.array_equal(rep, built["rep"])
    longest = [int(np.nonzero(built["sfam"] == -1 - t)[0][0]) for t in range(ct.LONGEST_IMPOSTORS)]
    assert all(rep[r] == r and (rep == r).sum() > 1 for r in longest)     # an impostor REPRESENTS a family it does not belong to


@pytest.mark.parametrize("layout", ["sfa", "spt"])
def test_k3_complete_writes_the_k8_file_and_fastmode_the_same_partition(families, layout):
    work, _names, built = families
    for mode in ("greedy", "connected"):
        _run(work, layout, "k8_%s_%s" % (mode, layout), mintm=ct.MINTM, mode=mode)
        _rep, _score, info = _run(work, layout, "k3c_%s_%s" % (mode, layout), mintm=ct.MINTM, mode=mode, topk=3, complete=True)
        assert _tsv(work, "k3c_%s_%s" % (mode, layout)) == _tsv(work, "k8_%s_%s" % (mode, layout)), mode
        assert info["edges"] > 0 and info["saturated"] > 0 and info["tm_rejected_pairs"] == ct.pipeline_np(built)[3]["tm_rejected_pairs"]
        rep, _score, cut = _run(work, layout, "k3_%s_%s" % (mode, layout), mintm=ct.MINTM, mode=mode, topk=3)
        assert cut["saturated"] == info["saturated"] and cut["tm_pairs"] < info["tm_pairs"]
    rep, _score, info = _run(work, layout, "fast_" + layout, mintm=ct.MINTM, fastmode=True, tm_batchsize=50)
    assert np.array_equal(rep, built["rep"]) and np.array_equal(rep, ct.pipeline_np(built, fast=True)[0])


def test_mintm_none_writes_what_the_old_signature_writes(tmp_path):
    """cluster_case's planted database through the signature the parent commit has (no mintm argument) and with mintm=None,
    fastmode and tm_batchsize given: one file, byte for byte, the same info keys -- greedy, connected, complete."""
    from merizo_search_amd.foldclass import cluster
    Engine = ct.install_oracle_cluster_tm()
    work = str(tmp_path / "db")
    cc.write_planted(work)
    run = lambda out, **kw: cluster.run_cluster(os.path.join(work, "fa"), str(tmp_path / out), str(tmp_path / "t"), "cuda", topk=4,
                                                mincos=cc.PLANTED_MINCOS, mincov=0.7, header=True, engine=Engine(), **kw)
    for kw in (dict(), dict(mode="connected"), dict(complete=True)):
        _rep, _score, old = run("old", **kw)
        _rep, _score, new = run("new", mintm=None, fastmode=True, tm_batchsize=7, **kw)
        assert open(str(tmp_path / "old_cluster.tsv"), "rb").read() == open(str(tmp_path / "new_cluster.tsv"), "rb").read()
        assert old == new and not any(key.startswith("tm_") for key in new)


@pytest.mark.parametrize("bad", [float("nan"), 0.0, 1.5, -0.2])
def test_mintm_outside_its_range_is_refused_before_anything_is_read(tmp_path, caplog, bad):
    from merizo_search_amd.foldclass import cluster
    Engine = ct.install_oracle_cluster_tm()
    with pytest.raises(SystemExit):
        cluster.run_cluster(str(tmp_path / "nodb"), str(tmp_path / "o"), str(tmp_path / "t"), "cuda", mincos=0.7, engine=Engine(), mintm=bad)
    assert "--mintm must lie in (0, 1]" in caplog.text and not os.path.exists(str(tmp_path / "o_cluster.tsv"))


def test_chains_tm_align_cannot_score_are_rejected_with_one_warning(tmp_path, caplog):
    """An impostor with a NaN coordinate and a family member cut down to 5 residues: their pairs are not aligned, count as rejected,
    one warning says how many, both rows end up alone and everything else clusters as before."""
    built = ct.structured()
    bad = int(np.nonzero(built["sfam"] == -1)[0][0])
    short = int(np.nonzero(built["sfam"] == 5)[0][0])

    def edit(coords, seqs, _built):
        coords[bad][3, 1] = np.nan
        coords[short], seqs[short] = coords[short][:5].copy(), seqs[short][:5]

    work = str(tmp_path / "db")
    ct.write_structured(work, edit=edit)
    with caplog.at_level(logging.WARNING):
        rep, _score, info = _run(work, "sfa", "odd", mintm=ct.MINTM, mincov=0.0)
    degree = lambda r: int((built["efam"] == built["efam"][r]).sum()) - 1
    assert info["tm_unaligned_pairs"] == degree(bad) + degree(short)
    assert caplog.text.count("residues or fewer") == 1 and "%d of %d pairs" % (info["tm_unaligned_pairs"], info["tm_pairs"]) in caplog.text
    assert rep[bad] == bad and rep[short] == short and (rep == short).sum() == 1
    others = np.array([r for r in range(rep.shape[0]) if built["sfam"][r] != 5])
    assert np.array_equal(rep[others], built["rep"][others])


def test_a_row_without_coordinates_is_refused(families, tmp_path, caplog):
    """The `.pt` layout's index with one entry's coordinates taken out: the run says which row and writes nothing."""
    import pickle
    import shutil
    work, _names, built = families
    for ext in (".pt", ".index"):
        shutil.copy(os.path.join(work, "spt" + ext), str(tmp_path / ("nocoords" + ext)))
    with open(str(tmp_path / "nocoords.index"), "rb") as handle:
        index = pickle.load(handle)
    row = int(np.nonzero(built["sfam"] == 2)[0][0])
    index[row] = (index[row][0], None) + tuple(index[row][2:])
    with open(str(tmp_path / "nocoords.index"), "wb") as handle:
        pickle.dump(index, handle)
    with pytest.raises(SystemExit):
        _run(str(tmp_path), "nocoords", "none", mintm=ct.MINTM)
    assert "database row %d has none" % row in caplog.text and not os.path.exists(str(tmp_path / "none_cluster.tsv"))
    _run(str(tmp_path), "nocoords", "cosine")                             # (without --mintm the coordinates are never read)
    assert os.path.exists(str(tmp_path / "cosine_cluster.tsv"))


def test_cli_takes_mintm_and_fastmode(tmp_path, capsys):
    from merizo_search_amd import cli
    with pytest.raises(SystemExit) as exc:
        cli.main(["cluster", str(tmp_path / "nodb"), str(tmp_path / "o"), str(tmp_path / "t"), "-s", "0.7", "-m", "half"])
    assert exc.value.code == 2 and "--mintm" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        cli.main(["cluster", "--help"])
    text = capsys.readouterr().out
    assert exc.value.code == 0 and "-m MINTM, --mintm MINTM" in text and "-f, --fastmode" in text
