"""The best-mapping report without a GPU: the restatement of ms_md_best_mappings (best_mapping_case) against brute force over
chain_mappings' own enumeration, its fixed cases and its quantiser; best_lines and its writer on crafted outputs; the command
line of `--multi_domain_report`."""
import itertools
import logging

import numpy as np
import pytest

import best_mapping_case as bm


def _paths(m):
    """The one-to-one paths chain_mappings enumerates for a matrix (the product of the rows' non-zero columns)."""
    from merizo_search_amd.foldclass import multidomain as md
    m = np.asarray(m, np.float32)
    nqd, nhd = m.shape
    lines = md.chain_mappings(m, "q", "h", ["q%d" % i for i in range(nqd)], [{"hd": "%d" % j, "hm": "{ }"} for j in range(nhd)])
    return [[int(e.split(":")[1]) for e in l[5].split(",")] for l in lines]


# ------------------------------------------------------------------ 1. the restatement ---
def test_the_restatement_finds_the_brute_force_optimum_of_both_kinds():
    """300 random matrices, nqd 1-5, nhd nqd-8, half the cells zero, values on the grid k / 64 with negatives (ties are common):
    feasibility and the integer totals equal the maximum over chain_mappings' enumeration; the paths are valid."""
    rng = np.random.default_rng(5)
    seen = {(k, f): 0 for k in (0, 1) for f in (0, 1)}
    for _ in range(300):
        nqd = int(rng.integers(1, 6))
        nhd = int(rng.integers(nqd, 9))
        m = (rng.integers(-64, 65, (nqd, nhd)) / 64.0).astype(np.float32) * (rng.random((nqd, nhd)) < 0.5)
        allowed, w = bm.quantise(m)
        paths = _paths(m)
        totals = [sum(int(w[i, j]) for i, j in enumerate(p)) for p in paths]
        ordered = [t for p, t in zip(paths, totals) if all(b > a for a, b in zip(p, p[1:]))]
        assert bm.brute_force(m) == [max(totals) if totals else None, max(ordered) if ordered else None]
        for kind, (solve, pool) in enumerate(((bm.best_any, totals), (bm.best_ordered, ordered))):
            st, tot, p = solve(m)
            seen[kind, st] += 1
            assert st == (1 if pool else 0), (m, kind)
            if st:
                assert tot == max(pool), (m, kind, tot, max(pool), p)
                assert len(set(p)) == nqd and all(allowed[i, j] for i, j in enumerate(p)), (m, kind, p)
                assert tot == sum(int(w[i, j]) for i, j in enumerate(p))
                if kind == 1:
                    assert all(b > a for a, b in zip(p, p[1:])), (m, p)
            else:
                assert tot == 0 and p == []
    assert min(seen.values()) >= 20, seen                      # both verdicts of both kinds occur


def test_fixed_cases():
    hall = np.asarray([[.9, 0, 0], [.8, 0, 0], [0, .7, .6]], np.float32)     # every row and three columns are non-zero: no mapping
    assert bm.best_any(hall) == (0, 0, []) and bm.best_ordered(hall) == (0, 0, [])
    assert _paths(hall) == []
    m = np.asarray([[.9, .8], [.9, .1]], np.float32)
    w = bm.quantise(m)[1]
    assert bm.best_any(m) == (1, int(w[0, 1] + w[1, 0]), [1, 0])
    assert abs(bm.best_any(m)[1] / 2.0 ** 32 - 1.7) < 1e-6
    assert bm.best_ordered(m) == (1, int(w[0, 0] + w[1, 1]), [0, 1])
    # the tie rules: all cells equal -> the identity for both kinds
    assert bm.best_any(np.full((3, 5), 0.75, np.float32))[2] == [0, 1, 2]
    assert bm.best_ordered(np.full((3, 5), 0.75, np.float32))[2] == [0, 1, 2]
    # more query domains than target domains
    assert bm.best_any(np.ones((3, 2), np.float32))[0] == 0 and bm.best_ordered(np.ones((3, 2), np.float32))[0] == 0


def test_the_quantiser():
    cells = np.asarray([2.0 ** -9, 2.0 ** -40, -0.0, np.inf, np.nan, 3 * 2.0 ** 19, -np.inf, 0.5, -(2.0 ** -9)], np.float32)
    allowed, w = bm.quantise(cells)
    assert allowed.tolist() == [True, True, False, True, False, True, True, True, True]
    assert w.tolist() == [2 ** 23, 0, 0, 2 ** 52, 0, 2 ** 52, -(2 ** 52), 2 ** 31, -(2 ** 23)]
    # every float32 in [2^-9, 2^20] is a multiple of 2^-32: its weight is exact
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(2.0 ** -9, 1.0, 1000), rng.uniform(1.0, 2.0 ** 20, 1000)]).astype(np.float32)
    assert np.array_equal(bm.quantise(x)[1].astype(np.float64) / 2.0 ** 32, x.astype(np.float64))
    # nearest even at a half: 2^-33 * (2 k + 1) -> the even neighbour
    assert bm.quantise(np.asarray([2.0 ** -33, 3 * 2.0 ** -33], np.float32))[1].tolist() == [0, 2]


def test_the_entry_point_statuses_and_fills():
    scores = np.arange(1, 13, dtype=np.float32) / 16
    cand = [(0, 2, 0, 3), (0, 65, 0, 1), (0, 1, 0, 1025), (0, 0, 0, 3), (0, 2, 0, -1), (0, 3, 0, 4), (0, 2, 0, 3), (0, 65, 0, 3)]
    off = [0, 0, 0, 0, 0, 1, -1, 10 ** 9]
    st, tot, path, cell = bm.best_mappings(scores, cand, off)
    assert st[:, 0].tolist() == [1, -2, -2, -1, -1, -1, -1, -2] and np.array_equal(st[:, 0], st[:, 1])
    assert (tot[1:] == 0).all() and (path[1:] == -1).all() and (cell[1:] == 0).all()
    # [[1, 2, 3], [4, 5, 6]] / 16: (2, 1) and (1, 2) tie at 8 / 16; row 0 took its best column, row 1 found column 1 free
    assert path[0, 0, :2].tolist() == [2, 1] and path[0, 1, :2].tolist() == [1, 2] and (path[0, :, 2:] == -1).all()
    assert tot[0].tolist() == [2 ** 31, 2 ** 31]
    assert cell[0, 0, :2].tolist() == [scores[2], scores[4]] and cell[0, 1, :2].tolist() == [scores[1], scores[5]]
    assert (cell[0, :, 2:] == 0).all()


# ------------------------------------------------------------------ 2. lines and writer ---
class _Store:
    def name_meta(self, row):
        self.read.append(row)
        return "t%d" % row, '{ "row": %d }' % row

    def __init__(self):
        self.read = []


def test_best_lines_order_second_line_and_the_limit(tmp_path, caplog):
    """Three pairs of one query chain and one of another: ordered by the kind-0 integer total within a query chain (ties in plan
    order); a second line only where the first has category 0 and kind 1 found a mapping; a pair with status -2 is logged and
    skipped; names and metadata are read for reported columns only."""
    from merizo_search_amd.foldclass import multidomain as md
    from merizo_search_amd.foldclass import results
    mats = [np.asarray([[.9, .8, 0], [.9, .1, 0]], np.float32),         # any order (1, 0) = 1.7; ordered (0, 1) = 1.0
            np.asarray([[.9, 0], [0, .95]], np.float32),                # (0, 1) = 1.85: category 3
            np.asarray([[0, .6], [.7, 0]], np.float32),                 # (1, 0) only: category 0, no second line
            np.asarray([[.5, 0, .5], [0, 0, .5]], np.float32),          # no pair of the other chain beats it in its own block
            np.asarray([[.5, 0], [.5, 0]], np.float32)]                 # no mapping
    rows = [np.arange(10, 13), np.arange(20, 22), np.arange(30, 32), np.arange(40, 43), np.arange(50, 52)]
    plans = [("qA", "h%d" % c, 0, 2, rows[c]) for c in range(3)] + [("qB", "h3", 2, 2, rows[3]), ("qB", "h4", 2, 2, rows[4])]
    plans.append(("qB", "h5", 2, 2, np.arange(60, 62)))
    hits = {"qA": {"a1": [], "a2": []}, "qB": {"b1": [], "b2": []}}
    cand = [(0, 2, 0, m.shape[1]) for m in mats] + [(0, 2, 0, 2000)]
    off = np.cumsum([0] + [m.size for m in mats])
    st, tot, path, cell = bm.best_mappings(np.concatenate([m.ravel() for m in mats]), cand, off)
    assert st[:, 0].tolist() == [1, 1, 1, 1, 0, -2]
    store, skipped = _Store(), []
    with caplog.at_level(logging.WARNING):
        lines = md.best_lines(plans, hits, store, st, tot, path, cell, skipped=skipped)
    assert "qB x hit chain h5" in caplog.text and skipped == [("qB", "h5", -2)]
    f32 = lambda x: str(np.float32(x))
    assert lines == [
        ("qA", 2, "h1", 2, 3, "%.6f" % (float(np.float32(.9)) + float(np.float32(.95))), "a1:t20:%s,a2:t21:%s" % (f32(.9), f32(.95)),
         '[{ "row": 20 },{ "row": 21 }]'),
        ("qA", 2, "h0", 3, 0, "%.6f" % (float(np.float32(.8)) + float(np.float32(.9))), "a1:t11:%s,a2:t10:%s" % (f32(.8), f32(.9)),
         '[{ "row": 11 },{ "row": 10 }]'),
        ("qA", 2, "h0", 3, 2, "%.6f" % (float(np.float32(.9)) + float(np.float32(.1))), "a1:t10:%s,a2:t11:%s" % (f32(.9), f32(.1)),
         '[{ "row": 10 },{ "row": 11 }]'),
        ("qA", 2, "h2", 2, 0, "%.6f" % (float(np.float32(.6)) + float(np.float32(.7))), "a1:t31:%s,a2:t30:%s" % (f32(.6), f32(.7)),
         '[{ "row": 31 },{ "row": 30 }]'),
        ("qB", 2, "h3", 3, 1, "1.000000", "b1:t40:0.5,b2:t42:0.5", '[{ "row": 40 },{ "row": 42 }]')]
    assert sorted(store.read) == [10, 11, 20, 21, 30, 31, 40, 42]
    out = str(tmp_path / "best.tsv")
    results.multi_dom_writer("best")(lines, out, True)
    text = open(out).read().splitlines()
    assert text[0].split("\t") == ["query_chain", "nqd", "hit_chain", "nhd", "match_category", "match_score", "match_info", "hit_metadata"]
    assert [l.split("\t") for l in text[1:]] == [[str(a) for a in l] for l in lines]
    assert results.multi_dom_writer("all") is results.write_all_dom_search_results


def test_the_category_helper_is_chain_mappings_rule():
    from merizo_search_amd.foldclass import multidomain as md
    for nqd, nhd in ((1, 1), (1, 3), (2, 2), (2, 4), (3, 3), (3, 5)):
        m = np.ones((nqd, nhd), np.float32)
        lines = md.chain_mappings(m, "q", "h", ["q%d" % i for i in range(nqd)], [{"hd": "%d" % j, "hm": "{ }"} for j in range(nhd)])
        want = [p for p in itertools.product(range(nhd), repeat=nqd) if len(set(p)) == nqd]
        assert [l[4] for l in lines] == [md.mapping_category(p, nhd) for p in want]
    assert md.mapping_category([4], 7) == 2 and md.mapping_category([0], 1) == 3
    assert [md.mapping_category(p, 4) for p in ([0, 1, 2], [1, 2, 3], [0, 1, 3], [0, 2, 1])] == [2, 2, 1, 0]


# ------------------------------------------------------------------ 3. the command line ---
def test_best_with_exhaustive_tmalign_is_refused_before_any_work(tmp_path, caplog, monkeypatch):
    from merizo_search_amd import _lib, cli
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU call was made"))
    for mode, argv in (("search", ["a.pdb"]), ("easy-search", ["a.pdb", "--chopping", "1-10"])):
        caplog.clear()
        with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as exc:
            cli.main([mode, argv[0], str(tmp_path / "no_such_db"), str(tmp_path / "o"), str(tmp_path / "t")] + argv[1:] +
                     ["--multi_domain_search", "--multi_domain_mode", "exhaustive_tmalign", "--multi_domain_report", "best"])
        assert exc.value.code not in (0, None)
        assert "exhaustive_cosine" in caplog.text and "database_cosine" in caplog.text, caplog.text
    from merizo_search_amd.foldclass import multidomain as md
    with pytest.raises(ValueError, match="exhaustive_cosine and database_cosine"):
        md.multi_domain_search(["a", "b"], [], "db", "tmp", mode="exhaustive_tmalign", report="best")
    with pytest.raises(ValueError, match="Unrecognised multi-domain report"):
        md.multi_domain_search(["a", "b"], [], "db", "tmp", mode="exhaustive_cosine", report="top")
    md.check_report("best", "exhaustive_cosine")
    md.check_report("best", "database_cosine")
    md.check_report("all", "exhaustive_tmalign")


def test_the_flag_parses_in_the_four_commands(capsys):
    import argparse
    from merizo_search_amd import cli
    p = cli.chain_search_parser()
    assert p.parse_args(["q", "t", "o", "tmp"]).multi_domain_report == "all"
    assert p.parse_args(["q", "t", "o", "tmp", "--multi_domain_report", "best"]).multi_domain_report == "best"
    with pytest.raises(SystemExit):
        p.parse_args(["q", "t", "o", "tmp", "--multi_domain_report", "top"])
    assert "invalid choice" in capsys.readouterr().err
    q = argparse.ArgumentParser()
    cli._add_search_flags(q, "query")
    assert q.parse_args([]).multi_domain_report == "all" and q.parse_args(["--multi_domain_report", "best"]).multi_domain_report == "best"
    for mode, argv in (("search", ["a.pdb", "db", "out", "tmp"]), ("easy-search", ["a.pdb", "db", "out", "tmp", "--chopping", "1-10"]),
                       ("db-search", ["q", "t", "out", "tmp"]), ("chain-search", ["q", "t", "out", "tmp"])):
        with pytest.raises(SystemExit) as exc:
            cli.main([mode] + argv + ["--multi_domain_report", "top"])
        assert exc.value.code == 2
        assert "--multi_domain_report" in capsys.readouterr().err


def test_the_drivers_refuse_an_unknown_report_before_any_gpu_work(tmp_path):
    from merizo_search_amd.foldclass import chainsearch, dbsearch

    class Engine:                                               # (never touched: the refusals come first)
        pass

    with pytest.raises(SystemExit):
        chainsearch.run_chain_search("q", "t", str(tmp_path / "o"), str(tmp_path / "t"), engine=Engine(), report="top")
    with pytest.raises(SystemExit):
        dbsearch.run_dbsearch_db("q", "t", str(tmp_path / "o"), str(tmp_path / "t"), engine=Engine(), multi_domain_search=True,
                                 multi_domain_report="top")
