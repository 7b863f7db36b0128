"""`--multi_domain_report best` through the drivers on the real engine: its file is the reduction of the `all` file of the same
command (per pair the best any-order mapping and, where that one breaks the order, the best order-preserving one), it serves the
pairs the enumeration cap skips, and it does not depend on batch sizes or on the residency of the target."""
import logging
import os

import numpy as np
import pytest

import best_mapping_case as bm
import multidom_case as mc

pytestmark = pytest.mark.gpu
MINCOS, MINCOV = "0.5", "0.7"
LOW = "0.02"                          # a --mincos at which 4 of 10 random cells stay: most pairs have several mappings


def _read(prefix):
    return open(prefix + "_search_multi_dom.tsv", "rb").read()


def _chain_search(db, out, tmp, report, mincos=MINCOS, extra=()):
    from merizo_search_amd import cli
    cli.main(["chain-search", db, db, out, tmp, "-s", mincos, "-c", MINCOV, "--output_headers", "--multi_domain_report", report] + list(extra))
    return _read(out)


def _db_search(db, out, tmp, report, k, mincos=MINCOS, extra=()):
    from merizo_search_amd import cli
    cli.main(["db-search", db, db, out, tmp, "--multi_domain_search", "--multi_domain_mode", "exhaustive_cosine", "--skip_tmalign",
              "-s", mincos, "-c", MINCOV, "-k", str(k), "--output_headers", "--multi_domain_report", report] + list(extra))
    return _read(out)


def _cells(info):
    return np.asarray([np.float32(e.split(":")[2]) for e in info.split(",")], np.float32)


def _int_total(info):
    return int(bm.quantise(_cells(info))[1].sum())


def _f64_total(info):
    return float(np.sum(_cells(info).astype(np.float64)))


def check_reduction(all_bytes, best_bytes):
    """The `best` file against the `all` file of the same command -> (pairs, second lines)."""
    all_lines = [l.split("\t") for l in all_bytes.decode().splitlines()]
    best_lines = [l.split("\t") for l in best_bytes.decode().splitlines()]
    assert all_lines[0] == ["query_chain", "nqd", "hit_chain", "nhd", "match_category", "match_info", "hit_metadata"]
    assert best_lines[0] == ["query_chain", "nqd", "hit_chain", "nhd", "match_category", "match_score", "match_info", "hit_metadata"]
    groups, order = {}, []                                       # (query chain, hit chain) -> its lines of the `all` file
    for l in all_lines[1:]:
        assert len(l) == 7
        key = (l[0], l[2])
        if key not in groups:
            order.append(key)
        groups.setdefault(key, []).append(l)
    got, got_order = {}, []
    for l in best_lines[1:]:
        assert len(l) == 8
        key = (l[0], l[2])
        if key not in got:
            got_order.append(key)
        else:
            assert got_order[-1] == key, "the lines of a pair are adjacent"
        got.setdefault(key, []).append(l)
    assert set(got) == set(groups), (set(got) ^ set(groups))       # pairs absent from `all` are absent from `best`, and vice versa
    seconds = 0
    for key, lines in got.items():
        group = groups[key]
        for l in lines:
            assert l[5] == "%.6f" % _f64_total(l[6])
            assert [l[:5] + l[6:]] == [g for g in group if g[5:] == l[6:]], "the path occurs in the group, with its category"
        first = lines[0]
        best_int = max(_int_total(g[5]) for g in group)
        assert _int_total(first[6]) == best_int, (key, first)
        assert abs(float(first[5]) - max(_f64_total(g[5]) for g in group)) <= 1e-6
        ordered = [g for g in group if int(g[4]) >= 1]
        if int(first[4]) == 0 and ordered:
            assert len(lines) == 2, key
            assert int(lines[1][4]) >= 1 and _int_total(lines[1][6]) == max(_int_total(g[5]) for g in ordered)
            assert abs(float(lines[1][5]) - max(_f64_total(g[5]) for g in ordered)) <= 1e-6
            seconds += 1
        else:
            assert len(lines) == 1, key
    # query chains in the order of `all`; within one, the kind-0 totals descend, ties in the order of `all` (the plan order)
    chains = lambda keys: [qc for i, (qc, _hc) in enumerate(keys) if i == 0 or keys[i - 1][0] != qc]
    assert chains(got_order) == chains(order)
    rank = {key: i for i, key in enumerate(order)}
    want = sorted(order, key=lambda key: (chains(order).index(key[0]), -_int_total(got[key][0][6]), rank[key]))
    assert got_order == want
    return len(got), seconds


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("best_mapping"))
    names, chain_of = mc.write_planted(work)
    return work, names, chain_of


@pytest.fixture(scope="module")
def resident_best(planted, tmp_path_factory):
    """chain-search --multi_domain_report best on the planted database (faiss layout, --mincos LOW), resident, one batch."""
    tmp = tmp_path_factory.mktemp("best_ref")
    return _chain_search(os.path.join(planted[0], "fa"), str(tmp / "best"), str(tmp / "t"), "best", mincos=LOW)


# ------------------------------------------------------------------ 1. best is the reduction of all ---
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_chain_search_and_db_search_best_reduce_their_all_files(planted, tmp_path, layout):
    """At --mincos 0.5 (the planted relatives: in order, reversed, inserted) through both commands and both layouts."""
    work, names, _chain_of = planted
    db, tmp = os.path.join(work, layout), str(tmp_path / "t")
    pairs, _seconds = check_reduction(_chain_search(db, str(tmp_path / "ca"), tmp, "all"), _chain_search(db, str(tmp_path / "cb"), tmp, "best"))
    assert pairs >= 8
    best = _db_search(db, str(tmp_path / "db"), tmp, "best", len(names))
    pairs, _seconds = check_reduction(_db_search(db, str(tmp_path / "da"), tmp, "all", len(names)), best)
    assert pairs >= 8
    rows = [l.split("\t") for l in best.decode().splitlines()[1:]]
    cats = {(r[0], r[2]): r[4] for r in reversed(rows)}          # (the first line of each pair)
    assert cats[mc.FAMILY["src"], mc.FAMILY["inorder"]] == "3" and cats[mc.FAMILY["src"], mc.FAMILY["reversed"]] == "0"
    assert cats[mc.FAMILY["src"], mc.FAMILY["inserted"]] == "1" and cats[mc.FAMILY["five"], mc.FAMILY["five_copy"]] == "3"
    # the default is `all`: the flag left out writes the bytes of `--multi_domain_report all`
    from merizo_search_amd import cli
    cli.main(["chain-search", db, db, str(tmp_path / "default"), tmp, "-s", MINCOS, "-c", MINCOV, "--output_headers"])
    assert _read(str(tmp_path / "default")) == _read(str(tmp_path / "ca"))


def test_many_mappings_per_pair_at_a_low_mincos(planted, resident_best, tmp_path):
    """--mincos LOW on random rows: pairs with many mappings and second lines occur, so the reduction has something to reduce."""
    db, tmp = os.path.join(planted[0], "fa"), str(tmp_path / "t")
    all_bytes = _chain_search(db, str(tmp_path / "all"), tmp, "all", mincos=LOW)
    pairs, seconds = check_reduction(all_bytes, resident_best)
    assert pairs >= 30 and seconds >= 3 and all_bytes.count(b"\n") > pairs + 20, (pairs, seconds, all_bytes.count(b"\n"))


# ------------------------------------------------------------------ 2. the enumeration cap is gone ---
def _write_repeats(work, seed=21):
    """Two chains of 12 near-duplicate domains (pairwise cosines about 0.96) between unrelated single-domain chains."""
    from merizo_search_amd.foldclass import dbutil, synthetic as syn
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(128)
    names, vecs = [], []
    for c, run in enumerate((1, 12, 2, 12, 1)):
        for d in range(run):
            names.append("r%05d_TED%02d" % (c, d + 1))
            v = base + 0.2 * np.linalg.norm(base) / np.sqrt(128.0) * rng.standard_normal(128) if run == 12 else rng.standard_normal(128)
            vecs.append(v)
    raw = np.stack(vecs)
    norm = (raw / np.linalg.norm(raw, axis=1, keepdims=True)).astype(np.float32)
    n = len(names)
    os.makedirs(work, exist_ok=True)
    dbutil.write_faiss_db(os.path.join(work, "rep"), norm, names, ["ACDEFGHIKL" * 4] * n, [syn.random_walk(40, seed + i) for i in range(n)],
                          metadata=['{ "row": %d }' % i for i in range(n)])
    return os.path.join(work, "rep"), names, norm


def test_a_pair_of_12_domain_repeat_chains_is_served(tmp_path, caplog):
    """12^12 candidate mappings: `all` skips the pair with its warning and writes no line for it; `best` writes the pair's lines,
    equal to the restatement applied to ops.md_chain_scores' matrix."""
    import torch
    from merizo_search_amd import _lib, ops
    db, names, norm = _write_repeats(str(tmp_path / "case"))
    tmp = str(tmp_path / "t")
    with caplog.at_level(logging.WARNING):
        all_bytes = _chain_search(db, str(tmp_path / "all"), tmp, "all", extra=["--exclude_same_chain"])
    assert caplog.text.count("candidate mappings (more than 1000000): skipped") == 2, caplog.text
    assert all_bytes.count(b"\n") == 1                               # the header: neither repeat pair has a line
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        best = _chain_search(db, str(tmp_path / "best"), tmp, "best", extra=["--exclude_same_chain"])
    assert "skipped" not in caplog.text
    rows = [l.split("\t") for l in best.decode().splitlines()[1:]]
    assert {(r[0], r[2]) for r in rows} == {("r00001", "r00003"), ("r00003", "r00001")}
    first = {"r00001": 1, "r00003": 15}
    for qc, hc in (("r00001", "r00003"), ("r00003", "r00001")):
        q0, t0 = first[qc], first[hc]
        rows_d = torch.from_numpy(norm).cuda()
        scores, match = ops.md_chain_scores(rows_d, rows_d[q0: q0 + 12].contiguous(), _lib.MODE_IP_PRENORM, np.asarray([(0, 12, 0, 12)], np.int32),
                                            np.arange(t0, t0 + 12), np.zeros(1, np.int64), float(MINCOS))
        m = scores.cpu().numpy().reshape(12, 12)
        assert match.cpu().numpy().tolist() == [[12, 12]] and (m != 0).all()
        want = []
        st0, _tot0, p0 = bm.best_any(m)
        st1, _tot1, p1 = bm.best_ordered(m)
        assert st0 == 1 and st1 == 1 and p1 == list(range(12))
        for p in [p0] + ([p1] if any(b < a for a, b in zip(p0, p0[1:])) else []):
            cells = m[np.arange(12), p]
            cat = 0 if any(b < a for a, b in zip(p, p[1:])) else 3
            want.append([qc, "12", hc, "12", str(cat), "%.6f" % float(np.sum(cells.astype(np.float64))),
                         ",".join("%s:%s:%s" % (names[q0 + i], names[t0 + j], str(cells[i])) for i, j in enumerate(p)),
                         "[" + ",".join('{ "row": %d }' % (t0 + j) for j in p) + "]"])
        assert [r for r in rows if (r[0], r[2]) == (qc, hc)] == want


# ------------------------------------------------------------------ 3. easy-search ---
def test_easy_search_database_cosine_best_reduces_its_own_all_run(tmp_path, monkeypatch):
    import md_case
    from merizo_search_amd import cli
    monkeypatch.setenv("MERIZO_ALLOW_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("MERIZO_TMALIGN", raising=False)
    monkeypatch.setenv("PATH", str(tmp_path / "nowhere"))
    qpdb, dbdir = md_case.write_inputs(tmp_path)
    db, tmp = str(tmp_path / "db"), str(tmp_path / "tmp")
    cli.main(["createdb", dbdir, db, "-d", "cuda", "--layout", "faiss"])
    files = {}
    for mode in ("database_cosine", "exhaustive_cosine"):
        for report in ("all", "best"):
            out = str(tmp_path / (mode + "_" + report))
            cli.main(["easy-search", qpdb, db, out, tmp, "-d", "cuda", "-k", "6", "-s", "0.5", "-c", "0.0", "--chopping", md_case.CHOPPING,
                      "--multi_domain_search", "--multi_domain_mode", mode, "--output_headers", "--multi_domain_report", report])
            files[mode, report] = _read(out)
    pairs, _seconds = check_reduction(files["database_cosine", "all"], files["database_cosine", "best"])
    assert pairs >= 2                                                # T1 (category 2) and T3 (category 0)
    assert files["exhaustive_cosine", "best"] == files["database_cosine", "best"]       # (-k 6: every row is a hit)
    assert b"AF-T3-F1-model_v4" in files["database_cosine", "best"]


# ------------------------------------------------------------------ 4. streamed and batched ---
def test_a_streamed_target_and_small_query_batches_write_the_same_bytes(planted, resident_best, tmp_path, monkeypatch, caplog):
    db, tmp = os.path.join(planted[0], "fa"), str(tmp_path / "t")
    assert _chain_search(db, str(tmp_path / "b3"), tmp, "best", mincos=LOW, extra=["--query_batchsize", "3"]) == resident_best
    n = len(planted[1])
    want = _db_search(db, str(tmp_path / "d"), tmp, "best", n, mincos=LOW)
    assert _db_search(db, str(tmp_path / "d3"), tmp, "best", n, mincos=LOW, extra=["--query_batchsize", "3"]) == want
    assert want == resident_best                                     # (-k covers the target: db-search's file is chain-search's)
    from merizo_search_amd.foldclass.engine import HipEngine
    monkeypatch.setattr(HipEngine, "resident_budget", lambda self, nq=0, k=0: 1 << 10)
    with caplog.at_level(logging.INFO):
        got = _chain_search(db, str(tmp_path / "streamed"), tmp, "best", mincos=LOW, extra=["--search_batchsize", "5"])
    assert "the target is streamed in blocks of 5 rows" in caplog.text
    assert got == resident_best
