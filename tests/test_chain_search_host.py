"""The host side of `chain-search` without a GPU: which query chains are served and how they are batched, the own-chain filter, the
choice of the scan's route, the command line and its refusals."""
import logging
import os

import numpy as np
import pytest

import dbquery_case as dq
from merizo_search_amd.foldclass import chainsearch as cs, multidomain as md


def _runs(lengths, offset=0, ids=None):
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if ids is None:
        ids = ["c%d" % c for c, n in enumerate(lengths) for _ in range(n)]
    return cs.served_runs(starts, ids, offset)


# ------------------------------------------------------------------ 1. the query chains and their batches ---
def test_served_runs_skip_single_domains_and_more_than_64(caplog):
    with caplog.at_level(logging.DEBUG):
        runs = _runs([1, 2, 64, 65, 3, 1, 200, 2], offset=100)
    assert runs == [(101, 103, "c1"), (103, 167, "c2"), (232, 235, "c4"), (436, 438, "c7")]
    assert "Query chain c0: only one detected domain" in caplog.text and "Query chain c5: only one detected domain" in caplog.text
    for qc, n in (("c3", 65), ("c6", 200)):
        assert "Query chain %s has %d domains, more than the 64 the database scan serves per query chain: skipped" % (qc, n) in caplog.text
    assert [r.levelname for r in caplog.records if "more than the 64" in r.getMessage()] == ["WARNING"] * 2
    assert _runs([]) == [] and _runs([1, 1]) == []


def test_served_runs_follow_query_rows_as_db_search_forms_them():
    """The runs are those of the names INSIDE the slice: a chain the slice cuts is served with the domains that are left."""
    names, _first, _last = dq.chain_names(300, 3)
    ids = [md.domid2chainid(n) for n in names]
    for lo, hi in ((0, 300), (17, 203), (5, 7)):
        got = cs.served_runs(md.chain_runs(names[lo:hi]), ids[lo:hi], lo)
        want, a = [], lo
        while a < hi:
            b = a + 1
            while b < hi and ids[b] == ids[a]:
                b += 1
            if 2 <= b - a <= 64:
                want.append((a, b, ids[a]))
            a = b
        assert got == want and (len(got) > 20 or hi - lo < 10)


def test_batches_hold_whole_chains_up_to_the_batch_size():
    runs = _runs([2, 3, 5, 2, 64, 2, 2])
    flat = lambda batches: [r for b in batches for r in b]
    for size in (1, 3, 5, 7, 10, 64, 66, 4096):
        batches = cs.chain_batches(runs, size)
        assert flat(batches) == runs and all(batches)
        for batch in batches:
            rows = sum(b - a for a, b, _qc in batch)
            assert rows <= size or len(batch) == 1                       # (a chain longer than the batch size is a batch of its own)
        for one, two in zip(batches, batches[1:]):                       # greedy: the next chain did not fit
            assert sum(b - a for a, b, _qc in one) + (two[0][1] - two[0][0]) > size
    assert [len(b) for b in cs.chain_batches(runs, 10)] == [3, 1, 1, 2]
    assert cs.chain_batches([], 10) == []
    # a chain id that comes back starts a new batch: the chains of a batch are keyed by their id
    again = _runs([2, 2, 2, 2], ids=["a", "a", "b", "b", "a", "a", "c", "c"])
    assert [[qc for _a, _b, qc in b] for b in cs.chain_batches(again, 4096)] == [["a", "b"], ["a", "c"]]


# ------------------------------------------------------------------ 2. the own-chain filter ---
def test_a_query_chain_is_never_its_own_candidate():
    starts = np.asarray([0, 2, 5, 6, 10], np.int64)
    pairs = np.asarray([(g, c) for g in range(3) for c in range(4)], np.int64)
    # query chains that start at rows 2, 7 (inside target run 3: --query_rows cut it) and 0
    kept = cs.drop_own_chain(pairs, [2, 7, 0], starts)
    assert sorted(map(tuple, kept.tolist())) == sorted((g, c) for g in range(3) for c in range(4) if (g, c) not in ((0, 1), (1, 3), (2, 0)))
    assert cs.drop_own_chain(np.zeros((0, 2), np.int64), [2, 7, 0], starts).shape == (0, 2)
    assert cs.drop_own_chain([(0, 2)], [2], starts).tolist() == [[0, 2]]


# ------------------------------------------------------------------ 3. the route ---
def test_auto_takes_the_matrix_route_from_the_measured_size_on_when_a_bound_is_given():
    from merizo_search_amd import _lib, ops
    n = ops.MD_SCAN_MATRIX_MIN_NQ
    assert n in (16, 64, 256, 1024, 4096)                                # a point of tools/chain_search_bench.py's sweep
    assert ops.md_scan_route("auto", n, 1.0 + 1e-6) == "matrix" and ops.md_scan_route("auto", n - 1, 1.0 + 1e-6) == "lane"
    assert ops.md_scan_route("auto", n, None) == "lane" and ops.md_scan_route("auto", 1 << 20, None) == "lane"
    assert ops.md_scan_route("lane", 1 << 20, 1.0) == "lane" and ops.md_scan_route("matrix", 1, 1.0) == "matrix"
    with pytest.raises(_lib.MerizoHipError):
        ops.md_scan_route("matrix", 4096, None)
    with pytest.raises(_lib.MerizoHipError):
        ops.md_scan_route("mfma", 4096, 1.0)


def test_the_drivers_forward_the_route():
    """engine.md_chain_scan gives the unit-row bound to every route but "lane"; database_candidates passes its route on and leaves
    the call of an engine without one as it was."""
    from merizo_search_amd.foldclass.engine import HipEngine
    seen = []

    class Ops:
        MODE_IP_NORMQ, MODE_IP_PRENORM, MODE_COSINE_UNIT = 3, 0, 2

        @staticmethod
        def md_chain_scan(*a, **kw):
            seen.append(kw)
            return "out"

    eng = HipEngine.__new__(HipEngine)
    eng._ops = Ops
    assert eng.md_chain_scan(None, None, None, "ip", None, 0.5) == "out" and seen[-1]["route"] == "lane" and seen[-1]["row_norm_bound"] is None
    eng.md_chain_scan(None, None, None, "cosine", None, 0.5, route="auto")
    assert seen[-1]["route"] == "auto" and seen[-1]["row_norm_bound"] == 1.0 + 1e-6
    eng.md_chain_scan(None, None, None, "ip_prenorm", None, 0.5, route="matrix", row_norm_bound=2.0)
    assert seen[-1]["route"] == "matrix" and seen[-1]["row_norm_bound"] == 2.0


# ------------------------------------------------------------------ 4. the command line ---
def test_argparse_of_chain_search():
    from merizo_search_amd import cli
    p = cli.chain_search_parser()
    a = p.parse_args(["q", "t", "out", "tmp"])
    assert (a.query_db, a.target_db, a.output, a.tmp, a.device) == ("q", "t", "out", "tmp", "cuda")
    assert (a.mincos, a.mincov, a.query_batchsize, a.search_batchsize, a.query_rows) == (0.5, 0.7, 4096, 262144, None)
    assert a.exclude_same_chain is False and a.output_headers is False
    a = p.parse_args(["q", "t", "out", "tmp", "-d", "cuda:1", "-s", "0.8", "-c", "0.5", "--query_batchsize", "100", "--search_batchsize", "7",
                      "--query_rows", "3:9", "--exclude_same_chain", "--output_headers"])
    assert (a.device, a.mincos, a.mincov, a.query_batchsize, a.search_batchsize, a.query_rows) == ("cuda:1", 0.8, 0.5, 100, 7, "3:9")
    assert a.exclude_same_chain and a.output_headers
    a = p.parse_args(["q", "t", "out", "tmp", "--mincos", "0.3", "--mincov", "0.1"])
    assert (a.mincos, a.mincov) == (0.3, 0.1)
    for bad in (["q", "t", "out"], ["q", "t", "out", "tmp", "-k", "3"], ["q", "t", "out", "tmp", "--multi_domain_mode", "database_cosine"]):
        with pytest.raises(SystemExit) as exc:
            p.parse_args(bad)
        assert exc.value.code == 2
    assert "chain-search" in cli.__doc__


def _refused(argv, caplog):
    from merizo_search_amd import cli
    caplog.clear()
    with pytest.raises(SystemExit) as exc:
        cli.main(["chain-search"] + argv)
    assert exc.value.code == 1
    return caplog.text


def test_refusals_come_before_any_gpu_work(tmp_path, caplog):
    """Each ends with the drivers' error line and exit status 1 on a machine without a GPU: nothing was asked of a device."""
    work = str(tmp_path / "case")
    dq.write_case(work, n=60, seed=5)
    dq.write_case(os.path.join(work, "other"), n=30, seed=6)
    fa, pt, other = os.path.join(work, "fa"), os.path.join(work, "pt"), os.path.join(work, "other", "fa")
    out, tmp = str(tmp_path / "o"), str(tmp_path / "t")
    assert "not supported by merizo_search_amd" in _refused([fa, fa, out, tmp, "-d", "cpu"], caplog)
    assert "neither" in _refused([fa + "_missing", fa, out, tmp], caplog)
    assert "neither" in _refused([fa, fa + "_missing", out, tmp], caplog)
    assert "needs the query database and the target database to be the same" in _refused([fa, other, out, tmp, "--exclude_same_chain"], caplog)
    assert "needs the query database" in _refused([fa, pt, out, tmp, "--exclude_same_chain"], caplog)      # another layout: another database
    for cov in ("-0.1", "1.5", "nan"):
        assert "--mincov must lie in [0, 1]" in _refused([fa, fa, out, tmp, "--mincov=" + cov], caplog), cov
    for rows in ("7:7", "9:3", "60:", "0:61", "abc"):
        assert "--query_rows" in _refused([fa, fa, out, tmp, "--query_rows=" + rows], caplog), rows
    assert not os.path.exists(out + "_search_multi_dom.tsv")
