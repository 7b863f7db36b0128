"""`chain-search` on the real engine: its file is, byte for byte, the file `db-search --multi_domain_search --multi_domain_mode
exhaustive_cosine --skip_tmalign` writes when -k covers every row of the target that is not excluded -- on the planted database of
multidom_case (both layouts) and on the random chains of dbquery_case at a low --mincos -- whatever the query batch size, the
residency of the target, the route of the scan or the number of ranks."""
import os
import subprocess
import sys

import pytest

import dbquery_case as dq
import multidom_case as mc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINCOS, MINCOV = "0.5", "0.7"


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("chain_search"))
    names, chain_of = mc.write_planted(work)
    return work, names, chain_of


def _bytes(prefix):
    return open(prefix + "_search_multi_dom.tsv", "rb").read()


def _db_search(db, out, tmp, k, mincos=MINCOS, extra=()):
    from merizo_search_amd import cli
    cli.main(["db-search", db, db, out, tmp, "--multi_domain_search", "--multi_domain_mode", "exhaustive_cosine", "--skip_tmalign",
              "-s", mincos, "-c", MINCOV, "-k", str(k), "--output_headers"] + list(extra))
    return _bytes(out)


def _chain_search(db, out, tmp, mincos=MINCOS, extra=(), target=None):
    from merizo_search_amd import cli
    cli.main(["chain-search", db, target or db, out, tmp, "-s", mincos, "-c", MINCOV, "--output_headers"] + list(extra))
    return _bytes(out)


@pytest.fixture(scope="module")
def reference(planted, tmp_path_factory):
    """chain-search's own bytes on the planted database, per layout and flags (the comparisons below share them)."""
    tmp = tmp_path_factory.mktemp("chain_search_ref")
    out = {}
    for layout in ("fa", "pt"):
        db = os.path.join(planted[0], layout)
        out[layout, False] = _chain_search(db, str(tmp / (layout + "_all")), str(tmp / "t"))
        out[layout, True] = _chain_search(db, str(tmp / (layout + "_excl")), str(tmp / "t"), extra=["--exclude_same_chain"])
    return out


# ------------------------------------------------------------------ 1. the definition ---
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_the_file_is_db_search_with_k_covering_the_target(planted, reference, tmp_path, layout):
    """With and without --exclude_same_chain (db-search fetches k plus the longest excluded run, 5 rows here, so k = n - 5 still
    reaches every row outside the query's chain), and with --query_rows cutting the first and the last query chain."""
    work, names, _chain_of = planted
    db, tmp, n = os.path.join(work, layout), str(tmp_path / "t"), len(names)
    want = _db_search(db, str(tmp_path / "ref_all"), tmp, n)
    assert reference[layout, False] == want and want.count(b"\n") > 8
    lines = [l.decode() for l in want.splitlines(keepends=True)][1:]
    assert "3" in mc.categories(lines, mc.FAMILY["src"], mc.FAMILY["src"])              # nothing excludes the query's own chain
    want = _db_search(db, str(tmp_path / "ref_excl"), tmp, n - 5, extra=["--exclude_same_chain"])
    assert reference[layout, True] == want and 5 < want.count(b"\n") < reference[layout, False].count(b"\n")
    mc.check_planted_categories([l.decode() for l in want.splitlines(keepends=True)][1:])
    rows = ["--query_rows", "%d:%d" % (names.index("c00003_TED02"), names.index("c00026_TED04")), "--exclude_same_chain"]
    want = _db_search(db, str(tmp_path / "ref_rows"), tmp, n - 5, extra=rows)
    got = _chain_search(db, str(tmp_path / "rows"), tmp, extra=rows)
    assert got == want and want.count(b"\n") > 2 and want != reference[layout, True]
    assert b"\nc00003\t2\t" in want and b"\nc00003\t3\t" not in want                     # the cut chain is served with its two domains left


def test_random_chains_at_a_low_mincos(tmp_path):
    """dbquery_case's 200 random rows in chains of 1-7 at --mincos 0.15 (1.7 sigma of a random cosine: dozens of chain pairs
    qualify by chance, and the exact duplicates qualify always), the faiss layout against itself."""
    work = str(tmp_path / "case")
    dq.write_case(work, n=200)
    fa, tmp = os.path.join(work, "fa"), str(tmp_path / "t")
    want = _db_search(fa, str(tmp_path / "ref"), tmp, 200, mincos="0.15")
    got = _chain_search(fa, str(tmp_path / "got"), tmp, mincos="0.15")
    assert got == want and want.count(b"\n") > 20


# ------------------------------------------------------------------ 2. batches, residency, route ---
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_query_batches_of_three_rows_write_the_same_bytes(planted, reference, tmp_path, layout):
    db = os.path.join(planted[0], layout)
    got = _chain_search(db, str(tmp_path / "b3"), str(tmp_path / "t"), extra=["--query_batchsize", "3", "--exclude_same_chain"])
    assert got == reference[layout, True]


def test_a_streamed_target_in_blocks_of_five_rows_writes_the_same_bytes(planted, reference, tmp_path, monkeypatch, caplog):
    """The faiss layout beyond the resident budget: blocks of 5 rows cut chains at their edges (the edge rule makes them
    everybody's candidates, the scoring half decides them)."""
    import logging
    from merizo_search_amd.foldclass.engine import HipEngine
    monkeypatch.setattr(HipEngine, "resident_budget", lambda self, nq=0, k=0: 1 << 10)
    db = os.path.join(planted[0], "fa")
    with caplog.at_level(logging.INFO):
        got = _chain_search(db, str(tmp_path / "streamed"), str(tmp_path / "t"), extra=["--search_batchsize", "5"])
    assert got == reference["fa", False]
    assert "the target is streamed in blocks of 5 rows" in caplog.text


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_the_lane_route_through_the_driver_writes_the_bytes_of_the_matrix_route(planted, reference, tmp_path, monkeypatch, layout):
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import chainsearch
    taken = []
    launch = ops.md_chain_scan_launch

    def spy(*a, **kw):
        taken.append(ops.md_scan_route(kw.get("route", "lane"), a[2].shape[0], kw.get("row_norm_bound")))
        return launch(*a, **kw)

    monkeypatch.setattr(ops, "md_chain_scan_launch", spy)
    db = os.path.join(planted[0], layout)
    for route in ("lane", "matrix", "auto"):
        del taken[:]
        out = str(tmp_path / route)
        chainsearch.run_chain_search(db, db, out, str(tmp_path / "t"), "cuda", mincos=float(MINCOS), mincov=float(MINCOV),
                                     output_headers=True, route=route)
        assert _bytes(out) == reference[layout, False], route
        nq = sum(1 for c in planted[2] if planted[2].count(c) >= 2)
        assert nq >= ops.MD_SCAN_MATRIX_MIN_NQ                                        # (so "auto" takes the matrix route here)
        assert taken and set(taken) == {"lane" if route == "lane" else "matrix"}, (route, taken)


# ------------------------------------------------------------------ 3. two ranks ---
def test_two_ranks_on_one_gpu_write_the_bytes_of_one_process(planted, reference, tmp_path):
    """`torchrun --nproc-per-node 2 -m merizo_search_amd.cli chain-search` (both ranks on cuda:0 over gloo): every rank scans its
    half of the rows, the candidate lists are gathered, rank 0 scores and writes."""
    from conftest import free_port
    db = os.path.join(planted[0], "fa")
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", MERIZO_SAME_DEVICE="1", PYTHONPATH=REPO, GLOO_SOCKET_IFNAME="lo")
    argv = ["-m", "merizo_search_amd.cli", "chain-search", db, db, str(tmp_path / "two"), str(tmp_path / "t"), "-s", MINCOS, "-c", MINCOV,
            "--output_headers", "--exclude_same_chain", "--query_batchsize", "40"]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + argv, capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert _bytes(str(tmp_path / "two")) == reference["fa", True]
