"""`exhaustive_cosine` multi-domain search without a GPU: the commands and the db-search driver on the oracle engine (its
score matrices = the oracle's own search scores, multidom_case.install_oracle_md), against the driver step restated from
group_hits, sibling_rows and chain_mappings."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import dbquery_case as dq
import multidom_case as mc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = "query,emb_rank,target,emb_score,q_len,t_len,metadata"
MINCOS, MINCOV, K = 0.5, 0.7, 10


def _engine():
    dq.install_oracle_drop()
    return mc.install_oracle_md()()


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("multidom"))
    names, chain_of = mc.write_planted(work)
    return work, names, chain_of


def _run(planted, tmp_path, tag, layout="fa", engine=None, timings=None, **kw):
    from merizo_search_amd.foldclass import dbsearch as ds
    work = planted[0]
    db = os.path.join(work, layout)
    out = str(tmp_path / tag)
    args = dict(topk=K, mincos=MINCOS, mincov=MINCOV, skip_tmalign=True, format_list=FMT.split(","), exclude_same_chain=True,
                multi_domain_search=True)
    args.update(kw)
    ds.run_dbsearch_db(db, db, out, str(tmp_path / "t"), "cuda", engine=engine or _engine(), timings=timings, **args)
    return out


def _expected(planted, layout, search_tsv, lo=0, hi=None, **kw):
    kw.setdefault("mincos", MINCOS)
    return mc.expected_lines(planted, layout, search_tsv, mc.oracle_pair_scores, lo, hi, mincov=MINCOV, **kw)


# ------------------------------------------------------------------ 1. search / easy-search --------------
def test_cli_easy_search_exhaustive_cosine_needs_no_aligner(tmp_path, monkeypatch, caplog):
    """`easy-search --multi_domain_search --multi_domain_mode exhaustive_cosine` on the md_case scenario with no TM-align binary
    anywhere: T1 (both domains in order, three target domains) is reported in category 2, T3 (order swapped) in category 0, the
    single-domain chain T2 never; every score is a float32 at or above --mincos.  exhaustive_tmalign is still refused."""
    import md_case
    from oracle_engine import oracle_network
    from merizo_search_amd import cli
    from merizo_search_amd.foldclass import dbsearch as ds, makedb
    mc.install_oracle_md()
    net = oracle_network()
    monkeypatch.setattr(ds, "network_setup", lambda **kw: (net, "cpu"))
    monkeypatch.setattr(makedb, "network_setup", lambda **kw: (net, "cpu"))
    monkeypatch.delenv("MERIZO_TMALIGN", raising=False)
    monkeypatch.setenv("PATH", str(tmp_path / "nowhere"))
    qpdb, dbdir = md_case.write_inputs(tmp_path)
    for layout in ("faiss", "pt"):
        db, out = str(tmp_path / ("db_" + layout)), str(tmp_path / ("out_" + layout))
        cli.main(["createdb", dbdir, db, "--layout", layout])
        cli.main(["easy-search", qpdb, db, out, str(tmp_path / "tmp"), "-k", "3", "-s", "0.5", "-c", "0.0", "--chopping", md_case.CHOPPING,
                  "--multi_domain_search", "--multi_domain_mode", "exhaustive_cosine", "--output_headers"])
        mc.check_md_case_outputs(out, 0.5)
    caplog.clear()
    with pytest.raises(SystemExit) as exc:                              # the TM-align mode without a binary: refused, as before
        cli.main(["easy-search", qpdb, db, str(tmp_path / "o3"), str(tmp_path / "tmp"), "-k", "3", "--chopping", md_case.CHOPPING,
                  "--multi_domain_search", "--multi_domain_mode", "exhaustive_tmalign"])
    assert exc.value.code == 1 and "needs a" in caplog.text and "TM-align binary" in caplog.text


# ------------------------------------------------------------------ 2. db-search, planted database -------
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_db_search_multi_domain_equals_the_restated_driver(planted, tmp_path, monkeypatch, layout):
    """`db-search db db --multi_domain_search --exclude_same_chain -k 10 --skip_tmalign` through the command line:
    `_search_multi_dom.tsv` equals the driver restatement applied to that run's `_search.tsv`; the planted relatives of the
    source chain land in categories 3 (in order), 0 (reversed), 1 (a domain inserted) and nowhere (one domain missing)."""
    from merizo_search_amd import cli
    from merizo_search_amd.foldclass import dbsearch as ds
    eng = _engine()
    monkeypatch.setattr(ds, "engine_setup", lambda device: eng)
    db, out = os.path.join(planted[0], layout), str(tmp_path / "cli")
    cli.main(["db-search", db, db, out, str(tmp_path / "t"), "--multi_domain_search", "--exclude_same_chain", "-k", "10", "--skip_tmalign",
              "-s", str(MINCOS), "-c", str(MINCOV), "--format", FMT])
    got = open(out + "_search_multi_dom.tsv").readlines()
    assert got == _expected(planted, layout, out + "_search.tsv") and len(got) > 5
    mc.check_planted_categories(got)
    # with the header asked for it appears once, in front
    out2 = _run(planted, tmp_path, "hdr", layout, header=True, query_batchsize=7)
    lines = open(out2 + "_search_multi_dom.tsv").readlines()
    assert lines[0].startswith("query_chain\tnqd\t") and lines[1:] == got


# ------------------------------------------------------------------ 3. batch carry ----------------------
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_db_search_multi_domain_is_independent_of_the_query_batches(planted, tmp_path, layout):
    _work, names, chain_of = planted
    big = _run(planted, tmp_path, "big", layout, query_batchsize=4096)
    small = _run(planted, tmp_path, "small", layout, query_batchsize=3)
    spans = {c: {r // 3 for r, cc in enumerate(chain_of) if cc == c} for c in set(chain_of)}
    assert max(len(v) for v in spans.values()) == 3                     # a chain of 5 domains spans three batches of 3
    for suffix in ("_search.tsv", "_search_multi_dom.tsv"):
        assert open(big + suffix, "rb").read() == open(small + suffix, "rb").read(), suffix
    assert os.path.getsize(big + "_search_multi_dom.tsv") > 0
    # --query_rows cutting the first and the last chain: the cut runs are the query chains
    lo = next(r for r in range(1, len(names)) if chain_of[r] == chain_of[r - 1] and chain_of[r] == mc.FAMILY["src"])
    hi = next(r for r in range(len(names) - 1, 0, -1) if chain_of[r] == chain_of[r - 1] == chain_of[r - 2])
    assert chain_of[hi] == chain_of[hi - 1] and chain_of[lo] == chain_of[lo - 1]
    cutrun = _run(planted, tmp_path, "cut", layout, query_batchsize=4, query_rows="%d:%d" % (lo, hi))
    got = open(cutrun + "_search_multi_dom.tsv").readlines()
    assert got == _expected(planted, layout, cutrun + "_search.tsv", lo, hi)
    assert any(l.startswith(mc.FAMILY["src"] + "\t2\t") for l in got)   # the source chain, cut to its last two domains


# ------------------------------------------------------------------ 4. two ranks ------------------------
_SHIM = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import dbquery_case as dq
import multidom_case as mc
from merizo_search_amd import cli
from merizo_search_amd.foldclass import dbsearch as ds, sharded
dq.install_oracle_drop()
Engine = mc.install_oracle_md()
work, tag = sys.argv[2], sys.argv[3]
ds.engine_setup = lambda device: Engine()
for layout in ("fa", "pt"):
    db = os.path.join(work, layout)
    cli.db_search([db, db, os.path.join(work, "%s_%s" % (layout, tag)), os.path.join(work, "tmp_" + tag), "--multi_domain_search",
                   "--exclude_same_chain", "-k", "10", "--skip_tmalign", "-s", "0.5", "-c", "0.7", "--query_batchsize", "16",
                   "--format", "query,emb_rank,target,emb_score,q_len,t_len,metadata"])
sharded.finalize_distributed()
'''


def test_db_search_multi_domain_two_gloo_ranks_equal_one_rank(planted, tmp_path):
    """Under two ranks rank 0 does the step from the database files (no rank holds all rows): the same bytes."""
    from conftest import free_port
    work = planted[0]
    shim = str(tmp_path / "shim.py")
    with open(shim, "w") as handle:
        handle.write(_SHIM)
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
    for nproc, tag in ((1, "one"), (2, "two")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), shim, REPO, work, tag]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for layout in ("fa", "pt"):
        for suffix in ("_search.tsv", "_search_multi_dom.tsv"):
            one = open(os.path.join(work, "%s_one%s" % (layout, suffix)), "rb").read()
            two = open(os.path.join(work, "%s_two%s" % (layout, suffix)), "rb").read()
            assert one == two and one.count(b"\n") > 5, (layout, suffix)
        assert open(os.path.join(work, layout + "_one_search_multi_dom.tsv")).readlines() == \
            _expected(planted, layout, os.path.join(work, layout + "_one_search.tsv"))


# ------------------------------------------------------------------ 5. own chain ------------------------
def test_db_search_exclude_self_never_reports_the_own_chain(planted, tmp_path):
    """--exclude_self keeps the sibling domains of the query's chain among its hits; they seed no candidate."""
    out = _run(planted, tmp_path, "self", "fa", exclude_same_chain=False, exclude_self=True, mincos=-2.0, topk=6)
    hits = dq.read_tsv(out + "_search.tsv")
    from merizo_search_amd.foldclass.multidomain import domid2chainid
    assert any(domid2chainid(h[0]) == domid2chainid(h[2]) for h in hits)          # siblings ARE hits here
    got = open(out + "_search_multi_dom.tsv").readlines()
    assert got and all(l.split("\t")[0] != l.split("\t")[2] for l in got)
    assert got == _expected(planted, "fa", out + "_search.tsv", own=True, mincos=-2.0)


# ------------------------------------------------------------------ 6. enumeration cap ------------------
def test_enumeration_cap_skips_exactly_the_pairs_above_it(planted, tmp_path, caplog):
    times = {}
    with caplog.at_level(logging.WARNING):
        out = _run(planted, tmp_path, "cap", "fa", mincos=0.0, topk=4, max_mapping_paths=10, timings=times)
    skipped = []
    want = _expected(planted, "fa", out + "_search.tsv", mincos=0.0, max_paths=10, skipped=skipped)
    assert open(out + "_search_multi_dom.tsv").readlines() == want
    assert len(skipped) > 0 and times["md_candidates_skipped"] == len(skipped)
    for qc, hc in skipped:
        assert any("query chain %s x hit chain %s" % (qc, hc) in r.getMessage() for r in caplog.records), (qc, hc)
    # at the default nothing in this database is skipped: the cap hides nothing
    times = {}
    out = _run(planted, tmp_path, "nocap", "fa", mincos=0.0, topk=4, timings=times)
    assert times["md_candidates_skipped"] == 0 and times["md_resident"] is True
    assert open(out + "_search_multi_dom.tsv").readlines() == _expected(planted, "fa", out + "_search.tsv", mincos=0.0)


def test_md_chain_scores_host_refusals_without_a_gpu():
    """The return codes that need no device: NULL pointers, an unsupported mode, a NaN cut, nq < 1, a short workspace; no
    candidates is a success without a launch."""
    import ctypes
    from merizo_search_amd import _lib
    _lib.build()
    lib = _lib.load()
    p = 0x1000                                                          # never dereferenced: the host checks come first
    ok = dict(db=p, n=10, q=p, nq=4, mode=_lib.MODE_IP_PRENORM, lengths=None, qlen=None, mincov=0.0, cand=p, ncand=3, trows=p, ntrows=5,
              mat_off=p, min_score=-float("inf"), out_scores=p, out_match=p, workspace=p, workspace_bytes=4 * 512)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ms_md_chain_scores(a["db"], a["n"], a["q"], a["nq"], a["mode"], a["lengths"], a["qlen"], ctypes.c_float(a["mincov"]),
                                      a["cand"], a["ncand"], a["trows"], a["ntrows"], a["mat_off"], ctypes.c_float(a["min_score"]),
                                      a["out_scores"], a["out_match"], a["workspace"], a["workspace_bytes"], None)

    for name in ("db", "q", "cand", "trows", "mat_off", "out_scores", "out_match", "workspace"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(mode=_lib.MODE_COSINE_RAW), dict(mode=7), dict(min_score=float("nan")), dict(nq=0), dict(ncand=-1),
                dict(lengths=p), dict(mode=_lib.MODE_COSINE_UNIT, lengths=p)):
        assert call(**bad) == -1, bad
        assert b"ms_md_chain_scores" in lib.ms_last_error()
    assert call(workspace_bytes=4 * 512 - 1) == -2
    assert call(ncand=0) == 0
    assert int(lib.ms_md_chain_scores_workspace_bytes(4)) == 4 * 512 and int(lib.ms_md_chain_scores_workspace_bytes(0)) == 0
    assert lib.ms_version() == 210
