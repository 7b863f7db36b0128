"""The host side of the multi-domain mode `database_cosine` without a GPU: chain_runs against the domid2chainid loop, the edge
rule of shards and streamed blocks with a numpy stand-in for the scan (md_scan_case.scan_ref), the plans' order, the command
line's choices, and run_dbsearch's target_db parameter."""
import os

import numpy as np
import pytest

import md_scan_case as sc
import multidom_case as mc
from merizo_search_amd.foldclass import multidomain as md

MINCOS = 0.5


def _loop_runs(names):
    """The definition: a new chain wherever domid2chainid changes between neighbours."""
    ids = [md.domid2chainid(n) for n in names]
    return [r for r in range(len(ids)) if r == 0 or ids[r] != ids[r - 1]] + [len(ids)]


def _id_runs(ids):
    return [r for r in range(len(ids)) if r == 0 or ids[r] != ids[r - 1]] + [len(ids)]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("md_scan_host"))
    names, chain_of = mc.write_planted(work)
    return work, names, chain_of


# ------------------------------------------------------------------ 1. chain_runs ---
def test_chain_runs_equals_the_domid2chainid_loop(golden_dir, planted):
    from merizo_search_amd.foldclass import dbutil
    raw = open(os.path.join(golden_dir, "ted100_slice", "names.index_names"), "rb").read()
    ted = [r.decode().rstrip() for r in np.frombuffer(raw, dtype="S%d" % dbutil.NAME_RECORD)]
    assert len(ted) > 10
    adversarial = ["x/app.pdb", "x/app01.pdb", "ap_TED01", "ap_TED02", "apd_TED01", "b.pdb", "b", "bd01", "bdb02.pdb", "Q._TED03", "Q_TED",
                   "Q_TED7", "Q_TED07", "Q_TED123", "Q_TED12", "cath-dompdb/2pi4A04.pdb", "2pi4A05", "2pi4B01", "2pi4A04", "AF-P1-F1-model_v4_TED01",
                   "AF-P1-F1-model_v4_TED02.pdb", "AF-P1-F1-model_v4_TED", "AF-P11-F1-model_v4_TED01", "d", "d", "p01", "", "_TED01", "a..pdb",
                   "a.", "a.01", "a_01", "a__TED01"]
    for names in (ted, planted[1], ["/x/" + n + ".pdb" for n in planted[1]], adversarial, adversarial[::-1], ["one"], []):
        runs = md.chain_runs(names)
        assert runs.dtype == np.int64 and runs.tolist() == _loop_runs(names)
    assert md.chain_runs(planted[1]).tolist() == _id_runs(planted[2])            # the planted chains, as write_planted names them
    # the quirks the loop inherits: rstrip('.pdb') eats trailing p, d, b and dots; two runs with one id are two chains
    assert md.domid2chainid("bdb02.pdb") == "bdb" and md.domid2chainid("app.pdb") == "a"
    assert md.chain_runs(["c1_TED01", "c2_TED01", "c1_TED02"]).tolist() == [0, 1, 2, 3]


def test_the_store_computes_its_chain_table_once(planted):
    from merizo_search_amd.foldclass.dbquery import QueryDB
    for layout in ("fa", "pt"):
        db = QueryDB(os.path.join(planted[0], layout))
        starts = db.chain_starts()
        assert starts.tolist() == _id_runs(planted[2]) and db.chain_starts() is starts
        assert db.stored_names(3, 6) == [n if layout == "fa" else "/x/" + n + ".pdb" for n in planted[1][3:6]]     # as write_planted stores them
        db.close()


# ------------------------------------------------------------------ 2. the edge rule ---
def _planted_case(planted):
    from merizo_search_amd.foldclass.dbquery import QueryDB
    work, names, chain_of = planted
    db = QueryDB(os.path.join(work, "fa"))
    emb = db.embeddings(0, db.n)
    db.close()
    starts = md.chain_runs(names)
    rows = {k: [r for r, c in enumerate(chain_of) if c == v] for k, v in mc.FAMILY.items()}
    q = np.concatenate([emb[rows["src"]], emb[rows["five"]]])
    qchain = np.asarray([(0, 3), (3, 5)], np.int32)
    return emb, starts, q, qchain, rows


def test_clip_chain_table():
    starts = np.asarray([0, 3, 4, 9, 12], np.int64)
    assert [x if isinstance(x, (int, bool)) else x.tolist() for x in md.clip_chain_table(starts, 0, 12)] == [[0, 3, 4, 9, 12], 0, False, False]
    assert [x if isinstance(x, (int, bool)) else x.tolist() for x in md.clip_chain_table(starts, 3, 9)] == [[0, 1, 6], 1, False, False]
    assert [x if isinstance(x, (int, bool)) else x.tolist() for x in md.clip_chain_table(starts, 5, 10)] == [[0, 4, 5], 2, True, True]
    assert [x if isinstance(x, (int, bool)) else x.tolist() for x in md.clip_chain_table(starts, 5, 6)] == [[0, 1], 2, True, True]
    assert [x if isinstance(x, (int, bool)) else x.tolist() for x in md.clip_chain_table(starts, 11, 12)] == [[0, 1], 3, True, False]


@pytest.mark.parametrize("shards", [1, 2, 3, 8])
def test_edge_rule_merged_candidates_after_phase_two_equal_the_unsharded_set(planted, shards):
    """Every shard scans its rows block by block (block sizes 1, 2, 7, n) with the restatement as the scan, under the clipped
    table; chains cut by a shard or block edge lose their verdict and become everybody's candidates.  After the exact decision on
    whole chains (phase 2) the merged set is the unsharded one -- which holds the planted relatives."""
    from merizo_search_amd.foldclass.sharded import shard_bounds
    emb, starts, q, qchain, rows = _planted_case(planted)
    n, nqc = len(emb), len(qchain)
    exact, _st = sc.scan_ref(emb, q, starts, qchain, MINCOS)
    chain_at = lambda key: int(np.searchsorted(starts, rows[key][0], side="right")) - 1
    assert {(0, chain_at("src")), (0, chain_at("inorder")), (0, chain_at("reversed")), (0, chain_at("inserted")), (1, chain_at("five")),
            (1, chain_at("five_copy"))} <= set(exact) and (0, chain_at("nearmiss")) not in exact
    whole = md.range_candidates(starts, 0, n, nqc, lambda table: sc.scan_ref(emb, q, table, qchain, MINCOS)[0])
    assert [tuple(p) for p in md.merge_candidates([whole]).tolist()] == exact
    for block in (1, 2, 7, n):
        parts, cut_chains = [], 0
        for rank in range(shards):
            lo, hi = shard_bounds(n, shards, rank)
            for a in range(lo, hi, block):
                b = min(hi, a + block)
                table, _first, cf, cl = md.clip_chain_table(starts, a, b)
                assert table[0] == 0 and table[-1] == b - a and (np.diff(table) > 0).all()
                cut_chains += int(cf) + int(cl)
                parts.append(md.range_candidates(starts, a, b, nqc, lambda t, a=a, b=b: sc.scan_ref(emb[a:b], q, t, qchain, MINCOS)[0]))
                assert len(parts[-1]) <= len(sc.scan_ref(emb[a:b], q, table, qchain, MINCOS)[0]) + 2 * nqc
        merged = [tuple(p) for p in md.merge_candidates(parts).tolist()]
        assert merged == sorted(set(merged)) and set(exact) <= set(merged), (shards, block)
        assert [p for p in merged if p in set(exact)] == exact
        if block < n and shards * block < n:
            assert cut_chains > 0 and len(merged) > len(exact)              # (some verdicts WERE discarded and decided again)


def test_candidate_plans_order_and_rows(planted):
    """Query chains in the order given, target chains by chain id, the rows of each run; a chain with fewer rows than the query
    chain has domains (an unconditional candidate from an edge) is dropped."""
    from merizo_search_amd.foldclass.dbquery import QueryDB
    work, names, chain_of = planted
    db = QueryDB(os.path.join(work, "pt"))
    starts = db.chain_starts()
    hits = {"B": {"B1": [], "B2": [], "B3": []}, "A": {"A1": [], "A2": []}}
    nch = len(starts) - 1
    pairs = np.asarray([(0, c) for c in range(nch)][::-1] + [(1, 5), (1, 2)], np.int64)
    plans = md.candidate_plans(pairs, ["B", "A"], hits, {"B": 0, "A": 3}, starts, db)
    db.close()
    long_enough = [c for c in range(nch) if starts[c + 1] - starts[c] >= 3]
    assert [p[0] for p in plans] == ["B"] * len(long_enough) + ["A"] * sum(1 for c in (2, 5) if starts[c + 1] - starts[c] >= 2)
    assert [p[1] for p in plans[: len(long_enough)]] == sorted(chain_of[starts[c]] for c in long_enough)
    for qc, hc, q0, nqd, grows in plans:
        assert (q0, nqd) == ((0, 3) if qc == "B" else (3, 2))
        assert [chain_of[r] for r in grows] == [hc] * len(grows) and grows.tolist() == [r for r, c in enumerate(chain_of) if c == hc]


def test_gather_pairs_is_the_identity_on_one_rank():
    from merizo_search_amd.foldclass import sharded
    pairs = np.asarray([(1, 2), (0, 7)], np.int64)
    assert np.array_equal(sharded.gather_pairs(pairs, "cpu"), pairs)
    assert sharded.gather_pairs(np.zeros((0, 2), np.int64), "cpu").shape == (0, 2)


# ------------------------------------------------------------------ 3. the command line ---
def test_argparse_accepts_the_mode_for_search_and_easy_search_only(monkeypatch, capsys):
    from merizo_search_amd import cli
    assert "database_cosine" in md.MODES
    seen = []
    monkeypatch.setattr(cli, "_join_process_group", lambda args: seen.append((args.multi_domain_search, args.multi_domain_mode)) or (_ for _ in ()).throw(KeyboardInterrupt()))
    for mode, argv in (("search", ["a.pdb", "db", "out", "tmp"]), ("easy-search", ["a.pdb", "db", "out", "tmp", "--chopping", "1-10"])):
        with pytest.raises(KeyboardInterrupt):
            cli.main([mode] + argv + ["--multi_domain_search", "--multi_domain_mode", "database_cosine"])
    assert seen == [(True, "database_cosine")] * 2
    with pytest.raises(SystemExit) as exc:
        cli.main(["db-search", "q", "t", "out", "tmp", "--multi_domain_search", "--multi_domain_mode", "database_cosine"])
    assert exc.value.code == 2 and "invalid choice: 'database_cosine'" in capsys.readouterr().err
    assert seen == [(True, "database_cosine")] * 2
    with pytest.raises(ValueError):
        md.multi_domain_search([], [], "db", "tmp", mode="database_tmalign")


# ------------------------------------------------------------------ 4. run_dbsearch(target_db) ---
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_run_dbsearch_target_db_none_takes_the_old_path(planted, tmp_path, monkeypatch, layout):
    """With target_db=None run_dbsearch opens the database itself, exactly once, as before; with the dict of an earlier open it
    opens nothing, returns the same results, and leaves the rows it made resident in that dict."""
    from oracle_engine import oracle_network
    from merizo_search_amd.foldclass import dbsearch as ds, synthetic as syn
    net = oracle_network(0)
    prefix = os.path.join(planted[0], layout)
    queries = [dict(coords=syn.random_walk(30 + i, 50 + i), seq="A" * (30 + i), name="q%d" % i) for i in range(3)]
    opened = []
    real = ds.read_database
    monkeypatch.setattr(ds, "read_database", lambda *a, **kw: opened.append(1) or real(*a, **kw))
    run = lambda **kw: ds.run_dbsearch([dict(q) for q in queries], prefix, str(tmp_path / "t"), "cpu", topk=4, fastmode=False, threads=-1,
                                       mincos=-1.0, mintm=0.5, mincov=0.0, inputs_are_ca=True, skip_tmalign=True, network=net, **kw)
    old = run()
    assert len(opened) == 1
    assert run(target_db=None) == old and len(opened) == 2
    target = real(prefix, engine=net.engine)
    assert run(target_db=target) == old and len(opened) == 2
    from merizo_search_amd.foldclass.target import Target
    resident = Target.cached(target, net.engine)
    if layout == "pt":
        assert resident.engine is net.engine and (resident.lo, resident.hi) == (0, len(planted[1]))
    else:
        assert (resident.lo, resident.hi) == (0, len(planted[1])) and resident.rows.shape == (len(planted[1]), 128)
