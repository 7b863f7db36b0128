"""The multi-domain mode `database_cosine` through the drivers on the real engine: the md_case scenario at -k 1 (where
`exhaustive_cosine` loses chain T3), the planted database at the driver-function level against the restated driver fed with
complete hit lists, a streamed target, and two ranks under torchrun with a chain across the shard boundary."""
import os
import subprocess
import sys

import numpy as np
import pytest

import multidom_case as mc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINCOS, MINCOV = 0.5, 0.7


def _md_lines(prefix):
    return open(prefix + "_search_multi_dom.tsv", "rb").read()


def _easy(cli, qpdb, db, out, tmp, k, mode, extra=()):
    import md_case
    cli.main(["easy-search", qpdb, db, out, tmp, "-d", "cuda", "-k", str(k), "-s", "0.5", "-c", "0.0", "--chopping", md_case.CHOPPING,
              "--multi_domain_search", "--multi_domain_mode", mode, "--output_headers"] + list(extra))
    return out


# ------------------------------------------------------------------ 1. md_case ---
@pytest.mark.parametrize("layout", ["faiss", "pt"])
def test_md_case_at_k_1_reports_the_chain_the_top_k_lists_miss(tmp_path, monkeypatch, layout):
    """T1 and T3 hold the same two domains and identical embeddings tie by ascending row: at -k 1 both query domains hit T1 only.
    `exhaustive_cosine` then never looks at T3; `database_cosine` reports it, writes byte for byte what `exhaustive_cosine` writes
    at -k 6 (every row a hit), and `search` with the two domains as two PDB files maps the same targets under query chain A."""
    import md_case
    from merizo_search_amd import cli
    monkeypatch.setenv("MERIZO_ALLOW_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("MERIZO_TMALIGN", raising=False)
    monkeypatch.setenv("PATH", str(tmp_path / "nowhere"))
    qpdb, dbdir = md_case.write_inputs(tmp_path)
    db, tmp = str(tmp_path / "db"), str(tmp_path / "tmp")
    cli.main(["createdb", dbdir, db, "-d", "cuda", "--layout", layout])
    scan = _easy(cli, qpdb, db, str(tmp_path / "scan"), tmp, 1, "database_cosine")
    body = mc.check_md_case_outputs(scan, 0.5)                                   # T1 in category 2 AND T3 in category 0
    full = _easy(cli, qpdb, db, str(tmp_path / "full"), tmp, 6, "exhaustive_cosine")
    assert _md_lines(scan) == _md_lines(full) and _md_lines(scan).count(b"\n") > 2
    topk = _easy(cli, qpdb, db, str(tmp_path / "topk"), tmp, 1, "exhaustive_cosine")
    assert b"AF-T3-F1-model_v4" not in _md_lines(topk) and b"AF-T1-F1-model_v4" in _md_lines(topk)      # what the feature changes
    # `search`: the two query domains as two PDB files of one chain 'A'
    # (read_pdb looks at column 22 of every line, as the reference does: the copies leave the closing END line out)
    os.makedirs(str(tmp_path / "doms"))
    doms = []
    for d in (1, 2):
        doms.append(str(tmp_path / "doms" / ("AF-T1-F1-model_v4_TED0%d.pdb" % d)))
        with open(os.path.join(dbdir, os.path.basename(doms[-1]))) as src, open(doms[-1], "w") as dst:
            dst.writelines(l for l in src if l.startswith("ATOM"))
    out = str(tmp_path / "files")
    cli.main(["search"] + doms + [db, out, tmp, "-d", "cuda", "-k", "1", "-s", "0.5", "-c", "0.0", "--multi_domain_search", "--multi_domain_mode",
                                  "database_cosine", "--output_headers"])
    rows = [l.rstrip("\n").split("\t") for l in open(out + "_search_multi_dom.tsv")][1:]
    strip = lambda r: (r[1:5], [e.split(":")[1:] for e in r[5].split(",")], r[6])
    assert [r[0] for r in rows] == ["A"] * len(rows) and [strip(r) for r in rows] == [strip(r) for r in body]
    # a streamed target (faiss layout; the blocks of 5 rows cut chain T3): the same bytes
    if layout == "faiss":
        from merizo_search_amd.foldclass.engine import HipEngine
        monkeypatch.setattr(HipEngine, "resident_budget", lambda self, nq=0, k=0: 1 << 10)
        streamed = _easy(cli, qpdb, db, str(tmp_path / "streamed"), tmp, 1, "database_cosine", ["--search_batchsize", "5"])
        assert _md_lines(streamed) == _md_lines(scan)


# ------------------------------------------------------------------ 2. the planted database ---
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("md_scan_gpu"))
    names, chain_of = mc.write_planted(work)
    return work, names, chain_of


def _pair_scores(layout, emb, seqlen, qrows, rows, mincov):
    """What the search on the real engine scores stored rows `qrows` against stored rows `rows` with (the restatement of
    test_multidom_drivers_gpu.py): the faiss layout takes both as stored; the `.pt` layout normalises both with eps 1e-8 on the
    device and masks by length."""
    import torch
    from merizo_search_amd import ops
    if layout == "fa":
        return mc.dot_matrix(emb[qrows], emb[rows])
    unit = lambda x: ops.l2_normalize_rows(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda(), 1e-8).cpu().numpy()
    s = mc.dot_matrix(unit(emb[qrows]), unit(emb[rows]))
    mk = (seqlen[qrows][:, None] >= (seqlen[rows] * np.float32(mincov)).astype(np.float32)[None, :]).astype(np.float32)
    return (s * mk).astype(np.float32)


def _planted_run(planted, layout, engine, target_db, search_batchsize=262144):
    """The driver functions of the mode on query chains `src` and `five` (their stored rows are the query embeddings) ->
    (lines, candidate pairs, query rows, reader facts for the restated driver)."""
    from merizo_search_amd.foldclass import multidomain as md
    from merizo_search_amd.foldclass.dbquery import QueryDB
    work, names, chain_of = planted
    reader = QueryDB(os.path.join(work, layout))
    qrows = [r for key in ("src", "five") for r, c in enumerate(chain_of) if c == mc.FAMILY[key]]
    served = [mc.FAMILY["src"], mc.FAMILY["five"]]
    hits = {qc: {names[r]: [] for r in qrows if chain_of[r] == qc} for qc in served}
    q_first = {served[0]: 0, served[1]: 3}
    emb = reader.embeddings(0, reader.n)
    seqlen = np.asarray([len(s) for s in reader.seqs(0, reader.n)], np.float32)
    q_emb = engine.to_device(emb[qrows])
    mode, qlen, cov = ("ip_prenorm", None, 0.0) if layout == "fa" else ("cosine", engine.to_device(seqlen[qrows]), MINCOV)
    starts = reader.chain_starts()
    qchain = np.asarray([(0, 3), (3, 5)], np.int32)
    pairs = md.database_candidates(engine, reader, target_db, starts, q_emb, mode, qchain, MINCOS, qlen, cov, search_batchsize)
    plans = md.candidate_plans(pairs, served, hits, q_first, starts, reader)
    res = md.score_plans(plans, hits, q_emb, mode, engine, reader, lambda rows: md.compact_target_rows(engine, reader, rows), MINCOS,
                         qlen=qlen, mincov=cov)
    # the restated driver, fed with COMPLETE hit lists: every row at or above mincos is a hit of its query domain
    scores = _pair_scores(layout, emb, seqlen, qrows, list(range(reader.n)), MINCOV)
    results = [{k: {"query": names[qr], "target": reader.entry_name(int(r)), "dbindex": int(r)}
                for k, r in enumerate(np.flatnonzero(scores[i] >= np.float32(MINCOS)))} for i, qr in enumerate(qrows)]
    want = mc.driver_ref([names[r] for r in qrows], [chain_of[r] for r in qrows], results, reader.n, reader.name, reader.entry_name,
                         lambda r: reader.name_meta(r)[1],
                         lambda qi, rows: _pair_scores(layout, emb, seqlen, [qrows[i] for i in qi], rows, MINCOV), MINCOS)
    reader.close()
    return mc.tsv_rows(res), mc.tsv_rows(want), pairs


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_planted_database_equals_the_restated_driver_with_complete_hit_lists(planted, layout):
    """Resident rows (the dict a search leaves behind), then streamed in blocks of 7 rows (no target_db): the same lines, equal to
    driver_ref fed with every row at or above mincos; inorder -> 3, reversed -> 0, inserted -> 1, nearmiss absent, five_copy -> 3,
    and the query's own chain in category 3 (nothing excludes it)."""
    from merizo_search_amd.foldclass import dbsearch as ds
    from merizo_search_amd.foldclass.target import Target
    engine = ds.engine_setup("cuda:0")
    prefix = os.path.join(planted[0], layout)
    n = len(planted[1])
    if layout == "pt":
        target = ds.read_database(prefix, engine=engine)
    else:
        target = ds.read_database(prefix)
        resident = Target.of(target, engine, 8, 10)
        assert resident.rows is not None and (resident.lo, resident.hi) == (0, n)
    got, want, pairs = _planted_run(planted, layout, engine, target)
    assert got == want and len(got) > 5
    fam = mc.FAMILY
    assert mc.categories(got, fam["src"], fam["inorder"]) == ["3"] and mc.categories(got, fam["src"], fam["reversed"]) == ["0"]
    assert mc.categories(got, fam["src"], fam["inserted"]) == ["1"] and mc.categories(got, fam["src"], fam["nearmiss"]) == []
    assert mc.categories(got, fam["five"], fam["five_copy"]) == ["3"]
    assert "3" in mc.categories(got, fam["src"], fam["src"]) and "3" in mc.categories(got, fam["five"], fam["five"])
    streamed, _want, more = _planted_run(planted, layout, engine, None, search_batchsize=7)
    assert streamed == got
    assert {tuple(p) for p in pairs.tolist()} < {tuple(p) for p in more.tolist()}       # the block edges added candidates; phase 2 decided them


# ------------------------------------------------------------------ 3. two ranks ---
def test_two_ranks_on_one_gpu_write_the_bytes_of_one_process(tmp_path, monkeypatch):
    """`torchrun --nproc-per-node 2 -m merizo_search_amd.cli easy-search ... database_cosine` (both ranks on cuda:0 over gloo):
    every rank scans its 4 of the 8 rows, chain T1 (rows 2..4) straddles the shard boundary, the candidate lists are gathered,
    rank 0 writes the bytes one process writes.  Three processes use the GPU at most (this one and the two ranks)."""
    import md_case
    from conftest import free_port
    from merizo_search_amd import cli
    from merizo_search_amd.foldclass import multidomain as md, pdbio, synthetic as syn
    from merizo_search_amd.foldclass.sharded import shard_bounds
    monkeypatch.setenv("MERIZO_ALLOW_SYNTHETIC_WEIGHTS", "1")
    qpdb, dbdir = md_case.write_inputs(tmp_path)
    for d, (length, seed) in enumerate(((35, 21), (45, 22)), start=1):           # chain T0 in front: T1 moves to rows 2..4
        walk = np.round(syn.random_walk(length, seed).astype(np.float64), 3).astype(np.float32)
        pdbio.write_pdb(dbdir, walk, ("ACDEFGHIKLMNPQRSTVWY" * 5)[:length], name="AF-T0-F1-model_v4_TED0%d" % d)
    names = sorted(f for f in os.listdir(dbdir) if f.endswith(".pdb"))
    starts = md.chain_runs(names).tolist()
    assert starts == [0, 2, 5, 6, 8] and shard_bounds(8, 2, 0) == (0, 4) and starts[1] < 4 < starts[2]      # T1 straddles
    db = str(tmp_path / "db")
    cli.main(["createdb", dbdir, db, "-d", "cuda", "--layout", "faiss"])
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", MERIZO_SAME_DEVICE="1", PYTHONPATH=REPO, GLOO_SOCKET_IFNAME="lo",
               MERIZO_ALLOW_SYNTHETIC_WEIGHTS="1")
    argv = ["-m", "merizo_search_amd.cli", "easy-search", qpdb, db, None, str(tmp_path / "t"), "-d", "cuda", "-k", "1", "-s", "0.5", "-c", "0.0",
            "--chopping", md_case.CHOPPING, "--multi_domain_search", "--multi_domain_mode", "database_cosine", "--output_headers",
            "--skip_tmalign"]
    one = [a if a is not None else str(tmp_path / "one") for a in argv]
    two = [a if a is not None else str(tmp_path / "two") for a in argv]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable] + one, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + two, capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for suffix in ("_search.tsv", "_search_multi_dom.tsv"):
        assert open(str(tmp_path / "one") + suffix, "rb").read() == open(str(tmp_path / "two") + suffix, "rb").read(), suffix
    mc.check_md_case_outputs(str(tmp_path / "two"), 0.5)
