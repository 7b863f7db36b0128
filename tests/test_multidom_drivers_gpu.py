"""`exhaustive_cosine` through the drivers on the real engine: `easy-search` on the md_case scenario without an aligner, and
a self `db-search --multi_domain_search` over the planted database in both layouts -- on the resident path and with the target
streamed -- equal to the restated driver whose score is the kernel's (fmaf chain of the prepared operands)."""
import os

import numpy as np
import pytest

import multidom_case as mc

pytestmark = pytest.mark.gpu
FMT = "query,emb_rank,target,emb_score,q_len,t_len,metadata"
MINCOS, MINCOV, K = 0.5, 0.7, 10


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("multidom_gpu"))
    names, chain_of = mc.write_planted(work)
    return work, names, chain_of


def _gpu_pair_scores(layout, emb, seqlen, qrows, rows, mincov):
    """What the search on the real engine scores stored rows `qrows` against stored rows `rows` with: the faiss layout takes
    both as stored (MS_MODE_IP_PRENORM); the `.pt` layout normalises both with eps 1e-8 on the device and masks by length."""
    import torch
    from merizo_search_amd import ops
    if layout == "fa":
        return mc.dot_matrix(emb[qrows], emb[rows])
    unit = lambda x: ops.l2_normalize_rows(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda(), 1e-8).cpu().numpy()
    s = mc.dot_matrix(unit(emb[qrows]), unit(emb[rows]))
    mk = (seqlen[qrows][:, None] >= (seqlen[rows] * np.float32(mincov)).astype(np.float32)[None, :]).astype(np.float32)
    return (s * mk).astype(np.float32)


def _run(planted, tmp_path, tag, layout, engine=None, timings=None, **kw):
    from merizo_search_amd.foldclass import dbsearch as ds
    db = os.path.join(planted[0], layout)
    out = str(tmp_path / tag)
    args = dict(topk=K, mincos=MINCOS, mincov=MINCOV, skip_tmalign=True, format_list=FMT.split(","), exclude_same_chain=True,
                multi_domain_search=True)
    args.update(kw)
    ds.run_dbsearch_db(db, db, out, str(tmp_path / "t"), "cuda:0", engine=engine or ds.engine_setup("cuda:0"), timings=timings, **args)
    return out


def test_easy_search_exhaustive_cosine_on_the_gpu_without_an_aligner(tmp_path, monkeypatch):
    import md_case
    from merizo_search_amd import cli
    monkeypatch.setenv("MERIZO_ALLOW_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("MERIZO_TMALIGN", raising=False)
    monkeypatch.setenv("PATH", str(tmp_path / "nowhere"))
    qpdb, dbdir = md_case.write_inputs(tmp_path)
    for layout in ("faiss", "pt"):
        db, out = str(tmp_path / ("db_" + layout)), str(tmp_path / ("out_" + layout))
        cli.main(["createdb", dbdir, db, "-d", "cuda", "--layout", layout])
        cli.main(["easy-search", qpdb, db, out, str(tmp_path / "tmp"), "-d", "cuda", "-k", "3", "-s", "0.5", "-c", "0.0", "--chopping",
                  md_case.CHOPPING, "--multi_domain_search", "--multi_domain_mode", "exhaustive_cosine", "--output_headers"])
        body = mc.check_md_case_outputs(out, 0.5)
        _scores_agree_with_the_search(out + "_search.tsv", body, header=True, target_col=5, score_col=6)


def _scores_agree_with_the_search(search_tsv, md_rows, header=False, target_col=2, score_col=3):
    """Every cosine of match_info whose (query domain, target) pair is a line of `_search.tsv` formats to that line's emb_score."""
    lines = [l.rstrip("\n").split("\t") for l in open(search_tsv)][1 if header else 0:]
    emb = {(f[0], f[target_col]): f[score_col] for f in lines}
    seen = 0
    for r in md_rows:
        for e in r[5].split(","):
            qd, hd, v = e.split(":")
            if (qd, hd) in emb:
                assert "{:.4f}".format(np.float32(v)) == emb[(qd, hd)], (qd, hd, v)
                seen += 1
    assert seen > 0


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_db_search_multi_domain_on_the_gpu_equals_the_restated_driver(planted, tmp_path, layout):
    times = {}
    out = _run(planted, tmp_path, "res", layout, timings=times, query_batchsize=16)
    assert times["md_resident"] is True and times["streamed"] is False and times["md_scores_calls"] >= 1
    got = open(out + "_search_multi_dom.tsv").readlines()
    assert got == mc.expected_lines(planted, layout, out + "_search.tsv", _gpu_pair_scores, mincos=MINCOS, mincov=MINCOV) and len(got) > 5
    mc.check_planted_categories(got)
    _scores_agree_with_the_search(out + "_search.tsv", [l.rstrip("\n").split("\t") for l in got])


def test_db_search_multi_domain_with_a_streamed_target_writes_the_same_bytes(planted, tmp_path):
    """A resident budget too small for the rows: the scan streams the target and the step reads the chain runs it needs from
    the database files."""
    from merizo_search_amd.foldclass import dbsearch as ds
    ta, tb = {}, {}
    small = ds.engine_setup("cuda:0")
    small.resident_budget = lambda nq=0, k=0: 1 << 10
    a = _run(planted, tmp_path, "stream", "fa", engine=small, timings=ta, search_batchsize=37, query_batchsize=16)
    b = _run(planted, tmp_path, "res", "fa", timings=tb, query_batchsize=16)
    assert ta["streamed"] is True and ta["md_resident"] is False and tb["md_resident"] is True
    for suffix in ("_search.tsv", "_search_multi_dom.tsv"):
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read() and os.path.getsize(a + suffix) > 0, suffix
