"""db-search on the GPU: ms_topk_drop_ranges against its numpy restatement (bits), exactness of the over-fetch + drop against a
database with the rows physically removed, queries read in place from the resident rows, parity with `search` on the same
structures, self-search with exclusions, two ranks, a streamed target."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import dbquery_case as dq

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NINF = -np.inf
EMB_FMT = "query,emb_rank,target,emb_score,q_len,t_len,metadata"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. the kernel ---------------
def _lists(nq, kin, seed):
    """Sorted lists with runs of equal scores and (-inf, -1) tails of every length, and per query one of five exclusion ranges:
    none (lo >= hi), the whole list, the head, the tail, a run across the first 64-entry piece boundary (or the middle)."""
    rng = np.random.default_rng(seed)
    scores = np.sort(np.round(rng.random((nq, kin)) * 12) / np.float32(16), axis=1)[:, ::-1].astype(np.float32)
    idx = np.empty((nq, kin), np.int64)
    lo, hi = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    for q in range(nq):
        real = kin if q % 3 else int(rng.integers(0, kin + 1))                    # every third list is padded (possibly entirely)
        kind = q % 5
        a, b = {0: (0, 0), 1: (0, kin), 2: (0, min(kin, 3)), 3: (max(0, real - 4), real), 4: (min(60, kin // 2), min(kin, 70))}[kind]
        b = max(a, min(b, kin))
        rows = 5000 + rng.permutation(4 * kin + 8)[:kin].astype(np.int64) * 3      # rows outside the excluded block
        base = 1000 + 7 * q
        rows[a:b] = base + np.arange(b - a)                                        # the excluded block: adjacent rows
        rows[real:] = -1
        scores[q, real:] = NINF
        idx[q] = rows
        lo[q], hi[q] = (base, base + (b - a)) if kind else (base + 5, base + 5 - (q % 2))      # kind 0: lo == hi or lo > hi
        if kind == 1:
            lo[q], hi[q] = 0, 1 << 40
    return scores, idx, lo, hi


@pytest.mark.parametrize("kin", [1, 11, 64, 65, 200])
@pytest.mark.parametrize("nq", [1, 33, 257])
def test_drop_kernel_equals_the_numpy_restatement_bit_for_bit(nq, kin):
    import torch
    from merizo_search_amd import ops
    scores, idx, lo, hi = _lists(nq, kin, seed=1000 * nq + kin)
    d_s, d_i = torch.from_numpy(scores).cuda(), torch.from_numpy(idx).cuda()
    inside = float(np.median(scores[np.isfinite(scores)])) if np.isfinite(scores).any() else 0.5
    short = 0
    for kout in sorted({1, (kin + 1) // 2, max(1, kin - 1), kin}):
        for cut in (NINF, -1.0, inside, 0.40, 2.0):                                # no cut, below, inside, between two levels, above all
            want = dq.drop_ranges_np(scores, idx, lo, hi, cut, kout)
            got = ops.topk_drop_ranges(d_s, d_i, lo, hi, kout, cut)
            got = [t.cpu().numpy() for t in got]
            assert np.array_equal(got[1], want[1]), (kout, cut)
            assert np.array_equal(_bits(got[0]), _bits(want[0])), (kout, cut)
            assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), (kout, cut)
            short += int((want[2] < kout).sum())
    assert short > 0 or nq == 1                                                    # survivors < kout were among the cases
    # preallocated outputs, device-side lo / hi
    out = (torch.full((nq, kin), 7.0, device="cuda"), torch.full((nq, kin), 7, dtype=torch.int64, device="cuda"),
           torch.full((nq,), 7, dtype=torch.int32, device="cuda"))
    got = ops.topk_drop_ranges(d_s, d_i, torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda(), kin, NINF, out=out)
    want = dq.drop_ranges_np(scores, idx, lo, hi, NINF, kin)
    assert got[0] is out[0] and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_drop_kernel_refuses_what_the_header_says():
    import torch
    from merizo_search_amd import ops
    from merizo_search_amd._lib import MerizoHipError
    s, i = torch.zeros((4, 8), device="cuda"), torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    z = np.zeros(4, np.int64)
    for kout in (0, 9):
        with pytest.raises(MerizoHipError, match="kout"):
            ops.topk_drop_ranges(s, i, z, z, kout)
    with pytest.raises(MerizoHipError, match="expected 4 rows"):
        ops.topk_drop_ranges(s, i, np.zeros(3, np.int64), z, 2)
    with pytest.raises(MerizoHipError):
        ops.topk_drop_ranges(s, i.int(), z, z, 2)


# ------------------------------------------------------------------ 2. exactness end to end -----
def _self_queries(n, nq, seed):
    """Unit rows, chains of 1..7 adjacent rows, nq query rows spread over the database (two of them neighbours in one chain)."""
    from merizo_search_amd.foldclass import synthetic as syn
    db = syn.normalized_database(n, seed=seed)
    _names, first, last = dq.chain_names(n, seed=seed + 1)
    rows = (np.arange(nq, dtype=np.int64) * (n - 1)) // (nq - 1)
    rows[1] = rows[0] + 1
    db[rows[5] + 9] = db[rows[5]]                                                 # an exact duplicate of a query outside its chain
    assert int((last - first).max()) == 7
    return db, rows, first, last


def test_topk_excluding_equals_the_oracle_on_the_database_without_the_rows():
    import torch
    from oracle import oracle as orc
    from merizo_search_amd import ops
    n, nq, k = 5000, 130, 10
    db, rows, first, last = _self_queries(n, nq, seed=31)
    d_db = torch.from_numpy(db).cuda()
    s, i, c = ops.topk_excluding(d_db, d_db[rows].contiguous(), k, first[rows], last[rows])
    s, i, c = s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()
    assert (c == k).all()
    for j, r in enumerate(rows):
        keep = np.r_[0:first[r], last[r]:n]
        ref_s, ref_i = orc.ip_topk(np.ascontiguousarray(db[keep]), db[r:r + 1], k, order=1)
        assert np.array_equal(i[j], keep[ref_i[0]]), r
        assert np.array_equal(_bits(s[j]), _bits(ref_s[0])), r
    assert i[5, 0] == rows[5] + 9                                                 # the duplicate is the best remaining hit


@pytest.fixture(scope="module")
def above_the_prefilter_floor():
    """70,001 rows x 130 queries: ms_ip_topk at k + 7 followed by the numpy drop, computed once."""
    import torch
    from merizo_search_amd import ops
    n, nq, k = 70_001, 130, 10
    db, rows, first, last = _self_queries(n, nq, seed=41)
    d_db = torch.from_numpy(db).cuda()
    d_q = d_db[rows].contiguous()
    s, i = ops.ip_topk(d_db, d_q, k + 7)
    want = dq.drop_ranges_np(s.cpu().numpy(), i.cpu().numpy(), first[rows], last[rows], NINF, k)
    return d_db, d_q, k, first[rows], last[rows], want


@pytest.mark.parametrize("image", [False, True])
def test_topk_excluding_takes_the_prefiltered_search_just_above_its_floor(above_the_prefilter_floor, image):
    from merizo_search_amd import ops
    d_db, d_q, k, lo, hi, want = above_the_prefilter_floor
    bound = 1.0 + 1e-6
    img = ops.pf_build_image(d_db, row_norm_bound=bound) if image else None
    assert ops.prefilter_serves(d_db.shape[0], d_q.shape[0], k + 7, img)
    ws = ops.PrefilterWorkspace(d_db.device)
    s, i, c = ops.topk_excluding(d_db, d_q, k, lo, hi, row_norm_bound=bound, image=img, workspace=ws, max_excluded=7)
    assert ws.buf is not None                                                     # the prefiltered search ran
    assert np.array_equal(i.cpu().numpy(), want[1]) and np.array_equal(_bits(s.cpu().numpy()), _bits(want[0]))
    assert np.array_equal(c.cpu().numpy(), want[2])


# ------------------------------------------------------------------ the driver, in process ------
@pytest.fixture(scope="module")
def engine():
    from merizo_search_amd.foldclass import dbsearch as ds
    return ds.engine_setup("cuda:0")


def _db_search(engine, query, target, out, tmp, **kw):
    from merizo_search_amd.foldclass import dbsearch as ds
    args = dict(topk=3, mincos=-2.0, skip_tmalign=True, format_list=EMB_FMT.split(","), header=True, engine=engine)
    args.update(kw)
    ds.run_dbsearch_db(query, target, str(out), str(tmp), "cuda:0", **args)
    return open(str(out) + "_search.tsv", "rb").read()


@pytest.fixture(scope="module")
def chain_case(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("dbq_gpu"))
    names, first, last = dq.write_case(work, n=20_000, seed=8)
    return work, names, first, last


# ------------------------------------------------------------------ 3. queries in place ---------
def test_in_place_queries_equal_copied_queries_bit_for_bit(chain_case, engine, tmp_path):
    import torch
    from merizo_search_amd import ops
    work = chain_case[0]
    db = torch.from_numpy(np.fromfile(os.path.join(work, "fa_raw_128d_norm.db"), np.float32).reshape(-1, 128)).cuda()
    for i0, i1, k in ((0, 70, 10), (4097, 4097 + 131, 17), (19_999, 20_000, 3)):    # (a slice that starts at an odd row; one query)
        view = db[i0:i1]
        assert view.data_ptr() == db.data_ptr() + 512 * i0 and view.data_ptr() % 16 == 0
        copy = view.clone()
        for mode in (ops.MODE_IP_PRENORM, ops.MODE_IP_NORMQ):
            a, b = ops.ip_topk(db, view, k, mode=mode), ops.ip_topk(db, copy, k, mode=mode)
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    # the driver: self-search of the slice [4097, 4400) in place == the same against a copy of the database under another
    # prefix (its queries go through the host)
    other = tmp_path / "copy"
    other.mkdir()
    for f in os.listdir(work):
        if f.startswith("fa"):
            shutil.copy(os.path.join(work, f), other / f)
    fa = os.path.join(work, "fa")
    ta, tb = {}, {}
    a = _db_search(engine, fa, fa, tmp_path / "in_place", tmp_path / "t", query_rows="4097:4400", query_batchsize=128, timings=ta)
    b = _db_search(engine, fa, str(other / "fa"), tmp_path / "copied", tmp_path / "t", query_rows="4097:4400", query_batchsize=128,
                   timings=tb)
    assert ta["in_place"] is True and tb["in_place"] is False and not ta["streamed"] and not tb["streamed"]
    assert a == b and a.count(b"\n") == 1 + 3 * 303


# ------------------------------------------------------------------ 5. self-search --------------
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_exclude_self_equals_the_unfiltered_search_without_the_self_row(chain_case, engine, tmp_path, layout):
    work, names, _first, _last = chain_case
    db = os.path.join(work, layout)
    kw = dict(query_rows="100:1500", query_batchsize=512, mincov=0.0)
    dq_excl = _db_search(engine, db, db, tmp_path / "excl", tmp_path / "t", topk=3, exclude_self=True, **kw)
    plain = _db_search(engine, db, db, tmp_path / "plain", tmp_path / "t", topk=4, **kw)
    excl = [r for r in dq.read_tsv(str(tmp_path / "excl") + "_search.tsv")[1:]]
    assert all(r[0] != r[2] for r in excl) and len(excl) == 3 * 1400
    want, seen = [], {}
    for r in dq.read_tsv(str(tmp_path / "plain") + "_search.tsv")[1:]:
        if r[0] == r[2]:
            continue
        rank = seen.get(r[0], 0)
        if rank < 3:
            want.append([r[0], str(rank)] + r[2:])
            seen[r[0]] = rank + 1
    assert excl == want
    assert [r[0] for r in excl] == [n for n in names[100:1500] for _ in range(3)]
    assert dq_excl != plain


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_exclude_same_chain_reports_no_row_of_the_querys_chain(chain_case, engine, tmp_path, layout):
    from merizo_search_amd.foldclass.multidomain import domid2chainid
    work, names, first, last = chain_case
    db = os.path.join(work, layout)
    _db_search(engine, db, db, tmp_path / "chain", tmp_path / "t", topk=5, exclude_same_chain=True, query_rows="7:900",
               query_batchsize=300, mincov=0.0)
    rows = dq.read_tsv(str(tmp_path / "chain") + "_search.tsv")[1:]
    assert len(rows) == 5 * 893 and all(domid2chainid(r[0]) != domid2chainid(r[2]) for r in rows)
    assert int((last - first)[7:900].max()) > 1                                   # (there were chains to exclude)
    # and it is the unfiltered search at k + 7 without those rows
    _db_search(engine, db, db, tmp_path / "plain", tmp_path / "t", topk=12, query_rows="7:900", mincov=0.0)
    want, seen = [], {}
    for r in dq.read_tsv(str(tmp_path / "plain") + "_search.tsv")[1:]:
        rank = seen.get(r[0], 0)
        if domid2chainid(r[0]) != domid2chainid(r[2]) and rank < 5:
            want.append([r[0], str(rank)] + r[2:])
            seen[r[0]] = rank + 1
    assert rows == want


# ------------------------------------------------------------------ 7. a streamed target --------
def test_streamed_target_equals_the_resident_run(chain_case, tmp_path):
    from merizo_search_amd.foldclass import dbsearch as ds
    work = chain_case[0]
    fa, pt = os.path.join(work, "fa"), os.path.join(work, "pt")
    small = ds.engine_setup("cuda:0")
    small.resident_budget = lambda nq=0, k=0: 1 << 20                             # 1 MiB: 20,000 rows do not fit
    big = ds.engine_setup("cuda:0")
    for name, query, kw in (("self", fa, dict(exclude_same_chain=True, query_rows="4000:4700", query_batchsize=256)),
                            ("raw", pt, dict(query_rows=":130", mincos=0.2))):
        ta, tb = {}, {}
        a = _db_search(small, query, fa, tmp_path / (name + "_stream"), tmp_path / "t", search_batchsize=4099, timings=ta, **kw)
        b = _db_search(big, query, fa, tmp_path / (name + "_res"), tmp_path / "t", timings=tb, **kw)
        assert ta["streamed"] is True and ta["in_place"] is False and tb["streamed"] is False and tb["in_place"] is (name == "self")
        assert a == b and a.count(b"\n") > 100, name


# ------------------------------------------------------------------ 4. parity with `search` -----
@pytest.fixture(scope="module")
def structure_case(tmp_path_factory):
    """createdb (both layouts) on the four golden PDBs plus 300 synthetic structures of 20..300 residues."""
    from merizo_search_amd import cli
    from merizo_search_amd.foldclass import pdbio, synthetic as syn
    root = tmp_path_factory.mktemp("dbq_parity")
    pdbs = root / "pdbs"
    pdbs.mkdir()
    for f in ("M0_ca.pdb", "3w5h_ca.pdb", "AF-Q96HM7-F1-model_v4_ca.pdb", "AF-Q96PD2-F1-model_v4_ca.pdb"):
        shutil.copy(os.path.join(GOLDEN, f), pdbs / f)
    names, coords, seqs = syn.synthetic_structures(300, seed=17, min_len=20, max_len=300)
    for n, c, s in zip(names, coords, seqs):
        path = pdbio.write_pdb(str(pdbs), np.round(c.astype(np.float64), 3).astype(np.float32), s, name=os.path.basename(n).replace(".pdb", ""))
        with open(path) as handle:                  # `search` reads column 22 of every line, as the reference does: no short END line
            atoms = [line for line in handle if line.startswith("ATOM")]
        with open(path, "w") as handle:
            handle.writelines(atoms)
    old = os.environ.get("MERIZO_ALLOW_SYNTHETIC_WEIGHTS")
    os.environ["MERIZO_ALLOW_SYNTHETIC_WEIGHTS"] = "1"
    try:
        for layout in ("pt", "faiss"):
            cli.createdb([str(pdbs), str(root / ("db_" + layout)), "--layout", layout])
    finally:
        if old is None:
            del os.environ["MERIZO_ALLOW_SYNTHETIC_WEIGHTS"]
    return root, sorted(str(pdbs / f) for f in os.listdir(pdbs))


def _without_query_column(path):
    rows = dq.read_tsv(path)
    assert all(len(r) > 1 for r in rows)
    return [r[1:] for r in rows]


@pytest.mark.parametrize("tm", ["skip", "hip"])
@pytest.mark.parametrize("layout", ["pt", "faiss"])
def test_db_search_equals_search_on_the_same_structures(structure_case, tmp_path, monkeypatch, layout, tm):
    from merizo_search_amd import cli
    monkeypatch.setenv("MERIZO_ALLOW_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("MERIZO_TMALIGN", raising=False)
    root, pdbs = structure_case
    db = str(root / ("db_" + layout))
    flags = ["-k", "5", "--output_headers", "--report_insignificant_hits"] + (["--skip_tmalign"] if tm == "skip" else ["--tmalign_backend", "hip"])
    cli.search(pdbs + [db, str(tmp_path / "search"), str(tmp_path / "t1")] + flags)
    cli.db_search([db, db, str(tmp_path / "dbsearch"), str(tmp_path / "t2"), "--query_batchsize", "128"] + flags)
    for suffix in ("_search.tsv", "_search_insignificant.tsv"):
        a, b = _without_query_column(str(tmp_path / "search") + suffix), _without_query_column(str(tmp_path / "dbsearch") + suffix)
        assert a == b, suffix
    hits = dq.read_tsv(str(tmp_path / "dbsearch") + "_search.tsv")
    assert len(hits) > 304 and hits[0][0] == "query"
    assert hits[1][0] == os.path.basename(pdbs[0]).replace(".pdb", "")             # the stored name, in row order


# ------------------------------------------------------------------ 6. two ranks ----------------
def test_db_search_two_ranks_on_one_gpu_equal_one_process(chain_case, tmp_path):
    """`torchrun --nproc-per-node 2 -m merizo_search_amd.cli db-search` (both ranks on cuda:0 over gloo) against the one-process
    command: sharded rows, over-fetch on every rank, exchange + merge, then the drop; byte-identical files."""
    from conftest import free_port
    work = chain_case[0]
    env = dict(os.environ, MERIZO_DIST_BACKEND="gloo", MERIZO_SAME_DEVICE="1", PYTHONPATH=REPO, GLOO_SOCKET_IFNAME="lo")
    fa = os.path.join(work, "fa")
    argv = ["-m", "merizo_search_amd.cli", "db-search", fa, fa, None, str(tmp_path / "t"), "-k", "4", "-s", "0.1", "--skip_tmalign",
            "--exclude_same_chain", "--query_rows", "9000:11000", "--query_batchsize", "700", "--format", EMB_FMT, "--output_headers"]
    one = [a if a is not None else str(tmp_path / "one") for a in argv]
    two = [a if a is not None else str(tmp_path / "two") for a in argv]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable] + one, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + two, capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b = open(str(tmp_path / "one") + "_search.tsv", "rb").read(), open(str(tmp_path / "two") + "_search.tsv", "rb").read()
    assert a == b and a.count(b"\n") > 2000
