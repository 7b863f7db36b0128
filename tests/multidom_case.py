"""Helpers of the `exhaustive_cosine` multi-domain tests (TEST INFRASTRUCTURE; the product never imports this).

    chain_scores_ref   ms_md_chain_scores restated candidate by candidate; the cell score is a true fmaf chain (multidom_ref.c,
                       built on first use with the host gcc).  It takes PREPARED queries: the preparation is the scan's own
                       launch, which test 1 of test_multidom_gpu.py anchors to the product's scan
    driver_ref         the multi-domain step restated from group_hits, sibling_rows, chain_mappings and a score function
    install_oracle_md  OracleEngine.md_chain_scores: the oracle's own search scores (top-k with k = all rows, scattered back)
    write_planted      a small database in both layouts whose names form chains, with planted relatives
"""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from merizo_search_amd.foldclass import multidomain as md

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multidom_ref.c")
_lib = None
MAX_DOMAINS = 4096            # include/merizo_search_amd.h: nqd, nhd above it are refused like a bad descriptor


def _load():
    global _lib
    if _lib is None:
        base = os.environ.get("MS_TEST_CACHE") or os.path.join(tempfile.gettempdir(), "merizo_search_amd_%d" % os.getuid())
        os.makedirs(base, exist_ok=True)
        so = os.path.join(base, "multidom_ref_%s.so" % hashlib.sha256(open(_SRC, "rb").read()).hexdigest()[:16])
        if not os.path.exists(so):
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, _SRC, "-lm"], check=True)
            os.replace(tmp, so)
        _lib = ctypes.CDLL(so)
        _lib.md_dot_matrix.restype = None
        _lib.md_dot_matrix.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return _lib


def dot_matrix(q, t) -> np.ndarray:
    """float32 [nq,nt]: the scan's fmaf chain of every prepared query with every row."""
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 128)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 128)
    out = np.zeros((q.shape[0], t.shape[0]), np.float32)
    if out.size:
        _load().md_dot_matrix(q.ctypes.data, q.shape[0], t.ctypes.data, t.shape[0], out.ctypes.data)
    return out


def cut(scores, min_score) -> np.ndarray:
    """NaN and scores below min_score -> +0.0; a score equal to it stays."""
    scores = np.array(scores, dtype=np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        scores[~(scores >= np.float32(min_score))] = np.float32(0.0)
    return scores


def match_counts(matrix):
    nz = matrix != 0                                           # (-0.0 is zero)
    return int(nz.any(axis=1).sum()), int(nz.any(axis=0).sum())


def chain_scores_ref(db, qprep, cand, trows, mat_off, min_score, scores, match, lengths=None, qlen=None, mincov=0.0):
    """include/merizo_search_amd.h, ms_md_chain_scores, on copies of the output arrays `scores` / `match` as they were before
    the call (whatever it does not write keeps its value).  qprep: the queries as the scan of the mode prepares them."""
    db = np.asarray(db, np.float32).reshape(-1, 128)
    qprep = np.asarray(qprep, np.float32).reshape(-1, 128)
    n, nq = db.shape[0], qprep.shape[0]
    cand = np.asarray(cand, np.int64).reshape(-1, 4)
    trows = np.asarray(trows, np.int64)
    scores, match = np.array(scores, np.float32, copy=True), np.array(match, np.int32, copy=True)
    for c, (q0, nqd, t_off, nhd) in enumerate(cand):
        if (nqd < 1 or nhd < 1 or nqd > MAX_DOMAINS or nhd > MAX_DOMAINS or q0 < 0 or q0 + nqd > nq or t_off < 0
                or t_off + nhd > len(trows)):
            match[c] = (-1, -1)
            continue
        rows = trows[t_off: t_off + nhd]
        ok = (rows >= 0) & (rows < n)
        m = np.zeros((nqd, nhd), np.float32)
        if ok.any():
            s = dot_matrix(qprep[q0: q0 + nqd], db[rows[ok]])
            if lengths is not None:
                lim = (np.asarray(lengths, np.float32)[rows[ok]] * np.float32(mincov)).astype(np.float32)
                mk = (np.asarray(qlen, np.float32)[q0: q0 + nqd, None] >= lim[None, :]).astype(np.float32)
                with np.errstate(invalid="ignore"):
                    s = (s * mk).astype(np.float32)
            m[:, ok] = cut(s, min_score)
        scores[mat_off[c]: mat_off[c] + nqd * nhd] = m.reshape(-1)
        match[c] = match_counts(m)
    return scores, match


# ------------------------------------------------------------------ the oracle engine's scores
def oracle_scores(mode, rows, q, lengths=None, qlen=None, mincov=0.0) -> np.ndarray:
    """float32 [nq,nt]: what OracleEngine's search of `mode` reports for every (query, row): its top-k with k = all rows,
    scattered back by row."""
    from oracle import oracle as orc
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 128)
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 128)
    nt = rows.shape[0]
    if mode == "cosine":
        s, i = orc.cosine_topk(rows, q, nt, lengths, qlen, mincov)
    else:
        s, i = orc.ip_topk(rows, orc.l2_normalize_rows(q, 1e-12) if mode == "ip" else q, nt, order=1)
    out = np.zeros((q.shape[0], nt), np.float32)
    np.put_along_axis(out, i, s, axis=1)
    return out


def install_oracle_md():
    """OracleEngine.md_chain_scores = the oracle's own scores, cut and counted as the header defines (the CPU runs of the drivers)."""
    import torch
    from oracle_engine import OracleEngine

    def md_chain_scores(self, db, q, mode, cand, trows, mat_off, min_score, lengths=None, qlen=None, mincov=0.0, total=None):
        db, q = db.numpy(), q.numpy()
        cand, trows, mat_off = (np.asarray(x) for x in (cand, trows, mat_off))
        lengths = None if lengths is None else lengths.numpy()
        qlen = None if qlen is None else qlen.numpy()
        ends = [int(o) + int(c[1]) * int(c[3]) for c, o in zip(cand, mat_off)]
        scores = np.zeros(int(total) if total is not None else max(ends + [0]), np.float32)
        match = np.zeros((len(cand), 2), np.int32)
        for c, (q0, nqd, t_off, nhd) in enumerate(cand):
            rows = trows[t_off: t_off + nhd]
            m = cut(oracle_scores(mode, db[rows], q[q0: q0 + nqd], None if lengths is None else lengths[rows],
                                  None if qlen is None else qlen[q0: q0 + nqd], mincov), min_score)
            scores[mat_off[c]: mat_off[c] + nqd * nhd] = m.reshape(-1)
            match[c] = match_counts(m)
        return torch.from_numpy(scores), torch.from_numpy(match)

    OracleEngine.md_chain_scores = md_chain_scores
    return OracleEngine


# ------------------------------------------------------------------ the driver step, restated
def driver_ref(query_names, query_chains, search_results, n_rows, stored_name, entry_name, metadata, score_fn, mincos,
               own_rows=None, max_paths=None, skipped=None):
    """The multi-domain step from group_hits, sibling_rows, chain_mappings and score_fn alone: per query chain ONE matrix over
    the sorted rows of all its hit chains, entries below mincos -> 0, split by hit chain in np.unique order.
    score_fn(indices of the chain's query domains in query_names, database rows) -> float32 [nqd,nt];
    own_rows {chain: (lo, hi)}: hits in that row range seed nothing; max_paths: the enumeration cap (pairs above it go to
    `skipped` as (qc, hc))."""
    hits = md.group_hits(query_names, query_chains, search_results)
    where = {n: i for i, n in enumerate(query_names)}
    out = []
    for qc, domains in hits.items():
        nqd = len(domains)
        if nqd < 2:
            continue
        rows = set()
        for per_domain in domains.values():
            for hit in per_domain:
                if own_rows is not None and own_rows[qc][0] <= hit["hi"] < own_rows[qc][1]:
                    continue
                chain_rows = md.sibling_rows(hit["hi"], hit["hc"], n_rows, stored_name)
                if len(chain_rows) >= nqd:
                    rows.update(chain_rows)
        if not rows:
            continue
        rows = sorted(rows)
        scores = cut(score_fn([where[qd] for qd in domains], rows), mincos)
        hit_chain = np.asarray([md.domid2chainid(entry_name(r)) for r in rows])
        info = [{"hd": entry_name(r), "hc": hc, "hi": r, "hm": metadata(r)} for r, hc in zip(rows, hit_chain)]
        for hc in np.unique(hit_chain):
            cols = np.flatnonzero(hit_chain == hc)
            sub = scores[:, cols]
            nr, nc = match_counts(sub)
            if max_paths is not None and nr == nqd and nc >= nqd:
                paths = int(np.prod([int(np.count_nonzero(sub[r])) for r in range(nqd)], dtype=object))
                if paths > max_paths:
                    if skipped is not None:
                        skipped.append((qc, str(hc)))
                    continue
            out.extend(md.chain_mappings(sub, qc, str(hc), list(domains.keys()), [info[c] for c in cols]))
    return out


def search_results_from_tsv(path, row_of):
    """`_search.tsv` (default columns, no header) -> (query names in order of appearance, search_results as group_hits reads
    them); row_of: target name -> database row."""
    names, per_query = [], {}
    with open(path) as handle:
        for line in handle:
            f = line.rstrip("\n").split("\t")
            if f[0] not in per_query:
                names.append(f[0])
                per_query[f[0]] = {}
            per_query[f[0]][len(per_query[f[0]])] = {"query": f[0], "target": f[2], "dbindex": row_of[f[2]]}
    return names, [per_query[n] for n in names]


def tsv_rows(results):
    return ["\t".join(str(a) for a in res) + "\n" for res in results]


# ------------------------------------------------------------------ a planted database
FAMILY = {"src": "c00003", "inorder": "c00007", "reversed": "c00011", "inserted": "c00015", "nearmiss": "c00019",
          "five": "c00022", "five_copy": "c00026"}


def write_planted(work, seed=11, n_chains=34):
    """A database in BOTH layouts under `work` ('fa', 'pt') whose names form chains of 1..5 adjacent domains
    ('c00012_TED03'), random rows (pairwise cosines far below 0.5) and planted relatives of chain `src` (3 domains), each
    domain a noisy copy (cosine about 0.98): `inorder` (the copies in order), `reversed`, `inserted` (an unrelated domain
    between the first and the second copy), `nearmiss` (two copies and an unrelated domain); `five_copy` copies the 5
    domains of `five` in order.  Every domain of those chains has 40 residues (the `.pt` length mask passes both ways).
    -> (names, chain id per row)."""
    from merizo_search_amd.foldclass import dbutil, synthetic as syn
    os.makedirs(work, exist_ok=True)
    rng = np.random.default_rng(seed)
    planted = {int(v[1:]): k for k, v in FAMILY.items()}
    sizes = {"src": 3, "inorder": 3, "reversed": 3, "inserted": 4, "nearmiss": 3, "five": 5, "five_copy": 5}
    names, chain_of, vecs, lengths = [], [], [], []
    start = {}
    for c in range(n_chains):
        run = sizes[planted[c]] if c in planted else int(rng.integers(1, 6))
        start[c] = len(names)
        for d in range(run):
            names.append("c%05d_TED%02d" % (c, d + 1))
            chain_of.append("c%05d" % c)
            vecs.append(rng.standard_normal(128).astype(np.float32) * np.float32(rng.uniform(0.5, 2.0)))
            lengths.append(40 if c in planted else int(rng.integers(20, 61)))
    raw = np.stack(vecs)

    def copy_of(row):
        v = raw[row]
        return (v + 0.2 * np.linalg.norm(v) / np.sqrt(128.0) * rng.standard_normal(128)).astype(np.float32)

    at = {k: start[int(v[1:])] for k, v in FAMILY.items()}
    for d in range(3):
        raw[at["inorder"] + d] = copy_of(at["src"] + d)
        raw[at["reversed"] + d] = copy_of(at["src"] + 2 - d)
    for d, col in zip(range(3), (0, 2, 3)):
        raw[at["inserted"] + col] = copy_of(at["src"] + d)
    for d in range(2):
        raw[at["nearmiss"] + d] = copy_of(at["src"] + d)
    for d in range(5):
        raw[at["five_copy"] + d] = copy_of(at["five"] + d)
    n = len(names)
    seqs = ["".join(rng.choice(list("ACDEFGHIKL"), size=int(l))) for l in lengths]
    coords = [syn.random_walk(int(l), seed * 7919 + i) for i, l in enumerate(lengths)]
    norm = (raw / np.linalg.norm(raw, axis=1, keepdims=True)).astype(np.float32)
    dbutil.write_faiss_db(os.path.join(work, "fa"), norm, names, seqs, coords, metadata=['{ "row": %d }' % i for i in range(n)])
    dbutil.write_pt_db(os.path.join(work, "pt"), raw, ["/x/" + nm + ".pdb" for nm in names], coords, seqs)
    return names, chain_of


def oracle_pair_scores(layout, emb, seqlen, qrows, rows, mincov):
    """The oracle engine's search score of stored rows `qrows` (as queries) against stored rows `rows` of a database."""
    if layout == "fa":
        return oracle_scores("ip_prenorm", emb[rows], emb[qrows])
    return oracle_scores("cosine", emb[rows], emb[qrows], seqlen[rows], seqlen[qrows], mincov)


def expected_lines(planted, layout, search_tsv, pair_scores=oracle_pair_scores, lo=0, hi=None, own=False, mincos=0.5, mincov=0.7,
                   max_paths=None, skipped=None):
    """The lines of `_search_multi_dom.tsv` a self db-search over query rows [lo, hi) of the planted database must write:
    driver_ref applied to that run's `_search.tsv`.  planted = (work, names, chain id per row); own: the query chain's own rows
    seed no candidate (--exclude_self)."""
    from merizo_search_amd.foldclass import dbquery
    work, names, chain_of = planted
    hi = len(names) if hi is None else hi
    db = dbquery.QueryDB(os.path.join(work, layout))
    emb = db.embeddings(0, db.n)
    seqlen = np.asarray([len(x) for x in db.seqs(0, db.n)], np.float32)
    seen, results = search_results_from_tsv(search_tsv, {n: r for r, n in enumerate(names)})
    by_name = dict(zip(seen, results))
    qnames = names[lo:hi]
    own_rows = None
    if own:
        own_rows = {}
        for r in range(lo, hi):
            full = [i for i, c in enumerate(chain_of) if c == chain_of[r]]
            own_rows[chain_of[r]] = (full[0], full[-1] + 1)
    out = driver_ref(qnames, chain_of[lo:hi], [by_name.get(n, {}) for n in qnames], db.n, db.name, db.entry_name,
                     lambda r: db.name_meta(r)[1], lambda qi, rows: pair_scores(layout, emb, seqlen, [lo + i for i in qi], rows, mincov),
                     mincos, own_rows=own_rows, max_paths=max_paths, skipped=skipped)
    db.close()
    return tsv_rows(out)


def categories(lines, qc, hc):
    return sorted({l.split("\t")[4] for l in lines if l.split("\t")[0] == qc and l.split("\t")[2] == hc})


def check_planted_categories(lines):
    """The planted relatives of the source chain: in order -> 3, reversed -> 0, a domain inserted -> 1, one missing -> none."""
    assert categories(lines, FAMILY["src"], FAMILY["inorder"]) == ["3"]
    assert categories(lines, FAMILY["src"], FAMILY["reversed"]) == ["0"]
    assert categories(lines, FAMILY["src"], FAMILY["inserted"]) == ["1"]
    assert categories(lines, FAMILY["src"], FAMILY["nearmiss"]) == []
    assert categories(lines, FAMILY["five"], FAMILY["five_copy"]) == ["3"]
    assert all(l.split("\t")[0] != l.split("\t")[2] for l in lines)


def check_md_case_outputs(prefix, mincos=0.5):
    """The md_case scenario in mode exhaustive_cosine: T1 (both query domains in order, three target domains) is reported in
    category 2, T3 (order swapped) in category 0, the single-domain chain T2 never; every score is str() of a float32 at or
    above mincos."""
    rows = [l.rstrip("\n").split("\t") for l in open(prefix + "_search_multi_dom.tsv")]
    assert rows[0] == ["query_chain", "nqd", "hit_chain", "nhd", "match_category", "match_info", "hit_metadata"]
    body = rows[1:]
    pairs = lambda r: [tuple(e.split(":")[:2]) for e in r[5].split(",")]
    t1 = [r for r in body if r[2] == "AF-T1-F1-model_v4" and r[4] == "2"]
    assert any(pairs(r) == [("Q_merizo_01", "AF-T1-F1-model_v4_TED01"), ("Q_merizo_02", "AF-T1-F1-model_v4_TED02")] for r in t1), body
    assert all(r[:2] == ["Q", "2"] and r[3] == "3" for r in t1)
    t3 = [r for r in body if r[2] == "AF-T3-F1-model_v4" and r[4] == "0"]
    assert any(pairs(r) == [("Q_merizo_01", "AF-T3-F1-model_v4_TED02"), ("Q_merizo_02", "AF-T3-F1-model_v4_TED01")] for r in t3), body
    assert not any(r[2] == "AF-T2-F1-model_v4" for r in body)
    for r in body:
        for e in r[5].split(","):
            v = np.float32(e.split(":")[2])
            assert str(v) == e.split(":")[2] and v >= np.float32(mincos)
    return body
