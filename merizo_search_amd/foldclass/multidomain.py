"""Multi-domain ("full-length") search on top of the per-domain top-k results.

Mirror of programs/Foldclass/dbsearch_fulllength.py.  Nothing here is on the GPU path: the
inputs are the hit dictionaries the (GPU) per-domain search produced, the work is
  1. group the query domains by query chain and their hits by target chain
     (dbsearch_fulllength.py:230-272);
  2. for every hit, walk the database index left and right to collect the sibling domains of
     the hit's chain -- database rows of one chain are adjacent (:346-394);
  3. TM-align every query domain of a chain against every collected target domain
     (external binary, a process pool; scores below mintm -> 0) (:55-92, :468-483);
  4. per (query chain, target chain) sub-matrix, enumerate the one-to-one assignments of query
     domains to target domains and classify them 0-3 (:95-180).
Step 3 needs a TM-align executable ($MERIZO_TMALIGN): without one the reference cannot run this
mode either, and `multi_domain_search` raises -- unless tmalign_backend='hip', which aligns the pairs of ALL query
chains in one GPU batch (ms_tmalign.hip) from the coordinates in memory, without files or processes.  Steps 1, 2 and 4 are plain functions, tested
against outputs of the reference's own functions (tests/golden/multidomain.json).

mode='exhaustive_cosine' (the "embscore mode" the reference leaves as a TODO, :202-203, :558-571) runs the same steps 1, 2 and
4 with another step 3: the matrix holds the SEARCH'S OWN score of (query domain, database row) -- bit for bit the emb_score
the per-domain search reports for that pair -- with entries below mincos set to 0.  All matrices of a call come from one
launch of ms_md_chain_scores (`cosine_step`), which also takes chain_mappings' two early exits on the device:
names and metadata are fetched only for the (query chain, hit chain) pairs that survive them.  No coordinates, no files, no
processes, no TM-align binary.

mode='database_cosine'  asks the same question of the WHOLE database instead of the chains the top-k lists
name: ms_md_chain_scan reads every row once and reports every (query chain, target chain) pair that passes chain_mappings' two
early exits (`database_candidates`; the target chains are the runs of adjacent rows with one chain id, `chain_runs`), and the
second half of `cosine_step` (`score_plans`) turns those pairs into the same result tuples.  Its answer does not depend on -k.

report='best' (both embedding-score modes) replaces step 4's enumeration: ms_md_best_mappings solves, on the device
buffers ms_md_chain_scores wrote, the best any-order and the best order-preserving mapping of every pair (`best_lines`).
"""
from __future__ import annotations

import itertools
import logging
import os
import re
import shutil
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .dbquery import QueryDB
from .dbrecords import Records, chain_runs, domid2chainid, equal_runs      # (callers and tests say md.chain_runs, md.domid2chainid)
from .pdbio import read_pdb, write_pdb
from .tmalign import align_many, check_backend, find_tmalign, run_tmalign

logger = logging.getLogger(__name__)

FIELD_SET_SEPARATOR = ","       # between the per-domain entries of one mapping
FIELD_SEPARATOR = ":"           # inside an entry: query domain : hit domain : TM score

MODES = ("exhaustive_tmalign", "exhaustive_cosine", "database_cosine")
SCAN_MAX_DOMAINS = 64           # database_cosine: query domains per query chain ms_md_chain_scan serves (include/merizo_search_amd.h)
# exhaustive_cosine: chain_mappings enumerates a Cartesian product; a (query chain, hit chain) pair with more paths than
# this is skipped with a warning (at database scale one pair of 12-domain chains could run for hours)
MAX_MAPPING_PATHS = 1_000_000
# what `<output>_search_multi_dom.tsv` holds: 'all' = every valid mapping of a pair (chain_mappings' enumeration, capped by
# MAX_MAPPING_PATHS); 'best' = per pair the best any-order mapping and, when that one breaks the order, the best order-preserving
# one, solved on the GPU (ms_md_best_mappings) -- no cap; the embedding-score modes only
REPORTS = ("all", "best")
BEST_MAX_HIT_DOMAINS = 1024     # report 'best': target domains per chain ms_md_best_mappings serves (MS_MD_BEST_MAX_HD)

_MERIZO_SUFFIX = re.compile(r"_merizo_[0-9]*$")


def mapping_category(path: Sequence[int], nhd: int) -> int:
    """The category of one one-to-one mapping (path[i] = the target domain of query domain i) onto a chain of nhd domains
    (:140-160): 3 = same number of domains, same order; 2 = order kept, contiguous target domains; 1 = order kept with gaps;
    0 = any order."""
    nqd = len(path)
    steps = np.diff(path)
    if nqd > 1 and not (steps > 0).all():
        return 0
    if nqd == nhd:
        return 3
    if (steps == 1).all():
        return 2
    return 1


def check_report(report: str, mode: str) -> None:
    """Refuse a report / mode combination before any work is done."""
    if report not in REPORTS:
        raise ValueError("Unrecognised multi-domain report: %s (expected one of: %s)" % (report, ", ".join(REPORTS)))
    if report == "best" and mode not in ("exhaustive_cosine", "database_cosine"):
        raise ValueError("--multi_domain_report best is served by the multi-domain modes exhaustive_cosine and database_cosine "
                         "(the embedding-score matrices on the GPU), not by %s" % mode)


def chain_mappings(tm: np.ndarray, query_chain: str, hit_chain: str, query_domains: Sequence[str],
                   hit_domains: Sequence[dict]) -> List[tuple]:
    """All one-to-one assignments of a chain's query domains (rows of `tm`) to the domains of one
    target chain (columns; dicts with 'hd' name and 'hm' metadata) whose TM scores are non-zero.

    Returns tuples (query_chain, nqd, hit_chain, nhd, category, 'qd:hd:tm,...', '[metadata,...]')
    in the reference's enumeration order (:95-180).  category: 3 = same number of domains, same
    order; 2 = order kept, contiguous target domains; 1 = order kept with gaps; 0 = any order."""
    tm = np.asarray(tm)
    nqd, nhd = tm.shape
    assert len(query_domains) == nqd and len(hit_domains) == nhd
    nonzero = tm != 0
    if not nonzero.any(axis=1).all():                 # a query domain matches nothing in this chain
        return []
    if int(nonzero.any(axis=0).sum()) < nqd:          # fewer matching target domains than query domains
        return []
    choices = [np.flatnonzero(nonzero[row]).tolist() for row in range(nqd)]
    out = []
    for path in itertools.product(*choices):
        if len(set(path)) != nqd:                     # two query domains on the same target domain
            continue
        category = mapping_category(path, nhd)
        info = [FIELD_SEPARATOR.join([query_domains[q], hit_domains[c]["hd"], str(tm[q, c])]) for q, c in enumerate(path)]
        meta = [hit_domains[c]["hm"] for c in path]
        out.append((query_chain, nqd, hit_chain, nhd, category, FIELD_SET_SEPARATOR.join(info),
                    "[" + FIELD_SET_SEPARATOR.join(meta) + "]"))
    return out


def sibling_rows(anchor: int, chain: str, n_rows: int, name_of: Callable[[int], str]) -> List[int]:
    """Database rows of the other domains of `chain` around row `anchor`, then `anchor` itself --
    empty if the chain has a single domain (:363-394).  Rows of a chain are adjacent; the walk
    stops at the database ends (the reference indexes past them)."""
    rows = []
    i = anchor - 1
    while i >= 0 and domid2chainid(name_of(i)) == chain:
        rows.append(i)
        i -= 1
    i = anchor + 1
    while i < n_rows and domid2chainid(name_of(i)) == chain:
        rows.append(i)
        i += 1
    if rows:
        rows.append(anchor)
    return rows


def tm_matrix(query_files: Sequence[str], target_files: Sequence[str], threads: int = -1, mintm: float = 0.5,
              options: Optional[str] = None, runner: Callable = run_tmalign) -> np.ndarray:
    """max(TM by query, TM by target) for every (query, target) pair; values below mintm -> 0
    (:55-92).  Pairs run concurrently (each one is a TM-align subprocess)."""
    pairs = [(q, t) for q in query_files for t in target_files]
    if not pairs:
        return np.zeros((len(query_files), len(target_files)))
    workers = threads if threads and threads > 0 else min(len(pairs), os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        results = list(pool.map(lambda p: runner(p[0], p[1], options, True), pairs))
    scores = np.asarray([max(r["qtm"], r["ttm"]) for r in results], dtype=np.float64)
    scores = scores.reshape(len(query_files), len(target_files))
    scores[scores < mintm] = 0.0
    return scores


def group_hits(query_names: Sequence[str], query_chains: Sequence[str], search_results) -> Dict[str, Dict[str, list]]:
    """{query chain: {query domain: [{'hc','hd','hi'}, ...]}} from the per-domain search results
    (a list of {rank: hit dict} as run_dbsearch returns them) (:246-272)."""
    index: Dict[str, Dict[str, list]] = {}
    chain_of = {}
    for qc, qd in zip(query_chains, query_names):
        index.setdefault(qc, {}).setdefault(qd, [])
        chain_of[qd] = qc
    for per_query in search_results:
        for hit in per_query.values():
            qd = hit["query"]
            index[chain_of[qd]][qd].append({"hc": domid2chainid(hit["target"]), "hd": hit["target"], "hi": int(hit["dbindex"])})
    return index


def multi_domain_search(queries, search_results, db_name: str, tmp_root: str, device=None, fastmode: bool = False,
                        threads: int = -1, mintm: float = 0.5, inputs_from_easy_search: bool = False,
                        mode: str = "exhaustive_tmalign", pdb_chain: Optional[str] = None, tmalign_backend: str = "auto",
                        mincos: float = 0.5, mincov: float = 0.7, network=None, max_mapping_paths: int = MAX_MAPPING_PATHS,
                        target_db: Optional[dict] = None, search_batchsize: int = 262144, report: str = "all"):
    """The reference's multi_domain_search (:183-574): same arguments, same result tuples (feed
    them to results.write_all_dom_search_results).  `queries`: PDB file names (search) or domain
    dicts with 'coords', 'seq', 'name' (easy-search).  tmalign_backend: 'auto' = the TM-align binary (required),
    'hip' = the GPU aligner on `device`.
    mode='exhaustive_cosine': step 3 scores with the search's own embedding score instead (entries below `mincos` -> 0; the
    `.pt` layout masks by `mincov` as its search does); needs no aligner.  `network`: the encoder the search ran with (set up
    from `device` when absent) -- the query embeddings are recomputed with it, bit-identical to the search's.
    mode='database_cosine': the lines `exhaustive_cosine` would write if every database row at or above mincos were a hit, from
    one pass over all rows (ms_md_chain_scan); search_results is not read (the answer does not depend on -k).  target_db: the
    dict the search opened this database into (dbsearch.read_database) -- its resident rows are then scanned in place; without
    it, or when they did not fit, the rows are streamed from the files in blocks of search_batchsize.  Under a process group
    EVERY rank must call it (each scans its shard); ranks other than 0 get None.
    report='best' (the two embedding-score modes): per (query chain, hit chain) pair the best mapping instead of every mapping --
    the eight-column tuples of best_lines, for results.write_best_dom_search_results; MAX_MAPPING_PATHS does not apply."""
    if mode not in MODES:
        raise ValueError("Unrecognised multi-domain search mode: " + mode)
    check_report(report, mode)
    if mode == "database_cosine":
        return _multi_domain_embedding(queries, None, db_name, device, inputs_from_easy_search, pdb_chain, mincos, mincov, network,
                                       threads, max_mapping_paths, True, target_db, search_batchsize, report)
    if mode == "exhaustive_cosine":
        return _multi_domain_embedding(queries, search_results, db_name, device, inputs_from_easy_search, pdb_chain, mincos, mincov,
                                       network, threads, max_mapping_paths, False, None, 0, report)
    check_backend(tmalign_backend, device)
    if len(queries) == 1:
        logger.warning("Cannot execute multi-domain search with only one query domain.")
        return None
    if tmalign_backend == "auto" and find_tmalign() is None:
        raise FileNotFoundError("multi-domain search aligns every query domain with every candidate target domain: "
                                "it needs a TM-align binary (set $MERIZO_TMALIGN)")
    names, query_chains, queries = _query_structures(queries, inputs_from_easy_search, pdb_chain)
    structures = dict(zip(names, queries))
    hits = group_hits(names, query_chains, search_results)

    store = Records(db_name)
    try:
        if tmalign_backend == "hip":
            return _multi_domain_hip(hits, structures, store, fastmode, mintm, device)
        results = []
        for qc, domains in hits.items():
            entries = _chain_entries(qc, domains, store)
            if entries is None:
                continue
            tmp = os.path.join(tmp_root, "MD_search_structures_" + qc)
            os.makedirs(tmp, exist_ok=True)
            try:
                qfiles = [write_pdb(tmp, structures[qd]["coords"], structures[qd]["seq"], name="FSQUERY-" + qd) for qd in domains]
                tfiles = [write_pdb(tmp, e[1], e[2], name="FSTARGET-" + e[0]) for e in entries]
                logger.info("TM-align %d query domains of chain %s against %d target domains" % (len(domains), qc, len(tfiles)))
                scores = tm_matrix(qfiles, tfiles, threads=threads, mintm=mintm, options="-fast" if fastmode else None)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            results.extend(_entry_mappings(scores, qc, list(domains.keys()), entries))
        return results
    finally:
        store.close()


def _entry_mappings(scores: np.ndarray, qc: str, qds: List[str], entries) -> list:
    """Step 4 for one query chain: its score matrix over `entries` (_chain_entries) split by the entries' chain id (np.unique
    order), chain_mappings per target chain."""
    hit_chain = np.asarray([domid2chainid(e[0]) for e in entries])
    info = [{"hd": e[0], "hc": hc, "hi": e[3], "hm": e[4]} for e, hc in zip(entries, hit_chain)]
    results = []
    for hc in np.unique(hit_chain):
        cols = np.flatnonzero(hit_chain == hc)
        results.extend(chain_mappings(scores[:, cols], qc, str(hc), qds, [info[c] for c in cols]))
    logger.info("Finished multi-domain search for query chain %s." % qc)
    return results


def _chain_entries(qc: str, domains: dict, store: Records):
    """The database entries of every hit chain with at least as many domains as query chain qc has (:346-394), or
    None (with the reference's log line) when there is nothing to align."""
    nqd = len(domains)
    if nqd < 2:
        logger.info("Query chain %s: only one detected domain, multi-domain hits equal the per-domain hits." % qc)
        return None
    rows = set()
    for per_domain in domains.values():
        for hit in per_domain:
            chain_rows = sibling_rows(hit["hi"], hit["hc"], store.n, store.name)
            if len(chain_rows) >= nqd:
                rows.update(chain_rows)
    if not rows:
        logger.info("Query chain %s: every hit chain has fewer domains than the query; try a larger -k." % qc)
        return None
    return [store.entry(r) for r in sorted(rows)]


def _multi_domain_hip(hits, structures, store, fastmode: bool, mintm: float, device) -> list:
    """Step 3 on the GPU: every query-domain x target-domain pair of every query chain in ONE align_many batch, then the
    per-chain matrices (max of the two TM-scores, below mintm -> 0, as tm_matrix) and steps 4 as on the binary path."""
    plans = []
    for qc, domains in hits.items():
        entries = _chain_entries(qc, domains, store)
        if entries is not None:
            plans.append((qc, list(domains.keys()), entries))
    items = [(structures[qd]["coords"], structures[qd]["seq"], e[1], e[2]) for _qc, qds, entries in plans for qd in qds
             for e in entries]
    logger.info("TM-align %d query-domain x target-domain pairs of %d query chains on the GPU" % (len(items), len(plans)))
    outs = align_many(items, fast=fastmode, device=device or "cuda")
    results, at = [], 0
    for qc, qds, entries in plans:
        n = len(qds) * len(entries)
        scores = np.asarray([max(o["qtm"], o["ttm"]) if o is not None else 0.0 for o in outs[at:at + n]], dtype=np.float64)
        at += n
        scores = scores.reshape(len(qds), len(entries))
        scores[scores < mintm] = 0.0
        results.extend(_entry_mappings(scores, qc, qds, entries))
    return results


# ------------------------------------------------------------------ exhaustive_cosine ---
def _query_structures(queries, inputs_from_easy_search: bool, pdb_chain: Optional[str]):
    """(names, query chains, structures) of multi_domain_search's inputs (:183-245)."""
    if not inputs_from_easy_search:
        chains = pdb_chain.rstrip(",").split(",") if pdb_chain else ["A"] * len(queries)
        if len(chains) == 1:
            chains = chains * len(queries)
        queries = [read_pdb(pdbfile=q, pdb_chain=c) for q, c in zip(queries, chains)]
    names = [os.path.basename(q["name"]) for q in queries]
    names = [n[: -len(".pdb")] if n.endswith(".pdb") else n for n in names]
    query_chains = [_MERIZO_SUFFIX.sub("", n) for n in names] if inputs_from_easy_search else ["A"] * len(names)
    return names, query_chains, list(queries)


def chain_target_rows(qc: str, domains: dict, n_rows: int, name_of: Callable[[int], str], own_rows=None, log=logger.info):
    """Step 2 for one query chain: the sorted database rows of every hit chain with at least as many domains as the query
    chain has (_chain_entries' row logic), or None (with the reference's log line) when there is nothing to score.
    own_rows = (lo, hi): hits inside that row range -- the query chain itself in a self-search -- seed no candidate."""
    nqd = len(domains)
    if nqd < 2:
        log("Query chain %s: only one detected domain, multi-domain hits equal the per-domain hits." % qc)
        return None
    rows = set()
    for per_domain in domains.values():
        for hit in per_domain:
            if own_rows is not None and own_rows[0] <= hit["hi"] < own_rows[1]:
                continue
            chain_rows = sibling_rows(hit["hi"], hit["hc"], n_rows, name_of)
            if len(chain_rows) >= nqd:
                rows.update(chain_rows)
    if not rows:
        log("Query chain %s: every hit chain has fewer domains than the query; try a larger -k." % qc)
        return None
    return sorted(rows)


def compact_target_rows(engine, reader, rows: np.ndarray):
    """Target rows read from the database files and uploaded as a compact matrix -- the path of a process that does not hold
    all rows resident (several ranks, a streamed target, `search` / `easy-search`).  reader: a dbquery.QueryDB of the target;
    rows: sorted unique global rows.  -> (matrix on the device, lengths on the device or None, local index of each row).
    `.pt` rows are normalised on the device by engine.cosine_rows (ms_l2_normalize_rows, eps 1e-8): the call the resident
    copy was made with, so the bits are the resident copy's."""
    rows = np.asarray(rows, dtype=np.int64)
    parts, lens = [], []
    for a, b in equal_runs((rows - np.arange(len(rows))).tolist()):       # one read per run of adjacent rows (a chain is one run)
        lo, hi = int(rows[a]), int(rows[b - 1]) + 1
        parts.append(reader.embeddings(lo, hi))
        if not reader.faiss:
            lens.extend(len(s) for s in reader.seqs(lo, hi))
    matrix = engine.to_device(np.concatenate(parts, axis=0) if parts else np.zeros((0, 128), np.float32))
    if reader.faiss:
        return matrix, None, np.arange(len(rows), dtype=np.int64)
    return engine.cosine_rows(matrix), engine.to_device(np.asarray(lens, dtype=np.float32)), np.arange(len(rows), dtype=np.int64)


def cosine_step(hits, q_first: Dict[str, int], q_emb, score_mode: str, engine, store: Records, target_rows: Callable,
                mincos: float, qlen=None, mincov: float = 0.0, own_rows: Optional[dict] = None,
                max_mapping_paths: int = MAX_MAPPING_PATHS, log=logger.info, skipped: Optional[list] = None, times=None,
                report: str = "all") -> list:
    """Steps 2-4 of `exhaustive_cosine` for the query chains of `hits` (group_hits' dictionary) -> result tuples.
    q_emb [nq,128] on the engine's device holds the query embeddings as the search took them, the domains of chain qc in
    rows [q_first[qc], q_first[qc] + nqd) in the order of hits[qc]; score_mode: 'ip' (raw queries, faiss layout), 'ip_prenorm'
    (stored faiss rows as queries) or 'cosine' (`.pt` layout, with qlen / mincov).  target_rows(sorted unique global rows) ->
    (matrix, lengths or None, local index per row).  ONE engine.md_chain_scores call scores every (query chain, hit chain)
    matrix; names and metadata are read for the pairs its match counts keep.  skipped: receives (qc, hc, paths) of the pairs
    above max_mapping_paths; times: dbsearch._DeviceTimes, which then receives the span of the scoring call ('md_scores').
    report: score_plans'."""
    plans = hit_chain_plans(hits, q_first, store, own_rows, log)
    return score_plans(plans, hits, q_emb, score_mode, engine, store, target_rows, mincos, qlen=qlen, mincov=mincov,
                       max_mapping_paths=max_mapping_paths, skipped=skipped, times=times, report=report)


def hit_chain_plans(hits, q_first: Dict[str, int], store: Records, own_rows: Optional[dict] = None, log=logger.info) -> list:
    """cosine_step's first half: (qc, hc, q0, nqd, global rows of the hit chain) for every chain the hits of a query chain name
    (step 2), query chains in the order of `hits`, hit chains per query chain in np.unique order of their chain id."""
    plans = []
    for qc, domains in hits.items():
        rows = chain_target_rows(qc, domains, store.n, store.name, own_rows.get(qc) if own_rows else None, log)
        if rows is None:
            continue
        hit_chain = np.asarray([domid2chainid(store.entry_name(r)) for r in rows])
        rows = np.asarray(rows, dtype=np.int64)
        for hc in np.unique(hit_chain):
            plans.append((qc, str(hc), int(q_first[qc]), len(domains), rows[hit_chain == hc]))
    return plans


def score_plans(plans, hits, q_emb, score_mode: str, engine, store: Records, target_rows: Callable, mincos: float, qlen=None,
                mincov: float = 0.0, max_mapping_paths: int = MAX_MAPPING_PATHS, skipped: Optional[list] = None, times=None,
                report: str = "all") -> list:
    """cosine_step's second half: plans (qc, hc, q0, nqd, global rows) -> result tuples.  ONE engine.md_chain_scores call for all
    matrices, chain_mappings' two early exits from its match counts, the max_mapping_paths skip, names and metadata for the
    pairs that remain, chain_mappings.
    report='best': the matrices stay on the device and go straight into ONE engine.md_best_mappings call; status, total, path and
    chosen cells come back, not the matrices, and best_lines forms the eight-column tuples.  No path cap applies; skipped receives
    (qc, hc, -2) for a pair beyond that call's limits (more than BEST_MAX_HIT_DOMAINS target domains)."""
    if report not in REPORTS:
        raise ValueError("Unrecognised multi-domain report: %s" % (report,))
    if not plans:
        return []
    needed = np.unique(np.concatenate([p[4] for p in plans]))
    matrix, lengths, local = target_rows(needed)
    cand = np.empty((len(plans), 4), np.int32)
    mat_off = np.empty(len(plans), np.int64)
    trows, t_off, m_off = [], 0, 0
    for c, (_qc, _hc, q0, nqd, grows) in enumerate(plans):
        cand[c] = (q0, nqd, t_off, len(grows))
        mat_off[c] = m_off
        trows.append(local[np.searchsorted(needed, grows)])
        t_off += len(grows)
        m_off += nqd * len(grows)
    cand_d, trows_d, off_d = engine.to_device(cand), engine.to_device(np.concatenate(trows)), engine.to_device(mat_off)
    t0 = times.mark() if times is not None else None
    scores, match = engine.md_chain_scores(matrix, q_emb, score_mode, cand_d, trows_d, off_d, float(mincos),
                                           lengths=lengths, qlen=qlen, mincov=float(mincov), total=m_off)
    if times is not None:
        times.add("md_scores", t0)
    if report == "best":
        t0 = times.mark() if times is not None else None
        best = engine.md_best_mappings(scores, cand_d, off_d)
        if times is not None:
            times.add("md_best", t0)
        return best_lines(plans, hits, store, *(t.cpu().numpy() for t in best), skipped=skipped)
    scores, match = scores.cpu().numpy(), match.cpu().numpy()
    results = []
    for c, (qc, hc, _q0, nqd, grows) in enumerate(plans):
        if match[c, 0] != nqd or match[c, 1] < nqd:           # chain_mappings' two early exits
            continue
        tm = scores[mat_off[c]: mat_off[c] + nqd * len(grows)].reshape(nqd, len(grows))
        paths = 1
        for row in range(nqd):
            paths *= int(np.count_nonzero(tm[row]))
        if paths > max_mapping_paths:
            logger.warning("multi-domain search: query chain %s x hit chain %s has %d candidate mappings (more than %d): skipped"
                           % (qc, hc, paths, max_mapping_paths))
            if skipped is not None:
                skipped.append((qc, hc, paths))
            continue
        info = []
        for r in grows:
            hd, hm = store.name_meta(int(r))
            info.append({"hd": hd, "hc": hc, "hi": int(r), "hm": hm})
        results.extend(chain_mappings(tm, qc, hc, list(hits[qc].keys()), info))
    return results


def best_lines(plans, hits, store: Records, status, total, path, cell, skipped: Optional[list] = None) -> list:
    """Report 'best': md_best_mappings' outputs for `plans` -> tuples (query_chain, nqd, hit_chain, nhd, category, 'score',
    'qd:hd:score,...', '[metadata,...]').  Per pair with an any-order mapping (kind-0 status 1) one line for it and, when its
    category is 0 and an order-preserving mapping exists (kind-1 status 1), a second line for that one.  score: the float64 sum
    of the path's cells in row order, '%.6f'.  Within a query chain the pairs are ordered by the kind-0 integer total,
    descending, ties in plan order; query chains keep the order of `plans`.  Names and metadata are read for reported pairs only."""
    chain_rank, order = {}, []
    for c, (qc, hc, _q0, nqd, grows) in enumerate(plans):
        chain_rank.setdefault(qc, len(chain_rank))
        if status[c, 0] == -2:
            logger.warning("multi-domain search: query chain %s x hit chain %s has %d x %d domains (the best-mapping step serves "
                           "up to %d x %d): skipped" % (qc, hc, nqd, len(grows), SCAN_MAX_DOMAINS, BEST_MAX_HIT_DOMAINS))
            if skipped is not None:
                skipped.append((qc, hc, -2))
        elif status[c, 0] < 0:
            raise RuntimeError("multi-domain search: ms_md_best_mappings refused the descriptor of %s x %s" % (qc, hc))
        elif status[c, 0] == 1:
            order.append(c)
    order.sort(key=lambda c: (chain_rank[plans[c][0]], -int(total[c, 0])))           # (stable: ties stay in plan order)
    results = []
    for c in order:
        qc, hc, _q0, nqd, grows = plans[c]
        qds = list(hits[qc].keys())
        info = {}
        kinds = [0]
        if mapping_category(path[c, 0, :nqd], len(grows)) == 0 and status[c, 1] == 1:
            kinds.append(1)
        for kind in kinds:
            cols = [int(j) for j in path[c, kind, :nqd]]
            for j in cols:
                if j not in info:
                    info[j] = store.name_meta(int(grows[j]))
            cells = cell[c, kind, :nqd]
            score = float(np.sum(cells.astype(np.float64)))
            fields = [FIELD_SEPARATOR.join([qds[i], info[j][0], str(cells[i])]) for i, j in enumerate(cols)]
            results.append((qc, nqd, hc, len(grows), mapping_category(cols, len(grows)), "%.6f" % score,
                            FIELD_SET_SEPARATOR.join(fields), "[" + FIELD_SET_SEPARATOR.join(info[j][1] for j in cols) + "]"))
    return results


# ------------------------------------------------------------------ database_cosine ---
def clip_chain_table(starts: np.ndarray, a: int, b: int):
    """The chain table of rows [a, b) (a < b) of a database whose chains start at `starts` (chain_runs), local to a:
    -> (int64 table [m + 1] from 0 to b - a, global number of its first chain, first chain cut by a?, last chain cut by b?)."""
    first = int(np.searchsorted(starts, a, side="right")) - 1
    last = int(np.searchsorted(starts, b, side="left"))
    table = np.clip(starts[first: last + 1], a, b) - a
    return np.ascontiguousarray(table, dtype=np.int64), first, bool(starts[first] < a), bool(starts[last] > b)


def range_candidates(starts: np.ndarray, a: int, b: int, nqc: int, scan: Callable) -> np.ndarray:
    """The candidates a process finds in rows [a, b) -- its shard, or one streamed block: int64 [m,2] = (query chain, GLOBAL
    target chain).  scan(table) -> the qualifying (query chain, local chain) pairs of those rows under the clipped table.
    The edge rule: the verdict on a chain that a or b cuts was formed on a part of its rows, so it is discarded and the chain
    becomes a candidate of EVERY query chain (at most two chains per range; the scoring half decides them exactly, on all their
    rows).  No state crosses ranges."""
    if b <= a or nqc < 1:
        return np.zeros((0, 2), np.int64)
    table, first, cut_first, cut_last = clip_chain_table(starts, a, b)
    pairs = np.asarray(scan(table), dtype=np.int64).reshape(-1, 2)
    cut = sorted(({0} if cut_first else set()) | ({len(table) - 2} if cut_last else set()))
    pairs = pairs[~np.isin(pairs[:, 1], cut)] + np.asarray([0, first], np.int64)
    extra = np.asarray([(g, first + c) for c in cut for g in range(nqc)], dtype=np.int64).reshape(-1, 2)
    return np.concatenate([pairs, extra], axis=0)


def merge_candidates(parts: Sequence[np.ndarray]) -> np.ndarray:
    """Candidate lists of several ranges -> one list without duplicates, sorted by (query chain, target chain)."""
    parts = [np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in parts]
    if not parts:
        return np.zeros((0, 2), np.int64)
    return np.unique(np.concatenate(parts, axis=0), axis=0)


def database_candidates(engine, reader, target_db: Optional[dict], starts: np.ndarray, q_emb, score_mode: str, qchain: np.ndarray,
                        mincos: float, qlen, mincov: float, search_batchsize: int = 262144, route: str = "lane") -> np.ndarray:
    """ms_md_chain_scan over this process's rows of the database -> the candidates of ALL rows, identical on every rank (a
    collective under a process group: sharded.gather_pairs).  The rows: the resident copy the search left in target_db
    (target.Target.for_reader) read in place; else streamed from the files once more, block by block (Target.blocks), each
    block a range of its own (range_candidates).
    route: engine.md_chain_scan's (the pairs do not depend on it)."""
    from . import sharded
    from .target import Target
    nqc = int(qchain.shape[0])
    qchain_d = engine.to_device(np.ascontiguousarray(qchain, dtype=np.int32))
    kw = {} if route == "lane" else {"route": route}              # (engines without a matrix route keep their signature)
    target = Target.for_reader(target_db, engine, reader)
    if target.hi > target.lo:
        logger.info("multi-domain search: scanning the %d resident rows of this process for matching chains" % (target.hi - target.lo)
                    if not target.streamed else
                    "multi-domain search: the database rows are not resident: streaming rows %d..%d once more for the chain scan, "
                    "in blocks of %d" % (target.lo, target.hi - 1, max(1, int(search_batchsize))))
    parts = []
    for block, a, lengths in target.blocks(reader, search_batchsize):
        scan = lambda table: engine.md_chain_scan(block, engine.to_device(table), q_emb, score_mode, qchain_d, float(mincos),
                                                  lengths=lengths, qlen=qlen, mincov=float(mincov), **kw)[0]
        parts.append(range_candidates(starts, a, a + int(block.shape[0]), nqc, scan))
    return merge_candidates([sharded.gather_pairs(merge_candidates(parts), engine.device)])


def candidate_plans(pairs: np.ndarray, served: Sequence[str], hits, q_first: Dict[str, int], starts: np.ndarray,
                    store: Records) -> list:
    """Candidates (index into `served`, target chain number) -> the plans score_plans takes, in `exhaustive_cosine`'s order: query
    chains as `hits` has them, target chains per query chain by chain id (np.unique's order; two runs with one id: by row)."""
    plans = []
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    for g, qc in enumerate(served):
        nqd = len(hits[qc])
        chains = []
        for c in pairs[pairs[:, 0] == g, 1]:
            a, b = int(starts[c]), int(starts[c + 1])
            if b - a >= nqd:                                  # (a cut chain is everybody's candidate; fewer domains cannot match)
                chains.append((domid2chainid(store.entry_name(a)), a, b))
        for hc, a, b in sorted(chains):
            plans.append((qc, hc, int(q_first[qc]), nqd, np.arange(a, b, dtype=np.int64)))
    return plans


def _multi_domain_embedding(queries, search_results, db_name, device, inputs_from_easy_search, pdb_chain, mincos, mincov, network,
                            threads, max_mapping_paths, whole_database: bool, target_db, search_batchsize, report: str = "all"):
    """Both embedding-score modes.  whole_database (`database_cosine`): the candidates are every (query chain, target chain) pair
    of the database that passes the two early exits (database_candidates: EVERY rank of a process group scans its rows and
    takes part in the gather; rank 0 alone goes on to the scoring half and returns results, the others return None); else
    (`exhaustive_cosine`) the chains the hits of search_results name.  The query embeddings are recomputed with the search's
    encoder (ragged embedding is bit-identical to one-by-one); the scoring half reads its target rows from the database files
    (compact_target_rows)."""
    if len(queries) == 1:
        logger.warning("Cannot execute multi-domain search with only one query domain.")
        return None
    from .target import score_mode as target_score_mode
    names, query_chains, structures = _query_structures(queries, inputs_from_easy_search, pdb_chain)
    if len(set(names)) != len(names):
        raise ValueError("multi-domain search: query domain names must be unique")
    hits = group_hits(names, query_chains, [] if whole_database else search_results)
    if network is None:
        from . import dbsearch
        network, _device = dbsearch.network_setup(threads=threads, device=device)
    engine = network.engine
    order = [i for qc in hits for i, c in enumerate(query_chains) if c == qc]        # the domains of a chain made adjacent
    q_first, at = {}, 0
    for qc, domains in hits.items():
        q_first[qc] = at
        at += len(domains)
    q_emb = engine.to_device(network.embed_many([structures[i]["coords"] for i in order]))
    reader = QueryDB(db_name)
    try:
        qlen = None if reader.faiss else engine.to_device(np.asarray([len(structures[i]["seq"]) for i in order], dtype=np.float32))
        score_mode, masked = target_score_mode(reader.faiss, False)
        cov = mincov if masked else 0.0
        target_rows = lambda rows: compact_target_rows(engine, reader, rows)
        if not whole_database:
            return cosine_step(hits, q_first, q_emb, score_mode, engine, reader, target_rows, mincos, qlen=qlen, mincov=cov,
                               max_mapping_paths=max_mapping_paths, report=report)
        served = []
        for qc, domains in hits.items():
            if len(domains) < 2:
                logger.info("Query chain %s: only one detected domain, multi-domain hits equal the per-domain hits." % qc)
            elif len(domains) > SCAN_MAX_DOMAINS:
                logger.warning("Query chain %s has %d domains, more than the %d the database scan serves per query chain: skipped"
                               % (qc, len(domains), SCAN_MAX_DOMAINS))
            else:
                served.append(qc)
        if not served:
            return []
        starts = reader.chain_starts()
        qchain = np.asarray([(q_first[qc], len(hits[qc])) for qc in served], dtype=np.int32)
        pairs = database_candidates(engine, reader, target_db, starts, q_emb, score_mode, qchain, mincos, qlen, cov, search_batchsize)
        from . import sharded
        if sharded.rank_world()[0] != 0:
            return None
        plans = candidate_plans(pairs, served, hits, q_first, starts, reader)
        return score_plans(plans, hits, q_emb, score_mode, engine, reader, target_rows, mincos, qlen=qlen, mincov=cov,
                           max_mapping_paths=max_mapping_paths, report=report)
    finally:
        reader.close()
