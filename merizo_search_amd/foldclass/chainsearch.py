"""`chain-search`: every multi-domain match between two databases.

The query side is a whole database: its query chains are the runs of adjacent query rows with one chain id (multidomain.chain_runs,
as `db-search --multi_domain_search` forms them), and for each of them EVERY chain of the target database is decided -- not only the
chains a top-k list names.  Per batch of whole query chains: multidomain.database_candidates (ms_md_chain_scan / ms_md_chain_scan_mq
over the resident target, this rank's shard under torchrun, or streamed blocks), then on rank 0 candidate_plans and score_plans,
unchanged, and the lines appended to `<output>_search_multi_dom.tsv`.

The file is the one `db-search query_db target_db --multi_domain_search --multi_domain_mode exhaustive_cosine --skip_tmalign -s S -c C
-k K` writes when K is at least the target's row count (every row at or above S is then a hit), on databases whose chains are
adjacent runs, with the same --query_rows and --exclude_same_chain."""
from __future__ import annotations

import logging
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import sharded
from .multidomain import MAX_MAPPING_PATHS, SCAN_MAX_DOMAINS

logger = logging.getLogger(__name__)


def served_runs(starts: np.ndarray, ids: Sequence[str], offset: int = 0, log=logger) -> List[Tuple[int, int, str]]:
    """The query chains a chain-search serves: (first row, one past the last row, chain id) of every run of chain_runs' table
    `starts` (local rows; `offset` makes them global) with 2..SCAN_MAX_DOMAINS domains.  ids: the chain id of every local row.
    Runs of one domain and runs of more than SCAN_MAX_DOMAINS are logged and skipped."""
    out = []
    for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
        qc = ids[a]
        if b - a < 2:
            log.debug("Query chain %s: only one detected domain, multi-domain hits equal the per-domain hits." % qc)
        elif b - a > SCAN_MAX_DOMAINS:
            log.warning("Query chain %s has %d domains, more than the %d the database scan serves per query chain: skipped"
                        % (qc, b - a, SCAN_MAX_DOMAINS))
        else:
            out.append((offset + a, offset + b, qc))
    return out


def chain_batches(runs: Sequence[Tuple[int, int, str]], batch_rows: int) -> List[List[Tuple[int, int, str]]]:
    """Whole query chains, in order, up to batch_rows query rows per batch (a batch always takes at least one chain); a chain id
    that comes back starts a new batch, as a batch's chains are keyed by their id."""
    batches, cur, rows, seen = [], [], 0, set()
    for run in runs:
        n = run[1] - run[0]
        if cur and (rows + n > batch_rows or run[2] in seen):
            batches.append(cur)
            cur, rows, seen = [], 0, set()
        cur.append(run)
        rows += n
        seen.add(run[2])
    if cur:
        batches.append(cur)
    return batches


def drop_own_chain(pairs: np.ndarray, first_rows: Sequence[int], target_starts: np.ndarray) -> np.ndarray:
    """The candidates (query chain of the batch, target chain) without the pairs whose target run holds the query chain's own first
    row: in a search of a database against itself a query chain is never its own candidate."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if not len(pairs):
        return pairs
    own = np.searchsorted(np.asarray(target_starts, np.int64), np.asarray(first_rows, np.int64), side="right") - 1
    return pairs[own[pairs[:, 0]] != pairs[:, 1]]


def run_chain_search(query_db: str, db_name: str, output: str, tmp: str, device="cuda", mincos: float = 0.5, mincov: float = 0.7,
                     query_batchsize: int = 4096, search_batchsize: int = 262144, query_rows: Optional[str] = None,
                     exclude_same_chain: bool = False, output_headers: bool = False, max_mapping_paths: Optional[int] = None,
                     route: str = "auto", engine=None, report: str = "all") -> int:
    """-> the number of query chains served.  report: 'all' = every mapping of a pair (capped by max_mapping_paths), 'best' = the
    best one(s) per pair with their score (multidomain.best_lines; no cap).  route: multidomain.database_candidates' ("auto": the matrix route from
    ops.MD_SCAN_MATRIX_MIN_NQ query rows per batch on; the file does not depend on it).  Under a process group every rank calls it;
    rank 0 writes."""
    from . import dbsearch
    from . import multidomain as md
    from .dbquery import QueryDB
    from .results import append_written, multi_dom_writer
    from .target import Target, score_mode as target_score_mode

    if engine is None:
        from .engine import resolve_device
        device = resolve_device(device)                                   # ('cpu' is refused here, before anything else)
    if not 0.0 <= float(mincov) <= 1.0:
        dbsearch._refuse("--mincov must lie in [0, 1], got %r." % (mincov,))
    if query_batchsize < 1 or search_batchsize < 1:
        dbsearch._refuse("--query_batchsize and --search_batchsize must be >= 1.")
    if report not in md.REPORTS:
        dbsearch._refuse("--multi_domain_report must be one of %s, got %r." % (", ".join(md.REPORTS), report))
    write_multi_dom = multi_dom_writer(report)
    target_db, qdb, same, q_lo, q_hi = dbsearch.open_query_and_target(
        query_db, db_name, query_rows,
        "--exclude_same_chain removes the query chain itself from its candidates: it needs" if exclude_same_chain else None)
    rank = sharded.rank_world()[0]
    os.makedirs(tmp, exist_ok=True)
    multi_output = output + "_search_multi_dom.tsv"
    if rank == 0:
        if os.path.exists(multi_output):
            logger.warning(f"Search output file '{multi_output}' already exists. Results will be overwritten!")
        open(multi_output, "w").close()

    engine = engine or dbsearch.engine_setup(device)
    ids = [md.domid2chainid(n) for n in qdb.stored_names(q_lo, q_hi)]
    runs = served_runs(md.chain_runs(qdb.stored_names(q_lo, q_hi)), ids, q_lo)
    batches = chain_batches(runs, int(query_batchsize))
    # the target: made resident once (streamed per batch beyond the HBM budget)
    nq_batch = max([sum(b - a for a, b, _qc in batch) for batch in batches] or [1])
    target = Target.of(target_db, engine, nq_batch, 1)
    reader = qdb if same else QueryDB(db_name)
    starts = reader.chain_starts()
    score_mode, masked = target_score_mode(target.faiss, qdb.normalized)
    cov = float(mincov) if masked else 0.0
    logger.info("chain-search: %d query chains of %s (rows %d..%d) against the %d chains of %s in %d batches%s"
                % (len(runs), query_db, q_lo, q_hi - 1, len(starts) - 1, db_name, len(batches),
                   "; the target is streamed in blocks of %d rows" % int(search_batchsize) if target.streamed else ""))
    target_rows = lambda rows: target.rows_for(rows, reader)
    max_paths = MAX_MAPPING_PATHS if max_mapping_paths is None else int(max_mapping_paths)
    part = os.path.join(tmp, "chain_search_batch.tsv")
    try:
        for number, batch in enumerate(batches):
            # the batch's query rows, chain after chain (the served chains need not be adjacent)
            emb, names, seqlen, q_first, qchain, at = [], [], [], {}, [], 0
            for a, b, qc in batch:
                emb.append(qdb.embeddings(a, b))
                names.extend(dbsearch._query_name(qd) for qd in qdb.records(a, b, with_coords=False))
                if score_mode == "cosine":
                    seqlen.extend(len(s) for s in qdb.seqs(a, b))
                q_first[qc] = at
                qchain.append((at, b - a))
                at += b - a
            chain_of = [qc for a, b, qc in batch for _ in range(b - a)]
            hits = md.group_hits(names, chain_of, [])
            q_emb = engine.to_device(np.concatenate(emb, axis=0))
            qlen = engine.to_device(np.asarray(seqlen, dtype=np.float32)) if score_mode == "cosine" else None
            pairs = md.database_candidates(engine, reader, target_db, starts, q_emb, score_mode, np.asarray(qchain, dtype=np.int32),
                                           mincos, qlen, cov, search_batchsize, route=route)
            if rank != 0:
                continue
            if exclude_same_chain:
                pairs = drop_own_chain(pairs, [a for a, _b, _qc in batch], starts)
            served = [qc for _a, _b, qc in batch]
            plans = md.candidate_plans(pairs, served, hits, q_first, starts, reader)
            results = md.score_plans(plans, hits, q_emb, score_mode, engine, reader, target_rows, mincos, qlen=qlen, mincov=cov,
                                     max_mapping_paths=max_paths, report=report)
            append_written(multi_output, part, lambda f: write_multi_dom(results, f, output_headers and number == 0))
            logger.info("chain-search: batch %d of %d done (%d query chains, %d candidate pairs)"
                        % (number + 1, len(batches), len(batch), len(pairs)))
        if rank == 0 and output_headers and not batches:
            write_multi_dom([], multi_output, True)
    finally:
        if reader is not qdb:
            reader.close()
        qdb.close()
    return len(runs)
