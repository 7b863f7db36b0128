"""`cluster`: a database made non-redundant on the GPU (no counterpart in the reference).

The self-search of `db-search --exclude_self` (dbsearch._BatchScan: the scan at k + 1, the exchange + merge under several
ranks, the drop of the own row and of everything below --mincos) writes each batch's neighbour lists straight into rows
[b0, b1) of two device tensors [n,k]; ms_cluster_greedy turns that graph into representatives and assignments.  The lists
never reach the host.  Output `<output>_cluster.tsv`: representative, member, cosine -- one line per database row.

The clustering's definition is the header's (include/merizo_search_amd.h, ms_cluster_greedy): an edge needs a cosine at or
above --mincos in either direction and the shorter domain to cover --mincov of the longer; the longer domain is the
representative (cd-hit's greedy order), every other domain goes to its best-scoring adjacent representative.  Coverage is that
SYMMETRIC rule on the edge: the search itself runs without the one-sided query-length mask of `search`.
"""
from __future__ import annotations

import logging
import math
import os
from typing import Optional

import numpy as np

from . import dbsearch as ds
from . import sharded
from .dbsearch import _BatchScan, _DeviceTimes, _refuse, _require_database, read_database
from .target import Target

logger = logging.getLogger(__name__)


def database_lengths(target_db: dict, qdb) -> np.ndarray:
    """Domain lengths int32 [n] of an opened database: the `.pt` layout's `lengths` (read_database), the faiss layout's
    sequence offsets (end - start of the int64 pairs of `sif`, one view of the mapped file)."""
    if qdb.faiss:
        offsets = np.frombuffer(qdb.store.seq[0], dtype=np.int64).reshape(-1, 2)
        return (offsets[:, 1] - offsets[:, 0]).astype(np.int32)
    return np.asarray(target_db["lengths"]).astype(np.int32)


def write_cluster_tsv(path: str, names, rep: np.ndarray, rep_score: np.ndarray, header: bool) -> None:
    """Clusters by the representative's row; its own line first, then its members by row.  The cosine column is formatted as
    results.write_search_results formats emb_score."""
    rows = np.arange(rep.shape[0], dtype=np.int64)
    order = np.lexsort((rows, rows != rep, rep))
    with open(path, "w") as handle:
        if header:
            handle.write("representative\tmember\temb_score\n")
        for r in order:
            handle.write("%s\t%s\t%s\n" % (names[int(rep[r])], names[int(r)], "{:.4f}".format(rep_score[r])))


def run_cluster(db_name: str, output: str, tmp: str, device="cuda", topk: int = 20, mincos: Optional[float] = None,
                mincov: float = 0.7, query_batchsize: int = 4096, search_batchsize: int = 262144, header: bool = False,
                engine=None, timings: Optional[dict] = None):
    """Cluster the rows of database `db_name` and write `<output>_cluster.tsv`.  topk: neighbours kept per row (the search
    fetches topk + 1 and drops the row itself); a row whose topk entries all count as edges may have neighbours the clustering
    never sees (`saturated`: raise -k).  Under several ranks every rank scans its shard of the rows; rank 0 alone keeps the
    graph, clusters and writes.  -> (rep int64 [n], rep_score float32 [n], info) as numpy arrays on rank 0, (None, None, info)
    elsewhere; info: n, n_reps, singletons, rounds, saturated.  `timings`: as run_dbsearch_db's, plus the HIP-event span of
    ms_cluster_greedy ('cluster_ms')."""
    from .dbquery import QueryDB

    if engine is None:
        from .engine import resolve_device
        device = resolve_device(device)                                   # ('cpu' is refused here, before anything else)
    if mincos is None or math.isnan(float(mincos)):
        _refuse("cluster needs -s/--mincos: the cosine at or above which two domains are neighbours (there is no default).")
    if not 0.0 <= float(mincov) <= 1.0:                                   # (NaN fails both comparisons)
        _refuse("-c/--mincov must lie in [0, 1], got %r." % (mincov,))
    if topk < 1 or query_batchsize < 1 or search_batchsize < 1:
        _refuse("-k, --query_batchsize and --search_batchsize must be >= 1.")
    _require_database(db_name)
    target_db = read_database(db_name=db_name)                            # (host side only: nothing is uploaded yet)
    qdb = QueryDB(db_name, loaded=target_db if not target_db["faiss"] else None)
    n, k = int(qdb.n), int(topk)
    if k + 1 > n:
        _refuse("-k %d plus the row itself exceed the %d rows of the database." % (k, n))
    lengths = database_lengths(target_db, qdb)
    rank, _world = sharded.rank_world()
    out_path = output + "_cluster.tsv"
    if rank == 0 and os.path.exists(out_path):
        logger.warning(f"Cluster output file '{out_path}' already exists. Results will be overwritten!")
    if not os.path.exists(tmp):
        os.makedirs(tmp, exist_ok=True)

    engine = engine or ds.engine_setup(device)
    torch = engine.torch
    times = _DeviceTimes(engine, timings)
    scan = _BatchScan(Target.of(target_db, engine, min(int(query_batchsize), n), k + 1), qdb, True, k + 1, search_batchsize, times)
    if timings is not None:
        timings["in_place"], timings["streamed"] = scan.in_place, scan.streamed
    logger.info("cluster: %d rows of %s, %d neighbours per row at cosine >= %s, coverage >= %s, batches of %d%s"
                % (n, db_name, k, mincos, mincov, int(query_batchsize),
                   "; queries read in place from the resident rows" if scan.in_place else ""))
    own = engine.to_device(np.arange(n + 1, dtype=np.int64))              # row q excludes [q, q + 1): slices of one array
    nbr_s = nbr_i = count = None
    if rank == 0:                                                         # the graph: rank 0's device, never the host
        nbr_s = torch.empty((n, k), dtype=torch.float32, device=engine.device)
        nbr_i = torch.empty((n, k), dtype=torch.int64, device=engine.device)
        count = torch.empty((n,), dtype=torch.int32, device=engine.device)
    for b0 in range(0, n, int(query_batchsize)):
        b1 = min(n, b0 + int(query_batchsize))
        seqs = None if target_db["faiss"] else qdb.seqs(b0, b1)
        out = (nbr_s[b0:b1], nbr_i[b0:b1], count[b0:b1]) if rank == 0 else None
        scan.search(b0, b1, seqs, 0.0, own[b0:b1], own[b0 + 1:b1 + 1], k, float(mincos), out=out)
    info = {"n": n, "k": k}
    if rank != 0:
        times.finish()
        qdb.close()
        return None, None, info
    t0 = times.mark()
    rep, rep_score, found = engine.cluster_greedy(nbr_i, nbr_s, lengths, float(mincos), float(mincov))
    times.add("cluster", t0)
    times.finish()
    rep, rep_score = rep.cpu().numpy(), rep_score.cpu().numpy()
    sizes = np.bincount(rep, minlength=n)
    info.update(found, singletons=int((sizes == 1).sum()))
    write_cluster_tsv(out_path, qdb.names(0, n), rep, rep_score, header)
    qdb.close()
    logger.info("cluster: %d clusters (%d singletons) of %d rows in %d rounds -> %s"
                % (info["n_reps"], info["singletons"], n, info["rounds"], out_path))
    if info["saturated"] > 0:
        logger.warning("cluster: %d rows have all %d kept neighbours above the thresholds: their lists may have been cut short "
                       "and neighbours beyond them are unknown to the clustering. Raise -k." % (info["saturated"], k))
    return rep, rep_score, info
