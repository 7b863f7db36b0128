"""`cluster`: a database made non-redundant on the GPU (no counterpart in the reference).

The self-search of `db-search --exclude_self` (dbsearch._BatchScan: the scan at k + 1, the exchange + merge under several
ranks, the drop of the own row and of everything below --mincos) writes each batch's neighbour lists straight into rows
[b0, b1) of two device tensors [n,k]; ms_cluster_greedy turns that graph into representatives and assignments.  The lists
never reach the host.  Output `<output>_cluster.tsv`: representative, member, cosine -- one line per database row.

`--complete` (run_cluster(complete=True)) makes the answer independent of -k: the rows whose lists came back FULL get all
their neighbours at the threshold from one more pass (ms_threshold_edges: every cell of those rows against the whole database,
decided against the fixed threshold), and ms_cluster_greedy_edges clusters the lists plus those entries -- the true threshold
graph ("The complete graph").

`--cluster_mode connected` (run_cluster(mode="connected")) reads the connected components off the same graph instead
(ms_cluster_components; DESIGN.md section 5.8, "Connected components"): the longest domain of a component represents it, and the
third column is each member's strongest own link.

`-m/--mintm` (run_cluster(mintm=...)) verifies every edge with TM-align before anything is clustered (DESIGN.md section 5.8,
"Structure-verified edges"): ms_cluster_pairs reads the distinct unordered pairs off the lists and extras on the device, the
batched aligner scores them, ms_cluster_pairs_apply takes the pairs below the cut out of the graph in both directions, and the
cluster call runs on what is left.  The greedy TSV gains a fourth column, the TM-score of (representative, member).

The clustering's definition is the header's (include/merizo_search_amd.h, ms_cluster_greedy): an edge needs a cosine at or
above --mincos in either direction and the shorter domain to cover --mincov of the longer; the longer domain is the
representative (cd-hit's greedy order), every other domain goes to its best-scoring adjacent representative.  Coverage is that
SYMMETRIC rule on the edge: the search itself runs without the one-sided query-length mask of `search`.
"""
from __future__ import annotations

import logging
import math
import os
from typing import Optional, Sequence

import numpy as np

from . import dbsearch as ds
from . import sharded
from .dbsearch import _BatchScan, _DeviceTimes, _refuse, _require_database, read_database
from .target import Target, score_mode

logger = logging.getLogger(__name__)


def write_cluster_tsv(path: str, names, rep: np.ndarray, rep_score: np.ndarray, header: bool, score_name: str = "emb_score",
                      tm_score: Optional[np.ndarray] = None) -> None:
    """Clusters by the representative's row; its own line first, then its members by row.  The cosine column is formatted as
    results.write_search_results formats emb_score; score_name: its name in the header line.  tm_score: a fourth column
    `tm_score` per row, formatted the same way (`cluster --mintm`, greedy mode)."""
    rows = np.arange(rep.shape[0], dtype=np.int64)
    order = np.lexsort((rows, rows != rep, rep))
    with open(path, "w") as handle:
        if header:
            handle.write("representative\tmember\t%s%s\n" % (score_name, "" if tm_score is None else "\ttm_score"))
        for r in order:
            tm = "" if tm_score is None else "\t" + "{:.4f}".format(tm_score[r])
            handle.write("%s\t%s\t%s%s\n" % (names[int(rep[r])], names[int(r)], "{:.4f}".format(rep_score[r]), tm))


def write_tree_tsv(path: str, names, a: np.ndarray, b: np.ndarray, weight: np.ndarray, header: bool) -> None:
    """The single-linkage tree, one line per forest edge: member_a, member_b (a the smaller row), link_score -- in the forest's own
    order, weight descending, then rows ascending.  The weight is printed with %.9g: a float32 round-trips, and other programs cut
    this file at thresholds of their own."""
    order = np.lexsort((b, a, -weight.astype(np.float64)))
    with open(path, "w") as handle:
        if header:
            handle.write("member_a\tmember_b\tlink_score\n")
        for e in order:
            handle.write("%s\t%s\t%.9g\n" % (names[int(a[e])], names[int(b[e])], float(weight[e])))


def _check_levels(levels, mincos: float):
    """`--levels` as given (strings as typed, or numbers) -> [(label, T)]: the label names the level's file.  Refused: a level that is
    no number, NaN, below mincos, or given twice."""
    checked = []
    for item in levels:
        label = item.strip() if isinstance(item, str) else str(item)
        try:
            value = float(item)
        except (TypeError, ValueError):
            _refuse("--levels: %r is not a number." % (item,))
        if math.isnan(value):
            _refuse("--levels: a level is NaN.")
        if value < float(mincos):
            _refuse("--levels: level %s lies below -s/--mincos %s: the neighbour graph holds no edge below --mincos, and the tree "
                    "cannot be cut there. Lower --mincos to the smallest level." % (label, mincos))
        if any(value == seen or label == name for name, seen in checked):
            _refuse("--levels: level %s is given twice." % label)
        checked.append((label, value))
    return checked


MAX_EDGES = 2 ** 27       # directed entries the edge pass of --complete may hold: a memory budget (20 B each: 2.7 GB), not a measurement


def _edge_pass(engine, target: Target, qdb, in_place: bool, full_rows: np.ndarray, mincos: float, query_batchsize: int,
               search_batchsize: int, edge_room: int, max_edges: int, times):
    """Every neighbour at or above mincos of the rows `full_rows` (global, ascending) among THIS rank's rows of the database ->
    (src, dst, score, found, rescored): directed entries src -> dst in global rows (device tensors of one length), the number
    found -- larger than that length only when it exceeds max_edges: the scan then goes on counting without keeping -- and the
    cells that went to the exact chain.  The queries are what the self-search used for those rows, in its mode; a query's own row
    is excluded.  The buffer starts at min(max_edges, edge_room) entries and grows geometrically; a call whose exact count
    exceeds the room left is repeated once after growing.  times: one 'edges' span per batch of query_batchsize full rows."""
    torch = engine.torch
    mode, _masked = score_mode(target.faiss, qdb.normalized)
    bound = target.row_norm_bound if target.faiss else None             # (None: unit rows, the engine's default)
    cap = max(1, min(int(max_edges), int(edge_room)))
    buf = [torch.empty((cap,), dtype=dt, device=engine.device) for dt in (torch.int64, torch.int64, torch.float32)]
    used = found = rescored = 0
    for f0 in range(0, full_rows.shape[0], int(query_batchsize)):
        t0 = times.mark()
        rows = engine.to_device(full_rows[f0:f0 + int(query_batchsize)])
        q = target.rows[rows] if in_place else engine.to_device(qdb.embeddings_of(full_rows[f0:f0 + int(query_batchsize)]))
        for block, a, _lengths in target.blocks(qdb, search_batchsize):
            stats = {}
            scan = lambda keep: engine.threshold_edges(block, q, mode, mincos, lo=rows, hi=rows + 1, row_offset=a, row_norm_bound=bound,
                                                       out=tuple(b[used:used + keep] for b in buf), stats=stats)
            if found > max_edges:                                       # over the budget already: count on, keep nothing
                found += scan(0)[3]
                rescored += stats["rescored"]
                continue
            src, _dst, _score, count = scan(cap - used)
            if used + count > max_edges:
                found = used + count
                rescored += stats["rescored"]
                continue
            if count > cap - used:
                cap = min(int(max_edges), max(2 * cap, used + count))
                grown = [torch.empty((cap,), dtype=b.dtype, device=engine.device) for b in buf]
                for g, b in zip(grown, buf):
                    g[:used] = b[:used]
                buf = grown
                src, _dst, _score, count = scan(cap - used)
            rescored += stats["rescored"]
            buf[0][used:used + count] = rows[src]                       # the query's number -> its global row
            used += count
            found = used
        times.add("edges", t0)
    return buf[0][:used], buf[1][:used], buf[2][:used], found, rescored


def _verify_edges(engine, qdb, graph, lengths: np.ndarray, mincos: float, mincov: float, mintm: float, fastmode: bool,
                  tm_batchsize: int):
    """The TM-align stage of `cluster --mintm` on graph = (nbr_idx, nbr_score, edge_src, edge_dst, edge_score), device tensors that
    are EDITED: the distinct canonical pairs (engine.cluster_pairs: chain 1 is the would-be representative) are aligned in batches of
    tm_batchsize, longest first -- each batch fetches the coordinates and sequences of its rows once (Records) and converts each
    row's coordinates once (tmalign.pdb_values) -- and a pair is kept when the aligner reports TM_OK and max(qtm, ttm), on the
    5-decimal values tmalign.printed_values returns (what `search --tmalign_backend hip` compares), is >= mintm.  A pair with a chain
    of <= 5 residues or a non-finite coordinate is not aligned and not kept.  engine.cluster_pairs_apply then takes the pairs that are
    not kept out of the lists and extras.  -> (workspace holding the set, tm float64 [pairs] by slot (max(qtm, ttm), -1.0 where not
    aligned), info: saturated (before the edit), tm_pairs, tm_rejected_pairs (not kept), tm_unaligned_pairs (of those: never aligned
    or refused by the aligner), tm_removed_entries (directed entries overwritten))."""
    from .._lib import TM_OK
    from . import tmalign
    torch = engine.torch
    pairs, counts, workspace = engine.cluster_pairs(*graph, lengths, mincos, mincov)
    count, saturated = (int(c) for c in counts.cpu().numpy())
    pairs = pairs[:count].cpu().numpy().astype(np.int64)
    tm = np.full(count, -1.0, dtype=np.float64)
    keep = np.zeros(count, dtype=np.uint8)
    unaligned = 0
    work = lengths[pairs[:, 0]].astype(np.int64) * lengths[pairs[:, 1]].astype(np.int64)
    order = np.argsort(-work, kind="stable")                              # longest first, as the aligner orders a launch
    for b0 in range(0, count, int(tm_batchsize)):
        slots = order[b0:b0 + int(tm_batchsize)]
        rows, local = np.unique(pairs[slots], return_inverse=True)
        local = local.reshape(-1, 2)
        coords, seqs = qdb.coords(rows), qdb.seqs(rows)
        missing = [int(r) for r, c in zip(rows, coords) if c is None]
        if missing:
            _refuse("cluster --mintm needs the coordinates of every row: database row %d has none." % missing[0])
        with np.errstate(over="ignore"):                                  # (the fp32 cast turns |v| > 3.4e38 into inf)
            good = np.array([len(c) > 5 and bool(np.isfinite(np.asarray(c, dtype=np.float32)).all()) for c in coords], dtype=bool)
        alignable = good[local[:, 0]] & good[local[:, 1]]
        unaligned += int((~alignable).sum())
        if not alignable.any():
            continue
        used = np.unique(local[alignable])                                # only the rows that are aligned are converted and uploaded
        place = np.full(len(rows), -1, dtype=np.int64)
        place[used] = np.arange(used.shape[0])
        got = engine.tmalign_batch([tmalign.pdb_values(coords[r]) for r in used], [seqs[r] for r in used], place[local[alignable]],
                                   fast=bool(fastmode))
        for p, slot in enumerate(slots[alignable]):
            if got["status"][p] != TM_OK:
                unaligned += 1
                continue
            v = tmalign.printed_values(got["qtm"][p], got["ttm"][p], got["rmsd"][p], got["n_ali8"][p], got["n_identical"][p])
            tm[slot] = max(v["qtm"], v["ttm"])
            keep[slot] = tm[slot] >= mintm
    if unaligned:
        logger.warning("cluster: %d of %d pairs have a chain of 5 residues or fewer or with a non-finite coordinate: TM-align cannot "
                       "score them, and they are treated as below --mintm." % (unaligned, count))
    removed = engine.cluster_pairs_apply(*graph, lengths, mincos, mincov, engine.to_device(keep), workspace)
    return workspace, tm, {"saturated": saturated, "tm_pairs": count, "tm_rejected_pairs": int(count - keep.sum()),
                           "tm_unaligned_pairs": unaligned, "tm_removed_entries": int(removed.cpu().numpy()[0])}


def _write_tree(engine, forest, levels, names, lengths: np.ndarray, mincov: float, output: str, header: bool, info: dict) -> None:
    """The files of `cluster --tree / --levels` from forest = engine.cluster_tree(...): `<output>_cluster_tree.tsv`, and per level
    (label, T) `<output>_cluster_<label>.tsv` -- the components of the forest's edges at T (engine.cluster_components with k = 0: the
    edges as extras, which stay on the device), written as the connected mode writes its own file.  info gains tree_edges,
    tree_rounds and levels."""
    torch = engine.torch
    pairs, weight, found = forest
    filled = pairs[:, 0] >= 0
    a, b, w = pairs[filled, 0].to(torch.int64).contiguous(), pairs[filled, 1].to(torch.int64).contiguous(), weight[filled].contiguous()
    info.update(tree_edges=int(found["n_edges"]), tree_rounds=int(found["rounds"]), levels={})
    tree_path = output + "_cluster_tree.tsv"
    write_tree_tsv(tree_path, names, a.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy(), header)
    logger.info("cluster: single-linkage tree of %d edges in %d rounds -> %s" % (info["tree_edges"], info["tree_rounds"], tree_path))
    for label, level in levels:
        rep, link, cut = engine.cluster_components(None, None, a, b, w, lengths, float(level), mincov)
        info["levels"][label] = int(cut["n_components"])
        path = "%s_cluster_%s.tsv" % (output, label)
        write_cluster_tsv(path, names, rep.cpu().numpy(), link.cpu().numpy(), header, "link_score")
        logger.info("cluster: level %s: %d components -> %s" % (label, info["levels"][label], path))


def run_cluster(db_name: str, output: str, tmp: str, device="cuda", topk: int = 20, mincos: Optional[float] = None,
                mincov: float = 0.7, query_batchsize: int = 4096, search_batchsize: int = 262144, header: bool = False,
                engine=None, timings: Optional[dict] = None, complete: bool = False, max_edges: int = MAX_EDGES,
                edge_room: int = 2 ** 20, mode: str = "greedy", mintm: Optional[float] = None, fastmode: bool = False,
                tm_batchsize: int = 65536, tree: bool = False, levels: Optional[Sequence] = None):
    """Cluster the rows of database `db_name` and write `<output>_cluster.tsv`.  topk: neighbours kept per row (the search
    fetches topk + 1 and drops the row itself); a row whose topk entries all count as edges may have neighbours the clustering
    never sees (`saturated`: raise -k).  Under several ranks every rank scans its shard of the rows; rank 0 alone keeps the
    graph, clusters and writes.  -> (rep int64 [n], rep_score float32 [n], info) as numpy arrays on rank 0, (None, None, info)
    elsewhere; info: n, n_reps, singletons, rounds, saturated, full_lists (rows whose list holds topk entries at or above
    mincos, whether or not they pass mincov: the lists that may have been cut short).  `timings`: as run_dbsearch_db's, plus the
    HIP-event span of ms_cluster_greedy ('cluster_ms').
    complete: cluster the TRUE threshold graph, whatever topk -- the rows with a full list get all their neighbours from an
    edge pass over this rank's rows (_edge_pass; gathered to rank 0 under several ranks) and ms_cluster_greedy_edges runs on the
    lists plus those entries: the TSV a run at topk = n - 1 would write.  At most max_edges directed entries are held (beyond
    that the run is refused and nothing is written); edge_room: the entries the buffer starts with.  info gains `complete`,
    `edges` and `rescored`, timings 'edges_ms' (the edge pass: one span per batch of full rows, as 'scan_ms' has one per batch).
    mode: 'greedy' (above) or 'connected': the connected components of the same graph (ms_cluster_components on the lists, plus the
    edge pass's entries under complete) -- rep[i] the longest row of i's component, rep_score[i] the row's strongest own link (the
    TSV's third column is then headed `link_score`); info holds `n_components` in place of `n_reps`, and `largest`, the rows of the
    largest component.  Without complete a list that -k cut short may split a component.  info gains `mode` in both.
    mintm: None (nothing changes), or the TM-score in (0, 1] an edge must reach: on rank 0, once the lists (and under complete the
    gathered extras) are on the device, _verify_edges aligns every distinct pair (fastmode: TM-align -fast; tm_batchsize: pairs per
    launch) and takes the pairs below mintm out of the graph before the cluster call, which is unchanged.  info['saturated'] is then
    the count BEFORE the edit, info gains tm_pairs, tm_rejected_pairs, tm_unaligned_pairs and tm_removed_entries, timings 'tm_ms';
    the greedy TSV gains a fourth column `tm_score`: max(qtm, ttm) of (representative, member), 1.0000 on a representative's line.
    The connected mode keeps its three columns (a member need not be adjacent to its representative).
    tree (connected mode only): after the unchanged steps ms_cluster_tree builds the single-linkage tree of the same graph -- its
    maximum spanning forest -- and `<output>_cluster_tree.tsv` holds it (write_tree_tsv).  levels (implies tree): thresholds at or
    above mincos, numbers or strings as typed; for each one ms_cluster_components runs on the forest's edges alone (k = 0, extras)
    and `<output>_cluster_<level>.tsv` is the file a separate run at that --mincos would write, without a second search.  info gains
    tree_edges (= n - n_components), tree_rounds and levels ({level: n_components}), timings 'tree_ms' (the ms_cluster_tree call)."""
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
    if mode not in ("greedy", "connected"):
        _refuse("cluster mode must be 'greedy' or 'connected', got %r." % (mode,))
    if int(max_edges) < 1 or int(edge_room) < 1:
        _refuse("--max_edges must be >= 1, got %r." % (max_edges,))
    if mintm is not None and not 0.0 < float(mintm) <= 1.0:               # (NaN fails both comparisons)
        _refuse("-m/--mintm must lie in (0, 1], got %r." % (mintm,))
    if mintm is not None and int(tm_batchsize) < 1:
        _refuse("--tm_batchsize must be >= 1, got %r." % (tm_batchsize,))
    tree = bool(tree) or levels is not None
    if tree and mode != "connected":
        _refuse("--tree and --levels read the single-linkage tree: they need --cluster_mode connected, got %r." % (mode,))
    levels = _check_levels(levels, float(mincos)) if levels is not None else []
    _require_database(db_name)
    target_db = read_database(db_name=db_name)                            # (host side only: nothing is uploaded yet)
    qdb = QueryDB(db_name, loaded=target_db if not target_db["faiss"] else None)
    n, k = int(qdb.n), int(topk)
    if k + 1 > n:
        _refuse("-k %d plus the row itself exceed the %d rows of the database." % (k, n))
    lengths = qdb.lengths()
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
    logger.info("cluster: %d rows of %s, %d neighbours per row at cosine >= %s, coverage >= %s, batches of %d%s%s"
                % (n, db_name, k, mincos, mincov, int(query_batchsize),
                   "; queries read in place from the resident rows" if scan.in_place else "",
                   "; complete: rows with a full list get all their neighbours from an edge pass" if complete else "")
                + ("; connected components" if mode == "connected" else ""))
    own = engine.to_device(np.arange(n + 1, dtype=np.int64))              # row q excludes [q, q + 1): slices of one array
    nbr_s = nbr_i = count = None
    if rank == 0:                                                         # the graph: rank 0's device, never the host
        nbr_s = torch.empty((n, k), dtype=torch.float32, device=engine.device)
        nbr_i = torch.empty((n, k), dtype=torch.int64, device=engine.device)
        count = torch.empty((n,), dtype=torch.int32, device=engine.device)
    counts = []                                                           # every rank gets each batch's counts back from the drop step
    for b0 in range(0, n, int(query_batchsize)):
        b1 = min(n, b0 + int(query_batchsize))
        seqs = None if target_db["faiss"] else qdb.seqs(b0, b1)
        out = (nbr_s[b0:b1], nbr_i[b0:b1], count[b0:b1]) if rank == 0 else None
        counts.append(scan.search(b0, b1, seqs, 0.0, own[b0:b1], own[b0 + 1:b1 + 1], k, float(mincos), out=out)[2])
    full_rows = np.nonzero(torch.cat(counts).cpu().numpy() == k)[0].astype(np.int64)      # the lists that k may have cut short
    info = {"n": n, "k": k, "full_lists": int(full_rows.shape[0]), "complete": bool(complete), "mode": mode}
    edges = None
    if complete:
        info.update(edges=0, rescored=0)
    if complete and full_rows.shape[0] > 0:
        src, dst, score, found, rescored = _edge_pass(engine, scan.target, qdb, scan.in_place, full_rows, float(mincos), query_batchsize,
                                                      search_batchsize, edge_room, int(max_edges), times)
        edges, info["edges"], info["rescored"] = sharded.gather_edges(src, dst, score, engine.device, total=found, rescored=rescored,
                                                                      limit=int(max_edges))
        if edges is None:                                                 # (every rank learns it from the same counts)
            times.finish()
            qdb.close()
            _refuse("cluster --complete: the %d rows with a full list have %d neighbours at cosine >= %s, more than --max_edges %d "
                    "directed entries. Raise -s/--mincos, or raise --max_edges (20 bytes of device memory per entry)."
                    % (info["full_lists"], info["edges"], mincos, int(max_edges)))
    if rank != 0:
        times.finish()
        qdb.close()
        return None, None, info
    e_src, e_dst, e_score = edges if edges is not None else (None, None, None)
    verified = None
    if mintm is not None:
        t0 = times.mark()
        verified = _verify_edges(engine, qdb, (nbr_i, nbr_s, e_src, e_dst, e_score), lengths, float(mincos), float(mincov), float(mintm),
                                 fastmode, tm_batchsize)
        times.add("tm", t0)
    t0 = times.mark()
    if mode == "connected":
        rep, rep_score, found = engine.cluster_components(nbr_i, nbr_s, e_src, e_dst, e_score, lengths, float(mincos), float(mincov))
    elif complete:
        rep, rep_score, found = engine.cluster_greedy_edges(nbr_i, nbr_s, e_src, e_dst, e_score, lengths, float(mincos), float(mincov))
    else:
        rep, rep_score, found = engine.cluster_greedy(nbr_i, nbr_s, lengths, float(mincos), float(mincov))
    times.add("cluster", t0)
    forest = None
    if tree:
        t0 = times.mark()
        forest = engine.cluster_tree(nbr_i, nbr_s, e_src, e_dst, e_score, lengths, float(mincos), float(mincov))
        times.add("tree", t0)
    times.finish()
    rep, rep_score = rep.cpu().numpy(), rep_score.cpu().numpy()
    sizes = np.bincount(rep, minlength=n)
    info.update(found, singletons=int((sizes == 1).sum()))
    tm_score = None
    if verified is not None:
        workspace, tm, tm_info = verified
        info.update(tm_info)                                              # ('saturated': the lists as the search left them)
        logger.info("cluster: TM-align on %d distinct pairs: %d below --mintm %s (%d of them not alignable), %d directed entries removed"
                    % (info["tm_pairs"], info["tm_rejected_pairs"], mintm, info["tm_unaligned_pairs"], info["tm_removed_entries"]))
        if mode == "greedy":                                              # (a member is adjacent to its representative: the pair has a slot)
            members = np.nonzero(rep != np.arange(n))[0]
            slots = engine.cluster_pairs_find(rep[members], members, lengths, workspace).cpu().numpy()
            tm_score = np.ones(n, dtype=np.float64)
            tm_score[members] = np.where(slots >= 0, tm[np.maximum(slots, 0)], -1.0) if tm.shape[0] else -1.0
    write_cluster_tsv(out_path, qdb.names(0, n), rep, rep_score, header, "link_score" if mode == "connected" else "emb_score", tm_score)
    if forest is not None:
        _write_tree(engine, forest, levels, qdb.names(0, n), lengths, float(mincov), output, header, info)
    qdb.close()
    if mode == "connected":
        info["largest"] = int(sizes.max())
        logger.info("cluster: %d components (%d singletons, the largest of %d rows) of %d rows in %d rounds -> %s"
                    % (info["n_components"], info["singletons"], info["largest"], n, info["rounds"], out_path))
        if complete:
            logger.info("cluster: complete: %d rows had a full list of %d; the edge pass added %d directed entries (%d cells re-scored "
                        "exactly): the components are those of the full threshold graph"
                        % (info["full_lists"], k, info["edges"], info["rescored"]))
        elif info["full_lists"] > 0:
            logger.warning("cluster: %d lists are full: -k %d may have cut them short, and a component whose only bridge was cut comes "
                           "out split in two. --complete gives the true components, whatever -k." % (info["full_lists"], k))
        return rep, rep_score, info
    logger.info("cluster: %d clusters (%d singletons) of %d rows in %d rounds -> %s"
                % (info["n_reps"], info["singletons"], n, info["rounds"], out_path))
    if complete:
        logger.info("cluster: complete: %d rows had a full list of %d; the edge pass added %d directed entries (%d cells re-scored "
                    "exactly): the clustering is that of the full threshold graph" % (info["full_lists"], k, info["edges"], info["rescored"]))
        return rep, rep_score, info
    if info["saturated"] > 0:
        logger.warning("cluster: %d rows have all %d kept neighbours above the thresholds: their lists may have been cut short "
                       "and neighbours beyond them are unknown to the clustering. Raise -k." % (info["saturated"], k))
    if info["full_lists"] > info["saturated"]:
        logger.warning("cluster: %d lists are full when the entries that fail --mincov are counted too: such a list may have been cut "
                       "short as well. --complete clusters the full threshold graph, whatever -k." % info["full_lists"])
    return rep, rep_score, info
