"""Search drivers: the host-side mirror of programs/Foldclass/dbsearch.py on the HIP engine.

Same function names, argument meaning, return shapes and on-disk layouts as the reference:

    network_setup            (network.py)        dbsearch.py:35-45
    read_database                                 dbsearch.py:48-72
    search_query_against_db                       dbsearch.py:75-81
    knn_exact                                     dbsearch.py:213-248 (knn_exact_faiss)
    dbsearch                                      dbsearch.py:84-200   `.pt` database, one query
    dbsearch_faiss                                dbsearch.py:203-472  faiss-layout database
    hit_records                                   dbsearch.py:119-200 and :312-472  top-k lists -> hit records, both layouts
    run_dbsearch                                  dbsearch.py:475-551
    run_dbsearch_db                               (no counterpart: a database as the query side, `db-search`)

Every driver turns its top-k lists into hit records with hit_records: one selection, one fetch per field from the database's
one host-side reader (dbrecords.Records, which maps each record file once per run), one TM-align batch or one call of the
binary per hit, one loop; what the two layouts do differently there is a rule that names `faiss`.

What differs, deliberately (DESIGN.md "host drivers"):
  * all queries of a call are embedded in ONE ragged GPU launch and searched in ONE batched
    scan, instead of the reference's per-query Python loop; results are the same lists;
  * database row norms are computed once per database (the reference re-normalises the whole
    database for every query);
  * a faiss-layout database that fits in HBM is uploaded ONCE as one contiguous tensor and scanned
    with one launch per query batch; only a database larger than the resident budget is streamed
    in `search_batchsize` blocks (pinned, double-buffered: engine.device_blocks);
  * with an initialised torch.distributed process group (cli under torchrun) every rank holds and
    scans only its `sharded.shard_bounds` rows, one all-gather + merge gives every rank the global
    top-k, and rank 0 alone assembles hit records (sharded.py; replaces index_cpu_to_all_gpus,
    dbsearch.py:228-230);
  * TM-align is optional (tmalign.py): with no binary the search is embedding-only; with tmalign_backend='hip' every
    (query, hit) pair of a call that passes mincos is aligned on the GPU in ONE batch (ms_tmalign.hip), then the
    reference's per-hit logic runs unchanged on those results;
  * reference defects are not reproduced: a single --pdb_chain with several inputs is applied
    to every input (dbsearch.py:523-524 builds a list of lists; :296 raises IndexError); a
    faiss-layout search with zero hits returns empty lists instead of crashing (:390); the
    returned lists always have one entry per query.
"""
from __future__ import annotations

import logging
import os
import pickle
import sys
from typing import List, Optional

import numpy as np

from . import sharded
from . import tmalign as tm
from .dbquery import QueryDB, parse_row_slice, same_database
from .dbrecords import Records
from .dbutil import load_pt_matrix, pt_metadata_files
from .network import network_setup
from .pdbio import read_pdb, write_pdb
from .target import Target, score_mode

logger = logging.getLogger(__name__)


# ------------------------------------------------------------------ database open ------
def read_database(db_name: str, device=None, engine=None) -> dict:
    """Open a database by prefix: `<db>.pt` first, else `<db>.json` (dbsearch.py:50,65).

    pt layout -> {'database': [N,128] on the host (RAW, memory-mapped), 'index': list of (path, coords, seq), 'lengths':
    float32 [N], 'faiss': False, 'mdfn', 'mifn'}; with an engine this rank's rows are made resident on its device at once,
    L2-normalised (engine.cosine_rows: the row half of cosine_similarity, done once) -- in the dict's Target (target.py), which
    the searches ask for the rows.  faiss layout -> {'database': json path, 'faiss': True}; the matrix is opened by Target.of.
    The host-side rows of either dict -- names, sequences, coordinates, metadata -- are read through Records.of (dbrecords.py).
    """
    if os.path.exists(db_name + ".pt"):
        import torch

        raw = load_pt_matrix(db_name + ".pt")       # (memory-mapped: Target.of slices this rank's rows first)
        with open(db_name + ".index", "rb") as handle:
            target_index = pickle.load(handle)
        assert len(target_index) == raw.size(0)
        lengths = np.asarray([len(entry[2]) for entry in target_index], dtype=np.float32)
        mifn, mdfn = pt_metadata_files(db_name)
        out = {"database": raw, "index": target_index, "lengths": torch.from_numpy(lengths),
               "faiss": False, "mdfn": mdfn, "mifn": mifn}
        if engine is not None:
            Target.of(out, engine)
        return out
    if os.path.exists(db_name + ".json"):
        return {"database": db_name + ".json", "faiss": True}
    logger.error("%s is not a valid db or the path basename is incorrect; neither %s.pt nor %s.json were found."
                 % (db_name, db_name, db_name))
    sys.exit(1)


# ------------------------------------------------------------------ numeric kernels ----
def search_query_against_db(query_dict, target_dict, mincov, topk, score_corrections=None, engine=None):
    """cosine_similarity(db, q) * (len(q_seq) >= lengths * mincov) -> top-k (dbsearch.py:75-81).

    query_dict['embedding'] may hold one query [1,128] (the reference's shape) or a batch
    [nq,128] with query_dict['seq'] a list of sequences; returns {'scores', 'indices'} of shape
    [k] or [nq,k] accordingly.  k > Ndb raises, as torch.topk does.
    """
    target = Target.of(target_dict, engine)
    engine = target.engine
    seqs = query_dict["seq"]
    single = isinstance(seqs, str)
    qlen = np.asarray([len(seqs)] if single else [len(s) for s in seqs], dtype=np.float32)
    if topk > target.n:
        raise RuntimeError("selected index k out of range")
    scores, idx = target.topk(engine.to_device(query_dict["embedding"]).reshape(-1, 128), int(topk), qlen=engine.to_device(qlen),
                              mincov=mincov)
    if single:
        return {"scores": scores[0], "indices": idx[0]}
    return {"scores": scores, "indices": idx}


def knn_exact(xq, db_blocks, k: int, engine, log=logger, row_offset: int = 0, to_host: bool = True, raw_queries: bool = False,
              row_norm_bound=None, pf_image=None):
    """Exact max-inner-product kNN over a database delivered block by block (knn_exact_faiss,
    dbsearch.py:213-248): per block IndexFlat.add/search -> `I += i0` -> ResultHeap merge.

    xq: [nq,d], already normalised -- or raw with raw_queries=True: F.normalize(xq) (eps 1e-12, :303-304) is then applied
    inside every block's search call (bit-identical to normalising first); db_blocks: iterable of float32 [b,d] blocks -- host arrays
    (memmap slices: streamed through engine.device_blocks, the copy of block b+1 overlapping the
    scan of block b) or device tensors (scanned in place; a resident database is ONE such block).
    Rows are numbered from `row_offset`.  Returns (D float32 [nq,k], I int64 [nq,k]), best first,
    as numpy arrays (device tensors with to_host=False); missing entries are (-inf, -1) like faiss.
    """
    import time

    t0 = time.time()
    q = engine.to_device(xq)
    nq = q.shape[0]
    log.info("knn_exact queries size %s k=%d" % (tuple(q.shape), k))
    blocks = list(db_blocks) if isinstance(db_blocks, (list, tuple)) else db_blocks
    on_host = not (isinstance(blocks, list) and all(isinstance(b, engine.torch.Tensor) and b.device == q.device for b in blocks))
    best_s = best_i = None
    i0 = int(row_offset)
    for block in (engine.device_blocks(b for b in blocks if b.shape[0] > 0) if on_host else blocks):
        ni = block.shape[0]
        if ni == 0:
            continue
        # (a resident shard comes with its row-norm bound and, memory permitting, its fp16 image (built on first use): large batches -- and, from 1M rows, any batch -- then take the
        #  prefiltered search -- same results)
        s, i = (engine.ip_topk(block, q, k, row_offset=i0, normalize_queries=raw_queries, row_norm_bound=row_norm_bound, pf_image=pf_image)
                if row_norm_bound is not None else engine.ip_topk(block, q, k, row_offset=i0, normalize_queries=raw_queries))
        if best_s is None:
            best_s, best_i = s, i
        else:
            best_s, best_i = engine.topk_merge(_stack(best_s, s), _stack(best_i, i))
        i0 += ni
        log.info("%d DB elements, %.3f s" % (i0 - int(row_offset), time.time() - t0))
    if best_s is None:
        best_s = engine.to_device(np.full((nq, k), -np.inf, np.float32))
        best_i = engine.to_device(np.full((nq, k), -1, np.int64))
    if not to_host:
        return best_s, best_i
    D, I = best_s.cpu().numpy(), best_i.cpu().numpy()
    log.info("kNN time: %.3f s (%d vectors)" % (time.time() - t0, i0 - int(row_offset)))
    return D, I


def _stack(a, b):
    import torch
    return torch.stack([a, b])


# ------------------------------------------------------------------ helpers ------------
def _query_name(query_dict) -> str:
    return os.path.basename(query_dict["name"]).replace(".pdb", "")


def _hit(query_dict, target_name, score, t_len, tm_output, dbindex, metadata) -> dict:
    """The per-hit record consumed by write_search_results (keys: dbsearch.py:126-138)."""
    return {
        "query": _query_name(query_dict),
        "target": os.path.basename(target_name).replace(".pdb", ""),
        "score": score,
        "q_len": len(query_dict["seq"]),
        "t_len": t_len,
        "tmalign_output": tm_output,
        "dom_str": query_dict.get("dom_str"),
        "dom_conf": query_dict.get("dom_conf"),
        "dom_plddt": query_dict.get("dom_plddt"),
        "dbindex": dbindex,
        "metadata": metadata,
    }


def _load_queries(inputs, inputs_are_ca: bool, pdb_chains: List[str]) -> List[dict]:
    if inputs_are_ca:
        return list(inputs)                       # dicts {coords, seq, name, ...} (merizo.py:367-383)
    return [read_pdb(pdbfile=path, pdb_chain=chain) for path, chain in zip(inputs, pdb_chains)]


def _chain_list(pdb_chain: Optional[str], n_inputs: int) -> List[str]:
    """Chain ids per input: comma separated list, one id broadcast to all inputs, default 'A'."""
    if not pdb_chain:
        return ["A"] * n_inputs
    chains = pdb_chain.rstrip(",").split(",")
    if len(chains) == n_inputs:
        return chains
    if len(chains) == 1:
        return chains * n_inputs
    logger.error("Number of specified chain IDs not equal to number of input PDB files.")
    sys.exit(1)


def _aligner_device(engine, device):
    return getattr(engine, "device", None) or device or "cuda"


def _refused(query_dict, target_name) -> None:
    logger.warning("TM-align refuses %s x %s (a structure of <= 5 residues): hit dropped"
                   % (_query_name(query_dict), os.path.basename(str(target_name))))


def _tmalign_pair(tmp, query_dict, target_coords, target_seq, fastmode, target_name=None, named=False):
    if named:
        qfn = write_pdb(tmp, query_dict["coords"], query_dict["seq"], name=os.path.basename(query_dict["name"]))
        tfn = write_pdb(tmp, target_coords, target_seq, name=target_name)
    else:
        qfn = write_pdb(tmp, query_dict["coords"], query_dict["seq"])
        tfn = write_pdb(tmp, target_coords, target_seq)
    return tm.run_tmalign(qfn, tfn, options="-fast" if fastmode else None, keep_pdbs=False)


# ------------------------------------------------------------------ top-k lists -> hit records
def hit_records(query_dicts, D, I, records: Records, faiss: bool, *, mincos, mintm, mincov, fastmode, skip_tmalign, tmalign_backend,
                tmp, aligner_device, tm_excluded_before: int = 0):
    """The top-k lists of a call's queries -> (results, all_results), one dict of hit records per query, twice: the hits at or
    above mintm and those below it (dbsearch.py:119-200 and :312-472).  D float32 / I int64 [nq,k]: scores and global rows, best
    first, (-inf, -1) behind the real entries.  A hit is an entry with D >= mincos and I >= 0; names, sequences, coordinates and
    metadata of ALL hits of the call come from `records` (the target database's reader) in one fetch per field, with
    tmalign_backend 'hip' they are aligned in ONE GPU batch, else one call of the binary per hit.
    faiss: the layout of the target database, which decides the keys (`.pt`: the hit's rank = its column in D, in both dicts;
    faiss: a dense counter per query, and for hits below mintm ONE counter over all queries of a search, dbsearch.py:449-452),
    the coverage rule (`.pt` only, :165), the names of the binary's temporary files and the three log lines of the faiss path.
    tm_excluded_before: a search made in several calls (run_dbsearch_db's query batches) passes how many hits below mintm the
    earlier calls counted."""
    nq = len(query_dicts)
    results = [dict() for _ in range(nq)]
    all_results = [dict() for _ in range(nq)]
    keep = np.where((D >= mincos) & (I >= 0))                  # row-major: grouped by query, rank order
    rows, scores, queries, ranks = I[keep], D[keep], keep[0], keep[1]
    n_hits = len(rows)
    if n_hits == 0:
        return results, all_results
    if faiss:
        logger.info("Retrieve domain hits...")
    # (each hit reports its OWN metadata, also one that follows a rank below mincos; "{ }" only in a database without any)
    names, seqs, metadata = records.stored_names(rows), records.seqs(rows), records.metadata(rows)
    hip_outputs = None
    if not skip_tmalign:
        if faiss:
            logger.info("TM-align top hits...")
        coords = records.coords(rows)
        if tmalign_backend == "hip":                           # every (query, hit) pair of the call in one GPU batch
            hip_outputs = tm.align_many([(query_dicts[q]["coords"], query_dicts[q]["seq"], c, s) for q, c, s in zip(queries, coords, seqs)],
                                        fast=fastmode, device=aligner_device)
    counts = [0] * nq
    n_tm_exclude = int(tm_excluded_before)
    for h, (qi, row, rank) in enumerate(zip(queries.tolist(), rows.tolist(), ranks.tolist())):      # (plain ints)
        qd, t_len = query_dicts[qi], len(seqs[h])
        key = counts[qi] if faiss else rank
        tm_output = None
        if not skip_tmalign:
            if hip_outputs is None:
                tm_output = _tmalign_pair(tmp, qd, coords[h], seqs[h], fastmode, target_name=names[h], named=faiss)
            else:
                tm_output = hip_outputs[h]
                if tm_output is None:
                    _refused(qd, names[h])
                    continue
            if not faiss and not (tm_output["len_ali"] >= t_len * mincov):        # coverage filter, `.pt` path only (:165)
                continue
        rec = _hit(qd, names[h], scores[h], t_len, tm_output, row, metadata[h])
        if skip_tmalign or max(tm_output["qtm"], tm_output["ttm"]) >= mintm:
            results[qi][key] = rec
            counts[qi] += 1
        else:
            all_results[qi][n_tm_exclude if faiss else key] = rec
            n_tm_exclude += 1
    if faiss and n_tm_exclude > tm_excluded_before:
        logger.info("Excluded " + str(n_tm_exclude - int(tm_excluded_before)) + " hits (across all query domains) by TM-score threshold(>=" + str(mintm) + ")")
    return results, all_results


# ------------------------------------------------------------------ `.pt` driver -------
def dbsearch(query, target_dict: dict, tmp: str, network, topk: int, mincov: float, mincos: float, mintm: float,
             fastmode: bool, device=None, inputs_are_ca: bool = False, pdb_chain: str = "A", skip_tmalign: bool = False,
             score_corrections=None, tmalign_backend: str = "auto"):
    """One query against a `.pt` database -> (results, all_results), dicts keyed by the hit's position in the top-k
    (dbsearch.py:84-200): embed, scan, hit_records on the one list."""
    query_dict = query if inputs_are_ca else read_pdb(pdbfile=query, pdb_chain=pdb_chain)
    query_dict["embedding"] = network.embed_many([query_dict["coords"]]).reshape(1, -1)
    top = search_query_against_db(query_dict, target_dict, mincov, topk, score_corrections, engine=network.engine)
    results, all_results = hit_records([query_dict], top["scores"].cpu().numpy()[None], top["indices"].cpu().numpy()[None],
                                       Records.of(target_dict), False, mincos=mincos, mintm=mintm, mincov=mincov, fastmode=fastmode,
                                       skip_tmalign=skip_tmalign, tmalign_backend=tmalign_backend, tmp=tmp,
                                       aligner_device=_aligner_device(network.engine, device))
    return results[0], all_results[0]


# ------------------------------------------------------------------ faiss-layout driver -
def dbsearch_faiss(queries, target_dict: dict, tmp: str, network, topk: int, mincov: float, mincos: float,
                   mintm: float, fastmode: bool, device=None, inputs_are_ca: bool = False,
                   search_batchsize: int = 262144, search_type: str = "IP", pdb_chain: str = "A",
                   skip_tmalign: bool = False, score_corrections=None, tmalign_backend: str = "auto"):
    """All queries against a faiss-layout database -> (results, all_results): one dict per query,
    keyed by a dense counter of retained hits (dbsearch.py:203-472).  No mincov length mask on this
    path (acknowledged TODO at dbsearch.py:307-310)."""
    if len(queries) == 0:
        logger.error("No inputs were provided!")
        sys.exit(1)
    if not os.path.exists(tmp):
        os.mkdir(tmp)
    if search_type != "IP":
        logging.error("Invalid/unsupported faiss search type: " + search_type + "\n\tOnly 'IP' is currently supported.")
        sys.exit(1)
    engine = network.engine
    nq = len(queries)
    logger.info("DB iterator using batchsize of " + str(search_batchsize))

    query_dicts = _load_queries(queries, inputs_are_ca, _chain_list(pdb_chain, nq))
    emb = sharded.embed_distributed(network, [qd["coords"] for qd in query_dicts])   # ragged launches, data-parallel over ranks

    # this rank's rows of the matrix, resident (F.normalize, :303-304, + knn_exact_faiss, :213-248, as ONE launch for the few
    # queries of a CLI search; more than 64 queries: the prefiltered search) or streamed block by block; then the exchange
    Ds, Is = Target.of(target_dict, engine, nq, int(topk)).topk(emb, int(topk), raw_queries=True, search_batchsize=search_batchsize)
    if sharded.rank_world()[0] != 0:
        return [dict() for _ in range(nq)], [dict() for _ in range(nq)]   # rank 0 assembles the hit records
    return hit_records(query_dicts, Ds.cpu().numpy(), Is.cpu().numpy(), Records.of(target_dict), True, mincos=mincos, mintm=mintm,
                       mincov=mincov, fastmode=fastmode, skip_tmalign=skip_tmalign, tmalign_backend=tmalign_backend, tmp=tmp,
                       aligner_device=_aligner_device(network.engine, device))


# ------------------------------------------------------------------ dispatcher ---------
def run_dbsearch(inputs, db_name: str, tmp: str, device, topk: int, fastmode: bool, threads: int, mincos: float,
                 mintm: float, mincov: float, inputs_are_ca: bool = False, search_batchsize: int = 262144,
                 search_type: str = "IP", pdb_chain: Optional[str] = None, skip_tmalign: bool = False,
                 network=None, weights_path: Optional[str] = None, tmalign_backend: str = "auto", target_db: Optional[dict] = None):
    """Set up the encoder, open the database, search every input (dbsearch.py:475-551).
    target_db: the database opened already (read_database's dict, with the engine of `network`); None = opened here.  A caller
    that goes on with the same dict (the multi-domain mode `database_cosine`) finds the rows this search made resident in it.
    Returns (search_results, all_search_results): one dict rank -> hit per input, twice.
    tmalign_backend: 'auto' = the TM-align binary if one is found, else an embedding-only search; 'hip' = the GPU
    aligner (needs a cuda device).  skip_tmalign wins over both."""
    tm.check_backend(tmalign_backend, device)
    if len(inputs) == 0:
        logger.error("No inputs were provided!")
        sys.exit(1)
    if not os.path.exists(tmp):
        os.mkdir(tmp)
    if network is None:
        network, device = network_setup(threads=threads, device=device, weights_path=weights_path)
    skip_tmalign = tm.skip_without_binary(skip_tmalign, tmalign_backend)
    if target_db is None:
        target_db = read_database(db_name=db_name, device=device, engine=network.engine)

    if target_db["faiss"]:
        if search_batchsize < 1:
            logger.error("search_batchsize must be >= 1.")
            sys.exit(1)
        return dbsearch_faiss(queries=inputs, target_dict=target_db, tmp=tmp, network=network, topk=topk,
                              mincov=mincov, mincos=mincos, mintm=mintm, fastmode=fastmode, device=device,
                              inputs_are_ca=inputs_are_ca, search_batchsize=search_batchsize, search_type=search_type,
                              pdb_chain=pdb_chain, skip_tmalign=skip_tmalign, tmalign_backend=tmalign_backend)

    query_dicts = _load_queries(inputs, inputs_are_ca, _chain_list(pdb_chain, len(inputs)))
    emb = sharded.embed_distributed(network, [qd["coords"] for qd in query_dicts])   # ragged launches, data-parallel over ranks
    batch = {"seq": [qd["seq"] for qd in query_dicts], "embedding": emb}
    top = search_query_against_db(batch, target_db, mincov, topk, engine=network.engine)   # one batched scan (+ exchange)
    if sharded.rank_world()[0] != 0:
        return [dict() for _ in query_dicts], [dict() for _ in query_dicts]      # rank 0 assembles the hit records
    return hit_records(query_dicts, top["scores"].cpu().numpy(), top["indices"].cpu().numpy(), Records.of(target_db), False,
                       mincos=mincos, mintm=mintm, mincov=mincov, fastmode=fastmode, skip_tmalign=skip_tmalign,
                       tmalign_backend=tmalign_backend, tmp=tmp, aligner_device=_aligner_device(network.engine, device))


# ------------------------------------------------------------------ database x database -
def engine_setup(device):
    """The engine of a db-search.  No encoder and no weights: its queries are stored embeddings."""
    from .engine import HipEngine, resolve_device
    return HipEngine(resolve_device(device))


def _refuse(message: str) -> None:
    logger.error(message)
    sys.exit(1)


class _DeviceTimes:
    """HIP-event spans of the scan calls and the drop kernel of a db-search (tools/dbsearch_bench.py); off unless asked for."""

    def __init__(self, engine, sink):
        self.sink = sink
        self.torch = engine.torch if sink is not None and getattr(engine.device, "type", "cpu") == "cuda" else None
        self.spans = {}

    def mark(self):
        if self.torch is None:
            return None
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def add(self, name, start, end=None):
        if self.torch is not None:
            self.spans.setdefault(name, []).append((start, end or self.mark()))

    def finish(self):
        if self.torch is None:
            return
        self.torch.cuda.synchronize()
        for name, spans in self.spans.items():
            self.sink[name + "_ms"] = float(sum(a.elapsed_time(b) for a, b in spans))
            self.sink[name + "_first_ms"] = float(spans[0][0].elapsed_time(spans[0][1]))
            self.sink[name + "_calls"] = len(spans)


class _BatchScan:
    """The per-batch half of a search of query batches taken from a database (run_dbsearch_db, cluster.run_cluster) against a
    Target: per batch of query rows [b0, b1) the scan at k' with its exchange + merge (Target.topk) and the drop step down to
    kout entries at or above min_score, between timing marks."""

    def __init__(self, target: Target, qdb, same: bool, kk: int, search_batchsize: int, times):
        self.target, self.qdb, self.kk, self.search_batchsize, self.times = target, qdb, int(kk), int(search_batchsize), times
        # the same faiss-layout database on one rank: the resident rows ARE the queries (normalised, 16-byte aligned at 512 B per
        # row), read in place by the scan.  (`.pt`: the resident rows were normalised in place, the raw queries come from the file.)
        self.in_place = bool(same and qdb.faiss and target.whole)
        self.streamed = target.streamed

    def search(self, b0: int, b1: int, seqs, mincov: float, d_lo, d_hi, kout: int, min_score: float, out=None):
        """Query rows [b0, b1) of the query database -> (scores [nq,kout], rows [nq,kout], count [nq]) on the device, the rows
        [d_lo[q], d_hi[q]) of each query excluded; seqs: the queries' sequences (the `.pt` layout's length mask; unused in the
        faiss layout).  out: the preallocated triple the drop step writes into."""
        target, qdb, times = self.target, self.qdb, self.times
        engine = target.engine
        q = target.rows[b0:b1] if self.in_place else engine.to_device(qdb.embeddings(b0, b1))
        t0 = times.mark()
        qlen = None if target.faiss else engine.to_device(np.asarray([len(s) for s in seqs], dtype=np.float32))
        Ds, Is = target.topk(q, self.kk, qlen=qlen, mincov=mincov, raw_queries=not qdb.normalized,
                             search_batchsize=self.search_batchsize, log=_QUIET)
        t1 = times.mark()
        times.add("scan", t0, t1)
        kw = {} if out is None else {"out": out}
        dropped = engine.topk_drop_ranges(Ds, Is, d_lo, d_hi, int(kout), float(min_score), **kw)
        times.add("drop", t1)
        return dropped


class _ChainStep:
    """The multi-domain step of a db-search (multidomain.cosine_step, mode `exhaustive_cosine`): the query chains are the runs of
    adjacent query rows with one chain id inside [q_lo, q_hi); a batch's step covers the chains that END in it, the reported
    results of a chain's earlier rows are carried over on the host.  Target rows: the resident matrix when this process
    holds all rows (one rank, not streamed), else the needed chain runs read from the database files (rank 0)."""

    def __init__(self, qdb, q_lo: int, q_hi: int, target: Target, db_name: str, same: bool, exclude_self: bool,
                 mincos: float, mincov: float, max_mapping_paths: int, times, timings, report: str = "all"):
        from . import multidomain as md
        self.md, self.qdb, self.q_lo, self.engine, self.target = md, qdb, q_lo, target.engine, target
        self.mincos, self.max_paths, self.times = float(mincos), int(max_mapping_paths), times
        self.exclude_self, self.report = exclude_self, report
        chains = [md.domid2chainid(n) for n in qdb.stored_names(q_lo, q_hi)]
        self.chains = chains
        self.run_end = np.empty(q_hi - q_lo, np.int64)          # one past the last row (global) of each query row's run
        for a, b in md.equal_runs(chains):
            self.run_end[a:b] = q_lo + b
        self.reader = qdb if same else QueryDB(db_name)
        self.owns_reader = not same
        self.score_mode, masked = score_mode(target.faiss, qdb.normalized)
        self.mincov = float(mincov) if masked else 0.0
        if timings is not None:
            timings["md_resident"] = target.whole
            timings["md_candidates_skipped"] = 0
        self.timings = timings
        self.pending = []                                      # (global row, query name, its reported results) of the open chain
        self.skipped = []

    def close(self) -> None:
        if self.owns_reader:
            self.reader.close()

    def batch(self, b0: int, b1: int, query_dicts, results) -> list:
        """The result tuples of the chains that end in query rows [b0, b1), in query-chain order."""
        rows = self.pending + [(b0 + r, _query_name(qd), res) for r, (qd, res) in enumerate(zip(query_dicts, results))]
        ended = [e for e in rows if self.run_end[e[0] - self.q_lo] <= b1]
        self.pending = rows[len(ended):]
        out, group, seen = [], [], set()
        for e in ended:                                         # one step per batch -- split only where a chain id comes back
            qc = self.chains[e[0] - self.q_lo]
            if qc in seen and self.chains[group[-1][0] - self.q_lo] != qc:
                out.extend(self._step(group))
                group, seen = [], set()
            group.append(e)
            seen.add(qc)
        if group:
            out.extend(self._step(group))
        return out

    def _step(self, group) -> list:
        md, engine = self.md, self.engine
        r0, r1 = group[0][0], group[-1][0] + 1
        chains = self.chains[r0 - self.q_lo: r1 - self.q_lo]
        hits = md.group_hits([e[1] for e in group], chains, [e[2] for e in group])
        if all(len(domains) < 2 for domains in hits.values()):
            for qc in hits:
                logger.debug("Query chain %s: only one detected domain, multi-domain hits equal the per-domain hits." % qc)
            return []
        q_first, own = {}, {}
        for i, qc in enumerate(chains):
            if qc not in q_first:
                q_first[qc] = i
                if self.exclude_self:
                    first, last = self.qdb.exclusion_ranges(r0 + i, r0 + i + 1, True)
                    own[qc] = (int(first[0]), int(last[0]))
        q_emb = engine.to_device(self.qdb.embeddings(r0, r1))
        qlen = None
        if self.score_mode == "cosine":
            qlen = engine.to_device(np.asarray([len(s) for s in self.qdb.seqs(r0, r1)], dtype=np.float32))
        skipped = []
        target_rows = lambda rows: self.target.rows_for(rows, self.reader)
        res = md.cosine_step(hits, q_first, q_emb, self.score_mode, engine, self.reader, target_rows, self.mincos,
                             qlen=qlen, mincov=self.mincov, own_rows=own or None,
                             max_mapping_paths=self.max_paths, log=logger.debug, skipped=skipped, times=self.times,
                             report=self.report)
        self.skipped.extend(skipped)
        if self.timings is not None:
            self.timings["md_candidates_skipped"] = len(self.skipped)
        return res


def _require_database(prefix: str) -> None:
    """Refuse a prefix that names no database of either layout (the `.pt` layout needs its `.index` too)."""
    if not (os.path.exists(prefix + ".json") or (os.path.exists(prefix + ".pt") and os.path.exists(prefix + ".index"))):
        _refuse("%s is not a valid db or the path basename is incorrect; neither %s.pt nor %s.json were found."
                % (prefix, prefix, prefix))


def open_query_and_target(query_db: str, db_name: str, query_rows: Optional[str], needs_same: Optional[str] = None):
    """The two sides of a search of database `query_db` against database `db_name` (run_dbsearch_db, chainsearch.run_chain_search)
    -> (target_db: read_database's dict, host side only -- nothing is uploaded yet; qdb: the query side's QueryDB; same: do both
    prefixes name one database; q_lo, q_hi: the query rows of query_rows = 'LO:HI', all rows for None).
    needs_same: an option that only a search of a database against itself can serve was given -- the refusal's opening words."""
    same = same_database(query_db, db_name)
    if needs_same and not same:
        _refuse("%s the query database and the target database to be the same, got %s and %s." % (needs_same, query_db, db_name))
    for prefix in (query_db, db_name):
        _require_database(prefix)
    target_db = read_database(db_name=db_name)
    # (a `.pt` database searched against itself: ONE unpickled index and one mapped tensor serve both sides)
    qdb = QueryDB(query_db, loaded=target_db if same and not target_db["faiss"] else None)
    try:
        q_lo, q_hi = parse_row_slice(query_rows, qdb.n)
    except ValueError as exc:
        _refuse("--query_rows: %s" % exc)
    return target_db, qdb, same, q_lo, q_hi


def run_dbsearch_db(query_db: str, db_name: str, output: str, tmp: str, device="cuda", topk: int = 1, fastmode: bool = False,
                    mincos: float = 0.5, mintm: float = 0.5, mincov: float = 0.7, search_batchsize: int = 262144,
                    search_type: str = "IP", skip_tmalign: bool = False, tmalign_backend: str = "auto",
                    query_batchsize: int = 4096, query_rows: Optional[str] = None, exclude_self: bool = False,
                    exclude_same_chain: bool = False, format_list=None, header: bool = False, metadata_json: bool = False,
                    report_insignificant_hits: bool = False, engine=None, timings: Optional[dict] = None,
                    multi_domain_search: bool = False, multi_domain_mode: str = "exhaustive_cosine",
                    max_mapping_paths: Optional[int] = None, multi_domain_report: str = "all") -> int:
    """Search the rows of database `query_db` (all, or the slice query_rows = 'LO:HI') against database `db_name` and write
    `<output>_search.tsv` (+ `_search_insignificant.tsv`), in query-row order: `search` with a database in the place of the
    PDB files.  No structure is parsed or embedded -- the stored embeddings are the queries (dbquery.QueryDB), so the
    search runs in the batches the kernels were built for: per `query_batchsize` queries ONE scan (resident target; the
    streamed knn_exact over engine.device_blocks beyond the HBM budget), one exchange + merge under several ranks, one
    ms_topk_drop_ranges, one record retrieval, one TM-align batch ('hip'), one append to the output.

    exclude_self / exclude_same_chain (query and target the SAME database): the query's own row / every row of its chain
    is taken out of its list EXACTLY: the scan fetches k' = k + the longest excluded run and the drop kernel removes
    them (include/merizo_search_amd.h).  mincos is the kernel's min_score: only surviving hits are retrieved.
    multi_domain_search: also write `<output>_search_multi_dom.tsv`, the multi-domain search in mode `exhaustive_cosine` (the only
    one here; multidomain.cosine_step): the query chains are the runs of adjacent query rows with one chain id, the hits that
    seed the candidates are each batch's reported results, and with exclude_self a query chain is never its own candidate
    (_ChainStep).  max_mapping_paths: multidomain.MAX_MAPPING_PATHS unless given.  multi_domain_report: 'all' = every mapping of a
    pair, 'best' = the best one(s) per pair with their score (multidomain.best_lines; no path cap).
    Everything else -- thresholds, hit records, columns -- is the code of `search` (hit_records).  Returns the number of
    queries searched.  `timings`: a dict that receives which path ran ('in_place': the queries were row ranges of the resident
    matrix; 'streamed': the target went through engine.device_blocks) and HIP-event totals of the scan calls and the drop step."""
    import time

    from .results import SEARCH_FIELDS, append_written, embedding_only_format, multi_dom_writer, write_search_results

    t_start = time.perf_counter()
    if engine is None:
        from .engine import resolve_device
        device = resolve_device(device)                                   # ('cpu' is refused here, before anything else)
    if tmalign_backend not in tm.BACKENDS:
        _refuse("tmalign_backend must be one of %s, got %r" % (", ".join(tm.BACKENDS), tmalign_backend))
    if topk < 1 or query_batchsize < 1 or search_batchsize < 1:
        _refuse("-k, --query_batchsize and --search_batchsize must be >= 1.")
    if multi_domain_search and multi_domain_mode != "exhaustive_cosine":
        _refuse("db-search --multi_domain_mode: only 'exhaustive_cosine' is available here, got %r." % (multi_domain_mode,))
    if multi_domain_report not in ("all", "best"):
        _refuse("--multi_domain_report must be 'all' or 'best', got %r." % (multi_domain_report,))
    write_multi_dom = multi_dom_writer(multi_domain_report)
    exclude_self = exclude_self or exclude_same_chain
    target_db, qdb, same, q_lo, q_hi = open_query_and_target(
        query_db, db_name, query_rows,
        "--exclude_self / --exclude_same_chain remove the query's own rows from its hits: they need" if exclude_self else None)
    if target_db["faiss"] and search_type != "IP":
        _refuse("Invalid/unsupported faiss search type: " + search_type + "\n\tOnly 'IP' is currently supported.")
    records = qdb if same else Records.of(target_db)                      # the target's rows on the host: one reader for the run
    n_target = records.n
    ex_lo = ex_hi = np.zeros(q_hi - q_lo, np.int64)                       # lo >= hi: nothing excluded
    if exclude_self:
        ex_lo, ex_hi = qdb.exclusion_ranges(q_lo, q_hi, exclude_same_chain)
    max_excluded = int((ex_hi - ex_lo).max())
    kk = int(topk) + max_excluded
    if kk > n_target and (exclude_self or not target_db["faiss"]):
        _refuse("-k %d plus the %d rows excluded for a query exceed the %d rows of the target database."
                % (topk, max_excluded, n_target))

    rank, world = sharded.rank_world()
    skip_tmalign = tm.skip_without_binary(skip_tmalign, tmalign_backend)
    fields = embedding_only_format(list(format_list) if format_list is not None else SEARCH_FIELDS.split(","), skip_tmalign)
    if not os.path.exists(tmp):
        os.makedirs(tmp, exist_ok=True)
    search_output, all_output = output + "_search.tsv", output + "_search_insignificant.tsv"
    written = (search_output, all_output) if report_insignificant_hits else (search_output,)      # the files this run writes
    multi_output = output + "_search_multi_dom.tsv"
    if rank == 0:
        for out_path in written + ((multi_output,) if multi_domain_search else ()):
            if os.path.exists(out_path):
                logger.warning(f"Search output file '{out_path}' already exists. Results will be overwritten!")
            open(out_path, "w").close()

    engine = engine or engine_setup(device)
    times = _DeviceTimes(engine, timings)
    target = Target.of(target_db, engine, min(int(query_batchsize), q_hi - q_lo), kk)      # resident once, or streamed per batch
    scan = _BatchScan(target, qdb, same, kk, search_batchsize, times)
    logger.info("db-search: %d queries of %s against %d rows of %s in batches of %d (k = %d%s)%s"
                % (q_hi - q_lo, query_db, n_target, db_name, int(query_batchsize), int(topk),
                   ", %d fetched: up to %d rows excluded per query" % (kk, max_excluded) if exclude_self else "",
                   "; queries read in place from the resident rows" if scan.in_place else ""))
    if timings is not None:
        timings["in_place"], timings["streamed"] = scan.in_place, scan.streamed
    d_lo, d_hi = engine.to_device(ex_lo), engine.to_device(ex_hi)        # once for the run: a batch's ranges are a slice
    chain_step = None
    if multi_domain_search and rank == 0:
        from .multidomain import MAX_MAPPING_PATHS
        chain_step = _ChainStep(qdb, q_lo, q_hi, target, db_name, same, exclude_self, mincos, mincov,
                                MAX_MAPPING_PATHS if max_mapping_paths is None else max_mapping_paths, times, timings,
                                report=multi_domain_report)
    md_all = {}
    tm_excluded = 0                                                       # (hits below mintm so far: the faiss layout keys them by it)
    t_loop = time.perf_counter()
    for b0 in range(q_lo, q_hi, int(query_batchsize)):
        b1 = min(q_hi, b0 + int(query_batchsize))
        query_dicts = seqs = None
        if rank == 0:
            query_dicts = qdb.records(b0, b1, with_coords=not skip_tmalign)
            seqs = [qd["seq"] for qd in query_dicts]
        elif not target_db["faiss"]:
            seqs = qdb.seqs(b0, b1)                                       # (every rank masks by query length)
        Ds, Is, _counts = scan.search(b0, b1, seqs, mincov, d_lo[b0 - q_lo: b1 - q_lo], d_hi[b0 - q_lo: b1 - q_lo], int(topk), float(mincos))
        if rank != 0:
            continue
        # (the drop step pads a list with (-inf, -1) behind its entries: hit_records needs no count)
        results, all_results = hit_records(query_dicts, Ds.cpu().numpy(), Is.cpu().numpy(), records, target_db["faiss"], mincos=mincos,
                                           mintm=mintm, mincov=mincov, fastmode=fastmode, skip_tmalign=skip_tmalign,
                                           tmalign_backend=tmalign_backend, tmp=tmp, aligner_device=_aligner_device(engine, device),
                                           tm_excluded_before=tm_excluded)
        tm_excluded += sum(len(per_query) for per_query in all_results)
        part = os.path.join(tmp, "db_search_batch.tsv")
        first = header and b0 == q_lo
        for out_path, per_batch in zip(written, (results, all_results)):
            append_written(out_path, part, lambda f: write_search_results(results=per_batch, output_file=f, format_list=fields, header=first))
        if chain_step is not None:
            lines = chain_step.batch(b0, b1, query_dicts, results)
            append_written(multi_output, part, lambda f: write_multi_dom(lines, f, first))
        if metadata_json:
            for out_path, per_batch in zip(written, (results, all_results)):
                md_all.setdefault(out_path, []).extend(hit["metadata"] for per_query in per_batch for hit in per_query.values()
                                                       if hit["metadata"] != "{ }")
        logger.info("db-search: queries %d..%d done" % (b0, b1 - 1))
    times.finish()
    if timings is not None:
        timings["setup_s"], timings["loop_s"] = t_loop - t_start, time.perf_counter() - t_loop
    if chain_step is not None:
        chain_step.close()
    qdb.close()
    if rank == 0 and metadata_json:                                       # (results.write_search_results' file, for the whole run)
        import ast
        import json
        for out_path in written:
            with open(out_path + ".hit_metadata.json", "w") as handle:
                json.dump([ast.literal_eval(m) for m in md_all.get(out_path, [])], handle)
            logger.info("Metadata for hits written to " + out_path + ".hit_metadata.json")
    return q_hi - q_lo


class _Quiet:
    """knn_exact's per-call log lines are per query batch here: kept at debug level."""

    @staticmethod
    def info(*args, **kw):
        logger.debug(*args, **kw)


_QUIET = _Quiet()
