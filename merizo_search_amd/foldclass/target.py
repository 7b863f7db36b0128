"""`Target`: this rank's rows of a target database on the engine's device, or streamed when they do not fit.
dbsearch.read_database's dict keeps the reference's keys (host-side values, never overwritten) plus two private keys, each read by
one module alone: here the Target of one (database, engine, shard); in dbrecords.py the host-side Records of the same rows."""
from __future__ import annotations

import logging

import numpy as np

from . import multidomain, sharded
from .dbutil import db_iterator, open_faiss_matrix

logger = logging.getLogger(__name__)

_KEY = "_target"


def score_mode(faiss: bool, prenormalised_queries: bool):
    """(md_chain_scores / md_chain_scan mode, does mincov apply?): the faiss layout scores inner products of its unit rows with
    queries taken as given ('ip_prenorm') or normalised by the kernel ('ip'), unmasked; `.pt` scores cosines masked by mincov."""
    if faiss:
        return ("ip_prenorm" if prenormalised_queries else "ip"), False
    return "cosine", True


class Target:
    """faiss: the layout; n: rows of the whole database; [lo, hi): this rank's rows (sharded.shard_bounds); rows: those rows on
    the device (`.pt`: L2-normalised once, engine.cosine_rows) or None when they are streamed from `matrix`, the mapped file
    of the faiss layout; lengths: the `.pt` layout's domain lengths of [lo, hi) on the device; row_norm_bound / pf_image: what
    the prefiltered search takes of resident rows (None on an engine without one: the CPU oracle engine of the tests)."""

    def __init__(self, engine, faiss: bool, n: int, matrix=None):
        self.engine, self.faiss, self.n, self.matrix = engine, bool(faiss), int(n), matrix
        self.shard = rank, world = sharded.rank_world()         # (what [lo, hi) depends on besides n)
        self.lo, self.hi = sharded.shard_bounds(self.n, world, rank)
        self.rows = self.lengths = self.row_norm_bound = self.pf_image = None

    @property
    def streamed(self) -> bool:
        return self.rows is None

    @property
    def whole(self) -> bool:
        """Does this process hold ALL rows resident (one rank, not streamed)?"""
        return self.shard[1] == 1 and self.rows is not None

    # -- construction ------------------------------------------------------------------
    @classmethod
    def cached(cls, target_dict, engine):
        """The resident Target kept in target_dict, if it is on this engine and spans this rank's rows; else None."""
        t = target_dict.get(_KEY) if target_dict is not None else None
        return t if t is not None and t.engine is engine and t.shard == sharded.rank_world() else None

    @classmethod
    def of(cls, target_dict: dict, engine=None, nq: int = 1, k: int = 1) -> "Target":
        """The Target of read_database's dict on `engine` (None: the engine it is resident on already), made on the first call
        and kept in the dict while it is resident: the `.pt` rows always (normalised once per engine), the faiss shard unless
        its bytes exceed engine.resident_budget(nq, k) -- such a Target is streamed and NOT kept: the next call asks again."""
        engine = engine or target_dict[_KEY].engine
        t = cls.cached(target_dict, engine)
        if t is not None:
            return t
        target_dict.pop(_KEY, None)
        prefilter = hasattr(engine, "lazy_pf_image")        # (the CPU oracle engine of the tests has no prefiltered search)
        if target_dict["faiss"]:
            info, matrix = open_faiss_matrix(target_dict["database"])
            t = cls(engine, True, info["DB_SIZE"], matrix)
            if (t.hi - t.lo) * matrix.shape[1] * 4 > engine.resident_budget(int(nq), int(k)):
                logger.info("database shard of %d rows exceeds the resident budget: it is streamed in blocks" % (t.hi - t.lo))
                return t
            t.rows = engine.upload_rows(matrix, t.lo, t.hi)
            if prefilter:                                   # (the row-norm bound: measured once, when the shard becomes resident)
                t.row_norm_bound = engine.row_norm_bound(t.rows)
                t.pf_image = engine.lazy_pf_image(t.rows, t.row_norm_bound)
        else:
            raw = target_dict["database"]                   # (memory-mapped: a rank reads only the pages of ITS rows)
            t = cls(engine, False, raw.shape[0])
            t.rows = engine.cosine_rows(engine.to_device(raw[t.lo:t.hi].float().contiguous()))
            t.lengths = engine.to_device(target_dict["lengths"][t.lo:t.hi])
            if prefilter:                                   # (the image: built by the first batch of more than 64 queries)
                t.pf_image = engine.lazy_pf_image(t.rows, engine.UNIT_ROW_BOUND)
        target_dict[_KEY] = t
        return t

    @classmethod
    def for_reader(cls, target_dict, engine, reader) -> "Target":
        """The resident Target an earlier search left in target_dict (None: no dict) when it is this engine's and spans this
        rank's rows of `reader` (a dbquery.QueryDB of the database); else a streamed one over the reader's files.  No upload."""
        t = cls.cached(target_dict, engine)
        if t is not None and t.n == reader.n:
            return t
        return cls(engine, reader.faiss, reader.n, reader.matrix if reader.faiss else None)

    # -- the rows, three ways ----------------------------------------------------------
    def topk(self, q, k: int, *, qlen=None, mincov: float = 0.0, raw_queries: bool = False, search_batchsize: int = 262144,
             log=logger):
        """The global top-k of queries q [nq,128] (on the device) over the database -> (scores [nq,k], rows [nq,k]) on the device, after the
        exchange + merge under several ranks.  `.pt`: cosine with the length mask (qlen on the device, mincov).  faiss layout:
        exact inner products, the queries normalised by the scan (raw_queries) or taken as given; a resident shard is ONE
        launch, a streamed one goes block by block through dbsearch.knn_exact with raw queries normalised once, out of place."""
        from .dbsearch import knn_exact
        engine = self.engine
        if not self.faiss:
            extra = {"pf_image": self.pf_image} if self.pf_image is not None else {}
            scores, idx = engine.cosine_topk(self.rows, q, int(k), lengths=self.lengths, qlen=qlen, mincov=float(mincov),
                                             row_offset=self.lo, **extra)
        elif self.rows is not None:
            scores, idx = knn_exact(q, [self.rows], int(k), engine, log=log, row_offset=self.lo, to_host=False, raw_queries=raw_queries,
                                    row_norm_bound=self.row_norm_bound, pf_image=self.pf_image)
        else:
            qn = engine.normalized(q, 1e-12) if raw_queries else q
            scores, idx = knn_exact(qn, db_iterator(self.matrix[self.lo:self.hi], int(search_batchsize)), int(k), engine, log=log,
                                    row_offset=self.lo, to_host=False)
        return sharded.exchange_and_merge(scores, idx, engine)          # all-gather + merge; no-op on one rank

    def rows_for(self, global_rows, reader):
        """Sorted unique global rows -> (matrix on the device, lengths or None, local index of each row): the resident rows in
        place when this process holds them all, else read from the files (multidomain.compact_target_rows)."""
        if not self.whole:
            return multidomain.compact_target_rows(self.engine, reader, global_rows)
        return self.rows, self.lengths, global_rows - self.lo

    def blocks(self, reader, search_batchsize: int):
        """This rank's rows once, in order: (rows on the device, first global row, lengths or None) -- one block when resident,
        else blocks of search_batchsize rows read through `reader` (faiss: engine.device_blocks, the copy of the next block
        under the consumer's work on this one; `.pt`: normalised as the resident copy is)."""
        engine, step = self.engine, max(1, int(search_batchsize))
        if self.hi <= self.lo:
            return
        if self.rows is not None:
            yield self.rows, self.lo, self.lengths
        elif self.faiss:
            a = self.lo
            for block in engine.device_blocks(db_iterator(self.matrix[self.lo:self.hi], step)):
                yield block, a, None
                a += int(block.shape[0])
        else:
            for a in range(self.lo, self.hi, step):
                b = min(self.hi, a + step)
                lengths = np.asarray([len(s) for s in reader.seqs(a, b)], dtype=np.float32)
                yield engine.cosine_rows(engine.to_device(reader.embeddings(a, b))), a, engine.to_device(lengths)
