"""A Foldclass database as the QUERY side of a search (`db-search`, dbsearch.run_dbsearch_db).

The reference searches PDB files only ("a few query domains per call", dbsearch.py:531-546): a user who holds embeddings in
a database -- createdb output of a proteome, a TED shard -- has to re-parse and re-embed the structures to search with them.
`QueryDB` is the database's `dbrecords.Records` (names, sequences, coordinates, metadata of its rows, either on-disk layout) plus
what a search needs of its queries besides:

    embeddings(lo, hi)    float32 [hi-lo,128] as STORED: raw in the `.pt` layout (the searches normalise queries themselves:
                          MS_MODE_COSINE_UNIT, MS_MODE_IP_NORMQ -- results bit-identical to `search` on the same structure),
                          F.normalize'd in the faiss layout (searched as they are, MS_MODE_IP_PRENORM: a second normalisation
                          would change bits)
    records(lo, hi)       the query dicts of the drivers: name (as reported: Records.names), seq, coords (only when an
                          aligner will read them)
    exclusion_ranges(..)  per query row the database rows a self-search must not report: the row itself, or the contiguous
                          run of rows of its chain (dbrecords.domid2chainid; rows of one chain are adjacent, as
                          multidomain.sibling_rows relies on)
"""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np

from . import dbutil
from .dbrecords import Records, domid2chainid, equal_runs


def same_database(prefix_a: str, prefix_b: str) -> bool:
    """Do two database prefixes name the same files?"""
    return os.path.realpath(prefix_a) == os.path.realpath(prefix_b)


def parse_row_slice(text, n: int) -> Tuple[int, int]:
    """'LO:HI' (either side may be empty) -> (lo, hi) with 0 <= lo < hi <= n; None: all rows.  ValueError otherwise."""
    if text is None:
        lo, hi = 0, n
    else:
        parts = str(text).split(":")
        if len(parts) != 2:
            raise ValueError("expected LO:HI, got %r" % (text,))
        try:
            lo = int(parts[0]) if parts[0].strip() else 0
            hi = int(parts[1]) if parts[1].strip() else n
        except ValueError:
            raise ValueError("expected LO:HI with integer row numbers, got %r" % (text,))
    if lo < 0 or hi > n:
        raise ValueError("rows %d:%d lie outside the query database (%d rows)" % (lo, hi, n))
    if lo >= hi:
        raise ValueError("rows %d:%d select no query (the query database has %d rows)" % (lo, hi, n))
    return lo, hi


class QueryDB(Records):
    """A database's Records plus its stored embeddings (`matrix`), for either layout."""

    def __init__(self, db_name: str, loaded=None):
        """loaded: dbsearch.read_database's dict of this same `.pt` database -- its unpickled index and its mapped tensor are
        used instead of reading both a second time (a database searched against itself)."""
        shared = loaded is not None and not loaded.get("faiss")
        super().__init__(db_name, index=loaded["index"] if shared else None)
        self.prefix = db_name
        if self.faiss:
            info, self.matrix = dbutil.open_faiss_matrix(db_name + ".json")
            if int(info["DB_SIZE"]) != self.n:
                raise ValueError("%s.json: DB_SIZE %d, but the names file holds %d records" % (db_name, int(info["DB_SIZE"]), self.n))
        else:       # the raw rows on the host (the engine gets its own, normalised copy)
            self.matrix = loaded["database"] if shared else dbutil.load_pt_matrix(db_name + ".pt")
            if self.matrix.size(0) != self.n:
                raise ValueError("%s.pt holds %d rows, its index %d entries" % (db_name, self.matrix.size(0), self.n))

    @property
    def normalized(self) -> bool:
        """Are the stored rows L2-normalised already (the faiss layout)?"""
        return self.faiss

    def embeddings(self, lo: int, hi: int) -> np.ndarray:
        if self.faiss:
            return np.ascontiguousarray(self.matrix[lo:hi], dtype=np.float32)
        return np.ascontiguousarray(self.matrix[lo:hi].float().numpy())

    def embeddings_of(self, rows) -> np.ndarray:
        """embeddings() of the given rows (an int64 array, any order) instead of a range."""
        rows = np.asarray(rows, dtype=np.int64)
        if self.faiss:
            return np.ascontiguousarray(self.matrix[rows], dtype=np.float32)
        import torch
        return np.ascontiguousarray(self.matrix[torch.from_numpy(rows)].float().numpy())

    def records(self, lo: int, hi: int, with_coords: bool = True) -> List[dict]:
        """Query dicts {name, seq, coords} of rows [lo, hi), in row order (coords None unless asked for)."""
        coords = self.coords(lo, hi) if with_coords else [None] * (hi - lo)
        return [{"name": n, "seq": s, "coords": c} for n, s, c in zip(self.names(lo, hi), self.seqs(lo, hi), coords)]

    def exclusion_ranges(self, lo: int, hi: int, same_chain: bool) -> Tuple[np.ndarray, np.ndarray]:
        """(first, past-last) database row a self-search excludes for every query row of [lo, hi): the row itself, or with
        same_chain the whole run of adjacent rows whose chain id equals the query's (it may reach beyond [lo, hi))."""
        rows = np.arange(lo, hi, dtype=np.int64)
        if not same_chain:
            return rows, rows + 1
        chains = [domid2chainid(n) for n in self.stored_names(lo, hi)]
        first, last = np.empty(hi - lo, np.int64), np.empty(hi - lo, np.int64)
        for a, b in equal_runs(chains):
            first[a:b], last[a:b] = lo + a, lo + b
        r = lo - 1                                  # the first and the last run may continue outside the slice
        while r >= 0 and domid2chainid(self.name(r)) == chains[0]:
            r -= 1
        first[first == first[0]] = r + 1
        r = hi
        while r < self.n and domid2chainid(self.name(r)) == chains[-1]:
            r += 1
        last[last == last[-1]] = r
        return first, last

