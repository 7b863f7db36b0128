"""`Records`: names, sequences, coordinates and metadata of a database's rows on the host, for either on-disk layout (dbutil.py;
DESIGN.md 2.1) -- the one reader of the drivers (`search`, `db-search`, `cluster`, `chain-search`, the multi-domain modes) -- and
the pure functions of names the multi-domain code is built on (`domid2chainid`, `equal_runs`, `chain_runs`).

Every accessor takes rows as `(lo, hi)` -- the range [lo, hi), read with one slice of the mapped file -- or as one int sequence
(any order, duplicates allowed, order preserved), and returns one list entry per row.
"""
from __future__ import annotations

import os
import pickle
import re
from typing import List, Sequence, Tuple

import numpy as np

from . import dbutil

_KEY = "_records"       # dbsearch.read_database's dict keeps its Records here (read by this module alone)

_TWO_DIGITS = re.compile(r"[0-9]{2}$")


def domid2chainid(domain_id: str) -> str:
    """'cath-dompdb/2pi4A04.pdb' -> '2pi4A'; 'x/AF-Q93009-F1-model_v4_TED02.pdb' -> 'AF-Q93009-F1-model_v4'.

    Same steps as the reference (dbsearch_fulllength.py:36-39), including its use of str.rstrip('.pdb'), which strips
    any trailing run of the characters '.', 'p', 'd', 'b' rather than the literal suffix."""
    stem = os.path.basename(domain_id).rstrip(".pdb")
    stem = _TWO_DIGITS.sub("", stem).rstrip("_")
    return stem[: -len("_TED")] if stem.endswith("_TED") else stem


def equal_runs(keys: Sequence) -> List[Tuple[int, int]]:
    """(first, one past the last) position of every run of adjacent equal keys, in order; a key that comes back after another
    one starts a new run."""
    runs, a = [], 0
    for b in range(1, len(keys) + 1):
        if b == len(keys) or keys[b] != keys[a]:
            runs.append((a, b))
            a = b
    return runs


def chain_runs(names: Sequence[str]) -> np.ndarray:
    """int64 [nchains + 1]: the first row of every run of adjacent names with one domid2chainid (its rstrip('.pdb') quirk
    included), closed by len(names) -- the target chains of mode `database_cosine`, where a chain IS a run of rows.  Two runs
    with one chain id that are not adjacent are two chains here (`exhaustive_cosine` would merge them by name; the reference
    assumes adjacency, :363-394).  A plain loop: about a microsecond-scale call of domid2chainid per name."""
    starts = [a for a, _b in equal_runs([domid2chainid(name) for name in names])]
    return np.asarray(starts + [len(names)], dtype=np.int64)


def _rows(lo, hi):
    """An accessor's arguments -> slice(lo, hi), or with hi None the int64 array of the row sequence `lo`."""
    return slice(int(lo), int(hi)) if hi is not None else np.asarray(lo, dtype=np.int64).reshape(-1)


class Records:
    """faiss: the layout; n: the number of rows; index: the unpickled `<db>.index` of the `.pt` layout (None: faiss layout)."""

    def __init__(self, db_name: str, index=None):
        """index: the unpickled `<db>.index` of a `.pt` database when the caller holds it already."""
        if os.path.exists(db_name + ".pt"):
            if index is None:
                with open(db_name + ".index", "rb") as handle:
                    index = pickle.load(handle)
            self._open_pt(index, *dbutil.pt_metadata_files(db_name))
        else:
            self._open_faiss(db_name + ".json")

    @classmethod
    def of(cls, target_dict: dict) -> "Records":
        """The Records of dbsearch.read_database's dict, opened on the first call and kept in the dict: the `.pt` layout shares
        the dict's unpickled index and opens its metadata pair, the faiss layout opens the files the json names."""
        records = target_dict.get(_KEY)
        if records is None:
            records = cls.__new__(cls)
            if target_dict["faiss"]:
                records._open_faiss(target_dict["database"])
            else:
                records._open_pt(target_dict["index"], target_dict["mifn"], target_dict["mdfn"])
            target_dict[_KEY] = records
        return records

    def _open_pt(self, index, mifn, mdfn) -> None:
        self.faiss, self.index, self.n = False, index, len(index)
        self._meta = dbutil.Blob(mifn, mdfn) if mifn is not None and mdfn is not None else None
        self._chain_starts = None

    def _open_faiss(self, json_path: str) -> None:
        info = dbutil.read_dbinfo(json_path)
        path = lambda key: os.path.join(os.path.dirname(json_path), info[key])
        self.faiss, self.index = True, None
        self._names = dbutil.map_file(path("db_names_f"))
        self.n = len(self._names) // dbutil.NAME_RECORD
        self._seq, self._coords = dbutil.Blob(path("sif"), path("sdf")), dbutil.Blob(path("cif"), path("cdf"))
        self._meta = dbutil.Blob(path("mif"), path("mdf")) if "mif" in info and "mdf" in info else None
        self._chain_starts = None

    def close(self) -> None:
        """(may be called twice)"""
        for part in ("_names", "_seq", "_coords", "_meta"):
            if getattr(self, part, None) is not None:
                getattr(self, part).close()

    # -- rows, as (lo, hi) or as one int sequence -----------------------------------------
    def _entries(self, rows, field: int) -> list:
        """Field 0 (path), 1 (coords) or 2 (seq) of the `.pt` index entries of `rows`."""
        entries = self.index[rows] if isinstance(rows, slice) else [self.index[r] for r in rows]
        return [entry[field] for entry in entries]

    def stored_names(self, lo, hi=None) -> List[str]:
        """Names as stored (the `.pt` index keeps paths): what domid2chainid is applied to."""
        rows = _rows(lo, hi)
        if not self.faiss:
            return self._entries(rows, 0)
        records = np.frombuffer(self._names, dtype="S%d" % dbutil.NAME_RECORD, count=self.n)[rows]
        return [r.decode().rstrip() for r in records]        # (32 characters + '\n': a name of full width has no padding)

    def names(self, lo, hi=None) -> List[str]:
        """Names as reported: the stored name (faiss layout), the `.pt` path's basename without '.pdb'."""
        stored = self.stored_names(lo, hi)
        return stored if self.faiss else [os.path.basename(path).replace(".pdb", "") for path in stored]

    def seqs(self, lo, hi=None) -> List[str]:
        rows = _rows(lo, hi)
        return self._seq.fetch(rows, dbutil.ascii_conv) if self.faiss else self._entries(rows, 2)

    def coords(self, lo, hi=None) -> List[np.ndarray]:
        rows = _rows(lo, hi)
        return self._coords.fetch(rows, dbutil.coord_conv) if self.faiss else self._entries(rows, 1)

    def metadata(self, lo, hi=None) -> List[str]:
        """The metadata json of each row; "{ }" per row when the database has none."""
        rows = _rows(lo, hi)
        if self._meta is not None:
            return self._meta.fetch(rows, dbutil.ascii_conv)
        return ["{ }"] * (max(0, rows.stop - rows.start) if isinstance(rows, slice) else len(rows))

    # -- one row (the multi-domain code) ----------------------------------------------------
    def name(self, row: int) -> str:
        return self.stored_names([row])[0]

    def entry_name(self, row: int) -> str:
        """The domain name entry() reports for a database row."""
        return self.names([row])[0]

    def name_meta(self, row: int):
        """(domain name, metadata json) of a database row, as entry() gives them -- without its coordinates and sequence."""
        return self.entry_name(row), self.metadata([row])[0]

    def entry(self, row: int):
        """(domain name, coords [N,3], sequence, row, metadata json) of a database row (dbsearch_fulllength.py:426-466)."""
        return (self.entry_name(row), self.coords([row])[0], self.seqs([row])[0], row, self.metadata([row])[0])

    # -- the whole database -----------------------------------------------------------------
    def lengths(self) -> np.ndarray:
        """Domain lengths int32 [n]: the faiss layout's sequence offsets (end - start of `sif`, one view of the mapped file), the
        `.pt` index's sequences."""
        if self.faiss:
            offsets = self._seq.offsets(slice(0, self.n))
            return (offsets[:, 1] - offsets[:, 0]).astype(np.int32)
        return np.asarray([len(entry[2]) for entry in self.index], dtype=np.int32)

    def chain_starts(self) -> np.ndarray:
        """chain_runs of all rows, computed once per open database."""
        if self._chain_starts is None:
            self._chain_starts = chain_runs(self.stored_names(0, self.n))
        return self._chain_starts
