"""TM-align verification of hits (mirror of programs/Foldclass/utils.py:75-158).

Two backends:
  * `auto` (the default): the third-party CPU binary the reference shells out to for every hit, when one is
    available ($MERIZO_TMALIGN, or `tmalign` / `TMalign` on PATH, or next to this file) -- called exactly like the
    reference; otherwise searches run embedding-only (skip_tmalign) and say so;
  * `hip`: the batched GPU aligner (csrc/ms_tmalign.hip through ops.tmalign_batch): every pair of a call in one launch,
    from the coordinates in memory, no files or processes.  `align_many` returns the dicts `extract_tmalign_values`
    returns for the binary's output, its values rounded as the binary prints them.
"""
from __future__ import annotations

import logging
import os
import re
import shutil
import subprocess
from typing import List, Optional, Sequence, Tuple

import numpy as np

logger = logging.getLogger(__name__)

_ALIGNED = re.compile(r"Aligned length=\s*(\d+),\s+RMSD=\s*([0-9.]+),\s+Seq_ID=n_identical/n_aligned=\s*([0-9.]+)")
_TMSCORE = re.compile(r"TM-score=\s*([0-9.]+)")


def find_tmalign() -> Optional[str]:
    cands = [os.environ.get("MERIZO_TMALIGN"), os.path.join(os.path.dirname(os.path.realpath(__file__)), "tmalign"),
             shutil.which("tmalign"), shutil.which("TMalign")]
    for c in cands:
        if c and os.path.isfile(c) and os.access(c, os.X_OK):
            return c
    return None


def extract_tmalign_values(tmalign_output: str, return_alignment: bool = False) -> dict:
    """Parse TM-align's stdout -> {len_ali, rmsd, seq_id, qtm, ttm[, alignment]}.
    Two `TM-score=` lines are expected (normalised by query, then by target)."""
    m = _ALIGNED.search(tmalign_output)
    scores = [float(x) for x in _TMSCORE.findall(tmalign_output)]
    result = {
        "len_ali": int(m.group(1)) if m else None,
        "rmsd": float(m.group(2)) if m else None,
        "seq_id": float(m.group(3)) if m else None,
        "qtm": scores[0],
        "ttm": scores[1],
    }
    if return_alignment:
        start = tmalign_output.find('(":" denotes residue pairs')
        result["alignment"] = tmalign_output[start:].split("\n")[1:4]
    return result


def run_tmalign(structure1_path: str, structure2_path: str, options: Optional[str] = None, keep_pdbs: bool = False,
                binary: Optional[str] = None):
    """Run TM-align on two CA-only PDB files; returns the parsed dict ("" on failure, like the
    reference).  Input files are removed unless keep_pdbs."""
    binary = binary or find_tmalign()
    if binary is None:
        raise FileNotFoundError("no TM-align binary found (set $MERIZO_TMALIGN)")
    cmd = [binary, structure1_path, structure2_path] + ([options] if options else [])
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if proc.returncode != 0:
        logger.error(f"Error running tmalign: {proc.stderr}")
        return ""
    if not keep_pdbs:
        for path in (structure1_path, structure2_path):
            try:
                os.remove(path)
            except OSError as exc:
                logger.error(f"Error deleting structure files: {exc}")
    return extract_tmalign_values(proc.stdout)


BACKENDS = ("auto", "hip")


def check_backend(backend: str, device=None) -> None:
    """`hip` needs a HIP device ('cuda' / 'cuda:N'); unknown names are refused."""
    if backend not in BACKENDS:
        raise ValueError("tmalign_backend must be one of %s, got %r" % (", ".join(BACKENDS), backend))
    if backend == "hip" and device is not None and not str(device).startswith("cuda"):
        raise ValueError("tmalign_backend 'hip' runs TM-align on the GPU: it needs a cuda device, got %r" % (device,))


def skip_without_binary(skip_tmalign: bool, backend: str) -> bool:
    """The skip_tmalign a search runs with: backend 'auto' with no TM-align binary makes it embedding-only, and says so."""
    if not skip_tmalign and backend == "auto" and find_tmalign() is None:
        logger.warning("no TM-align binary found (set $MERIZO_TMALIGN): running an embedding-only search; "
                       "TM-align columns are unavailable")
        return True
    return skip_tmalign


def pdb_values(coords) -> np.ndarray:
    """The fp64 coordinates TM-align parses from the %8.3f PDB text the binary path writes: float("%.3f" % v)."""
    c = np.asarray(coords, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    return np.asarray([float("%.3f" % v) for v in c.reshape(-1)], dtype=np.float64).reshape(-1, 3)


def printed_values(qtm: float, ttm: float, rmsd: float, n_ali8: int, n_identical: int) -> dict:
    """The dict extract_tmalign_values makes of the binary's output: TM-score %.5f, RMSD %.2f, Seq_ID %.3f."""
    seq_id = n_identical / n_ali8 if n_ali8 > 0 else 0.0
    return {"len_ali": int(n_ali8), "rmsd": float("%.2f" % rmsd), "seq_id": float("%.3f" % seq_id),
            "qtm": float("%.5f" % qtm), "ttm": float("%.5f" % ttm)}


def align_many(items: Sequence[Tuple], fast: bool = False, device="cuda") -> List[Optional[dict]]:
    """TM-align every (coords1, seq1, coords2, seq2) of `items` on the GPU in one launch; chain 1 is the query.
    Returns one extract_tmalign_values-shaped dict per item, or None where TM-align refuses the input (a chain of
    <= 5 residues) and where a chain has a NaN or infinite coordinate.  Structures that occur in several items (a query,
    a target domain) are uploaded once."""
    if not items:
        return []
    finite = {}

    def is_finite(coords):
        key = id(coords)
        if key not in finite:
            with np.errstate(over="ignore"):                  # pdb_values' fp32 cast turns |v| > 3.4e38 into inf
                finite[key] = bool(np.isfinite(np.asarray(coords, dtype=np.float32)).all())
        return finite[key]

    keep = [p for p, (c1, _s1, c2, _s2) in enumerate(items) if is_finite(c1) and is_finite(c2)]
    out: List[Optional[dict]] = [None] * len(items)
    if len(keep) < len(items):
        logger.warning("TM-align: %d of %d pairs have a chain with a non-finite coordinate; they are not aligned",
                       len(items) - len(keep), len(items))
    if not keep:
        return out
    from .. import ops
    from .._lib import TM_OK

    structs, seqs, index = [], [], {}

    def slot(coords, seq):
        key = (id(coords), seq)
        if key not in index:
            index[key] = len(structs)
            structs.append(pdb_values(coords))
            seqs.append(seq)
        return index[key]

    pairs = [(slot(items[p][0], items[p][1]), slot(items[p][2], items[p][3])) for p in keep]
    got = ops.tmalign_batch(structs, seqs, pairs, fast=fast, device=device)
    for k, p in enumerate(keep):
        if got["status"][k] == TM_OK:
            out[p] = printed_values(got["qtm"][k], got["ttm"][k], got["rmsd"][k], got["n_ali8"][k], got["n_identical"][k])
    return out
