"""ctypes binding of tests/tmalign_ref.c, the CPU restatement of TM-align (TEST INFRASTRUCTURE; the product never
imports it).  Built on first use with the host gcc into a cache directory keyed by the source's hash."""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tmalign_ref.c")
ORDERS = {"seq": 0, "kernel": 1}
_lib = None


def _cache_dir() -> str:
    base = os.environ.get("MS_TEST_CACHE") or os.path.join(tempfile.gettempdir(), "merizo_search_amd_%d" % os.getuid())
    os.makedirs(base, exist_ok=True)
    return base


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = open(_SRC, "rb").read()
    so = os.path.join(_cache_dir(), "tmalign_ref_%s.so" % hashlib.sha256(src).hexdigest()[:16])
    if not os.path.exists(so):
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, _SRC, "-lm"], check=True)
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.tm_align.restype = ctypes.c_int
    lib.tm_align.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    lib.tm_kabsch.restype = ctypes.c_int
    lib.tm_kabsch.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    _lib = lib
    return lib


def pdb_values(coords) -> np.ndarray:
    """What TM-align parses from the %8.3f text of a written PDB: float("%.3f" % v) -- as the product's aligner."""
    return np.asarray([[float("%.3f" % v) for v in row] for row in np.asarray(coords, dtype=np.float64)], dtype=np.float64).reshape(-1, 3)


def _seq_bytes(seq, n):
    if seq is None:
        return np.zeros(n, np.uint8)
    return np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8).copy()


def tm_align(x, y, seqx=None, seqy=None, fast=False, order="seq", quantize=True) -> dict:
    """x = chain 1 (query), y = chain 2.  -> {qtm, ttm, rmsd, n_ali8, n_identical, invmap}; raises ValueError for a chain
    of <= 5 residues (TM-align refuses them)."""
    x = pdb_values(x) if quantize else np.ascontiguousarray(x, dtype=np.float64)
    y = pdb_values(y) if quantize else np.ascontiguousarray(y, dtype=np.float64)
    sx, sy = _seq_bytes(seqx, len(x)), _seq_bytes(seqy, len(y))
    out_f = np.zeros(3, np.float64)
    out_i = np.zeros(2, np.int32)
    inv = np.zeros(max(len(y), 1), np.int32)
    rc = load().tm_align(x.ctypes.data, len(x), sx.ctypes.data, y.ctypes.data, len(y), sy.ctypes.data, int(bool(fast)),
                         ORDERS[order], out_f.ctypes.data, out_i.ctypes.data, inv.ctypes.data)
    if rc != 0:
        raise ValueError("TM-align refuses structures of <= 5 residues (%d, %d)" % (len(x), len(y)))
    return {"qtm": float(out_f[0]), "ttm": float(out_f[1]), "rmsd": float(out_f[2]), "n_ali8": int(out_i[0]),
            "n_identical": int(out_i[1]), "invmap": inv[:len(y)].copy()}


def kabsch(r1, r2):
    """The restatement's superposition of the point pairs r1 -> r2 in order=kernel (the kernel's solver, op for op):
    (t [3], u [3][3]) with r2 ~ r1 @ u.T + t."""
    r1 = np.ascontiguousarray(r1, dtype=np.float64).reshape(-1, 3)
    r2 = np.ascontiguousarray(r2, dtype=np.float64).reshape(-1, 3)
    assert len(r1) == len(r2)
    t, u = np.zeros(3), np.zeros((3, 3))
    if load().tm_kabsch(r1.ctypes.data, r2.ctypes.data, len(r1), t.ctypes.data, u.ctypes.data) != 0:
        raise ValueError("tm_kabsch refused n = %d" % len(r1))
    return t, u
