"""Structures and pairs shared by the TM-align tests (TEST INFRASTRUCTURE).

The golden CA traces, contiguous truncations, noisy copies and copies with a displaced loop insert of them, and random
walks.  Every coordinate is what the %8.3f PDB text of the binary path carries (tmalign_ref.pdb_values)."""
import glob
import os

import numpy as np

from merizo_search_amd.foldclass import pdbio, synthetic as syn
from tmalign_ref import pdb_values

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AA = "ACDEFGHIKLMNPQRSTVWY"


def golden_traces():
    """[(name, coords fp64, seq)] of tests/golden/*_ca.pdb, shortest first."""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*_ca.pdb"))):
        d = pdbio.read_pdb(path, "A")
        out.append((os.path.basename(path)[:-len("_ca.pdb")], pdb_values(d["coords"]), d["seq"]))
    return sorted(out, key=lambda t: len(t[1]))


def seq_of(n: int, seed: int) -> str:
    rng = np.random.default_rng(seed)
    return "".join(AA[i] for i in rng.integers(0, len(AA), n))


def walk(n: int, seed: int) -> np.ndarray:
    return pdb_values(syn.random_walk(n, seed))


def rigid(x: np.ndarray, seed: int) -> np.ndarray:
    """A random rotation + translation of x (then rounded as the PDB text rounds it)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(4)
    a, b, c, d = q / np.linalg.norm(q)
    r = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    return pdb_values(x @ r.T + rng.uniform(-30, 30, 3))


def noisy(x: np.ndarray, sigma: float, seed: int) -> np.ndarray:
    return pdb_values(x + np.random.default_rng(seed).normal(0, sigma, x.shape))


def with_insert(x: np.ndarray, at: int, n: int = 15, seed: int = 0) -> np.ndarray:
    """x with an n-residue loop inserted after residue `at`, displaced away from the chain; x's residues keep their
    coordinates."""
    loop = syn.random_walk(n, seed).astype(np.float64)
    loop = loop - loop[0] + x[at] + np.array([0.0, 0.0, 12.0])
    return pdb_values(np.concatenate([x[:at + 1], loop, x[at + 1:]]))


def fixture_structures():
    """[(name, coords, seq)]: the golden traces and their derived copies, and random walks."""
    out = []
    for k, (name, x, s) in enumerate(golden_traces()):
        n = len(x)
        out.append((name, x, s))
        a, b = n // 5, n - n // 6
        out.append((name + "_trunc", x[a:b].copy(), s[a:b]))
        out.append((name + "_noisy", noisy(x, 1.0, 10 + k), s))
        if n > 40:
            at = n // 2
            out.append((name + "_ins", with_insert(x, at, 15, k), s[:at + 1] + "G" * 15 + s[at + 1:]))
        out.append((name + "_rigid", rigid(x, 20 + k), s))
    for n, seed in ((6, 1), (19, 2), (22, 3), (40, 4), (150, 5), (150, 6)):
        out.append(("walk%d_%d" % (n, seed), walk(n, seed), seq_of(n, seed)))
    return out


def fixture_pairs(structs, max_len: int = 450):
    """Pairs (i, j) of fixture_structures: every structure with itself, each derived copy with its origin both ways,
    and a few unrelated pairs; chains longer than max_len are left to the GPU-only tests."""
    idx = {name: i for i, (name, _x, _s) in enumerate(structs)}
    ok = lambda i: len(structs[i][1]) <= max_len
    pairs = []
    for name, i in idx.items():
        if not ok(i):
            continue
        pairs.append((i, i))
        for suffix in ("_trunc", "_noisy", "_ins", "_rigid"):
            j = idx.get(name + suffix)
            if j is not None and ok(j):
                pairs += [(i, j), (j, i)]
    walks = [i for n, i in idx.items() if n.startswith("walk") and ok(i)]
    golds = [idx[name] for name, _x, _s in golden_traces() if ok(idx[name])]
    pairs += [(a, b) for a in walks for b in golds]
    pairs += [(walks[-1], walks[-2]), (walks[0], walks[-1])]
    return pairs
