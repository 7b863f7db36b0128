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


# ------------------------------------------------------------------ sets aimed at the kernel's edges ---------------------
# Each set is ([(name, coords, seq)], [(i, j)]).  Slices come from the 775-residue golden trace (AlphaFold model: real helices
# and strands for make_sec / get_initial_ss / ssplus).
BOUNDARY_LENGTHS = (6, 7, 11, 12, 15, 19, 20, 21, 22, 24, 27, 40, 41, 63, 64, 65, 127, 128, 129, 150, 151, 192, 193, 200,
                    201, 250, 251)


def _longest_golden():
    return golden_traces()[-1]


def golden_slice(n: int, at: int):
    _name, x, s = _longest_golden()
    at = at % (len(x) - n + 1)
    return x[at:at + n].copy(), s[at:at + n]


def boundary_set():
    """Slices and noisy copies (sigma 1.5 A) at the lengths where a parameter or the DP's 64-row block structure changes:
    d0 (19/20, 21/22), min_ali (11/12), fra_min against len/3 (12/15 normal, 24/27 fast), ddcc (40/41), 64k +- 1, the
    initial5 jumps (150/151, 200/201, 250/251), 192/193.  Every length is chain 1 and chain 2 against its noisy copy,
    the next longer and the next shorter length."""
    structs, pairs = [], []
    for k, n in enumerate(BOUNDARY_LENGTHS):
        x, s = golden_slice(n, 97 * k + 11)
        structs.append(("slice%d" % n, x, s))
        structs.append(("noisy%d" % n, noisy(x, 1.0 + 0.5 * (k % 3), 500 + k), s))
    for k in range(len(BOUNDARY_LENGTHS)):
        a, na = 2 * k, 2 * k + 1
        pairs += [(a, na), (na, a)]
        for o in (k - 1, k + 1):
            if 0 <= o < len(BOUNDARY_LENGTHS):
                pairs += [(a, 2 * o + 1), (2 * o + 1, a)]
    return structs, pairs


def _translated(x: np.ndarray, v) -> np.ndarray:
    return pdb_values(x + np.asarray(v, dtype=np.float64))


def _linker(a: np.ndarray, b: np.ndarray, step: float = 3.8) -> np.ndarray:
    """Points on the segment from a to b (exclusive), about `step` apart."""
    m = max(int(np.ceil(np.linalg.norm(b - a) / step)), 1)
    return np.array([a + (b - a) * (i / m) for i in range(1, m)]).reshape(-1, 3)


def tandem_repeat(fragment: np.ndarray, copies: int, shift) -> np.ndarray:
    """`copies` translated copies of fragment (translation k * shift: the copies' internal geometry is identical, so a
    threading onto any copy scores exactly the same) joined by straight linkers."""
    parts = [fragment]
    for k in range(1, copies):
        nxt = _translated(fragment, np.asarray(shift) * k)
        parts += [pdb_values(_linker(parts[-1][-1], nxt[0])), nxt]
    return np.concatenate([p for p in parts if len(p)])


def collinear(n: int, step: float = 3.8) -> np.ndarray:
    return pdb_values(np.outer(np.arange(n), [step, 0.0, 0.0]) + np.array([1.5, -2.25, 3.0]))


def zigzag(n: int) -> np.ndarray:
    """A planar zig-zag in z = 0: CA steps of 3.8 A at +-30 degrees about the x axis."""
    return pdb_values(np.array([[3.8 * np.cos(np.pi / 6) * i, 1.9 * (i % 2), 0.0] for i in range(n)]))


def ties_set():
    """Exact ties and near-ties: a tandem repeat against one copy and itself (the threading shifts onto each copy tie
    exactly), a circular permutation, chains whose longest continuous fragments are equally long (fgt's Lx == Ly branch
    with xlen < ylen and xlen > ylen), and straight chains of different lengths (every shift of the full overlap ties)."""
    frag, fs = golden_slice(40, 300)
    frag = pdb_values(frag)
    rep3 = tandem_repeat(frag, 3, [41.5, 0.0, 0.0])
    rep2 = tandem_repeat(frag, 2, [0.0, 38.25, 0.0])
    g, gs = golden_slice(90, 150)
    perm = np.concatenate([g[30:], g[:30]])

    def broken(x, at):            # chain breaks (10 A jumps) before the residues `at`: continuous fragments between them
        x = x.copy()
        for a in at:
            x[a:] += np.array([0.0, 0.0, 10.0])
        return pdb_values(x)
    a60, s60 = golden_slice(60, 420)
    a80, s80 = golden_slice(80, 520)
    structs = [("frag40", frag, fs), ("rep3", rep3, seq_of(len(rep3), 71)), ("rep2", rep2, seq_of(len(rep2), 72)),
               ("g90", g, gs), ("g90_perm", perm, gs[30:] + gs[:30]),
               ("brk60", broken(a60, [30]), s60), ("brk80", broken(a80, [30, 50]), s80),
               ("line50", collinear(50), seq_of(50, 73)), ("line30", collinear(30), seq_of(30, 74))]
    idx = {s[0]: i for i, s in enumerate(structs)}
    names = [("frag40", "rep3"), ("rep3", "frag40"), ("rep3", "rep3"), ("frag40", "rep2"), ("rep2", "frag40"),
             ("rep2", "rep3"), ("g90", "g90_perm"), ("g90_perm", "g90"), ("brk60", "brk80"), ("brk80", "brk60"),
             ("line50", "line30"), ("line30", "line50"), ("line50", "line50")]
    return structs, [(idx[a], idx[b]) for a, b in names]


def degenerate_set():
    """Geometry where a superposition or a relaxation loop could go wrong: a mirror image, a straight line, a planar
    zig-zag, all residues on one point, every residue twice, a chain 9,000 A from the origin, and an "exploded" chain
    (CA steps of 2 kA: find_max_frag never finds a fragment and stops at its cap), aligned only with its rigid copies."""
    g, gs = golden_slice(70, 230)
    mirror = g * np.array([1.0, 1.0, -1.0])
    dup = np.repeat(g[:35], 2, axis=0)
    far = _translated(g, [9000.0, -9000.0, 9000.0])
    point = pdb_values(np.tile([[12.5, -3.25, 7.0]], (20, 1)))
    boom = pdb_values(syn.random_walk(12, 77, step=2000.0).astype(np.float64))
    structs = [("g70", g, gs), ("g70_mirror", mirror, gs), ("line40", collinear(40), seq_of(40, 81)),
               ("zigzag60", zigzag(60), seq_of(60, 82)), ("point20", point, "A" * 20), ("g35_dup", dup, seq_of(70, 83)),
               ("g70_far", far, gs), ("g70_far_rigid", rigid(far - 9000.0, 84) + 9000.0, gs),
               ("boom12", boom, seq_of(12, 85)), ("boom12_rigid", rigid(boom, 86), seq_of(12, 85))]
    idx = {s[0]: i for i, s in enumerate(structs)}
    names = [("g70", "g70_mirror"), ("g70_mirror", "g70"), ("line40", "g70"), ("g70", "line40"), ("line40", "zigzag60"),
             ("zigzag60", "zigzag60"), ("zigzag60", "g70"), ("point20", "point20"), ("point20", "g70"), ("g70", "point20"),
             ("g35_dup", "g70"), ("g70", "g35_dup"), ("g70_far", "g70"), ("g70", "g70_far"), ("g70_far", "g70_far_rigid"),
             ("boom12", "boom12"), ("boom12", "boom12_rigid"), ("boom12_rigid", "boom12")]
    return structs, [(idx[a], idx[b]) for a, b in names]


def long_chain(n: int) -> np.ndarray:
    """n residues: the golden traces laid end to end (each translated to start 3.8 A past the previous one's end)."""
    traces = [t[1] for t in golden_traces()[::-1]]
    parts, have, k = [], 0, 0
    while have < n:
        x = traces[k % len(traces)][:n - have]
        if parts:
            x = x - x[0] + parts[-1][-1] + np.array([3.8, 0.0, 0.0])
        parts.append(x)
        have += len(x)
        k += 1
    return pdb_values(np.concatenate(parts))


def long_set(fast: bool):
    """The 775-residue golden trace with its truncated, noisy, loop-inserted and rigidly moved copies (both ways, and with
    itself); 1000 x 300 and 2000 x 120 (noisy slices of the long chain) both ways; 1500 and 2000 against a truncation of
    themselves and 2000 x 2000 in fast mode only (1500 x 1200 in normal mode takes ~14 s on one host core, too long for
    one wave).  Every pair here is at most ~5 s on one host core."""
    name = _longest_golden()[0]
    structs = [s for s in fixture_structures() if s[0].startswith(name)]
    idx = {s[0]: i for i, s in enumerate(structs)}
    pairs = [(idx[name], idx[name])]
    for suffix in ("_trunc", "_noisy", "_ins", "_rigid"):
        pairs += [(idx[name], idx[name + suffix]), (idx[name + suffix], idx[name])]

    def add(nm, x, s):
        structs.append((nm, x, s))
        return len(structs) - 1
    for n, m, at in ((1000, 300, 350), (2000, 120, 1234)):
        x = long_chain(n)
        s = seq_of(n, n)
        a = add("long%d" % n, x, s)
        b = add("long%d_slice%d" % (n, m), noisy(x[at:at + m], 1.0, n), s[at:at + m])
        pairs += [(a, b), (b, a)]
    for n, lo, hi in ((1500, 100, 1300), (2000, 300, 1700)) if fast else ():
        x, s = long_chain(n), seq_of(n, n)
        a = add("long%d_t" % n, x, s)
        pairs.append((a, add("long%d_trunc" % n, x[lo:hi].copy(), s[lo:hi])))
        if n == 2000:
            pairs.append((a, a))
    return structs, pairs
