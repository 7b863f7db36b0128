"""Batched TM-align on the MI355X (ms_tmalign.hip) against the CPU restatement tests/tmalign_ref.c, and the drivers'
`--tmalign_backend hip` against the binary path run with a stand-in binary that executes the same restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tm_case
import tmalign_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_batch(structs, pairs, fast):
    from merizo_search_amd import ops
    return ops.tmalign_batch([s[1] for s in structs], [s[2] for s in structs], pairs, fast=fast, device="cuda:0",
                             want_invmap=True)


@pytest.fixture(scope="module")
def fixtures():
    structs = tm_case.fixture_structures()
    return structs, tm_case.fixture_pairs(structs)


@pytest.mark.parametrize("fast", [False, True])
def test_kernel_matches_the_restatement_on_every_fixture_pair(fixtures, fast):
    structs, pairs = fixtures
    got = _gpu_batch(structs, pairs, fast)
    n_bits, n_seq_diff, worst_seq = 0, 0, 0.0
    for p, (i, j) in enumerate(pairs):
        (ni, x, sx), (nj, y, sy) = structs[i], structs[j]
        ref = R.tm_align(x, y, sx, sy, fast=fast, order="kernel", quantize=False)
        seq = R.tm_align(x, y, sx, sy, fast=fast, order="seq", quantize=False)
        what = "%s x %s fast=%s" % (ni, nj, fast)
        if min(len(x), len(y)) <= 5:
            assert got["status"][p] == 1, what
            continue
        assert got["status"][p] == 0, what
        assert np.array_equal(got["invmap"][p, :len(y)], ref["invmap"]), what
        assert got["n_ali8"][p] == ref["n_ali8"] and got["n_identical"][p] == ref["n_identical"], what
        for key in ("qtm", "ttm", "rmsd"):
            assert abs(got[key][p] - ref[key]) <= 1e-9, (what, key, got[key][p], ref[key])
        n_bits += all(np.float64(got[k][p]).tobytes() == np.float64(ref[k]).tobytes() for k in ("qtm", "ttm", "rmsd"))
        n_seq_diff += not np.array_equal(seq["invmap"], ref["invmap"])
        worst_seq = max(worst_seq, abs(seq["qtm"] - got["qtm"][p]), abs(seq["ttm"] - got["ttm"][p]))
        assert worst_seq <= 1e-4, what
    print("\n%d pairs (fast=%s): %d bit-identical to order=kernel; against order=seq %d alignments differ, max |dTM| %.2e"
          % (len(pairs), fast, n_bits, n_seq_diff, worst_seq))


def test_refused_and_oversized_inputs():
    from merizo_search_amd import ops
    from merizo_search_amd._lib import MerizoHipError
    x = tm_case.walk(30, 1)
    got = ops.tmalign_batch([x, x[:5], x[:6]], ["A" * 30, "A" * 5, "A" * 6], [(0, 1), (1, 0), (0, 2)], device="cuda:0")
    assert list(got["status"]) == [1, 1, 0]
    with pytest.raises(MerizoHipError, match="2000"):
        ops.tmalign_batch([tm_case.walk(2001, 1), x], ["A" * 2001, "A" * 30], [(0, 1)], device="cuda:0")


def _mixed_batch():
    from merizo_search_amd.foldclass import synthetic as syn
    lens = [int(n) for n in syn.ted_lengths(300, seed=5)] + [6, 7, 2000, 1500, 683]
    structs = [("s%d" % k, tm_case.walk(max(n, 6), 1000 + k), tm_case.seq_of(max(n, 6), k)) for k, n in enumerate(lens)]
    rng = np.random.default_rng(3)
    n = len(structs)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, n - 5, size=(300, 2))]
    pairs += [(n - 5, 0), (1, n - 4), (n - 3, 2), (3, n - 3), (n - 2, 4), (n - 1, n - 1), (5, 5)]
    return structs, pairs


def test_a_pair_gives_the_same_bits_alone_and_in_a_mixed_batch_and_from_run_to_run():
    structs, pairs = _mixed_batch()
    a = _gpu_batch(structs, pairs, False)
    b = _gpu_batch(structs, pairs, False)
    for key in ("qtm", "ttm", "rmsd", "n_ali8", "n_identical", "status", "invmap"):
        assert np.array_equal(a[key], b[key]), key
    assert (a["status"] == 0).all()
    for p in [0, 1, 150, len(pairs) - 7, len(pairs) - 5, len(pairs) - 3, len(pairs) - 1]:
        alone = _gpu_batch(structs, [pairs[p]], False)
        for key in ("qtm", "ttm", "rmsd"):
            assert np.float64(alone[key][0]).tobytes() == np.float64(a[key][p]).tobytes(), (p, key)
        assert alone["n_ali8"][0] == a["n_ali8"][p]
        assert np.array_equal(alone["invmap"][0, :len(structs[pairs[p][1]][1])], a["invmap"][p, :len(structs[pairs[p][1]][1])])


# ------------------------------------------------------------------ end to end against the binary path ------------------
STAND_IN = '''#!/usr/bin/env python3
"""Test stand-in for the TM-align binary: the CPU restatement (order=kernel) on two CA-only PDB files, TM-align's output."""
import sys
sys.path.insert(0, %(tests)r)
sys.path.insert(0, %(repo)r)
import numpy as np
import tmalign_ref as R
from merizo_search_amd.foldclass.constants import three_to_single_aa

def read(path):
    xyz, seq = [], []
    for line in open(path):
        if line.startswith("ATOM") and line[12:16] == " CA ":
            xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
            seq.append(three_to_single_aa.get(line[17:20], "X"))
    return np.asarray(xyz, dtype=np.float64).reshape(-1, 3), "".join(seq)

(x, sx), (y, sy) = read(sys.argv[1]), read(sys.argv[2])
try:
    r = R.tm_align(x, y, sx, sy, fast="-fast" in sys.argv[3:], order="kernel")
except ValueError:
    print("Sequence is too short <=5!", file=sys.stderr)
    sys.exit(1)
sid = r["n_identical"] / r["n_ali8"] if r["n_ali8"] else 0.0
print("Aligned length= %%4d, RMSD= %%6.2f, Seq_ID=n_identical/n_aligned= %%4.3f" %% (r["n_ali8"], r["rmsd"], sid))
print("TM-score= %%6.5f (if normalized by length of Chain_1)" %% r["qtm"])
print("TM-score= %%6.5f (if normalized by length of Chain_2)" %% r["ttm"])
'''


def _stand_in(tmp_path) -> str:
    import stat
    R.load()                                                    # build the restatement once, before the subprocesses
    path = os.path.join(str(tmp_path), "tmalign")
    with open(path, "w") as fh:
        fh.write(STAND_IN % {"tests": os.path.dirname(os.path.abspath(__file__)), "repo": REPO})
    os.chmod(path, os.stat(path).st_mode | stat.S_IEXEC)
    return path


def _runner(tmp_path):
    base = {k: v for k, v in os.environ.items() if k != "MERIZO_TMALIGN"}
    base.update(MERIZO_ALLOW_SYNTHETIC_WEIGHTS="1", PYTHONPATH=REPO)

    def run(*args, binary=None):
        env = dict(base, MERIZO_TMALIGN=binary) if binary else base
        r = subprocess.run([sys.executable, "-m", "merizo_search_amd.cli", *args], env=env, capture_output=True, text=True,
                           cwd=str(tmp_path), timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        return r
    return run


@pytest.fixture(scope="module")
def e2e_db(tmp_path_factory):
    from merizo_search_amd.foldclass import pdbio
    tmp = tmp_path_factory.mktemp("tm_e2e")
    pdbdir = tmp / "pdbs"
    pdbdir.mkdir()
    for name, x, s in tm_case.fixture_structures():
        pdbio.write_pdb(str(pdbdir), x.astype(np.float32), s, name=name)
    run = _runner(tmp)
    for layout in ("pt", "faiss"):
        run("createdb", str(pdbdir), str(tmp / ("db_" + layout)), "-d", "cuda", "--layout", layout)
    return tmp


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("layout", ["pt", "faiss"])
def test_search_and_easy_search_hip_equal_the_binary_path(e2e_db, tmp_path, golden_dir, fast, layout):
    run = _runner(tmp_path)
    standin = _stand_in(tmp_path)
    db = str(e2e_db / ("db_" + layout))
    common = ["-d", "cuda", "-s", "-1", "--report_insignificant_hits", "--output_headers"] + (["--fastmode"] if fast else [])
    queries = [os.path.join(golden_dir, f) for f in ("M0_ca.pdb", "3w5h_ca.pdb")]
    pd2 = os.path.join(golden_dir, "AF-Q96HM7-F1-model_v4_ca.pdb")
    for tag, extra in (("bin", {"binary": standin}), ("hip", {})):
        flags = ["--tmalign_backend", "hip"] if tag == "hip" else []
        run("search", *queries, db, str(tmp_path / ("s_" + tag)), str(tmp_path / "tmp"), "-k", "4", *common, *flags, **extra)
        run("easy-search", pd2, db, str(tmp_path / ("e_" + tag)), str(tmp_path / "tmp"), "-k", "3", "--chopping",
            "1-150,151-300,301-432", *common, *flags, **extra)
    for prefix in ("s_", "e_"):
        for suffix in ("_search.tsv", "_search_insignificant.tsv"):
            a = open(str(tmp_path / (prefix + "bin")) + suffix, "rb").read()
            b = open(str(tmp_path / (prefix + "hip")) + suffix, "rb").read()
            assert a == b, (prefix, suffix)
        head = open(str(tmp_path / (prefix + "hip")) + "_search.tsv").readline().rstrip("\n").split("\t")
        assert {"q_tm", "t_tm", "ali_len", "rmsd"} <= set(head), head
    rows = [l.split("\t") for l in open(str(tmp_path / "s_hip_search.tsv")).read().splitlines()[1:]]
    assert rows, "no hit passed the TM-score threshold"


def test_multi_domain_search_runs_on_the_gpu_aligner_without_a_binary(tmp_path):
    import md_case
    run = _runner(tmp_path)
    qpdb, dbdir = md_case.write_inputs(tmp_path)
    run("createdb", dbdir, str(tmp_path / "db"), "-d", "cuda", "--layout", "faiss")
    args = ["-d", "cuda", "-k", "3", "-s", "0.5", "--chopping", md_case.CHOPPING, "--multi_domain_search",
            "--multi_domain_mode", "exhaustive_tmalign", "--output_headers"]
    run("easy-search", qpdb, str(tmp_path / "db"), str(tmp_path / "hip"), str(tmp_path / "tmp"), *args, "--tmalign_backend", "hip")
    rows = [l.rstrip("\n").split("\t") for l in open(str(tmp_path / "hip") + "_search_multi_dom.tsv")]
    got = {(r[2], r[4]): r for r in rows[1:]}
    t1 = md_case.T1.replace(":0.9", ":1.0")
    t3 = md_case.T3.replace(":0.9", ":1.0")
    assert got[("AF-T1-F1-model_v4", "2")][:4] == ["Q", "2", "AF-T1-F1-model_v4", "3"] and got[("AF-T1-F1-model_v4", "2")][5] == t1
    assert got[("AF-T3-F1-model_v4", "0")][:4] == ["Q", "2", "AF-T3-F1-model_v4", "2"] and got[("AF-T3-F1-model_v4", "0")][5] == t3
    assert not any(r[2] == "AF-T2-F1-model_v4" for r in rows[1:])
    hits = [l.split("\t") for l in open(str(tmp_path / "hip") + "_search.tsv").read().splitlines()[1:]]
    exact = [h for h in hits if h[5] in ("AF-T1-F1-model_v4_TED01", "AF-T1-F1-model_v4_TED02", "AF-T3-F1-model_v4_TED01",
                                         "AF-T3-F1-model_v4_TED02")]
    assert len(exact) == 4
    run("easy-search", qpdb, str(tmp_path / "db"), str(tmp_path / "bin"), str(tmp_path / "tmp"), *args, binary=_stand_in(tmp_path))
    for suffix in ("_search.tsv", "_search_multi_dom.tsv"):
        assert open(str(tmp_path / "hip") + suffix, "rb").read() == open(str(tmp_path / "bin") + suffix, "rb").read(), suffix
