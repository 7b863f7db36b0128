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


# ------------------------------------------------------------------ edges, long chains, slot reuse, C-level statuses ----
def _restated(structs, pairs, fast):
    """order=kernel results of every pair (None where TM-align refuses it), on at most 16 host threads (ctypes releases
    the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    R.load()

    def one(pair):
        (_a, x, sx), (_b, y, sy) = structs[pair[0]], structs[pair[1]]
        if min(len(x), len(y)) <= 5:
            return None
        return R.tm_align(x, y, sx, sy, fast=fast, order="kernel", quantize=False)
    with ThreadPoolExecutor(max_workers=min(16, max(len(pairs), 1))) as ex:
        return list(ex.map(one, pairs))


def _assert_invariants(got, lens1, lens2):
    """What holds for every result whatever the restatement says: ordered in-range alignments, counts, score ranges;
    refused pairs: zero outputs and an all -1 row."""
    for p, (xlen, ylen) in enumerate(zip(lens1, lens2)):
        row = got["invmap"][p]
        if got["status"][p] != 0:
            assert got["qtm"][p] == 0 and got["ttm"][p] == 0 and got["rmsd"][p] == 0, p
            assert got["n_ali8"][p] == 0 and got["n_identical"][p] == 0, p
            assert (row == -1).all(), p
            continue
        assert (row[ylen:] == -1).all(), p
        inv = row[:ylen]
        ali = inv[inv >= 0]
        assert (inv >= -1).all() and (ali < xlen).all() and (np.diff(ali) > 0).all(), p
        assert 0 <= got["n_identical"][p] <= got["n_ali8"][p] <= len(ali), p
        for key in ("qtm", "ttm"):
            assert 0 <= got[key][p] <= 1 + 1e-12, (p, key, got[key][p])
        assert got["rmsd"][p] >= 0, p


def _assert_matches_restatement(label, structs, pairs, fast, got):
    """Per pair: the same alignment, n_ali8 and n_identical as order=kernel, |dTM|, |dRMSD| <= 1e-9; prints how many are
    bit-identical."""
    lens = [len(s[1]) for s in structs]
    _assert_invariants(got, [lens[i] for i, _j in pairs], [lens[j] for _i, j in pairs])
    refs = _restated(structs, pairs, fast)
    n_bits = n_ok = 0
    for p, ((i, j), ref) in enumerate(zip(pairs, refs)):
        what = "%s: %s x %s fast=%s" % (label, structs[i][0], structs[j][0], fast)
        if ref is None:
            assert got["status"][p] == 1, what
            continue
        assert got["status"][p] == 0, what
        n_ok += 1
        assert np.array_equal(got["invmap"][p, :lens[j]], ref["invmap"]), what
        assert got["n_ali8"][p] == ref["n_ali8"] and got["n_identical"][p] == ref["n_identical"], what
        for key in ("qtm", "ttm", "rmsd"):
            assert abs(got[key][p] - ref[key]) <= 1e-9, (what, key, got[key][p], ref[key])
        n_bits += all(np.float64(got[k][p]).tobytes() == np.float64(ref[k]).tobytes() for k in ("qtm", "ttm", "rmsd"))
    print("\n%s (fast=%s): %d / %d aligned pairs bit-identical to order=kernel (%d pairs, %d refused)"
          % (label, fast, n_bits, n_ok, len(pairs), len(pairs) - n_ok))


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("which", ["boundary_set", "ties_set", "degenerate_set"])
def test_kernel_matches_the_restatement_on_the_edge_sets(which, fast):
    structs, pairs = getattr(tm_case, which)()
    _assert_matches_restatement(which, structs, pairs, fast, _gpu_batch(structs, pairs, fast))


@pytest.mark.parametrize("fast", [False, True])
def test_kernel_matches_the_restatement_on_long_chains(fast):
    structs, pairs = tm_case.long_set(fast)
    _assert_matches_restatement("long_set", structs, pairs, fast, _gpu_batch(structs, pairs, fast))


def _short_chains(n_structs=120, seed=9):
    """Golden slices of 20-150 residues and noisy copies of them."""
    rng = np.random.default_rng(seed)
    structs = []
    for k in range(n_structs // 2):
        n = int(rng.integers(20, 151))
        x, s = tm_case.golden_slice(n, int(rng.integers(0, 10 ** 6)))
        structs += [("g%d_%d" % (k, n), x, s), ("g%d_%d_noisy" % (k, n), tm_case.noisy(x, 1.5, 900 + k), s)]
    return structs


def _slots(max1, max2, npairs):
    from merizo_search_amd import _lib
    lib = _lib.load()
    one = int(lib.ms_tmalign_workspace_bytes(max1, max2, 1))
    per = int(lib.ms_tmalign_workspace_bytes(max1, max2, 2)) - one
    return (int(lib.ms_tmalign_workspace_bytes(max1, max2, npairs)) - one) // per + 1


@pytest.mark.parametrize("fast", [False, True])
def test_workgroups_that_run_several_pairs_match_the_restatement(fast):
    structs = _short_chains()
    rng = np.random.default_rng(11)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, len(structs), size=(2300, 2))]
    lens = [len(s[1]) for s in structs]
    assert _slots(max(lens[i] for i, _ in pairs), max(lens[j] for _, j in pairs), len(pairs)) < len(pairs)
    _assert_matches_restatement("2300 short pairs", structs, pairs, fast, _gpu_batch(structs, pairs, fast))


def _packed(structs):
    import torch
    lens = np.array([len(s[1]) for s in structs], np.int64)
    offsets = np.zeros(len(structs) + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    xyz = np.concatenate([s[1] for s in structs]).astype(np.float64)
    seq = np.frombuffer("".join(s[2] for s in structs).encode(), np.uint8).copy()
    return [torch.from_numpy(a).to("cuda:0") for a in (xyz, seq, offsets)]


def _raw_batch(structs, pairs, fast, max1, max2, ws):
    """ms_tmalign_batch through ctypes, pairs in the order given (no host sort), on the caller's workspace tensor."""
    import torch
    from merizo_search_amd import _lib
    lib = _lib.load()
    d_xyz, d_seq, d_off = _packed(structs)
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda:0").reshape(-1, 2)
    npairs = d_pairs.shape[0]
    of = torch.full((npairs, 3), float("nan"), dtype=torch.float64, device="cuda:0")
    oi = torch.full((npairs, 3), -7, dtype=torch.int32, device="cuda:0")
    inv = torch.full((npairs, max2), -1, dtype=torch.int32, device="cuda:0")
    rc = lib.ms_tmalign_batch(d_xyz.data_ptr(), d_seq.data_ptr(), d_off.data_ptr(), len(structs), d_pairs.data_ptr(), npairs,
                              max1, max2, _lib.TM_FAST if fast else 0, ws.data_ptr(), ws.numel(), of.data_ptr(), oi.data_ptr(),
                              inv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ms_last_error()
    torch.cuda.synchronize()
    f, i = of.cpu().numpy(), oi.cpu().numpy()
    return {"qtm": f[:, 0], "ttm": f[:, 1], "rmsd": f[:, 2], "n_ali8": i[:, 0], "n_identical": i[:, 1], "status": i[:, 2],
            "invmap": inv.cpu().numpy()}


def _assert_same_bits(a, b, rows, what):
    for key in ("qtm", "ttm", "rmsd", "n_ali8", "n_identical", "status"):
        assert np.asarray(a[key])[rows].tobytes() == np.asarray(b[key])[rows].tobytes(), (what, key)
    for r in rows:
        assert np.array_equal(a["invmap"][r], b["invmap"][r][:a["invmap"].shape[1]]), (what, r)


@pytest.mark.parametrize("fast", [False, True])
def test_one_to_three_poisoned_slots_give_the_bits_of_a_plain_run(fast):
    """Workspaces of exactly 1, 2 and 3 slots, filled with random bytes and then 0xFF, pairs short -> long -> short: each
    slot (and its workgroup's LDS) takes pairs of growing, then shrinking extents over stale state of the pair before."""
    import torch
    from merizo_search_amd import _lib
    structs = _short_chains(16, 21) + [("walk5", tm_case.walk(5, 5), "A" * 5)]
    structs.sort(key=lambda t: len(t[1]))                                      # walk5 (refused) first, the longest last
    k = len(structs) - 1
    order = [1, 5, 9, 13, k - 1, k, 14, 10, 6, 2, k, 0, 3, 12, 4]            # short -> long -> short
    pairs = [(order[m], order[m + 1]) for m in range(len(order) - 1)] + [(k - 1, k - 1), (2, 0), (k, 5)]
    plain = _gpu_batch(structs, pairs, fast)
    lens = [len(s[1]) for s in structs]
    max1, max2 = max(lens[i] for i, _ in pairs), max(lens[j] for _, j in pairs)
    lib = _lib.load()
    base = int(lib.ms_tmalign_workspace_bytes(max1, max2, 1))
    per = int(lib.ms_tmalign_workspace_bytes(max1, max2, 2)) - base
    for slots in (1, 2, 3):
        ws = torch.empty(base + (slots - 1) * per, dtype=torch.uint8, device="cuda:0")
        for fill in ("random", 0xFF):
            if fill == "random":
                ws.copy_(torch.randint(0, 256, (ws.numel(),), dtype=torch.uint8, generator=torch.Generator().manual_seed(slots)))
            else:
                ws.fill_(fill)
            got = _raw_batch(structs, pairs, fast, max1, max2, ws)
            _assert_same_bits(got, plain, range(len(pairs)), (slots, fill))
    _assert_matches_restatement("poisoned slots", structs, pairs, fast, plain)


def test_long_and_index_statuses_leave_the_other_pairs_bits():
    """MS_TM_ERR_LONG (a chain over the max_len1 / max_len2 passed in) and MS_TM_ERR_INDEX next to valid pairs: the refused
    pairs get status, zero outputs and an untouched (-1) alignment row; the valid pairs keep the bits of a plain run."""
    import torch
    from merizo_search_amd import _lib
    structs = _short_chains(12, 31)
    lens = [len(s[1]) for s in structs]
    short = sorted(range(len(structs)), key=lambda s: lens[s])
    max1 = lens[short[6]]                              # chains 1 longer than this are refused
    pairs = [(short[0], short[1]), (short[-1], short[2]), (short[3], short[-1]), (len(structs), short[0]),
             (short[1], -1), (short[5], short[4]), (short[-2], short[-3]), (short[6], short[0])]
    max2 = max(lens[j] for _i, j in pairs if 0 <= j < len(structs))
    ws = torch.empty(int(_lib.load().ms_tmalign_workspace_bytes(max1, max2, len(pairs))), dtype=torch.uint8, device="cuda:0")
    ws.fill_(0xFF)
    got = _raw_batch(structs, pairs, False, max1, max2, ws)
    ns = len(structs)
    expect = [_lib.TM_ERR_INDEX if not (0 <= i < ns and 0 <= j < ns) else _lib.TM_ERR_LONG if lens[i] > max1 else 0
              for i, j in pairs]
    assert list(got["status"]) == expect and expect.count(_lib.TM_ERR_LONG) >= 2
    valid = [p for p, e in enumerate(expect) if e == 0]
    assert len(valid) >= 3
    plain = _gpu_batch(structs, [pairs[p] for p in valid], False)
    sub = {k: np.asarray(v)[valid] for k, v in got.items()}
    _assert_same_bits(sub, plain, range(len(valid)), "valid pairs")
    _assert_invariants(got, [lens[i] if 0 <= i < len(structs) else 0 for i, _ in pairs],
                       [lens[j] if 0 <= j < len(structs) else 0 for _, j in pairs])
