"""TM-align without a GPU: invariants of the CPU restatement (tests/tmalign_ref.c) that the kernel is tested against,
agreement of its two reduction orders, and the `--tmalign_backend` option of the command line."""
import os

import numpy as np
import pytest

import tm_case
import tmalign_ref as R
from merizo_search_amd.foldclass import synthetic as syn, tmalign as tm

LENGTHS = (6, 19, 20, 21, 22, 40, 150, 683, 2000)


def _fast(n):            # 2000 x 2000 in normal mode takes minutes on one core; the GPU tests cover it
    return n >= 2000


def _assert_identity(r, n):
    assert "%.5f" % r["qtm"] == "1.00000" and "%.5f" % r["ttm"] == "1.00000", r
    assert "%.2f" % r["rmsd"] == "0.00" and r["n_ali8"] == n, r


@pytest.mark.parametrize("n", LENGTHS)
def test_self_and_rigid_copy_align_perfectly(n):
    x = tm_case.walk(n, 100 + n)
    r = R.tm_align(x, x, fast=_fast(n))
    _assert_identity(r, n)
    assert np.array_equal(r["invmap"], np.arange(n))
    r = R.tm_align(x, tm_case.rigid(x, n), fast=_fast(n))
    _assert_identity(r, n)


@pytest.mark.parametrize("name", [g[0] for g in tm_case.golden_traces()])
def test_golden_traces_align_with_themselves_and_rigid_copies(name):
    _n, x, s = [g for g in tm_case.golden_traces() if g[0] == name][0]
    r = R.tm_align(x, x, s, s)
    _assert_identity(r, len(x))
    assert r["n_identical"] == len(x)
    _assert_identity(R.tm_align(x, tm_case.rigid(x, 7), s, s), len(x))


@pytest.mark.parametrize("n,a,b", [(40, 5, 30), (150, 20, 120), (292, 40, 250)])
def test_truncation_scores_its_fraction_of_the_whole(n, a, b):
    x = tm_case.golden_traces()[1][1] if n == 292 else tm_case.walk(n, n)
    r = R.tm_align(x, x[a:b])                 # chain 1 = the whole, chain 2 = the piece
    assert "%.5f" % r["ttm"] == "1.00000"
    assert abs(r["qtm"] - (b - a) / n) < 1e-12, (r["qtm"], (b - a) / n)
    assert r["n_ali8"] == b - a and np.array_equal(r["invmap"], np.arange(a, b))


def test_loop_insert_keeps_the_original_residues_paired():
    x = tm_case.walk(150, 8)
    y = tm_case.with_insert(x, 70, 15, 3)
    r = R.tm_align(x, y)
    expect = np.concatenate([np.arange(71), np.full(15, -1), np.arange(71, 150)])
    assert np.array_equal(r["invmap"], expect)
    assert "%.5f" % r["qtm"] == "1.00000" and r["n_ali8"] == 150


def test_tm_falls_with_noise():
    x = tm_case.walk(150, 9)
    tms = [R.tm_align(x, tm_case.noisy(x, s, 1))["qtm"] for s in (0.5, 1, 2, 4)]
    assert all(a > b for a, b in zip(tms, tms[1:])), tms


def test_unrelated_walks_score_low():
    for seed in range(3):
        r = R.tm_align(tm_case.walk(150, 200 + seed), tm_case.walk(150, 300 + seed))
        assert r["qtm"] < 0.5 and r["ttm"] < 0.5, r


def test_structures_of_five_residues_or_fewer_are_refused():
    x = tm_case.walk(30, 1)
    for n in (1, 3, 5):
        with pytest.raises(ValueError):
            R.tm_align(x, x[:n])
        with pytest.raises(ValueError):
            R.tm_align(x[:n], x)
    R.tm_align(x, x[:6])


def test_the_two_reduction_orders_agree_on_every_fixture_pair():
    structs = tm_case.fixture_structures()
    pairs = tm_case.fixture_pairs(structs, max_len=300)
    assert len(pairs) > 30
    for i, j in pairs:
        (_a, x, sx), (_b, y, sy) = structs[i], structs[j]
        if min(len(x), len(y)) <= 5:
            continue
        a = R.tm_align(x, y, sx, sy, order="seq", quantize=False)
        b = R.tm_align(x, y, sx, sy, order="kernel", quantize=False)
        assert np.array_equal(a["invmap"], b["invmap"]) and a["n_ali8"] == b["n_ali8"], (structs[i][0], structs[j][0])
        assert abs(a["qtm"] - b["qtm"]) <= 1e-9 and abs(a["ttm"] - b["ttm"]) <= 1e-9


def test_inputs_are_the_pdb_text_values_and_outputs_are_printed_values():
    c = np.array([[1.23456, -0.0004, 2.0005], [10.9999, 3.5, -7.12345]], np.float32)
    assert np.array_equal(tm.pdb_values(c), np.array([[float("%8.3f" % v) for v in row] for row in c]))
    assert tm.printed_values(0.123456, 0.99999951, 1.004999, 10, 3) == \
        {"len_ali": 10, "rmsd": 1.0, "seq_id": 0.3, "qtm": 0.12346, "ttm": 1.0}
    text = ("Aligned length=  %d, RMSD= %6.2f, Seq_ID=n_identical/n_aligned= %4.3f\n" % (10, 1.004999, 0.3) +
            "TM-score= %.5f (if normalized by length of Chain_1)\nTM-score= %.5f (if normalized by length of Chain_2)\n"
            % (0.123456, 0.99999951))
    assert tm.extract_tmalign_values(text) == tm.printed_values(0.123456, 0.99999951, 1.004999, 10, 3)


def test_backend_option_is_checked():
    tm.check_backend("auto", "cpu")
    tm.check_backend("hip", "cuda:0")
    with pytest.raises(ValueError):
        tm.check_backend("hip", "cpu")
    with pytest.raises(ValueError):
        tm.check_backend("binary", "cuda")


def _oracle_cli(tmp_path, monkeypatch):
    from oracle_engine import oracle_network
    from merizo_search_amd import cli
    from merizo_search_amd.foldclass import dbsearch as ds, makedb
    net = oracle_network()
    monkeypatch.setattr(ds, "network_setup", lambda **kw: (net, "cpu"))
    monkeypatch.setattr(makedb, "network_setup", lambda **kw: (net, "cpu"))
    monkeypatch.delenv("MERIZO_TMALIGN", raising=False)
    monkeypatch.setenv("PATH", os.path.dirname(os.__file__))       # no TM-align binary anywhere
    return cli


def test_cli_auto_backend_without_a_binary_writes_the_embedding_only_bytes(tmp_path, monkeypatch):
    import md_case
    cli = _oracle_cli(tmp_path, monkeypatch)
    qpdb, dbdir = md_case.write_inputs(tmp_path)
    cli.main(["createdb", dbdir, str(tmp_path / "db"), "--layout", "faiss"])
    base = ["easy-search", qpdb, str(tmp_path / "db"), None, str(tmp_path / "tmp"), "-k", "3", "-s", "0.1", "--output_headers",
            "--report_insignificant_hits", "--chopping", md_case.CHOPPING]
    cli.main([a if a is not None else str(tmp_path / "plain") for a in base])
    cli.main([a if a is not None else str(tmp_path / "auto") for a in base] + ["--tmalign_backend", "auto"])
    for suffix in ("_search.tsv", "_search_insignificant.tsv"):
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "auto") + suffix, "rb").read()
    assert "q_tm" not in open(str(tmp_path / "auto") + "_search.tsv").readline()


def test_cli_hip_backend_on_a_cpu_device_is_refused(tmp_path, monkeypatch):
    import md_case
    cli = _oracle_cli(tmp_path, monkeypatch)
    qpdb, _dbdir = md_case.write_inputs(tmp_path)
    with pytest.raises(SystemExit) as exc:
        cli.main(["easy-search", qpdb, str(tmp_path / "db"), str(tmp_path / "o"), str(tmp_path / "tmp"), "-d", "cpu",
                  "--tmalign_backend", "hip", "--chopping", md_case.CHOPPING])
    assert exc.value.code not in (0, None)
    with pytest.raises(SystemExit):                                 # argparse refuses other names
        cli.main(["search", qpdb, str(tmp_path / "db"), str(tmp_path / "o"), str(tmp_path / "tmp"), "--tmalign_backend", "x"])



# ------------------------------------------------------------------ the superposition against an SVD ------------------------
def _svd_kabsch(a, b):
    """fp64 SVD Kabsch with the determinant correction: the proper rotation u and t minimising |u a + t - b|; also the
    singular values of the covariance and the RMSD."""
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    h = (a - ca).T @ (b - cb)
    w, sv, vt = np.linalg.svd(h)
    dfix = np.diag([1.0, 1.0, np.sign(np.linalg.det(vt.T @ w.T)) or 1.0])
    u = vt.T @ dfix @ w.T
    t = cb - u @ ca
    return t, u, sv, _rmsd(a, b, t, u)


def _rmsd(a, b, t, u):
    return float(np.sqrt(((a @ u.T + t - b) ** 2).sum(axis=1).mean()))


def _assert_superposition(a, b, determined=True):
    t, u = R.kabsch(a, b)
    assert abs(np.linalg.det(u) - 1.0) < 1e-12 and np.abs(u @ u.T - np.eye(3)).max() < 1e-12
    t_s, u_s, sv, r_s = _svd_kabsch(a, b)
    r = _rmsd(a, b, t, u)
    assert abs(r - r_s) <= max(1e-9 * r_s, 1e-12 * max(1.0, np.abs(b).max())), (r, r_s)
    if determined:           # a clear gap between the two smallest singular values (after the sign fix): u is unique
        assert np.abs(u - u_s).max() < 1e-9 and np.abs(t - t_s).max() < 1e-9 * max(1.0, np.abs(b).max()), (u, u_s)
    return t, u


def _rotation(seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


@pytest.mark.parametrize("n", [3, 4, 7, 64, 65, 500])
def test_superposition_is_the_svd_optimum_on_random_clouds(n):
    rng = np.random.default_rng(n)
    for k in range(5):
        a = rng.normal(0, 10, (n, 3))
        _assert_superposition(a, rng.normal(0, 10, (n, 3)) + rng.uniform(-50, 50, 3), determined=n > 3)
        rot, shift = _rotation(100 * n + k), rng.uniform(-50, 50, 3)
        t, u = _assert_superposition(a, a @ rot.T + shift)         # a rigid copy: R and t come back exactly
        assert np.abs(u - rot).max() < 1e-12 and np.abs(t - shift).max() < 1e-12 * 100


def test_superposition_of_a_mirror_image_is_a_proper_rotation():
    for seed in range(4):
        a = tm_case.walk(40, 50 + seed)
        for mirror in (np.diag([1.0, 1.0, -1.0]), -np.eye(3)):
            b = a @ mirror.T @ _rotation(seed).T
            _t, u = _assert_superposition(a, b, determined=False)
            assert _rmsd(a, b, _t, u) > 1.0                       # no rotation undoes a reflection of a 3-d chain


def test_superposition_of_degenerate_sets():
    line = np.outer(np.arange(10.0), [3.8, 0.0, 0.0]) + np.array([1.0, 2.0, 3.0])
    plane = np.array([[3.3 * i, 1.9 * (i % 2), 0.0] for i in range(12)])
    point = np.tile([[5.0, -1.0, 2.0]], (8, 1))
    rot = _rotation(7)
    for a in (line, plane):            # coplanar / collinear: the rotation about the line / normal is not determined
        _assert_superposition(a, a @ rot.T + 4.0, determined=False)
        assert _rmsd(a, a @ rot.T + 4.0, *R.kabsch(a, a @ rot.T + 4.0)) < 1e-12
    _assert_superposition(plane, plane @ rot.T + np.array([0.0, 0.0, 1.0]), determined=True)
    _assert_superposition(point, point + 1.0, determined=False)
    t, u = R.kabsch(point, point @ rot.T)
    assert _rmsd(point, point @ rot.T, t, u) < 1e-12
    tri = np.array([[0.0, 0.0, 0.0], [3.8, 0.0, 0.0], [1.0, 3.5, 0.0]])
    _assert_superposition(tri, tri @ rot.T - 2.0, determined=True)
    t, u = R.kabsch(tri[:0], tri[:0])                               # n = 0: the identity
    assert np.array_equal(u, np.eye(3)) and np.array_equal(t, np.zeros(3))


def test_superposition_far_from_the_origin():
    rng = np.random.default_rng(3)
    a = tm_case.walk(60, 3) + 1e4
    rot = _rotation(11)
    for b in (a @ rot.T - 2e4, tm_case.noisy(a, 1.0, 4) @ rot.T + rng.uniform(-1e4, 1e4, 3)):
        _assert_superposition(a, b)


# ------------------------------------------------------------------ non-finite coordinates ---------------------------------
def test_restatement_ends_on_nan_and_inf_coordinates():
    """NaN / inf make every distance NaN: the relaxation loops of score_fun8 / get_score_fast must still end (a child
    process, so that a regression fails instead of hanging the suite)."""
    import subprocess
    import sys
    code = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import tm_case, tmalign_ref as R
x = tm_case.walk(40, 1)
for bad in (np.nan, np.inf, -np.inf):
    for where in ((3, 1), (0, 0), (39, 2)):
        y = tm_case.noisy(x, 1.0, 2)
        y[where] = bad
        for fast in (False, True):
            for a, b in ((x, y), (y, x), (y, y)):
                r = R.tm_align(a, b, fast=fast, order="kernel", quantize=False)
                assert len(r["invmap"]) == len(b)
z = np.full((12, 3), np.nan)
R.tm_align(z, x, quantize=False)
R.tm_align(x, z, fast=True, quantize=False)
print("ended")
''' % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    R.load()
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ended" in out.stdout, out.stderr[-2000:]


def test_tmalign_batch_refuses_non_finite_coordinates_before_the_device():
    from merizo_search_amd import ops
    from merizo_search_amd._lib import MerizoHipError
    x = tm_case.walk(30, 1)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 2] = bad
        with pytest.raises(MerizoHipError, match="structure 1 has a non-finite coordinate"):
            ops.tmalign_batch([x, y], ["A" * 30] * 2, [(0, 0)], device="cuda:0")


def test_align_many_leaves_non_finite_items_unaligned(monkeypatch):
    from merizo_search_amd import ops
    x = tm_case.walk(30, 1)
    nan, inf = x.copy(), x.copy()
    nan[3, 0] = np.nan
    inf[5, 1] = np.inf
    big = x.copy()
    big[0, 0] = 1e39                                   # finite in fp64, inf after the fp32 cast of the PDB path
    s = "A" * 30

    def no_device(*a, **k):
        raise AssertionError("a batch of only non-finite items reached ops.tmalign_batch")
    monkeypatch.setattr(ops, "tmalign_batch", no_device)
    assert tm.align_many([(nan, s, x, s), (x, s, inf, s), (big, s, big, s)], device="cuda:0") == [None, None, None]
    seen = {}

    def fake(structs, seqs, pairs, fast=False, device=None):
        seen["structs"], seen["pairs"] = structs, list(pairs)
        n = len(pairs)
        return {"qtm": np.full(n, 0.5), "ttm": np.arange(n) / 10.0, "rmsd": np.ones(n), "n_ali8": np.full(n, 20),
                "n_identical": np.full(n, 4), "status": np.zeros(n, np.int32)}
    monkeypatch.setattr(ops, "tmalign_batch", fake)
    got = tm.align_many([(nan, s, x, s), (x, s, x, s), (x, s, inf, s), (x, s, big, s), (x, s, x[:20], s[:20])], device="cuda:0")
    assert got[0] is None and got[2] is None and got[3] is None
    assert got[1]["ttm"] == 0.0 and got[4]["ttm"] == 0.1 and got[4]["len_ali"] == 20
    assert all(np.isfinite(c).all() for c in seen["structs"]) and len(seen["pairs"]) == 2


# ------------------------------------------------------------------ C entry points without a GPU ---------------------------
def test_tmalign_workspace_bytes_and_host_refusals():
    """ms_tmalign_workspace_bytes on invalid arguments, and ms_tmalign_batch's argument checks, which run on the host
    before any HIP call."""
    import ctypes
    from merizo_search_amd import _lib
    lib = _lib.load()
    wsb = lib.ms_tmalign_workspace_bytes
    for args in ((0, 10, 1), (10, 0, 1), (10, 10, 0), (-1, 10, 1), (2001, 10, 1), (10, 2001, 1), (10, 10, -5)):
        assert wsb(*args) == 0, args
    assert lib.ms_tmalign_max_len() == _lib.TMALIGN_MAX_LEN == 2000
    for x, y in ((6, 6), (64, 65), (2000, 2000), (150, 7)):
        one, two, three = wsb(x, y, 1), wsb(x, y, 2), wsb(x, y, 3)
        per = two - one
        assert per > 0 and three - two == per and per >= ((x + 63) // 64) * (y + 63) * 64, (x, y)
    assert wsb(150, 150, 10 ** 6) == wsb(150, 150, 2048)              # at most 2,048 slots
    assert wsb(2000, 2000, 10 ** 6) - wsb(2000, 2000, 1) <= (2 << 30)   # and at most 2 GiB of them
    p = ctypes.c_void_p(256)
    need = wsb(50, 50, 1)

    def call(xyz=p, npairs=1, max1=50, max2=50, flags=0, ws_bytes=need, out_i=p):
        return lib.ms_tmalign_batch(xyz, p, p, 2, p, npairs, max1, max2, flags, p, ws_bytes, p, out_i, None, None)
    for kw, code, msg in (({"xyz": None}, -1, b"NULL argument"), ({"out_i": None}, -1, b"NULL argument"),
                          ({"npairs": 0}, -1, b"npairs < 1"), ({"max1": 0}, -1, b"must be >= 1"),
                          ({"flags": 2}, -1, b"unknown flags 0x2"), ({"flags": -1}, -1, b"unknown flags"),
                          ({"max2": 2001}, -4, b"up to 2000 residues"), ({"max1": 2001}, -4, b"2001 x 50"),
                          ({"ws_bytes": need - 1}, -2, b"workspace of %d bytes, need at least %d" % (need - 1, need))):
        assert call(**kw) == code, kw
        assert msg in lib.ms_last_error(), (kw, lib.ms_last_error())
