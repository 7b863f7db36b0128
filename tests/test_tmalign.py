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

