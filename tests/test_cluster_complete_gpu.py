"""`cluster --complete` on the GPU, end to end on the two planted databases in both layouts: -k 4 --complete writes the TSV of
-k 20 byte for byte (families have at most 12 members: no list is full at 20), which is not the TSV of -k 4 alone; the same file
through the buffer's growth path, batches of 37 and a streamed target; and the numbers the driver reports."""
import os

import numpy as np
import pytest

import cluster_case as cc
import cluster_complete_case as ccc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_complete_gpu"))
    names, lengths, family = cc.write_planted(work)
    _names2, lengths2, family2 = ccc.write_split(work)
    assert np.array_equal(family, family2)
    want = {"": ccc.expected_counts(lengths, family, 4, 0.7), "2": ccc.expected_counts(lengths2, family, 4, ccc.SPLIT_MINCOV)}
    assert want["2"]["full_lists"] > want["2"]["saturated"]                # the old warning under-counts on the {50, 100} lengths
    return work, want


def _cli(db, out, tmp_path, *extra):
    from merizo_search_amd import cli
    cli.cluster([db, out, str(tmp_path / "t"), "-s", str(cc.PLANTED_MINCOS), "-c", "0.7", "--output_headers"] + list(extra))
    return open(out + "_cluster.tsv", "rb").read()


@pytest.mark.parametrize("which", ["", "2"])
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_cli_complete_at_k4_writes_the_k20_tsv(planted, tmp_path, monkeypatch, layout, which):
    from merizo_search_amd.foldclass import cluster
    from merizo_search_amd.foldclass.engine import HipEngine
    work, want = planted
    db = os.path.join(work, layout + which)
    full = _cli(db, str(tmp_path / "k20"), tmp_path, "-k", "20")
    assert full.count(b"\n") == 501
    assert _cli(db, str(tmp_path / "k4c"), tmp_path, "-k", "4", "--complete") == full
    assert _cli(db, str(tmp_path / "k4"), tmp_path, "-k", "4") != full
    assert _cli(db, str(tmp_path / "k4c37"), tmp_path, "-k", "4", "--complete", "--query_batchsize", "37") == full
    # the growth path: a buffer of 64 entries to begin with -- and what the driver reports
    times = {}
    _rep, _score, info = cluster.run_cluster(db, str(tmp_path / "room"), str(tmp_path / "t"), "cuda", topk=4, mincos=cc.PLANTED_MINCOS,
                                             mincov=0.7, header=True, complete=True, edge_room=64, timings=times)
    assert open(str(tmp_path / "room_cluster.tsv"), "rb").read() == full
    assert {key: info[key] for key in want[which]} == want[which] and info["complete"] is True
    assert info["edges"] <= info["rescored"] < 327 * 500 and times["edges_ms"] > 0.0 and times["edges_calls"] == 1
    if layout == "fa":                                                  # a streamed target: blocks of 97 rows, queries from the file
        monkeypatch.setattr(HipEngine, "resident_budget", lambda self, nq=0, k=0: 1 << 10)
        times = {}
        cluster.run_cluster(db, str(tmp_path / "stream"), str(tmp_path / "t"), "cuda", topk=4, mincos=cc.PLANTED_MINCOS, mincov=0.7,
                            header=True, complete=True, query_batchsize=120, search_batchsize=97, timings=times)
        assert times["streamed"] is True and open(str(tmp_path / "stream_cluster.tsv"), "rb").read() == full


def test_cli_refuses_more_edges_than_max_edges_and_writes_nothing(planted, tmp_path, caplog):
    from merizo_search_amd import cli
    work, want = planted
    out = str(tmp_path / "refused")
    with pytest.raises(SystemExit) as exc:
        cli.cluster([os.path.join(work, "fa"), out, str(tmp_path / "t"), "-s", str(cc.PLANTED_MINCOS), "-k", "4", "--complete", "--max_edges", "100"])
    assert exc.value.code == 1 and "have %d neighbours" % want[""]["edges"] in caplog.text and "--max_edges 100" in caplog.text
    assert not os.path.exists(out + "_cluster.tsv")
