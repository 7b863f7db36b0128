"""`cluster --cluster_mode connected` on the GPU, end to end on the planted chains and dumbbells in both layouts: with and without
--complete the command writes, byte for byte, the TSV the driver writes on the CPU oracle engine (the restatement behind it)."""
import os

import pytest

import cluster_components_case as cpc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_components_gpu"))
    cpc.write_chains(work)
    return work


def _oracle(work, db, out, **kw):
    from merizo_search_amd.foldclass import cluster
    Engine = cpc.install_oracle_components()
    info = cluster.run_cluster(os.path.join(work, db), out, os.path.join(work, "t"), "cuda", mincos=cpc.MINCOS, mincov=0.7, header=True,
                               engine=Engine(), mode="connected", **kw)[2]
    return open(out + "_cluster.tsv", "rb").read(), info


def _cli(work, db, out, *extra):
    from merizo_search_amd import cli
    cli.cluster([os.path.join(work, db), out, os.path.join(work, "t"), "-s", str(cpc.MINCOS), "-c", "0.7", "--output_headers", "--cluster_mode",
                 "connected"] + list(extra))
    return open(out + "_cluster.tsv", "rb").read()


@pytest.mark.parametrize("layout", ["cfa", "cpt"])
def test_cli_connected_writes_the_oracle_engines_tsv(chains, tmp_path, layout):
    want_cut, info_cut = _oracle(chains, layout, str(tmp_path / "o_cut"), topk=4)
    want_full, info_full = _oracle(chains, layout, str(tmp_path / "o_full"), topk=4, complete=True)
    assert info_cut["n_components"] == cpc.SPLIT_AT_K4 and info_full["n_components"] == cpc.GROUPS and want_cut != want_full
    assert want_full.splitlines()[0] == b"representative\tmember\tlink_score" and want_full.count(b"\n") == cpc.ROWS + 1
    assert _cli(chains, layout, str(tmp_path / "cut"), "-k", "4") == want_cut
    assert _cli(chains, layout, str(tmp_path / "full"), "-k", "4", "--complete") == want_full
    assert _cli(chains, layout, str(tmp_path / "k40"), "-k", "40") == want_full
    assert _cli(chains, layout, str(tmp_path / "full37"), "-k", "4", "--complete", "--query_batchsize", "37") == want_full


def test_driver_reports_components_largest_and_the_cluster_span(chains, tmp_path):
    from merizo_search_amd.foldclass import cluster
    times = {}
    rep, link, info = cluster.run_cluster(os.path.join(chains, "cfa"), str(tmp_path / "r"), str(tmp_path / "t"), "cuda", topk=4, mincos=cpc.MINCOS,
                                          mincov=0.7, complete=True, mode="connected", timings=times)
    assert info["mode"] == "connected" and info["n_components"] == cpc.GROUPS and info["largest"] == cpc.LARGEST and info["singletons"] == 8
    assert info["full_lists"] == 120 and info["edges"] == 1320 and 1 <= info["rounds"] <= cpc.ROWS and times["cluster_ms"] > 0.0
    assert (link == 1.0).sum() == cpc.GROUPS and len(set(rep.tolist())) == cpc.GROUPS
