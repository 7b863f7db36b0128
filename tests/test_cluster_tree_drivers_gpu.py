"""`cluster --cluster_mode connected --levels` on the GPU, end to end on the planted chains and dumbbells (faiss layout): every level
file is, byte for byte, the `_cluster.tsv` of a separate run of the command at that --mincos; the same at -k 4 --complete; the default
file is the one a run without --levels writes; the tree file holds n - 50 edges in the forest's order."""
import os

import numpy as np
import pytest

import cluster_components_case as cpc

pytestmark = pytest.mark.gpu

LEVELS = ("0.76", "0.8", "0.85")


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_tree_gpu"))
    names, _lengths, _group = cpc.write_chains(work)
    return work, names


def _cli(work, out, mincos, *extra):
    from merizo_search_amd import cli
    cli.cluster([os.path.join(work, "cfa"), out, os.path.join(work, "t"), "-s", mincos, "-c", "0.7", "--output_headers", "--cluster_mode",
                 "connected"] + list(extra))
    return open(out + "_cluster.tsv", "rb").read()


def test_cli_levels_write_the_files_of_separate_runs(chains, tmp_path):
    work, names = chains
    plain = _cli(work, str(tmp_path / "plain"), "0.7", "-k", "40")
    separate = {level: _cli(work, str(tmp_path / ("at" + level)), level, "-k", "40") for level in LEVELS}
    counts = lambda text: len({line.split(b"\t")[0] for line in text.splitlines()[1:]})
    assert counts(plain) == 50 and counts(separate["0.85"]) == 344
    assert 50 <= counts(separate["0.76"]) <= counts(separate["0.8"]) <= 344
    trees = []
    for name, flags in (("tree", ("-k", "40")), ("tree4", ("-k", "4", "--complete"))):
        out = str(tmp_path / name)
        assert _cli(work, out, "0.7", "--levels", ",".join(LEVELS), *flags) == plain
        for level in LEVELS:
            assert open("%s_cluster_%s.tsv" % (out, level), "rb").read() == separate[level], (name, level)
        lines = open(out + "_cluster_tree.tsv").read().splitlines()
        assert lines[0] == "member_a\tmember_b\tlink_score" and len(lines) == 1 + cpc.ROWS - 50
        row = {nm: r for r, nm in enumerate(names)}
        edges = [(np.float32(w), row[a], row[b]) for a, b, w in (line.split("\t") for line in lines[1:])]
        assert all(a < b for _w, a, b in edges) and edges == sorted(edges, key=lambda e: (-float(e[0]), e[1], e[2]))
        trees.append({(a, b) for _w, a, b in edges})
    assert trees[0] == trees[1]                                            # (the edge pass may score a pair in other last bits: the pairs)
    assert not os.path.exists(str(tmp_path / "plain_cluster_tree.tsv"))


def test_driver_reports_the_tree_and_its_span(chains, tmp_path):
    from merizo_search_amd.foldclass import cluster
    work = chains[0]
    times = {}
    _rep, _link, info = cluster.run_cluster(os.path.join(work, "cfa"), str(tmp_path / "r"), str(tmp_path / "t"), "cuda", topk=4, mincos=cpc.MINCOS,
                                            mincov=0.7, complete=True, mode="connected", timings=times, levels=["0.85"])
    assert info["n_components"] == 50 and info["tree_edges"] == cpc.ROWS - 50 and info["levels"] == {"0.85": 344}
    assert 1 <= info["tree_rounds"] <= 9 and times["tree_ms"] > 0.0 and times["cluster_ms"] > 0.0       # floor(log2 444) + 1 = 9
