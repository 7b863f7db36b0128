"""`cluster --mintm` on the GPU, end to end on the planted structure families (about 230 alignments of chains of at most 80 residues
per run, one launch): the command and the driver in both layouts, greedy and connected, with and without --complete, in fast mode --
the TSV byte-equal to the one the numpy pipeline (cluster_tm_case.pipeline_graph_np: the restatements of the pair calls and of the
cluster calls, TM-scores from the CPU restatement of TM-align) derives from the graph the GPU search itself handed to
ms_cluster_pairs; `saturated` the count before the edit; and chains TM-align cannot score rejected with one warning."""
import logging
import os

import numpy as np
import pytest

import cluster_tm_case as ct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_tm_gpu"))
    names, built = ct.write_structured(work)
    return work, names, built


@pytest.fixture()
def graph_spy(monkeypatch):
    """What the driver hands to HipEngine.cluster_pairs, copied to the host BEFORE the lists are edited."""
    from merizo_search_amd.foldclass.engine import HipEngine
    seen = {}
    real = HipEngine.cluster_pairs

    def spy(self, nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score, mincov=0.0, cap=None):
        host = lambda t: None if t is None else t.cpu().numpy().copy()
        seen.update(graph=tuple(host(t) for t in (nbr_idx, nbr_score, edge_src, edge_dst, edge_score)), lengths=np.asarray(lengths).copy(),
                    cut=min_score, cov=mincov)
        return real(self, nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score, mincov, cap)

    monkeypatch.setattr(HipEngine, "cluster_pairs", spy)
    return seen


def _want_tsv(path, names, seen, tm_of, mode):
    """The file the numpy pipeline writes for the graph the spy saw -> (bytes, rep, info)."""
    from merizo_search_amd.foldclass import cluster
    rep, rep_score, tm_score, info = ct.pipeline_graph_np(*seen["graph"], seen["lengths"], tm_of, mode, ct.MINTM, seen["cut"], seen["cov"])
    cluster.write_cluster_tsv(path, names, rep, rep_score, True, "link_score" if mode == "connected" else "emb_score", tm_score)
    return open(path, "rb").read(), rep, info


@pytest.mark.parametrize("complete", [False, True])
@pytest.mark.parametrize("mode", ["greedy", "connected"])
@pytest.mark.parametrize("layout", ["sfa", "spt"])
def test_driver_writes_the_numpy_pipelines_file(families, graph_spy, tmp_path, layout, mode, complete):
    from merizo_search_amd.foldclass import cluster
    work, names, built = families
    out, timings = str(tmp_path / "got"), {}
    topk = 3 if complete else ct.K_ALL
    rep, _score, info = cluster.run_cluster(os.path.join(work, layout), out, str(tmp_path / "t"), "cuda", topk=topk, mincos=ct.MINCOS,
                                            mincov=ct.MINCOV, header=True, complete=complete, mode=mode, mintm=ct.MINTM, query_batchsize=37,
                                            timings=timings)
    want, want_rep, want_info = _want_tsv(str(tmp_path / "want.tsv"), names, graph_spy, lambda a, b: built["tm"][False][(a, b)], mode)
    assert open(out + "_cluster.tsv", "rb").read() == want
    assert np.array_equal(rep, want_rep) and np.array_equal(rep, built["rep"])
    for key, value in want_info.items():                                  # 'saturated': the lists as the search left them
        assert info[key] == value, key
    assert graph_spy["graph"][0].shape == (len(names), topk) and (graph_spy["graph"][2] is not None) == complete
    assert info["tm_unaligned_pairs"] == 0 and info["tm_rejected_pairs"] > 0 and (info["saturated"] > 0) == complete
    assert timings["tm_ms"] > 0.0 and timings["tm_calls"] == 1


@pytest.mark.parametrize("layout", ["sfa", "spt"])
def test_command_with_fastmode(families, graph_spy, tmp_path, layout):
    from merizo_search_amd import cli
    work, names, built = families
    out = str(tmp_path / "got")
    cli.cluster([os.path.join(work, layout), out, str(tmp_path / "t"), "-s", str(ct.MINCOS), "-k", str(ct.K_ALL), "-m", str(ct.MINTM), "-f",
                 "--output_headers"])
    want, want_rep, _info = _want_tsv(str(tmp_path / "want.tsv"), names, graph_spy, lambda a, b: built["tm"][True][(a, b)], "greedy")
    text = open(out + "_cluster.tsv", "rb").read()
    assert text == want and np.array_equal(want_rep, built["rep"])
    assert text.splitlines()[0] == b"representative\tmember\temb_score\ttm_score"


def test_chains_tm_align_cannot_score_are_rejected_with_one_warning(graph_spy, tmp_path, caplog):
    from merizo_search_amd.foldclass import cluster
    built = ct.structured()
    bad = int(np.nonzero(built["sfam"] == -1)[0][0])
    short = int(np.nonzero(built["sfam"] == 5)[0][0])
    edited = {}

    def edit(coords, seqs, _built):
        coords[bad][3, 1] = np.inf
        coords[short], seqs[short] = coords[short][:5].copy(), seqs[short][:5]
        edited.update(coords=coords, seqs=seqs)

    work = str(tmp_path / "db")
    names, _built = ct.write_structured(work, edit=edit)
    out = str(tmp_path / "got")
    with caplog.at_level(logging.WARNING):
        rep, _score, info = cluster.run_cluster(os.path.join(work, "sfa"), out, str(tmp_path / "t"), "cuda", topk=ct.K_ALL, mincos=ct.MINCOS,
                                                mincov=0.0, header=True, mintm=ct.MINTM)
    tm_of = lambda a, b: ct.printed_max_tm(edited["coords"][a], edited["seqs"][a], edited["coords"][b], edited["seqs"][b], False)
    want, want_rep, want_info = _want_tsv(str(tmp_path / "want.tsv"), names, graph_spy, tm_of, "greedy")
    assert open(out + "_cluster.tsv", "rb").read() == want and np.array_equal(rep, want_rep)
    assert info["tm_unaligned_pairs"] == want_info["tm_unaligned_pairs"] > 0 and info["tm_rejected_pairs"] == want_info["tm_rejected_pairs"]
    assert caplog.text.count("residues or fewer") == 1 and rep[bad] == bad and rep[short] == short and (rep == short).sum() == 1
