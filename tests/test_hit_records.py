"""dbsearch.hit_records -- the one step from top-k lists to the hit records write_search_results prints -- through its drivers,
without a GPU (oracle engine, md_case's stand-in aligner): the files of a db-search and the dicts of a `search` in both
database layouts equal the ones recorded before the two layouts shared that step (tests/golden/hit_records/, made by
hit_records_case.record), whatever the query batch size, and the GPU aligner's branch drops exactly the pairs it refuses."""
import ast
import json
import logging
import os

import pytest

import hit_records_case as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hit_records")
TSVS = hc.SUFFIXES[:2]


def golden(name: str) -> bytes:
    with open(os.path.join(GOLDEN, name), "rb") as handle:
        return handle.read()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    import md_case
    path = str(tmp_path_factory.mktemp("hit_records"))
    hc.write_database(path)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MERIZO_TMALIGN", md_case.fake_tmalign(path))
        yield path


@pytest.fixture()
def stub_aligner(monkeypatch):
    from merizo_search_amd.foldclass import tmalign
    monkeypatch.setattr(tmalign, "align_many", hc.align_many_stub)


def body(data: bytes):
    """The rows of a TSV file without its header line, as lists of columns."""
    return [line.split("\t") for line in data.decode().splitlines()[1:]]


@pytest.mark.parametrize("layout", hc.LAYOUTS)
def test_db_search_files_equal_the_recorded_ones(layout, work):
    got = hc.db_search(work, layout, os.path.join(work, "bin_" + layout))
    for suffix in hc.SUFFIXES:
        assert got[suffix] == golden(layout + suffix), (layout, suffix)
    reported, below = body(got[TSVS[0]]), body(got[TSVS[1]])
    assert reported and below                                               # both branches of the mintm rule are populated
    if layout == "fa":      # hits below mintm: ONE counter over the run (the reported ones: dense per query)
        assert [int(r[1]) for r in below] == list(range(len(below))) and len({r[0] for r in below}) > 1
    else:                   # ranks in both files: a query's keys are 0..3 between them, each file alone has gaps
        assert max(int(r[1]) for r in reported) == max(int(r[1]) for r in below) == 3
        assert len({(r[0], r[1]) for r in reported + below}) == len(reported + below)
    skipped = hc.db_search(work, layout, os.path.join(work, "skip_" + layout), skip=True)
    for suffix in hc.SUFFIXES:
        assert skipped[suffix] == golden(layout + "_skip" + suffix), (layout, suffix)


def without_refused(layout, files):
    """The binary run's `files` as the stub GPU aligner's run must write them: the hits with a target of REFUSED_LEN residues gone,
    the keys that are counters (faiss layout) counted without them -> (files, the (query, target) of the removed hits)."""
    out, removed = {}, []
    for suffix in TSVS:
        lines = files[suffix].decode().splitlines()
        kept, counters = [lines[0]], {}
        for line in lines[1:]:
            cols = line.split("\t")
            if int(cols[5]) == hc.REFUSED_LEN:
                removed.append((cols[0], cols[2]))
                continue
            if layout == "fa":
                counter = cols[0] if suffix == TSVS[0] else None          # dense per query | one counter over the run
                cols[1] = str(counters.get(counter, 0))
                counters[counter] = counters.get(counter, 0) + 1
            kept.append("\t".join(cols))
        out[suffix] = ("\n".join(kept) + "\n").encode()
        metadata = [ast.literal_eval(line.split("\t")[-1]) for line in kept[1:] if line.split("\t")[-1] != "{ }"]
        out[suffix + ".hit_metadata.json"] = json.dumps(metadata).encode()
    return out, removed


@pytest.mark.parametrize("layout", hc.LAYOUTS)
def test_gpu_aligner_branch_drops_exactly_the_refused_pairs(layout, work, stub_aligner, caplog):
    """tmalign_backend 'hip' with align_many replaced by the stand-in's rule, None for every target of REFUSED_LEN residues: the
    binary run's files without those hits, one `_refused` warning per removed hit -- in both layouts (as before the layouts shared
    the step: recorded with this test there).  No reported hit has that length here (the stand-in reports equal lengths only,
    nearly all of them 60), so the removals are in the file of the hits below mintm, the faiss layout's run-wide counter."""
    want, removed = without_refused(layout, {suffix: golden(layout + suffix) for suffix in hc.SUFFIXES})
    assert len(removed) >= 3
    with caplog.at_level(logging.WARNING, logger="merizo_search_amd.foldclass.dbsearch"):
        got = hc.db_search(work, layout, os.path.join(work, "hip_" + layout), backend="hip")
    assert got == want
    warnings = [r.getMessage() for r in caplog.records if r.getMessage().startswith("TM-align refuses ")]
    for query, target in removed:
        stored = target + (".pdb" if layout == "pt" else "")
        assert sum(m.startswith("TM-align refuses %s x %s (" % (query, stored)) for m in warnings) == 1, (query, target)


@pytest.mark.parametrize("layout", hc.LAYOUTS)
def test_db_search_files_do_not_depend_on_the_query_batch_size(layout, work, stub_aligner):
    """50 queries in one batch and in batches of 17: the faiss layout's counter of hits below mintm is carried from batch to batch
    (refused pairs not counted), the `.pt` layout's keys are ranks and carry nothing.  (The stub aligner: no processes.)"""
    for tag, kw in (("hip", dict(backend="hip")), ("skip", dict(skip=True))):
        one = hc.db_search(work, layout, os.path.join(work, "b64_%s_%s" % (tag, layout)), batch=64, **kw)
        several = hc.db_search(work, layout, os.path.join(work, "b17_%s_%s" % (tag, layout)), batch=17, **kw)
        assert one == several and len(body(one[TSVS[0]])) > 0, (layout, tag)
        assert tag == "skip" or len(body(one[TSVS[1]])) > 0


def test_coverage_rule_drops_a_hit_of_the_pt_layout_only(work, stub_aligner):
    """hit_records on one hand-built list: a short query, a target more than 1 / mincov times as long.  (The drivers never hand
    the `.pt` layout such a pair while the aligner aligns min(q_len, t_len) residues, as the stand-in does: the scan's length mask
    has zeroed its score.  So the db-search case above drops no hit by this rule -- its `.pt` files are shorter by the mask.)"""
    import numpy as np
    from merizo_search_amd.foldclass import dbsearch as ds
    from merizo_search_amd.foldclass.dbrecords import Records
    D, I = np.array([[0.9, 0.8, 0.7, -np.inf]], np.float32), np.array([[0, 0, 0, -1]], np.int64)
    for layout in hc.LAYOUTS:
        rec = Records(os.path.join(work, layout))
        lengths = rec.lengths()
        short, long_ = int(np.argmin(lengths)), int(np.argmax(lengths))
        assert lengths[short] < 0.7 * lengths[long_]
        I[0, :3] = [long_, short, long_]
        query = {"name": "q", "seq": rec.seqs([short])[0], "coords": rec.coords([short])[0]}
        kw = dict(mincos=0.0, mintm=0.5, fastmode=False, skip_tmalign=False, tmalign_backend="hip", tmp=work, aligner_device="cpu")
        with_rule = ds.hit_records([query], D, I, rec, layout == "fa", mincov=0.7, **kw)
        without = ds.hit_records([query], D, I, rec, layout == "fa", mincov=0.0, **kw)
        rec.close()
        keys = lambda pair: [list(side[0]) for side in pair]
        if layout == "fa":                                                  # no such rule: the long target is below mintm, twice
            assert keys(with_rule) == keys(without) == [[0], [0, 1]]
        else:                                                               # ranks 0 and 2 dropped from both dicts
            assert keys(with_rule) == [[1], []] and keys(without) == [[1], [0, 2]]


@pytest.mark.parametrize("layout", hc.LAYOUTS)
def test_search_result_dicts_equal_the_recorded_ones(layout, work):
    results, all_results = hc.search(work, layout)
    assert hc.as_json(results).encode() == golden(layout + "_search.json")
    assert hc.as_json(all_results).encode() == golden(layout + "_search_all.json")
    assert len(results) == len(all_results) == len(hc.QUERY_ROWS) and any(results) and any(all_results)
    for per_query, below in zip(results, all_results):
        assert all(type(key) is int and type(hit["dbindex"]) is int for d in (per_query, below) for key, hit in d.items())
        if layout == "fa":                                                  # dense per query; below mintm: one counter over the call
            assert list(per_query) == list(range(len(per_query)))
        else:                                                               # ranks: each one in at most one of the two dicts
            assert sorted(list(per_query) + list(below)) == sorted(set(per_query) | set(below)) and all(0 <= k < 6 for k in list(per_query) + list(below))
    below_keys = [key for below in all_results for key in below]
    if layout == "fa":
        assert below_keys == list(range(len(below_keys)))
        return
    assert any(list(d) != list(range(len(d))) for d in results + all_results)      # ranks leave gaps where the other dict has the hit
    # dbsearch(), one query per call (the reference's function): the same dicts
    from oracle_engine import oracle_network
    from merizo_search_amd.foldclass import dbsearch as ds
    net = oracle_network(0)
    target = ds.read_database(os.path.join(work, "pt"), engine=net.engine)
    for q, query in enumerate(hc.search_queries(work)):
        one = ds.dbsearch(query, target, os.path.join(work, "tmp"), net, topk=6, mincov=0.7, mincos=0.0, mintm=0.5, fastmode=False,
                          inputs_are_ca=True)
        assert one == (results[q], all_results[q])
