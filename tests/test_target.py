"""target.Target -- one rank's rows of a target database on the device, or streamed -- on the CPU with the oracle engine over the
planted databases of test_md_scan_host.py in both layouts: what is cached and when, that resident and streamed rows give the same
bits through topk / rows_for / blocks, and multidomain.equal_runs against a plain restatement.  One gpu test: the `.pt` rows are
normalised once (the oracle engine's cosine_rows is the identity and cannot show it)."""
import collections
import os

import numpy as np
import pytest
import torch

import multidom_case as mc
from oracle_engine import OracleEngine
from merizo_search_amd.foldclass import dbsearch as ds, multidomain as md
from merizo_search_amd.foldclass.dbquery import QueryDB
from merizo_search_amd.foldclass.target import Target, score_mode


class CountingEngine(OracleEngine):
    def __init__(self):
        super().__init__()
        self.calls = collections.Counter()

    def upload_rows(self, matrix, lo, hi):
        self.calls["upload_rows"] += 1
        return super().upload_rows(matrix, lo, hi)

    def cosine_rows(self, db):
        self.calls["cosine_rows"] += 1
        return super().cosine_rows(db)

    def resident_budget(self, nq=4096, k=64):
        self.calls["resident_budget"] += 1
        return super().resident_budget(nq, k)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("target"))
    names, _chain_of = mc.write_planted(work)
    return work, len(names)


def _bits(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. what is cached ---
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_of_builds_once_per_engine_and_rebuilds_for_another(planted, layout):
    work, n = planted
    target_db = ds.read_database(os.path.join(work, layout))
    engine = CountingEngine()
    first = Target.of(target_db, engine, 3, 4)
    assert Target.of(target_db, engine, 3, 4) is first and Target.cached(target_db, engine) is first
    made = {"fa": {"upload_rows": 1, "cosine_rows": 0}, "pt": {"upload_rows": 0, "cosine_rows": 1}}[layout]
    assert {key: engine.calls[key] for key in made} == made
    assert first.faiss == (layout == "fa") and (first.n, first.lo, first.hi) == (n, 0, n) and first.rows.shape == (n, 128)
    assert first.whole and not first.streamed and first.row_norm_bound is None and first.pf_image is None    # (no prefilter here)
    assert (first.lengths is None) == (layout == "fa")
    engine.budget = 0                                       # a cached resident shard is reused without asking the budget again
    asked = engine.calls["resident_budget"]
    assert Target.of(target_db, engine, 3, 4) is first and engine.calls["resident_budget"] == asked
    assert Target.of(target_db) is first                    # (engine None: the engine the rows are resident on)
    other = CountingEngine()
    second = Target.of(target_db, other, 3, 4)
    assert second is not first and second.engine is other and Target.cached(target_db, other) is second
    assert Target.cached(target_db, engine) is None and {key: other.calls[key] for key in made} == made
    assert np.array_equal(_bits(second.rows), _bits(first.rows))           # built from the file's rows again, all of them
    # the dict keeps the reference's keys as read_database set them, plus one private key
    assert sorted(k for k in target_db if not k.startswith("_")) == sorted(
        ["database", "faiss"] if layout == "fa" else ["database", "index", "lengths", "faiss", "mdfn", "mifn"])
    assert len([k for k in target_db if k.startswith("_")]) == 1


def test_a_faiss_shard_beyond_the_budget_is_streamed_and_nothing_is_cached(planted):
    work, n = planted
    target_db = ds.read_database(os.path.join(work, "fa"))
    engine = CountingEngine()
    engine.budget = 0
    streamed = Target.of(target_db, engine, 3, 4)
    assert streamed.streamed and not streamed.whole and streamed.rows is None and (streamed.lo, streamed.hi) == (0, n)
    assert Target.cached(target_db, engine) is None and [k for k in target_db if k.startswith("_")] == []
    assert engine.calls["upload_rows"] == 0 and engine.calls["resident_budget"] == 1
    assert Target.of(target_db, engine, 3, 4) is not streamed and engine.calls["resident_budget"] == 2      # asked again
    engine.budget = n * 128 * 4                             # exactly the shard's bytes: resident
    assert Target.of(target_db, engine, 3, 4).rows.shape == (n, 128) and Target.cached(target_db, engine) is not None
    engine.budget = 0                                       # another engine that has no room: the stale copy goes
    other = CountingEngine()
    other.budget = 0
    assert Target.of(target_db, other, 3, 4).streamed and [k for k in target_db if k.startswith("_")] == []


# ------------------------------------------------------------------ 2. the same bits, resident and streamed ---
@pytest.mark.parametrize("raw_queries", [True, False])
def test_topk_is_bit_equal_resident_and_streamed(planted, raw_queries):
    work, n = planted
    prefix = os.path.join(work, "fa")
    rng = np.random.default_rng(5)
    q = rng.standard_normal((3, 128)).astype(np.float32)
    if not raw_queries:
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    resident = Target.of(ds.read_database(prefix), CountingEngine(), 3, 4)
    engine = CountingEngine()
    engine.budget = 0
    streamed = Target.of(ds.read_database(prefix), engine, 3, 4)
    assert not resident.streamed and streamed.streamed
    s0, i0 = resident.topk(torch.from_numpy(q), 4, raw_queries=raw_queries, search_batchsize=3)
    s1, i1 = streamed.topk(torch.from_numpy(q), 4, raw_queries=raw_queries, search_batchsize=3)
    assert s0.shape == (3, 4) and i0.dtype == torch.int64 and torch.equal(i0, i1) and np.array_equal(_bits(s0), _bits(s1))
    assert (np.diff(s0.numpy(), axis=1) <= 0).all() and 0 <= int(i0.min()) and int(i0.max()) < n


def test_pt_topk_is_search_query_against_db(planted):
    work, n = planted
    target_db = ds.read_database(os.path.join(work, "pt"))
    engine = CountingEngine()
    rng = np.random.default_rng(6)
    q = torch.from_numpy(rng.standard_normal((3, 128)).astype(np.float32))
    seqs = ["A" * 30, "A" * 45, "A" * 60]
    got = ds.search_query_against_db({"embedding": q, "seq": seqs}, target_db, 0.7, 4, engine=engine)
    qlen = torch.tensor([30.0, 45.0, 60.0])
    s, i = Target.of(target_db, engine).topk(q, 4, qlen=qlen, mincov=0.7)
    assert torch.equal(got["indices"], i) and np.array_equal(_bits(got["scores"]), _bits(s)) and engine.calls["cosine_rows"] == 1
    s_ref, i_ref = engine.cosine_topk(target_db["database"].float(), q, 4, lengths=target_db["lengths"], qlen=qlen, mincov=0.7)
    assert torch.equal(i, i_ref) and np.array_equal(_bits(s), _bits(s_ref))


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_rows_for_in_place_and_compact_give_the_same_bits(planted, layout):
    work, n = planted
    prefix = os.path.join(work, layout)
    engine = CountingEngine()
    reader = QueryDB(prefix)
    rows = np.asarray([1, 2, 5], np.int64)
    whole = Target.of(ds.read_database(prefix), engine, 3, 4)
    assert whole.whole
    m0, l0, x0 = whole.rows_for(rows, reader)
    assert m0 is whole.rows and x0.tolist() == [1, 2, 5]
    m1, l1, x1 = md.compact_target_rows(engine, reader, rows)
    assert m1.shape == (3, 128) and x1.tolist() == [0, 1, 2]
    assert np.array_equal(_bits(m0[x0]), _bits(m1[x1]))
    if layout == "fa":
        assert l0 is None and l1 is None
        engine.budget = 0                                   # a streamed target takes the compact path itself
        m2, l2, x2 = Target.of(ds.read_database(prefix), engine, 3, 4).rows_for(rows, reader)
        assert l2 is None and x2.tolist() == [0, 1, 2] and np.array_equal(_bits(m2), _bits(m1))
    else:
        assert np.array_equal(_bits(l0[x0]), _bits(l1[x1])) and l1.tolist() == [float(len(s)) for s in reader.seqs(1, 3) + reader.seqs(5, 6)]
    reader.close()


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_blocks_cover_the_rows_exactly_once(planted, layout):
    work, n = planted
    prefix = os.path.join(work, layout)
    engine = CountingEngine()
    reader = QueryDB(prefix)
    target_db = ds.read_database(prefix)
    streamed = Target.for_reader(target_db, engine, reader)             # nothing is resident yet: streamed, and nothing uploaded
    assert streamed.streamed and (streamed.lo, streamed.hi) == (0, n) and engine.calls["upload_rows"] == 0
    assert Target.for_reader(None, engine, reader).streamed
    resident = Target.of(target_db, engine, 3, 4)
    assert Target.for_reader(target_db, engine, reader) is resident and Target.for_reader(target_db, CountingEngine(), reader).streamed
    one = list(resident.blocks(reader, 3))
    assert len(one) == 1 and one[0][0] is resident.rows and one[0][1] == 0 and one[0][2] is resident.lengths
    parts = list(streamed.blocks(reader, 3))
    assert [a for _b, a, _l in parts] == list(range(0, n, 3))
    assert [int(b.shape[0]) for b, _a, _l in parts] == [min(3, n - a) for a in range(0, n, 3)]
    assert np.array_equal(_bits(torch.cat([b for b, _a, _l in parts])), _bits(resident.rows))
    if layout == "fa":
        assert all(l is None for _b, _a, l in parts)
    else:
        assert np.array_equal(_bits(torch.cat([l for _b, _a, l in parts])), _bits(resident.lengths))
    reader.close()


def test_score_mode():
    assert score_mode(True, True) == ("ip_prenorm", False) and score_mode(True, False) == ("ip", False)
    assert score_mode(False, False) == ("cosine", True) and score_mode(False, True) == ("cosine", True)


# ------------------------------------------------------------------ 3. the run helper ---
def _runs_restated(keys):
    """A run starts at position 0 and wherever a key differs from the one before it; it ends where the next one starts."""
    starts = [p for p in range(len(keys)) if p == 0 or keys[p] != keys[p - 1]]
    return list(zip(starts, starts[1:] + [len(keys)]))


@pytest.mark.parametrize("keys", [[], ["a"], ["a", "a", "a", "a"], ["a", "b", "c", "d"], ["a", "a", "b", "a", "a", "a"],
                                  ["a", "b", "b", "c", "c", "c", "b"], [3, 3, 4, 6, 6], list("aabbbcddddde")])
def test_equal_runs_equals_the_restatement(keys):
    runs = md.equal_runs(keys)
    assert runs == _runs_restated(keys)
    assert [p for a, b in runs for p in range(a, b)] == list(range(len(keys)))      # every position in exactly one run, in order
    assert md.chain_runs(["%s_TED01" % k for k in keys]).tolist() == [a for a, _b in runs] + [len(keys)]


def test_equal_runs_shapes():
    assert md.equal_runs([]) == [] and md.equal_runs(["x"]) == [(0, 1)] and md.equal_runs(["x"] * 5) == [(0, 5)]
    assert md.equal_runs(list("abcd")) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert md.equal_runs(["a", "a", "b", "a"]) == [(0, 2), (2, 3), (3, 4)]          # an id that comes back: two runs


# ------------------------------------------------------------------ 4. normalised once, on the real engine ---
@pytest.mark.gpu
def test_pt_rows_are_normalised_once_and_stay_where_they_are(tmp_path):
    """64 synthetic rows written by createdb's writer: after Target.of the rows are the file's rows normalised ONCE on the device
    (eps 1e-8); a second Target.of and a search neither move nor change them."""
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import synthetic as syn
    from merizo_search_amd.foldclass.makedb import write_pt_db
    rng = np.random.default_rng(9)
    raw = (rng.standard_normal((64, 128)) * rng.uniform(0.5, 3.0, (64, 1))).astype(np.float32)
    lengths = rng.integers(20, 61, 64)
    prefix = str(tmp_path / "db")
    write_pt_db(prefix, raw, ["/x/d%02d.pdb" % r for r in range(64)], [syn.random_walk(int(l), 100 + r) for r, l in enumerate(lengths)],
                ["A" * int(l) for l in lengths])
    engine = ds.engine_setup("cuda:0")
    target_db = ds.read_database(prefix)
    first = Target.of(target_db, engine, 3, 4)
    ptr, bits = first.rows.data_ptr(), first.rows.cpu().numpy().view(np.uint32).copy()
    once = ops.l2_normalize_rows(torch.from_numpy(raw).cuda(), 1e-8).cpu().numpy()
    assert np.array_equal(bits, once.view(np.uint32)) and not np.array_equal(bits, raw.view(np.uint32))
    assert Target.of(target_db, engine, 3, 4) is first
    top = ds.search_query_against_db({"embedding": torch.from_numpy(raw[:3].copy()), "seq": ["A" * 40] * 3}, target_db, 0.0, 4, engine=engine)
    assert top["indices"][:, 0].tolist() == [0, 1, 2]
    again = Target.of(target_db, engine, 3, 4)
    assert again is first and again.rows.data_ptr() == ptr and np.array_equal(again.rows.cpu().numpy().view(np.uint32), bits)
    assert np.array_equal(target_db["database"].numpy().view(np.uint32), raw.view(np.uint32))       # the dict keeps the file's rows
