"""ms_threshold_edges on the GPU: the emitted set {(src, dst, score bits)} against ms_ip_topk at k = n on the GPU and against the
oracle's search at order=1 (the prepared queries, the chain of 128 fmaf), in the three modes; the cut on, one ulp above and
without one; NaN, inf and zero vectors; a row above the bound; a row offset beyond 2^32; excluded ranges; a list that drains many
times; and the cap rule with guard zones.  Sets are compared exactly: the filter only ever proves a cell BELOW the cut."""
import numpy as np
import pytest

import cluster_complete_case as ccc
from mq_filter_case import mode_code as _code, prepared as _prepared, to_gpu as _t

pytestmark = pytest.mark.gpu
NINF = -np.inf
BOUND = 1.0 + 1e-6                     # the row-norm bound of unit rows
MODES = ("prenorm", "normq", "unit")
CUT = 0.5


def _unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _case(n, nq, seed, scale=True):
    """Unit rows; queries that are noisy copies of rows (cosines on both sides of CUT) and random directions, raw (scaled)."""
    rng = np.random.default_rng(seed)
    db = _unit(rng.standard_normal((n, 128)))
    pick = rng.integers(0, n, size=nq)
    noise = rng.choice([0.0, 0.3, 0.9, 1.0, 1.1, 3.0], size=(nq, 1))
    q = _unit(db[pick] + noise * rng.standard_normal((nq, 128)) / np.sqrt(128.0))
    if scale:
        q = (q * rng.uniform(0.5, 2.0, size=(nq, 1))).astype(np.float32)
    return db, q


def _gpu(db, q, mode, min_score, bound=BOUND, lo=None, hi=None, row_offset=0, **kw):
    from merizo_search_amd import ops
    stats = {}
    src, dst, score, count = ops.threshold_edges(_t(db, np.float32), _t(q, np.float32), _code(mode), float(min_score), bound,
                                                 lo=lo, hi=hi, row_offset=row_offset, stats=stats, **kw)
    return src.cpu().numpy(), dst.cpu().numpy(), score.cpu().numpy(), count, stats["rescored"]


def _topk_set(db, q, mode, min_score, lo=None, hi=None, row_offset=0):
    """ms_ip_topk at k = n on the GPU, filtered."""
    from merizo_search_amd import ops
    s, i = ops.ip_topk(_t(db, np.float32), _t(q, np.float32), db.shape[0], mode=_code(mode), row_offset=row_offset)
    return ccc.edges_of_lists(s.cpu().numpy(), i.cpu().numpy(), min_score, lo, hi)


def _oracle_set(db, q, mode, min_score, lo=None, hi=None, row_offset=0):
    """The oracle's search at order=1 over the prepared queries at k = n, filtered."""
    from oracle import oracle as orc
    s, i = orc.ip_topk(db, _prepared(q, mode), db.shape[0], row_offset=row_offset, order=1)
    return ccc.edges_of_lists(s, i, min_score, lo, hi)


def _check(db, q, mode, min_score, oracle=True, **kw):
    src, dst, score, count, rescored = _gpu(db, q, mode, min_score, **kw)
    got = ccc.edge_set(src, dst, score)
    ref = {key: kw[key] for key in ("lo", "hi", "row_offset") if key in kw}
    want = _topk_set(db, q, mode, min_score, **ref)
    assert count == len(src) == len(got), "duplicates, or a count that is not the number of cells"
    assert got == want, (len(got), len(want), sorted(got - want)[:3], sorted(want - got)[:3])
    if oracle:
        assert got == _oracle_set(db, q, mode, min_score, **ref)
    assert rescored >= count
    return got, rescored


# ------------------------------------------------------------------ 1. shapes and modes ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_emitted_set_equals_ip_topk_at_k_n_and_the_oracle(n, mode):
    """n across the 64-row tile and several workgroups, nq across the 32-query tile and the four waves.  MS_MODE_IP_PRENORM gets
    scaled queries as they are, the other two normalise them."""
    total = 0
    for nq in (1, 31, 32, 33, 129):
        db, q = _case(n, nq, seed=1000 * n + nq)
        got, _resc = _check(db, q, mode, CUT)
        total += len(got)
        assert len(got) < n * nq or n < 3
    assert total > 0


def test_one_query_past_a_block_of_4160():
    """nq = 4161: the matrix route of the chain scan serves queries in blocks of 4160; this one has no blocks -- one pass."""
    db, q = _case(300, 4161, seed=9)
    q[[0, 4159, 4160]] = db[[0, 1, 2]]
    got, _resc = _check(db, q, "prenorm", CUT, oracle=False)
    assert {s for s, _d, _b in got} > {4160, 4159, 0}


# ------------------------------------------------------------------ the cut ----
@pytest.mark.parametrize("mode", MODES)
def test_cut_on_an_occurring_score_one_ulp_above_and_without_one(mode):
    db, q = _case(257, 33, seed=5)
    everything, _resc = _check(db, q, mode, NINF)
    assert len(everything) == 257 * 33                                  # -inf cuts nothing: every cell is a number here
    by_score = sorted(everything, key=lambda e: np.array(e[2], np.uint32).view(np.float32))
    cell = by_score[len(by_score) * 9 // 10]                            # an occurring score, inside the top tenth
    s = np.array(cell[2], np.uint32).view(np.float32)
    assert 0.0 < s < 1.0
    on, _resc = _check(db, q, mode, s)
    above, _resc = _check(db, q, mode, np.nextafter(s, np.float32(2.0)))
    assert cell in on and cell not in above and above < on <= everything
    assert all(np.array(b, np.uint32).view(np.float32) >= s for _s, _d, b in on)


# ------------------------------------------------------------------ NaN, inf, zero vectors; a row above the bound ----
@pytest.mark.parametrize("mode", MODES)
def test_nan_inf_and_zero_vectors(mode):
    """Rows and queries holding NaN, inf and nothing: a NaN score is never emitted, +inf is; flagged rows and queries are scored
    exactly.  Against ms_ip_topk on the GPU (the oracle's list order is not defined for NaN)."""
    db, q = _case(130, 40, seed=6)
    db[3] = np.nan
    db[64, 5] = np.nan
    db[70] = 0.0
    db[100, 7] = np.inf
    db[129, 0] = -np.inf
    q[2] = np.nan
    q[5, 9] = np.inf
    q[7] = 0.0
    q[33, 1] = np.nan
    q[39] = db[100]
    for cut in (CUT, -1e30):
        src, dst, score, count, _resc = _gpu(db, q, mode, cut)
        got = ccc.edge_set(src, dst, score)
        assert count == len(got) and not np.isnan(score).any()
        assert got == _topk_set(db, q, mode, cut)
        assert not any(d in (3, 64) or s in (2, 33) for s, d, _b in got)
    assert any(s == 7 and d == 70 for s, d, _b in got)                     # zero against zero scores 0.0 >= -1e30


def test_a_row_of_norm_3_under_bound_1_is_scored_exactly_and_counted():
    db, q = _case(200, 40, seed=7, scale=False)
    db[77] = 3.0 * q[11]
    got, rescored = _check(db, q, "prenorm", 2.5, bound=1.0)
    assert [(s, d) for s, d, _b in got] == [(11, 77)]
    assert rescored == 40                                               # its 40 cells, and no other: unit rows score below 2.5 - margin
    db[77] = q[11]
    got, rescored = _check(db, q, "prenorm", 2.5, bound=1.0)
    assert not got and rescored == 0


# ------------------------------------------------------------------ row offset and ranges ----
@pytest.mark.parametrize("mode", MODES)
def test_row_offset_beyond_2_32_and_excluded_ranges(mode):
    """The queries are the rows themselves, each excluding its own row; some exclude a range across the first tile's edge, one
    everything, one nothing (lo == hi).  Rows are numbered from an offset beyond 2^32 and the ranges are global."""
    rng = np.random.default_rng(8)
    n = 200
    centres = _unit(rng.standard_normal((20, 128)))
    db = _unit(centres[rng.integers(0, 20, size=n)] + 0.5 * rng.standard_normal((n, 128)) / np.sqrt(128.0))
    off = (1 << 33) + 5
    rows = np.arange(n, dtype=np.int64)
    lo, hi = off + rows, off + rows + 1
    lo[10:20], hi[10:20] = off + 60, off + 70                            # across the tile edge at 64 (their own row is NOT excluded)
    lo[30], hi[30] = off, off + n
    lo[31], hi[31] = off + 31, off + 31
    lo[32], hi[32] = 0, 17                                              # below the offset: excludes nothing
    got, _resc = _check(db, db.copy(), mode, 0.7, lo=lo, hi=hi, row_offset=off)
    assert got and all(d >= off for _s, d, _b in got)
    pairs = {(s, d - off) for s, d, _b in got}
    assert (31, 31) in pairs and (32, 32) in pairs and (12, 12) in pairs and (40, 40) not in pairs
    assert not any(s == 30 for s, _d in pairs) and not any(10 <= s < 20 and 60 <= d < 70 for s, d in pairs)
    free, _resc = _check(db, db.copy(), mode, 0.7, row_offset=off)
    assert len(free) > len(got) and all((s, s + off) in {(a, b) for a, b, _c in free} for s in range(n))


# ------------------------------------------------------------------ a list that drains many times ----
def test_every_cell_unproved_drains_the_waves_lists_many_times():
    """n = 257, nq = 129, every row equal to every query: 33,153 cells, none proved, 256 at a time per wave."""
    rng = np.random.default_rng(10)
    v = _unit(rng.standard_normal(128))
    db, q = np.tile(v, (257, 1)), np.tile(v, (129, 1))
    got, rescored = _check(db, q, "prenorm", CUT)
    assert len(got) == 257 * 129 and rescored == 257 * 129 and len({b for _s, _d, b in got}) == 1


# ------------------------------------------------------------------ 2. the cap rule ----
def test_cap_rule_exact_count_subset_no_duplicates_and_guard_zones():
    import torch
    from merizo_search_amd import ops
    db, q = _case(257, 129, seed=12)
    d_db, d_q = _t(db, np.float32), _t(q, np.float32)
    code = _code("normq")
    src, dst, score, count = ops.threshold_edges(d_db, d_q, code, CUT, BOUND)
    true = ccc.edge_set(src.cpu().numpy(), dst.cpu().numpy(), score.cpu().numpy())
    assert count == len(true) > 50 and true == _topk_set(db, q, "normq", CUT)
    need = int(ops._lib.load().ms_threshold_edges_workspace_bytes(257, 129))
    G = 256
    ws_buf = torch.full((need + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    for cap in (count + 7, count, count - 1, 1, 0):
        bufs = (torch.full((cap + G,), -77, dtype=torch.int64, device="cuda"), torch.full((cap + G,), -77, dtype=torch.int64, device="cuda"),
                torch.full((cap + G,), -77.0, dtype=torch.float32, device="cuda"))
        for _again in range(2):                                          # the second call finds the first one's state in the workspace
            s, d, sc, found = ops.threshold_edges(d_db, d_q, code, CUT, BOUND, out=tuple(b[:cap] for b in bufs), workspace=ws_buf[G:G + need])
            assert found == count                                        # exact, whatever the cap
            kept = min(count, cap)
            assert s.numel() == kept
            got = ccc.edge_set(s.cpu().numpy(), d.cpu().numpy(), sc.cpu().numpy())
            assert len(got) == kept and got <= true and (cap < count or got == true)
            for b, fill in zip(bufs, (-77, -77, -77.0)):
                assert bool((b[kept:] == fill).all()), "a slot at or behind min(count, cap) was written"
            assert bool((ws_buf[:G] == 0x5A).all()) and bool((ws_buf[-G:] == 0x5A).all())
    # without out= the op launches again with `count` slots
    s, d, sc, found = ops.threshold_edges(d_db, d_q, code, CUT, BOUND, cap=5)
    assert found == count and ccc.edge_set(s.cpu().numpy(), d.cpu().numpy(), sc.cpu().numpy()) == true


def test_no_rows_and_what_the_op_refuses():
    import torch
    from merizo_search_amd import ops
    from merizo_search_amd._lib import MerizoHipError
    _db, q = _case(4, 3, seed=13)
    empty = torch.empty((0, 128), dtype=torch.float32, device="cuda")
    src, _dst, _score, count = ops.threshold_edges(empty, _t(q, np.float32), _code("prenorm"), CUT, BOUND)
    assert count == 0 and src.numel() == 0
    db = _t(_db, np.float32)
    with pytest.raises(MerizoHipError, match="go together"):
        ops.threshold_edges(db, _t(q, np.float32), _code("prenorm"), CUT, BOUND, lo=np.zeros(3, np.int64))
    with pytest.raises(MerizoHipError, match="row-norm bound"):
        ops.threshold_edges(db, _t(q, np.float32), _code("prenorm"), CUT, 0.0)
    with pytest.raises(MerizoHipError, match="mode"):
        ops.threshold_edges(db, _t(q, np.float32), 1, CUT, BOUND)
    with pytest.raises(MerizoHipError, match="lo"):
        ops.threshold_edges(db, _t(q, np.float32), _code("prenorm"), CUT, BOUND, lo=np.zeros(2, np.int64), hi=np.ones(2, np.int64))
