"""The fp16 cell filter of ms_threshold_edges and ms_md_chain_scan_mq (csrc/ms_mq.h) away from B = 1, on the GPU: mq_filter_case's
worst-case rows at row-norm bounds from 2^-40 to 2^40 and query norms from 2^-36 to 2^36, in the three modes, at cuts on, next to
and around the family cells' scores, at 0.0, -0.0, a negative cut, +inf and where a threshold vanishes.  The emitted sets are
compared exactly with the CPU chain (multidom_case.dot_matrix over the prepared queries; the one GPU reference is
ops.l2_normalize_rows for those), and out_stats[0] is held between bounds derived from the prep kernel: a filter that loses a cell
fails the first, a filter that proves nothing fails the second.  Then the edges of the row and query flags, and the bounds that are
refused."""
import numpy as np
import pytest

import mq_filter_case as fc

pytestmark = pytest.mark.gpu
CASES = fc.all_cases()
CANARY = -7777
TAIL = 16
CAP = 2048                             # pairs: 20 query chains x 75 chains at the most


class _Edges:
    """ms_threshold_edges over one case's rows and queries, uploaded once."""
    layout = "edges"

    def __init__(self, case):
        self.case, self.mode = case, fc.mode_code(case["mode"])
        self.db, self.q = fc.to_gpu(case["db"], np.float32), fc.to_gpu(case["q"], np.float32)

    def run(self, min_score):
        """-> (the emitted set, rescored), after the checks on the count."""
        from merizo_search_amd import ops
        stats = {}
        src, dst, score, count = ops.threshold_edges(self.db, self.q, self.mode, float(min_score), self.case["B"], stats=stats)
        src, dst, score = src.cpu().numpy(), dst.cpu().numpy(), score.cpu().numpy()
        got = set(zip(src.tolist(), dst.tolist(), score.view(np.uint32).tolist()))
        assert count == len(src) == len(got), "duplicates, or a count that is not the number of cells"
        return got, stats["rescored"]

    @staticmethod
    def ref(scores, min_score):
        return fc.edges_ref(scores, min_score)


class _Chains:
    """ms_md_chain_scan_mq (route "matrix") over one case's chains and query chains, uploaded once; one workspace per route."""
    layout = "chains"

    def __init__(self, case):
        import torch
        self.case, self.mode = case, fc.mode_code(case["mode"])
        self.db, self.q = fc.to_gpu(case["db"], np.float32), fc.to_gpu(case["q"], np.float32)
        self.table, self.qchain = fc.to_gpu(case["table"], np.int64), fc.to_gpu(case["qchain"], np.int32)
        self.pairs = torch.empty((CAP + TAIL, 2), dtype=torch.int64, device="cuda")
        self.count, self.stats = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
        self.status = torch.empty(len(case["qchain"]), dtype=torch.int32, device="cuda")
        self.ws = {}

    def run(self, min_score, route="matrix"):
        """-> (the sorted pairs, rescored), after the checks on the count, the slots behind it and the statuses."""
        import torch
        from merizo_search_amd import ops
        for t in (self.pairs, self.count, self.stats, self.status):
            t.fill_(CANARY)
        kw = dict(route="matrix", row_norm_bound=self.case["B"], out_stats=self.stats) if route == "matrix" else {}
        self.ws[route] = ops.md_chain_scan_launch(self.db, self.table, self.q, self.mode, self.qchain, float(min_score), self.pairs, self.count,
                                                  self.status, cap=CAP, workspace=self.ws.get(route), **kw)
        torch.cuda.synchronize()
        found, p = int(self.count.item()), self.pairs.cpu().numpy()
        assert 0 <= found <= CAP and (p[found:] == CANARY).all(), "a slot at or behind the count was written"
        got = [tuple(int(x) for x in r) for r in p[:found]]
        assert len(set(got)) == found and not self.status.cpu().numpy().any(), "duplicates, or a query chain that was not served"
        return sorted(got), int(self.stats.item()) if route == "matrix" else None

    @staticmethod
    def ref(scores, min_score):
        return fc.pairs_ref(scores, min_score)


ENTRIES = {"edges": _Edges, "chains": _Chains}


def _reference(case):
    """(prepared queries, exact scores) of a case: the GPU normalises, the CPU multiplies."""
    qprep = fc.prepared(case["q"], case["mode"])
    return qprep, fc.exact_scores(case, qprep)


# ------------------------------------------------------------------ 1. every case, every cut ----
@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_threshold_edges_emits_the_exact_set_and_rescores_within_its_bounds(case):
    """150 rows x 40 queries; 89 cuts per case.  rescored >= the cells at or above the cut (each is re-scored before it is emitted)
    and <= the cells within 2.001 E B |q| below it (mq_filter_case.rescored_bounds)."""
    c = fc.build(case, "edges")
    qprep, s = _reference(c)
    gpu = _Edges(c)
    emitted = 0
    for i, ms in enumerate(fc.cuts(c, s, qprep)):
        got, rescored = gpu.run(ms)
        want = fc.edges_ref(s, ms)
        assert got == want, (i, ms, len(got), len(want), sorted(got - want)[:3], sorted(want - got)[:3])
        lower, upper = fc.rescored_bounds(c, s, qprep, ms)
        assert lower <= rescored <= upper, (i, ms, lower, rescored, upper)
        emitted += len(got)
        if i < 7 * len(c["cells"]) and i % 7 == 0:                          # the cut s of a family cell: the cell is there, the filter works
            q, r = c["cells"][i // 7]
            assert (q, r, int(s[q, r].view(np.uint32))) in got and rescored < s.size // 10
    assert emitted > s.size // 2                                            # (the negative cut alone emits most cells)


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_chain_scan_mq_emits_the_exact_pairs_and_rescores_below_its_bound(case):
    """75 chains of 2 rows x 20 query chains of 2 domains; a family pair stands and falls with its family cell.  Route "lane" at the
    first family cell's cut."""
    c = fc.build(case, "chains")
    qprep, s = _reference(c)
    gpu = _Chains(c)
    for i, ms in enumerate(fc.cuts(c, s, qprep)):
        got, rescored = gpu.run(ms)
        want = fc.pairs_ref(s, ms)
        assert got == want, (i, ms, len(got), len(want), sorted(set(got) - set(want))[:3], sorted(set(want) - set(got))[:3])
        upper = fc.rescored_bounds(c, s, qprep, ms)[1]
        assert 0 <= rescored <= upper, (i, ms, rescored, upper)
        if i < 7 * len(c["cells"]):
            (q, r), pair = c["cells"][i // 7], c["pairs"][i // 7]
            assert (pair in got) == bool(s[q, r] >= ms)
            if i % 7 == 0:
                assert pair in got and 1 <= rescored < s.size // 10
        if i == 0:
            assert gpu.run(ms, route="lane")[0] == want


# ------------------------------------------------------------------ 2. the flags' edges ----
@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("bound", fc.BOUNDS, ids=lambda b: fc.case_id((b, 0, "prenorm"))[:-len("-f0-prenorm")])
def test_a_row_just_inside_the_bound_is_filtered_and_a_row_just_above_it_is_rescored_whole(bound, entry):
    """Filler row 5 at norm B (1 + 1e-6) -- inside the slack of B^2 (1 + 1e-5) on the sum of squares -- and at B x 1.0001.  Its scores
    against every query lie far below the cut (a family cell's score), so unflagged none of its cells reaches the exact chain and
    flagged exactly its nq cells do, on top of the same cells of the other rows."""
    base = fc.build((bound, 0, "prenorm"), entry)
    counts = []
    for factor in (1.0 + 1e-6, 1.0001):
        c = fc.with_row_of_norm(base, 5, factor)
        qprep, s = _reference(c)
        ms = fc.cuts(c, s, qprep)[0]
        assert fc.rescored_bounds(c, s[:, 5:6], qprep, ms) == (0, 0)         # not one of the row's cells is near the cut
        gpu = ENTRIES[entry](c)
        got, rescored = gpu.run(ms)
        assert got == gpu.ref(s, ms) and len(got) >= 1
        lower, upper = fc.rescored_bounds(c, s, qprep, ms, flagged_rows=[5] if factor > 1.00001 else [])
        assert (lower if entry == "edges" else 1) <= rescored <= upper, (factor, lower, rescored, upper)
        counts.append(rescored)
    assert counts[1] == counts[0] + fc.NQ, counts


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("bound", fc.BOUNDS, ids=lambda b: fc.case_id((b, 0, "prenorm"))[:-len("-f0-prenorm")])
def test_a_query_of_norm_2_39_is_filtered_and_one_of_norm_2_41_or_2_minus_41_is_rescored_whole(bound, entry):
    """The LEAN query: every filler row scores -0.05 |q| against it and every family row (and second row) 0, so at a family cell's
    cut the filter proves all of its cells at norm 1, all but those 12 (24) at norm 2^39 where the margin E B |q| dwarfs the cut,
    and nothing once the norm is outside [2^-40, 2^40]: exactly n more cells than at norm 1."""
    base = fc.build((bound, 0, "prenorm"), entry)
    lean = base["lean"]
    near_zero = len(base["cells"]) * (2 if entry == "chains" else 1)
    counts = {}
    for exponent in (0, 39, 41, -41):
        c = fc.with_lean_query_of_norm(base, exponent) if exponent else base
        qprep, s = _reference(c)
        ms = fc.cuts(base, s, qprep)[0]
        gpu = ENTRIES[entry](c)
        got, rescored = gpu.run(ms)
        assert got == gpu.ref(s, ms) and len(got) >= 1
        flagged = [lean] if abs(exponent) > 40 else []
        lower, upper = fc.rescored_bounds(c, s, qprep, ms, flagged_queries=flagged)
        assert (lower if entry == "edges" else 1) <= rescored <= upper, (exponent, lower, rescored, upper)
        own = fc.rescored_bounds(c, s[lean: lean + 1], qprep[lean: lean + 1], ms)
        assert (exponent != 0 or own == (0, 0)) and (exponent != 39 or own[1] == near_zero), (exponent, own)     # (its own cells, from the CPU)
        counts[exponent] = rescored
    assert counts[0] <= counts[39] <= counts[0] + near_zero, counts
    assert counts[41] == counts[-41] == counts[0] + fc.N, counts


# ------------------------------------------------------------------ 3. refusals ----
def test_bounds_outside_2_minus_40_to_2_40_are_refused_with_nothing_written():
    """One fp32 step below 2^-40, one above 2^40, NaN and -1: MS_ERR_RANGE (-4) from both entry points, every output and the
    workspace as they were; the two ends themselves are served."""
    import torch
    from merizo_search_amd import _lib
    lib = _lib.load()
    c = fc.build((1.0 + 1e-6, 0, "prenorm"), "chains")
    n, nq, nqc = fc.N, fc.NQ, len(c["qchain"])
    db, q = fc.to_gpu(c["db"], np.float32), fc.to_gpu(c["q"], np.float32)
    table, qchain = fc.to_gpu(c["table"], np.int64), fc.to_gpu(c["qchain"], np.int32)
    need = max(int(lib.ms_threshold_edges_workspace_bytes(n, nq)), int(lib.ms_md_chain_scan_mq_workspace_bytes(n, nq)))
    cap = 64
    out = dict(src=torch.int64, dst=torch.int64, score=torch.float32, pairs=torch.int64, count=torch.int64, stats=torch.int64,
               status=torch.int32)
    size = dict(src=cap, dst=cap, score=cap, pairs=2 * cap, count=1, stats=1, status=nqc)
    bufs = {k: torch.full((size[k],), CANARY, dtype=dt, device="cuda") for k, dt in out.items()}
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")

    def edges(bound):
        rc = lib.ms_threshold_edges(db.data_ptr(), n, 0, q.data_ptr(), nq, fc.mode_code("prenorm"), None, None, 0.5, bound,
                                    bufs["src"].data_ptr(), bufs["dst"].data_ptr(), bufs["score"].data_ptr(), cap, bufs["count"].data_ptr(),
                                    bufs["stats"].data_ptr(), ws.data_ptr(), need, None)
        torch.cuda.synchronize()
        return rc

    def chains(bound):
        rc = lib.ms_md_chain_scan_mq(db.data_ptr(), n, table.data_ptr(), n // 2, q.data_ptr(), nq, fc.mode_code("prenorm"), None, None, 0.0,
                                     qchain.data_ptr(), nqc, 0.5, bufs["pairs"].data_ptr(), cap, bufs["count"].data_ptr(),
                                     bufs["status"].data_ptr(), bound, bufs["stats"].data_ptr(), ws.data_ptr(), need, None)
        torch.cuda.synchronize()
        return rc

    lo, hi = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
    for bound in (float(np.nextafter(lo, np.float32(0))), float(np.nextafter(hi, np.float32(np.inf))), float("nan"), -1.0):
        for call in (edges, chains):
            assert call(bound) == -4 and b"row-norm bound" in lib.ms_last_error(), (call.__name__, bound)
            for k, b in bufs.items():
                assert bool((b == CANARY).all()), (call.__name__, bound, k)
            assert bool((ws == 0x5A).all()), (call.__name__, bound)
    for bound in (float(lo), float(hi)):
        for call in (edges, chains):
            assert call(bound) == 0 and int(bufs["count"].item()) >= 0 and int(bufs["stats"].item()) >= 0, (call.__name__, bound)
