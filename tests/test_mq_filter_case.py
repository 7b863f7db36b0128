"""The conditions on the inputs of tests/test_mq_filter_gpu.py, checked through the numpy model alone (no GPU): what
mq_filter_case builds is as adversarial at every row-norm bound and query scale as pf_adversarial's rows are at B ~ 1, the rows
and queries stay inside what the filter serves, and the bounds on `rescored` can tell a working filter from one that proves
nothing."""
import numpy as np
import pytest

import md_scan_case as sc
import mq_filter_case as fc
import pf_adversarial as pa

LAYOUTS = ("edges", "chains")
SETTINGS = [(b, f) for b in fc.BOUNDS for f in fc.QUERY_SCALES["prenorm"]]
# (cell, cut) combinations on the wrong side in the model, as the seeds stand (see the test that counts them)
ON_S = {"edges": 72, "chains": 72}
ALL_CUTS = {"edges": dict(zip(fc.BOUNDS, (107, 82, 107, 82, 82, 107))), "chains": dict(zip(fc.BOUNDS, (107, 82, 107, 88, 82, 107)))}


def _numpy_prepared(q, mode):
    """The normalising modes' queries, normalised in float64 (the GPU tests take the GPU's own launch; the conditions checked here
    do not hang on the last bit of a query)."""
    if mode == "prenorm":
        return np.array(q, np.float32)
    q64 = np.asarray(q, np.float64)
    return (q64 / np.linalg.norm(q64, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def unit_scale():
    """Per layout and mantissa of B: the case at ilogb(B) = 0, f = 0 with its exact and model scores."""
    out = {}
    for layout in LAYOUTS:
        for b in fc.BOUNDS:
            b0 = float(np.ldexp(np.float32(b), -pa.ilogb(b)))
            if (layout, b0) not in out:
                case = fc.build((b0, 0, "prenorm"), layout)
                out[layout, b0] = (case, fc.exact_scores(case, case["q"]), fc.model_scores(case, case["q"]))
    return out


def test_the_cases_cover_the_bounds_scales_and_tile_edges():
    cases = fc.all_cases()
    assert len(cases) == len(set(cases)) == 6 * 5 and len({fc.case_id(c) for c in cases}) == len(cases)
    assert {2.0 ** -40, 1.5 * 2.0 ** -20, 1.0 + 1e-6, 1.9999, 3.0, 2.0 ** 40} <= {b for b, _f, _m in cases}
    assert {pa.f16_sr(b) for b in fc.BOUNDS} == {54, 34, 14, 13, -26}
    edges, chains = fc.build(cases[0], "edges"), fc.build(cases[0], "chains")
    assert edges["db"].shape == chains["db"].shape == (150, 128) and edges["q"].shape == chains["q"].shape == (40, 128)
    assert {0, 63, 64, 127} <= {r for _q, r in edges["cells"]} and max(r for _q, r in edges["cells"]) >= 128
    assert {q // 32 for q, _r in edges["cells"]} == {0, 1} and {31, 32} <= {q for q, _r in edges["cells"]}
    assert len(set(edges["cells"])) == len(set(chains["cells"])) == 4 * fc.M
    # the scan packs 32 two-row chains into a tile: tile rows 0 and 62 of both whole tiles, and the partial tile
    assert {(r // 64, r % 64) for _q, r in chains["cells"]} >= {(0, 0), (0, 62), (1, 0), (1, 62)} and max(r for _q, r in chains["cells"]) >= 128
    assert all(q % 2 == 0 and r % 2 == 0 for q, r in chains["cells"]) and {q // 32 for q, _r in chains["cells"]} == {0, 1}
    assert np.array_equal(chains["table"], np.arange(0, 151, 2)) and chains["qchain"].tolist() == [[2 * g, 2] for g in range(20)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_scaling_rows_by_2_e_and_queries_by_2_f_scales_the_chain_and_the_model_exactly(unit_scale, layout):
    """dot_matrix (the exact fmaf chain) bit for bit and a_model (float64) exactly, at every (B, f): the rounding pattern is the one
    of B in [1, 2), f = 0."""
    for b, f in SETTINGS:
        case = fc.build((b, f, "prenorm"), layout)
        base, s0, a0 = unit_scale[layout, float(np.ldexp(np.float32(b), -case["e"]))]
        k = case["e"] + f
        assert np.array_equal(case["db"], np.ldexp(base["db"], case["e"])) and np.array_equal(case["q"], np.ldexp(base["q"], f))
        s = fc.exact_scores(case, case["q"])
        assert np.array_equal(s.view(np.uint32), fc.pow2(s0, k).view(np.uint32)), (b, f)
        assert np.array_equal(fc.model_scores(case, case["q"]), np.ldexp(a0, k)), (b, f)
        assert pa.f16_sr(case["B"]) == 14 - case["e"]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rows_stay_within_the_bound_and_query_norms_within_what_the_filter_serves(layout):
    for b, f, mode in fc.all_cases():
        case = fc.build((b, f, mode), layout)
        rn = np.linalg.norm(case["db"].astype(np.float64), axis=1)
        qn = fc.query_norms(case["q"])
        assert rn.max() <= case["B"] and rn.max() > 0.99 * 2.0 ** case["e"], (b, rn.max())
        assert 2.0 ** -39 <= qn.min() and qn.max() <= 2.0 ** 39, (f, qn.min(), qn.max())
        assert 2.0 ** -40 <= case["B"] <= 2.0 ** 40
    # the family rows' fp16 error against their own queries, per unit of |row||q|, at B = 1 + 1e-6 (any scale: see above)
    case = fc.build((1.0 + 1e-6, 0, "prenorm"), layout)
    s, a = fc.exact_scores(case, case["q"]).astype(np.float64), fc.model_scores(case, case["q"])
    rn, qn = np.linalg.norm(case["db"].astype(np.float64), axis=1), fc.query_norms(case["q"])
    err = np.array([abs(a[q, r] - s[q, r]) / (rn[r] * qn[q]) for q, r in case["cells"]]).reshape(4, fc.M) / fc.E
    assert (err[0] > 0.45).all() and (err[1] > 0.45).all() and (err[2] > 0.9).all() and (err < 1.0).all(), err
    assert (np.abs(a - s) <= fc.E * rn[None, :] * qn[:, None] * 1.001).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_model_puts_cells_on_the_wrong_side_of_the_cuts_at_every_setting(layout):
    """The number of (cell, cut) combinations whose model score lies on the other side of the cut from the exact score s, over all
    cells of the layout and the seven cuts of every family cell (the global cuts 0.0 and -0.0 are left out: there the filler's
    rounding residues would count by the thousand).  Over the cuts s and its two neighbours, which do not depend on the mantissa
    of B, the count is the same at all 18 settings (B, f): ON_S.  The cuts s +- E B |q| / 2 and s +- 2 E B |q| move with the
    mantissa of B while the model depends on ilogb(B) alone, so the count over all seven is the same at every f and at every B
    of one mantissa: ALL_CUTS.  Both are at least 12 at every setting."""
    on_s, total = {}, {}
    for b, f in SETTINGS:
        case = fc.build((b, f, "prenorm"), layout)
        s, a = fc.exact_scores(case, case["q"]), fc.model_scores(case, case["q"])
        cuts = fc.cuts(case, s, case["q"])[: 7 * len(case["cells"])]
        wrong = [int(((s >= c) != (a >= float(c))).sum()) for c in cuts]
        on_s[b, f] = sum(w for i, w in enumerate(wrong) if i % 7 < 3)
        total[b, f] = sum(wrong)
    print(layout, "on s and its neighbours:", sorted(set(on_s.values())), "all seven cuts:", {b: total[b, 0] for b in fc.BOUNDS})
    assert set(on_s.values()) == {ON_S[layout]} and ON_S[layout] >= 12, on_s
    for b in fc.BOUNDS:
        assert {total[b, f] for f in fc.QUERY_SCALES["prenorm"]} == {ALL_CUTS[layout][b]} and ALL_CUTS[layout][b] >= 12, (b, total)
    by_mantissa = {}
    for b in fc.BOUNDS:
        by_mantissa.setdefault(float(np.frexp(np.float32(b))[0]), set()).add(ALL_CUTS[layout][b])
    assert all(len(v) == 1 for v in by_mantissa.values()), by_mantissa


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rescored_bounds_hold_the_model_and_separate_a_working_filter_from_none(layout):
    """With the model's scores in place of the kernel's: at every cut of every case the cells left to the exact chain lie within
    rescored_bounds; at the cut s of every family cell the upper bound is below 10 % of the cells (a filter that proves nothing
    re-scores all of them); without a cut, and at the cut where a threshold vanishes, the bounds say so."""
    for b, f, mode in fc.all_cases():
        case = fc.build((b, f, mode), layout)
        qprep = _numpy_prepared(case["q"], mode)
        s, a = fc.exact_scores(case, qprep), fc.model_scores(case, qprep)
        cuts = fc.cuts(case, s, qprep)
        for i, c in enumerate(cuts):
            lower, upper = fc.rescored_bounds(case, s, qprep, c)
            got = fc.model_rescored(case, a, qprep, c)
            assert lower <= got <= upper, (b, f, mode, i, lower, got, upper)
            if i < 7 * len(case["cells"]) and i % 7 == 0:
                assert 1 <= lower and upper < s.size // 10, (b, f, mode, i, lower, upper)
        assert fc.rescored_bounds(case, s, qprep, -np.inf) == (s.size, s.size)
        assert fc.rescored_bounds(case, s, qprep, np.inf) == (0, 0)
        assert fc.rescored_bounds(case, s, qprep, cuts[-1])[1] >= s.shape[1]            # the vanishing threshold: that query's n cells
        lo0, up0 = fc.rescored_bounds(case, s, qprep, cuts[0])
        assert fc.rescored_bounds(case, s, qprep, cuts[0], flagged_rows=[5], flagged_queries=[3])[1] >= up0 + s.shape[0] + s.shape[1] - 1 - 2 * 12


def test_pairs_ref_is_scan_ref_and_a_pair_stands_and_falls_with_its_family_cell():
    for b, f, mode in ((1.9999, 0, "prenorm"), (2.0 ** -40, -36, "prenorm"), (3.0, 0, "unit")):
        case = fc.build((b, f, mode), "chains")
        qprep = _numpy_prepared(case["q"], mode)
        s = fc.exact_scores(case, qprep)
        cuts = fc.cuts(case, s, qprep)
        for i, c in enumerate(cuts):
            want = fc.pairs_ref(s, c)
            if i % 9 == 0 or i >= 7 * len(case["cells"]):
                assert want == sc.scan_ref(case["db"], qprep, case["table"], case["qchain"], c)[0]
            if i < 7 * len(case["cells"]):
                (qi, ri), pair = case["cells"][i // 7], case["pairs"][i // 7]
                assert (pair in want) == bool(s[qi, ri] >= c) and (i % 7 != 0 or pair in want)
        assert len(fc.pairs_ref(s, np.float32(-0.5 * case["B"]))) > 200 and fc.pairs_ref(s, np.inf) == []


def test_edges_ref_and_the_lean_query():
    case = fc.build((1.0 + 1e-6, 0, "prenorm"), "edges")
    s = fc.exact_scores(case, case["q"])
    assert len(fc.edges_ref(s, -np.inf)) == s.size and fc.edges_ref(s, np.inf) == set()
    q, r = case["cells"][0]
    at = fc.edges_ref(s, s[q, r])
    assert (q, r, int(s[q, r].view(np.uint32))) in at and len(fc.edges_ref(s, np.nextafter(s[q, r], np.float32(2)))) == len(at) - 1
    # every filler row scores -0.05 |q| against the LEAN query, every family row 0: proved, or within the margin, at any norm served
    for layout in LAYOUTS:
        case = fc.build((1.0 + 1e-6, 0, "prenorm"), layout)
        row = fc.exact_scores(case, case["q"])[case["lean"]]
        special = {r for _q, r in case["cells"]} | ({r + 1 for _q, r in case["cells"]} if layout == "chains" else set())
        for r in range(fc.N):
            assert (abs(row[r]) < 1e-6) if r in special else (-0.051 < row[r] < -0.049), (layout, r, row[r])
        for exponent in (39, 41, -41):
            big = fc.with_lean_query_of_norm(case, exponent)
            assert abs(np.log2(fc.query_norms(big["q"])[case["lean"]]) - exponent) < 0.01
    for factor in (1.0 + 1e-6, 1.0001):
        for b in fc.BOUNDS:
            case = fc.build((b, 0, "prenorm"), "edges")
            moved = fc.with_row_of_norm(case, 5, factor)
            assert abs(np.linalg.norm(moved["db"][5].astype(np.float64)) / (case["B"] * factor) - 1.0) < 1e-7
