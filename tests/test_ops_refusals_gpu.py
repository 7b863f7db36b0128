"""What the tensor-level entry points of merizo_search_amd.ops accept, refuse and leave untouched, on 8 to 64 rows: one minimal
valid call per entry point (against the numpy restatements where one is at hand), one refusal per kind of bad argument
(MerizoHipError whose message names the argument), host arrays and lists against device tensors bit for bit, guard zones around
caller-provided outputs and workspaces, and the launch count of the two calls that launch again beyond their cap.

TIGHTENED marks the three rules the shared argument checks state once for every entry point, where single entry points used to
differ: a caller's workspace that is too short is refused before the library is called, a floating-point lo / hi is refused as
every other integer descriptor is, and the chain scan's sizing message names the sizing function that was asked."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

import best_mapping_case as bm
import cluster_case as cc
import cluster_complete_case as ccc
import cluster_components_case as ccomp
import dbquery_case as dq
import md_scan_case as sc

pytestmark = pytest.mark.gpu
BOUND = 1.0 + 1e-6                     # the row-norm bound of unit rows
N, NQ, K = 64, 8, 4
NC, NCK, NEXTRA = 33, 5, 20            # the clustering case: rows, list width, extra entries
MINCOS = 0.5
TIGHTENED = "tightened"


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(a, b):
    """Bit for bit: dtype, shape and bytes of every array of two results."""
    a, b = [_np(x) for x in a], [_np(x) for x in b]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _strided(t):
    """t's values and shape in a tensor that is not contiguous."""
    import torch
    return torch.stack([t, t], dim=-1)[..., 0]


@pytest.fixture(scope="module")
def c():
    import torch
    from merizo_search_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(2024)
    db = sc.unit(rng.standard_normal((N, 128)))
    db[24:26] = db[0:2]                                   # chain 3 holds chain 0's first two rows again
    rows = np.asarray([0, 1, 8, 9, 10, 16, 17, 18], np.int64)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    c = SimpleNamespace(torch=torch, ops=ops, lib=lib, t=t, rows=rows, db_h=db, q_h=db[rows].copy(), db=t(db), q=t(db[rows]),
                        prenorm=_lib.MODE_IP_PRENORM, cosine=_lib.MODE_COSINE_UNIT)
    c.s8, c.i8 = ops.ip_topk(c.db, c.q, 8)
    c.idx_h, c.score_h, c.len_h = cc.random_lists(NC, NCK, seed=3)
    c.extra_h = ccc.random_extras(NC, NEXTRA, c.idx_h, c.score_h, seed=4)
    c.table = np.arange(0, N + 1, 8, dtype=np.int64)      # 8 target chains of 8 rows
    c.qchain = np.asarray([(0, 2), (2, 3), (5, 3)], np.int32)
    c.cand = np.asarray([(0, 2, 0, 8), (2, 3, 8, 8), (5, 3, 16, 8)], np.int32)     # each query chain against the chain it was cut from
    c.trows, c.mat_off = np.arange(N, dtype=np.int64), np.asarray([0, 16, 40], np.int64)
    c.md_scores = ops.md_chain_scores(c.db, c.q, c.prenorm, c.cand, c.trows, c.mat_off, MINCOS)[0]
    c.need = {"ip_topk": lib.ms_ip_topk_workspace_bytes(N, NQ, K), "cluster_greedy": lib.ms_cluster_workspace_bytes(NC),
              "cluster_greedy_edges": lib.ms_cluster_workspace_bytes(NC), "cluster_components": lib.ms_cluster_components_workspace_bytes(NC),
              "threshold_edges": lib.ms_threshold_edges_workspace_bytes(N, NQ), "md_chain_scores": lib.ms_md_chain_scores_workspace_bytes(NQ),
              "md_best_mappings": lib.ms_md_best_mappings_workspace_bytes(3, 64), "md_chain_scan_launch": lib.ms_md_chain_scan_workspace_bytes(N, NQ),
              "md_chain_scan_mq": lib.ms_md_chain_scan_mq_workspace_bytes(N, NQ)}
    c.need = {op: int(v) for op, v in c.need.items()}
    assert all(v > 0 for v in c.need.values())
    return c


def _base(c, op):
    """The arguments of the minimal valid call of `op`, by name."""
    torch, t = c.torch, c.t
    if op == "ip_topk":
        return dict(db=c.db, q=c.q, k=K)
    if op == "ip_topk_prefiltered":
        return dict(db=c.db, q=c.q, k=K, row_norm_bound=BOUND)
    if op == "topk_drop_ranges":
        return dict(scores=c.s8, idx=c.i8, lo=c.rows, hi=c.rows + 1, kout=K)
    if op == "topk_excluding":
        return dict(db=c.db, q=c.q, k=K, lo=c.rows, hi=c.rows + 1)
    if op.startswith("cluster"):
        a = dict(nbr_idx=t(c.idx_h), nbr_score=t(c.score_h), lengths=c.len_h, min_score=float(cc.CUT), mincov=0.7)
        if op != "cluster_greedy":
            a.update(edge_src=t(c.extra_h[0]), edge_dst=t(c.extra_h[1]), edge_score=t(c.extra_h[2]))
        return a
    if op == "threshold_edges":
        return dict(db=c.db, q=c.q, mode=c.prenorm, min_score=MINCOS, row_norm_bound=BOUND)
    if op == "md_chain_scores":
        return dict(db=c.db, q=c.q, mode=c.prenorm, cand=c.cand, trows=c.trows, mat_off=c.mat_off, min_score=MINCOS)
    if op == "md_best_mappings":
        return dict(scores=c.md_scores, cand=c.cand, mat_off=c.mat_off)
    if op == "md_chain_scan_launch":
        return dict(db=c.db, chain_start=t(c.table), q=c.q, mode=c.prenorm, qchain=t(c.qchain), min_score=MINCOS,
                    out_pairs=torch.full((16, 2), -7, dtype=torch.int64, device="cuda"), out_count=torch.zeros(1, dtype=torch.int64, device="cuda"),
                    out_qstatus=torch.zeros(3, dtype=torch.int32, device="cuda"))
    if op == "md_chain_scan":
        return dict(db=c.db, chain_start=c.table, q=c.q, mode=c.prenorm, qchain=c.qchain, min_score=MINCOS)
    raise KeyError(op)


def _call(c, op, **over):
    return getattr(c.ops, op)(**dict(_base(c, op), **over))


def _edge_set(result):
    src, dst, score, count = result
    got = ccc.edge_set(_np(src), _np(dst), _np(score))
    assert count == len(got) == len(_np(src))
    return got


# ------------------------------------------------------------------ 1. one minimal valid call each ---
def _form(tensors):
    return [(str(x.dtype).replace("torch.", ""), tuple(x.shape)) for x in tensors]


def test_search_calls_return_the_documented_form(c):
    s, i = _call(c, "ip_topk")
    assert _form((s, i)) == [("float32", (NQ, K)), ("int64", (NQ, K))]
    assert np.array_equal(_np(i)[2:, 0], c.rows[2:]) and set(_np(i)[0, :2]) == {0, 24}            # every query is a row (two of them twice)
    assert _same(_call(c, "ip_topk_prefiltered"), (s, i))                                           # (below its row limit: the same search)
    s, i, n = _call(c, "topk_excluding")
    assert _form((s, i, n)) == [("float32", (NQ, K)), ("int64", (NQ, K)), ("int32", (NQ,))]
    assert not (_np(i) == c.rows[:, None]).any() and (_np(n) == K).all()
    assert _same((s, i, n), dq.drop_ranges_np(_np(c.s8), _np(c.i8), c.rows, c.rows + 1, -np.inf, K))
    assert _same(_call(c, "topk_drop_ranges"), dq.drop_ranges_np(_np(c.s8), _np(c.i8), c.rows, c.rows + 1, -np.inf, K))


def _cluster_result(result):
    rep, rep_score, info = result
    return (_np(rep), _np(rep_score)), {key: v for key, v in info.items() if key != "rounds"}


def test_cluster_calls_equal_their_restatements_and_the_list_call_equals_the_edges_call_without_edges(c):
    args = (c.idx_h, c.score_h, c.len_h, float(cc.CUT), 0.7)
    got, info = _cluster_result(_call(c, "cluster_greedy"))
    want = cc.cluster_greedy_np(*args)
    assert _same(got, want[:2]) and info == {key: want[2][key] for key in ("n_reps", "saturated")}
    # ms_cluster_greedy against ms_cluster_greedy_edges at m = 0 on the same lists: rep, rep_score and info, rounds included
    rep, rep_score, full = _call(c, "cluster_greedy")
    e_rep, e_score, e_full = _call(c, "cluster_greedy_edges", edge_src=None, edge_dst=None, edge_score=None)
    assert _same((rep, rep_score), (e_rep, e_score)) and full == e_full and set(full) == {"n_reps", "rounds", "saturated"}
    got, info = _cluster_result(_call(c, "cluster_greedy_edges"))
    want = ccc.cluster_greedy_edges_np(c.idx_h, c.score_h, *c.extra_h, *args[2:])
    assert _same(got, want[:2]) and info == want[2]
    got, info = _cluster_result(_call(c, "cluster_components"))
    want = ccomp.cluster_components_np(c.idx_h, c.score_h, *c.extra_h, *args[2:])
    assert _same(got, want[:2]) and info == want[2]


def test_threshold_edges_and_the_chain_calls_on_the_planted_rows(c):
    cells = _edge_set(_call(c, "threshold_edges"))
    assert {(s, d) for s, d, _bits in cells} == {(qi, int(r)) for qi, r in enumerate(c.rows)} | {(0, 24), (1, 25)}
    scores, match = _call(c, "md_chain_scores")
    assert _form((scores, match)) == [("float32", (64,)), ("int32", (3, 2))] and _np(match).tolist() == [[2, 2], [3, 3], [3, 3]]
    got = _call(c, "md_best_mappings")
    assert _form(got) == [("int32", (3, 2)), ("int64", (3, 2)), ("int32", (3, 2, 64)), ("float32", (3, 2, 64))]
    assert _same(got, bm.best_mappings(_np(scores), c.cand, c.mat_off))
    want, want_status = sc.scan_ref(c.db_h, c.q_h, c.table, c.qchain, MINCOS)
    assert want == [(0, 0), (0, 3), (1, 1), (2, 2)]
    pairs, status = _call(c, "md_chain_scan")
    assert pairs.dtype == np.int64 and status.dtype == np.int32 and [tuple(p) for p in pairs.tolist()] == want and status.tolist() == want_status
    a = _base(c, "md_chain_scan_launch")
    ws = c.ops.md_chain_scan_launch(**a)
    assert ws.dtype == c.torch.uint8 and ws.numel() == c.need["md_chain_scan_launch"] and int(a["out_count"].item()) == len(want)
    assert sorted(tuple(p) for p in _np(a["out_pairs"])[:len(want)].tolist()) == want and (_np(a["out_pairs"])[len(want):] == -7).all()
    assert _np(a["out_qstatus"]).tolist() == want_status


# ------------------------------------------------------------------ 2. what the calls refuse ---
def _word(name):
    return r"\b%s\b" % re.escape(name)


LISTS = r"int64 / float32 CUDA tensors"            # how the three cluster calls name their two list tensors
ONE_SHAPE = r"float32 / int64 CUDA tensors"        # how topk_drop_ranges names its two
f64 = lambda x: x.double()
i32 = lambda x: x.int()
f32 = lambda x: x.float()
host = lambda x: x.cpu()
CLUSTER_EDGES = ("cluster_greedy_edges", "cluster_components")

# (entry point, argument -> how its valid value is spoilt, what the message must contain[, TIGHTENED])
REFUSALS = [
    ("ip_topk", {"db": f64}, _word("db")),
    ("ip_topk", {"q": host}, _word("q")),
    ("ip_topk", {"db": _strided}, _word("db")),
    ("ip_topk", {"lengths": lambda c: c.torch.ones(N - 1, device="cuda")}, _word("lengths")),
    ("ip_topk", {"qlen": lambda c: c.torch.ones(NQ + 1, device="cuda")}, _word("qlen")),
    ("ip_topk", {"inv_norm": lambda c: c.torch.ones(N, device="cuda").double()}, _word("inv_norm")),
    ("ip_topk", {"workspace": lambda c: c.torch.zeros(c.need["ip_topk"] - 1, dtype=c.torch.uint8, device="cuda")}, _word("workspace")),
    ("ip_topk_prefiltered", {"db": f64}, _word("db")),
    ("ip_topk_prefiltered", {"q": _strided}, _word("q")),
    ("ip_topk_prefiltered", {"lengths": lambda c: c.torch.ones(N, device="cuda")}, _word("lengths")),          # (not the cosine mode)
    ("ip_topk_prefiltered", {"mode": lambda c: c.cosine, "lengths": lambda c: c.torch.ones(N - 1, device="cuda"),
                             "qlen": lambda c: c.torch.ones(NQ, device="cuda")}, _word("lengths")),
    ("ip_topk_prefiltered", {"mode": lambda c: c.cosine, "lengths": lambda c: c.torch.ones(N, device="cuda"),
                             "qlen": lambda c: c.torch.ones(NQ).cuda().double()}, _word("qlen")),
    ("ip_topk_prefiltered", {"image": lambda c: c.db}, _word("image")),
    ("topk_drop_ranges", {"idx": i32}, ONE_SHAPE),
    ("topk_drop_ranges", {"scores": host}, ONE_SHAPE),
    ("topk_drop_ranges", {"lo": lambda c: c.rows[:-1]}, _word("lo")),
    ("topk_drop_ranges", {"hi": lambda c: c.t(c.rows + 1).reshape(NQ, 1)}, _word("hi")),
    ("topk_drop_ranges", {"lo": lambda c: c.t(c.rows).float()}, _word("lo") + ".*integers", TIGHTENED),
    ("topk_drop_ranges", {"kout": lambda c: 9}, _word("kout")),
    ("topk_excluding", {"db": f64}, _word("db")),
    ("topk_excluding", {"lo": lambda c: c.rows[:-1], "max_excluded": lambda c: 1}, _word("lo")),
    ("topk_excluding", {"hi": lambda c: c.t(c.rows + 1).double()}, _word("hi") + ".*integers", TIGHTENED),
    ("cluster_greedy", {"nbr_idx": lambda c: c.t(c.idx_h[:, :0]), "nbr_score": lambda c: c.t(c.score_h[:, :0])}, "k >= 1"),
    ("cluster_greedy", {"lengths": lambda c: np.zeros(NC + 1, np.int32)}, _word("lengths")),
    ("threshold_edges", {"db": f64}, _word("db")),
    ("threshold_edges", {"q": host}, _word("q")),
    ("threshold_edges", {"lo": lambda c: c.rows}, "go together"),
    ("threshold_edges", {"lo": lambda c: c.rows[:-1], "hi": lambda c: c.rows + 1}, _word("lo")),
    ("threshold_edges", {"lo": lambda c: c.t(c.rows).float(), "hi": lambda c: c.rows + 1}, _word("lo") + ".*integers", TIGHTENED),
    ("threshold_edges", {"out": lambda c: (c.t(c.rows).int(), c.t(c.rows), c.t(c.rows).float())}, _word("out")),
    ("threshold_edges", {"out": lambda c: (c.t(c.rows), c.t(c.rows).cpu(), c.t(c.rows).float())}, _word("out")),
    ("threshold_edges", {"out": lambda c: (c.t(c.rows), c.t(c.rows), _strided(c.t(c.rows).float()))}, _word("out")),
    ("threshold_edges", {"out": lambda c: (c.t(c.rows), c.t(c.rows)[:-1], c.t(c.rows).float())}, _word("out")),
    ("md_chain_scores", {"db": host}, _word("db")),
    ("md_chain_scores", {"cand": lambda c: c.cand[:, :3]}, _word("cand")),
    ("md_chain_scores", {"cand": lambda c: c.t(c.cand).float()}, _word("cand") + ".*integers"),
    ("md_chain_scores", {"trows": lambda c: c.t(c.trows).double()}, _word("trows") + ".*integers"),
    ("md_chain_scores", {"trows": lambda c: c.trows.reshape(8, 8)}, _word("trows")),
    ("md_chain_scores", {"mat_off": lambda c: c.mat_off[:2]}, _word("mat_off")),
    ("md_chain_scores", {"lengths": lambda c: c.torch.ones(N + 1, device="cuda")}, _word("lengths")),
    ("md_chain_scores", {"qlen": lambda c: c.torch.ones(NQ, device="cuda").double()}, _word("qlen")),
    ("md_best_mappings", {"scores": f64}, _word("scores")),
    ("md_best_mappings", {"scores": host}, _word("scores")),
    ("md_best_mappings", {"scores": lambda x: x.view(8, 8)}, _word("scores")),
    ("md_best_mappings", {"cand": lambda c: c.cand[:, :3]}, _word("cand")),
    ("md_best_mappings", {"mat_off": lambda c: c.mat_off[:2]}, _word("mat_off")),
    ("md_best_mappings", {"mat_off": lambda c: c.t(c.mat_off).float()}, _word("mat_off") + ".*integers"),
    ("md_chain_scan_launch", {"chain_start": i32}, _word("chain_start")),
    ("md_chain_scan_launch", {"qchain": host}, _word("qchain")),
    ("md_chain_scan_launch", {"qchain": lambda x: x.reshape(-1)[:5]}, _word("qchain")),
    ("md_chain_scan_launch", {"out_pairs": _strided}, _word("out_pairs")),
    ("md_chain_scan_launch", {"cap": lambda c: 17}, _word("out_pairs")),
    ("md_chain_scan_launch", {"out_qstatus": lambda x: x[:2]}, _word("out_qstatus")),
    ("md_chain_scan_launch", {"out_count": i32}, _word("out_count")),
    ("md_chain_scan_launch", {"lengths": lambda c: c.torch.ones(N - 1, device="cuda")}, _word("lengths")),
    ("md_chain_scan_launch", {"route": lambda c: "matrix", "row_norm_bound": lambda c: BOUND,
                              "out_stats": lambda c: c.torch.zeros(1, dtype=c.torch.int32, device="cuda")}, _word("out_stats")),
    ("md_chain_scan_launch", {"route": lambda c: "matrix", "row_norm_bound": lambda c: BOUND,
                              "workspace": lambda c: c.torch.zeros(c.need["md_chain_scan_mq"] - 1, dtype=c.torch.uint8, device="cuda")},
     _word("workspace") + ".*at least", TIGHTENED),
    ("md_chain_scan_launch", {"route": lambda c: "matrix", "row_norm_bound": lambda c: BOUND, "q": lambda x: x[:0]},
     "ms_md_chain_scan_mq_workspace_bytes", TIGHTENED),
    ("md_chain_scan_launch", {"q": lambda x: x[:0]}, "ms_md_chain_scan_workspace_bytes"),
    ("md_chain_scan", {"db": f64}, _word("db")),
    ("md_chain_scan", {"qchain": lambda c: c.t(c.qchain).float()}, "expected integers"),
    ("md_chain_scan", {"chain_start": lambda c: c.t(c.table).double()}, "expected integers"),
    ("md_chain_scan", {"route": lambda c: "diagonal"}, _word("route")),
    ("md_chain_scan", {"route": lambda c: "matrix"}, _word("row_norm_bound")),
]
for _op in ("cluster_greedy",) + CLUSTER_EDGES:
    REFUSALS += [
        (_op, {"nbr_idx": i32}, LISTS),
        (_op, {"nbr_score": host}, LISTS),
        (_op, {"nbr_idx": _strided}, "contiguous"),
        (_op, {"lengths": lambda c: c.t(c.len_h).float()}, _word("lengths")),
        (_op, {"lengths": lambda c: c.len_h.reshape(1, NC)}, _word("lengths")),
        (_op, {"mincov": lambda c: 1.5}, _word("mincov")),
    ]
for _op in CLUSTER_EDGES:
    REFUSALS += [
        (_op, {"edge_src": i32}, _word("edge_src")),
        (_op, {"edge_score": host}, _word("edge_score")),
        (_op, {"edge_dst": _strided}, _word("edge_dst")),
        (_op, {"edge_dst": lambda x: x[:-1]}, "one length"),
        (_op, {"edge_src": lambda c: None}, "go together"),
        (_op, {"nbr_idx": lambda c: None}, "go together"),
    ]
# a caller's workspace: another dtype, and one byte short (the four calls that left a short one to the library: TIGHTENED)
for _op, _tight in (("cluster_greedy", ()), ("cluster_greedy_edges", ()), ("cluster_components", ()), ("threshold_edges", (TIGHTENED,)),
                    ("md_chain_scores", (TIGHTENED,)), ("md_best_mappings", (TIGHTENED,)), ("md_chain_scan_launch", (TIGHTENED,))):
    REFUSALS += [
        (_op, {"workspace": lambda c, op=_op: c.torch.zeros(c.need[op], dtype=c.torch.int8, device="cuda")}, _word("workspace")),
        (_op, {"workspace": lambda c, op=_op: c.torch.zeros(c.need[op] - 1, dtype=c.torch.uint8, device="cuda")}, _word("workspace") + ".*at least") + _tight,
    ]


def _spoil(c, op, how):
    """The overrides of one refusal: a function of the fixture (its parameter is called c), or of the argument's valid value."""
    base = _base(c, op)
    return {name: fn(c) if fn.__code__.co_varnames[:1] == ("c",) else fn(base[name]) for name, fn in how.items()}


@pytest.mark.parametrize("case", REFUSALS, ids=lambda case: "%s-%s%s" % (case[0], "+".join(case[1]), "-tightened" if TIGHTENED in case else ""))
def test_refusals_name_the_argument(c, case):
    from merizo_search_amd._lib import MerizoHipError
    op, how, match = case[:3]
    with pytest.raises(MerizoHipError, match=match):
        _call(c, op, **_spoil(c, op, how))


OUT_ARITY = {"ip_topk": 2, "ip_topk_prefiltered": 2, "topk_drop_ranges": 3, "cluster_greedy": 2, "cluster_greedy_edges": 2, "cluster_components": 2,
             "md_chain_scores": 2, "md_best_mappings": 4}


@pytest.mark.parametrize("op", sorted(OUT_ARITY))
def test_an_out_tuple_with_one_wrong_dtype_or_one_wrong_shape_is_refused(c, op):
    from merizo_search_amd._lib import MerizoHipError
    good = tuple(_call(c, op)[:OUT_ARITY[op]])
    assert _call(c, op, out=good)[0] is good[0]                                   # its own outputs are a valid `out`
    first, last = good[0], good[-1]
    wider = last.new_empty(tuple(last.shape[:-1]) + (last.shape[-1] + 1,))
    for bad in ((first.to(c.torch.int16),) + good[1:], good[:-1] + (wider,), good[:-1] + (_strided(last),)):
        with pytest.raises(MerizoHipError, match="out must be"):
            _call(c, op, out=bad)


# ------------------------------------------------------------------ 3. host arrays, lists and tensors ---
def test_host_arrays_and_lists_give_what_device_tensors_give(c):
    t = c.t
    lo, hi = c.rows, c.rows + 1
    want = _call(c, "topk_drop_ranges", lo=t(lo), hi=t(hi))
    assert _same(want, _call(c, "topk_drop_ranges")) and _same(want, _call(c, "topk_drop_ranges", lo=lo.tolist(), hi=hi.tolist()))
    assert _same(want, _call(c, "topk_drop_ranges", lo=t(lo).int(), hi=t(hi).int()))                     # (another integer type is converted)
    want = _call(c, "topk_excluding", lo=t(lo), hi=t(hi))
    assert _same(want, _call(c, "topk_excluding")) and _same(want, _call(c, "topk_excluding", lo=lo.tolist(), hi=hi.tolist()))
    want = _edge_set(_call(c, "threshold_edges", lo=t(lo), hi=t(hi)))
    assert len(want) == 2 and want == _edge_set(_call(c, "threshold_edges", lo=lo, hi=hi))
    assert want == _edge_set(_call(c, "threshold_edges", lo=lo.tolist(), hi=hi.tolist()))
    for op in ("cluster_greedy",) + CLUSTER_EDGES:
        want = _cluster_result(_call(c, op, lengths=t(c.len_h)))
        for lengths in (c.len_h, c.len_h.tolist(), t(c.len_h).long()):
            got = _cluster_result(_call(c, op, lengths=lengths))
            assert _same(got[0], want[0]) and got[1] == want[1]
    want = _call(c, "md_chain_scores", cand=t(c.cand), trows=t(c.trows), mat_off=t(c.mat_off))
    assert _same(want, _call(c, "md_chain_scores"))
    out = tuple(x.clone().fill_(-7) for x in want)           # (lists: with out=, the scores' size is not derived from the descriptors)
    assert _same(want, _call(c, "md_chain_scores", cand=c.cand.tolist(), trows=c.trows.tolist(), mat_off=c.mat_off.tolist(), out=out))
    want = _call(c, "md_best_mappings", cand=t(c.cand), mat_off=t(c.mat_off))
    assert _same(want, _call(c, "md_best_mappings")) and _same(want, _call(c, "md_best_mappings", cand=c.cand.tolist(), mat_off=c.mat_off.tolist()))
    want = _call(c, "md_chain_scan", chain_start=t(c.table), qchain=t(c.qchain))
    assert len(want[0]) == 4 and _same(want, _call(c, "md_chain_scan"))
    assert _same(want, _call(c, "md_chain_scan", chain_start=c.table.tolist(), qchain=c.qchain.tolist()))
    assert _same(want, _call(c, "md_chain_scan", qchain=c.qchain.reshape(-1).tolist()))                  # a flat (q0, nqd, q0, nqd, ...) list
    assert _same(want, _call(c, "md_chain_scan", chain_start=t(c.table).reshape(-1, 1), qchain=t(c.qchain).reshape(-1)))


# ------------------------------------------------------------------ 4. guard zones ---
G = 256                                # guard elements on either side


class _Guarded:
    """A tensor of `shape` inside a filled buffer with G elements of the fill on either side."""

    def __init__(self, torch, shape, dtype, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
        self.fill, self.n = fill, n
        self.t = self.buf[G:G + n].view(shape)

    def untouched(self):
        return bool((self.buf[:G] == self.fill).all()) and bool((self.buf[G + self.n:] == self.fill).all())


def test_guard_zones_around_the_outputs_of_topk_drop_ranges(c):
    torch = c.torch
    out = [_Guarded(torch, (NQ, K), torch.float32, -77.0), _Guarded(torch, (NQ, K), torch.int64, -77), _Guarded(torch, (NQ,), torch.int32, -77)]
    got = _call(c, "topk_drop_ranges", out=tuple(g.t for g in out))
    assert all(r is g.t for r, g in zip(got, out)) and all(g.untouched() for g in out)
    assert _same(got, _call(c, "topk_drop_ranges"))


def test_guard_zones_around_the_outputs_and_the_workspace_of_threshold_edges_below_the_count(c):
    torch = c.torch
    want = _edge_set(_call(c, "threshold_edges"))
    cap = len(want) - 3
    out = [_Guarded(torch, (cap,), torch.int64, -77), _Guarded(torch, (cap,), torch.int64, -77), _Guarded(torch, (cap,), torch.float32, -77.0)]
    ws = _Guarded(torch, (c.need["threshold_edges"],), torch.uint8, 0x5A)
    src, dst, score, count = _call(c, "threshold_edges", out=tuple(g.t for g in out), workspace=ws.t)
    assert count == len(want) and [x.data_ptr() for x in (src, dst, score)] == [g.t.data_ptr() for g in out] and len(src) == cap
    assert ccc.edge_set(_np(src), _np(dst), _np(score)) <= want and all(g.untouched() for g in out + [ws])


def test_guard_zones_around_the_outputs_and_the_workspace_of_md_best_mappings(c):
    torch = c.torch
    out = [_Guarded(torch, (3, 2), torch.int32, -77), _Guarded(torch, (3, 2), torch.int64, -77), _Guarded(torch, (3, 2, 64), torch.int32, -77),
           _Guarded(torch, (3, 2, 64), torch.float32, -77.0)]
    ws = _Guarded(torch, (c.need["md_best_mappings"],), torch.uint8, 0x5A)
    got = _call(c, "md_best_mappings", out=tuple(g.t for g in out), workspace=ws.t)
    assert all(r is g.t for r, g in zip(got, out)) and all(g.untouched() for g in out + [ws])
    assert _same(got, bm.best_mappings(_np(c.md_scores), c.cand, c.mat_off))


# ------------------------------------------------------------------ 5. the second launch beyond the cap ---
@pytest.fixture
def launches(c, monkeypatch):
    """Counts the library calls by name: every entry point's return code goes through ops.check(rc, name)."""
    seen = []
    inner = c.ops.check
    monkeypatch.setattr(c.ops, "check", lambda rc, what: (seen.append(what), inner(rc, what))[1])
    return seen


def test_threshold_edges_launches_again_only_beyond_its_cap(c, launches):
    want = _edge_set(_call(c, "threshold_edges"))
    assert launches == ["ms_threshold_edges"] and len(want) == 10
    for cap, expected in ((0, 2), (len(want) - 1, 2), (len(want), 1), (len(want) + 1, 1)):
        del launches[:]
        stats = {}
        result = _call(c, "threshold_edges", cap=cap, stats=stats)
        assert _edge_set(result) == want and result[3] == len(want) and "rescored" in stats
        assert launches == ["ms_threshold_edges"] * expected, cap


@pytest.mark.parametrize("route", ["lane", "matrix"])
def test_md_chain_scan_launches_again_only_beyond_its_cap(c, launches, route):
    entry = "ms_md_chain_scan" if route == "lane" else "ms_md_chain_scan_mq"
    kw = dict(route=route, row_norm_bound=None if route == "lane" else BOUND)
    want = _call(c, "md_chain_scan", **kw)
    assert launches == [entry] and len(want[0]) == 4
    for cap, expected in ((0, 2), (3, 2), (4, 1), (5, 1)):
        del launches[:]
        stats = {}
        assert _same(_call(c, "md_chain_scan", cap=cap, stats=stats, **kw), want) and stats["route"] == route
        assert launches == [entry] * expected, cap
