"""ms_md_chain_scores on the GPU against its restatement (multidom_case.chain_scores_ref: a true fmaf chain per cell), bit for
bit: out_scores compared as uint32, out_match exactly, guard zones around the outputs and the workspace.  Test 1 anchors the
cell score to the product's own scan without the restatement; the others use queries prepared by the scan's normalisation
(ops.l2_normalize_rows with the mode's eps -- the arithmetic ms_ip_topk documents as bit-identical to its own)."""
import numpy as np
import pytest

import multidom_case as mc

pytestmark = pytest.mark.gpu
NINF = -np.inf
GUARD = 1024                          # floats / int32s (4 KB) in front of and behind every output
FILL_S, FILL_M, FILL_W = np.float32(-123.25), np.int32(-77), 0xAB
MODES = ("prenorm", "normq", "unit")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mode_code(mode):
    from merizo_search_amd import _lib
    return {"prenorm": _lib.MODE_IP_PRENORM, "normq": _lib.MODE_IP_NORMQ, "unit": _lib.MODE_COSINE_UNIT}[mode]


def _prepared(q, mode):
    """The queries as the scan of the mode multiplies them."""
    import torch
    from merizo_search_amd import ops
    if mode == "prenorm":
        return np.array(q, np.float32)
    return ops.l2_normalize_rows(torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda(), 1e-12 if mode == "normq" else 1e-8).cpu().numpy()


def _unit_rows(raw):
    import torch
    from merizo_search_amd import ops
    return ops.l2_normalize_rows_(torch.from_numpy(np.ascontiguousarray(raw, np.float32)).cuda(), 1e-8).cpu().numpy()


def _layout(cand, rng=None):
    """mat_off of candidates packed back to back (with random gaps of 0..7 floats when rng is given) -> (mat_off, total)."""
    off, at = np.zeros(len(cand), np.int64), 0
    for c, (_q0, nqd, _t, nhd) in enumerate(cand):
        if rng is not None:
            at += int(rng.integers(0, 8))
        off[c] = at
        at += max(int(nqd), 0) * max(int(nhd), 0)
    return off, at + (3 if rng is not None else 0)


def _gpu(db, q, mode, cand, trows, mat_off, min_score, total, lengths=None, qlen=None, mincov=0.0):
    """One call with guard zones -> (scores [total], match [ncand,2]) after checking that the guards kept their fill."""
    import torch
    from merizo_search_amd import _lib, ops
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    ncand = len(cand)
    big_s = torch.full((2 * GUARD + total,), float(FILL_S), dtype=torch.float32, device=dev)
    big_m = torch.full((2 * GUARD + 2 * ncand,), int(FILL_M), dtype=torch.int32, device=dev)
    need = int(_lib.load().ms_md_chain_scores_workspace_bytes(len(q)))
    big_w = torch.full((8192 + need,), FILL_W, dtype=torch.uint8, device=dev)
    out = (big_s[GUARD: GUARD + total], big_m[GUARD: GUARD + 2 * ncand].view(ncand, 2))
    ops.md_chain_scores(t(db, np.float32), t(q, np.float32), _mode_code(mode), t(np.asarray(cand).reshape(-1, 4), np.int32), t(trows, np.int64),
                        t(mat_off, np.int64), min_score, lengths=None if lengths is None else t(lengths, np.float32),
                        qlen=None if qlen is None else t(qlen, np.float32), mincov=mincov, out=out, workspace=big_w[4096: 4096 + need])
    torch.cuda.synchronize()
    s, m, w = big_s.cpu().numpy(), big_m.cpu().numpy(), big_w.cpu().numpy()
    assert (_bits(s[:GUARD]) == _bits(FILL_S)).all() and (_bits(s[GUARD + total:]) == _bits(FILL_S)).all(), "guard zone of out_scores"
    assert (m[:GUARD] == FILL_M).all() and (m[GUARD + 2 * ncand:] == FILL_M).all(), "guard zone of out_match"
    assert (w[:4096] == FILL_W).all() and (w[4096 + need:] == FILL_W).all(), "guard zone of the workspace"
    return s[GUARD: GUARD + total].copy(), m[GUARD: GUARD + 2 * ncand].reshape(ncand, 2).copy()


def _check(db, q, mode, cand, trows, mat_off, min_score, total, lengths=None, qlen=None, mincov=0.0, what=None):
    cand = np.asarray(cand, np.int64).reshape(-1, 4)
    s, m = _gpu(db, q, mode, cand, trows, mat_off, min_score, total, lengths, qlen, mincov)
    want_s, want_m = mc.chain_scores_ref(db, _prepared(q, mode), cand, trows, mat_off, min_score, np.full(total, FILL_S, np.float32),
                                         np.full((len(cand), 2), FILL_M, np.int32), lengths, qlen, mincov)
    assert np.array_equal(m, want_m), (what, m[(m != want_m).any(axis=1)][:5], want_m[(m != want_m).any(axis=1)][:5])
    bad = np.flatnonzero(_bits(s) != _bits(want_s))
    assert bad.size == 0, (what, bad[:5], s[bad[:5]], want_s[bad[:5]])
    return s, m


def _data(n, nq, seed, mode):
    """Random rows and queries for a mode: unit rows (the faiss layout's, the resident `.pt` rows), raw queries unless the
    mode takes them as given; `unit` also gets lengths with the mask's edge among them (mincov 0.5: qlen 30 against 60)."""
    rng = np.random.default_rng(seed)
    db = _unit_rows(rng.standard_normal((n, 128)).astype(np.float32) * rng.uniform(0.5, 3.0, (n, 1)).astype(np.float32))
    q = rng.standard_normal((nq, 128)).astype(np.float32) * rng.uniform(0.5, 3.0, (nq, 1)).astype(np.float32)
    if mode == "prenorm":
        q = _unit_rows(q)
    extra = {}
    if mode == "unit":
        extra = dict(lengths=rng.choice([40, 60, 61, 80], n).astype(np.float32), qlen=rng.choice([20, 30, 40], nq).astype(np.float32), mincov=0.5)
    return db, q, extra, rng


# ------------------------------------------------------------------ 1. against the product's own scan ---
@pytest.mark.parametrize("mode", MODES)
def test_cells_equal_the_scores_of_ip_topk_bit_for_bit(mode):
    """n = 300, 40 queries in chains, one candidate per chain over ALL rows, no cut: the matrices are ops.ip_topk(k = n)
    scattered by row -- the search's own emb_score for every (query, row), masked scores included."""
    import torch
    from merizo_search_amd import ops
    n, nq = 300, 40
    db, q, extra, _rng = _data(n, nq, 7, mode)
    runs = [1, 2, 3, 5, 7, 4, 6, 8, 4]
    assert sum(runs) == nq
    cand = np.array([(sum(runs[:c]), r, 0, n) for c, r in enumerate(runs)], np.int64)
    mat_off, total = _layout(cand)
    s, m = _gpu(db, q, mode, cand, np.arange(n), mat_off, NINF, total, **extra)
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    ts, ti = ops.ip_topk(cu(db), cu(q), n, mode=_mode_code(mode), lengths=cu(extra.get("lengths")), qlen=cu(extra.get("qlen")),
                         mincov=extra.get("mincov", 0.0))
    ts, ti = ts.cpu().numpy(), ti.cpu().numpy()
    assert (np.sort(ti, axis=1) == np.arange(n)).all()
    want = np.zeros((nq, n), np.float32)
    np.put_along_axis(want, ti, ts, axis=1)
    assert np.array_equal(_bits(s), _bits(want.reshape(-1)))
    if mode == "unit":
        assert (want == 0).any() and (want != 0).any()                  # the mask cut some pairs and kept others
    for c, (q0, nqd, _t, _nhd) in enumerate(cand):
        assert tuple(m[c]) == mc.match_counts(want[q0: q0 + nqd])


# ------------------------------------------------------------------ 2. shapes ------------------------------
NQD, NHD = (1, 2, 3, 7, 33), (1, 2, 5, 63, 64, 65, 200)


@pytest.mark.parametrize("matrix", ["compact", "large"])
@pytest.mark.parametrize("mode", MODES)
def test_every_shape_below_at_and_beyond_one_stride(mode, matrix):
    """nqd x nhd from 1 cell to 6,600, one candidate each in ONE call: over a compact matrix (trows = 0, 1, ...) and over
    n = 5,000 rows named in scattered order with repeats.  With a cut in the middle of the scores, and without one."""
    n = 200 if matrix == "compact" else 5000
    shapes = [(a, b) for a in NQD for b in NHD]
    nq = sum(a for a, _b in shapes)
    db, q, extra, rng = _data(n, nq, 21 + len(mode), mode)
    cand, trows, q0 = [], [], 0
    for nqd, nhd in shapes:
        cand.append((q0, nqd, len(trows), nhd))
        trows.extend(range(nhd) if matrix == "compact" else rng.integers(0, n, nhd).tolist())
        q0 += nqd
    if matrix == "large":
        trows[5] = trows[4]                                             # a row named twice next to itself
    mat_off, total = _layout(cand)
    for cutoff in (np.float32(0.05), NINF):
        s, m = _check(db, q, mode, cand, trows, mat_off, cutoff, total, what=(mode, matrix, cutoff), **extra)
        if cutoff > 0:
            assert (s == 0).any() and (s != 0).any() and (m[:, 0] < np.array([a for a, _b in shapes])).any()


# ------------------------------------------------------------------ 3. the cut -----------------------------
def test_the_cut_keeps_equal_scores_and_zeroes_nan_rows():
    """0.5 e3 . 0.25 e3 = 0.125 exactly: a cut equal to it keeps it, one ulp above zeroes it, one ulp below keeps it.  A NaN in
    a query: every cell of its row is +0.0.  A masked negative cosine is -0.0: stored as is, counted as zero."""
    db = np.zeros((4, 128), np.float32)
    db[0, 3], db[1, 3], db[2, 70], db[3, 3] = 0.25, -0.25, 1.0, 0.5
    q = np.zeros((3, 128), np.float32)
    q[0, 3], q[1, 3], q[1, 100], q[2, 70] = 0.5, 0.5, np.nan, 2.0
    cand, trows = [(0, 3, 0, 4)], [0, 1, 2, 3]
    exact = np.float32(0.125)
    for cutoff, kept in ((exact, True), (np.nextafter(exact, np.float32(1)), False), (np.nextafter(exact, np.float32(0)), True)):
        s, m = _check(db, q, "prenorm", cand, trows, [0], cutoff, 12, what=cutoff)
        s = s.reshape(3, 4)
        assert _bits(s[0, 0]) == (_bits(exact) if kept else 0) and s[0, 3] == np.float32(0.25) and s[2, 2] == np.float32(2.0)
        assert (_bits(s[1]) == 0).all() and _bits(s[0, 1]) == 0         # the NaN row; -0.125 is below the cut
        assert tuple(m[0]) == (2, 3 if kept else 2)
    s, m = _check(db, q, "prenorm", cand, trows, [0], NINF, 12)
    assert (_bits(s.reshape(3, 4)[1]) == 0).all() and s[1] == np.float32(-0.125) and tuple(m[0]) == (2, 4)
    # MS_MODE_COSINE_UNIT: query -2 e5 against the unit row e5 scores -1; masked (qlen 10 < 100 * 0.7) it is -1 * 0 = -0.0
    db = np.zeros((2, 128), np.float32)
    db[0, 5] = db[1, 6] = 1.0
    q = np.zeros((2, 128), np.float32)
    q[0, 5], q[1, 6] = -2.0, 3.0
    for cutoff in (NINF, np.float32(0.0)):
        s, m = _check(db, q, "unit", [(0, 1, 0, 1), (1, 1, 1, 1)], [0, 1], [0, 1], cutoff, 2, lengths=[100, 100], qlen=[10, 90], mincov=0.7)
        assert _bits(s[0]) == 0x80000000 and s[1] == np.float32(1.0) and m.tolist() == [[0, 0], [1, 1]]


# ------------------------------------------------------------------ 4. match counts ------------------------
def test_match_counts_of_planted_patterns():
    """One-hot queries and rows: cell (i, j) is 1 where they share their dimension, else 0."""
    e = np.eye(128, dtype=np.float32)
    ones = np.full(128, 0.125, np.float32)
    db = np.stack([e[0], e[1], e[2], e[3], e[0], ones])
    #   queries: a zero row | two queries on one column | exactly nqd columns | all cells non-zero
    q = np.stack([e[0], e[9], e[1],   e[0], e[0], e[1],   e[2], e[1], e[0],   ones, ones])
    cand = [(0, 3, 0, 4), (3, 3, 0, 4), (6, 3, 0, 4), (9, 2, 5, 1), (3, 2, 0, 5)]
    mat_off, total = _layout(cand)
    s, m = _check(db, q, "prenorm", cand, [0, 1, 2, 3, 4, 5], mat_off, np.float32(0.5), total)
    assert m.tolist() == [[2, 2], [3, 2], [3, 3], [2, 1], [2, 2]]
    assert s[mat_off[2]: mat_off[2] + 12].reshape(3, 4).tolist() == [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]]
    keep = lambda c: m[c, 0] == cand[c][1] and m[c, 1] >= cand[c][1]    # the host's test = chain_mappings' two early exits
    assert [bool(keep(c)) for c in range(5)] == [False, False, True, False, True]


# ------------------------------------------------------------------ 5. many candidates ---------------------
@pytest.fixture(scope="module")
def many():
    n, nq, ncand = 5000, 700, 3000
    db, q, extra, rng = _data(n, nq, 99, "normq")
    cand, trows = [], []
    for c in range(ncand):
        nqd, nhd = (40, 100) if c % 500 == 7 else (int(rng.integers(1, 6)), int(rng.integers(1, 9)))
        cand.append((int(rng.integers(0, nq - nqd + 1)), nqd, len(trows), nhd))
        first = int(rng.integers(0, n - nhd))
        trows.extend(range(first, first + nhd))                          # a chain: adjacent rows
    mat_off, total = _layout(cand, rng)
    return db, q, np.asarray(cand, np.int64), np.asarray(trows, np.int64), mat_off, total


def test_many_candidates_gaps_and_guard_zones(many):
    """3,000 candidates of random small shapes and six of 40 x 100, matrices laid out with gaps: the gaps and the 4 KB around
    out_scores, out_match and the workspace keep their fill pattern (the restatement starts from the same fill)."""
    db, q, cand, trows, mat_off, total = many
    s, m = _check(db, q, "normq", cand, trows, mat_off, np.float32(0.1), total)
    assert (_bits(s) == _bits(FILL_S)).sum() >= 3 and (m >= 0).all()
    s2, m2 = _gpu(db, q, "normq", cand, trows, mat_off, np.float32(0.1), total)
    assert np.array_equal(_bits(s), _bits(s2)) and np.array_equal(m, m2)         # run to run


# ------------------------------------------------------------------ 6. descriptors the kernel must ignore --
def test_bad_descriptors_write_what_the_header_defines_and_nothing_else():
    """Rows outside [0, n) are never read (their cells are +0.0); candidates that leave the queries or the row list, or name no
    cell, get {-1, -1} and nothing else -- the floats they point at keep their fill."""
    n, nq = 50, 12
    db, q, _extra, _rng = _data(n, nq, 5, "prenorm")
    trows = [3, -1, 7, n, 1 << 40, 9, -(1 << 40), n - 1]
    cand = [(0, 3, 0, 8),              # good, with five rows outside the database
            (10, 3, 0, 2),             # q0 + nqd > nq
            (0, 2, 6, 3),              # t_off + nhd > ntrows
            (4, 0, 0, 2),              # nqd = 0
            (4, 2, 0, 0),              # nhd = 0
            (-1, 2, 0, 2), (0, 2, -3, 2), (0, -2, 0, 2), (2147483647, 2, 0, 2), (0, 2, 2147483647, 2), (0, 5000, 0, 2),
            (9, 3, 5, 3)]              # good, at the very end of both
    mat_off = np.arange(len(cand), dtype=np.int64) * 32
    total = 32 * len(cand)
    s, m = _check(db, q, "prenorm", cand, trows, mat_off, NINF, total)
    assert m[1:11].tolist() == [[-1, -1]] * 10 and (m[[0, 11]] >= 0).all()
    first = s[:24].reshape(3, 8)
    assert (_bits(first[:, [1, 3, 4, 6]]) == 0).all() and (first[:, [0, 2, 5, 7]] != 0).all()
    assert (_bits(s[32: 32 * 11]) == _bits(FILL_S)).all()


# ------------------------------------------------------------------ 7. return codes ------------------------
def test_return_codes_on_the_device():
    import torch
    from merizo_search_amd import _lib, ops
    db, q, _extra, _rng = _data(20, 4, 3, "prenorm")
    d, qq = torch.from_numpy(db).cuda(), torch.from_numpy(q).cuda()
    cand, trows, off = np.array([[0, 2, 0, 3]], np.int32), np.arange(3), np.zeros(1, np.int64)
    s, m = ops.md_chain_scores(d, qq, _lib.MODE_IP_PRENORM, np.zeros((0, 4), np.int32), trows, np.zeros(0, np.int64), NINF)
    assert s.numel() == 0 and tuple(m.shape) == (0, 2)
    s, m = ops.md_chain_scores(d, qq, _lib.MODE_IP_PRENORM, cand, trows, off, NINF)
    assert s.numel() == 6 and m.cpu().tolist() == [[2, 3]]
    for kw, code in ((dict(mode=_lib.MODE_COSINE_RAW), "(-1)"), (dict(min_score=float("nan")), "(-1)"),
                     (dict(workspace=torch.empty(4 * 512 - 16, dtype=torch.uint8, device="cuda")), "(-2)")):
        args = dict(mode=_lib.MODE_IP_PRENORM, min_score=NINF, workspace=None)
        args.update(kw)
        with pytest.raises(_lib.MerizoHipError) as exc:
            ops.md_chain_scores(d, qq, args["mode"], cand, trows, off, args["min_score"], workspace=args["workspace"])
        assert code in str(exc.value) and "ms_md_chain_scores" in str(exc.value)
    lib = _lib.load()
    ws = torch.empty(4 * 512, dtype=torch.uint8, device="cuda")
    import ctypes
    rc = lib.ms_md_chain_scores(d.data_ptr(), 20, qq.data_ptr(), 4, _lib.MODE_IP_PRENORM, None, None, ctypes.c_float(0.0), ws.data_ptr(), 0,
                                ws.data_ptr(), 0, ws.data_ptr(), ctypes.c_float(NINF), ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), 4 * 512, None)
    assert rc == 0                                                      # no candidates: success, nothing launched
    rc = lib.ms_md_chain_scores(d.data_ptr(), 20, None, 4, _lib.MODE_IP_PRENORM, None, None, ctypes.c_float(0.0), ws.data_ptr(), 1,
                                ws.data_ptr(), 3, ws.data_ptr(), ctypes.c_float(NINF), ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), 4 * 512, None)
    assert rc == -1 and b"NULL" in lib.ms_last_error()
