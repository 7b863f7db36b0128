"""The prefilter's error bound on worst-case rows (tests/pf_adversarial.py), on the GPU.

The prefiltered search is exact only if |a - s| <= E |row||q| holds for every row (csrc/ms_search.hip, ms_rescore_body).  These
tests check what `a` is made of and how far it strays:
  * the images bit for bit against the numpy model (ties to even, fp16 subnormals, the +-65504 clamp, partial tiles, the trailer);
  * on rows that push one budget term to its limit, planted among random rows: for every candidate the scan kept, the matrix pipe's
    own accumulation |a_kernel - a_model| <= (products) x 2^-23 |row||q|, the rounding terms |a_model - s| within their budget, and
    the whole |a_kernel - s| <= E;
  * end to end: near-ties planted so that every decoy out-ranks the true answer on `a` -- a sound E flags those queries and the
    exact pass returns the oracle's answer; an E below 0.85 rho would accept a wrong one.
The fp16 conversion keeps subnormals (the build sets no flush-to-zero mode), so the images must match the model with no
deviation at all."""
import ctypes

import numpy as np
import pytest

import pf_adversarial as pa

pytestmark = pytest.mark.gpu

FMT = {"f16x2": pa.PF_F16X2, "f16x1": pa.PF_F16X1, "bf16x3": pa.PF_BF16X3}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    from merizo_search_amd import _lib
    _lib.require_gpu()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the images against the model -----------------------------------------------------------------------------------
def _special_rows(rng, n, bound):
    """n rows of norm ~0.9 bound, the first ones full of edge values placed in the fp16 image's scaled domain."""
    sr = pa.f16_sr(bound)
    down = np.float32(2.0 ** -sr)
    db = rng.standard_normal((n, pa.DIM)).astype(np.float32)
    db = (db / np.linalg.norm(db, axis=1, keepdims=True) * np.float32(0.9 * bound)).astype(np.float32)
    h = np.sort(rng.integers(0x0400, 0x7800, size=64, dtype=np.uint16)).view(np.float16).astype(np.float32)  # fp16 normals
    nxt = np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float32)
    mids = (h + nxt) / 2                                                            # exact in fp32: ties to even
    sub = rng.integers(1, 0x0400, size=64, dtype=np.uint16).view(np.float16).astype(np.float32)
    sub_mid = sub + np.float32(2.0 ** -25)                                          # midpoints between fp16 subnormals
    scaled = [np.zeros(8, np.float32), -np.zeros(8, np.float32), mids, -mids, np.nextafter(mids, np.float32(np.inf)),
              np.nextafter(mids, np.float32(0)), sub, -sub_mid, sub_mid, np.nextafter(sub_mid, np.float32(0)),
              rng.uniform(-2.0 ** -14, 2.0 ** -14, 64).astype(np.float32)]
    vals = np.concatenate([np.concatenate(scaled) * down,
                           np.array([1e-40, -1e-45, 1.1754942e-38, -3e-39], np.float32)])       # fp32 subnormals, unscaled
    m = min(n, (vals.size + pa.DIM - 1) // pa.DIM)
    flat = db[:m].reshape(-1)
    flat[:vals.size] = vals[:flat.size]
    db[:m] = flat.reshape(m, pa.DIM)
    return db


@pytest.mark.parametrize("bound", [2.0 ** -40, 2.0 ** 40, 1.0, 3.7])
@pytest.mark.parametrize("n", [1, 31, 33, 63, 65, 70_001])
def test_fp16_image_equals_the_model_bit_for_bit(n, bound, torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    db = _special_rows(np.random.default_rng(n), n, bound)
    img = ops.pf_build_image(_dev(torch, db), fmt=ops.PF_F16X2, row_norm_bound=bound)
    got = img.data.cpu().numpy()
    want = pa.f16_image(db, bound)
    assert got.size >= want.size
    bad = np.flatnonzero(got[:want.size] != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def test_fp16_image_clamps_rows_whose_bound_is_understated(torch_gpu):
    """A bound 4x too small: components up to 2^16 after scaling land on +-65504, never on inf."""
    torch = torch_gpu
    from merizo_search_amd import ops
    bound = 1.0
    db = _special_rows(np.random.default_rng(4), 200, bound)
    db[:100] *= np.float32(4.0 / 0.9)
    db[100, :8] = np.array([65504, 65505, 65519, 65520, 65536, -65520, -65519.99, 70000], np.float32) * np.float32(2.0 ** -14)
    want = pa.f16_image(db, bound)
    assert np.sum(np.abs(pa.f16_values(db, bound).astype(np.float32)) == 65504) >= 8
    got = ops.pf_build_image(_dev(torch, db), fmt=ops.PF_F16X2, row_norm_bound=bound).data.cpu().numpy()
    assert np.array_equal(got[:want.size], want)


@pytest.mark.parametrize("n", [1, 31, 33, 63, 65, 70_001])
def test_split_bf16_image_equals_the_model_bit_for_bit(n, torch_gpu):
    torch = torch_gpu
    from merizo_search_amd import ops
    rng = np.random.default_rng(100 + n)
    db = _special_rows(rng, n, 1.0)
    if n > 3:                            # significands with their low bits all ones, both signs
        db[2] = np.float32(1.0 + (2.0 ** 16 - 1) * 2.0 ** -23) * np.where(np.arange(pa.DIM) % 2, 1, -1).astype(np.float32)
    img = ops.pf_build_image(_dev(torch, db), fmt=ops.PF_BF16X3)
    got = img.data.cpu().numpy()
    want = pa.bf16_image(db)
    bad = np.flatnonzero(got[:want.size] != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}"


# ---- 2. the error terms, measured against float64 -----------------------------------------------------------------------
KINDS = ["row_down", "row_up", "f16x1_query", "bf16_trunc", "underflow", "accumulation"]
BOUND = 1.0 + 2.0 ** -10         # >= every generator's row norm; sr = 14


def _planted(kind, seed, m, fmt):
    if kind == "row_down":
        return pa.f16_row_rounding(seed, m, -1)
    if kind == "row_up":
        return pa.f16_row_rounding(seed, m, +1)
    if kind == "f16x1_query":
        return pa.f16x1_query_rounding(seed, m)
    if kind == "bf16_trunc":
        return pa.bf16_truncation(seed, m)
    if kind == "underflow":
        return pa.query_underflow(seed, m)
    q, rows, _ = pa.accumulation(seed, m, fmt if fmt is not None else pa.PF_BF16X3)
    return q, rows


def _case(torch, n, nq, seed, fmt, per_query=3):
    """Random rows of norm 0.25 (on the GPU), and per query one adversarial query with `per_query` rows of its own planted."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    d = torch.randn((n, pa.DIM), generator=g, device="cuda")
    d = d / d.norm(dim=1, keepdim=True) * 0.25
    rng = np.random.default_rng(seed)
    slots = rng.choice(n, size=nq * per_query, replace=False)
    qs, kinds = [], []
    for j in range(nq):
        kind = KINDS[j % len(KINDS)]
        q, rows = _planted(kind, seed * 1000 + j, per_query, fmt)
        d[torch.from_numpy(slots[j * per_query:(j + 1) * per_query]).cuda()] = _dev(torch, rows)
        qs.append(q)
        kinds.append(kind)
    return d.contiguous(), np.stack(qs).astype(np.float32), kinds


def _lists(ops, ws, n, nq, k, image_code):
    from merizo_search_amd import _lib
    a_s = np.zeros((nq, 64), np.float32)
    a_i = np.zeros((nq, 64), np.int64)
    kp = ctypes.c_int(0)
    rc = _lib.load().ms_debug_prefilter_lists(ws.data_ptr(), n, nq, k, image_code, a_s.ctypes.data, a_i.ctypes.data, ctypes.byref(kp))
    assert rc == 0
    kp = kp.value
    return a_s.reshape(-1)[:nq * kp].reshape(nq, kp), a_i.reshape(-1)[:nq * kp].reshape(nq, kp)


def _kernel_query(q_raw):
    """The fp16 scan's own normalisation of a raw query (a few ulp from the exact one: the 4.8e-7 term)."""
    q = np.asarray(q_raw, np.float32)
    rinv = np.float32(1.0) / np.float32(max(np.sqrt(np.float32(np.sum(q.astype(np.float64) ** 2))), np.float32(1e-12)))
    return (q * rinv).astype(np.float32)


def _measure(torch, ops, n, nq, k, fmt_name, raw=False, seed=1):
    fmt = FMT.get(fmt_name)
    d, q, kinds = _case(torch, n, nq, seed, fmt)
    q_in = (q * np.float32(2.7)).astype(np.float32) if raw else q
    dq = _dev(torch, q_in)
    img = ops.pf_build_image(d, fmt=fmt, row_norm_bound=BOUND) if fmt is not None else None
    assert ops.prefilter_serves(n, nq, k, fmt)
    ws = ops.PrefilterWorkspace(d.device).get(n, nq, k)
    mode = ops.MODE_IP_NORMQ if raw else ops.MODE_IP_PRENORM
    s, i = ops.ip_topk_prefiltered(d, dq, k, BOUND, mode=mode, workspace=ws, image=img)
    s0, i0 = ops.ip_topk(d, dq, k, mode=mode)
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
    a_s, a_i = _lists(ops, ws, n, nq, k, 0 if fmt is None else (1 if fmt == pa.PF_BF16X3 else 2))
    qn = ops.l2_normalize_rows(dq, 1e-12).cpu().numpy() if raw else q         # what the exact chain multiplies
    model_fmt = pa.PF_BF16X3 if fmt is None else fmt
    # what the scan multiplies: the fp16 scan normalises raw queries itself; the bf16 paths take the prepared copy (= qn)
    qs = np.stack([_kernel_query(x) for x in q_in]) if (raw and fmt in (pa.PF_F16X2, pa.PF_F16X1)) else qn
    slack = 4.8e-7 if (raw and fmt in (pa.PF_F16X2, pa.PF_F16X1)) else 0.0
    E = ops.pf_err_coef(model_fmt)
    worst = {}
    for j in range(nq):
        ok = a_i[j] >= 0
        assert ok.all(), "a full candidate list"
        rows = d[torch.from_numpy(a_i[j]).cuda()].cpu().numpy()
        am = pa.a_model(rows, qs[j], model_fmt, BOUND)
        s64 = pa.exact(rows, qn[j])
        sc = pa.scale_of(rows, qn[j])
        ak = a_s[j].astype(np.float64)
        pipe = np.abs(ak - am) / sc
        rnd = np.abs(am - s64) / sc
        tot = np.abs(ak - s64) / (BOUND * np.linalg.norm(qn[j].astype(np.float64)))
        w = worst.setdefault(kinds[j], [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], pipe.max()), max(w[1], rnd.max()), max(w[2], tot.max())
        msg = f"{fmt_name} query {j} ({kinds[j]}): pipe {pipe.max():.3e} rounding {rnd.max():.3e} total {tot.max():.3e} (E {E:.3e})"
        assert pipe.max() <= pa.PRODUCTS[model_fmt] * pa.U23 + slack, msg
        assert rnd.max() <= pa.ROUNDING_BUDGET[model_fmt] + slack, msg
        assert tot.max() <= E, msg
    report = "; ".join(f"{kd}: pipe {w[0] / pa.U23:.1f} x 2^-23, rounding {w[1]:.3e}, total {w[2]:.3e} = {w[2] / E:.2f} E"
                       for kd, w in worst.items())
    print(f"[{fmt_name}, n={n}, nq={nq}, raw={raw}] {report}")
    return worst


@pytest.mark.parametrize("fmt_name", ["f16x2", "f16x1", "bf16x3", None])
@pytest.mark.parametrize("nq", [72, 300])
def test_error_terms_on_worst_case_rows_many_queries(nq, fmt_name, torch_gpu):
    from merizo_search_amd import ops
    worst = _measure(torch_gpu, ops, 65_536 + 17, nq, 10, fmt_name, seed=nq)
    if fmt_name in ("f16x2", "f16x1"):      # the row term was reached, not only bounded
        assert max(worst["row_down"][1], worst["row_up"][1]) >= 0.9 * pa.U11
    if fmt_name == "f16x1":
        assert worst["f16x1_query"][1] >= 0.9 * 2 * pa.U11
    if fmt_name in ("bf16x3", None):
        assert worst["bf16_trunc"][1] >= 0.9 * 2.0 ** -13


@pytest.mark.parametrize("fmt_name", ["f16x2", "bf16x3", None])
def test_error_terms_with_raw_queries_normalised_in_the_scan(fmt_name, torch_gpu):
    """MS_MODE_IP_NORMQ: the fp16 scan normalises the raw query itself (q * (1 / |q|), a few ulp from F.normalize's).  F16X1 is left
    out: there an ulp of difference can move a component of the query across an fp16 midpoint, which the model cannot follow."""
    from merizo_search_amd import ops
    _measure(torch_gpu, ops, 70_000, 96, 10, fmt_name, raw=True, seed=7)


@pytest.mark.parametrize("fmt_name", ["f16x2", "f16x1"])
@pytest.mark.parametrize("n,nq", [(1_000_000, 1), (1_000_000, 8), (1_000_000, 32), (200_000, 33), (200_000, 64)])
def test_error_terms_on_the_few_query_fp16_path(n, nq, fmt_name, torch_gpu):
    from merizo_search_amd import ops
    assert not ops.prefilter_serves(n, nq, 10) and ops.prefilter_serves(n, nq, 10, FMT[fmt_name])
    _measure(torch_gpu, ops, n, nq, 10, fmt_name, seed=nq + 3)


# ---- 3. the proof against a planted wrong answer ------------------------------------------------------------------------
def _near_tie_case(torch, n, nq, k, kp, seed, control, mode):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    d = torch.randn((n, pa.DIM), generator=g, device="cuda")
    d = d / d.norm(dim=1, keepdim=True) * (1.0 - 1e-6)
    rng = np.random.default_rng(seed)
    fam = [pa.near_tie_family(seed * 1000 + j, k, kp, control) for j in range(nq)]
    per = max(f[1].shape[0] + f[2].shape[0] + f[3].shape[0] for f in fam)
    slots = rng.choice(n, size=nq * per, replace=False)
    planted = []
    for j, (q, T, U, L) in enumerate(fam):
        rows = np.concatenate([T, U, L])
        idx = slots[j * per: j * per + rows.shape[0]]
        d[torch.from_numpy(idx).cuda()] = _dev(torch, rows)
        planted.append(idx[:T.shape[0]])
    q = np.stack([f[0] for f in fam])
    lengths = qlen = None
    if mode == "cosine":
        lengths = rng.integers(40, 400, size=n).astype(np.float32)
        lengths[slots] = 100.0                                     # the planted rows pass the mask at any mincov <= 1
        qlen = np.full(nq, 100.0, np.float32)
    return d.contiguous(), q, planted, lengths, qlen


@pytest.mark.parametrize("control", [False, True])
@pytest.mark.parametrize("fmt_name", ["f16x2", "f16x1"])
@pytest.mark.parametrize("k", [5, 10, 24, 48])
@pytest.mark.parametrize("n,nq,mode,mincov", [(65_536, 72, "ip", 0.0), (1_000_000, 8, "ip", 0.0), (200_000, 33, "raw", 0.0),
                                              (65_536, 80, "cosine", 0.0), (65_536, 80, "cosine", 0.7)])
def test_the_proof_flags_near_ties_that_rank_the_true_answer_out(n, nq, mode, mincov, k, fmt_name, control, torch_gpu):
    """For every query: k true rows T (exact S, rounded down: a = S - rho), k upper decoys U (S - 0.05 rho, rounded up) and kp - k lower
    decoys L (S - 1.9 rho, rounded up), rho ~ 2^-11 |row||q| (the row term; the queries are exact in fp16, so this is all of it for
    both fp16 formats).  The candidates are U and L; a proof with E >= 0.85 rho must fail for every query and the exact pass must
    return T, bit for bit as the oracle.  Control: T and L only, L 2^-7 below -- the proof must pass for every query, same answers."""
    torch = torch_gpu
    from merizo_search_amd import ops
    from oracle import oracle as orc
    fmt = FMT[fmt_name]
    bound = 1.0 + 1e-5 if mode == "cosine" else 1.0 + 1e-6
    kp = {5: 10, 10: 20, 24: 32, 48: 64}[k]
    d, q, planted, lengths, qlen = _near_tie_case(torch, n, nq, k, kp, seed=k * 7 + nq, control=control, mode=mode)
    assert ops.prefilter_serves(n, nq, k, fmt)
    img = ops.pf_build_image(d, fmt=fmt, row_norm_bound=bound)
    ws = ops.PrefilterWorkspace(d.device).get(n, nq, k)
    kw = {}
    if mode == "cosine":
        kw = dict(mode=ops.MODE_COSINE_UNIT, lengths=_dev(torch, lengths), qlen=_dev(torch, qlen), mincov=mincov)
    else:
        kw = dict(mode=ops.MODE_IP_NORMQ if mode == "raw" else ops.MODE_IP_PRENORM)
    dq = _dev(torch, q)             # (|q| = 1 exactly: a raw query normalises to itself)
    s, i = ops.ip_topk_prefiltered(d, dq, k, bound, workspace=ws, image=img, **kw)
    flagged = ops.prefilter_flagged(ws)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    db = d.cpu().numpy()
    if mode == "cosine":        # (the rows are unit only to 0.3 %: the fp32 scan of the same mode, which the suite pins to the oracle)
        s0, i0 = ops.ip_topk(d, dq, k, **kw)
        s_ref, i_ref = s0.cpu().numpy(), i0.cpu().numpy()
    else:
        s_ref, i_ref = orc.ip_topk(db, q, k, order=1)
    assert np.array_equal(i, i_ref), "the prefiltered answer is not the oracle's"
    assert np.array_equal(s.view(np.uint32), s_ref.view(np.uint32))
    for j in range(nq):                     # float64 ranking: the true rows, up to ties within 2e-6
        ex = pa.exact(db[i[j]], q[j])
        assert np.all(np.abs(ex - s[j]) <= 2e-6)
        assert sorted(i[j].tolist()) == sorted(planted[j].tolist()), f"query {j}: the answer is not the planted true rows"
    if control:
        assert flagged == 0, f"{flagged} queries flagged with the true rows among the candidates"
    else:
        assert flagged >= nq, f"only {flagged} of {nq} near-tie queries flagged (E = {ops.pf_err_coef(fmt):.3e})"
