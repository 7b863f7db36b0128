"""CPU checks of tests/pf_adversarial.py: the numpy model of the prefilter's images and operands is self-consistent, and every
worst-case generator reaches at least 0.9 of the analytic value of the budget term it is built for -- through the model alone, so
that the GPU tests built on them (test_prefilter_bound_gpu.py) cannot pass without testing anything."""
import numpy as np
import pytest

import pf_adversarial as pa

FP16 = [pa.PF_F16X2, pa.PF_F16X1]


def _ratio(a, rows, q):
    return (a - pa.exact(rows, q)) / pa.scale_of(rows, q)


@pytest.mark.parametrize("side", [-1, 1])
@pytest.mark.parametrize("fmt", FP16)
def test_row_rounding_generator_reaches_the_fp16_row_term(side, fmt):
    q, rows = pa.f16_row_rounding(seed=11 + side, m=64, side=side)
    assert len({r.tobytes() for r in rows}) == 64
    r = _ratio(pa.a_model(rows, q, fmt), rows, q)
    assert np.all(np.sign(r) == side), "every row pushed the same way"
    assert np.abs(r).min() >= 0.9 * pa.U11, np.abs(r).min() / pa.U11
    assert np.abs(r).max() <= pa.ROUNDING_BUDGET[fmt]


def test_query_rounding_generator_reaches_twice_the_row_term_under_f16x1():
    q, rows = pa.f16x1_query_rounding(seed=3, m=64)
    r1 = _ratio(pa.a_model(rows, q, pa.PF_F16X1), rows, q)
    assert r1.max() <= -0.9 * 2 * pa.U11, r1.max() / pa.U11
    assert np.abs(r1).max() <= pa.ROUNDING_BUDGET[pa.PF_F16X1]
    # the two-part query absorbs the query's rounding: back to the row term alone
    r2 = _ratio(pa.a_model(rows, q, pa.PF_F16X2), rows, q)
    assert np.abs(r2).max() <= 1.01 * pa.U11


def test_truncation_generator_reaches_the_split_bf16_term():
    q, rows = pa.bf16_truncation(seed=5, m=64)
    assert len({r.tobytes() for r in rows}) == 64
    r = _ratio(pa.a_model(rows, q, pa.PF_BF16X3), rows, q)
    assert r.max() < 0, "truncation only ever loses"
    attainable = 2.0 ** -13              # (3 x 2^-14 in the budget: see the generator)
    assert -r.max() >= 0.9 * attainable, -r.max() / attainable
    assert -r.min() <= pa.ROUNDING_BUDGET[pa.PF_BF16X3]


@pytest.mark.parametrize("fmt", FP16)
def test_underflow_generator_reaches_the_flushed_query_term(fmt):
    q, rows = pa.query_underflow(seed=7, m=16)
    _, qh, _ = pa.f16_query(q, fmt)
    small = np.abs(qh.astype(np.float64)) < 2.0 ** -14
    assert small.sum() == 127 and np.all(qh[small] != 0), "127 components land in the fp16 subnormal range (and survive rounding)"
    flushed = np.abs(_ratio(pa.a_model(rows, q, fmt, flush=True), rows, q))
    assert flushed.min() >= 0.9 * pa.UNDERFLOW, flushed.min() / pa.UNDERFLOW
    kept = np.abs(_ratio(pa.a_model(rows, q, fmt), rows, q))
    assert kept.max() <= 2.0 ** -10 * pa.UNDERFLOW, "subnormals kept: only their own rounding is lost"
    cos = pa.exact(rows, q) / pa.scale_of(rows, q)
    assert cos.min() > 0.3, "the rows stay on top of their query"


@pytest.mark.parametrize("fmt", [pa.PF_F16X2, pa.PF_F16X1, pa.PF_BF16X3])
def test_accumulation_generator_loses_every_small_product_to_a_truncating_accumulator(fmt):
    q, rows, lead = pa.accumulation(seed=9, m=8, fmt=fmt)
    bound = 1.0 + 2.0 ** -10
    assert np.linalg.norm(rows.astype(np.float64), axis=1).max() <= bound
    assert len({r.tobytes() for r in rows}) == 8
    # the model's operands are the rows and queries themselves: no rounding term, everything left is the pipe's
    r = np.abs(_ratio(pa.a_model(rows, q, fmt, bound), rows, q))
    assert r.max() < 1e-7
    for row in rows:
        loss = pa.truncation_loss(row, q, fmt, lead, bound)
        assert loss >= 0.9 * 127 * pa.U23, loss / pa.U23
        assert loss <= pa.PRODUCTS[fmt] * pa.U23


def test_f16_image_model_layout_and_trailer():
    rng = np.random.default_rng(1)
    n = 70
    db = rng.standard_normal((n, pa.DIM)).astype(np.float32)
    img = pa.f16_image(db, 3.7)
    assert img.size == 2 * 16384 + 256
    sr = pa.f16_sr(3.7)
    assert sr == 13
    v = img[:2 * 16384].view(np.float16)
    for row, dim in [(0, 0), (5, 77), (33, 127), (64 + 5, 64), (69, 8)]:
        T, rr = divmod(row, 64)
        half, r = divmod(rr, 32)
        h, d = divmod(dim, 64)
        b, j = divmod(d, 8)
        off = T * 16384 + 1024 * (2 * b + half) + 16 * (32 * h + r) + 2 * j
        assert v[off // 2] == np.float16(db[row, dim] * np.float32(2.0 ** sr))
    tail = img[2 * 16384:].view(np.uint32)
    assert list(tail[:4]) == [pa.F16_MAGIC, 13, n, 0] and not tail[4:].any()
    # the rows past n are zero: rows 70..127 of tile 1
    rows_of = np.zeros((128, pa.DIM), np.float16)
    t = v.reshape(2, 8, 2, 2, 32, 8)                      # [T, b, half, h, r, j]
    rows_of[:] = t.transpose(0, 2, 4, 3, 1, 5).reshape(128, pa.DIM)
    assert np.array_equal(rows_of[:n], pa.f16_values(db, 3.7)) and not rows_of[n:].view(np.uint16).any()


def test_f16_values_round_to_nearest_even_and_clamp():
    sr = pa.f16_sr(1.0)
    s = np.float32(2.0 ** -sr)
    mid = np.float32(2049.0)                              # between 2048 and 2050: ties to even -> 2048
    x = np.array([mid, np.nextafter(mid, np.float32(3000)), np.float32(2051.0), 65519.0, 65520.0, 1e6, -1e6], np.float32) * s
    got = pa.f16_values(x[None, :], 1.0)[0]
    assert list(got.astype(np.float64)) == [2048.0, 2050.0, 2052.0, 65504.0, 65504.0, 65504.0, -65504.0]


def test_bf16_split_is_two_truncations():
    x = np.array([1.0 + (2 ** 16 - 1) * 2.0 ** -23, -3.0000002, 1e-40, -0.0], np.float32)
    hi, lo = pa.bf16_split(x)
    h, l = pa.bf16_to_f64(hi), pa.bf16_to_f64(lo)
    assert h[0] == 1.0 and l[0] == 2.0 ** -8 * (2 - 2.0 ** -7)
    assert np.all(np.abs(h) <= np.abs(x)) and np.all(np.abs(h + l) <= np.abs(x.astype(np.float64)))
    assert hi[3] == 0x8000 and lo[3] == 0


def test_bf16_image_model_layout():
    rng = np.random.default_rng(2)
    n = 33
    db = rng.standard_normal((n, pa.DIM)).astype(np.float32)
    img = pa.bf16_image(db).view(np.uint16)
    assert img.size * 2 == 2 * 16384
    hi, lo = pa.bf16_split(db)
    for row, dim in [(0, 0), (31, 127), (32, 70)]:
        T, r = divmod(row, 32)
        h, d = divmod(dim, 64)
        b, j = divmod(d, 8)
        for part, want in ((0, hi), (1, lo)):
            off = T * 16384 + 1024 * (2 * b + part) + 16 * (32 * h + r) + 2 * j
            assert img[off // 2] == want[row, dim]
    assert not img.reshape(2, 8192)[1].reshape(8, 2, 2, 32, 8)[:, :, :, 1:, :].any()     # rows 33..63 of tile 1 are zero


def test_near_tie_family_puts_every_decoy_above_every_true_row():
    for k, kp in ((5, 10), (10, 20), (24, 32), (48, 64)):
        q, T, U, L = pa.near_tie_family(seed=k, k=k, kp=kp)
        assert np.linalg.norm(np.concatenate([T, U, L]).astype(np.float64), axis=1).max() < 1.0
        aT, aU, aL = (pa.a_model(x, q, pa.PF_F16X2, 1.0 + 1e-6) for x in (T, U, L))
        sT, sU, sL = (pa.exact(x, q) for x in (T, U, L))
        rho = float(np.mean(sT - aT))
        assert rho >= 0.99 * pa.U11 * pa.scale_of(T, q).max()
        assert min(aU.min(), aL.min()) > aT.max()
        assert sT.min() > sU.max() > sL.max()
        margin = sU.min() - aL.max()          # the proof passes iff E < this
        assert 0.84 * rho < margin < 0.86 * rho
        for fmt in FP16:                       # the query is exact in fp16: F16X1 has the same approximate scores
            assert np.array_equal(pa.a_model(U, q, fmt, 1.0 + 1e-6), aU)
        q, T, U, L = pa.near_tie_family(seed=k, k=k, kp=kp, control=True)
        aT, aL = (pa.a_model(x, q, pa.PF_F16X2, 1.0 + 1e-6) for x in (T, L))
        assert U.shape[0] == 0 and aT.min() > aL.max()
        assert pa.exact(T, q).min() - aL.max() > 2 * 1.05e-3 + 2 * rho
