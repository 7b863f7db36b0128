"""Worst-case inputs for the prefilter's error bound, and a plain numpy model of what the prefilter computes (TEST INFRASTRUCTURE,
no GPU).

The prefiltered search ranks rows on approximate scores `a` and proves its answer with |a - s| <= E |row| |q| (s = the exact fp32
chain, E = ms_pf_err_coef(format) times the row-norm bound).  This module states, in numpy, what `a` is made of:

* the fp16 image of the rows (MS_PF_F16X2 / MS_PF_F16X1, csrc/ms_scan_pf16.h and ms_pf16_build_image_kernel): row * 2^sr,
  sr = 14 - ilogb(row_norm_bound), clamped to +-65504 and rounded to nearest even; 64-row tiles of 16 KiB, fragment f = 2 b + half,
  lane (r, h) at byte 16 (32 h + r) holding dimensions 64 h + 8 b + j of row 64 T + 32 half + r; zero rows past n; a 256-byte trailer
  {magic, sr, n low, n high, 0 ...} of 32-bit words;
* the split-bf16 image (MS_PF_BF16X3, csrc/ms_scan_pf.h and ms_split8): hi = the upper 16 bits of x, lo = the upper 16 bits of the
  (exact) fp32 difference x - hi -- both truncations; 32-row tiles of 16 KiB, fragment f = 2 b + part;
* the query operands: fp16 formats q * 2^sq, sq = 13 - exponent(max |q_i|) clamped to +-60, qh = fp16(clamp(q * 2^sq)) and (F16X2)
  ql = fp16(that - qh), both rounded to nearest even; split-bf16 the same hi / lo split as the rows;
* a_model: the float64 sum of the exact products of those operands, scaled back -- what the matrix pipe returns if it accumulates
  exactly.  The difference a_kernel - a_model is the pipe's own accumulation, the one term of the budget nobody had measured.

The generators build rows (and queries) that drive one term of the budget close to its analytic maximum; tests/test_pf_adversarial.py
checks through the model alone that each one does, tests/test_prefilter_bound_gpu.py measures the kernels on them."""
import numpy as np

DIM = 128
F16_MAGIC = 0x3631464D
PF_BF16X3, PF_F16X2, PF_F16X1 = 0, 1, 2      # (the values of the C ABI: merizo_search_amd/_lib.py)
U11 = 2.0 ** -11                             # fp16 rounding to nearest, relative (mantissa 1.0)
U23 = 2.0 ** -23                             # one fp32 truncation of a partial sum, relative
PRODUCTS = {PF_F16X2: 256, PF_F16X1: 128, PF_BF16X3: 384}      # products the matrix pipe accumulates per score
# the rounding terms of the budgets in csrc/ms_scan_pf16.h / ms_scan.h (everything but the pipe's accumulation and the exact chain)
UNDERFLOW = np.sqrt(127.0) * 2.0 ** -27      # 8.4e-8: the query's components below the fp16 normal range, flushed
ROUNDING_BUDGET = {PF_F16X2: U11 + 2.0 ** -22 + 2 * UNDERFLOW,
                   PF_F16X1: 2 * U11 + 2.0 ** -22 + 2 * UNDERFLOW,
                   PF_BF16X3: 3 * 2.0 ** -14}


def ilogb(x: float) -> int:
    return int(np.frexp(np.float32(x))[1]) - 1


def f16_sr(row_norm_bound: float) -> int:
    return 14 - ilogb(row_norm_bound)


# ---- the images -------------------------------------------------------------------------------------------------------------
def f16_values(db, row_norm_bound):
    """fp16 values the image holds for the rows of db (same shape, float16)."""
    scale = np.float32(2.0 ** f16_sr(row_norm_bound))
    x = np.asarray(db, np.float32) * scale                      # (a power of two: exact)
    return np.clip(x, np.float32(-65504.0), np.float32(65504.0)).astype(np.float16)


def f16_image(db, row_norm_bound) -> np.ndarray:
    """The bytes of ms_pf_build_image(db, MS_PF_F16X2, row_norm_bound) (uint8, ms_pf_image_bytes of them)."""
    db = np.asarray(db, np.float32)
    n = db.shape[0]
    nt = (n + 63) // 64
    v = np.zeros((nt * 64, DIM), np.float16)
    v[:n] = f16_values(db, row_norm_bound)
    # [T, half, r, h, b, j] -> [T, b, half, h, r, j]: fragment f = 2 b + half, lane 32 h + r, eight fp16 each
    tiles = v.reshape(nt, 2, 32, 2, 8, 8).transpose(0, 4, 1, 3, 2, 5)
    trailer = np.zeros(64, np.uint32)
    trailer[:4] = [F16_MAGIC, np.uint32(f16_sr(row_norm_bound) & 0xFFFFFFFF), n & 0xFFFFFFFF, n >> 32]
    return np.concatenate([np.ascontiguousarray(tiles).view(np.uint8).reshape(-1), trailer.view(np.uint8)])


def bf16_split(x):
    """(hi, lo) as uint16 bit patterns: hi = upper half of x, lo = upper half of fp32(x - hi)."""
    x = np.asarray(x, np.float32)
    bits = x.view(np.uint32)
    hi = bits & np.uint32(0xFFFF0000)
    rest = (x - hi.view(np.float32)).astype(np.float32)          # exact in fp32
    return (bits >> 16).astype(np.uint16), (rest.view(np.uint32) >> 16).astype(np.uint16)


def bf16_to_f64(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_image(db) -> np.ndarray:
    """The bytes of ms_pf_build_image(db, MS_PF_BF16X3) (uint8)."""
    db = np.asarray(db, np.float32)
    n = db.shape[0]
    nt = (n + 31) // 32
    x = np.zeros((nt * 32, DIM), np.float32)
    x[:n] = db
    hi, lo = bf16_split(x)
    parts = np.stack([hi, lo], axis=0).reshape(2, nt, 32, 2, 8, 8)          # [part, T, r, h, b, j]
    tiles = parts.transpose(1, 4, 0, 3, 2, 5)                               # [T, b, part, h, r, j]
    return np.ascontiguousarray(tiles).view(np.uint8).reshape(-1)


# ---- the query operands and the approximate score ------------------------------------------------------------------------
def f16_query(q, fmt):
    """(sq, qh, ql) as the fp16 scan prepares the query (ql = 0 for F16X1)."""
    q = np.asarray(q, np.float32)
    m = np.float32(np.abs(q).max()) if q.size else np.float32(0)
    sq = 0
    if 0 < m < np.inf:
        sq = 13 - (int((np.float32(m).view(np.uint32) >> 23) & 0xFF) - 127)
    sq = max(-60, min(60, sq))
    c = np.clip(q * np.float32(2.0 ** sq), np.float32(-65504.0), np.float32(65504.0)).astype(np.float32)
    qh = c.astype(np.float16)
    ql = (c - qh.astype(np.float32)).astype(np.float16) if fmt == PF_F16X2 else np.zeros_like(qh)
    return sq, qh, ql


def a_model(rows, q, fmt, row_norm_bound=1.0, flush=False):
    """Approximate scores of rows [m, 128] against one query, the pipe taken as exact (float64).
    flush: fp16 formats -- the operands that are fp16 subnormals taken as 0 (what a flushing kernel would use)."""
    rows = np.atleast_2d(np.asarray(rows, np.float32))
    if fmt == PF_BF16X3:
        hx, lx = (bf16_to_f64(t) for t in bf16_split(rows))
        hq, lq = (bf16_to_f64(t) for t in bf16_split(q))
        return hx @ hq + hx @ lq + lx @ hq
    sr = f16_sr(row_norm_bound)
    sq, qh, ql = f16_query(q, fmt)
    rh = f16_values(rows, row_norm_bound).astype(np.float64)
    qh, ql = qh.astype(np.float64), ql.astype(np.float64)
    if flush:
        rh[np.abs(rh) < 2.0 ** -14] = 0.0
        qh[np.abs(qh) < 2.0 ** -14] = 0.0
        ql[np.abs(ql) < 2.0 ** -14] = 0.0
    return (rh @ qh + rh @ ql) * 2.0 ** -(sr + sq)


def exact(rows, q):
    return np.atleast_2d(np.asarray(rows, np.float64)) @ np.asarray(q, np.float64)


def scale_of(rows, q):
    """|row| |q| per row (float64)."""
    return np.linalg.norm(np.atleast_2d(np.asarray(rows, np.float64)), axis=1) * np.linalg.norm(np.asarray(q, np.float64))


def trunc_f32(x: float) -> float:
    """x rounded toward zero to fp32."""
    f = np.float32(x)
    if abs(float(f)) > abs(x):
        f = np.nextafter(f, np.float32(0))
    return float(f)


def truncating_sum(products) -> float:
    """Sequential fp32 accumulation that truncates after every add: the budget's model of the worst matrix pipe."""
    acc = 0.0
    for p in products:
        acc = trunc_f32(acc + float(p))
    return acc


# ---- the query pattern the fp16 generators share ------------------------------------------------------------------------
# 48 dimensions of magnitude 2^-3, 64 of 2^-4, 16 zero: |q| = 1 EXACTLY (so a raw query normalises to itself, bit for bit), every
# component exactly representable in fp16 after the scan's scaling (sq = 16).  Rows follow it, component by component, at the
# fp16 image's scale (sr = 14 for any bound in [1, 2)): 2^11 (ulp 2) on the first class, 2^10 (ulp 1) on 60 dimensions of the
# second and 2^9 (ulp 1/2) on its last 4 -- which keeps |row| <= 0.998 with every component just off a midpoint.
_BASE = {3: 2048.0, 4: 1024.0, 5: 512.0}           # scaled row base per class (mantissa 1.0)
_QMAG = {3: 2.0 ** -3, 4: 2.0 ** -4, 5: 2.0 ** -4}


class Pattern:
    """Signs and magnitude classes of one query; rows are built to match it."""

    def __init__(self, rng):
        perm = rng.permutation(DIM)
        self.cls = np.zeros(DIM, np.int64)
        self.cls[perm[:48]] = 3
        self.cls[perm[48:108]] = 4
        self.cls[perm[108:112]] = 5
        self.sign = rng.choice([-1.0, 1.0], size=DIM)
        self.rng = rng

    def query(self) -> np.ndarray:
        q = np.array([_QMAG.get(c, 0.0) for c in self.cls]) * self.sign
        return q.astype(np.float32)

    def base(self):
        return np.array([_BASE.get(c, 0.0) for c in self.cls])

    def ulp(self):
        return self.base() / 1024.0

    def row(self, t, side, flip=()):
        """Scaled value of dimension i = base_i + ulp_i (t_i + 1/2) + side * (1..8 fp32 ulps): just below (side -1) or above (+1) the
        fp16 midpoint, so that it rounds to base + ulp t (-1) or base + ulp (t + 1) (+1).  `flip`: dimensions whose sign is reversed.
        Returned at the unscaled value (sr = 14)."""
        t = np.broadcast_to(np.asarray(t, np.float64), (DIM,))
        base, u = self.base(), self.ulp()
        f32ulp = np.where(base > 0, base * 2.0 ** -23, 0.0)
        d = self.rng.integers(1, 9, size=DIM) * f32ulp
        v = np.where(base > 0, base + u * (t + 0.5) + side * d, 0.0) * self.sign
        v[list(flip)] *= -1.0
        out = (v * 2.0 ** -14).astype(np.float32)
        assert np.array_equal(out.astype(np.float64), v * 2.0 ** -14)          # (the construction is exact in fp32)
        return out

    def lowered(self, units):
        """t per dimension: 3 everywhere, lowered by `units` x 2^-19 of score (class 3 steps 8 units, class 4 two, class 5 one)."""
        t = np.full(DIM, 3.0)
        step = {3: 8, 4: 2, 5: 1}
        left = int(units)
        for c in (3, 4, 5):
            for i in np.flatnonzero(self.cls == c):
                while left >= step[c] and t[i] > 0:
                    t[i] -= 1
                    left -= step[c]
        assert left == 0, "cannot lower a row by that much"
        return t


H_UNITS = 7.9375 * 2.0 ** -14 / 2.0 ** -19          # sum |q_i| ulp_i / 2 in units of 2^-19 (254)


# ---- generators (seeded), one per budget term ------------------------------------------------------------------------------
def f16_row_rounding(seed, m, side=-1):
    """fp16 row rounding: q (the shared pattern) and m rows whose every component sits 1-8 fp32 ulps below (side -1) or above (+1) an
    fp16 midpoint at mantissa ~1.0, signs matching q -- every product's rounding error has the same sign, |row_i| ~ |q_i|: the row term
    (2^-11 |row||q|) reached to ~0.5 %.  Rows differ in t (0..3) and in their sub-fp16 bits."""
    rng = np.random.default_rng(seed)
    p = Pattern(rng)
    rows = np.stack([p.row(rng.integers(0, 4, size=DIM), side) for _ in range(m)])
    return p.query(), rows


def f16x1_query_rounding(seed, m):
    """F16X1 adds the query's own rounding (its hi part alone): q's components also sit just below fp16 midpoints after scaling
    (sq = 16: 2^13 + 8 (t + 1/2) - d on the first class, 2^12 + 4 (t + 1/2) - d on the second), rows as in f16_row_rounding with
    side -1 -- both errors pull every product down: target 2 x 2^-11."""
    rng = np.random.default_rng(seed)
    p = Pattern(rng)
    qb = np.array([{3: 8192.0, 4: 4096.0, 5: 4096.0}.get(c, 0.0) for c in p.cls])
    tq = rng.integers(0, 4, size=DIM)
    d = rng.integers(1, 9, size=DIM) * qb * 2.0 ** -23
    q = (np.where(qb > 0, qb + qb / 1024.0 * (tq + 0.5) - d, 0.0) * p.sign * 2.0 ** -16).astype(np.float32)
    rows = np.stack([p.row(rng.integers(0, 4, size=DIM), -1) for _ in range(m)])
    return q, rows


_TRUNC_Q = {3: 44, 4: 64}


def bf16_truncation(seed, m):
    """Split-bf16 truncation: every significand of q and of the rows is 1.0000000 followed by sixteen ones (lo ~ 2^-7 |x| and the part
    lost below lo ~ 2^-15 |x|, both at their maximum for a mantissa near 1), every product positive: all three omitted terms (lo.lo,
    the rows' and the query's remainders) have the same sign.  Attainable: 2^-13 / (1 + 2^-7)^2 = 0.98 x 2^-13 -- the comment's
    3 x 2^-14 counts 2^-14 for each remainder where the truncated split leaves 2^-15."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(DIM)
    mag = np.zeros(DIM)
    mag[perm[:44]] = 2.0 ** -3
    mag[perm[44:108]] = 2.0 ** -4
    sign = rng.choice([-1.0, 1.0], size=DIM)
    ones = np.float32(1.0 + (2.0 ** 16 - 1) * 2.0 ** -23)

    def vec(clear):
        v = (mag * float(ones) * sign).astype(np.float32)
        bits = v.view(np.uint32)
        for i in clear:                      # (rows differ in one of the three lowest bits of a few components)
            bits[i] &= ~np.uint32(1 << int(rng.integers(0, 3)))
        return bits.view(np.float32)

    q = vec(())
    rows = np.stack([vec(rng.choice(perm[:108], size=4, replace=False)) for _ in range(m)])
    return q, rows


def query_underflow(seed, m):
    """The query's components that fall below the fp16 normal range after scaling (q_i < 2^-27 max|q|): a lead component 2^-3 and
    127 components just below 2^-30 (subnormal in fp16 once scaled), rows 2^-2 on the lead and 2^-4 on the rest, signs matching: the
    whole flushed mass adds up.  Target (flushed): sqrt(127) 2^-27 |row||q| -- reached to ~0.94 (the lead must keep these rows on
    top).  A kernel that keeps fp16 subnormals (no flush) loses at most 2^-25 per component after scaling, ~2^-11 of that."""
    rng = np.random.default_rng(seed)
    lead = int(rng.integers(0, DIM))
    sign = rng.choice([-1.0, 1.0], size=DIM)
    low = 1.0 - rng.integers(8, 24, size=DIM) * 2.0 ** -12      # (>= 2^-23 below 2^-14 once scaled: stays subnormal)
    q = (sign * 2.0 ** -30 * low).astype(np.float32)
    q[lead] = np.float32(sign[lead] * 2.0 ** -3)
    rows = np.tile((sign * 2.0 ** -4).astype(np.float32), (m, 1))
    rows[:, lead] = np.float32(sign[lead] * 2.0 ** -2)
    for r in range(m):                                           # (distinct rows: a few components one fp32 ulp lower)
        i = rng.choice(np.flatnonzero(np.arange(DIM) != lead), size=3, replace=False)
        rows[r, i] = np.nextafter(rows[r, i], np.float32(0))
    return q, rows


def accumulation(seed, m, fmt):
    """The matrix pipe's accumulation: one large product first (the lead component, |row_lead| = 1, q_lead = 2^-3, the partial sum
    at 2^-3 -- a mantissa of 1.0) and then 127 products just below the partial sum's fp32 ulp, their significands all ones:
    an accumulator that truncates after every add loses every one of them, 127 x 2^-23 |row||q|.  That is the budget's P x 2^-23
    for F16X1 (P = 128) to 1 %; for F16X2 and BF16X3 the other P - 128 products are the query's low part times the same row
    components (|ql| <= 2^-11 |qh|, |lo| < 2^-7 |hi|) and cannot also sit at the accumulator's ulp: 127 of 256 / 384 is the most a
    single row can reach.  Rows need a row-norm bound >= 1 + 4e-6 (the bound tests use 1 + 2^-10)."""
    rng = np.random.default_rng(seed)
    lead = int(rng.integers(0, DIM))
    sign = rng.choice([-1.0, 1.0], size=DIM)
    if fmt == PF_BF16X3:   # bf16-exact: 2^-13 (2 - 2^-7) x 2^-14 = 2^-26 (1 - 2^-8), the ulp of 2^-3 being 2^-26
        xs, qs = 2.0 ** -13 * (2.0 - 2.0 ** -7), 2.0 ** -14
    else:                  # fp16-exact after scaling (sr = 14, sq = 16): (2047 / 512) x 4 = 16 (1 - 2^-11), the ulp of 2^27 being 16
        xs, qs = (2047.0 / 512.0) * 2.0 ** -14, 4.0 * 2.0 ** -16
    q = (sign * qs).astype(np.float32)
    q[lead] = np.float32(sign[lead] * 2.0 ** -3)
    rows = np.tile((sign * xs).astype(np.float32), (m, 1))
    rows[:, lead] = np.float32(sign[lead])
    others = np.flatnonzero(np.arange(DIM) != lead)
    for r in range(m):                 # (distinct rows: a few of the small components one step smaller -- each still lost)
        i = rng.choice(others, size=2, replace=False)
        step = 2.0 ** -13 * 2.0 ** -7 if fmt == PF_BF16X3 else 2.0 ** -9 * 2.0 ** -14
        rows[r, i] = (rows[r, i] - np.sign(rows[r, i]) * step).astype(np.float32)
    return q, rows, lead


def acc_order(lead):
    """Dimensions in the order the analysis accumulates them: the lead first."""
    return [lead] + [i for i in range(DIM) if i != lead]


def truncation_loss(row, q, fmt, lead, row_norm_bound=1.0):
    """|exact sum - truncating sequential sum| of the products the pipe sees (the model's operands), per |row||q|."""
    if fmt == PF_BF16X3:
        hx, lx = (bf16_to_f64(t) for t in bf16_split(row))
        hq, lq = (bf16_to_f64(t) for t in bf16_split(q))
        prods = [p for i in acc_order(lead) for p in (hx[i] * hq[i], hx[i] * lq[i], lx[i] * hq[i])]
        sc = 1.0
    else:
        sr = f16_sr(row_norm_bound)
        sq, qh, ql = f16_query(q, fmt)
        rh = f16_values(row[None, :], row_norm_bound)[0].astype(np.float64)
        prods = [p for i in acc_order(lead) for p in (rh[i] * float(qh[i]), rh[i] * float(ql[i]))]
        sc = 2.0 ** -(sr + sq)
    ex = float(np.sum(np.array(prods, np.float64)))
    return abs(ex - truncating_sum(prods)) * sc / float(scale_of(row, q)[0])


# ---- the near-tie families of the end-to-end proof test -------------------------------------------------------------------
def near_tie_family(seed, k, kp, control=False):
    """One query and the rows of tests/test_prefilter_bound_gpu.py's planted wrong answer (fp16 formats, sr = 14, the query exactly
    representable: all the error is the rows' rounding, rho = H ~ 0.995 x 2^-11 |row||q| each way):
      T (k rows): t = 3, rounded down: s = S, a = S - rho;
      U (k rows): side +1, lowered by g1 = 0.05 rho: s = S - g1, a = S - g1 + rho;
      L (kp - k rows): side +1, lowered by g2 = 1.9 rho: s = S - g2, a = S - g2 + rho.
    Every decoy out-ranks every true row on a, so the candidates are U and L, and the proof (kth > a_last + E) passes iff
    g2 - g1 - rho > E, i.e. E < 0.85 rho.  control: T and L only, L one sign flip below (s = S - 2^-7 > 2E + 2 rho away).
    Returns (q, T, U, L)."""
    rng = np.random.default_rng(seed)
    p = Pattern(rng)
    q = p.query()
    T = np.stack([p.row(np.full(DIM, 3.0), -1) for _ in range(k)])
    if control:
        i = int(np.flatnonzero(p.cls == 4)[0])
        L = np.stack([p.row(np.full(DIM, 3.0), +1, flip=(i,)) for _ in range(kp - k)])
        return q, T, T[:0], L
    g1, g2 = int(round(0.05 * H_UNITS)), int(round(1.9 * H_UNITS))
    U = np.stack([p.row(p.lowered(g1), +1) for _ in range(k)])
    L = np.stack([p.row(p.lowered(g2), +1) for _ in range(kp - k)])
    return q, T, U, L
