"""Tensor-level front end of the C ABI: torch tensors in, torch tensors out, HIP underneath.

Every function runs on the tensors' device via libmerizo_search_amd.so on torch's current
stream and raises ``MerizoHipError`` when the library or a GPU is missing (no fallback).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import logging
import os

import numpy as np

from . import _lib
from ._lib import DIM, MODE_COSINE_RAW, MODE_COSINE_UNIT, MODE_IP_NORMQ, MODE_IP_PRENORM, MerizoHipError, check, ptr


class _on:
    """Device scope of one C-ABI call: the library launches on HIP's CURRENT device, so every entry
    point makes the tensors' device current for the call and hands over THAT device's current
    stream.  All tensor arguments must live on one device."""

    def __init__(self, *tensors):
        torch = _lib.require_gpu()
        devs = {t.device for t in tensors if t is not None}
        if len(devs) != 1:
            raise MerizoHipError(f"tensors of one call must share a device, got {sorted(str(d) for d in devs)}")
        self.device = devs.pop()
        if self.device.type != "cuda":
            raise MerizoHipError("expected CUDA/HIP tensors")
        self._guard = torch.cuda.device(self.device)
        self.stream = None

    def __enter__(self):
        import torch
        self._guard.__enter__()
        self.stream = torch.cuda.current_stream(self.device).cuda_stream
        return self

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)


def _f32_cuda(t, name: str, cols: Optional[int] = None):
    torch = _lib.require_gpu()
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MerizoHipError(f"{name}: expected a CUDA/HIP tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise MerizoHipError(f"{name}: expected a contiguous float32 tensor")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise MerizoHipError(f"{name}: expected shape [n,{cols}], got {tuple(t.shape)}")
    return t


def _row_vectors(*vectors):
    """The optional per-row vectors of a call, each given as (name, tensor or None, size): float32 CUDA/HIP vectors of `size` elements."""
    for name, t, size in vectors:
        if t is not None:
            _f32_cuda(t, name)
            if t.numel() != size:
                raise MerizoHipError(f"{name}: expected {size} elements, got {t.numel()}")


def _int_desc(x, dtype, name: str, device, who: str, cols: Optional[int] = None, length: Optional[int] = None, reshape: bool = False):
    """An integer descriptor of `who` as a contiguous tensor of the numpy `dtype` on `device`: a tensor of any integer type (a
    floating-point one is refused), or a host array or list, which is converted as numpy converts it and uploaded.  One dimension,
    or [rows,cols] when cols is given; of `length` rows when given.  reshape: a descriptor of another shape is laid out in that form
    (a flat (q0, nqd, q0, nqd, ...) list for [nqc,2]) where its entries allow it."""
    torch = _lib.require_gpu()
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype)))
    if t.is_floating_point():
        raise MerizoHipError(f"{who}: {name}: expected integers, got {t.dtype}")
    t = t.to(device=device, dtype=getattr(torch, np.dtype(dtype).name)).contiguous()
    if reshape and t.numel() % (cols or 1) == 0:
        t = t.reshape(-1, cols) if cols else t.reshape(-1)
    if t.dim() != (1 if cols is None else 2) or (cols is not None and t.shape[1] != cols) or (length is not None and t.shape[0] != length):
        raise MerizoHipError(f"{who}: {name}: expected {'n' if length is None else length} rows{f' of {cols}' if cols else ''}, got {tuple(t.shape)}")
    return t


def _outputs(who: str, spec, out, device):
    """The outputs of `who` as a tuple: new tensors after spec = ((dtype, shape), ...), or the caller's `out` once each of its tensors
    is a contiguous CUDA/HIP tensor of that dtype and shape (a shape of None: the caller sized that one)."""
    torch = _lib.require_gpu()
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=device) for dtype, shape in spec)
    out = tuple(out)
    if len(out) != len(spec) or any(not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous()
                                    or (shape is not None and tuple(t.shape) != tuple(shape)) for t, (dtype, shape) in zip(out, spec)):
        form = ", ".join(f"{str(dtype)[6:]} {list(shape) if shape is not None else '[...]'}" for dtype, shape in spec)
        raise MerizoHipError(f"{who}: out must be contiguous CUDA/HIP tensors ({form})")
    return out


def _workspace_bytes(sizing: str, *sizes) -> int:
    """What the library's sizing function `sizing` answers for `sizes`; 0 is its refusal."""
    need = int(getattr(_lib.load(), sizing)(*sizes))
    if need == 0:
        raise MerizoHipError(f"{sizing} rejected the sizes {sizes}")
    return need


def _workspace(who: str, sizing: str, sizes, workspace, device):
    """The scratch of one call of `who`: a new uint8 tensor of `sizing`(*sizes) bytes, or the caller's `workspace` once it is a
    contiguous uint8 tensor of at least as many (the library would refuse a shorter one with MS_ERR_WORKSPACE, -2)."""
    torch = _lib.require_gpu()
    need = _workspace_bytes(sizing, *sizes)
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise MerizoHipError(f"{who}: workspace must be a contiguous uint8 tensor of at least {need} bytes ({sizing}: MS_ERR_WORKSPACE (-2))")
    return workspace


def _capped_relaunch(launch, buffers, cap: int):
    """launch(buffers(cap), cap) -> how many entries the call found; once more into buffers of exactly that many when they exceed cap.
    -> (the buffers of the last launch, their slots, found).  launch synchronises (it reads the count back): one sync per launch."""
    cap = max(int(cap), 0)
    bufs = buffers(cap)
    found = launch(bufs, cap)
    if found > cap:
        bufs, cap = buffers(found), found
        found = launch(bufs, cap)
    return bufs, cap, found


def l2_normalize_rows_(x, eps: float = 1e-12):
    """In-place F.normalize(x) (reference dbsearch.py:303-304)."""
    _f32_cuda(x, "x", DIM)
    with _on(x) as dev:
        check(_lib.load().ms_l2_normalize_rows(ptr(x), x.shape[0], DIM, eps, dev.stream), "ms_l2_normalize_rows")
    return x


def l2_normalize_rows(x, eps: float = 1e-12, out=None):
    """F.normalize(x) out of place (reference dbsearch.py:303-304) -> a new tensor, or `out`."""
    torch = _lib.require_gpu()
    _f32_cuda(x, "x", DIM)
    y = torch.empty_like(x) if out is None else _f32_cuda(out, "out", DIM)
    if y.shape != x.shape or y.data_ptr() == x.data_ptr():
        raise MerizoHipError("l2_normalize_rows: out must have x's shape and not alias it")
    with _on(x, y) as dev:
        check(_lib.load().ms_l2_normalize_rows_to(ptr(x), ptr(y), x.shape[0], DIM, eps, dev.stream), "ms_l2_normalize_rows_to")
    return y


def row_inv_norms(x, eps: float = 1e-8):
    """1 / max(||row||, eps) for every database row (the DB half of cosine_similarity)."""
    torch = _lib.require_gpu()
    _f32_cuda(x, "x", DIM)
    inv = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    with _on(x) as dev:
        check(_lib.load().ms_row_inv_norms(ptr(x), x.shape[0], DIM, eps, ptr(inv), dev.stream), "ms_row_inv_norms")
    return inv


class TopKWorkspace:
    """Scratch buffer for ms_ip_topk, grown on demand and reused across calls."""
    _sizing = "ms_ip_topk_workspace_bytes"

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, n: int, nq: int, k: int):
        torch = _lib.require_gpu()
        with torch.cuda.device(self.device):          # the plan depends on the device's CU count
            need = _workspace_bytes(self._sizing, n, nq, k)
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.buf


def _out_pair(nq: int, k: int, device, out, who: str):
    """The (scores f32 [nq,k], idx i64 [nq,k]) outputs of a search: new tensors, or the caller's `out` once it has that form
    (_outputs written out for this one form: every search call passes through here, and a timed step should not build a table)."""
    torch = _lib.require_gpu()
    if out is None:
        return (torch.empty((nq, k), dtype=torch.float32, device=device), torch.empty((nq, k), dtype=torch.int64, device=device))
    out_s, out_i = out
    if (tuple(out_s.shape) != (nq, k) or tuple(out_i.shape) != (nq, k) or out_s.dtype != torch.float32
            or out_i.dtype != torch.int64 or not out_s.is_contiguous() or not out_i.is_contiguous()):
        raise MerizoHipError(f"{who}: out must be contiguous (float32 [nq,k], int64 [nq,k]) tensors")
    return out_s, out_i


def ip_topk(db, q, k: int, mode: int = MODE_IP_PRENORM, inv_norm=None, lengths=None, qlen=None,
            mincov: float = 0.0, row_offset: int = 0, workspace=None, out=None):
    """Exact top-k of q [nq,128] against db [n,128] -> (scores f32 [nq,k], idx i64 [nq,k]).
    workspace: a TopKWorkspace (grown on demand) or a uint8 tensor of ms_ip_topk_workspace_bytes;
    out: optional preallocated (scores, idx) tensors."""
    torch = _lib.require_gpu()
    _f32_cuda(db, "db", DIM)
    _f32_cuda(q, "q", DIM)
    n, nq = db.shape[0], q.shape[0]
    _row_vectors(("inv_norm", inv_norm, n), ("lengths", lengths, n), ("qlen", qlen, nq))
    ws = workspace if isinstance(workspace, torch.Tensor) else (workspace or TopKWorkspace(db.device)).get(n, nq, k)
    out_s, out_i = _out_pair(nq, k, db.device, out, "ip_topk")
    with _on(db, q, inv_norm, lengths, qlen, ws, out_s, out_i) as dev:
        check(_lib.load().ms_ip_topk(ptr(db), n, row_offset, ptr(q), nq, k, mode, ptr(inv_norm), ptr(lengths), ptr(qlen),
                                     mincov, ptr(out_s), ptr(out_i), ptr(ws), ws.numel(), dev.stream), "ms_ip_topk")
    return out_s, out_i


def ip_topk_prepare(db, q, k: int, ws, mode: int = MODE_IP_PRENORM, inv_norm=None, lengths=None, qlen=None,
                    mincov: float = 0.0):
    """Stage 1 of ip_topk (k <= 64): query preparation + sample pass."""
    with _on(db, q, inv_norm, lengths, qlen, ws) as dev:
        check(_lib.load().ms_ip_topk_prepare(ptr(db), db.shape[0], ptr(q), q.shape[0], k, mode, ptr(inv_norm), ptr(lengths),
                                             ptr(qlen), mincov, ptr(ws), ws.numel(), dev.stream), "ms_ip_topk_prepare")


def ip_topk_scan(db, q, k: int, ws, mode: int = MODE_IP_PRENORM, inv_norm=None, lengths=None, qlen=None,
                 mincov: float = 0.0):
    """Stage 2 of ip_topk (k <= 64): the one launch of the fused score + top-k scan kernel (bench timing)."""
    with _on(db, q, inv_norm, lengths, qlen, ws) as dev:
        check(_lib.load().ms_ip_topk_scan(ptr(db), db.shape[0], ptr(q), q.shape[0], k, mode, ptr(inv_norm), ptr(lengths),
                                          ptr(qlen), mincov, ptr(ws), ws.numel(), dev.stream), "ms_ip_topk_scan")


def ip_topk_finish(n: int, nq: int, k: int, ws, out_s, out_i, row_offset: int = 0):
    """Stage 3 of ip_topk (k <= 64): merge the per-stream lists into the outputs."""
    with _on(ws, out_s, out_i) as dev:
        check(_lib.load().ms_ip_topk_finish(n, row_offset, nq, k, ptr(out_s), ptr(out_i), ptr(ws), ws.numel(),
                                            dev.stream), "ms_ip_topk_finish")


class LargeKWorkspace(TopKWorkspace):
    """Scratch buffer for ms_ip_topk_large (operands, group lists, one bin per query, and the plain search's workspace)."""
    _sizing = "ms_ip_topk_large_workspace_bytes"


# The fewest rows from which the searches route 64 < k <= LARGE_K_MAX to ip_topk_large (large_k_serves); read once from
# MS_LARGE_K_MIN_ROWS.  The default is what tools/time_large_k.py measured; a test sets the attribute.
LARGE_K_MIN_ROWS = int(os.environ.get("MS_LARGE_K_MIN_ROWS", "200000"))
# k = 65..128 is two scans on the old path against two reads of the fp32 rows on this one: it pays from this many queries on
# (measured: 0.83-0.93x for one query, 1.06-2.1x for eight; profiles/large_k_timing.log).  A module attribute, as the row count.
LARGE_K_TWO_SCAN_MIN_NQ = 8
LARGE_K_FALLBACK_NOTE = 0.1        # more than this share of a call's queries on the fallback: one INFO line


def large_k_serves(n: int, nq: int, k: int) -> bool:
    """The shapes the searches hand to ip_topk_large: 64 < k <= MS_LARGE_K_MAX, at least 128 rows in each of the G = ceil(k / 64)
    groups of the bound (what ms_ip_topk_large itself takes), at least LARGE_K_MIN_ROWS rows, and for k <= 128 at least
    LARGE_K_TWO_SCAN_MIN_NQ queries (from where it is no slower than ms_ip_topk's ceil(k / 64) scans).  ONE statement of the rule
    for the engine, the drivers and the tests."""
    groups = -(-int(k) // 64)
    return (64 < k <= _lib.LARGE_K_MAX and n >= 128 * groups and n >= LARGE_K_MIN_ROWS and nq >= 1
            and (k > 128 or nq >= LARGE_K_TWO_SCAN_MIN_NQ))


def _large_k_rounds(call, fallback, q, qlen, stats=None):
    """The rounds of ip_topk_large on any device (the CPU tests drive it with stubs).  call(q, qlen, lb_in) -> (scores [nq,k], idx
    [nq,k], status int32 [nq], lb float32 [nq], st int64 [4]) is one ms_ip_topk_large; fallback(q, qlen) -> (scores, idx) is ip_topk.
    First round on all queries; the status-1 queries once more with lb_in = their out_lb; whatever is then not status 0 goes to
    the fallback; everything is scattered back into the first round's outputs.  One read-back per round."""
    def pick(t, rows):
        return None if t is None else t.index_select(0, rows).contiguous()

    nq = q.shape[0]
    out_s, out_i, status, lb, st = call(q, qlen, None)
    c = [int(x) for x in st.tolist()]                       # (the one sync of the round)
    info = {"first_round": c[0], "second_round": 0, "fallback": 0, "rescored": max(c[3], 0), "forwarded": c[3] < 0}
    left = c[1] + c[2]
    if c[1] > 0:
        again = (status == 1).nonzero().flatten()
        s2, i2, status2, _, st2 = call(pick(q, again), pick(qlen, again), pick(lb, again))
        c2 = [int(x) for x in st2.tolist()]
        out_s.index_copy_(0, again, s2)                     # (a row that is not final is padding, and the fallback's to fill)
        out_i.index_copy_(0, again, i2)
        status.index_copy_(0, again, status2)
        info["second_round"] = c2[0]
        info["rescored"] += max(c2[3], 0)
        left -= c2[0]
    if left > 0:
        rest = (status != 0).nonzero().flatten()
        sf, jf = fallback(pick(q, rest), pick(qlen, rest))
        out_s.index_copy_(0, rest, sf)
        out_i.index_copy_(0, rest, jf)
        info["fallback"] = left
    if info["first_round"] + info["second_round"] + info["fallback"] != nq:
        raise MerizoHipError(f"ip_topk_large: the rounds account for {info} of {nq} queries")
    if info["fallback"] > LARGE_K_FALLBACK_NOTE * nq:
        logging.info(f"large-k search: {info['fallback']} of {nq} queries took the ceil(k/64)-scan path (a database ordered by family "
                     "weakens the per-group bound and overflows the candidate bins; the results are exact either way).")
    if stats is not None:
        stats.update(info)
    return out_s, out_i


def ip_topk_large(db, q, k: int, row_norm_bound: float, mode: int = MODE_IP_PRENORM, lengths=None, qlen=None, mincov: float = 0.0,
                  row_offset: int = 0, workspace=None, out=None, stats=None):
    """ip_topk for 64 < k <= MS_LARGE_K_MAX with the same results bit for bit, from one fp32 read of the rows and one read behind
    the fp16 matrix pipe instead of ceil(k / 64) fp32 scans (ms_ip_topk_large: the definition and the exactness argument are the
    header's).  Always the complete exact answer: queries whose bin overflowed get a second round with the tighter bound the first
    left, and whatever is still open goes to ip_topk.  Shapes the route does not take are ip_topk inside the first call.
    row_norm_bound: an upper bound on every row's L2 norm (1.0 + 1e-6 for unit rows; it need not hold).  Synchronises once per
    round (it reads the status counts back).  workspace: a LargeKWorkspace or a uint8 tensor of ms_ip_topk_large_workspace_bytes;
    stats: a dict that receives 'first_round', 'second_round' and 'fallback' (queries answered by each; they add up to nq),
    'rescored' (cells sent to the exact chain) and 'forwarded' (the first call was ip_topk's)."""
    torch = _lib.require_gpu()
    _f32_cuda(db, "db", DIM)
    _f32_cuda(q, "q", DIM)
    if mode not in (MODE_IP_PRENORM, MODE_IP_NORMQ, MODE_COSINE_UNIT):
        raise MerizoHipError("ip_topk_large: MODE_IP_PRENORM, MODE_IP_NORMQ or MODE_COSINE_UNIT")
    if mode != MODE_COSINE_UNIT and (lengths is not None or qlen is not None):
        raise MerizoHipError("ip_topk_large: lengths / qlen go with MODE_COSINE_UNIT")
    n, k = db.shape[0], int(k)
    _row_vectors(("lengths", lengths, n), ("qlen", qlen, q.shape[0]))
    shared = workspace if isinstance(workspace, LargeKWorkspace) else LargeKWorkspace(db.device)

    def call(qs, qls, lb_in):
        nqs = qs.shape[0]
        first = lb_in is None
        if first and isinstance(workspace, torch.Tensor):
            ws = _workspace("ip_topk_large", "ms_ip_topk_large_workspace_bytes", (n, nqs, k), workspace, db.device)
        else:
            ws = shared.get(n, nqs, k)
        out_s, out_i = _out_pair(nqs, k, db.device, out if first else None, "ip_topk_large")
        status, lb, st = _outputs("ip_topk_large", ((torch.int32, (nqs,)), (torch.float32, (nqs,)), (torch.int64, (4,))), None, db.device)
        with _on(db, qs, lengths, qls, lb_in, ws, out_s, out_i) as dev:
            check(_lib.load().ms_ip_topk_large(ptr(db), n, int(row_offset), ptr(qs), nqs, k, int(mode), ptr(lengths), ptr(qls), float(mincov),
                                               float(row_norm_bound), ptr(lb_in), ptr(out_s), ptr(out_i), ptr(status), ptr(lb), ptr(st),
                                               ptr(ws), ws.numel(), dev.stream), "ms_ip_topk_large")
        return out_s, out_i, status, lb, st

    def fallback(qs, qls):
        return ip_topk(db, qs, k, mode=mode, lengths=lengths, qlen=qls, mincov=mincov, row_offset=row_offset)

    return _large_k_rounds(call, fallback, q, qlen, stats)


class PrefilterWorkspace(TopKWorkspace):
    """Scratch buffer for ms_ip_topk_prefiltered (the plain search's workspace plus the candidate lists)."""
    _sizing = "ms_ip_topk_prefiltered_workspace_bytes"


PF_BF16X3, PF_F16X2, PF_F16X1 = _lib.PF_BF16X3, _lib.PF_F16X2, _lib.PF_F16X1
_PF_NAMES = {"bf16x3": PF_BF16X3, "f16x2": PF_F16X2, "f16x1": PF_F16X1}


def pf_default_format() -> int:
    """The image the driver builds: fp16 rows (256 B per row; MS_PF_F16X2 / MS_PF_F16X1 share it -- which of the two arithmetics runs
    is decided per database by pf_choose_format unless MS_PF_FORMAT names one); MS_PF_FORMAT=bf16x3|f16x2|f16x1|auto overrides
    (A/B runs; MS_PF_BF16X3 is also what the engine falls back to for databases whose rows leave the fp16 range)."""
    name = os.environ.get("MS_PF_FORMAT", "auto").lower()
    if name == "auto":
        return PF_F16X2
    if name not in _PF_NAMES:
        raise MerizoHipError(f"MS_PF_FORMAT={name}: expected one of {sorted(_PF_NAMES) + ['auto']}")
    return _PF_NAMES[name]


def pf_format_is_auto() -> bool:
    return os.environ.get("MS_PF_FORMAT", "auto").lower() == "auto"


class PfImage:
    """An MFMA-ready image of a resident database (ms_pf_build_image) with the arithmetic it was built for.  `data`: uint8 tensor;
    `format`: PF_BF16X3 (512 B per row) or PF_F16X2 / PF_F16X1 (ONE fp16 image, 256 B per row: `as_format` switches between the two)."""
    __slots__ = ("data", "format", "n")

    def __init__(self, data, fmt: int, n: int):
        self.data, self.format, self.n = data, int(fmt), int(n)

    def numel(self) -> int:
        return self.data.numel()

    def as_format(self, fmt: int) -> "PfImage":
        if fmt == self.format:
            return self
        if PF_BF16X3 in (fmt, self.format):
            raise MerizoHipError("the split-bf16 image and the fp16 image are different buffers: build the one you want")
        return PfImage(self.data, fmt, self.n)


def pf_err_coef(fmt: int) -> float:
    """E of the format: |approximate - exact| <= E |row| |q| (ms_pf_err_coef)."""
    return float(_lib.load().ms_pf_err_coef(int(fmt)))


def pf_build_image(db, fmt=None, row_norm_bound=None, out=None) -> PfImage:
    """The image of a resident database for the prefiltered search (ms_pf_build_image), built once next to the fp32 rows:
    fp16 rows (PF_F16X2 / PF_F16X1, 256 B per row; needs the rows' norm bound -- measured here when not given) or split-bf16
    (PF_BF16X3, 512 B per row)."""
    torch = _lib.require_gpu()
    _f32_cuda(db, "db", DIM)
    fmt = pf_default_format() if fmt is None else int(fmt)
    n = db.shape[0]
    need = int(_lib.load().ms_pf_image_bytes(n, fmt))
    if fmt != PF_BF16X3 and row_norm_bound is None:
        row_norm_bound = (float(1.0 / row_inv_norms(db, 1e-30).min()) * (1.0 + 1e-6)) if n > 0 else 1.0
    img = torch.empty(max(need, 16), dtype=torch.uint8, device=db.device) if out is None else out
    if img.dtype != torch.uint8 or img.numel() < need or not img.is_contiguous():
        raise MerizoHipError("pf_build_image: out must be a contiguous uint8 tensor of ms_pf_image_bytes(n, fmt)")
    with _on(db, img) as dev:
        check(_lib.load().ms_pf_build_image(ptr(db), n, fmt, float(row_norm_bound or 0.0), ptr(img), dev.stream), "ms_pf_build_image")
    return PfImage(img, fmt, n)


def pf_choose_format(db, image: PfImage, row_norm_bound: float, nsample: int = 256, k: int = 10, max_flagged: float = 0.02) -> PfImage:
    """F16X1 or F16X2 for a resident database, decided ONCE by running the search itself: `nsample` rows of the database, evenly
    spaced, are searched as queries (top-k) with the one-instruction arithmetic (MS_PF_F16X1: E = 1.05e-3 |row||q|); if more than
    `max_flagged` of them fail their proof -- the database has families of rows within ~1e-3 of each other around its own entries,
    as real embedding databases do -- the two-instruction arithmetic (MS_PF_F16X2, E = 5.5e-4) is used from then on (the SAME
    image: nothing is rebuilt).  The answers are exact either way; this only picks the faster of two exact paths.  One sync."""
    torch = _lib.require_gpu()
    if image is None or image.format == PF_BF16X3:
        return image
    n = db.shape[0]
    if not prefilter_serves(n, max(nsample, 65), k):
        return image
    idx = (torch.arange(nsample, dtype=torch.int64, device=db.device) * (n - 1)) // max(1, nsample - 1)      # (integers: float32 cannot count 45 M rows)
    q = db[idx].contiguous()
    ws = PrefilterWorkspace(db.device).get(n, nsample, k)
    ip_topk_prefiltered(db, q, k, row_norm_bound, mode=MODE_IP_NORMQ, workspace=ws, image=image.as_format(PF_F16X1))
    flagged = prefilter_flagged(ws)
    return image.as_format(PF_F16X1 if flagged <= max_flagged * nsample else PF_F16X2)


def small_batch_thresholds():
    """(fused_merge_max_nq, inkernel_norm_max_nq) as the loaded library applies them (ms_small_batch_thresholds)."""
    import ctypes
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().ms_small_batch_thresholds(ctypes.byref(a), ctypes.byref(b))
    return int(a.value), int(b.value)


def prefilter_serves(n: int, nq: int, k: int, image=None) -> bool:
    """The shapes ms_ip_topk_prefiltered serves itself (everything else it hands to ms_ip_topk): ONE statement of the rule for the
    engine, the bench and the tests (the library applies the same in pf_layout).  More than 64 queries, k <= 48, >= 65,536 rows; and,
    over an fp16 `image` (a PfImage, or a format), ANY number of queries from ms_pf_few_min_rows(nq) rows on (1M rows for 1..32 queries:
    the HBM-bound regime at half the bytes; 200k rows for 33..64: two query tiles of fp32 matrix work against one fp16 pass)."""
    if k > _lib.PREFILTER_MAX_K or n < _lib.PREFILTER_MIN_ROWS:
        return False
    if nq > 64:
        return True
    fmt = image.format if isinstance(image, PfImage) else image
    return fmt in (PF_F16X2, PF_F16X1) and n >= int(_lib.load().ms_pf_few_min_rows(int(nq)))


def _pf_args(db, image, q, mode, lengths, qlen):
    _f32_cuda(db, "db", DIM)
    _f32_cuda(q, "q", DIM)
    if mode not in (MODE_IP_PRENORM, MODE_IP_NORMQ, MODE_COSINE_UNIT):
        raise MerizoHipError("ip_topk_prefiltered: MODE_IP_PRENORM, MODE_IP_NORMQ or MODE_COSINE_UNIT")
    if mode != MODE_COSINE_UNIT and (lengths is not None or qlen is not None):
        raise MerizoHipError("ip_topk_prefiltered: lengths / qlen go with MODE_COSINE_UNIT")
    if image is not None and (not isinstance(image, PfImage) or image.n != db.shape[0] or
                              image.data.numel() < int(_lib.load().ms_pf_image_bytes(db.shape[0], image.format))):
        raise MerizoHipError("ip_topk_prefiltered: image is not pf_build_image(db)")
    _row_vectors(("lengths", lengths, db.shape[0]), ("qlen", qlen, q.shape[0]))


def ip_topk_prefiltered(db, q, k: int, row_norm_bound: float = 1.0, mode: int = MODE_IP_PRENORM, row_offset: int = 0,
                        workspace=None, out=None, image=None, lengths=None, qlen=None, mincov: float = 0.0):
    """ip_topk with the same results bit for bit, several times faster for more than 64 queries and k <= 48: 16-bit prefilter
    scan (over `image` = pf_build_image(db) -- fp16 or split-bf16 -- when given, else splitting the rows in registers), exact re-scoring, per-query proof,
    and an exact fp32 pass over the queries whose proof failed (include/merizo_search_amd.h).  row_norm_bound: an upper bound on
    every row's L2 norm (1.0 + 1e-6 for unit rows).  workspace: a PrefilterWorkspace or a uint8 tensor of
    ms_ip_topk_prefiltered_workspace_bytes."""
    torch = _lib.require_gpu()
    _pf_args(db, image, q, mode, lengths, qlen)
    n, nq = db.shape[0], q.shape[0]
    ws = workspace if isinstance(workspace, torch.Tensor) else (workspace or PrefilterWorkspace(db.device)).get(n, nq, k)
    out_s, out_i = _out_pair(nq, k, db.device, out, "ip_topk_prefiltered")
    idata, ifmt = (image.data, image.format) if image is not None else (None, 0)
    with _on(db, q, ws, out_s, out_i, idata, lengths, qlen) as dev:
        check(_lib.load().ms_ip_topk_prefiltered(ptr(db), ptr(idata), ifmt, n, row_offset, ptr(q), nq, k, mode, ptr(lengths), ptr(qlen), mincov,
                                                 float(row_norm_bound), ptr(out_s), ptr(out_i), ptr(ws), ws.numel(), dev.stream),
              "ms_ip_topk_prefiltered")
    return out_s, out_i


def ip_topk_prefiltered_stage(stage: str, db, q, k: int, ws, row_norm_bound: float = 1.0, mode: int = MODE_IP_PRENORM,
                              out=None, row_offset: int = 0, image=None, lengths=None, qlen=None, mincov: float = 0.0):
    """One stage of ip_topk_prefiltered ('prepare', 'scan', 'finish'): lets a bench time the scan launch alone."""
    lib = _lib.load()
    n, nq = db.shape[0], q.shape[0]
    idata, ifmt = (image.data, image.format) if image is not None else (None, 0)
    fin = stage not in ("prepare", "scan")          # 'finish' also takes the row offset and the outputs
    name = "ms_ip_topk_prefiltered_" + ("finish" if fin else stage)
    with _on(db, q, ws, idata, lengths, qlen) as dev:
        args = (ptr(db), ptr(idata), ifmt, n) + ((row_offset,) if fin else ()) + (
            ptr(q), nq, k, mode, ptr(lengths), ptr(qlen), mincov, float(row_norm_bound)) + (
            (ptr(out[0]), ptr(out[1])) if fin else ()) + (ptr(ws), ws.numel(), dev.stream)
        check(getattr(lib, name)(*args), name)


def prefilter_flagged(ws) -> int:
    """Diagnostics (synchronises): how many queries of the last prefiltered search on this workspace needed the exact pass."""
    import ctypes
    g, e, c = ctypes.c_uint(0), ctypes.c_uint(0), ctypes.c_uint(0)
    check(_lib.load().ms_debug_prefilter_state(ptr(ws), ctypes.byref(g), ctypes.byref(e), ctypes.byref(c)), "ms_debug_prefilter_state")
    return int(c.value) if e.value != 0 else 0


def prefilter_poison(ws, slot_counter: int, ticket: int) -> None:
    """Diagnostics for the tests (synchronises): overwrite the compaction's slot counter and ticket in the library-owned block of this
    workspace -- the state an aborted launch or a second stream on the workspace would leave (ms_debug_prefilter_poison).  The next
    prefiltered search on `ws` must fail loudly."""
    check(_lib.load().ms_debug_prefilter_poison(ptr(ws), int(slot_counter) & 0xFFFFFFFF, int(ticket) & 0xFFFFFFFF), "ms_debug_prefilter_poison")


def device_pci_bus_id(device=None) -> str:
    """PCI bus id of `device` (default: torch's current device), e.g. '0000:c1:00.0' (ms_device_pci_bus_id)."""
    import ctypes
    torch = _lib.require_gpu()
    buf = ctypes.create_string_buffer(64)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(_lib.load().ms_device_pci_bus_id(buf, 64), "ms_device_pci_bus_id")
    return buf.value.decode()


def prefilter_fell_back(ws) -> bool:
    """Diagnostics (synchronises): did any query of the last prefiltered search on this workspace need the exact pass?"""
    return prefilter_flagged(ws) > 0


def topk_merge(scores, idx):
    """Merge [S,nq,k] sorted result lists (shards or blocks) into [nq,k]."""
    torch = _lib.require_gpu()
    if scores.dim() != 3 or idx.shape != scores.shape:
        raise MerizoHipError("topk_merge: expected scores/idx of shape [S,nq,k]")
    scores = scores.contiguous()
    idx = idx.contiguous()
    if scores.dtype != torch.float32 or idx.dtype != torch.int64 or not scores.is_cuda:
        raise MerizoHipError("topk_merge: expected float32 / int64 CUDA tensors")
    S, nq, k = scores.shape
    out_s, out_i = _out_pair(nq, k, scores.device, None, "topk_merge")
    with _on(scores, idx) as dev:
        check(_lib.load().ms_topk_merge(ptr(scores), ptr(idx), S, nq, k, ptr(out_s), ptr(out_i), dev.stream),
              "ms_topk_merge")
    return out_s, out_i


def topk_merge_packed(gathered, S: int, nq: int, k: int, idx_offset: int, out_s, out_i):
    """Merge S packed result blocks [scores f32 nq*k | pad | rows i64 nq*k] laid out back to back in the
    uint8 buffer ``gathered`` (the all-gather output) without unpacking them."""
    torch = _lib.require_gpu()
    if gathered.dtype != torch.uint8 or not gathered.is_cuda or not gathered.is_contiguous():
        raise MerizoHipError("topk_merge_packed: expected a contiguous uint8 CUDA buffer")
    stride = gathered.numel() // S
    if stride * S != gathered.numel() or stride < idx_offset + 8 * nq * k:
        raise MerizoHipError("topk_merge_packed: buffer size does not match S blocks of nq*k results")
    base = gathered.data_ptr()
    with _on(gathered, out_s, out_i) as dev:
        check(_lib.load().ms_topk_merge_strided(base, base + idx_offset, stride, stride, S, nq, k, ptr(out_s), ptr(out_i),
                                                dev.stream), "ms_topk_merge_strided")
    return out_s, out_i


def topk_drop_ranges(scores, idx, lo, hi, kout: int, min_score: float = float("-inf"), out=None):
    """Drop from sorted top-k lists [nq,kin] the entries whose row lies in [lo[q], hi[q]) and those scoring below min_score;
    the first kout of what remains, in order, (-inf, -1) behind them (ms_topk_drop_ranges).
    -> (scores f32 [nq,kout], idx i64 [nq,kout], count i32 [nq]).  Exact top-kout of the database without those rows when
    the input is the exact top-kin and kin >= kout + max(hi - lo).  Asynchronous; out: optional preallocated triple."""
    torch = _lib.require_gpu()
    if (not isinstance(scores, torch.Tensor) or not isinstance(idx, torch.Tensor) or scores.dim() != 2 or idx.shape != scores.shape
            or scores.dtype != torch.float32 or idx.dtype != torch.int64 or not scores.is_cuda):
        raise MerizoHipError("topk_drop_ranges: expected float32 / int64 CUDA tensors of one shape [nq,kin]")
    scores, idx = scores.contiguous(), idx.contiguous()
    nq, kin = scores.shape
    kout = int(kout)
    if nq < 1 or not 1 <= kout <= kin:
        raise MerizoHipError(f"topk_drop_ranges: need nq >= 1 and 1 <= kout <= kin (nq={nq} kin={kin} kout={kout})")
    lo, hi = (_int_desc(x, np.int64, name, scores.device, "topk_drop_ranges", length=nq) for name, x in (("lo", lo), ("hi", hi)))
    out_s, out_i, out_c = _outputs("topk_drop_ranges", ((torch.float32, (nq, kout)), (torch.int64, (nq, kout)), (torch.int32, (nq,))), out,
                                   scores.device)
    with _on(scores, idx, lo, hi, out_s, out_i, out_c) as dev:
        check(_lib.load().ms_topk_drop_ranges(ptr(scores), ptr(idx), nq, kin, ptr(lo), ptr(hi), float(min_score), int(kout),
                                              ptr(out_s), ptr(out_i), ptr(out_c), dev.stream), "ms_topk_drop_ranges")
    return out_s, out_i, out_c


def topk_excluding(db, q, k: int, lo, hi, mode: int = MODE_IP_PRENORM, row_norm_bound=None, image=None,
                   min_score: float = float("-inf"), row_offset: int = 0, lengths=None, qlen=None, mincov: float = 0.0,
                   workspace=None, max_excluded: Optional[int] = None):
    """Exact top-k of q against db WITHOUT the rows [lo[q], hi[q]) of each query (global row numbers, as the search
    reports them: row_offset + row) -> (scores [nq,k], idx [nq,k], count [nq]).  The search runs with
    k' = k + max(hi - lo) -- the prefiltered search when a row_norm_bound is given and prefilter_serves(n, nq, k', image),
    ip_topk_large when one is given and large_k_serves(n, nq, k'), ms_ip_topk otherwise -- and ms_topk_drop_ranges takes the excluded rows out again (exactness: the header).
    lo / hi: int64 [nq], host arrays or tensors; max_excluded: max(hi - lo) when the caller knows it (a device tensor
    costs a sync to find it).  min_score: also drop the entries scoring below it."""
    torch = _lib.require_gpu()
    nq = q.shape[0]
    if max_excluded is None:
        if isinstance(lo, torch.Tensor) or isinstance(hi, torch.Tensor):
            span = torch.as_tensor(hi).to(torch.int64).cpu() - torch.as_tensor(lo).to(torch.int64).cpu()
            max_excluded = int(span.max()) if nq else 0
        else:
            max_excluded = int((np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64)).max()) if nq else 0
    kk = int(k) + max(0, int(max_excluded))
    n = db.shape[0]
    if row_norm_bound is not None and prefilter_serves(n, nq, kk, image):
        s, i = ip_topk_prefiltered(db, q, kk, float(row_norm_bound), mode=mode, row_offset=row_offset, image=image, lengths=lengths,
                                   qlen=qlen, mincov=mincov, workspace=workspace if isinstance(workspace, PrefilterWorkspace) else None)
    elif row_norm_bound is not None and mode != MODE_COSINE_RAW and large_k_serves(n, nq, kk):
        s, i = ip_topk_large(db, q, kk, float(row_norm_bound), mode=mode, lengths=lengths, qlen=qlen, mincov=mincov, row_offset=row_offset,
                             workspace=workspace if isinstance(workspace, LargeKWorkspace) else None)
    else:
        s, i = ip_topk(db, q, kk, mode=mode, lengths=lengths, qlen=qlen, mincov=mincov, row_offset=row_offset,
                       workspace=workspace if isinstance(workspace, TopKWorkspace) and not isinstance(workspace, PrefilterWorkspace) else None)
    return topk_drop_ranges(s, i, lo, hi, int(k), min_score)


def cluster_greedy(nbr_idx, nbr_score, lengths, min_score: float, mincov: float = 0.0, out=None, workspace=None):
    """Greedy representative clustering of n rows from their neighbour lists (ms_cluster_greedy: the definition is the
    header's).  nbr_idx int64 [n,k], nbr_score float32 [n,k] as topk_drop_ranges writes them, lengths int32 [n] (a tensor, or a
    host array that is uploaded).  -> (rep int64 [n], rep_score float32 [n], info) with info = {'n_reps', 'rounds',
    'saturated'}.  Synchronises: the call returns when the clustering has finished.  out: optional preallocated (rep,
    rep_score); workspace: optional uint8 tensor of ms_cluster_workspace_bytes(n)."""
    return _cluster("cluster_greedy", "ms_cluster_greedy", "ms_cluster_workspace_bytes", "n_reps", nbr_idx, nbr_score, None, lengths, min_score,
                    mincov, out, workspace)


def _cluster_graph(who, nbr_idx, nbr_score, edges, lengths):
    """The graph arguments every cluster call takes, checked once: lists int64 / float32 [n,k] or None None, edges = (edge_src,
    edge_dst, edge_score) int64 / int64 / float32 [m] or None (an entry point without edge arguments: its lists need k >= 1),
    lengths int32 [n] (a tensor, or a host array that is uploaded).  -> (lengths tensor, n, k, m)."""
    torch = _lib.require_gpu()
    edge_src, edge_dst, edge_score = edges or (None, None, None)
    device = next((x.device for x in (nbr_score, edge_score, lengths) if isinstance(x, torch.Tensor) and x.is_cuda), None)
    t = _int_desc(lengths, np.int32, "lengths", device or torch.device("cuda", torch.cuda.current_device()), who)
    n = int(t.numel())
    if n < 1:
        raise MerizoHipError(f"{who}: lengths: expected n >= 1 integers, got none")
    if (nbr_idx is None) != (nbr_score is None) or len({edge_src is None, edge_dst is None, edge_score is None}) != 1:
        raise MerizoHipError(f"{who}: the two list tensors go together, and so do the three edge tensors")
    k = 0
    if nbr_idx is not None:
        if (not isinstance(nbr_idx, torch.Tensor) or not isinstance(nbr_score, torch.Tensor) or nbr_score.dim() != 2
                or nbr_idx.shape != nbr_score.shape or nbr_score.dtype != torch.float32 or nbr_idx.dtype != torch.int64
                or not nbr_score.is_cuda or not (nbr_idx.is_contiguous() and nbr_score.is_contiguous())):
            raise MerizoHipError(f"{who}: expected contiguous int64 / float32 CUDA tensors of one shape [n,k]")
        if nbr_score.shape[0] != n:
            raise MerizoHipError(f"{who}: lengths: expected {nbr_score.shape[0]} integers, one per row of the lists, got {n}")
        k = int(nbr_score.shape[1])
    if edges is None and k < 1:
        raise MerizoHipError(f"{who}: need n >= 1 and k >= 1 (n={n} k={k})")
    m = 0
    if edge_src is not None:
        for name, e, dtype in (("edge_src", edge_src, torch.int64), ("edge_dst", edge_dst, torch.int64), ("edge_score", edge_score, torch.float32)):
            if not isinstance(e, torch.Tensor) or not e.is_cuda or e.dtype != dtype or e.dim() != 1 or not e.is_contiguous():
                raise MerizoHipError(f"{who}: {name}: expected a contiguous {dtype} CUDA/HIP tensor [m]")
        m = int(edge_src.numel())
        if edge_dst.numel() != m or edge_score.numel() != m:
            raise MerizoHipError(f"{who}: edge_src, edge_dst and edge_score must have one length")
    return t, n, k, m


def _graph_call(entry, nbr_idx, nbr_score, edges, t, n, k, m, min_score, mincov, others, rest):
    """One call shape for every entry point that takes the graph: lists, n, k[, extras, m], lengths, min_score, mincov, then `rest`
    (a function of the stream) -- on the device of the graph's tensors and of `others`."""
    edge_src, edge_dst, edge_score = edges or (None, None, None)
    extra = () if edges is None else (ptr(edge_src) if m else 0, ptr(edge_dst) if m else 0, ptr(edge_score) if m else 0, m)
    with _on(nbr_idx, nbr_score, edge_src, edge_dst, edge_score, t, *others) as dev:
        check(getattr(_lib.load(), entry)(ptr(nbr_idx) if k else 0, ptr(nbr_score) if k else 0, n, k, *extra, ptr(t), float(min_score),
                                          float(mincov), *rest(dev.stream)), entry)


def _cluster(who, entry, workspace_bytes, count_key, nbr_idx, nbr_score, edges, lengths, min_score, mincov, out, workspace):
    """The three cluster calls: one argument check (_cluster_graph), one call shape (`entry`, `workspace_bytes`: the library's names;
    count_key: what the first count is called in info).  edges: (edge_src, edge_dst, edge_score), or None for ms_cluster_greedy,
    whose entry point takes no edge arguments and needs lists of k >= 1."""
    import ctypes
    torch = _lib.require_gpu()
    t, n, k, m = _cluster_graph(who, nbr_idx, nbr_score, edges, lengths)
    rep, rep_score = _outputs(who, ((torch.int64, (n,)), (torch.float32, (n,))), out, t.device)
    workspace = _workspace(who, workspace_bytes, (n,), workspace, t.device)
    n_reps, rounds, saturated = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
    _graph_call(entry, nbr_idx, nbr_score, edges, t, n, k, m, min_score, mincov, (rep, rep_score, workspace),
                lambda stream: (ptr(rep), ptr(rep_score), ctypes.addressof(n_reps), ctypes.addressof(rounds), ctypes.addressof(saturated),
                                ptr(workspace), workspace.numel(), stream))
    return rep, rep_score, {count_key: int(n_reps.value), "rounds": int(rounds.value), "saturated": int(saturated.value)}


def cluster_greedy_edges(nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score: float, mincov: float = 0.0, out=None,
                         workspace=None):
    """cluster_greedy over the union of the lists and m extra directed entries edge_src[e] -> edge_dst[e] with score edge_score[e]
    (ms_cluster_greedy_edges: the definition is the header's).  nbr_idx int64 [n,k] / nbr_score float32 [n,k], or None None (k = 0:
    extra entries only); edge_src / edge_dst int64 [m], edge_score float32 [m] CUDA/HIP tensors, or None None None (m = 0);
    lengths int32 [n] says what n is.  -> (rep, rep_score, info) as cluster_greedy; 'saturated' counts over the lists only."""
    return _cluster("cluster_greedy_edges", "ms_cluster_greedy_edges", "ms_cluster_workspace_bytes", "n_reps", nbr_idx, nbr_score,
                    (edge_src, edge_dst, edge_score), lengths, min_score, mincov, out, workspace)


def cluster_components(nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score: float, mincov: float = 0.0, out=None,
                       workspace=None):
    """Connected components of the graph cluster_greedy_edges clusters (ms_cluster_components: the definition is the header's), with
    its arguments: lists or None None, extra entries or None None None, lengths int32 [n].  -> (rep int64 [n], link_score float32
    [n], info): rep[i] the highest-priority row of i's component, link_score[i] 1.0 for a representative and otherwise the largest
    weight among the row's own edges; info = {'n_components', 'rounds', 'saturated'} ('rounds' may differ from run to run).
    Synchronises.  out: optional preallocated (rep, link_score); workspace: optional uint8 tensor of
    ms_cluster_components_workspace_bytes(n)."""
    return _cluster("cluster_components", "ms_cluster_components", "ms_cluster_components_workspace_bytes", "n_components", nbr_idx,
                    nbr_score, (edge_src, edge_dst, edge_score), lengths, min_score, mincov, out, workspace)


def cluster_tree(nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score: float, mincov: float = 0.0, out=None,
                 workspace=None):
    """The single-linkage tree of the graph cluster_components reads (ms_cluster_tree: the definition is the header's), with its
    arguments: the maximum spanning forest under the order weight descending, then (min row, max row) ascending.  -> (pairs int32
    [n,2], weight float32 [n], info): slot r holds the edge {a, b}, a < b, by which row r stopped being the root of its tree, and
    its weight; (-1, -1) and -inf: the row never hooked.  info = {'n_edges' (= n - components), 'rounds' (<= floor(log2 n) + 1, a
    function of the entries), 'saturated'}.  Cutting the forest at any T >= min_score gives the components of the graph at T.
    Synchronises.  out: optional preallocated (pairs, weight); workspace: optional uint8 tensor of ms_cluster_tree_workspace_bytes(n)."""
    import ctypes
    who = "cluster_tree"
    torch = _lib.require_gpu()
    edges = (edge_src, edge_dst, edge_score)
    t, n, k, m = _cluster_graph(who, nbr_idx, nbr_score, edges, lengths)
    pairs, weight = _outputs(who, ((torch.int32, (n, 2)), (torch.float32, (n,))), out, t.device)
    workspace = _workspace(who, "ms_cluster_tree_workspace_bytes", (n,), workspace, t.device)
    n_edges, rounds, saturated = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
    _graph_call("ms_cluster_tree", nbr_idx, nbr_score, edges, t, n, k, m, min_score, mincov, (pairs, weight, workspace),
                lambda stream: (ptr(pairs), ptr(weight), ctypes.addressof(n_edges), ctypes.addressof(rounds), ctypes.addressof(saturated),
                                ptr(workspace), workspace.numel(), stream))
    return pairs, weight, {"n_edges": int(n_edges.value), "rounds": int(rounds.value), "saturated": int(saturated.value)}


def _pairs_workspace(who, n, k, m, workspace, device):
    if n * k + m >= 2 ** 31:
        raise MerizoHipError(f"{who}: n k + m = {n * k + m} directed entries, the set holds fewer than 2^31 (MS_ERR_RANGE (-4))")
    return _workspace(who, "ms_cluster_pairs_workspace_bytes", (n, k, m), workspace, device)


def cluster_pairs(nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score: float, mincov: float = 0.0, cap=None, out=None,
                  workspace=None):
    """The distinct canonical pairs (a, b) -- a the higher-priority row -- of the graph cluster_greedy_edges clusters, with its
    arguments (ms_cluster_pairs: the definition is the header's).  cap: slots of the pair buffer (default n k + m: every pair
    fits; 0: count only).  -> (pairs int32 [cap,2], count int64 [2], workspace), device tensors: count[0] the distinct pairs (exact
    whatever cap), count[1] the rows whose k list entries are all valid; pairs[:min(count[0], cap)] hold the pairs in unspecified
    order; the workspace holds the set for cluster_pairs_apply / cluster_pairs_find.  Asynchronous: nothing is read back.
    out: optional preallocated (pairs, count); workspace: optional uint8 tensor of ms_cluster_pairs_workspace_bytes(n, k, m)."""
    who = "cluster_pairs"
    torch = _lib.require_gpu()
    edges = (edge_src, edge_dst, edge_score)
    t, n, k, m = _cluster_graph(who, nbr_idx, nbr_score, edges, lengths)
    if cap is None:                                      # (a caller's pair buffer says what its cap is)
        cap = n * k + m if out is None or not isinstance(out[0], torch.Tensor) else int(out[0].shape[0])
    cap = int(cap)
    if cap < 0:
        raise MerizoHipError(f"{who}: need cap >= 0, got {cap}")
    pairs, count = _outputs(who, ((torch.int32, (cap, 2)), (torch.int64, (2,))), out, t.device)
    workspace = _pairs_workspace(who, n, k, m, workspace, t.device)
    _graph_call("ms_cluster_pairs", nbr_idx, nbr_score, edges, t, n, k, m, min_score, mincov, (pairs, count, workspace),
                lambda stream: (ptr(pairs) if cap else 0, cap, ptr(count), ptr(workspace), workspace.numel(), stream))
    return pairs, count, workspace


def cluster_pairs_apply(nbr_idx, nbr_score, edge_src, edge_dst, edge_score, lengths, min_score: float, mincov: float, keep, workspace):
    """Take the pairs with keep[slot] == 0 out of the graph IN PLACE, in both directions (ms_cluster_pairs_apply: the definition is
    the header's): the graph arguments and thresholds of the cluster_pairs call that left `workspace`, keep uint8 [count] on the
    device, indexed by slot.  A valid entry without a verdict (pair not in the set, slot >= count or >= that call's cap) is removed
    too.  -> the directed entries removed, a device tensor int64 [1].  Asynchronous."""
    who = "cluster_pairs_apply"
    torch = _lib.require_gpu()
    edges = (edge_src, edge_dst, edge_score)
    t, n, k, m = _cluster_graph(who, nbr_idx, nbr_score, edges, lengths)
    if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype != torch.uint8 or keep.dim() != 1 or not keep.is_contiguous():
        raise MerizoHipError(f"{who}: keep: expected a contiguous uint8 CUDA/HIP tensor [count]")
    if workspace is None:
        raise MerizoHipError(f"{who}: needs the workspace cluster_pairs returned")
    workspace = _pairs_workspace(who, n, k, m, workspace, t.device)
    removed = torch.empty((1,), dtype=torch.int64, device=t.device)
    count = int(keep.numel())
    _graph_call("ms_cluster_pairs_apply", nbr_idx, nbr_score, edges, t, n, k, m, min_score, mincov, (keep, workspace, removed),
                lambda stream: (ptr(keep) if count else 0, count, ptr(workspace), workspace.numel(), ptr(removed), stream))
    return removed


def cluster_pairs_find(a, b, lengths, workspace):
    """The slot of every unordered pair {a[e], b[e]} in the set cluster_pairs left in `workspace` (ms_cluster_pairs_find): a / b
    int64 [cnt] tensors or host arrays, lengths int32 [n] as in that call.  -> slot int64 [cnt] on the device; -1: not in the set,
    a row outside [0, n), or a[e] == b[e].  Asynchronous."""
    who = "cluster_pairs_find"
    torch = _lib.require_gpu()
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda:
        raise MerizoHipError(f"{who}: needs the workspace cluster_pairs returned")
    t = _int_desc(lengths, np.int32, "lengths", workspace.device, who)
    n = int(t.numel())
    if n < 1:
        raise MerizoHipError(f"{who}: lengths: expected n >= 1 integers, got none")
    a = _int_desc(a, np.int64, "a", workspace.device, who)
    b = _int_desc(b, np.int64, "b", workspace.device, who, length=int(a.numel()))
    workspace = _pairs_workspace(who, n, 0, 0, workspace, workspace.device)
    cnt = int(a.numel())
    slot = torch.empty((cnt,), dtype=torch.int64, device=workspace.device)
    with _on(a, b, t, workspace, slot) as dev:
        check(_lib.load().ms_cluster_pairs_find(ptr(a) if cnt else 0, ptr(b) if cnt else 0, cnt, ptr(t), n, ptr(workspace), workspace.numel(),
                                                ptr(slot) if cnt else 0, dev.stream), "ms_cluster_pairs_find")
    return slot


THRESHOLD_EDGES_CAP = 1 << 16      # slots of threshold_edges' first launch when the caller names none (it launches again beyond)


def threshold_edges(db, q, mode: int, min_score: float, row_norm_bound: float, lo=None, hi=None, row_offset: int = 0,
                    cap: int = THRESHOLD_EDGES_CAP, out=None, workspace=None, stats=None):
    """Every (query, row) cell of db float32 [n,128] x q float32 [nq,128] (raw, as the search of `mode` takes them) that scores at or
    above min_score and whose global row row_offset + r lies outside [lo[qi], hi[qi]) (ms_threshold_edges: the definition is the
    header's; the score is ip_topk's for that query and row, bit for bit).  lo / hi: int64 [nq] tensors or host arrays, both or neither.
    -> (src int64 [count], dst int64 [count], score float32 [count], count) in unspecified order; src = the query's number,
    dst = the global row.  Synchronises (it reads the count back) and launches a second time with a buffer of `count` slots when
    more than `cap` cells qualify -- unless out = (src, dst, score) preallocated tensors of one length (the cap) is given: then
    count may exceed what was written (the first min(count, cap) slots) and the caller decides.
    stats: a dict that receives 'rescored', the cells of the last launch that went to the exact chain."""
    torch = _lib.require_gpu()
    _f32_cuda(db, "db", DIM)
    _f32_cuda(q, "q", DIM)
    n, nq = db.shape[0], q.shape[0]
    if (lo is None) != (hi is None):
        raise MerizoHipError("threshold_edges: lo and hi go together")
    if lo is not None:
        lo, hi = (_int_desc(x, np.int64, name, db.device, "threshold_edges", length=nq) for name, x in (("lo", lo), ("hi", hi)))
    workspace = _workspace("threshold_edges", "ms_threshold_edges_workspace_bytes", (n, nq), workspace, db.device)
    count = torch.zeros(1, dtype=torch.int64, device=db.device)
    st = torch.zeros(1, dtype=torch.int64, device=db.device)

    def launch(bufs, slots):
        src, dst, score = bufs
        with _on(db, q, lo, hi, src, dst, score, count, st, workspace) as d:
            check(_lib.load().ms_threshold_edges(ptr(db), n, int(row_offset), ptr(q), nq, int(mode), ptr(lo), ptr(hi), float(min_score),
                                                 float(row_norm_bound), ptr(src), ptr(dst), ptr(score), int(slots), ptr(count), ptr(st),
                                                 ptr(workspace), workspace.numel(), d.stream), "ms_threshold_edges")
        return int(count.item())

    def buffers(slots, out=None):         # (src, dst, score) of `slots` entries each
        return _outputs("threshold_edges", ((torch.int64, (slots,)), (torch.int64, (slots,)), (torch.float32, (slots,))), out, db.device)

    if out is not None:
        cap = int(out[0].numel()) if isinstance(out[0], torch.Tensor) else 0           # (the first tensor says what the one length is)
        src, dst, score = buffers(cap, out)
        found = launch(out, cap)
    else:
        (src, dst, score), cap, found = _capped_relaunch(launch, lambda slots: buffers(max(slots, 1)), cap)
    if stats is not None:
        stats["rescored"] = int(st.item())
    kept = min(found, cap)
    return src[:kept], dst[:kept], score[:kept], found


def md_chain_scores(db, q, mode: int, cand, trows, mat_off, min_score: float, lengths=None, qlen=None, mincov: float = 0.0,
                    out=None, workspace=None):
    """Score matrices of (query chain, target chain) candidates (ms_md_chain_scores: the definition is the header's).
    db float32 [n,128], q float32 [nq,128] (raw, as the search of `mode` takes them); cand int32 [ncand,4] = (q0, nqd, t_off,
    nhd), trows int64 [ntrows], mat_off int64 [ncand]: tensors, or host arrays that are uploaded.
    -> (scores float32 [total], match int32 [ncand,2]); candidate c's matrix is scores[mat_off[c]:][:nqd * nhd] row-major,
    every cell bit for bit the score ip_topk gives that (query, row) in `mode`, below min_score -> +0.0.  Asynchronous.
    out: optional preallocated (scores, match) -- without it `scores` is sized from the descriptors (zero-filled, so gaps
    between matrices read 0; device descriptors cost a copy to the host for that); workspace: optional uint8 tensor of
    ms_md_chain_scores_workspace_bytes(nq)."""
    torch = _lib.require_gpu()
    _f32_cuda(db, "db", DIM)
    _f32_cuda(q, "q", DIM)
    n, nq = db.shape[0], q.shape[0]
    _row_vectors(("lengths", lengths, n), ("qlen", qlen, nq))
    cand_t = _int_desc(cand, np.int32, "cand", db.device, "md_chain_scores", cols=4)
    ncand = cand_t.shape[0]
    trows_t = _int_desc(trows, np.int64, "trows", db.device, "md_chain_scores")
    off_t = _int_desc(mat_off, np.int64, "mat_off", db.device, "md_chain_scores", length=ncand)
    if out is None:
        c_h = (cand if not isinstance(cand, torch.Tensor) else cand.cpu().numpy()).reshape(-1, 4).astype(np.int64)
        o_h = np.asarray(mat_off if not isinstance(mat_off, torch.Tensor) else mat_off.cpu().numpy(), dtype=np.int64).reshape(-1)
        ends = o_h + np.clip(c_h[:, 1], 0, None) * np.clip(c_h[:, 3], 0, None)
        total = int(ends.max()) if ncand else 0
        scores = torch.zeros((max(total, 1),), dtype=torch.float32, device=db.device)[:total]
        match = torch.empty((ncand, 2), dtype=torch.int32, device=db.device)
    else:
        scores, match = _outputs("md_chain_scores", ((torch.float32, None), (torch.int32, (ncand, 2))), out, db.device)
    if ncand == 0:                      # (nothing to score: the library would not launch either)
        return scores, match
    workspace = _workspace("md_chain_scores", "ms_md_chain_scores_workspace_bytes", (nq,), workspace, db.device)
    with _on(db, q, lengths, qlen, cand_t, trows_t, off_t, scores, match, workspace) as d:
        check(_lib.load().ms_md_chain_scores(ptr(db), n, ptr(q), nq, int(mode), ptr(lengths), ptr(qlen), float(mincov), ptr(cand_t), ncand,
                                             ptr(trows_t), trows_t.numel(), ptr(off_t), float(min_score), ptr(scores), ptr(match),
                                             ptr(workspace), workspace.numel(), d.stream), "ms_md_chain_scores")
    return scores, match


MD_BEST_MAX_QD, MD_BEST_MAX_HD = 64, 1024      # ms_md_best_mappings' limits (include/merizo_search_amd.h: 64, MS_MD_BEST_MAX_HD)


def md_best_mappings(scores, cand, mat_off, out=None, workspace=None):
    """The best any-order and the best order-preserving mapping of every candidate matrix (ms_md_best_mappings: the definition
    is the header's).  scores float32 [total_cells]: the CUDA/HIP tensor md_chain_scores returned; cand int32 [ncand,4] and
    mat_off int64 [ncand] as that call took them: tensors, or host arrays that are uploaded.
    -> (status int32 [ncand,2], total int64 [ncand,2], path int32 [ncand,2,64], cell float32 [ncand,2,64]) on the device, every
    entry written.  Asynchronous.  out: optional preallocated (status, total, path, cell); workspace: optional uint8 tensor of
    ms_md_best_mappings_workspace_bytes(ncand, total_cells) bytes, reusable as it is."""
    torch = _lib.require_gpu()
    _f32_cuda(scores, "scores")
    if scores.dim() != 1:
        raise MerizoHipError(f"md_best_mappings: scores: expected float32 [total_cells], got shape {tuple(scores.shape)}")
    cand_t = _int_desc(cand, np.int32, "cand", scores.device, "md_best_mappings", cols=4)
    ncand, total_cells = cand_t.shape[0], int(scores.numel())
    off_t = _int_desc(mat_off, np.int64, "mat_off", scores.device, "md_best_mappings", length=ncand)
    status, total, path, cell = _outputs("md_best_mappings", ((torch.int32, (ncand, 2)), (torch.int64, (ncand, 2)),
                                                              (torch.int32, (ncand, 2, MD_BEST_MAX_QD)), (torch.float32, (ncand, 2, MD_BEST_MAX_QD))),
                                         out, scores.device)
    if ncand == 0:                      # (nothing to solve: the library would not launch either)
        return status, total, path, cell
    workspace = _workspace("md_best_mappings", "ms_md_best_mappings_workspace_bytes", (ncand, total_cells), workspace, scores.device)
    with _on(scores, cand_t, off_t, status, total, path, cell, workspace) as d:
        check(_lib.load().ms_md_best_mappings(ptr(scores), total_cells, ptr(cand_t), ncand, ptr(off_t), ptr(status), ptr(total), ptr(path),
                                              ptr(cell), ptr(workspace), workspace.numel(), d.stream), "ms_md_best_mappings")
    return status, total, path, cell


# Query rows from which md_chain_scan's route "auto" takes the matrix route: the smallest nq of tools/chain_search_bench.py's sweep from
# which ms_md_chain_scan_mq is faster than ms_md_chain_scan on both of its shapes (profiles/chain_search_bench.log).
MD_SCAN_MATRIX_MIN_NQ = 64
MD_SCAN_ROUTES = ("lane", "matrix", "auto")


def md_scan_route(route: str, nq: int, row_norm_bound) -> str:
    """The route one md_chain_scan call takes: "lane" (ms_md_chain_scan) or "matrix" (ms_md_chain_scan_mq; needs a row-norm bound).
    "auto": the matrix route from MD_SCAN_MATRIX_MIN_NQ query rows on when a bound is given."""
    if route not in MD_SCAN_ROUTES:
        raise MerizoHipError(f"md_chain_scan: route must be one of {MD_SCAN_ROUTES}, got {route!r}")
    if route == "matrix" and row_norm_bound is None:
        raise MerizoHipError("md_chain_scan: route 'matrix' needs row_norm_bound (1 + 1e-6 for unit rows)")
    if route == "auto":
        return "matrix" if row_norm_bound is not None and int(nq) >= MD_SCAN_MATRIX_MIN_NQ else "lane"
    return route


def md_chain_scan_launch(db, chain_start, q, mode: int, qchain, min_score: float, out_pairs, out_count, out_qstatus, cap: Optional[int] = None,
                         lengths=None, qlen=None, mincov: float = 0.0, workspace=None, route: str = "lane", row_norm_bound=None,
                         out_stats=None):
    """ONE ms_md_chain_scan call into preallocated outputs (the definition is the header's): db float32 [n,128], chain_start int64
    [nchains + 1], q float32 [nq,128] (raw, as the search of `mode` takes them), qchain int32 [nqc,2] = (q0, nqd), out_pairs int64
    [>= cap,2], out_count int64 [1], out_qstatus int32 [nqc] -- all device tensors.  cap: slots the call may write (default:
    all of out_pairs).  route: md_scan_route's; the matrix route is ms_md_chain_scan_mq with row_norm_bound and out_stats (int64 [1]
    device tensor or None: the cells it re-scored exactly).  A workspace serves one route.
    Asynchronous; -> the workspace used (reusable by the next call as it is)."""
    torch = _lib.require_gpu()
    _f32_cuda(db, "db", DIM)
    _f32_cuda(q, "q", DIM)
    n, nq = db.shape[0], q.shape[0]
    matrix = md_scan_route(route, nq, row_norm_bound) == "matrix"
    if out_stats is not None and (not isinstance(out_stats, torch.Tensor) or not out_stats.is_cuda or out_stats.dtype != torch.int64
                                  or out_stats.numel() < 1):
        raise MerizoHipError("md_chain_scan: out_stats: expected an int64 CUDA/HIP tensor of one element")
    _row_vectors(("lengths", lengths, n), ("qlen", qlen, nq))
    for name, t, dtype in (("chain_start", chain_start, torch.int64), ("qchain", qchain, torch.int32), ("out_pairs", out_pairs, torch.int64),
                           ("out_count", out_count, torch.int64), ("out_qstatus", out_qstatus, torch.int32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise MerizoHipError(f"md_chain_scan: {name}: expected a contiguous {dtype} CUDA/HIP tensor")
    nchains = max(int(chain_start.numel()) - 1, 0)
    nqc = int(qchain.numel()) // 2
    cap = int(out_pairs.numel()) // 2 if cap is None else int(cap)
    if qchain.numel() != 2 * nqc or out_qstatus.numel() < nqc or out_count.numel() < 1 or cap < 0 or 2 * cap > out_pairs.numel():
        raise MerizoHipError("md_chain_scan: qchain [nqc,2], out_qstatus [nqc], out_count [1] and out_pairs [>= cap,2] do not fit together")
    lib = _lib.load()
    workspace = _workspace("md_chain_scan", "ms_md_chain_scan_mq_workspace_bytes" if matrix else "ms_md_chain_scan_workspace_bytes", (n, nq),
                           workspace, db.device)
    with _on(db, q, lengths, qlen, chain_start, qchain, out_pairs, out_count, out_qstatus, out_stats, workspace) as d:
        args = (ptr(db), n, ptr(chain_start), nchains, ptr(q), nq, int(mode), ptr(lengths), ptr(qlen), float(mincov), ptr(qchain), nqc,
                float(min_score), ptr(out_pairs), cap, ptr(out_count), ptr(out_qstatus))
        if matrix:
            check(lib.ms_md_chain_scan_mq(*args, float(row_norm_bound), ptr(out_stats), ptr(workspace), workspace.numel(), d.stream),
                  "ms_md_chain_scan_mq")
        else:
            check(lib.ms_md_chain_scan(*args, ptr(workspace), workspace.numel(), d.stream), "ms_md_chain_scan")
    return workspace


def md_chain_scan(db, chain_start, q, mode: int, qchain, min_score: float, lengths=None, qlen=None, mincov: float = 0.0, cap: int = 4096,
                  route: str = "lane", row_norm_bound=None, stats=None):
    """Every (query chain, target chain) pair of a whole matrix that passes the mapping step's two early exits (ms_md_chain_scan).
    chain_start int64 [nchains + 1] and qchain int32 [nqc,2]: tensors, or host arrays that are uploaded.
    -> (pairs int64 [count,2] SORTED by (query chain, target chain), qstatus int32 [nqc]), numpy arrays: a function of the inputs
    alone.  Synchronises (it reads the count back); runs a second time with the exact count when more than `cap` pairs qualify.
    route, row_norm_bound: md_scan_route's -- the answer does not depend on them.  stats: a dict that receives 'route' and, on the
    matrix route, 'rescored' (cells of the last call that went to the exact chain).
    A chain table that breaks the header's rules raises."""
    torch = _lib.require_gpu()
    cs = _int_desc(chain_start, np.int64, "chain_start", db.device, "md_chain_scan", reshape=True)
    qc = _int_desc(qchain, np.int32, "qchain", db.device, "md_chain_scan", cols=2, reshape=True)
    nqc = qc.shape[0]
    count = torch.zeros(1, dtype=torch.int64, device=db.device)
    status = torch.zeros(max(nqc, 1), dtype=torch.int32, device=db.device)[:nqc]
    taken = md_scan_route(route, q.shape[0], row_norm_bound)
    st = torch.zeros(1, dtype=torch.int64, device=db.device) if taken == "matrix" else None
    kw = dict(lengths=lengths, qlen=qlen, mincov=mincov, route=taken, row_norm_bound=row_norm_bound, out_stats=st, workspace=None)

    def launch(pairs, slots):
        kw["workspace"] = md_chain_scan_launch(db, cs, q, mode, qc, min_score, pairs, count, status, cap=slots, **kw)     # (kept for a second launch)
        return int(count.item())

    pairs, _cap, found = _capped_relaunch(launch, lambda slots: torch.empty((max(slots, 1), 2), dtype=torch.int64, device=db.device), cap)
    if stats is not None:
        stats["route"] = taken
        if st is not None:
            stats["rescored"] = int(st.item())
    if found < 0:
        raise MerizoHipError("md_chain_scan: chain_start must rise strictly from 0 to the number of rows")
    out = pairs[:found].cpu().numpy()
    return out[np.lexsort((out[:, 1], out[:, 0]))], status.cpu().numpy()


class EgnnEncoder:
    """The Foldclass structure encoder on one GPU: prepared weights + positional table.

    ``embed(list of [N,3] arrays)`` -> float32 [B,128] tensor on the device.  Replaces
    ``network(x)`` of the reference (dbsearch.py:97-98, :299-301; makedb.py:75-79) for a whole
    ragged batch per launch.

    Streams: an encoder owns ONE device staging buffer and ONE workspace, which the kernels of a call read and write until the
    last of them has finished.  ``embed`` runs on torch's current stream, records an event behind its last launch, and the next
    call makes ITS stream wait on that event before the staging copy and before it reuses the workspace: calls on different
    streams are correct and run one after the other.  For embeddings that overlap on the device take one encoder per stream; one
    encoder serves one host thread at a time.
    """

    def __init__(self, weights: np.ndarray, pe: np.ndarray, device="cuda:0"):
        torch = _lib.require_gpu()
        lib = _lib.load()
        self.device = torch.device(device)
        nfl = int(lib.ms_egnn_weight_floats())
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if weights.size != nfl:
            raise MerizoHipError(f"encoder weights: expected {nfl} floats, got {weights.size}")
        pe = np.ascontiguousarray(pe, dtype=np.float32).reshape(-1, DIM)
        with torch.cuda.device(self.device):
            w_dev = torch.from_numpy(weights).to(self.device)
            self.pe = torch.from_numpy(pe).to(self.device)
            self.prepared = torch.empty(int(lib.ms_egnn_prepared_bytes()), dtype=torch.uint8, device=self.device)
            check(lib.ms_egnn_prepare_weights(ptr(w_dev), ptr(self.prepared),
                                              torch.cuda.current_stream(self.device).cuda_stream), "ms_egnn_prepare_weights")
            torch.cuda.current_stream(self.device).synchronize()
        self.max_len = pe.shape[0]
        self._ws = None
        self._last = None          # (nb, total, sum_sq) of the last embed: where its node features lie in the workspace
        self._stage = self._stage_dev = self._stage_free = None
        self._done = None          # event behind the last launch of the last embed: staging buffer and workspace are free from there on

    def embed(self, coords_list: Sequence[np.ndarray]):
        torch = _lib.require_gpu()
        lib = _lib.load()
        nb = len(coords_list)
        if nb == 0:
            return torch.empty((0, DIM), dtype=torch.float32, device=self.device)
        lens = np.array([int(np.asarray(c).shape[0]) for c in coords_list], dtype=np.int64)
        if lens.min() < 1:
            raise MerizoHipError("embed: empty structure")
        if lens.max() > self.max_len:
            raise MerizoHipError(f"embed: structure of {int(lens.max())} residues exceeds the positional table "
                                 f"({self.max_len}); the reference fails here too (nndef_fold_egnn_embed.py:12)")
        total = int(lens.sum())
        # offsets and coordinates go to the device in ONE asynchronous copy out of a pinned staging buffer (two pageable
        # copies cost a query of a few domains ~50 us of host time): [int32 offsets (nb + 1) | pad | float32 coords (total x 3)]
        head = ((nb + 1) * 4 + 15) // 16 * 16
        nbytes = head + total * 12
        with torch.cuda.device(self.device):
            if self._stage is None or self._stage.numel() < nbytes:
                cap = max(nbytes, 1 << 16) * 2
                self._stage = torch.empty(cap, dtype=torch.uint8).pin_memory()
                self._stage_dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
                self._stage_free = None
            if self._stage_free is not None:
                self._stage_free.synchronize()            # the previous call's copy has left the staging buffer
            host = self._stage.numpy()
            offsets = host[: (nb + 1) * 4].view(np.int32)
            offsets[0] = 0
            offsets[1:] = np.cumsum(lens)
            flat = host[head: nbytes].view(np.float32).reshape(total, 3)
            pos = 0
            for c, n in zip(coords_list, lens):
                flat[pos: pos + int(n)] = np.asarray(c, dtype=np.float32).reshape(-1, 3)
                pos += int(n)
            stream = torch.cuda.current_stream(self.device)
            if self._done is not None:
                stream.wait_event(self._done)             # the previous call's kernels, on whatever stream, have left staging buffer and workspace
            self._stage_dev[:nbytes].copy_(self._stage[:nbytes], non_blocking=True)
            self._stage_free = stream.record_event()
            offs_ptr = self._stage_dev.data_ptr()
            coords_ptr = offs_ptr + head
            sum_sq = int((lens * lens).sum())
            need = int(lib.ms_egnn_workspace_bytes(nb, total, sum_sq))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            out = torch.empty((nb, DIM), dtype=torch.float32, device=self.device)
            # (`offsets` in the pinned buffer is only read by the host during the call itself)
            check(lib.ms_egnn_embed(ptr(self.prepared), ptr(self.pe), self.max_len, coords_ptr, offs_ptr,
                                    offsets.ctypes.data, nb, ptr(out), ptr(self._ws), self._ws.numel(), stream.cuda_stream),
                  "ms_egnn_embed")
            self._done = stream.record_event()
            self._last = (nb, total, sum_sq)
        return out

    def node_features(self, layer: int) -> np.ndarray:
        """Diagnostics (tests): the per-residue features float32 [total,128] after EGNN layer ``layer`` (0 or 1) of the LAST
        ``embed`` call, structures concatenated in batch order.  Valid only directly after that call: the next one reuses the
        workspace.  Synchronises the device."""
        if self._last is None:
            raise MerizoHipError("node_features: no embed call on this encoder yet")
        nb, total, sum_sq = self._last
        out = np.empty((total, DIM), dtype=np.float32)
        check(_lib.load().ms_debug_egnn_node_features(ptr(self._ws), nb, total, sum_sq, int(layer), out.ctypes.data),
              "ms_debug_egnn_node_features")
        return out


_tm_ws = {}          # device -> the scratch of ms_tmalign_batch there, grown on demand and kept across calls


def tmalign_batch(coords_list: Sequence[np.ndarray], seqs: Sequence[bytes], pairs, fast: bool = False, device="cuda",
                  want_invmap: bool = False) -> dict:
    """TM-align every pair (s1, s2) of `pairs` -- chain 1 = coords_list[s1] (the query), chain 2 = coords_list[s2] -- in ONE
    launch of ms_tmalign_batch.  Coordinates are used as given, in fp64 (callers that stand in for the TM-align binary pass
    the values of its %8.3f PDB text).  Returns numpy arrays indexed like `pairs`: qtm (TM-score normalised by chain 1),
    ttm (by chain 2), rmsd, n_ali8, n_identical, status (_lib.TM_*), and invmap ([npairs, max chain-2 length], -1 = gap)
    if asked.  A structure longer than _lib.TMALIGN_MAX_LEN or with a non-finite coordinate raises; pairs with a chain of
    <= 5 residues get TM_ERR_SHORT.  Runs on torch's current stream and returns when the results are on the host.  The scratch is
    shared per device (_tm_ws): calls from one host thread follow each other whatever their streams; two host threads must not
    call it for one device at the same time."""
    for s, c in enumerate(coords_list):                  # checked before the device: NaN / inf never reach the kernel
        if not np.isfinite(np.asarray(c, dtype=np.float64)).all():
            raise MerizoHipError(f"tmalign_batch: structure {s} has a non-finite coordinate")
    torch = _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise MerizoHipError("tmalign_batch runs on a HIP device only")
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ns, npairs = len(coords_list), pairs.shape[0]
    out = {"qtm": np.zeros(npairs), "ttm": np.zeros(npairs), "rmsd": np.zeros(npairs), "n_ali8": np.zeros(npairs, np.int32),
           "n_identical": np.zeros(npairs, np.int32), "status": np.zeros(npairs, np.int32)}
    if npairs == 0:
        if want_invmap:
            out["invmap"] = np.zeros((0, 0), np.int32)
        return out
    if len(seqs) != ns:
        raise MerizoHipError("tmalign_batch: one sequence per structure")
    if pairs.min() < 0 or pairs.max() >= ns:
        raise MerizoHipError("tmalign_batch: pair index outside the structure list")
    lens = np.array([int(np.asarray(c).reshape(-1, 3).shape[0]) for c in coords_list], dtype=np.int64)
    for c, s, n in zip(coords_list, seqs, lens):
        if len(s) != n:
            raise MerizoHipError("tmalign_batch: a sequence differs in length from its coordinates")
    used = np.unique(pairs)
    if lens[used].max() > _lib.TMALIGN_MAX_LEN:
        raise MerizoHipError(f"tmalign_batch: a structure of {int(lens[used].max())} residues exceeds the aligner's limit of "
                             f"{_lib.TMALIGN_MAX_LEN}")
    offsets = np.zeros(ns + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    xyz = np.zeros((max(int(offsets[-1]), 1), 3), np.float64)
    seq = np.zeros(max(int(offsets[-1]), 1), np.uint8)
    for s in range(ns):
        if lens[s]:
            xyz[offsets[s]:offsets[s + 1]] = np.asarray(coords_list[s], dtype=np.float64).reshape(-1, 3)
            b = seqs[s].encode() if isinstance(seqs[s], str) else bytes(seqs[s])
            seq[offsets[s]:offsets[s + 1]] = np.frombuffer(b, dtype=np.uint8)
    # one wave per pair, longest first (L1 * L2); the outputs are put back in the caller's order
    work = lens[pairs[:, 0]] * lens[pairs[:, 1]]
    order = np.argsort(-work, kind="stable")
    sp = np.ascontiguousarray(pairs[order], dtype=np.int32)
    max1 = max(int(lens[sp[:, 0]].max()), 1)
    max2 = max(int(lens[sp[:, 1]].max()), 1)
    need = _workspace_bytes("ms_tmalign_workspace_bytes", max1, max2, npairs)
    with torch.cuda.device(dev):
        d_xyz = torch.from_numpy(xyz).to(dev)
        d_seq = torch.from_numpy(seq).to(dev)
        d_off = torch.from_numpy(offsets).to(dev)
        d_pairs = torch.from_numpy(sp).to(dev)
        ws = _tm_ws.get(dev)
        if ws is None or ws.numel() < need:
            ws = _tm_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
        of = torch.empty((npairs, 3), dtype=torch.float64, device=dev)
        oi = torch.empty((npairs, 3), dtype=torch.int32, device=dev)
        inv = torch.full((npairs, max2), -1, dtype=torch.int32, device=dev) if want_invmap else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib.ms_tmalign_batch(ptr(d_xyz), ptr(d_seq), ptr(d_off), ns, ptr(d_pairs), npairs, max1, max2,
                                   _lib.TM_FAST if fast else 0, ptr(ws), ws.numel(), ptr(of), ptr(oi), ptr(inv), stream),
              "ms_tmalign_batch")
        f, i = of.cpu().numpy(), oi.cpu().numpy()
        inv_h = inv.cpu().numpy() if want_invmap else None
    for name, col in (("qtm", f[:, 0]), ("ttm", f[:, 1]), ("rmsd", f[:, 2]), ("n_ali8", i[:, 0]), ("n_identical", i[:, 1]),
                      ("status", i[:, 2])):
        out[name][order] = col
    if want_invmap:
        out["invmap"] = np.empty_like(inv_h)
        out["invmap"][order] = inv_h
    return out
