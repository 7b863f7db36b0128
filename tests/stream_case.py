"""The case table of tests/test_streams_gpu.py (TEST INFRASTRUCTURE): one case per entry point of include/merizo_search_amd.h that
takes a stream, and per plan form of the searches.

A case builds two input sets A and B of the same shapes that differ ONLY in floating-point payload (rows, queries, scores,
coordinates): every integer input is identical in both, so that any element-wise mix of A and B is a valid input and no address is
ever formed from stale data.  The test primes the case's buffers, workspace and outputs with A on the default stream, then runs the op
on a side stream behind a delay, with B copied into the input buffers on that stream in front of it and A copied back behind it.  A
launch that escaped to another stream, or drifted behind the side stream, read A (or the primed state) and shows in the bits.

A case is a `Case`; `Case.build()` (GPU only; everything it imports from the product is imported there) returns a namespace with
    A, B       lists of device tensors, the payload of the two sets (B uploaded before anything is enqueued)
    fresh()    -> a new state: workspace and out= tensors, whatever run() writes into
    run(bufs, state, side)   the call(s) on torch's CURRENT stream -> tuple of output tensors (or numpy arrays for the wrappers that
               read back).  bufs: the input buffers (holding A or B); side: "A" / "B" for the wrappers that take host data
    canon(outs)   optional: outputs -> list of numpy arrays to compare bit for bit (default: each as it is); for outputs whose order
               the header leaves unspecified
    check(want, torch)   optional: the default-stream result on B against the suite's independent statement of the operation
    same       {output index: reason} for the outputs that are a function of the integer inputs alone and so equal in A and B
This module imports without a GPU: the CPU test tests/test_streams_table.py keeps TABLE complete."""
import functools
import os
import re
import types

import numpy as np

BOUND = 1.0 + 1e-6                     # the row-norm bound of unit rows
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "merizo_search_amd.h")


def streamed_entry_points():
    """The functions include/merizo_search_amd.h declares with a trailing `ms_stream_t stream` parameter."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\b(ms_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
                  if re.search(r"ms_stream_t\s+\w+\s*$", m.group(2).strip()))


class Case:
    """asynchronous: the call must return while the delay in front of it is still running (`gate.query()` is False).  A case that is
    not names in `sync_why` the line of the header or docstring that says the call reads back."""

    def __init__(self, cid, entries, build, asynchronous=True, sync_why=""):
        self.id, self.entries, self.build, self.asynchronous, self.sync_why = cid, tuple(entries), build, asynchronous, sync_why


def _ns(**kw):
    kw.setdefault("canon", None)
    kw.setdefault("check", None)
    kw.setdefault("same", {})
    return types.SimpleNamespace(**kw)


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def _u8(nbytes):
    import torch
    return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")      # (zeroed: bytes a call leaves alone compare equal)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=4)
def _unit_rows(n, seed):
    from merizo_search_amd.foldclass import synthetic as syn
    a = syn.normalized_database(n, seed)
    a.setflags(write=False)
    return a


def _rolled(a):
    """The other database of a search case: the same rows 17 places on (every index of every list changes)."""
    return np.ascontiguousarray(np.roll(a, 17, axis=0))


def _oracle_check(db, q, k, row_offset, rows=slice(None)):
    def check(want, torch):
        from oracle import oracle as orc
        s_ref, i_ref = orc.ip_topk(db, q, k, row_offset=row_offset, order=1)
        s, i = want[0][rows], want[1][rows]
        assert np.array_equal(i, i_ref[rows]) and _bits_equal(s.view(np.uint32), s_ref[rows].view(np.uint32)), "default-stream result != the oracle"
    return check


# ------------------------------------------------------------------ rows ----
def _normalize(which):
    def build():
        import torch
        from merizo_search_amd import ops
        rng = np.random.default_rng(3)
        a = (rng.standard_normal((1003, 128)) * rng.uniform(0.1, 9.0, (1003, 1))).astype(np.float32)
        b = (rng.standard_normal((1003, 128)) * rng.uniform(0.1, 9.0, (1003, 1))).astype(np.float32)

        def run(bufs, st, side):
            if which == "inplace":           # (the input buffer is the output: a copy on the same stream, before A comes back)
                return (ops.l2_normalize_rows_(bufs[0], 1e-12).clone(),)
            if which == "to":
                return (ops.l2_normalize_rows(bufs[0], 1e-12, out=st),)
            return (ops.row_inv_norms(bufs[0], 1e-8),)

        def check(want, torch):
            from oracle import oracle as orc
            if which == "inv":
                ref = 1.0 / np.maximum(np.linalg.norm(b.astype(np.float64), axis=1), 1e-8)
                np.testing.assert_allclose(want[0], ref, rtol=1e-6)
            else:
                np.testing.assert_allclose(want[0], orc.l2_normalize_rows(b, 1e-12), rtol=1e-5, atol=1e-7)

        return _ns(A=[_t(a)], B=[_t(b)], fresh=lambda: torch.empty((1003, 128), dtype=torch.float32, device="cuda"), run=run, check=check)
    return build


# ------------------------------------------------------------------ ms_ip_topk ----
def _ip_topk(n, nq, k, mode="prenorm", staged=False, seed=700):
    def build():
        import torch
        from merizo_search_amd import _lib, ops
        from merizo_search_amd.foldclass import synthetic as syn
        code = {"prenorm": ops.MODE_IP_PRENORM, "normq": ops.MODE_IP_NORMQ, "raw": ops.MODE_COSINE_RAW, "unit": ops.MODE_COSINE_UNIT}[mode]
        kw, off = dict(mode=code), 11
        if mode in ("raw", "unit"):
            raw_a, lengths = syn.raw_database(n, seed)
            raw_b = _rolled(raw_a)
            (qa, qlen), (qb, _) = syn.raw_queries(nq, seed + 1), syn.raw_queries(nq, seed + 2)
            kw.update(lengths=_t(lengths), qlen=_t(qlen), mincov=0.7)
            da, db_ = _t(raw_a), _t(raw_b)
            if mode == "unit":
                ops.l2_normalize_rows_(da, 1e-8)
                ops.l2_normalize_rows_(db_, 1e-8)
        else:
            rows_a = _unit_rows(n, seed)
            rows_b = _rolled(rows_a)
            if mode == "normq":
                qa, qb = syn.raw_queries(nq, seed + 1)[0], syn.raw_queries(nq, seed + 2)[0]
            else:
                qa, qb = syn.normalized_database(nq, seed + 1), syn.normalized_database(nq, seed + 2)
            da, db_ = _t(rows_a), _t(rows_b)
        need = int(_lib.load().ms_ip_topk_workspace_bytes(n, nq, k))

        def fresh():
            return dict(ws=_u8(need), out=(torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda")))

        def run(bufs, st, side):
            d, q = bufs
            if staged:
                ops.ip_topk_prepare(d, q, k, st["ws"], **kw)
                ops.ip_topk_scan(d, q, k, st["ws"], **kw)
                ops.ip_topk_finish(n, nq, k, st["ws"], st["out"][0], st["out"][1], row_offset=off)
                return st["out"]
            return ops.ip_topk(d, q, k, row_offset=off, workspace=st["ws"], out=st["out"], **kw)

        if mode in ("raw", "unit"):
            def check(want, torch):
                from conftest import assert_topk_equivalent
                from oracle import oracle as orc
                s_ref, i_ref = orc.cosine_topk(raw_b, qb, k, lengths, qlen, 0.7, row_offset=off)
                assert_topk_equivalent(want[0], want[1], s_ref, i_ref, tol=2e-6)
        elif mode == "normq":
            def check(want, torch):
                qn = ops.l2_normalize_rows(_t(qb), 1e-12).cpu().numpy()          # (the library's own F.normalize, as the existing files do)
                _oracle_check(rows_b, qn, k, off)(want, torch)
        else:
            check = _oracle_check(rows_b, qb, k, off)
        return _ns(A=[da, _t(qa)], B=[db_, _t(qb)], fresh=fresh, run=run, check=check)
    return build


def _ip_topk_large(raw, with_lb=False):
    """(3,000, 37, 200).  B's query 0 is NaN, so that out_status differs between the sets (status 2: not served)."""
    n, nq, k, off = 3000, 37, 200, 1000

    def build():
        import torch
        from merizo_search_amd import _lib, ops
        from merizo_search_amd._lib import ptr
        lib = _lib.load()
        rows_a = _unit_rows(n, 9)
        rows_b = _rolled(rows_a)
        qa, qb = np.array(_unit_rows(nq, 10)), np.array(_unit_rows(nq, 12))
        if raw:
            qb[0] = np.nan
        A, B = [_t(rows_a), _t(qa)], [_t(rows_b), _t(qb)]
        if with_lb:                           # the k-th best itself: valid and tight; with the other set's rows it is too high, never invalid
            for S in (A, B):
                S.append(ops.ip_topk(S[0], S[1], k)[0][:, k - 1].contiguous())
        need = int(lib.ms_ip_topk_large_workspace_bytes(n, nq, k))

        def fresh():
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
            return dict(ws=_u8(need), out=(e((nq, k), torch.float32), e((nq, k), torch.int64), e((nq,), torch.int32), e((nq,), torch.float32),
                                           e((4,), torch.int64)))

        def run(bufs, st, side):
            if not raw:
                return ops.ip_topk_large(bufs[0], bufs[1], k, BOUND, row_offset=off, workspace=st["ws"], out=st["out"][:2])
            s, i, status, lb, stats = st["out"]
            rc = lib.ms_ip_topk_large(ptr(bufs[0]), n, off, ptr(bufs[1]), nq, k, 0, 0, 0, 0.0, BOUND, ptr(bufs[2]) if with_lb else 0, ptr(s), ptr(i),
                                      ptr(status), ptr(lb), ptr(stats), ptr(st["ws"]), st["ws"].numel(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.ms_last_error()
            return st["out"]

        def check(want, torch):
            _oracle_check(rows_b, qb, k, off, rows=slice(1, None) if raw else slice(None))(want, torch)
            if raw:
                assert want[2][0] == 2 and (want[2][1:] == 0).all() and (want[1][0] == -1).all()

        return _ns(A=A, B=B, fresh=fresh, run=run, check=check)
    return build


# ------------------------------------------------------------------ the prefiltered search ----
def _formats(ops):
    return {"bf16x3": ops.PF_BF16X3, "f16x2": ops.PF_F16X2, "f16x1": ops.PF_F16X1}


def _pf_image(fmt):
    n = 70_000

    def build():
        from merizo_search_amd import _lib, ops
        code = _formats(ops)[fmt]
        rows_a = _unit_rows(n, 700)
        need = int(_lib.load().ms_pf_image_bytes(n, code))
        return _ns(A=[_t(rows_a)], B=[_t(_rolled(rows_a))], fresh=lambda: _u8(need),
                   run=lambda bufs, st, side: (ops.pf_build_image(bufs[0], fmt=code, row_norm_bound=BOUND, out=st).data,))
    return build


def _near_tie_rows(rows, q, per_query=300, seed=6):
    """tests/test_prefilter_gpu.py's near-tie data at this row count: `per_query` rows within 1e-6 of every query's best score."""
    rng = np.random.default_rng(seed)
    rows = np.array(rows)
    pick = rng.choice(rows.shape[0], size=(q.shape[0], per_query), replace=False)
    for j in range(q.shape[0]):
        v = q[j][None, :] + rng.normal(0, 2e-7, size=(per_query, 128)).astype(np.float32)
        rows[pick[j]] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    rows[pick[0, :50]] = rows[pick[0, 0]]
    return rows


def _prefiltered(fmt, n=70_000, nq=100, k=5, staged=False, near_ties=False, seed=700):
    def build():
        import torch
        from merizo_search_amd import _lib, ops
        from merizo_search_amd.foldclass import synthetic as syn
        code = _formats(ops)[fmt]
        assert ops.prefilter_serves(n, nq, k, code), "the shape must select the prefiltered form"
        rows_a = _unit_rows(n, seed)
        qa, qb = syn.normalized_database(nq, seed + 1), syn.normalized_database(nq, seed + 2)
        rows_b = _near_tie_rows(_rolled(rows_a), qb) if near_ties else _rolled(rows_a)
        da, db_ = _t(rows_a), _t(rows_b)
        img_a, img_b = (ops.pf_build_image(d, fmt=code, row_norm_bound=BOUND).data for d in (da, db_))
        need = int(_lib.load().ms_ip_topk_prefiltered_workspace_bytes(n, nq, k))
        off = 11

        def fresh():
            return dict(ws=_u8(need), out=(torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda")))

        def run(bufs, st, side):
            d, q, img = bufs
            image = ops.PfImage(img, code, n)
            if staged:
                for stage in ("prepare", "scan", "finish"):
                    ops.ip_topk_prefiltered_stage(stage, d, q, k, st["ws"], BOUND, out=st["out"], row_offset=off, image=image)
                return st["out"]
            return ops.ip_topk_prefiltered(d, q, k, BOUND, row_offset=off, workspace=st["ws"], out=st["out"], image=image)

        def check(want, torch):
            _oracle_check(rows_b, qb, k, off)(want, torch)
            if near_ties:                     # every query of B took the gated exact pipeline
                st = fresh()
                run([db_, _t(qb), img_b], st, "B")
                assert ops.prefilter_flagged(st["ws"]) == nq

        return _ns(A=[da, _t(qa), img_a], B=[db_, _t(qb), img_b], fresh=fresh, run=run, check=check)
    return build


def _prefiltered_few():
    """nq = 3 over the fp16 image: the smallest row count ms_pf_few_min_rows() serves."""
    def build():
        from merizo_search_amd import _lib
        n = int(_lib.load().ms_pf_few_min_rows(3))
        return _prefiltered("f16x1", n=n, nq=3, k=10, seed=561)()
    return build


# ------------------------------------------------------------------ merges and the range filter ----
def _sorted_lists(S, nq, k, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(-np.sort(-rng.standard_normal((S, nq, k)).astype(np.float32), axis=2))


def _merge(S, packed=False):
    nq, k = 9, 10

    def build():
        import torch
        from merizo_search_amd import ops
        sa, sb = _sorted_lists(S, nq, k, 20 + S), _sorted_lists(S, nq, k, 90 + S)
        idx = np.stack([np.arange(nq * k, dtype=np.int64).reshape(nq, k) * S + s for s in range(S)])
        idx[S - 1, 0, k - 1] = -1                                              # a padding entry, in both sets
        sa[S - 1, 0, k - 1] = sb[S - 1, 0, k - 1] = -np.inf

        def check(want, torch):
            from oracle import oracle as orc
            s_ref, i_ref = orc.topk_merge(sb, idx)
            assert np.array_equal(want[1], i_ref) and _bits_equal(want[0], s_ref)

        if not packed:
            d_idx = _t(idx)
            return _ns(A=[_t(sa)], B=[_t(sb)], fresh=lambda: None, run=lambda bufs, st, side: ops.topk_merge(bufs[0], d_idx), check=check)
        idx_off = (4 * nq * k + 15) // 16 * 16
        stride = idx_off + 8 * nq * k

        def block(scores):
            g = np.zeros((S, stride), np.uint8)
            for s in range(S):
                g[s, : 4 * nq * k] = scores[s].view(np.uint8).reshape(-1)
                g[s, idx_off:] = idx[s].view(np.uint8).reshape(-1)
            return _t(g.reshape(-1))

        def fresh():
            return (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))

        return _ns(A=[block(sa)], B=[block(sb)], fresh=fresh, check=check,
                   run=lambda bufs, st, side: ops.topk_merge_packed(bufs[0], S, nq, k, idx_off, st[0], st[1]))
    return build


def _drop_ranges():
    nq, kin, kout, cut = 37, 40, 20, 0.25

    def build():
        import torch
        from merizo_search_amd import ops
        rng = np.random.default_rng(8)
        sa, sb = (np.ascontiguousarray(-np.sort(-rng.standard_normal((nq, kin)).astype(np.float32), axis=1)) for _ in range(2))
        idx = rng.permuted(np.tile(np.arange(400, dtype=np.int64), (nq, 1)), axis=1)[:, :kin].copy()
        idx[:, kin - 3:] = -1
        sa[:, kin - 3:] = sb[:, kin - 3:] = -np.inf
        lo = rng.integers(0, 300, nq).astype(np.int64)
        hi = lo + rng.integers(0, 100, nq)
        d_idx, d_lo, d_hi = _t(idx), _t(lo), _t(hi)

        def fresh():
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
            return (e((nq, kout), torch.float32), e((nq, kout), torch.int64), e((nq,), torch.int32))

        def check(want, torch):
            import dbquery_case as dq
            for g, w in zip(want, dq.drop_ranges_np(sb, idx, lo, hi, cut, kout)):
                assert _bits_equal(g, w)

        return _ns(A=[_t(sa)], B=[_t(sb)], fresh=fresh, check=check,
                   run=lambda bufs, st, side: ops.topk_drop_ranges(bufs[0], d_idx, d_lo, d_hi, kout, cut, out=st))
    return build


# ------------------------------------------------------------------ the cluster calls ----
def _cluster_graph_data():
    """n = 1,000, k = 5, m = 300: lists and extras of cluster_case.random_lists / cluster_complete_case.random_extras (every kind of
    entry that is no edge among them); set B has other scores at the same places."""
    import cluster_case as cc
    import cluster_complete_case as ccc
    n, k, m = 1000, 5, 300
    idx, score_a, lengths = cc.random_lists(n, k, seed=2000 * n + k)
    src, dst, esc_a = ccc.random_extras(n, m, idx, score_a, seed=n + 1)
    rng = np.random.default_rng(77)
    score_b = rng.choice(cc.SCORE_VALUES, size=(n, k)).astype(np.float32)
    esc_b = rng.choice(cc.SCORE_VALUES, size=m).astype(np.float32)
    return dict(n=n, k=k, m=m, idx=idx, src=src, dst=dst, lengths=lengths, a=(score_a, esc_a), b=(score_b, esc_b), cut=float(cc.CUT), cov=0.7)


def _cluster(which):
    def build():
        import torch
        import cluster_case as cc
        import cluster_complete_case as ccc
        import cluster_components_case as cpc
        import cluster_tree_case as ctc
        from merizo_search_amd import _lib, ops
        g = _cluster_graph_data()
        n, cut, cov = g["n"], g["cut"], g["cov"]
        d_idx, d_src, d_dst, d_len = _t(g["idx"]), _t(g["src"]), _t(g["dst"]), _t(g["lengths"])
        sizing = {"greedy": "ms_cluster_workspace_bytes", "edges": "ms_cluster_workspace_bytes", "components": "ms_cluster_components_workspace_bytes",
                  "tree": "ms_cluster_tree_workspace_bytes"}[which]
        need = int(getattr(_lib.load(), sizing)(n))
        count_key = {"greedy": "n_reps", "edges": "n_reps", "components": "n_components", "tree": "n_edges"}[which]

        def fresh():
            if which == "tree":
                out = (torch.empty((n, 2), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.float32, device="cuda"))
            else:
                out = (torch.empty((n,), dtype=torch.int64, device="cuda"), torch.empty((n,), dtype=torch.float32, device="cuda"))
            return dict(ws=_u8(need), out=out)

        def run(bufs, st, side):
            score, esc = bufs
            if which == "greedy":
                a, b, info = ops.cluster_greedy(d_idx, score, d_len, cut, cov, out=st["out"], workspace=st["ws"])
            else:
                fn = {"edges": ops.cluster_greedy_edges, "components": ops.cluster_components, "tree": ops.cluster_tree}[which]
                a, b, info = fn(d_idx, score, d_src, d_dst, esc, d_len, cut, cov, out=st["out"], workspace=st["ws"])
            return a, b, np.array([info[count_key], info["saturated"]], np.int64)       # ('rounds' may differ from run to run)

        def canon(outs):
            a, b, counts = (np.asarray(o.cpu() if hasattr(o, "cpu") else o) for o in outs)
            if which == "tree":               # the forest as a sorted set: which slot holds an edge is the kernel's business
                x, y, w = ctc.slots_as_forest(a, b)
                return [np.array(sorted(ctc.forest_set(x, y, w)), np.int64).reshape(-1, 3), counts]
            return [a, b, counts]

        def check(want, torch):
            sb, eb = g["b"]
            if which == "tree":
                x, y, w, info = ctc.cluster_tree_np(g["idx"], sb, g["src"], g["dst"], eb, g["lengths"], cut, cov)
                assert np.array_equal(want[0], np.array(sorted(ctc.forest_set(x, y, w)), np.int64).reshape(-1, 3))
                assert want[1].tolist() == [info["n_edges"], info["saturated"]]
                return
            if which == "greedy":
                rep, score, info = cc.cluster_greedy_np(g["idx"], sb, g["lengths"], cut, cov)
            elif which == "edges":
                rep, score, info = ccc.cluster_greedy_edges_np(g["idx"], sb, g["src"], g["dst"], eb, g["lengths"], cut, cov)
            else:
                rep, score, info = cpc.cluster_components_np(g["idx"], sb, g["src"], g["dst"], eb, g["lengths"], cut, cov)
            assert np.array_equal(want[0], rep) and _bits_equal(want[1], score) and want[2].tolist() == [info[count_key], info["saturated"]]

        return _ns(A=[_t(g["a"][0]), _t(g["a"][1])], B=[_t(g["b"][0]), _t(g["b"][1])], fresh=fresh, run=run, canon=canon, check=check)
    return build


def _cluster_pairs():
    """ms_cluster_pairs -> ms_cluster_pairs_apply -> ms_cluster_pairs_find, three calls in a row.  The slot of a pair is unspecified, so
    the verdicts are computed on the device from the pair itself (keep iff a + b is even) and every output is compared in a form that does
    not depend on the slots: the sorted set, the edited graph, and the PAIR found for every probe.  apply edits the graph in place: the
    integer halves of the graph (identical in A and B) are input buffers too, and are put back with the rest."""
    def build():
        import torch
        import cluster_tm_case as ct
        from merizo_search_amd import _lib, ops
        g = _cluster_graph_data()
        n, k, m, cut, cov = g["n"], g["k"], g["m"], g["cut"], g["cov"]
        cap = n * k + m
        d_src, d_len = _t(g["src"]), _t(g["lengths"])
        rng = np.random.default_rng(5)
        pa, pb = _t(rng.integers(0, n, 2000).astype(np.int64)), _t(rng.integers(0, n, 2000).astype(np.int64))
        need = int(_lib.load().ms_cluster_pairs_workspace_bytes(n, k, m))

        def fresh():
            return dict(ws=_u8(need), out=(torch.empty((cap, 2), dtype=torch.int32, device="cuda"), torch.empty((2,), dtype=torch.int64, device="cuda")))

        def run(bufs, st, side):
            idx, score, dst, esc = bufs
            pairs, count, ws = ops.cluster_pairs(idx, score, d_src, dst, esc, d_len, cut, cov, out=st["out"], workspace=st["ws"])
            keep = ((pairs[:, 0] + pairs[:, 1]) % 2 == 0).to(torch.uint8)
            slot = ops.cluster_pairs_find(pa, pb, d_len, ws)                   # (before apply: the set is what cluster_pairs left)
            found = torch.where((slot >= 0)[:, None], pairs[slot.clamp(min=0)], torch.full_like(pairs[:1], -1))
            removed = ops.cluster_pairs_apply(idx, score, d_src, dst, esc, d_len, cut, cov, keep, ws)
            return pairs.clone(), count.clone(), found, removed, idx.clone(), score.clone(), dst.clone(), esc.clone()

        def canon(outs):
            pairs, count, *rest = (o.cpu().numpy() for o in outs)
            c = int(count[0])
            return [np.array(sorted(map(tuple, pairs[:c].tolist())), np.int32).reshape(-1, 2), count] + rest

        def check(want, torch):
            sb, eb = g["b"]
            ref, sat = ct.cluster_pairs_np(g["idx"], sb, g["src"], g["dst"], eb, g["lengths"], cut, cov)
            assert want[1].tolist() == [ref.shape[0], sat] and {tuple(p) for p in want[0].tolist()} == {tuple(p) for p in ref.tolist()}
            keep = ((ref[:, 0] + ref[:, 1]) % 2 == 0).astype(np.uint8)
            new_idx, new_score, new_dst, new_esc, removed = ct.pairs_apply_np(g["idx"], sb, g["src"], g["dst"], eb, g["lengths"], cut, cov, ref, keep)
            assert int(want[3][0]) == removed > 0
            assert np.array_equal(want[4], new_idx) and _bits_equal(want[5], new_score) and np.array_equal(want[6], new_dst) and _bits_equal(want[7], new_esc)
            slots = ct.pairs_find_np(pa.cpu().numpy(), pb.cpu().numpy(), g["lengths"], ref)
            assert np.array_equal(want[2], np.where((slots >= 0)[:, None], ref[np.maximum(slots, 0)], -1))

        ints = [_t(g["idx"]), _t(g["dst"])]
        return _ns(A=[ints[0], _t(g["a"][0]), ints[1], _t(g["a"][1])], B=[ints[0].clone(), _t(g["b"][0]), ints[1].clone(), _t(g["b"][1])],
                   fresh=fresh, run=run, canon=canon, check=check)
    return build


def _threshold_edges(raw=False):
    def build():
        import torch
        import cluster_complete_case as ccc
        from merizo_search_amd import _lib, ops
        from merizo_search_amd._lib import ptr
        lib = _lib.load()
        n, nq, cut = 1000, 37, 0.5
        rows_a = np.array(_unit_rows(n, 31))
        rows_b = _rolled(rows_a)
        rng = np.random.default_rng(32)

        def queries(rows):                    # noisy copies of rows (cosines on both sides of the cut), raw
            pick, noise = rng.integers(0, n, nq), rng.choice([0.0, 0.3, 0.9, 1.0, 1.1, 3.0], size=(nq, 1))
            return (rows[pick] + noise * rng.standard_normal((nq, 128)) / np.sqrt(128.0)).astype(np.float32)

        qa, qb = queries(rows_a), queries(rows_b)

        cap = n * nq
        need = int(lib.ms_threshold_edges_workspace_bytes(n, nq))

        def fresh():
            if not raw:
                return None
            e = lambda count, dt: torch.zeros((count,), dtype=dt, device="cuda")
            return dict(ws=_u8(need), out=(e(cap, torch.int64), e(cap, torch.int64), e(cap, torch.float32), e(1, torch.int64), e(1, torch.int64)))

        def run(bufs, st, side):
            if raw:
                src, dst, score, count, stats = st["out"]
                rc = lib.ms_threshold_edges(ptr(bufs[0]), n, 5, ptr(bufs[1]), nq, ops.MODE_IP_NORMQ, 0, 0, cut, BOUND, ptr(src), ptr(dst), ptr(score), cap,
                                            ptr(count), ptr(stats), ptr(st["ws"]), st["ws"].numel(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, lib.ms_last_error()
                return st["out"]
            src, dst, score, count = ops.threshold_edges(bufs[0], bufs[1], ops.MODE_IP_NORMQ, cut, BOUND, row_offset=5)
            return src, dst, score, np.array([count], np.int64)

        def canon(outs):
            count = np.asarray(outs[3].cpu() if hasattr(outs[3], "cpu") else outs[3]).reshape(-1)
            src, dst, score = (o.cpu().numpy()[: int(count[0])] for o in outs[:3])
            return [np.array(sorted(ccc.edge_set(src, dst, score)), np.int64).reshape(-1, 3), count] + [o.cpu().numpy() for o in outs[4:]]

        def check(want, torch):
            s, i = ops.ip_topk(_t(rows_b), _t(qb), n, mode=ops.MODE_IP_NORMQ, row_offset=5)
            ref = ccc.edges_of_lists(s.cpu().numpy(), i.cpu().numpy(), cut)
            assert {tuple(e) for e in want[0].tolist()} == ref and int(want[1][0]) == len(ref) > 0

        return _ns(A=[_t(rows_a), _t(qa)], B=[_t(rows_b), _t(qb)], fresh=fresh, run=run, canon=canon, check=check)
    return build


# ------------------------------------------------------------------ multi-domain ----
def _md_layouts():
    """md_scan_case.fixed_layout twice: the same chains and descriptors, other vectors; in B one planted match of query chain 0 is
    overwritten, so that counts and statuses differ too."""
    import md_scan_case as sc
    a, b = sc.fixed_layout(seed=5), sc.fixed_layout(seed=6)
    assert np.array_equal(a["table"], b["table"]) and np.array_equal(a["qchain"], b["qchain"])
    db = np.array(b["db"])
    db[int(b["table"][1])] = sc.unit(np.random.default_rng(1).standard_normal(128))
    b = dict(b, db=db)
    return a, b


def _md_scores_and_mappings():
    def build():
        import torch
        import best_mapping_case as bm
        import md_scan_case as sc
        import multidom_case as mc
        from merizo_search_amd import _lib, ops
        a, b = _md_layouts()
        table, qchain = a["table"], a["qchain"]
        cand, trows, off, at = [], [], [], 0
        for (g, c) in sorted(a["expect"]):                                     # the planted (query chain, target chain) pairs
            q0, nqd = (int(x) for x in qchain[g])
            r0, r1 = int(table[c]), int(table[c + 1])
            cand.append((q0, nqd, len(trows), r1 - r0))
            trows.extend(range(r0, r1))
            off.append(at)
            at += nqd * (r1 - r0)
        cand, trows, off = np.asarray(cand, np.int32), np.asarray(trows, np.int64), np.asarray(off, np.int64)
        ncand, total = len(cand), at
        d_cand, d_trows, d_off = _t(cand), _t(trows), _t(off)
        lib = _lib.load()
        need_s, need_b = int(lib.ms_md_chain_scores_workspace_bytes(a["q"].shape[0])), int(lib.ms_md_best_mappings_workspace_bytes(ncand, total))

        def fresh():
            e = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
            return dict(ws_s=_u8(need_s), ws_b=_u8(need_b), scores=(e((total,), torch.float32), e((ncand, 2), torch.int32)),
                        best=(e((ncand, 2), torch.int32), e((ncand, 2), torch.int64), e((ncand, 2, 64), torch.int32), e((ncand, 2, 64), torch.float32)))

        def run(bufs, st, side):
            scores, match = ops.md_chain_scores(bufs[0], bufs[1], ops.MODE_IP_PRENORM, d_cand, d_trows, d_off, float(sc.MINCOS), out=st["scores"],
                                                workspace=st["ws_s"])
            return (scores, match) + tuple(ops.md_best_mappings(scores, d_cand, d_off, out=st["best"], workspace=st["ws_b"]))

        def check(want, torch):
            s_ref, m_ref = mc.chain_scores_ref(b["db"], b["q"], cand, trows, off, sc.MINCOS, np.zeros(total, np.float32), np.zeros((ncand, 2), np.int32))
            assert _bits_equal(want[0], s_ref) and np.array_equal(want[1], m_ref)
            for got, ref in zip(want[2:], bm.best_mappings(s_ref, cand, off)):
                assert _bits_equal(got, np.asarray(ref, got.dtype))

        return _ns(A=[_t(a["db"]), _t(a["q"])], B=[_t(b["db"]), _t(b["q"])], fresh=fresh, run=run, check=check)
    return build


def _md_scan(route, wrapper=False):
    def build():
        import torch
        import md_scan_case as sc
        from merizo_search_amd import _lib, ops
        a, b = _md_layouts()
        n, nq, cap = a["n"], a["q"].shape[0], 4096
        d_table, d_qchain = _t(a["table"]), _t(a["qchain"])
        nqc = a["qchain"].shape[0]
        sizing = "ms_md_chain_scan_mq_workspace_bytes" if route == "matrix" else "ms_md_chain_scan_workspace_bytes"
        need = int(getattr(_lib.load(), sizing)(n, nq))
        kw = dict(route="matrix", row_norm_bound=BOUND) if route == "matrix" else dict(route="lane")

        def fresh():
            e = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
            return dict(ws=_u8(need), pairs=e((cap, 2), torch.int64), count=e((1,), torch.int64), status=e((nqc,), torch.int32), stats=e((1,), torch.int64))

        def run(bufs, st, side):
            if wrapper:
                pairs, status = ops.md_chain_scan(bufs[0], d_table, bufs[1], ops.MODE_IP_PRENORM, d_qchain, float(sc.MINCOS), cap=cap, **kw)
                return pairs, status
            more = dict(out_stats=st["stats"]) if route == "matrix" else {}
            ops.md_chain_scan_launch(bufs[0], d_table, bufs[1], ops.MODE_IP_PRENORM, d_qchain, float(sc.MINCOS), st["pairs"], st["count"], st["status"],
                                     cap=cap, workspace=st["ws"], **kw, **more)
            return (st["pairs"], st["count"], st["status"]) + ((st["stats"],) if route == "matrix" else ())

        def canon(outs):
            if wrapper:
                return [np.asarray(o) for o in outs]
            pairs, count, status, *stats = (o.cpu().numpy() for o in outs)
            return [np.array(sorted(map(tuple, pairs[: int(count[0])].tolist())), np.int64).reshape(-1, 2), count, status] + stats

        def check(want, torch):
            ref, ref_status = sc.scan_ref(b["db"], b["q"], b["table"], b["qchain"], sc.MINCOS)
            assert [tuple(p) for p in want[0].tolist()] == ref and len(ref) > 0
            assert want[-1 if wrapper else 2].tolist() == ref_status

        status_at = 1 if wrapper else 2
        return _ns(A=[_t(a["db"]), _t(a["q"])], B=[_t(b["db"]), _t(b["q"])], fresh=fresh, run=run, canon=canon, check=check,
                   same={status_at: "out_qstatus is a function of the query chain descriptors alone"})
    return build


# ------------------------------------------------------------------ the encoder ----
EGNN_LENGTHS = (1, 33, 129, 181)


def _egnn_coords(side):
    import egnn_cases
    return [egnn_cases.walk(n, seed=(4100 if side == "A" else 5200) + n) for n in EGNN_LENGTHS]


def _egnn_check(side="B"):
    def check(want, torch):
        from merizo_search_amd.foldclass import weights as W
        from oracle import oracle as orc
        weights, pe = W.pack_state_dict(W.synthetic_state_dict(0))
        ref = orc.egnn_embed(weights, pe, _egnn_coords(side))
        for e, r in zip(want[0], ref):        # tests/test_egnn_gpu.py's ORACLE_REL: two fp32 evaluations of the network
            assert np.abs(e - r).max() <= 2e-6 * np.abs(r).max()
    return check


def _egnn_prepare():
    def build():
        from merizo_search_amd import _lib
        from merizo_search_amd._lib import ptr
        from merizo_search_amd.foldclass import weights as W
        import torch
        lib = _lib.load()
        wa, wb = (np.ascontiguousarray(W.pack_state_dict(W.synthetic_state_dict(seed))[0], np.float32).reshape(-1) for seed in (0, 1))
        nbytes = int(lib.ms_egnn_prepared_bytes())

        def run(bufs, st, side):
            rc = lib.ms_egnn_prepare_weights(ptr(bufs[0]), ptr(st), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.ms_last_error()
            return (st,)

        return _ns(A=[_t(wa)], B=[_t(wb)], fresh=lambda: _u8(nbytes), run=run)
    return build


def _egnn_embed_raw():
    def build():
        import torch
        from merizo_search_amd import _lib, ops
        from merizo_search_amd._lib import ptr
        from merizo_search_amd.foldclass import weights as W
        lib = _lib.load()
        weights, pe = W.pack_state_dict(W.synthetic_state_dict(0))
        enc = ops.EgnnEncoder(weights, pe, "cuda:0")
        lens = np.asarray(EGNN_LENGTHS, np.int64)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        d_off = _t(offsets)
        nb, total, sum_sq = len(lens), int(lens.sum()), int((lens * lens).sum())
        need = int(lib.ms_egnn_workspace_bytes(nb, total, sum_sq))
        flat = lambda side: _t(np.concatenate(_egnn_coords(side)).astype(np.float32).reshape(total, 3))

        def fresh():
            return dict(ws=_u8(need), out=torch.empty((nb, 128), dtype=torch.float32, device="cuda"))

        def run(bufs, st, side):
            rc = lib.ms_egnn_embed(ptr(enc.prepared), ptr(enc.pe), enc.max_len, ptr(bufs[0]), ptr(d_off), offsets.ctypes.data, nb, ptr(st["out"]),
                                   ptr(st["ws"]), st["ws"].numel(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.ms_last_error()
            return (st["out"],)

        return _ns(A=[flat("A")], B=[flat("B")], fresh=fresh, run=run, check=_egnn_check(), keep=enc)
    return build


def _egnn_embed_wrapper():
    def build():
        from merizo_search_amd import ops
        from merizo_search_amd.foldclass import weights as W
        weights, pe = W.pack_state_dict(W.synthetic_state_dict(0))
        coords = {side: _egnn_coords(side) for side in "AB"}
        return _ns(A=[], B=[], fresh=lambda: ops.EgnnEncoder(weights, pe, "cuda:0"), run=lambda bufs, st, side: (st.embed(coords[side]),),
                   check=_egnn_check())
    return build


# ------------------------------------------------------------------ TM-align ----
# One wave aligns one pair, so a call takes as long as its longest pair: measured 1.0 ms per residue of the longer chain with
# MS_TM_FAST and 1.0 .. 1.7 ms without, whatever the number of pairs.  The delay rule (ten times the warm call, at most 1 s) therefore
# calls the upper end of 40 .. 150 residues mis-sized; the cases stay in the part of that range the rule admits.
TM_LENGTHS = (40, 45, 57, 63, 64, 65, 90, 100)
TM_LENGTHS_FULL = (40, 41, 44, 47, 51, 57, 63, 64)


def _tm_structures(side, lengths=TM_LENGTHS):
    """Eight pairs: a walk and a moved, noisy copy of it -- in set B a copy of its first three quarters followed by another walk, so that
    the aligned lengths differ between the sets too.  Same lengths and sequences on both sides, other coordinates."""
    import tm_case
    base = 0 if side == "A" else 1000
    structs = []
    for j, n in enumerate(lengths):
        x = tm_case.walk(n, base + j)
        y = tm_case.noisy(tm_case.rigid(x, base + 50 + j), 1.0, base + 90 + j)
        if side == "B":
            cut = n - n // 4
            y = np.concatenate([y[:cut], y[cut - 1] + tm_case.walk(n - cut, base + 200 + j)])
        structs += [(x, tm_case.seq_of(n, j)), (tm_case.pdb_values(y), tm_case.seq_of(n, 100 + j))]
    return structs


def _tm_check(fast, keys, lengths):
    def check(want, torch):
        import tmalign_ref as R
        structs = _tm_structures("B", lengths)
        for p in range(len(lengths)):
            (x, sx), (y, sy) = structs[2 * p], structs[2 * p + 1]
            ref = R.tm_align(x, y, sx, sy, fast=fast, order="kernel", quantize=False)
            got = keys(want, p)
            assert got["status"] == 0 and got["n_ali8"] == ref["n_ali8"] and got["n_identical"] == ref["n_identical"]
            assert np.array_equal(got["invmap"][: len(y)], ref["invmap"])
            for key in ("qtm", "ttm", "rmsd"):                                 # tests/test_tmalign_gpu.py's bar against the restatement
                assert abs(got[key] - ref[key]) <= 1e-9, (p, key)
    return check


def _tmalign_raw(fast):
    def build():
        import torch
        from merizo_search_amd import _lib
        from merizo_search_amd._lib import ptr
        lib = _lib.load()
        lengths = TM_LENGTHS if fast else TM_LENGTHS_FULL
        sa, sb = _tm_structures("A", lengths), _tm_structures("B", lengths)
        lens = np.array([len(x) for x, _ in sa], np.int64)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        seq = np.frombuffer("".join(s for _, s in sa).encode(), np.uint8).copy()
        npairs, mx = len(lengths), max(lengths)
        pairs = np.array([(2 * p, 2 * p + 1) for p in reversed(range(npairs))], np.int32)      # longest first, as the wrapper sorts them
        d_seq, d_off, d_pairs = _t(seq), _t(offsets), _t(pairs)
        need = int(lib.ms_tmalign_workspace_bytes(mx, mx, npairs))
        xyz = lambda structs: _t(np.concatenate([x for x, _ in structs]).astype(np.float64))

        def fresh():
            return dict(ws=_u8(need), of=torch.zeros((npairs, 3), dtype=torch.float64, device="cuda"), oi=torch.zeros((npairs, 3), dtype=torch.int32, device="cuda"),
                        inv=torch.full((npairs, mx), -1, dtype=torch.int32, device="cuda"))

        def run(bufs, st, side):
            rc = lib.ms_tmalign_batch(ptr(bufs[0]), ptr(d_seq), ptr(d_off), len(sa), ptr(d_pairs), npairs, mx, mx, _lib.TM_FAST if fast else 0, ptr(st["ws"]),
                                      st["ws"].numel(), ptr(st["of"]), ptr(st["oi"]), ptr(st["inv"]), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.ms_last_error()
            return st["of"], st["oi"], st["inv"]

        def keys(want, p):
            r = npairs - 1 - p
            return dict(qtm=want[0][r, 0], ttm=want[0][r, 1], rmsd=want[0][r, 2], n_ali8=want[1][r, 0], n_identical=want[1][r, 1], status=want[1][r, 2],
                        invmap=want[2][r])

        return _ns(A=[xyz(sa)], B=[xyz(sb)], fresh=fresh, run=run, check=_tm_check(fast, keys, lengths))
    return build


def _tmalign_wrapper():
    def build():
        from merizo_search_amd import ops
        structs = {side: _tm_structures(side, TM_LENGTHS_FULL) for side in "AB"}
        pairs = [(2 * p, 2 * p + 1) for p in range(len(TM_LENGTHS_FULL))]
        names = ("qtm", "ttm", "rmsd", "n_ali8", "n_identical", "status", "invmap")

        def run(bufs, st, side):
            got = ops.tmalign_batch([x for x, _ in structs[side]], [s for _, s in structs[side]], pairs, device="cuda:0", want_invmap=True)
            return tuple(got[name] for name in names)

        keys = lambda want, p: {name: want[j][p] for j, name in enumerate(names)}
        return _ns(A=[], B=[], fresh=lambda: None, run=run, check=_tm_check(False, keys, TM_LENGTHS_FULL), same={5: "status 0 for every pair of both sets"})
    return build


# ------------------------------------------------------------------ the table ----
_CLUSTER_SYNC = "include/merizo_search_amd.h: the cluster calls \"return after all work on `stream` has finished\" (the rounds read a word back)"
_CASES = [
    Case("l2_normalize_rows_", ["ms_l2_normalize_rows"], _normalize("inplace")),
    Case("l2_normalize_rows", ["ms_l2_normalize_rows_to"], _normalize("to")),
    Case("row_inv_norms", ["ms_row_inv_norms"], _normalize("inv")),
    Case("ip_topk-few-1q", ["ms_ip_topk"], _ip_topk(5000, 1, 10)),
    Case("ip_topk-few-5q", ["ms_ip_topk"], _ip_topk(5000, 5, 10)),
    Case("ip_topk-ordinary", ["ms_ip_topk"], _ip_topk(70_000, 7, 10)),
    Case("ip_topk-loader-wave", ["ms_ip_topk"], _ip_topk(70_000, 100, 10)),
    Case("ip_topk-multipass", ["ms_ip_topk"], _ip_topk(3000, 70, 100)),
    Case("ip_topk-cosine-raw", ["ms_ip_topk"], _ip_topk(5000, 5, 10, mode="raw")),
    Case("ip_topk-cosine-unit", ["ms_ip_topk"], _ip_topk(70_000, 7, 10, mode="unit")),
    Case("ip_topk-normq", ["ms_ip_topk"], _ip_topk(70_000, 100, 10, mode="normq")),
    Case("ip_topk-staged", ["ms_ip_topk_prepare", "ms_ip_topk_scan", "ms_ip_topk_finish"], _ip_topk(70_000, 100, 10, staged=True)),
    Case("pf_build_image-bf16x3", ["ms_pf_build_image"], _pf_image("bf16x3")),
    Case("pf_build_image-f16x2", ["ms_pf_build_image"], _pf_image("f16x2")),
    Case("pf_build_image-f16x1", ["ms_pf_build_image"], _pf_image("f16x1")),
    Case("prefiltered-bf16x3", ["ms_ip_topk_prefiltered"], _prefiltered("bf16x3")),
    Case("prefiltered-f16x2", ["ms_ip_topk_prefiltered"], _prefiltered("f16x2")),
    Case("prefiltered-f16x1", ["ms_ip_topk_prefiltered"], _prefiltered("f16x1")),
    Case("prefiltered-near-ties", ["ms_ip_topk_prefiltered"], _prefiltered("f16x2", nq=96, k=10, near_ties=True)),
    Case("prefiltered-few-queries", ["ms_ip_topk_prefiltered"], _prefiltered_few()),
    Case("prefiltered-staged", ["ms_ip_topk_prefiltered_prepare", "ms_ip_topk_prefiltered_scan", "ms_ip_topk_prefiltered_finish"],
         _prefiltered("f16x2", staged=True)),
    Case("ms_ip_topk_large", ["ms_ip_topk_large"], _ip_topk_large(raw=True)),
    Case("ms_ip_topk_large-lb_in", ["ms_ip_topk_large"], _ip_topk_large(raw=True, with_lb=True)),
    Case("ip_topk_large", ["ms_ip_topk_large"], _ip_topk_large(raw=False), asynchronous=False,
         sync_why="ops.ip_topk_large: \"Synchronises once per round (it reads the status counts back)\""),
    Case("topk_merge-3", ["ms_topk_merge"], _merge(3)),
    Case("topk_merge-65", ["ms_topk_merge"], _merge(65)),
    Case("topk_merge_packed", ["ms_topk_merge_strided"], _merge(3, packed=True)),
    Case("topk_drop_ranges", ["ms_topk_drop_ranges"], _drop_ranges()),
    Case("cluster_greedy", ["ms_cluster_greedy"], _cluster("greedy"), asynchronous=False, sync_why=_CLUSTER_SYNC),
    Case("cluster_greedy_edges", ["ms_cluster_greedy_edges"], _cluster("edges"), asynchronous=False, sync_why=_CLUSTER_SYNC),
    Case("cluster_components", ["ms_cluster_components"], _cluster("components"), asynchronous=False, sync_why=_CLUSTER_SYNC),
    Case("cluster_tree", ["ms_cluster_tree"], _cluster("tree"), asynchronous=False, sync_why=_CLUSTER_SYNC),
    Case("cluster_pairs-apply-find", ["ms_cluster_pairs", "ms_cluster_pairs_apply", "ms_cluster_pairs_find"], _cluster_pairs()),
    Case("ms_threshold_edges", ["ms_threshold_edges"], _threshold_edges(raw=True)),
    Case("threshold_edges", ["ms_threshold_edges"], _threshold_edges(), asynchronous=False,
         sync_why="ops.threshold_edges: \"Synchronises (it reads the count back)\""),
    Case("md_chain_scores-best_mappings", ["ms_md_chain_scores", "ms_md_best_mappings"], _md_scores_and_mappings()),
    Case("md_chain_scan-lane", ["ms_md_chain_scan"], _md_scan("lane")),
    Case("md_chain_scan-matrix", ["ms_md_chain_scan_mq"], _md_scan("matrix")),
    Case("md_chain_scan-wrapper", ["ms_md_chain_scan"], _md_scan("lane", wrapper=True), asynchronous=False,
         sync_why="ops.md_chain_scan: \"Synchronises (it reads the count back)\""),
    Case("ms_egnn_prepare_weights", ["ms_egnn_prepare_weights"], _egnn_prepare()),
    Case("ms_egnn_embed", ["ms_egnn_embed"], _egnn_embed_raw()),
    Case("EgnnEncoder.embed", ["ms_egnn_embed"], _egnn_embed_wrapper(), asynchronous=False,
         sync_why="ops.EgnnEncoder.embed waits for its staging buffer and takes host arrays: the ordering check only"),
    Case("ms_tmalign_batch", ["ms_tmalign_batch"], _tmalign_raw(fast=False)),
    Case("ms_tmalign_batch-fast", ["ms_tmalign_batch"], _tmalign_raw(fast=True)),
    Case("tmalign_batch", ["ms_tmalign_batch"], _tmalign_wrapper(), asynchronous=False,
         sync_why="ops.tmalign_batch uploads pageable host arrays and copies the results back to numpy"),
]
CASES = {c.id: c for c in _CASES}
# entry point -> the ids of its cases
TABLE = {}
for _c in _CASES:
    for _e in _c.entries:
        TABLE.setdefault(_e, []).append(_c.id)
# entry points that take a stream and have no case, each with its reason
EXCLUDED = {
    "ms_debug_merge_lists": "a test hook, not a product call: one launch_merge, which every search case above makes on its stream",
    "ms_debug_sample_bound": "a test hook, not a product call: one launch_sample_bound, which every sampled search case above makes on its stream",
}
