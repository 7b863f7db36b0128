"""The two routes of the chain scan next to each other: ms_md_chain_scan (one lane per row) and
ms_md_chain_scan_mq (the fp16 matrix pipe in front of the exact cell).

    python tools/chain_search_bench.py [--rows 1000000] [--nq 16 64 256 1024 4096] [--reps 20]
    python tools/chain_search_bench.py --end_to_end 200000 [--tmp DIR]

Per nq and per shape one JSON line: HIP-event time of ONE call of each route (all its launches) over a resident fp32 matrix of unit
rows in chain runs of 1-5 rows at --mincos 0.5, both routes in the same process, each the median of --reps calls after 5 warm-up
calls; `rescored` of the matrix route as a fraction of all (query, row) cells; the ratio lane / matrix.  The query rows are in query
chains of 1-5 domains.  Shapes: "random" = random queries (no row matches); "self" = the first nq rows of the database (every query
has at least one match).  The two routes must report the same number of pairs.
Last lines: the smallest nq of the sweep from which the matrix route wins on both shapes (ops.MD_SCAN_MATRIX_MIN_NQ).
--end_to_end ROWS: one `chain-search` of a synthetic faiss-layout database of ROWS rows against itself (the shape of DESIGN.md 5.9):
wall time of the command and the device time of its scan calls."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BOUND = 1.0 + 1e-6


def _median_ms(call, reps):
    import torch
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def _runs(total, rng):
    """Runs of 1-5 that add up to total -> starts [nruns + 1]."""
    runs = rng.integers(1, 6, size=total)
    starts = np.concatenate([[0], np.cumsum(runs)])
    return np.concatenate([starts[starts < total], [total]]).astype(np.int64)


def sweep(rows, nqs, reps):
    import torch
    from merizo_search_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    db = ops.l2_normalize_rows_(torch.randn((rows, 128), device=dev, generator=g), 1e-8)
    table = torch.from_numpy(_runs(rows, np.random.default_rng(3))).to(dev)
    wins = {}
    for nq in nqs:
        qs = _runs(nq, np.random.default_rng(5))
        qchain = torch.from_numpy(np.stack([qs[:-1], np.diff(qs)], axis=1).astype(np.int32)).to(dev)
        for shape in ("random", "self"):
            q = torch.randn((nq, 128), device=dev, generator=g) if shape == "random" else db[:nq].clone()
            out = {}
            for route in ("lane", "matrix"):
                pairs = torch.empty((1 << 16, 2), dtype=torch.int64, device=dev)
                count = torch.zeros(1, dtype=torch.int64, device=dev)
                stats = torch.zeros(1, dtype=torch.int64, device=dev)
                status = torch.zeros(qchain.shape[0], dtype=torch.int32, device=dev)
                kw = dict(route="matrix", row_norm_bound=BOUND, out_stats=stats) if route == "matrix" else {}
                ws = ops.md_chain_scan_launch(db, table, q, _lib.MODE_IP_NORMQ, qchain, 0.5, pairs, count, status, **kw)
                call = lambda: ops.md_chain_scan_launch(db, table, q, _lib.MODE_IP_NORMQ, qchain, 0.5, pairs, count, status, workspace=ws, **kw)
                out[route] = (_median_ms(call, reps), int(count.item()), int(stats.item()))
            (t_lane, n_lane, _), (t_mat, n_mat, resc) = out["lane"], out["matrix"]
            assert n_lane == n_mat, (n_lane, n_mat)
            wins[(nq, shape)] = t_mat < t_lane
            print(json.dumps({"rows": rows, "nq": nq, "query_chains": int(qchain.shape[0]), "shape": shape, "lane_ms": round(t_lane, 4),
                              "matrix_ms": round(t_mat, 4), "lane_over_matrix": round(t_lane / t_mat, 2), "pairs": n_mat,
                              "rescored": resc, "rescored_fraction": resc / float(nq * rows)}), flush=True)
    best = None
    for nq in sorted(nqs, reverse=True):
        if not (wins[(nq, "random")] and wins[(nq, "self")]):
            break
        best = nq
    print(json.dumps({"matrix_wins_on_both_shapes_from_nq": best}), flush=True)


def end_to_end(rows, tmp):
    import torch
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import chainsearch, dbutil
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import dbsearch_bench
    db = os.path.join(tmp, "synth")
    dbsearch_bench.write_database(db, rows, seed=1)
    # its names again, as chains of 1-5 adjacent domains ('c000000012_TED03')
    starts = _runs(rows, np.random.default_rng(3))
    names = ["c%09d_TED%02d" % (c, d + 1) for c, n in enumerate(np.diff(starts).tolist()) for d in range(n)]
    info = dbutil.read_dbinfo(db + ".json")
    np.char.add(np.char.ljust(np.asarray(names), dbutil.NAME_WIDTH), "\n").astype("S%d" % dbutil.NAME_RECORD).tofile(
        os.path.join(tmp, info["db_names_f"]))
    device_ms = []
    launch = ops.md_chain_scan_launch

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = launch(*a, **kw)
        e1.record()
        device_ms.append((e0, e1))
        return out

    ops.md_chain_scan_launch = timed
    try:
        t0 = time.perf_counter()
        chainsearch.run_chain_search(db, db, os.path.join(tmp, "out"), tmp, "cuda")
        wall = time.perf_counter() - t0
    finally:
        ops.md_chain_scan_launch = launch
    torch.cuda.synchronize()
    out = os.path.join(tmp, "out_search_multi_dom.tsv")
    print(json.dumps({"end_to_end_rows": rows, "wall_s": round(wall, 2), "scan_calls": len(device_ms),
                      "scan_device_ms": round(sum(a.elapsed_time(b) for a, b in device_ms), 2),
                      "lines": sum(1 for _ in open(out)) if os.path.exists(out) else 0}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, nargs="*", default=[16, 64, 256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--end_to_end", type=int, default=0)
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    if args.end_to_end > 0:
        with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
            end_to_end(args.end_to_end, tmp)
    else:
        sweep(args.rows, args.nq, args.reps)


if __name__ == "__main__":
    main()
