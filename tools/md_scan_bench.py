"""Cost of the multi-domain mode `database_cosine`.

    python tools/md_scan_bench.py [--rows 1000000 4000000] [--reps 20] [--names 1000000]

Per --rows value and per query set (one chain of 3 domains; 16 domains in 5 chains) one JSON line: HIP-event time of ONE
ms_md_chain_scan call (all its launches: set-up, query preparation, table check, scan, count) over a resident fp32 matrix of
unit rows with synthetic chain runs of 1..5 rows, next to ms_ip_topk (k = 10) of the same queries over the same rows in the
same process -- it reads the same bytes once and is the yardstick -- both as the median of --reps calls after 5 warm-up
calls, with the fraction of the 8 TB/s HBM peak each reaches (rows x 512 bytes / time) and their ratio.
Last line: chain_runs' host time per million names (a CPU loop; no GPU involved)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK = 8.0e12


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


def scan_lines(rows, reps):
    import torch
    from merizo_search_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    db = ops.l2_normalize_rows_(torch.randn((rows, 128), device=dev, generator=g), 1e-8)
    runs = np.random.default_rng(3).integers(1, 6, size=rows)
    starts = np.concatenate([[0], np.cumsum(runs)])
    starts = np.concatenate([starts[starts < rows], [rows]]).astype(np.int64)
    table = torch.from_numpy(starts).to(dev)
    for label, nqds in (("1x3", [3]), ("16_in_5", [3, 3, 3, 3, 4])):
        nq = sum(nqds)
        q = torch.randn((nq, 128), device=dev, generator=g)
        qchain = torch.tensor([(sum(nqds[:i]), d) for i, d in enumerate(nqds)], dtype=torch.int32, device=dev)
        pairs = torch.empty((4096, 2), dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        status = torch.zeros(len(nqds), dtype=torch.int32, device=dev)
        ws = ops.md_chain_scan_launch(db, table, q, _lib.MODE_IP_NORMQ, qchain, 0.5, pairs, count, status)
        scan = lambda: ops.md_chain_scan_launch(db, table, q, _lib.MODE_IP_NORMQ, qchain, 0.5, pairs, count, status, workspace=ws)
        tws = ops.TopKWorkspace(dev)
        topk = lambda: ops.ip_topk(db, q, 10, mode=_lib.MODE_IP_NORMQ, workspace=tws)
        t_scan, t_topk = _median_ms(scan, reps), _median_ms(topk, reps)
        frac = lambda ms: round(rows * 512 / (ms * 1e-3) / HBM_PEAK, 3)
        print(json.dumps({"rows": rows, "chains": int(len(starts) - 1), "queries": label, "md_chain_scan_ms": round(t_scan, 4),
                          "ip_topk_k10_ms": round(t_topk, 4), "scan_hbm_fraction": frac(t_scan), "topk_hbm_fraction": frac(t_topk),
                          "scan_over_topk": round(t_scan / t_topk, 2), "pairs": int(count.item())}), flush=True)
    del db


def chain_runs_line(names):
    from merizo_search_amd.foldclass.multidomain import chain_runs
    runs = np.random.default_rng(3).integers(1, 6, size=names)
    chain = np.repeat(np.arange(names), runs)[:names]
    dom = np.arange(names) - (np.cumsum(runs) - runs)[chain] + 1
    items = ["AF-A0A%07d-F1-model_v4_TED%02d" % (c, d) for c, d in zip(chain.tolist(), dom.tolist())]
    t0 = time.perf_counter()
    starts = chain_runs(items)
    dt = time.perf_counter() - t0
    print(json.dumps({"chain_runs_names": names, "chains": int(len(starts) - 1), "seconds": round(dt, 3),
                      "seconds_per_million": round(dt * 1e6 / names, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 4_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--names", type=int, default=1_000_000)
    args = ap.parse_args()
    for rows in args.rows:
        scan_lines(rows, args.reps)
    if args.names > 0:
        chain_runs_line(args.names)


if __name__ == "__main__":
    main()
