"""Cost of the multi-domain step in mode `exhaustive_cosine`.

    python tools/multidom_bench.py [--rows 200000] [--queries 8192] [--k 10] [--mincos 0.25] [--batch 4096] [--dir DIR] [--no-tmalign]

Prints two JSON lines:
  db_search  a synthetic faiss-layout database whose names form chains of 1..5 domains, searched against itself through the
             product driver (run_dbsearch_db: --multi_domain_search --exclude_same_chain --skip_tmalign), HIP events around
             the scan calls (`scan_ms`; the first call builds the image: `scan_first_ms`) and around the ms_md_chain_scores
             calls (`md_scores_ms`, one per batch), with the candidates, cells and result lines of the run and its wall time
  matrix     the 3 x 200 matrix of DESIGN.md 5.6: ms_md_chain_scores on 3 query domains x 200 target rows (HIP events, mean
             of 200 launches) next to ms_tmalign_batch on tools/tmalign_bench.py's `multi` workload (wall time of a batch)
Unit rows drawn at random have cosines ~ N(0, 1/128): at --mincos 0.25 every query keeps its k hits, so every hit chain with
enough domains becomes a candidate, and hardly any candidate survives the match counts (the host enumerates next to nothing).
Needs an MI355X from the start (dbsearch_bench.write_database generates the rows on the device).  DESIGN.md 5.9.

    python tools/multidom_bench.py --best [--rows 200000] [--queries 8192] [--mincos 0.25] [--batch 4096] [--dir DIR]

prints the lines of `--multi_domain_report best` instead:
  best_kernel   HIP-event time of ms_md_best_mappings (mean of repeated calls after warm-up) on 100,000 candidates of 4 x 8 at half
                density, on one dense 64 x 1024 candidate and on the 64 x 1024 contention matrix (every row wants column 0), each next
                to the time of ms_md_chain_scores for candidates of the same shapes
  chain_search  wall time of run_chain_search with report 'all' and with report 'best' on the synthetic database"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def chain_names(prefix: str, rows: int, seed: int = 3) -> None:
    """Overwrite the names file of dbsearch_bench.write_database's layout with 'c0000012_TED03'-style names: chains of 1..5 rows."""
    from merizo_search_amd.foldclass import dbutil
    runs = np.random.default_rng(seed).integers(1, 6, size=rows)
    chain = np.repeat(np.arange(rows), runs)[:rows]
    dom = np.arange(rows) - (np.cumsum(runs) - runs)[chain] + 1
    names = np.char.add(np.char.add("c", np.char.zfill(chain.astype("U9"), 9)), np.char.add("_TED", np.char.zfill(dom.astype("U2"), 2)))
    names = np.char.ljust(names, dbutil.NAME_WIDTH)
    with open(prefix + ".json") as handle:
        info = json.load(handle)
    np.char.add(names, "\n").astype("S%d" % dbutil.NAME_RECORD).tofile(os.path.join(os.path.dirname(os.path.abspath(prefix)), info["db_names_f"]))


def matrix_line(no_tmalign: bool) -> dict:
    import torch
    from merizo_search_amd import _lib, ops
    g = torch.Generator(device="cuda:0").manual_seed(1)
    db = ops.l2_normalize_rows_(torch.randn((200, 128), device="cuda:0", generator=g), 1e-8)
    q = torch.randn((3, 128), device="cuda:0", generator=g)
    cand, trows, off = np.array([[0, 3, 0, 200]], np.int32), np.arange(200), np.zeros(1, np.int64)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    cand, trows, off = dev(cand, np.int32), dev(trows, np.int64), dev(off, np.int64)
    out = (torch.empty(600, device="cuda:0"), torch.empty((1, 2), dtype=torch.int32, device="cuda:0"))
    ws = torch.empty(int(_lib.load().ms_md_chain_scores_workspace_bytes(3)), dtype=torch.uint8, device="cuda:0")
    call = lambda: ops.md_chain_scores(db, q, _lib.MODE_IP_NORMQ, cand, trows, off, 0.5, out=out, workspace=ws)
    for _ in range(10):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        call()
    b.record()
    torch.cuda.synchronize()
    line = {"workload": "matrix_3x200", "md_chain_scores_us": round(1e3 * a.elapsed_time(b) / 200, 2)}
    if not no_tmalign:
        import tmalign_bench
        structs, seqs, pairs = tmalign_bench.workload("multi")
        ops.tmalign_batch(structs, seqs, pairs, device="cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.tmalign_batch(structs, seqs, pairs, device="cuda:0")
        line["tmalign_hip_s"] = round(time.perf_counter() - t0, 4)
        line["tmalign_over_cosine"] = round(line["tmalign_hip_s"] / (1e-6 * line["md_chain_scores_us"]), 1)
    return line


def _event_us(call, warm: int, reps: int) -> float:
    import torch
    for _ in range(warm):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def best_kernel_lines() -> list:
    """ms_md_best_mappings next to ms_md_chain_scores on candidates of the same shapes (the matrices the best-mapping step is
    timed on are crafted: chain scores of random rows would leave next to nothing above a cut)."""
    import torch
    from merizo_search_amd import _lib, ops
    rng = np.random.default_rng(7)
    g = torch.Generator(device="cuda:0").manual_seed(2)
    db = ops.l2_normalize_rows_(torch.randn((200_000, 128), device="cuda:0", generator=g), 1e-8)
    q = torch.randn((4096, 128), device="cuda:0", generator=g)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    i, j = np.mgrid[0:64, 0:1024]
    small = rng.uniform(0.5, 1.0, (100_000, 4, 8)).astype(np.float32) * (rng.random((100_000, 4, 8)) < 0.5)
    workloads = (("100000 x (4 x 8), half density", small.reshape(-1), 100_000, 4, 8, 20),
                 ("1 x (64 x 1024), dense", rng.uniform(0.5, 1.0, 65536).astype(np.float32), 1, 64, 1024, 50),
                 ("1 x (64 x 1024), contention", (1.0 - (j + 1) / 2048.0 - i / 4096.0).astype(np.float32).reshape(-1), 1, 64, 1024, 50))
    lines = []
    for name, cells, ncand, nqd, nhd, reps in workloads:
        c = np.arange(ncand)
        cand = dev(np.stack([(c % (4096 // nqd)) * nqd, np.full(ncand, nqd), c * nhd, np.full(ncand, nhd)], axis=1), np.int32)
        trows = dev(rng.integers(0, 200_000, ncand * nhd), np.int64)
        off = dev(c * nqd * nhd, np.int64)
        total = ncand * nqd * nhd
        out = (torch.empty(total, device="cuda:0"), torch.empty((ncand, 2), dtype=torch.int32, device="cuda:0"))
        ws = torch.empty(int(_lib.load().ms_md_chain_scores_workspace_bytes(4096)), dtype=torch.uint8, device="cuda:0")
        scores_us = _event_us(lambda: ops.md_chain_scores(db, q, _lib.MODE_IP_NORMQ, cand, trows, off, 0.5, out=out, workspace=ws), 3, reps)
        scores = dev(cells, np.float32)
        res = ops.md_best_mappings(scores, cand, off)
        ws = torch.empty(int(_lib.load().ms_md_best_mappings_workspace_bytes(ncand, total)), dtype=torch.uint8, device="cuda:0")
        best_us = _event_us(lambda: ops.md_best_mappings(scores, cand, off, out=res, workspace=ws), 3, reps)
        status = res[0].cpu().numpy()
        lines.append({"workload": "best_kernel", "candidates": name, "md_best_mappings_us": round(best_us, 2),
                      "md_chain_scores_us": round(scores_us, 2), "best_over_scores": round(best_us / scores_us, 2),
                      "found_any_order": int((status[:, 0] == 1).sum()), "found_ordered": int((status[:, 1] == 1).sum())})
    return lines


def best_workload(args, work: str, prefix: str) -> None:
    from merizo_search_amd.foldclass import chainsearch, dbsearch as ds
    for line in best_kernel_lines():
        print(json.dumps(line), flush=True)
    engine = ds.engine_setup("cuda:0")
    nq = min(args.queries, args.rows)
    out = {"workload": "chain_search", "rows": args.rows, "query_rows": nq, "mincos": args.mincos, "query_batchsize": args.batch}
    for report in ("all", "best", "all", "best"):                      # (the first pair warms the page cache and the kernels up)
        t0 = time.perf_counter()
        chainsearch.run_chain_search(prefix, prefix, os.path.join(work, "out_" + report), os.path.join(work, "tmp"), "cuda:0",
                                     mincos=args.mincos, query_batchsize=args.batch, query_rows="0:%d" % nq, exclude_same_chain=True,
                                     engine=engine, report=report)
        out[report + "_wall_s"] = round(time.perf_counter() - t0, 3)
        out[report + "_lines"] = sum(1 for _ in open(os.path.join(work, "out_" + report + "_search_multi_dom.tsv")))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--mincos", type=float, default=0.25)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dir", type=str, default=None, help="where the database goes (default: a temporary directory, removed)")
    ap.add_argument("--no-tmalign", action="store_true", help="skip the TM-align half of the 3 x 200 comparison")
    ap.add_argument("--best", action="store_true", help="the workloads of --multi_domain_report best instead (DESIGN.md 5.12)")
    args = ap.parse_args()
    import logging
    logging.getLogger().setLevel(logging.WARNING)
    from dbsearch_bench import write_database
    from merizo_search_amd.foldclass import dbsearch as ds, multidomain as md

    work = args.dir or tempfile.mkdtemp(prefix="multidom_bench_")
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, "syn")
    try:
        if not os.path.exists(prefix + ".json"):
            write_database(prefix, args.rows)
            chain_names(prefix, args.rows)
        if args.best:
            best_workload(args, work, prefix)
            return
        shapes = {"cand": 0, "cells": 0}
        engine = ds.engine_setup("cuda:0")
        real = engine.md_chain_scores

        def counted(db, q, mode, cand, trows, mat_off, min_score, **kw):
            shapes["cand"] += int(cand.shape[0])
            shapes["cells"] += int(kw.get("total") or 0)
            return real(db, q, mode, cand, trows, mat_off, min_score, **kw)

        engine.md_chain_scores = counted
        nq = min(args.queries, args.rows)
        times = {}
        t0 = time.perf_counter()
        ds.run_dbsearch_db(prefix, prefix, os.path.join(work, "out"), os.path.join(work, "tmp"), "cuda:0", topk=args.k, mincos=args.mincos,
                           skip_tmalign=True, exclude_same_chain=True, query_batchsize=args.batch, query_rows="0:%d" % nq,
                           format_list="query,emb_rank,target,emb_score".split(","), engine=engine, timings=times, multi_domain_search=True)
        wall = time.perf_counter() - t0
        lines = sum(1 for _ in open(os.path.join(work, "out_search_multi_dom.tsv")))
        calls = times.get("md_scores_calls", 0)
        print(json.dumps({
            "workload": "db_search", "rows": args.rows, "queries": nq, "k": args.k, "mincos": args.mincos, "query_batchsize": args.batch,
            "wall_s": round(wall, 3), "loop_s": round(times["loop_s"], 3), "md_resident": times["md_resident"],
            "scan_calls": times["scan_calls"], "scan_ms": round(times["scan_ms"], 3), "scan_first_ms": round(times["scan_first_ms"], 3),
            "md_scores_calls": calls, "md_scores_ms": round(times.get("md_scores_ms", 0.0), 3),
            "md_scores_first_ms": round(times.get("md_scores_first_ms", 0.0), 3),
            "candidates": shapes["cand"], "cells": shapes["cells"], "multi_dom_lines": lines,
            "pairs_skipped_by_cap": times["md_candidates_skipped"], "max_mapping_paths": md.MAX_MAPPING_PATHS}), flush=True)
        del engine
        print(json.dumps(matrix_line(args.no_tmalign)), flush=True)
    finally:
        if args.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
