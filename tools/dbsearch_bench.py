"""db-search throughput: a synthetic faiss-layout database searched against itself through the product driver
(dbsearch.run_dbsearch_db: --skip_tmalign --exclude_self -k 10, every hit reported), in query batches of 256 and 4096.

    python tools/dbsearch_bench.py [--rows 1000000] [--queries 32768] [--k 10] [--batches 256,4096] [--mincos -2] [--dir DIR]

Prints one JSON line per batch size:
  queries_per_s_end_to_end   queries / wall time of the batch loop (scan, exchange, drop, record retrieval, TSV append);
                             `setup_s` (opening both databases, the upload, the image) is reported next to it
  queries_per_s_scan         queries / HIP-event time of the scan calls alone (the image is built by the first batch:
                             `scan_first_ms` is that call, excluded from the rate when there is more than one batch)
  drop_us_per_batch          HIP-event time of the driver's drop step per batch (the launch and the allocation of its outputs)
  drop_kernel_us             ms_topk_drop_ranges alone on the batch's shape: 200 back-to-back launches between two HIP events
Needs an MI355X from the start: the rows of the database file are generated on the device (synthetic.device_database).
Compare `queries_per_s_scan` with the `prefiltered` block of `python bench.py --full` on the same box."""
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


def write_database(prefix: str, rows: int, seed: int = 0, residues: int = 8) -> None:
    """A faiss-layout database of `rows` unit rows (synthetic.device_database) with fixed-size name, sequence, coordinate and
    metadata records, written with numpy (dbutil.write_faiss_db loops over the entries in Python)."""
    import torch
    from merizo_search_amd.foldclass import dbutil, synthetic as syn
    base, folder = os.path.basename(prefix), os.path.dirname(os.path.abspath(prefix))
    files = {"dbfname_IP": base + "_raw_128d_norm.db", "db_names_f": base + "_raw_128d.index_names", "sif": base + "_seq.index",
             "sdf": base + "_seq.db", "cif": base + "_ca.index", "cdf": base + "_ca.db", "mif": base + "_metadata.index",
             "mdf": base + "_metadata.db"}
    with open(os.path.join(folder, files["dbfname_IP"]), "wb") as handle:
        for r0 in range(0, rows, 1 << 20):
            n = min(1 << 20, rows - r0)
            handle.write(syn.device_database(n, r0, seed, "cuda:0").cpu().numpy().tobytes())
    torch.cuda.empty_cache()
    names = np.char.ljust(np.char.add("syn", np.char.zfill(np.arange(rows).astype("U9"), 9)), dbutil.NAME_WIDTH)
    np.char.add(names, "\n").astype("S%d" % dbutil.NAME_RECORD).tofile(os.path.join(folder, files["db_names_f"]))
    for ikey, dkey, width, fill in (("sif", "sdf", residues, b"A"), ("cif", "cdf", 12 * residues, b"\0"), ("mif", "mdf", 3, None)):
        start = np.arange(rows, dtype=np.int64) * width
        np.stack([start, start + width], axis=1).tofile(os.path.join(folder, files[ikey]))
        with open(os.path.join(folder, files[dkey]), "wb") as handle:
            handle.write(b"{ }" * rows if fill is None else fill * (width * rows))
    with open(prefix + ".json", "w") as handle:
        json.dump(dict(files, DB_SIZE=rows, DB_DIM=128), handle)


def drop_kernel_us(nq: int, kin: int, kout: int, reps: int = 200) -> float:
    import torch
    from merizo_search_amd import ops
    s = torch.rand((nq, kin), device="cuda:0").sort(dim=1, descending=True).values
    i = torch.randint(0, 1 << 20, (nq, kin), dtype=torch.int64, device="cuda:0")
    lo = torch.arange(nq, dtype=torch.int64, device="cuda:0")
    out = (torch.empty((nq, kout), device="cuda:0"), torch.empty((nq, kout), dtype=torch.int64, device="cuda:0"),
           torch.empty((nq,), dtype=torch.int32, device="cuda:0"))
    for _ in range(10):
        ops.topk_drop_ranges(s, i, lo, lo + 1, kout, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        ops.topk_drop_ranges(s, i, lo, lo + 1, kout, out=out)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=32768, help="rows of the database searched as queries (a slice from row 0)")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=str, default="256,4096")
    ap.add_argument("--mincos", type=float, default=-2.0, help="-2: every hit is retrieved and written")
    ap.add_argument("--dir", type=str, default=None, help="where the database goes (default: a temporary directory, removed)")
    args = ap.parse_args()
    import logging
    logging.getLogger().setLevel(logging.WARNING)
    from merizo_search_amd.foldclass import dbsearch as ds

    work = args.dir or tempfile.mkdtemp(prefix="dbsearch_bench_")
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, "syn")
    try:
        t0 = time.perf_counter()
        if not os.path.exists(prefix + ".json"):
            write_database(prefix, args.rows)
        print("[dbsearch_bench] database of %d rows ready in %.1f s" % (args.rows, time.perf_counter() - t0), file=sys.stderr, flush=True)
        nq = min(args.queries, args.rows)
        for batch in [int(b) for b in args.batches.split(",")]:
            engine = ds.engine_setup("cuda:0")
            times = {}
            t0 = time.perf_counter()
            ds.run_dbsearch_db(prefix, prefix, os.path.join(work, "out_%d" % batch), os.path.join(work, "tmp"), "cuda:0", topk=args.k,
                               mincos=args.mincos, skip_tmalign=True, exclude_self=True, query_batchsize=batch, query_rows="0:%d" % nq,
                               format_list="query,emb_rank,target,emb_score,q_len,t_len,metadata".split(","), engine=engine, timings=times)
            wall = time.perf_counter() - t0
            calls = times["scan_calls"]
            # the first scan call builds the image: left out of the steady rate when other calls follow
            skip_first = calls > 1
            steady_calls = calls - 1 if skip_first else calls
            steady_ms = times["scan_ms"] - (times["scan_first_ms"] if skip_first else 0.0)
            steady_q = nq - (min(batch, nq) if skip_first else 0)
            hits = sum(1 for _ in open(os.path.join(work, "out_%d_search.tsv" % batch)))
            print(json.dumps({
                "rows": args.rows, "queries": nq, "k": args.k, "query_batchsize": batch, "batches": calls, "in_place": times["in_place"], "hits_written": hits,
                "wall_s": round(wall, 3), "setup_s": round(times["setup_s"], 3), "loop_s": round(times["loop_s"], 3),
                "queries_per_s_end_to_end": round(nq / times["loop_s"], 1),
                "queries_per_s_scan": round(steady_q / (steady_ms * 1e-3), 1), "scan_ms_per_batch": round(steady_ms / steady_calls, 4),
                "scan_first_ms": round(times["scan_first_ms"], 3),
                "drop_us_per_batch": round(1e3 * times["drop_ms"] / times["drop_calls"], 2),
                "drop_kernel_us": round(drop_kernel_us(min(batch, nq), args.k + 1, args.k), 2),
                "host_s_outside_scan_and_drop": round(times["loop_s"] - 1e-3 * (times["scan_ms"] + times["drop_ms"]), 3)}), flush=True)
            del engine
    finally:
        if args.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
