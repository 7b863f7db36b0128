"""Cost of the clustering step: a synthetic faiss-layout database clustered through the product driver (cluster.run_cluster,
-k 20), with HIP events around its three device parts.

    python tools/cluster_bench.py [--rows 1000000] [--k 20] [--mincos 0.4] [--mincov 0.7] [--batch 4096] [--dir DIR]

Prints one JSON line:
  scan_ms / scan_ms_per_batch     the scan calls (k' = k + 1; the first call builds the image: `scan_first_ms`, left out of the
                                  per-batch figure when other calls follow)
  graph_write_ms / _us_per_batch  the drop step of every batch, writing rows [b0, b1) of the [n,k] graph tensors in place
  cluster_ms, rounds              ms_cluster_greedy on the finished graph (one call; it synchronises) and its mark / decide rounds
  clusters, singletons, saturated what it found; wall_s, setup_s of the whole run next to them
Unit rows drawn at random have cosines ~ N(0, 1/128): at --mincos 0.4 a row of a 1M-row database has a handful of neighbours.
Needs an MI355X from the start: the rows of the database file are generated on the device (dbsearch_bench.write_database).
Compare `cluster_ms` with `scan_ms` of the same run."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--mincos", type=float, default=0.4)
    ap.add_argument("--mincov", type=float, default=0.7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dir", type=str, default=None, help="where the database goes (default: a temporary directory, removed)")
    args = ap.parse_args()
    import logging
    logging.getLogger().setLevel(logging.WARNING)
    from dbsearch_bench import write_database
    from merizo_search_amd.foldclass import cluster, dbsearch as ds

    work = args.dir or tempfile.mkdtemp(prefix="cluster_bench_")
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, "syn")
    try:
        t0 = time.perf_counter()
        if not os.path.exists(prefix + ".json"):
            write_database(prefix, args.rows)
        print("[cluster_bench] database of %d rows ready in %.1f s" % (args.rows, time.perf_counter() - t0), file=sys.stderr, flush=True)
        engine = ds.engine_setup("cuda:0")
        times = {}
        t0 = time.perf_counter()
        _rep, _score, info = cluster.run_cluster(prefix, os.path.join(work, "out"), os.path.join(work, "tmp"), "cuda:0", topk=args.k,
                                                 mincos=args.mincos, mincov=args.mincov, query_batchsize=args.batch, engine=engine,
                                                 timings=times)
        wall = time.perf_counter() - t0
        calls = times["scan_calls"]
        skip_first = calls > 1
        steady_ms = times["scan_ms"] - (times["scan_first_ms"] if skip_first else 0.0)
        print(json.dumps({
            "rows": args.rows, "k": args.k, "mincos": args.mincos, "mincov": args.mincov, "query_batchsize": args.batch, "batches": calls,
            "in_place": times["in_place"], "wall_s": round(wall, 3),
            "scan_ms": round(times["scan_ms"], 3), "scan_first_ms": round(times["scan_first_ms"], 3),
            "scan_ms_per_batch": round(steady_ms / (calls - 1 if skip_first else calls), 4),
            "graph_write_ms": round(times["drop_ms"], 3), "graph_write_us_per_batch": round(1e3 * times["drop_ms"] / times["drop_calls"], 2),
            "cluster_ms": round(times["cluster_ms"], 3), "rounds": info["rounds"],
            "clusters": info["n_reps"], "singletons": info["singletons"], "saturated": info["saturated"]}), flush=True)
    finally:
        if args.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
