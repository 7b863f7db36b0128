"""Cost of the clustering step: a synthetic faiss-layout database clustered through the product driver (cluster.run_cluster,
-k 20), with HIP events around its three device parts.

    python tools/cluster_bench.py [--rows 1000000] [--k 20] [--mincos 0.4] [--mincov 0.7] [--batch 4096] [--dir DIR]
                                  [--family_size S [--families F]] [--complete] [--cluster_mode {greedy,connected}]

Prints one JSON line:
  scan_ms / scan_ms_per_batch     the scan calls (k' = k + 1; the first call builds the image: `scan_first_ms`, left out of the
                                  per-batch figure when other calls follow)
  graph_write_ms / _us_per_batch  the drop step of every batch, writing rows [b0, b1) of the [n,k] graph tensors in place
  cluster_ms, rounds              ms_cluster_greedy on the finished graph (one call; it synchronises) and its mark / decide rounds
  clusters, singletons, saturated what it found; wall_s, setup_s of the whole run next to them
  --family_size S                 F planted families (--families, default 50) of S rows each replace rows of the database at
                                  random places: normalize(centre + 0.3 g / sqrt(128)), cosine ~ 0.92 inside a family -- lists
                                  that -k cuts short once S > k + 1
  --complete                      run `cluster --complete`: full_lists, edges, rescored (the share of the edge pass's cells that went
                                  to the exact chain: rescored_share) and edges_ms, the HIP-event spans of the edge pass's batches (edges_batches of them;
                                  edges_first_ms: the first, which loads the kernel), are added
  --cluster_mode connected        run `cluster --cluster_mode connected`: cluster_ms is then ms_cluster_components, rounds its hook /
                                  compress rounds, clusters its components; `largest` (the rows of the largest component) is added
  --tree                          run `cluster --cluster_mode connected --tree`: tree_ms (ms_cluster_tree inside the driver), tree_rounds
                                  and tree_edges are added, and tree_calls_ms / components_calls_ms: ms_cluster_tree and
                                  ms_cluster_components called alternately on the driver's graph tensors, seven times each, HIP events
                                  around each call (the first of each includes what a first call loads)
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


def plant_families(prefix: str, rows: int, families: int, size: int, seed: int = 1, sigma: float = 0.3) -> None:
    """Overwrite families * size rows of the database's matrix, at random places, with planted families: unit rows
    normalize(centre + sigma g / sqrt(128)) around random unit centres (what tests/cluster_case.planted_rows plants)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    count = families * size
    assert 0 < count <= rows
    centres = rng.standard_normal((families, 128))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    planted = np.repeat(centres, size, axis=0) + sigma * rng.standard_normal((count, 128)) / np.sqrt(128.0)
    planted = (planted / np.linalg.norm(planted, axis=1, keepdims=True)).astype(np.float32)
    with open(prefix + ".json") as handle:
        fname = json.load(handle)["dbfname_IP"]
    matrix = np.memmap(os.path.join(os.path.dirname(os.path.abspath(prefix)), fname), dtype=np.float32, mode="r+", shape=(rows, 128))
    matrix[np.sort(rng.choice(rows, size=count, replace=False))] = planted[rng.permutation(count)]
    matrix.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--mincos", type=float, default=0.4)
    ap.add_argument("--mincov", type=float, default=0.7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dir", type=str, default=None, help="where the database goes (default: a temporary directory, removed)")
    ap.add_argument("--family_size", type=int, default=0, help="rows per planted family (0: none)")
    ap.add_argument("--families", type=int, default=50, help="planted families, when --family_size is given")
    ap.add_argument("--complete", action="store_true", help="cluster the full threshold graph (cluster --complete)")
    ap.add_argument("--cluster_mode", type=str, default="greedy", choices=("greedy", "connected"), help="what is read off the graph")
    ap.add_argument("--tree", action="store_true", help="time ms_cluster_tree on the driver's graph (implies --cluster_mode connected)")
    args = ap.parse_args()
    if args.tree:
        args.cluster_mode = "connected"
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
            if args.family_size > 0:
                plant_families(prefix, args.rows, args.families, args.family_size)
        print("[cluster_bench] database of %d rows ready in %.1f s" % (args.rows, time.perf_counter() - t0), file=sys.stderr, flush=True)
        engine = ds.engine_setup("cuda:0")
        times = {}
        graph = []
        if args.tree:                                                     # keep the driver's graph tensors: the calls are repeated on them
            driver_call = engine.cluster_tree
            engine.cluster_tree = lambda *a: (graph.append(a), driver_call(*a))[1]
        t0 = time.perf_counter()
        _rep, _score, info = cluster.run_cluster(prefix, os.path.join(work, "out"), os.path.join(work, "tmp"), "cuda:0", topk=args.k,
                                                 mincos=args.mincos, mincov=args.mincov, query_batchsize=args.batch, engine=engine,
                                                 timings=times, complete=args.complete, mode=args.cluster_mode, tree=args.tree)
        wall = time.perf_counter() - t0
        extra = {"family_size": args.family_size, "families": args.families if args.family_size > 0 else 0, "complete": args.complete,
                 "full_lists": info["full_lists"], "cluster_mode": args.cluster_mode}
        if args.tree:
            import torch
            spans = {"tree": [], "components": []}
            graph[0] = graph[0][:5] + (engine.to_device(graph[0][5].astype("int32")),) + graph[0][6:]      # (the lengths: uploaded once, not per call)
            for _call in range(7):                                        # alternately, HIP events around each call (both synchronise)
                for name, call in (("tree", driver_call), ("components", engine.cluster_components)):
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    found = call(*graph[0])[2]
                    end.record()
                    torch.cuda.synchronize()
                    spans[name].append(round(start.elapsed_time(end), 3))
                    assert name != "tree" or (found["n_edges"], found["rounds"]) == (info["tree_edges"], info["tree_rounds"])
            extra.update(tree_ms=round(times["tree_ms"], 3), tree_rounds=info["tree_rounds"], tree_edges=info["tree_edges"],
                         tree_calls_ms=spans["tree"], components_calls_ms=spans["components"])
        if args.cluster_mode == "connected":
            extra["largest"] = info["largest"]
        if args.complete:
            cells = info["full_lists"] * args.rows
            extra.update(edges=info["edges"], rescored=info["rescored"], rescored_share=round(info["rescored"] / cells, 8) if cells else 0.0,
                         edges_ms=round(times.get("edges_ms", 0.0), 3), edges_first_ms=round(times.get("edges_first_ms", 0.0), 3),
                         edges_batches=times.get("edges_calls", 0))
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
            "clusters": info["n_components" if args.cluster_mode == "connected" else "n_reps"], "singletons": info["singletons"], "saturated": info["saturated"], **extra}), flush=True)
    finally:
        if args.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
