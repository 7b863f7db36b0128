"""The TM-align stage of `cluster --mintm` on a synthetic database large enough to fill the chip: pairs/s of the stage on one GPU
next to the CPU restatement (tests/tmalign_ref.c, order=seq, -O2) on 16 host threads over a sample of the same pairs.

    python tools/cluster_tm_bench.py [--rows 10000] [-k 10] [--fast] [--cpu-sample 3200] [--cpu-threads 16] [--no-cpu]

The database: random unit rows (every row's k nearest neighbours count: --mincos -1), random-walk CA traces with lengths drawn
from the shipped TED slice's histogram, coverage 0.7 -- so the pairs are the neighbour pairs whose lengths are compatible, which
is what decides an alignment's cost.  Prints one JSON line: the distinct pairs, the stage's HIP-event span (`tm_ms`: pair
extraction, record fetch, coordinate conversion, alignment launches, write-back), the time inside the alignment launches alone,
both as pairs/s, and the CPU figure."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("-k", "--topk", type=int, default=10)
    ap.add_argument("--mintm", type=float, default=0.5)
    ap.add_argument("--fast", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=3200)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from merizo_search_amd.foldclass import cluster, dbutil, synthetic as syn, tmalign
    from merizo_search_amd.foldclass.engine import HipEngine
    import tm_case

    n = args.rows
    lengths = np.maximum(syn.ted_lengths(n, seed=21), 6)
    coords = [syn.random_walk(int(l), 9000 + r) for r, l in enumerate(lengths)]
    seqs = [tm_case.seq_of(int(l), r) for r, l in enumerate(lengths)]
    rows = syn.normalized_database(n, seed=22)
    work = tempfile.mkdtemp(prefix="cluster_tm_bench_")
    dbutil.write_faiss_db(os.path.join(work, "db"), rows, ["d%06d" % r for r in range(n)], seqs, coords)

    spent, seen = {"align_s": 0.0, "launches": 0}, {}
    real = HipEngine.tmalign_batch

    def timed(self, coords_list, seq_list, pairs, fast=False):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = real(self, coords_list, seq_list, pairs, fast=fast)
        spent["align_s"] += time.perf_counter() - t0
        spent["launches"] += 1
        if not seen:                                                      # the first launch's pairs: what the CPU sample is drawn from
            seen.update(coords=coords_list, seqs=seq_list, pairs=np.asarray(pairs))
        return got

    HipEngine.tmalign_batch = timed
    timings = {}
    t0 = time.perf_counter()
    _rep, _score, info = cluster.run_cluster(os.path.join(work, "db"), os.path.join(work, "out"), os.path.join(work, "tmp"), "cuda", topk=args.topk,
                                             mincos=-1.0, mincov=0.7, mintm=args.mintm, fastmode=args.fast, timings=timings)
    wall = time.perf_counter() - t0
    pairs = info["tm_pairs"]
    line = {"rows": n, "k": args.topk, "fast": args.fast, "mean_len": round(float(lengths.mean()), 1), "max_len": int(lengths.max()),
            "tm_pairs": pairs, "tm_rejected_pairs": info["tm_rejected_pairs"], "tm_removed_entries": info["tm_removed_entries"],
            "n_reps": info["n_reps"], "run_s": round(wall, 2), "scan_ms": round(timings.get("scan_ms", 0.0), 1),
            "cluster_ms": round(timings["cluster_ms"], 2), "tm_ms": round(timings["tm_ms"], 1),
            "stage_pairs_per_s": round(pairs / (timings["tm_ms"] / 1e3), 1), "align_s": round(spent["align_s"], 3), "launches": spent["launches"],
            "align_pairs_per_s": round(pairs / spent["align_s"], 1)}
    if not args.no_cpu:
        import tmalign_ref as R
        R.load()
        sample = np.random.default_rng(0).choice(len(seen["pairs"]), size=min(args.cpu_sample, len(seen["pairs"])), replace=False)
        todo = [tuple(seen["pairs"][p]) for p in sample]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=args.cpu_threads) as pool:
            list(pool.map(lambda ab: R.tm_align(seen["coords"][ab[0]], seen["coords"][ab[1]], seen["seqs"][ab[0]], seen["seqs"][ab[1]],
                                                fast=args.fast, order="seq", quantize=False), todo))
        cpu_s = time.perf_counter() - t0
        line.update(cpu_threads=args.cpu_threads, cpu_sample=len(todo), cpu_s=round(cpu_s, 2), cpu_pairs_per_s=round(len(todo) / cpu_s, 1),
                    align_over_cpu=round((pairs / spent["align_s"]) / (len(todo) / cpu_s), 2))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
