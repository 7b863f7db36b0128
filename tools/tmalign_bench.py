"""Batched TM-align throughput: pairs/s of ms_tmalign_batch on one GPU against the CPU restatement
(tests/tmalign_ref.c, order=seq, -O2) on 16 host threads, for the two workloads of a search:

  hits   10 queries x their top-10 hits, every length drawn from the shipped TED slice's histogram (ted_length_hist.npy)
  multi  a multi-domain matrix: 3 query domains x 200 target domains, lengths from the same histogram

    python tools/tmalign_bench.py [--reps 3] [--cpu-threads 16] [--fast] [--no-cpu]

Prints one JSON line per workload: GPU seconds per batch (median of --reps after one warm-up batch), pairs/s, the CPU
figures, and whether every GPU result equals the restatement's (order=kernel) on a sample of pairs."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def workload(name: str):
    from merizo_search_amd.foldclass import synthetic as syn
    import tm_case
    if name == "hits":
        lens = syn.ted_lengths(110, seed=11)
        pairs = [(q, 10 + 10 * q + h) for q in range(10) for h in range(10)]
    else:
        lens = syn.ted_lengths(203, seed=12)
        pairs = [(q, 3 + t) for q in range(3) for t in range(200)]
    lens = np.maximum(lens, 6)
    structs = [tm_case.walk(int(n), 500 + k) for k, n in enumerate(lens)]
    seqs = [tm_case.seq_of(int(n), k) for k, n in enumerate(lens)]
    return structs, seqs, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--fast", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--check", type=int, default=8, help="pairs checked against the restatement (order=kernel)")
    args = ap.parse_args()
    import torch
    from merizo_search_amd import ops
    import tmalign_ref as R

    for name in ("hits", "multi"):
        structs, seqs, pairs = workload(name)
        lens = np.array([len(s) for s in structs])
        ops.tmalign_batch(structs, seqs, pairs, fast=args.fast, device="cuda:0")           # warm-up (workspace, code object)
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ops.tmalign_batch(structs, seqs, pairs, fast=args.fast, device="cuda:0")
            times.append(time.perf_counter() - t0)
        gpu_s = float(np.median(times))
        alone = []
        for p in sorted({0, len(pairs) - 1, int(np.argmax([lens[a] * lens[b] for a, b in pairs]))}):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.tmalign_batch(structs, seqs, [pairs[p]], fast=args.fast, device="cuda:0")
            alone.append({"pair": [int(lens[pairs[p][0]]), int(lens[pairs[p][1]])], "s": round(time.perf_counter() - t0, 4)})
        sample = np.random.default_rng(0).choice(len(pairs), size=min(args.check, len(pairs)), replace=False)
        equal = True
        for p in sample:
            a, b = pairs[p]
            ref = R.tm_align(structs[a], structs[b], seqs[a], seqs[b], fast=args.fast, order="kernel", quantize=False)
            equal &= all(np.float64(got[k][p]).tobytes() == np.float64(ref[k]).tobytes() for k in ("qtm", "ttm", "rmsd"))
        line = {"workload": name, "pairs": len(pairs), "fast": args.fast, "mean_len": round(float(lens.mean()), 1),
                "max_len": int(lens.max()), "gpu_s": round(gpu_s, 4), "gpu_pairs_per_s": round(len(pairs) / gpu_s, 1),
                "gpu_single_pair_s": alone, "bit_equal_to_restatement": bool(equal), "checked": len(sample)}
        if not args.no_cpu:
            R.load()
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=args.cpu_threads) as pool:
                list(pool.map(lambda pq: R.tm_align(structs[pq[0]], structs[pq[1]], seqs[pq[0]], seqs[pq[1]], fast=args.fast,
                                                    order="seq", quantize=False), pairs))
            cpu_s = time.perf_counter() - t0
            line.update(cpu_threads=args.cpu_threads, cpu_s=round(cpu_s, 3), cpu_pairs_per_s=round(len(pairs) / cpu_s, 1),
                        gpu_over_cpu=round(cpu_s / gpu_s, 2))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
