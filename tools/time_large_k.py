"""ops.ip_topk_large against ops.ip_topk (the ceil(k / 64)-scan path) in one process, on the synthetic unit database: device
events around each call, warm-up, medians, the two alternating; the results are compared bit for bit at every timed shape.
The log under profiles/ and the table of DESIGN.md section 5.13 come from this tool.

    python tools/time_large_k.py [--n 200000,1000000,4000000] [--nq 1,8,256,4096] [--k 100,200,1000] [--budget 2.0] [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from merizo_search_amd import ops
from merizo_search_amd.foldclass import synthetic as syn

BOUND = 1.0 + 1e-5


def ints(text):
    return [int(x) for x in text.split(",") if x]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=ints, default=[200_000, 1_000_000, 4_000_000])
    ap.add_argument("--nq", type=ints, default=[1, 8, 256, 4096])
    ap.add_argument("--k", type=ints, default=[100, 200, 1000])
    ap.add_argument("--budget", type=float, default=2.0, help="seconds of timed calls per shape and path (3..25 repetitions)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# n nq k | ip_topk ms (median, min) | ip_topk_large ms (median, min) | ratio | first second fallback rescored | reps")
    lws, tws = ops.LargeKWorkspace("cuda:0"), ops.TopKWorkspace("cuda:0")
    for n in args.n:
        db = syn.device_database(n, 0, 0, "cuda:0", normalize=True)
        for nq in args.nq:
            q = torch.randn(nq, 128, device="cuda", generator=torch.Generator("cuda").manual_seed(nq))
            q = q / q.norm(dim=1, keepdim=True)
            for k in args.k:
                st = {}
                base = lambda: ops.ip_topk(db, q, k, workspace=tws)
                large = lambda: ops.ip_topk_large(db, q, k, BOUND, workspace=lws, stats=st)
                t0, want = timed(base)                             # warm-up of both, and the comparison
                t1, got = timed(large)
                same = torch.equal(want[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(want[1], got[1])
                if not same:
                    say(f"{n} {nq} {k} | RESULTS DIFFER")
                    continue
                timed(base), timed(large)
                reps = int(min(25, max(3, args.budget * 1e3 / max(t0, t1, 1e-3))))
                tb, tl = [], []
                for _ in range(reps):                              # alternating: other work on the machine hits both alike
                    tb.append(timed(base)[0])
                    tl.append(timed(large)[0])
                mb, ml = float(np.median(tb)), float(np.median(tl))
                say(f"{n} {nq} {k} | {mb:.3f} {min(tb):.3f} | {ml:.3f} {min(tl):.3f} | {mb / ml:.2f} | {st['first_round']} {st['second_round']} "
                    f"{st['fallback']} {st['rescored']} | {reps}")
        del db
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
