"""The reference's drone SAA grid (4 alphas x 30 repeats = 120 reduced SCP problems, M = 50, S = 20, 60 iterations:
drone_risk.py:480-539) solved twice on identical draws: as ONE lockstep batch (scp.run_drone_reduced_batch ->
rato_scp_batch_run_drone) and as a sequence of solo native loops (scp.run_drone_reduced per problem).  Prints one JSON
line: both wall-clocks, the speedup, the batched oracle round trips, the cuts of all problems and n_threads.

    python tools/scp_grid_bench.py [--iters 60] [--repeats 30] [--M 50] [--S 20] [--threads N] [--batched-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--alphas", type=str, default="0.05,0.1,0.2,0.3")
    ap.add_argument("--M", type=int, default=50)
    ap.add_argument("--S", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=None)
    ap.add_argument("--batched-only", action="store_true", help="skip the sequential solo loops (profiling runs)")
    args = ap.parse_args()
    import torch
    from riskaversetrajopt_amd import drone_risk, scp
    alphas = [float(a) for a in args.alphas.split(",")]
    batches = scp.draw_saa_batches(args.repeats, args.M, args.S, args.seed)
    build = lambda: [drone_risk.Model(args.S, *batches[r], 'saa', a) for a in alphas for r in range(args.repeats)]
    n_threads = scp._default_threads() if args.threads is None else args.threads
    # warm-up (library load, first launches, pinned pools) on a small batch of the same shape
    scp.run_drone_reduced_batch(build()[:2], num_scp_iters_max=3, n_threads=n_threads)
    torch.cuda.synchronize()
    models = build()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rb = scp.run_drone_reduced_batch(models, num_scp_iters_max=args.iters, n_threads=n_threads)
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    out = {"problems": len(models), "M": args.M, "S": args.S, "iters": args.iters, "n_threads": n_threads,
           "batched_s": round(t_batch, 4), "rounds": rb[0]["rounds"],
           "total_cuts": int(sum(int(np.sum(r["cuts"])) for r in rb))}
    if not args.batched_only:
        solo = build()
        scp.run_drone_reduced(solo[0], num_scp_iters_max=3)     # (warm-up of the solo path)
        solo = build()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rs = [scp.run_drone_reduced(m, num_scp_iters_max=args.iters) for m in solo]
        torch.cuda.synchronize()
        t_seq = time.perf_counter() - t0
        out["sequential_s"] = round(t_seq, 4)
        out["speedup"] = round(t_seq / t_batch, 2)
        out["bitwise_equal"] = bool(all(np.array_equal(a["us_hist"], b["us_hist"]) for a, b in zip(rb, rs)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
