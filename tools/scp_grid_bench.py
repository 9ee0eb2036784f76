"""The reference's drone SAA grid (4 alphas x 30 repeats = 120 reduced SCP problems, M = 50, S = 20, 60 iterations:
drone_risk.py:480-539) solved twice on identical draws: as ONE lockstep batch (scp.run_drone_reduced_batch ->
rato_scp_batch_run_drone) and as a sequence of solo native loops (scp.run_drone_reduced per problem).  Prints one JSON
line: both wall-clocks, the speedup, the batched oracle round trips, the cuts of all problems and n_threads.

    python tools/scp_grid_bench.py [--iters 60] [--repeats 30] [--M 50] [--S 20] [--threads N] [--batched-only]

--system driving: the same for the reference's driving grid (alphas 0.01 / 0.02 / 0.05 / 0.1 x 30 repeats, 15 iterations,
every cell on draws of its own: driving.py:467-529) -- scp.run_driving_reduced_batch -> rato_scp_batch_run_car against
scp.run_driving_reduced(native_loop=True) per problem; --python-loop adds the per-iteration Python loop with the NumPy final
rows per problem (the driving path before the native loop existed).
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
    ap.add_argument("--system", choices=("drone", "driving"), default="drone")
    ap.add_argument("--iters", type=int, default=None, help="default: 60 (drone), 15 (driving)")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--alphas", type=str, default=None, help="default: 0.05,0.1,0.2,0.3 (drone), 0.01,0.02,0.05,0.1 (driving)")
    ap.add_argument("--M", type=int, default=50)
    ap.add_argument("--S", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=None)
    ap.add_argument("--batched-only", action="store_true", help="skip the sequential solo loops (profiling runs)")
    ap.add_argument("--python-loop", action="store_true", help="driving: also time the per-iteration Python loop per problem")
    args = ap.parse_args()
    import torch
    from riskaversetrajopt_amd import driving, drone_risk, scp
    car = args.system == "driving"
    if args.iters is None:
        args.iters = 15 if car else 60
    alphas = [float(a) for a in (args.alphas or ("0.01,0.02,0.05,0.1" if car else "0.05,0.1,0.2,0.3")).split(",")]
    if car:
        draws = scp.draw_driving_saa_batches(alphas, args.repeats, args.M, args.S, args.seed)
        build = lambda: [driving.Model(args.M, 'saa', a, S=args.S, samples=draws[i][r])
                         for i, a in enumerate(alphas) for r in range(args.repeats)]
        run_batch = scp.run_driving_reduced_batch
        run_solo = lambda m, iters: scp.run_driving_reduced(m, num_scp_iters_max=iters, native_loop=True)
    else:
        batches = scp.draw_saa_batches(args.repeats, args.M, args.S, args.seed)
        build = lambda: [drone_risk.Model(args.S, *batches[r], 'saa', a) for a in alphas for r in range(args.repeats)]
        run_batch = scp.run_drone_reduced_batch
        run_solo = lambda m, iters: scp.run_drone_reduced(m, num_scp_iters_max=iters)
    n_threads = scp._default_threads() if args.threads is None else args.threads
    # warm-up (library load, first launches, pinned pools) on a small batch of the same shape
    run_batch(build()[:2], num_scp_iters_max=3, n_threads=n_threads)
    torch.cuda.synchronize()
    models = build()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rb = run_batch(models, num_scp_iters_max=args.iters, n_threads=n_threads)
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    out = {"problems": len(models), "M": args.M, "S": args.S, "iters": args.iters, "n_threads": n_threads,
           "batched_s": round(t_batch, 4), "rounds": rb[0]["rounds"],
           "total_cuts": int(sum(int(np.sum(r["cuts"])) for r in rb))}
    if not args.batched_only:
        solo = build()
        run_solo(solo[0], 3)     # (warm-up of the solo path)
        solo = build()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rs = [run_solo(m, args.iters) for m in solo]
        torch.cuda.synchronize()
        t_seq = time.perf_counter() - t0
        out["sequential_s"] = round(t_seq, 4)
        out["speedup"] = round(t_seq / t_batch, 2)
        out["bitwise_equal"] = bool(all(np.array_equal(a["us_hist"], b["us_hist"]) for a, b in zip(rb, rs)))
    if car:
        out = {"system": "driving", **out}
        for key in ("define_s", "solve_s"):           # the batch's own clocks, summed over the iterations
            out["batch_" + key] = round(float(np.sum(rb[0][key])), 4)
        if args.python_loop:
            py = build()
            scp.run_driving_reduced(py[0], num_scp_iters_max=3)
            py = build()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for m in py:
                scp.run_driving_reduced(m, num_scp_iters_max=args.iters)
            torch.cuda.synchronize()
            out["python_loop_s"] = round(time.perf_counter() - t0, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
