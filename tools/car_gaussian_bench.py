"""Measures the driving Gaussian baseline on the GPU (nothing gates on it; bench.py is the flagship benchmark):

  * the K = 4 and K = 1 linearize launches (rato_car_gaussian_linearize) at S = 20 and S = 40: device events around
    `reps` back-to-back launches after a warm-up, repeated `rounds` times -> median and spread per launch;
  * the same define on the host by the fp64 NumPy restatement (tests/_car_gaussian.py), for scale;
  * the wall clock of the 4-alpha, 60-iteration experiment (scp.run_driving_gaussian_batch), split into defines (one K = 4
    launch + copy back per iteration) and QP solves, with the count of every qp.OSQP status: the reference's eps of 1e-8 may
    not be reached by the ADMM restatement within its iteration cap, and the reference itself only prints and continues;
  * the largest max-abs-scaled difference between the kernel and the restatement over the shapes of the GPU test
    (tests/test_gpu_car_gaussian.py), which sets that test's tolerance.

    python tools/car_gaussian_bench.py [--iters 60] [--out FILE.json]

Prints one JSON line.  There is no CPU fallback: without a GPU the kernel timings fail.
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_launch(model, us, al, reps, rounds):
    import torch
    us_d = torch.as_tensor(us, device=model.device)
    al_d = torch.as_tensor(al, device=model.device)
    for _ in range(10):
        model.linearize_device(us_d, al_d)
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            model.linearize_device(us_d, al_d)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / reps)
    per = np.array(per)
    return {"median_us": float(np.median(per)), "min_us": float(per.min()), "max_us": float(per.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("car_gaussian_bench needs a GPU: nothing here is measured on the host in its place")
    import _car_gaussian as R
    from riskaversetrajopt_amd import driving_gaussian as DG
    from riskaversetrajopt_amd import scp

    alphas = (0.01, 0.02, 0.05, 0.1)
    out = {"device": torch.cuda.get_device_name(0), "launch": {}, "host_restatement_define_s": {}}
    for S in (20, 40):
        m = DG.Model(alpha=0.05, S=S)
        us = np.stack([R.us_guess(S), R.us_steer(S), 0.5 * R.us_steer(S) + 0.01, 0.7 * R.us_steer(S) - 0.005])
        al = np.stack([R.alphas_uniform(S, a) for a in alphas])
        for K in (4, 1):
            out["launch"][f"S{S}_K{K}"] = time_launch(m, us[:K], al[:K], args.reps, args.rounds)
        t0 = time.perf_counter()
        for k in range(4):
            R.linearize(us[k], al[k])
        out["host_restatement_define_s"][f"S{S}_K4"] = time.perf_counter() - t0

    worst = 0.0
    for S in (1, 2, 5, 20, 40, 64):
        for outer in (False, True):
            m = DG.Model(alpha=0.05, S=S, outer_product=outer)
            us = np.stack([R.us_guess(S), R.us_steer(S), 0.5 * R.us_steer(S) + 0.01, 0.7 * R.us_steer(S) - 0.005])
            al = np.stack([R.alphas_uniform(S, 0.05), R.alphas_spread(S, 0.05), R.alphas_uniform(S, 0.1),
                           R.alphas_spread(S, 0.1)[::-1].copy()])
            got = {k: v.cpu().numpy() for k, v in m.linearize_device(us, al, want_trajectory=True).items()}
            for k in range(4):
                ref = R.linearize(us[k], al[k], outer)
                for key, g in got.items():
                    worst = max(worst, float(np.max(np.abs(g[k] - ref[key])) / np.max(np.abs(ref[key]))))
    out["kernel_vs_restatement_max_scaled_difference"] = worst

    models = [DG.Model(alpha=a, S=20) for a in alphas]
    scp.run_driving_gaussian_batch(models, 2)                      # warm-up: code objects, allocator, the QP set-up path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = scp.run_driving_gaussian_batch(models, args.iters)
    wall = time.perf_counter() - t0
    status = collections.Counter(s for r in res for s in r["status"])
    out["experiment"] = {"alphas": list(alphas), "S": 20, "iters": args.iters, "wall_s": wall,
                         "define_s": float(res[0]["define_s"].sum()), "solve_s": float(res[0]["solve_s"].sum()),
                         "qp_status": dict(status), "qp_solves": int(sum(status.values())),
                         "final_L2_error": [float(r["L2_error"][-1]) for r in res],
                         "alphas_risk_sum": [float(r["alphas_risk"].sum()) for r in res]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
