"""Measures the driving Gaussian baseline on the GPU (nothing gates on it; bench.py is the flagship benchmark):

  * the K = 4 and K = 1 linearize launches (rato_car_gaussian_linearize) at S = 20 and S = 40: device events around
    `reps` back-to-back launches after a warm-up, repeated `rounds` times -> median and spread per launch;
  * the same define on the host by the fp64 NumPy restatement (tests/_car_gaussian.py), for scale;
  * the wall clock of the 4-alpha, 60-iteration experiment (scp.run_driving_gaussian_batch), split into defines (one K = 4
    launch + copy back per iteration) and QP solves, with the count of every qp.OSQP status: the reference's eps of 1e-8 may
    not be reached by the ADMM restatement within its iteration cap, and the reference itself only prints and continues;
  * the largest max-abs-scaled difference between the kernel and the restatement over the shapes of the GPU test
    (tests/test_gpu_car_gaussian.py), which sets that test's tolerance;
  * the QP solve (rato_qp_ipm_batch_f64, ``qp_ipm``): ONE solve launch for K = 1 and K = 4 at S = 20 and S = 40 on the QPs of
    SCP iteration 2, device events as for the define, with the interior-point iterations each problem took; and the whole
    4-alpha experiment (``scp.driving_gaussian_experiment``) through solver='osqp' and through solver='ipm' in the same run:
    summed define_s / solve_s, and per alpha the status counts, the final L2 step, percentage_safe and cost.  This part goes
    to --qp-out (profiles/car_gaussian_qp.json).

    python tools/car_gaussian_bench.py [--iters 60] [--out FILE.json] [--qp-out FILE.json]

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


def time_events(fn, reps, rounds, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / reps)
    per = np.array(per)
    return {"median_us": float(np.median(per)), "min_us": float(per.min()), "max_us": float(per.max())}


def qp_launches(alphas, reps, rounds):
    """one rato_qp_ipm_batch_f64 launch on the QPs of SCP iteration 2 (iterations 0 and 1 run through solver='ipm')"""
    from riskaversetrajopt_amd import driving_gaussian as DG
    from riskaversetrajopt_amd import qp_ipm, scp
    out = {}
    for S in (20, 40):
        models = [DG.Model(alpha=a, S=S, solver='ipm') for a in alphas]
        us = [m.initial_guess_us_mat() for m in models]
        al = [m.initial_guess_alphas_risk() for m in models]
        for it in range(2):
            us, al, st = scp._gaussian_solve_all(models, us, al, it)
            assert st == ['solved'] * len(models), st
        lin = {k: v.cpu().numpy() for k, v in models[0].linearize_device(np.stack(us), np.stack(al)).items()}
        pres = []
        for k, m in enumerate(models):
            m.define_problem(us[k], al[k], 2, lin={key: v[k] for key, v in lin.items()})
            pres.append(qp_ipm.presolve(*m.osqp_prob.data()))
        for K in (1, 4):
            batch = qp_ipm.DeviceBatch(pres[0]["P"], pres[0]["q"], np.stack([p["A"] for p in pres[:K]]),
                                       np.stack([p["l"] for p in pres[:K]]), np.stack([p["u"] for p in pres[:K]]),
                                       DG.OSQP_TOL, 100, shared_objective=True)
            r = time_events(batch.launch, reps, rounds)
            info = batch.fetch()[2]
            r.update(n=int(batch.n), m=int(batch.m), status=[qp_ipm.STATUSES[int(s)] for s in info[:, 0]],
                     ipm_iterations=[int(i) for i in info[:, 1]], factorizations=[int(i) for i in info[:, 2]],
                     us_per_ipm_iteration=r["median_us"] / max(int(info[:, 1].max()), 1))
            out[f"S{S}_K{K}"] = r
    return out


def qp_experiment(alphas, iters, solver):
    from riskaversetrajopt_amd import scp
    r = scp.driving_gaussian_experiment(alphas, S=20, iters=iters, solver=solver)
    res = r["results"]
    return {"solver": solver, "S": 20, "iters": iters, "wall_s": r["wall_s"], "define_s": float(res[0]["define_s"].sum()),
            "solve_s": float(res[0]["solve_s"].sum()), "solve_s_per_scp_iteration_median": float(np.median(res[0]["solve_s"])),
            "define_s_per_scp_iteration_median": float(np.median(res[0]["define_s"])),
            "per_alpha": {str(a): {"status": dict(collections.Counter(x["status"])), "final_L2_step": float(x["L2_error"][-1]),
                                   "percentage_safe": float(r["percentage_safe"][k]), "cost": float(r["cost"][k])}
                          for k, (a, x) in enumerate(zip(alphas, res))},
            "solved": int(sum(s == "solved" for x in res for s in x["status"])), "qp_solves": int(sum(len(x["status"]) for x in res))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--qp-out", default=None)
    ap.add_argument("--qp-only", action="store_true", help="only the QP-solve part (--qp-out)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("car_gaussian_bench needs a GPU: nothing here is measured on the host in its place")
    import _car_gaussian as R
    from riskaversetrajopt_amd import driving_gaussian as DG
    from riskaversetrajopt_amd import scp

    alphas = (0.01, 0.02, 0.05, 0.1)
    if args.qp_out or args.qp_only:
        qp_experiment(alphas, 2, 'ipm')                            # warm-up: code objects, allocator
        qp = {"device": torch.cuda.get_device_name(0), "launch": qp_launches(alphas, max(args.reps // 10, 5), args.rounds),
              "experiment": {s: qp_experiment(alphas, args.iters, s) for s in ('osqp', 'ipm')}}
        qline = json.dumps(qp)
        print(qline)
        if args.qp_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.qp_out)), exist_ok=True)
            with open(args.qp_out, "w") as f:
                f.write(qline + "\n")
        if args.qp_only:
            return
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
