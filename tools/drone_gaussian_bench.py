"""Measures the drone Gaussian baseline on the GPU (nothing gates on it; bench.py is the flagship benchmark):

  * the linearize call (rato_drone_gaussian_linearize) and the Hessian call (rato_drone_gaussian_hessian) at S = 20 and
    S = 64 (the largest), K = 1 and K = 4: device events around `reps` back-to-back calls after a warm-up, repeated `rounds`
    times -> median and spread per call;
  * the same callbacks on the host by the fp64 NumPy restatement (tests/_drone_gaussian.py), and ONE torch
    jacfwd o jacfwd Hessian of an independent torch forward (tests/test_drone_gaussian_pin.py) at S = 5 and S = 20, for scale;
  * one full `scp.run_drone_gaussian` at S = 5 from the prototype's start point with its callback / total split, its
    status, iterations, violation and optimality;
  * the largest max-abs-scaled difference between the kernels and the restatement over the shapes of the GPU test
    (tests/test_gpu_drone_gaussian.py), the Hessian per block, which sets that test's tolerance.

    python tools/drone_gaussian_bench.py [--maxiter 3000] [--out profiles/drone_gaussian_bench.json]

With ``--solver {trust-constr,ipm,both}`` it measures the SOLVE instead and writes profiles/drone_gaussian_solve.json: the
script's experiment (S = 20, alpha in 0.05, 0.1, 0.2, 0.3, every alpha from its SAA repeat-0 solution, made first where
``--results-dir`` does not hold it) through ``scp.drone_gaussian_experiment`` with scipy's trust-constr (one alpha after the
other) and / or the batched interior-point method (``drone_gaussian_ipm``: all alphas in one ``solve_batch`` call), in the same
process.  Per alpha and solver: status, iterations, factorizations (ipm) or evaluations (trust-constr), E_0 (ipm) or
constraint violation and optimality (trust-constr), f, percentage_safe of the 10,000-sample Monte-Carlo block and the wall
clock; for the batch the split of its wall clock into callbacks / normal matrix / factor / solves / matvecs / host, in total
and per lockstep iteration.  Nothing is tuned towards an outcome: an alpha that ends in 'line_search' or 'max_iter' is
reported as that.

    python tools/drone_gaussian_bench.py --solver both [--results-dir results] [--out profiles/drone_gaussian_solve.json]

With ``--solver ipm --driver {host,device,both}`` it measures the interior-point solve under one or both drivers (DESIGN
§7.ag: the iterate on the host or on the device) and writes profiles/drone_gaussian_solve_device_driver.json: the same
batch of four alphas from their SAA starts, both drivers in this process on one board, each after a warm-up solve, the
median of ``--solves`` solves, the iterations per alpha, and from one more solve with a device-wide wait behind every block
the split of a lockstep iteration.

    python tools/drone_gaussian_bench.py --solver ipm --driver both [--solves 7]

``--driver`` also takes ``device_grid`` (the device driver with its own vector kernels spread over the rows) and
``all`` (host, device and device_grid; ``both`` stays host and device).  The timed solves of the drivers alternate.

With ``--solver ipm --chol {workgroup,grid,both}`` it measures the interior-point solve under one or both Choleskys (DESIGN
§7.ak: csrc/chol.hip, one workgroup per problem, or csrc/chol_grid.hip, one launch per panel over the whole device; the same
bits) and writes profiles/drone_gaussian_solve_chol_grid.json: the same batch under ``--driver`` (default device; with ``both``,
both), the methods in this process on one board, each after a warm-up solve, the median of ``--solves`` (default 5 here)
solves with min and max, the iterations per alpha, the split of a lockstep iteration from one more solve with a device-wide
wait behind every block, and whether every (Z, info) is bitwise the same under both methods.

    python tools/drone_gaussian_bench.py --solver ipm --chol both [--driver device] [--solves 5]

Prints one JSON line.  There is no CPU fallback: without a GPU the kernel timings fail.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_call(fn, reps, rounds):
    import torch
    for _ in range(10):
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


def scaled(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


def write(out, path):
    line = json.dumps(out)
    print(line, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


def solve_bench(args):
    """the S = 20 experiment with one or both solvers -> the dictionary written to profiles/drone_gaussian_solve.json"""
    import torch
    import _drone_gaussian as R
    from riskaversetrajopt_amd import drone_gaussian as DG
    from riskaversetrajopt_amd import drone_gaussian_ipm, scp
    S, alphas = 20, (0.05, 0.1, 0.2, 0.3)
    path = args.out or os.path.join(ROOT, "profiles", "drone_gaussian_solve.json")
    out = {"device": torch.cuda.get_device_name(0), "S": S, "alphas": list(alphas), "tol": args.tol, "maxiter": args.maxiter,
           "start": "SAA repeat 0 (drone_saa_experiment, M = 50, 60 iterations, seed 0)", "M_mc": 10000}
    # warm-up: code objects, allocator, the SAA starts
    drone_gaussian_ipm.solve_batch([DG.Model(5, alpha=0.1)], [R.start_point(5, 0.1)], max_iter=3)
    scp.run_drone_gaussian(DG.Model(5, alpha=0.1), Z0=R.start_point(5, 0.1), maxiter=3)
    if args.solver in ("ipm", "both"):
        clocks = {}
        r = scp.drone_gaussian_experiment(alphas, S=S, results_dir=args.results_dir, maxiter=args.maxiter, solver='ipm',
                                          tol=args.tol, clocks=clocks)
        rounds = max(1, max(x["info"]["iterations"] for x in r["results"]))
        out["ipm"] = {"wall_s": r["wall_s"], "clocks_s": clocks, "lockstep_iterations": rounds,
                      "per_iteration_ms": {k: 1e3 * v / rounds for k, v in clocks.items()},
                      "per_alpha": [{"alpha": a, "status": x["status"], "iterations": x["info"]["iterations"],
                                     "factorizations": x["info"]["factorizations"], "E0": x["info"]["E0"],
                                     "primal_infeasibility": x["info"]["primal_infeasibility"],
                                     "dual_infeasibility": x["info"]["dual_infeasibility"], "f": x["fun"],
                                     "percentage_safe": float(s), "cost": float(c)}
                                    for a, x, s, c in zip(alphas, r["results"], r["percentage_safe"], r["cost"])]}
        write(out, path)
    if args.solver in ("trust-constr", "both"):
        r = scp.drone_gaussian_experiment(alphas, S=S, results_dir=args.results_dir, maxiter=args.maxiter)
        out["trust_constr"] = {"wall_s": r["wall_s"],
                               "per_alpha": [{"alpha": a, "status": x["status"], "message": x["message"], "iterations": x["nit"],
                                              "evaluations": x["nfev"], "constr_violation": x["constr_violation"],
                                              "optimality": x["optimality"], "f": x["fun"], "callback_s": x["callback_s"],
                                              "wall_s": x["total_s"], "percentage_safe": float(s), "cost": float(c)}
                                             for a, x, s, c in zip(alphas, r["results"], r["percentage_safe"], r["cost"])]}
        write(out, path)


DRIVER_SETS = {"both": ("host", "device"), "all": ("host", "device", "device_grid")}


def driver_bench(args):
    """the S = 20 batch under the host and / or the device driver -> profiles/drone_gaussian_solve_device_driver.json"""
    import torch
    from riskaversetrajopt_amd import drone_gaussian as DG
    from riskaversetrajopt_amd import drone_gaussian_ipm, scp
    S, alphas = 20, (0.05, 0.1, 0.2, 0.3)
    path = args.out or os.path.join(ROOT, "profiles", "drone_gaussian_solve_device_driver.json")
    out = {"device": torch.cuda.get_device_name(0), "S": S, "alphas": list(alphas), "tol": args.tol, "maxiter": args.maxiter,
           "start": "SAA repeat 0 (drone_saa_experiment, M = 50, 60 iterations, seed 0)", "solves": args.solves, "drivers": {}}
    drivers = DRIVER_SETS.get(args.driver, (args.driver,))
    # the SAA starts where they are missing (and the code objects of everything around the solve)
    scp.drone_gaussian_experiment(alphas, S=S, results_dir=args.results_dir, maxiter=3, solver='ipm', tol=args.tol)
    models = [DG.Model(S, alpha=a) for a in alphas]
    Z0s = [m.initial_guess(args.results_dir) for m in models]
    solve = lambda d, ck=None: drone_gaussian_ipm.solve_batch(models, Z0s, tol=args.tol, max_iter=args.maxiter, driver=d, clocks=ck)
    for d in drivers:
        solve(d)                                                     # warm-up: code objects, allocator
    torch.cuda.synchronize()
    walls, sols = {d: [] for d in drivers}, {}
    for _ in range(args.solves):                                     # alternating: a drift of the board meets every driver
        for d in drivers:
            t0 = time.perf_counter()
            sols[d] = solve(d)
            walls[d].append(time.perf_counter() - t0)
    for d in drivers:
        rounds = max(1, max(info["iterations"] for _, info in sols[d]))
        drone_gaussian_ipm.DeviceBackend.sync_clocks = True          # one more solve, a device-wide wait behind every block
        try:
            clocks = {}
            solve(d, clocks)
        finally:
            drone_gaussian_ipm.DeviceBackend.sync_clocks = False
        w = walls[d]
        out["drivers"][d] = {"wall_ms": [1e3 * x for x in w], "median_wall_ms": 1e3 * float(np.median(w)),
                             "min_wall_ms": 1e3 * min(w), "max_wall_ms": 1e3 * max(w),
                             "lockstep_iterations": rounds, "median_ms_per_iteration": 1e3 * float(np.median(w)) / rounds,
                             "per_alpha": [{"alpha": a, "status": info["status"], "iterations": info["iterations"],
                                            "factorizations": info["factorizations"], "E0": info["E0"], "f": info["f"]}
                                           for a, (_, info) in zip(alphas, sols[d])],
                             "split_solve_wall_ms": 1e3 * clocks["wall"],
                             "split_ms_per_iteration": {k: 1e3 * v / rounds for k, v in clocks.items()}}
    if "host" in drivers and "device" in drivers:
        h, dv = out["drivers"]["host"], out["drivers"]["device"]
        out["host_over_device"] = h["median_wall_ms"] / dv["median_wall_ms"]
    if "device" in drivers and "device_grid" in drivers:
        dv, dg = out["drivers"]["device"], out["drivers"]["device_grid"]
        out["device_over_device_grid"] = dv["median_wall_ms"] / dg["median_wall_ms"]
        out["device_grid_is_bitwise_device"] = all(same_solution(a, b, but=("driver",)) for a, b in zip(sols["device_grid"], sols["device"]))
        out["command"] = "python tools/drone_gaussian_bench.py " + " ".join(sys.argv[1:])
    write(out, path)


def same_solution(r0, r1, but=()):
    (Z0, i0), (Z1, i1) = r0, r1
    eq = lambda a, b: a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b
    return Z0.tobytes() == Z1.tobytes() and set(i0) == set(i1) and all(eq(i0[k], i1[k]) for k in i0 if k not in but)


def chol_bench(args):
    """the S = 20 batch under one or both Choleskys -> profiles/drone_gaussian_solve_chol_grid.json"""
    import torch
    from riskaversetrajopt_amd import drone_gaussian as DG
    from riskaversetrajopt_amd import drone_gaussian_ipm, scp
    S, alphas = 20, (0.05, 0.1, 0.2, 0.3)
    path = args.out or os.path.join(ROOT, "profiles", "drone_gaussian_solve_chol_grid.json")
    solves = 5 if args.solves is None else args.solves
    out = {"device": torch.cuda.get_device_name(0), "S": S, "alphas": list(alphas), "tol": args.tol, "maxiter": args.maxiter,
           "start": "SAA repeat 0 (drone_saa_experiment, M = 50, 60 iterations, seed 0)", "solves": solves, "drivers": {}}
    drivers = DRIVER_SETS.get(args.driver, (args.driver or "device",))
    methods = ("workgroup", "grid") if args.chol == "both" else (args.chol,)
    scp.drone_gaussian_experiment(alphas, S=S, results_dir=args.results_dir, maxiter=3, solver='ipm', tol=args.tol)   # the SAA starts
    models = [DG.Model(S, alpha=a) for a in alphas]
    Z0s = [m.initial_guess(args.results_dir) for m in models]
    out["n"] = int(models[0].nvar)
    for d in drivers:
        solve = lambda c, ck=None: drone_gaussian_ipm.solve_batch(models, Z0s, tol=args.tol, max_iter=args.maxiter, driver=d,
                                                                  clocks=ck, chol=c)
        rec, sols = {}, {}
        for c in methods:
            solve(c)                                                 # warm-up of this method: code objects, allocator
        torch.cuda.synchronize()
        for c in methods:
            walls = []
            for _ in range(solves):
                t0 = time.perf_counter()
                sols[c] = solve(c)
                walls.append(time.perf_counter() - t0)
            rounds = max(1, max(info["iterations"] for _, info in sols[c]))
            drone_gaussian_ipm.DeviceBackend.sync_clocks = True      # one more solve, a device-wide wait behind every block
            try:
                clocks = {}
                solve(c, clocks)
            finally:
                drone_gaussian_ipm.DeviceBackend.sync_clocks = False
            rec[c] = {"wall_ms": [1e3 * w for w in walls], "median_wall_ms": 1e3 * float(np.median(walls)),
                      "min_wall_ms": 1e3 * min(walls), "max_wall_ms": 1e3 * max(walls), "lockstep_iterations": rounds,
                      "median_ms_per_iteration": 1e3 * float(np.median(walls)) / rounds,
                      "per_alpha": [{"alpha": a, "status": info["status"], "iterations": info["iterations"],
                                     "factorizations": info["factorizations"], "E0": info["E0"], "f": info["f"]}
                                    for a, (_, info) in zip(alphas, sols[c])],
                      "split_ms_per_iteration_sync_clocks": {k: 1e3 * v / rounds for k, v in clocks.items()}}
        if len(methods) == 2:
            w, g = rec["workgroup"], rec["grid"]
            rec["grid_is_bitwise_workgroup"] = all(same_solution(a, b) for a, b in zip(sols["grid"], sols["workgroup"]))
            rec["workgroup_over_grid"] = w["median_wall_ms"] / g["median_wall_ms"]
            rec["grid_wins"], rec["grid_loses"] = g["max_wall_ms"] < w["min_wall_ms"], g["min_wall_ms"] > w["max_wall_ms"]
        out["drivers"][d] = rec
    write(out, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--solver", choices=("trust-constr", "ipm", "both"), default=None)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--results-dir", default="results")
    ap.add_argument("--driver", choices=("host", "device", "device_grid", "both", "all"), default=None,
                    help="both: host and device; all: host, device and device_grid")
    ap.add_argument("--solves", type=int, default=None, help="timed solves per driver (default 7) or per Cholesky (default 5)")
    ap.add_argument("--chol", choices=("workgroup", "grid", "both"), default=None,
                    help="measure the interior-point solve under the Cholesky method(s) instead (with --solver ipm)")
    args = ap.parse_args()
    if args.driver is not None and args.solver != "ipm":
        raise SystemExit("--driver measures the interior-point solve: use it with --solver ipm")
    if args.chol is not None and args.solver != "ipm":
        raise SystemExit("--chol measures the interior-point solve: use it with --solver ipm")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("drone_gaussian_bench needs a GPU: nothing here is measured on the host in its place")
    if args.chol is not None:
        return chol_bench(args)
    if args.solves is None:
        args.solves = 7
    if args.driver is not None:
        return driver_bench(args)
    if args.solver is not None:
        return solve_bench(args)
    import _drone_gaussian as R
    from riskaversetrajopt_amd import drone_gaussian as DG
    from riskaversetrajopt_amd import scp

    out = {"device": torch.cuda.get_device_name(0), "linearize": {}, "hessian": {}, "host_restatement_s": {},
           "torch_hessian_s": {}}
    for S in (20, DG.MAX_S):
        m = DG.Model(S, alpha=0.1)
        pr = R.problems(S, 4)
        Z = torch.as_tensor(np.stack([p[0] for p in pr]), device="cuda")
        lam = torch.as_tensor(np.stack([p[1] for p in pr]), device="cuda")
        for K in (1, 4):
            out["linearize"][f"S{S}_K{K}"] = time_call(lambda: m.linearize_device(Z[:K]), args.reps, args.rounds)
            out["hessian"][f"S{S}_K{K}"] = time_call(lambda: m.hessian_device(Z[:K], lam[:K]), args.reps, args.rounds)
        t0 = time.perf_counter()
        R.evaluate(pr[0][0], S, [pr[0][1]])
        out["host_restatement_s"][f"S{S}_K1"] = time.perf_counter() - t0

    import test_drone_gaussian_pin as T
    for S in (5, 20):
        Z, lam = R.problems(S, 1)[0]
        Zt, lt, c = torch.as_tensor(Z), torch.as_tensor(lam), R.constants(S)
        t0 = time.perf_counter()
        torch.func.jacfwd(torch.func.jacfwd(lambda z: torch.dot(lt, T._torch_g(z, S, c))))(Zt)
        out["torch_hessian_s"][f"S{S}"] = time.perf_counter() - t0

    worst = {"linearize": 0.0, "hess_uu": 0.0, "hess_ua": 0.0, "hess_aa": 0.0}
    for S in (1, 2, 3, 5, 20, 22, DG.MAX_S):
        m = DG.Model(S, alpha=0.1)
        pr = R.problems(S, 4)
        Z, lam = np.stack([p[0] for p in pr]), np.stack([p[1] for p in pr])
        got = {k: v.cpu().numpy() for k, v in m.linearize_device(Z, want_trajectory=True).items()}
        hess = m.hessian_device(Z, lam).cpu().numpy()
        nvar = R.sizes(S)[0]
        for k in range(4):
            ref = R.evaluate(Z[k], S, [lam[k]])
            for key, g in got.items():
                worst["linearize"] = max(worst["linearize"], scaled(g[k], ref[key]))
            H = np.zeros((nvar, nvar))
            H[np.tril_indices(nvar)] = hess[k]
            H = H + np.tril(H, -1).T
            for name, a, b in zip(("hess_uu", "hess_ua", "hess_aa"), R.hess_blocks(H, S), R.hess_blocks(ref["hess"][0], S)):
                worst[name] = max(worst[name], scaled(a, b))
    out["kernel_vs_restatement_max_scaled_difference"] = worst

    S = 5
    m = DG.Model(S, alpha=0.1)
    scp.run_drone_gaussian(m, Z0=R.start_point(S, 0.1), maxiter=3)       # warm-up: code objects, allocator
    res = scp.run_drone_gaussian(m, Z0=R.start_point(S, 0.1), maxiter=args.maxiter)
    out["solve_S5"] = {k: res[k] for k in ("status", "message", "nit", "nfev", "constr_violation", "optimality", "fun",
                                           "callback_s", "total_s")}
    write(out, args.out)


if __name__ == "__main__":
    main()
