"""Solves the hopper script's two runs (hopper.py:455-680) on the GPU and reports what the solver did (nothing gates on it;
bench.py is the flagship benchmark):

  * the baseline from ``initial_guess()`` and the six alphas of the SAA problem in one lockstep batch from its solution
    (``scp.hopper_experiment``, S = M = 30, fields from ``RandomState(1)``, tol = 1e-3, max_iter = 3000): per problem the
    status, iterations, factorizations, the final E_0, primal and dual infeasibility, f and x_S[0];
  * the wall clock of both runs and its split over callbacks (``nlp_device`` and the read-back of g) / normal matrix / factor /
    solve / host (the rest: the matvec launches, the line search's vector algebra, Python), in total and per iteration of the
    batch;
  * the same two runs with backend='numpy' (the step on the host, the Model's device callbacks one problem at a time).

    python tools/hopper_solve_bench.py [--out profiles/hopper_solve.json] [--S 30 --M 30]

Prints one JSON line.  There is no CPU fallback: without a GPU nothing is measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem_record(r, S):
    i = r["info"]
    return {"status": i["status"], "iterations": int(i["iterations"]), "factorizations": int(i["factorizations"]),
            "E0": float(i["E0"]), "primal_infeasibility": float(i["primal_infeasibility"]),
            "dual_infeasibility": float(i["dual_infeasibility"]), "f": float(i["f"]), "x_S0": float(r["Z"][8 * S])}


def split(clock, iters):
    wall = clock["wall"]
    parts = {k: clock.get(k, 0.0) for k in ("callbacks", "normal", "factor", "solve")}
    parts["host"] = wall - sum(parts.values())
    return {"wall_s": wall, "batch_iterations": iters, "seconds": parts,
            "ms_per_iteration": {k: 1e3 * v / max(iters, 1) for k, v in parts.items()}}


def run(backend, args):
    from riskaversetrajopt_amd import scp
    clocks = {}
    out = scp.hopper_experiment(alphas=args.alphas, M=args.M, S=args.S, seed=1, tol=1e-3, max_iter=3000, backend=backend,
                                clocks=clocks)
    base = problem_record(out["base"], args.S)
    saa = {str(a): problem_record(r, args.S) for a, r in zip(out["alphas"], out["results"])}
    return {"baseline": base, "saa": saa, "wall_s": out["wall_s"],
            "baseline_split": split(clocks["base"], base["iterations"]),
            "saa_split": split(clocks["saa"], max([r["iterations"] for r in saa.values()] + [0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=30)
    ap.add_argument("--M", type=int, default=30)
    ap.add_argument("--alphas", type=float, nargs="*", default=[0.05, 0.1, 0.2, 0.3, 0.5, 0.75])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hopper_solve.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hopper_solve_bench needs a GPU: nothing here is measured on the host in its place")
    run("device", args)                                              # warm-up: library load, maps, allocator
    out = {"device": torch.cuda.get_device_name(0), "S": args.S, "M": args.M, "tol": 1e-3, "max_iter": 3000,
           "backend_device": run("device", args), "backend_numpy": run("numpy", args)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
