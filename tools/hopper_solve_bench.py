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

``--newton arrow --M 30,1000,10000`` measures the arrowhead Newton step (``hopper_arrow``, newton='arrow') instead,
into profiles/hopper_solve_large_m.json: per M the same two runs (one run after a warm-up, the same call capped at three
iterations), the training fields being the script's 30 of ``RandomState(1)`` extended to M by further draws of the same stream;
per problem the record above; the per-iteration split callbacks / reduction / assembly / factor / solves / products / host;
every solution's safe fraction and AVaR on the script's 10 000 validation fields (the draws that follow the 30 training fields
on the same stream, hopper.py:974-979); and at M = 30 the dense step in the same process.  The file is rewritten after every M,
and a later call with other M adds them to it.

``--driver host|device|both`` measures the solve under the interior-point driver on the host and / or on the device
(``solve_batch(driver=...)``) instead, into profiles/hopper_solve_device_driver.json -- or, with ``--newton
arrow --M 30,1000,10000``, per M into profiles/hopper_solve_large_m_device_driver.json (the training fields of ``--newton
arrow``; the file is rewritten after every M): the baseline from
``initial_guess()``, then the alphas as one batch from the HOST driver's baseline solution (both drivers solve the same
problems from the same starts); per run and driver the problems' iterations and factorizations, the wall clock of ``--solves``
solves after a warm-up (ms per batch, ms per lockstep iteration), the clocks' split of one more solve as it is (the time to
launch under the device driver) and of one with ``sync_clocks`` (a device-wide wait behind every block), and the
device-to-host copies (``Tensor.cpu()`` calls) per iteration.

``--repeats R`` measures the SAA grid over resampled terrains instead, into profiles/hopper_saa_grid.json: the
A alphas x R draws of the friction fields (``scp.draw_hopper_saa_fields``, seed 1) from the host driver's baseline solution,
solved as ONE ``solve_batch`` (one lockstep group of A R problems on their own fields) against the same problems repeat by
repeat, one ``solve_batch`` of A problems per draw -- what a list of such models executed while the fields were part of the
group key.  Per M of ``--M`` (a comma-separated list), ``--newton`` and driver (``--driver``, default both), in one process, a
warm-up solve each, then ``--solves`` timed solves each (median): the wall clock, the lockstep iterations (the batch: its
slowest member's; repeat by repeat: the sum over the draws of each draw's slowest), the largest and the median per-problem
iteration count, the status counts, and whether every (Z, info) of the batch is bitwise the repeat-by-repeat one.  The file is
rewritten after every measurement, and a later call with another M or newton adds to it.

``--chol {workgroup,grid,both}`` measures the solve under one or both Choleskys instead (csrc/chol.hip, one
workgroup per problem, or csrc/chol_grid.hip, one launch per panel over the whole device; the same bits), into
profiles/hopper_solve_chol_grid.json: under ``--driver`` (default device) and ``--newton``, per M of ``--M``, the baseline from
``initial_guess()`` and the alphas as one batch from the host driver's baseline solution -- or, with ``--repeats R``, the A R
problems of the SAA grid as ONE batch.  The methods run in one process, a warm-up solve each, then ``--solves`` timed solves each
(median, min, max), the per-iteration split of one more solve with ``sync_clocks`` (what is recorded today), and whether every
(Z, info) is bitwise the same under both.  The file is rewritten after every run, and a later call adds its runs to it.

``--driver`` also takes ``device_grid`` (the device driver with its own vector kernels spread over the rows) and
``all`` (host, device and device_grid; ``both`` stays host and device).

``--vec {workgroup,grid,both}`` measures the solve under one or both forms of the device driver's vector kernels instead
(driver='device' / 'device_grid': csrc/ipm_driver.hip, one workgroup per problem, or csrc/ipm_driver_grid.hip, a grid over the
rows; the same bits), into profiles/ipm_driver_grid.json: under ``--newton`` and ``--chol`` (one method, default workgroup), per
M of ``--M``, the baseline from ``initial_guess()`` and the alphas as one batch from the host driver's baseline solution -- or,
with ``--repeats R``, the A R problems of the SAA grid as ONE batch.  The forms run in one process, a warm-up solve each, then
``--solves`` timed solves each, ALTERNATING (median, min, max; ms per batch and per lockstep iteration); then one more solve per
form inside ``ipm.vector_clock()``, a device-wide wait around every call of the driver's own kernels: their share of the
iteration, their calls and their launches per iteration; and whether every (Z, info) is bitwise the same under both.  Every
run records its command line.  The file is rewritten after every run, and a later call adds its runs to it.

Prints one JSON line.  There is no CPU fallback: without a GPU nothing is measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


DRIVER_SETS = {"both": ("host", "device"), "all": ("host", "device", "device_grid")}


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


def arrow_split(clock, iters):
    wall = clock["wall"]
    parts = {"callbacks": clock.get("callbacks", 0.0), "reduction": clock.get("reduction", 0.0),
             "assembly": clock.get("normal", 0.0) + clock.get("assembly", 0.0), "factor": clock.get("factor", 0.0),
             "solves": clock.get("solve", 0.0), "products": clock.get("products", 0.0)}
    parts["host"] = wall - sum(parts.values())
    return {"wall_s": wall, "batch_iterations": iters, "seconds": parts,
            "ms_per_iteration": {k: 1e3 * v / max(iters, 1) for k, v in parts.items()}}


def script_fields(M_max):
    """-> (training fields (M_max, 30) x 3: the script's 30 then further draws, validation fields (10000, 30) x 3)"""
    from riskaversetrajopt_amd import hopper
    rng = np.random.RandomState(1)
    first = hopper.sample_friction_fields(30, rng)
    val = hopper.sample_friction_fields(10000, rng)
    more = hopper.sample_friction_fields(max(M_max - 30, 1), rng)
    return tuple(np.concatenate([a, b])[:M_max] for a, b in zip(first, more)), val


def run_arrow(M, newton, args, train, val_model, max_iter=3000):
    from riskaversetrajopt_amd import scp
    clocks = {}
    fields = tuple(f[:M] for f in train)
    out = scp.hopper_experiment(alphas=args.alphas, M=M, S=args.S, tol=1e-3, max_iter=max_iter, clocks=clocks, newton=newton,
                                fields=fields)

    def record(r, alpha):
        rec = problem_record(r, args.S)
        st = val_model.monte_carlo_statistics(*val_model.contact_inputs(r["Z"]), alpha=alpha if alpha else 0.5)
        rec["validation_safe_fraction"] = float(st["frac_satisfied"])
        if alpha:
            rec["validation_avar"] = float(st["cvar"])
        return rec
    base = record(out["base"], None)
    saa = {str(a): record(r, a) for a, r in zip(out["alphas"], out["results"])}
    split_of = arrow_split if newton == 'arrow' else split
    return {"baseline": base, "saa": saa, "wall_s": out["wall_s"], "baseline_split": split_of(clocks["base"], base["iterations"]),
            "saa_split": split_of(clocks["saa"], max([r["iterations"] for r in saa.values()] + [0]))}


def main_arrow(args):
    import torch
    from riskaversetrajopt_amd import hopper
    Ms = [int(m) for m in str(args.M).split(",")]
    train, val = script_fields(max(Ms))
    val_model = hopper.Model(10000, 'saa', 0.1, S=args.S, fields=val)
    out = {"device": torch.cuda.get_device_name(0), "S": args.S, "tol": 1e-3, "max_iter": 3000, "newton": "arrow",
           "validation_fields": 10000, "runs": {}}
    if args.out and os.path.exists(args.out):                        # a later call adds its M to the file of an earlier one
        with open(args.out) as f:
            old = json.loads(f.readline())
        if all(old.get(k) == out[k] for k in ("device", "S", "tol", "max_iter", "newton")):
            out["runs"] = old.get("runs", {})
    for M in Ms:
        run_arrow(M, 'arrow', args, train, val_model, max_iter=3)       # warm-up: library, maps, allocator
        rec = {"arrow": run_arrow(M, 'arrow', args, train, val_model)}
        if M == 30:
            run_arrow(M, 'dense', args, train, val_model, max_iter=3)
            rec["dense"] = run_arrow(M, 'dense', args, train, val_model)
        out["runs"][str(M)] = rec
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(out) + "\n")
        print("M = %d done: baseline %s, saa %s, wall %.2f s" % (M, rec["arrow"]["baseline"]["status"],
              [r["status"] for r in rec["arrow"]["saa"].values()], rec["arrow"]["wall_s"]), file=sys.stderr, flush=True)
    print(json.dumps(out))


def measure_drivers(models, Z0s, newton, drivers, solves, S):
    """one run (a batch of problems from fixed starts) under each driver -> its record in the profile"""
    import time

    import torch
    from riskaversetrajopt_amd import hopper_ipm, ipm
    rec = {}
    solve = lambda d, ck=None: hopper_ipm.solve_batch(models, Z0s, driver=d, clocks=ck, newton=newton)
    for d in drivers:
        solve(d)                                                     # warm-up: code objects, maps, allocator
        torch.cuda.synchronize()
        walls = []
        for _ in range(solves):
            t0 = time.perf_counter()
            sols = solve(d)
            walls.append(time.perf_counter() - t0)
        rounds = max(1, max(info["iterations"] for _, info in sols))
        launch = {}
        solve(d, launch)
        synced = {}
        ipm.DeviceBase.sync_clocks = True                            # one more solve, a device-wide wait behind every block
        try:
            solve(d, synced)
        finally:
            ipm.DeviceBase.sync_clocks = False
        copies, cpu = [0], torch.Tensor.cpu

        def counting(self, *a, **kw):
            copies[0] += 1
            return cpu(self, *a, **kw)
        torch.Tensor.cpu = counting
        try:
            solve(d)
        finally:
            torch.Tensor.cpu = cpu
        per_it = lambda ck: {k: 1e3 * v / rounds for k, v in ck.items()}
        rec[d] = {"wall_ms": [1e3 * w for w in walls], "median_ms_per_batch": 1e3 * float(np.median(walls)),
                  "lockstep_iterations": rounds, "median_ms_per_iteration": 1e3 * float(np.median(walls)) / rounds,
                  "problems": [{"method": m.method, "alpha": float(m.alpha), "status": info["status"],
                                "iterations": int(info["iterations"]), "factorizations": int(info["factorizations"]),
                                "E0": float(info["E0"]), "f": float(info["f"]), "x_S0": float(Z[8 * S])}
                               for m, (Z, info) in zip(models, sols)],
                  "split_ms_per_iteration": per_it(launch), "split_ms_per_iteration_sync_clocks": per_it(synced),
                  "device_to_host_copies_per_iteration": copies[0] / rounds}
    if "host" in rec and "device" in rec:
        rec["host_over_device"] = rec["host"]["median_ms_per_batch"] / rec["device"]["median_ms_per_batch"]
    if "device" in rec and "device_grid" in rec:
        rec["device_over_device_grid"] = rec["device"]["median_ms_per_batch"] / rec["device_grid"]["median_ms_per_batch"]
    return rec


def write_profile(out, path):
    line = json.dumps(out)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    return line


def driver_bench(args):
    """the script's two runs under the host and / or the device driver -> profiles/hopper_solve_device_driver.json, or with
    --newton arrow per M -> profiles/hopper_solve_large_m_device_driver.json"""
    import torch
    from riskaversetrajopt_amd import hopper, hopper_ipm, scp
    S, alphas, newton = args.S, [float(a) for a in args.alphas], args.newton
    drivers = DRIVER_SETS.get(args.driver, (args.driver,))
    out = {"device": torch.cuda.get_device_name(0), "S": S, "alphas": alphas, "tol": 1e-3, "max_iter": 3000, "newton": newton,
           "solves": args.solves, "saa_start": "the host driver's baseline solution", "runs": {}}

    def two_runs(M, fields):
        mk = lambda method, a: hopper.Model(M, method, a, S=S, fields=fields, precision='f64')
        base = mk('baseline', 0.1)
        (Zb, _), = hopper_ipm.solve_batch([base], newton=newton)     # the host driver's baseline: everyone's SAA start
        xs, us = base.convert_z_to_xs_us_mats(Zb)
        saa = [mk('saa', a) for a in alphas]
        runs = {"baseline": ([base], [base.initial_guess()]), "saa": (saa, [scp.hopper_saa_start(m, xs, us) for m in saa])}
        return {name: measure_drivers(models, Z0s, newton, drivers, args.solves, S) for name, (models, Z0s) in runs.items() if models}
    if newton == "arrow":                                            # the training fields of --newton arrow, per M
        Ms = [int(m) for m in str(args.M).split(",")]
        train, _ = script_fields(max(Ms))
        out["M"] = Ms
        for M in Ms:
            out["runs"][str(M)] = two_runs(M, tuple(f[:M] for f in train))
            write_profile(out, args.out)                             # rewritten after every M
            print("M = %d done" % M, file=sys.stderr, flush=True)
    else:
        out["M"] = int(args.M)
        out["runs"] = two_runs(out["M"], hopper.sample_friction_fields(out["M"], np.random.RandomState(1)))
    print(write_profile(out, args.out))


def grid_bench(args):
    """the alpha x repeat grid as one batch against repeat by repeat -> profiles/hopper_saa_grid.json"""
    import time

    import torch
    from riskaversetrajopt_amd import hopper, hopper_ipm, scp
    S, alphas, newton, R = args.S, [float(a) for a in args.alphas], args.newton, args.repeats
    drivers = ("device", "host") if args.driver in (None, "both") else ("device", "device_grid", "host") if args.driver == "all" \
        else (args.driver,)
    out = {"device": torch.cuda.get_device_name(0), "S": S, "alphas": alphas, "repeats": R, "tol": 1e-3, "max_iter": 3000,
           "seed": 1, "saa_start": "the host driver's baseline solution", "runs": {}}
    if args.out and os.path.exists(args.out):                        # a later call adds its runs to the file of an earlier one
        with open(args.out) as f:
            old = json.loads(f.readline())
        if all(old.get(k) == out[k] for k in ("device", "S", "alphas", "repeats", "tol", "max_iter", "seed")):
            out["runs"] = old.get("runs", {})

    def timed(call, warm):
        warm()
        torch.cuda.synchronize()
        walls = []
        for _ in range(args.solves):
            t0 = time.perf_counter()
            sols = call()
            walls.append(time.perf_counter() - t0)
        return sols, walls

    def same(r0, r1):
        (Z0, i0), (Z1, i1) = r0, r1
        return Z0.tobytes() == Z1.tobytes() and all(
            (i0[k].tobytes() == i1[k].tobytes()) if isinstance(i0[k], np.ndarray) else i0[k] == i1[k] for k in i0)
    for M in [int(m) for m in str(args.M).split(",")]:
        draws, _ = scp.draw_hopper_saa_fields(R, M, 1, seed=1)
        zero = np.zeros((M, hopper.num_mu_features))
        base = hopper.Model(M, 'baseline', S=S, fields=(zero, zero, zero), precision='f64')
        (Zb, ib), = hopper_ipm.solve_batch([base], newton=newton)
        xs, us = base.convert_z_to_xs_us_mats(Zb)
        models = [[hopper.Model(M, 'saa', a, S=S, fields=draws[r], precision='f64') for a in alphas] for r in range(R)]   # [repeat][alpha]
        starts = [[scp.hopper_saa_start(m, xs, us) for m in row] for row in models]
        flat_m, flat_z = [m for row in models for m in row], [z for row in starts for z in row]
        key = "M=%d,newton=%s" % (M, newton)
        rec = out["runs"].setdefault(key, {"baseline": {"status": ib["status"], "iterations": int(ib["iterations"])},
                                           "problems": len(flat_m), "stacked_fields_bytes": len(flat_m) * 3 * 30 * M * 8})
        for d in drivers:
            kw = dict(driver=d, newton=newton)
            batch = lambda: hopper_ipm.solve_batch(flat_m, flat_z, **kw)
            one = lambda r: hopper_ipm.solve_batch(models[r], starts[r], **kw)
            sols_b, walls_b = timed(batch, batch)
            sols_r, walls_r = timed(lambda: [sol for r in range(R) for sol in one(r)], lambda: one(0))
            its = np.array([info["iterations"] for _, info in sols_b])
            its_r = np.array([info["iterations"] for _, info in sols_r]).reshape(R, len(alphas))
            status = {}
            for _, info in sols_b:
                status[info["status"]] = status.get(info["status"], 0) + 1
            med_b, med_r = float(np.median(walls_b)), float(np.median(walls_r))
            rec[d] = {"solves": args.solves, "one_batch": {"wall_ms": [1e3 * w for w in walls_b], "median_ms": 1e3 * med_b, "lockstep_iterations": int(its.max()),
                                    "median_ms_per_lockstep_iteration": 1e3 * med_b / max(int(its.max()), 1)},
                      "repeat_by_repeat": {"wall_ms": [1e3 * w for w in walls_r], "median_ms": 1e3 * med_r,
                                           "lockstep_iterations": int(its_r.max(axis=1).sum()),
                                           "median_ms_per_lockstep_iteration": 1e3 * med_r / max(int(its_r.max(axis=1).sum()), 1)},
                      "repeat_by_repeat_over_one_batch": med_r / med_b,
                      "iterations_per_problem": {"largest": int(its.max()), "median": float(np.median(its)),
                                                 "slowest": {"alpha": float(flat_m[int(its.argmax())].alpha),
                                                             "repeat": int(its.argmax()) // len(alphas)}},
                      "status": status, "batch_is_bitwise_repeat_by_repeat": all(same(a, b) for a, b in zip(sols_b, sols_r))}
            write_profile(out, args.out)
            print("%s driver=%s done: one batch %.0f ms, repeat by repeat %.0f ms" % (key, d, 1e3 * med_b, 1e3 * med_r),
                  file=sys.stderr, flush=True)
    print(write_profile(out, args.out))


def runs_of(args, key_format):
    """the runs --chol and --vec measure, per M of --M: (name, models, starts) of the baseline from ``initial_guess()`` and of the
    alphas as one batch from the host driver's baseline solution -- or, with --repeats R, of the A R problems of the SAA grid as ONE
    batch.  ``key_format`` % (M, newton) names them."""
    from riskaversetrajopt_amd import hopper, hopper_ipm, scp
    S, alphas, newton, R = args.S, [float(a) for a in args.alphas], args.newton, args.repeats
    for M in [int(m) for m in str(args.M).split(",")]:
        mk = lambda method, a, fields: hopper.Model(M, method, a, S=S, fields=fields, precision='f64')
        key = key_format % (M, newton)
        if R is not None:
            draws, _ = scp.draw_hopper_saa_fields(R, M, 1, seed=1)
            zero = np.zeros((M, hopper.num_mu_features))
            base = mk('baseline', 0.1, (zero, zero, zero))
            (Zb, _), = hopper_ipm.solve_batch([base], newton=newton)
            xs, us = base.convert_z_to_xs_us_mats(Zb)
            models = [mk('saa', a, draws[r]) for r in range(R) for a in alphas]
            yield key + ",repeats=%d" % R, models, [scp.hopper_saa_start(m, xs, us) for m in models]
            continue
        fields = tuple(f[:M] for f in script_fields(M)[0]) if newton == "arrow" else \
            hopper.sample_friction_fields(M, np.random.RandomState(1))
        base = mk('baseline', 0.1, fields)
        (Zb, _), = hopper_ipm.solve_batch([base], newton=newton)
        xs, us = base.convert_z_to_xs_us_mats(Zb)
        saa = [mk('saa', a, fields) for a in alphas]
        yield key + ",baseline", [base], [base.initial_guess()]
        if saa:
            yield key + ",saa", saa, [scp.hopper_saa_start(m, xs, us) for m in saa]


def same_solution(r0, r1, but=()):
    (Z0, i0), (Z1, i1) = r0, r1
    eq = lambda a, b: a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b
    return Z0.tobytes() == Z1.tobytes() and set(i0) == set(i1) and all(eq(i0[k], i1[k]) for k in i0 if k not in but)


def vec_bench(args):
    """runs under one or both forms of the device driver's vector kernels -> profiles/ipm_driver_grid.json"""
    import time

    import torch
    from riskaversetrajopt_amd import _lib, hopper_ipm, ipm
    chol = args.chol or "workgroup"
    forms = ("workgroup", "grid") if args.vec == "both" else (args.vec,)
    driver_of = {v: d for d, v in ipm.VEC_OF_DRIVER.items()}
    out = {"device": torch.cuda.get_device_name(0), "S": args.S, "tol": 1e-3, "max_iter": 3000, "solves": args.solves,
           "rows_per_workgroup": int(_lib.load().rato_ipm_grid_rows()),
           "saa_start": "the host driver's baseline solution", "runs": {}}
    if args.out and os.path.exists(args.out):                        # a later call adds its runs to the file of an earlier one
        with open(args.out) as f:
            old = json.loads(f.readline())
        if all(old.get(k) == out[k] for k in ("device", "S", "tol", "max_iter", "solves")):
            out["runs"] = old.get("runs", {})

    def measure(models, Z0s):
        solve = lambda v, ck=None: hopper_ipm.solve_batch(models, Z0s, driver=driver_of[v], clocks=ck, newton=args.newton, chol=chol)
        st = hopper_ipm.structure(models[0])
        rec = {"command": "python tools/hopper_solve_bench.py " + " ".join(sys.argv[1:]), "problems": len(models),
               "alphas": sorted({float(m.alpha) for m in models if m.method == 'saa'}), "n": int(st["n"]), "m": int(st["ncon"])}
        sols, walls = {}, {v: [] for v in forms}
        for v in forms:
            solve(v)                                                 # warm-up of this form: code objects, maps, allocator
        torch.cuda.synchronize()
        for _ in range(args.solves):                                 # alternating: a drift of the board meets both forms
            for v in forms:
                t0 = time.perf_counter()
                sols[v] = solve(v)
                walls[v].append(time.perf_counter() - t0)
        for v in forms:
            rounds = max(1, max(info["iterations"] for _, info in sols[v]))
            with ipm.vector_clock() as own:                          # one more solve, a device-wide wait around the driver's kernels
                t0 = time.perf_counter()
                solve(v)
                waited = time.perf_counter() - t0
            synced = {}
            ipm.DeviceBase.sync_clocks = True                        # and one with a device-wide wait behind every block
            try:
                solve(v, synced)
            finally:
                ipm.DeviceBase.sync_clocks = False
            status = {}
            for _, info in sols[v]:
                status[info["status"]] = status.get(info["status"], 0) + 1
            w = walls[v]
            rec[v] = {"driver": driver_of[v], "wall_ms": [1e3 * x for x in w], "median_ms_per_batch": 1e3 * float(np.median(w)),
                      "min_ms_per_batch": 1e3 * min(w), "max_ms_per_batch": 1e3 * max(w), "lockstep_iterations": rounds,
                      "median_ms_per_iteration": 1e3 * float(np.median(w)) / rounds, "status": status,
                      "factorizations": int(sum(info["factorizations"] for _, info in sols[v])),
                      "driver_kernels_ms_per_iteration_waited": 1e3 * own["seconds"] / rounds,
                      "driver_calls_per_iteration": own["calls"] / rounds, "driver_launches_per_iteration": own["launches"] / rounds,
                      "waited_solve_ms_per_iteration": 1e3 * waited / rounds,
                      "split_ms_per_iteration_sync_clocks": {k: 1e3 * x / rounds for k, x in synced.items()}}
        if len(forms) == 2:
            w, g = rec["workgroup"], rec["grid"]
            rec["grid_is_bitwise_workgroup"] = all(same_solution(a, b, but=("driver",)) for a, b in zip(sols["grid"], sols["workgroup"]))
            rec["workgroup_over_grid"] = w["median_ms_per_batch"] / g["median_ms_per_batch"]
            rec["grid_wins"] = g["max_ms_per_batch"] < w["min_ms_per_batch"]
            rec["grid_loses"] = g["min_ms_per_batch"] > w["max_ms_per_batch"]
        return rec
    for name, models, Z0s in runs_of(args, "M=%d,newton=%s,chol=" + chol):
        out["runs"][name] = measure(models, Z0s)
        write_profile(out, args.out)
        print("%s done" % name, file=sys.stderr, flush=True)
    print(write_profile(out, args.out))


def chol_bench(args):
    """runs under one or both Choleskys -> profiles/hopper_solve_chol_grid.json"""
    import time

    import torch
    from riskaversetrajopt_amd import hopper_ipm, ipm
    S, newton = args.S, args.newton
    driver = "device" if args.driver in (None, "both", "all") else args.driver
    methods = ("workgroup", "grid") if args.chol == "both" else (args.chol,)
    out = {"device": torch.cuda.get_device_name(0), "S": S, "tol": 1e-3, "max_iter": 3000, "solves": args.solves,
           "saa_start": "the host driver's baseline solution", "runs": {}}
    if args.out and os.path.exists(args.out):                        # a later call adds its runs to the file of an earlier one
        with open(args.out) as f:
            old = json.loads(f.readline())
        if all(old.get(k) == out[k] for k in ("device", "S", "tol", "max_iter", "solves")):
            out["runs"] = old.get("runs", {})

    def same(r0, r1):
        (Z0, i0), (Z1, i1) = r0, r1
        eq = lambda a, b: a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b
        return Z0.tobytes() == Z1.tobytes() and set(i0) == set(i1) and all(eq(i0[k], i1[k]) for k in i0)

    def measure(models, Z0s):
        solve = lambda c, ck=None: hopper_ipm.solve_batch(models, Z0s, driver=driver, clocks=ck, newton=newton, chol=c)
        rec, sols = {"problems": len(models), "alphas": sorted({float(m.alpha) for m in models if m.method == 'saa'})}, {}
        for c in methods:
            solve(c)                                                 # warm-up of this method: code objects, maps, allocator
        torch.cuda.synchronize()
        for c in methods:
            walls = []
            for _ in range(args.solves):
                t0 = time.perf_counter()
                sols[c] = solve(c)
                walls.append(time.perf_counter() - t0)
            rounds = max(1, max(info["iterations"] for _, info in sols[c]))
            synced = {}
            ipm.DeviceBase.sync_clocks = True                        # one more solve, a device-wide wait behind every block
            try:
                solve(c, synced)
            finally:
                ipm.DeviceBase.sync_clocks = False
            status = {}
            for _, info in sols[c]:
                status[info["status"]] = status.get(info["status"], 0) + 1
            rec[c] = {"wall_ms": [1e3 * w for w in walls], "median_ms_per_batch": 1e3 * float(np.median(walls)),
                      "min_ms_per_batch": 1e3 * min(walls), "max_ms_per_batch": 1e3 * max(walls), "lockstep_iterations": rounds,
                      "median_ms_per_iteration": 1e3 * float(np.median(walls)) / rounds, "status": status,
                      "factorizations": int(sum(info["factorizations"] for _, info in sols[c])),
                      "split_ms_per_iteration_sync_clocks": {k: 1e3 * v / rounds for k, v in synced.items()}}
        if len(methods) == 2:
            w, g = rec["workgroup"], rec["grid"]
            rec["grid_is_bitwise_workgroup"] = all(same(a, b) for a, b in zip(sols["grid"], sols["workgroup"]))
            rec["workgroup_over_grid"] = w["median_ms_per_batch"] / g["median_ms_per_batch"]
            rec["grid_wins"] = g["max_ms_per_batch"] < w["min_ms_per_batch"]
            rec["grid_loses"] = g["min_ms_per_batch"] > w["max_ms_per_batch"]
        return rec
    for name, models, Z0s in runs_of(args, "M=%d,newton=%s,driver=" + driver):
        out["runs"][name] = measure(models, Z0s)
        write_profile(out, args.out)
        print("%s done" % name, file=sys.stderr, flush=True)
    print(write_profile(out, args.out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=30)
    ap.add_argument("--M", default="30", help="with --newton arrow: a comma-separated list")
    ap.add_argument("--newton", choices=("dense", "arrow"), default="dense")
    ap.add_argument("--alphas", type=float, nargs="*", default=[0.05, 0.1, 0.2, 0.3, 0.5, 0.75])
    ap.add_argument("--out", default=None)
    ap.add_argument("--driver", choices=("host", "device", "device_grid", "both", "all"), default=None,
                    help="measure the solve (either --newton) under the interior-point driver(s) instead; both: host and "
                         "device, all: host, device and device_grid")
    ap.add_argument("--vec", choices=("workgroup", "grid", "both"), default=None,
                    help="measure the solve under the form(s) of the device driver's vector kernels instead (--newton; --chol, one "
                         "method; --repeats)")
    ap.add_argument("--solves", type=int, default=5, help="with --driver or --repeats: timed solves per run and driver")
    ap.add_argument("--repeats", type=int, default=None,
                    help="measure the grid of alphas x this many draws of the fields as one batch against repeat by repeat instead")
    ap.add_argument("--chol", choices=("workgroup", "grid", "both"), default=None,
                    help="measure the solve under the Cholesky method(s) instead (--driver, default device; --newton; --repeats)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hopper_solve_bench needs a GPU: nothing here is measured on the host in its place")
    if args.vec is not None:
        if args.chol == "both" or args.driver is not None:
            raise SystemExit("--vec compares driver='device' and 'device_grid' under ONE Cholesky: --chol workgroup or grid, no --driver")
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "ipm_driver_grid.json")
        if args.repeats is not None and args.repeats < 1:
            raise SystemExit("--repeats needs at least one draw")
        return vec_bench(args)
    if args.chol is not None:
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "hopper_solve_chol_grid.json")
        if args.repeats is not None and args.repeats < 1:
            raise SystemExit("--repeats needs at least one draw")
        return chol_bench(args)
    if args.out is None and args.repeats is not None:
        args.out = os.path.join(ROOT, "profiles", "hopper_saa_grid.json")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "hopper_solve_large_m_device_driver.json"
                                if args.driver is not None and args.newton == "arrow" else
                                "hopper_solve_device_driver.json" if args.driver is not None else
                                "hopper_solve_large_m.json" if args.newton == "arrow" else "hopper_solve.json")
    if args.repeats is not None:
        if args.repeats < 1:
            raise SystemExit("--repeats needs at least one draw")
        return grid_bench(args)
    if args.driver is not None:
        return driver_bench(args)
    if args.newton == "arrow":
        return main_arrow(args)
    args.M = int(args.M)
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
