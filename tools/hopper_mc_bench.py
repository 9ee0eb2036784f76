"""Measures the hopper's Monte-Carlo validation of K solutions on M_mc validation fields on the GPU (nothing gates on it;
bench.py is the flagship benchmark): ONE ``Model.eval_batch_device`` call and one read-back of the K records
(rato_hopper_eval_batch) against the per-solution loop it replaces (``Model.monte_carlo_statistics`` per solution: one slip
launch, one selection launch and one blocking read-back each).

  * Cases: K = 7 (the script's six alphas and the baseline) and K = 120 at M_mc = 10 000, S = 30 (20 contact steps).  The
    solutions are synthetic trajectories at the hopper's scale: neither path's time depends on the values.
  * Both paths run in the same process, alternating, after a warm-up of both; every clock is read behind a device
    synchronise; per case the median, minimum and maximum over the rounds of the host time of one whole validation.
  * The two paths' records are compared to the bit before anything is timed.
  * The ideal trig issue time of the batched kernel (K M C 30 hardware cosines at a quarter of the VALU rate, the measure of
    DESIGN §4.4) is written beside the times; the kernel time itself comes from a profiler run of its own:

        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/hopper_mc_bench.py --kernel-only

    python tools/hopper_mc_bench.py [--out profiles/hopper_mc_batch.json] [--kernel-trace <dir>/..._kernel_trace.csv]

``--kernel-trace``: the profiler's per-dispatch file of such a run; the batched kernel's dispatches are matched to the cases by
their grid and their durations (and scratch size) are written into the result.
Prints one JSON line.  There is no CPU fallback: without a GPU nothing is measured.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRIG_PER_S = 1.2e8 / 12.2e-6        # 1.2e8 quarter-rate transcendentals issue in 12.2 us on the whole chip


def solutions(S, K, seed=5):
    """K synthetic NLP vectors (states and controls only) at the hopper's scale"""
    rng = np.random.RandomState(seed)
    Zs = []
    for k in range(K):
        xs = np.zeros((S + 1, 8))
        xs[:, 0] = np.linspace(0, 0.05 + 0.2 * rng.rand(), S + 1)
        xs[:, 1] = 1.0
        xs[:, 2] = 0.2 * np.sin(np.linspace(0, 3, S + 1) + rng.rand())
        xs[:, 3] = 0.9 + 0.1 * np.cos(np.linspace(0, 2, S + 1))
        us = np.zeros((S, 4))
        us[:, 3] = 32.0 + rng.randn(S)
        us[:, 2] = 0.08 * us[:, 3] + 0.3 * rng.randn(S)
        Zs.append(np.concatenate([xs.reshape(-1), us.reshape(-1)]))
    return Zs


def kernel_dispatches(path):
    """the batched kernel's dispatches in a rocprofv3 kernel-trace file -> {(grid_x, grid_y) in threads: [(us, scratch bytes)]}"""
    found = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "hopper_eval_batch_kernel" not in row.get("Kernel_Name", ""):
                continue
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3
            found.setdefault((int(row["Grid_Size_X"]), int(row["Grid_Size_Y"])), []).append((us, int(row.get("Scratch_Size", 0) or 0)))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M-mc", type=int, default=10000)
    ap.add_argument("--S", type=int, default=30)
    ap.add_argument("--Ks", type=int, nargs="+", default=[7, 120])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--kernel-only", action="store_true", help="a few batched calls and nothing else: the profiler's run")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hopper_mc_batch.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hopper_mc_bench needs a GPU: nothing here is measured on the host in its place")
    from riskaversetrajopt_amd import hopper, stats

    S, M = args.S, args.M_mc
    mc = hopper.Model(M, 'saa', S=S, fields=hopper.sample_friction_fields(M, np.random.RandomState(1)))
    names = stats._STAT_NAMES
    out = {"device": torch.cuda.get_device_name(0), "M_mc": M, "S": S, "rounds": args.rounds, "cases": {}}
    for K in args.Ks:
        alphas = [(0.05, 0.1, 0.2, 0.3, 0.5, 0.75)[k * 6 // K] for k in range(K)]       # alpha-major runs, as the grid study stacks them
        px, forces = mc.contact_inputs_batch(solutions(S, K))
        Cn = px.shape[1]
        bufs = {}

        def batched():
            _, rec = mc.eval_batch_device(px, forces, alphas=alphas, out=bufs)
            return rec.cpu().numpy()

        def loop():
            return [mc.monte_carlo_statistics(px[k], forces[k], alpha=alphas[k]) for k in range(K)]

        if args.kernel_only:
            for _ in range(5):
                batched()
            torch.cuda.synchronize()
            continue
        rec, sts = batched(), loop()
        for k in range(K):
            one = np.array([sts[k][n] for n in names])
            assert rec[k].tobytes() == one.tobytes(), ("the two paths differ", K, k)
        for _ in range(3):
            batched(), loop()
        t_b, t_l = [], []
        for _ in range(args.rounds):
            for fn, acc in ((batched, t_b), (loop, t_l)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append(time.perf_counter() - t0)
        summ = lambda t: {"median_ms": float(np.median(t) * 1e3), "min_ms": float(np.min(t) * 1e3), "max_ms": float(np.max(t) * 1e3)}
        nw, kc, gx, gy = mc.eval_batch_plan(Cn, K)
        case = {"C": Cn, "plan": {"nw_log2": nw, "k_chunk": kc, "grid_x": gx, "grid_y": gy},
                "batched": summ(t_b), "per_solution_loop": summ(t_l),
                "loop_over_batched": float(np.median(t_l) / np.median(t_b)),
                "cosines": K * M * Cn * hopper.num_mu_features,
                "ideal_trig_issue_us": K * M * Cn * hopper.num_mu_features / TRIG_PER_S * 1e6,
                "records_bitwise_equal": True}
        out["cases"][f"K{K}"] = case
    if args.kernel_only:
        print(json.dumps({"kernel_only": True, "Ks": args.Ks}))
        return
    if args.kernel_trace:
        found = kernel_dispatches(args.kernel_trace)
        for case in out["cases"].values():
            rows = found.get((case["plan"]["grid_x"] * 256, case["plan"]["grid_y"]), [])
            if rows:
                us = np.array([r[0] for r in rows])
                case["kernel"] = {"calls": len(rows), "median_us": float(np.median(us)), "min_us": float(us.min()),
                                  "max_us": float(us.max()), "scratch_bytes": max(r[1] for r in rows),
                                  "ideal_over_median": float(case["ideal_trig_issue_us"] / np.median(us))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
