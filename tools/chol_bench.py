"""Times the two batched Choleskys on the same inputs in one process (nothing gates on it; bench.py is the flagship benchmark):
``ipm.chol_factor`` / ``chol_solve`` with method='workgroup' (csrc/chol.hip, one workgroup per problem) and method='grid'
(csrc/chol_grid.hip, a stream-ordered sequence of launches over the whole device; the same bits).

    python tools/chol_bench.py [--out profiles/chol_grid.json] [--n 60,370,400,730] [--K 1,6,120] [--launches 30]

Per (n, K), nrhs = 1: K SPD matrices (B B' + I, uniform B) and right-hand sides; every shape and both methods are warmed up
first; then ``--launches`` (at least 20) timed launches per method, the two methods ALTERNATING, each between a pair of device
events on the current stream (the factor on a fresh copy of the input made before the first event).  Recorded: median, min and
max in microseconds per method, for the factor and for the solve; the launches one grid factorization takes; whether the grid
form's factor and solution are bitwise the workgroup form's; and ``grid_wins``: the grid form's MAX below the workgroup form's
MIN (the gain exceeds the spread of the repeated launches), ``grid_loses`` the reverse, otherwise neither.

Prints one JSON line.  There is no CPU fallback: without a GPU nothing is measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = ("workgroup", "grid")


def grid_launches(n, nb=32):
    """launches of one rato_chol_factor_grid_batch_f64 call: one per panel"""
    return (n + nb - 1) // nb


def stats(us):
    return {"median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us))}


def verdict(rec):
    w, g = rec["workgroup"], rec["grid"]
    return {"grid_over_workgroup_median": g["median_us"] / w["median_us"], "grid_wins": g["max_us"] < w["min_us"],
            "grid_loses": g["min_us"] > w["max_us"]}


def measure(n, K, launches, dev):
    import torch
    from riskaversetrajopt_amd import ipm
    rng = np.random.RandomState(1000 * n + K)
    B = rng.uniform(-1, 1, (n, n))
    A = B @ B.T + np.eye(n)
    A0 = torch.as_tensor(np.stack([A + k * np.eye(n) for k in range(K)]), device=dev).contiguous()
    b0 = torch.as_tensor(rng.uniform(-1, 1, (K, 1, n)), device=dev).contiguous()
    work = ipm.chol_grid_work(n, K, dev)
    kw = {"workgroup": {}, "grid": {"work": work}}
    L, X = {}, {}
    for m in METHODS:                                                 # warm-up of this shape, and the factors the solves use
        L[m] = A0.clone()
        info = ipm.chol_factor(L[m], method=m, **kw[m])
        assert info.cpu().tolist() == [0] * K
        X[m] = ipm.chol_solve(L[m], b0.clone(), method=m)
    torch.cuda.synchronize()
    bitwise = {"factor": L["grid"].cpu().numpy().tobytes() == L["workgroup"].cpu().numpy().tobytes(),
               "solve": X["grid"].cpu().numpy().tobytes() == X["workgroup"].cpu().numpy().tobytes()}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_factor, t_solve = {m: [] for m in METHODS}, {m: [] for m in METHODS}
    for _ in range(launches):
        for m in METHODS:                                             # the two methods alternate
            a, x = A0.clone(), b0.clone()
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            ipm.chol_factor(a, method=m, **kw[m])
            e1.record()
            ipm.chol_solve(L[m], x, method=m)
            e2.record()
            e2.synchronize()
            t_factor[m].append(1e3 * e0.elapsed_time(e1))
            t_solve[m].append(1e3 * e1.elapsed_time(e2))
    rec = {"n": n, "K": K, "nrhs": 1, "launches_timed": launches, "grid_launches_per_factorization": grid_launches(n),
           "grid_is_bitwise_workgroup": bitwise,
           "factor": {m: stats(t_factor[m]) for m in METHODS}, "solve": {m: stats(t_solve[m]) for m in METHODS}}
    rec["factor"].update(verdict(rec["factor"]))
    rec["solve"].update(verdict(rec["solve"]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="60,370,400,730", help="sizes (730: the hopper's dense n at S = 60)")
    ap.add_argument("--K", default="1,6,120", help="batch sizes")
    ap.add_argument("--launches", type=int, default=30, help="timed launches per method and shape (at least 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chol_grid.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chol_bench needs a GPU: nothing here is measured on the host in its place")
    if args.launches < 20:
        raise SystemExit("--launches: at least 20")
    dev = torch.device("cuda:0")
    ns, Ks = [int(v) for v in args.n.split(",")], [int(v) for v in args.K.split(",")]
    for n in ns:                                                     # every shape once before anything is timed
        for K in Ks:
            measure(n, K, 20, dev)
    out = {"device": torch.cuda.get_device_name(0), "timing": "device events around each call, methods alternating",
           "shapes": [measure(n, K, args.launches, dev) for n in ns for K in Ks]}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
