"""Measures the hopper NLP kernels on the GPU (nothing gates on it; bench.py is the flagship benchmark):

  * per-call device time of the linearize call (rato_hopper_nlp_linearize), the Hessian call (rato_hopper_nlp_hessian) and
    the emission (the three rato_scatter_f64 calls with their two template copies) at the script's size S = 30, M = 30, for
    K = 1 and K = 6 (the script's six alphas): device events around `reps` back-to-back calls after a warm-up, repeated
    `rounds` times -> median and spread per call;
  * the whole ``Model.nlp_device`` call (uploads and multiplier folding included) on the host clock;
  * the same quantities on the host by the fp64 NumPy restatement (tests/_hopper_nlp.py), K = 1;
  * the largest scaled difference between the kernels and the restatement over the shapes of the GPU test
    (tests/test_gpu_hopper_nlp.py), the Hessian per block, which sets that test's tolerance.

    python tools/hopper_nlp_bench.py [--out profiles/hopper_nlp_bench.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hopper_nlp_bench needs a GPU: nothing here is measured on the host in its place")
    import _hopper_nlp as R
    from riskaversetrajopt_amd import hopper

    S, M = 30, 30
    out = {"device": torch.cuda.get_device_name(0), "S": S, "M": M, "linearize": {}, "hessian": {}, "emission": {},
           "nlp_device_host_clock_us": {}, "host_restatement_s": {}}
    m = hopper.Model(M, 'saa', 0.2, S=S, rng=np.random.RandomState(1))
    ncon = m.nlp_layout()["ncon"]
    for K in (1, 6):
        Zs = np.stack([R.problem(S, M, k) for k in range(K)])
        lams = np.random.RandomState(3).uniform(-1, 1, (K, ncon))
        Zd = torch.as_tensor(Zs, device=m.device)
        lam_dyn, lam_rows = (torch.as_tensor(a, device=m.device) for a in m.fold_multipliers(lams))
        p = m._slip_params()
        lin = hopper.nlp_linearize_device(p, Zd)
        blocks = hopper.nlp_hessian_device(p, Zd, lam_dyn, lam_rows)

        def emit():                                                  # the two stages of the emission, their templates made once
            m.det_jacobian_values(lin, K)
            m.hess_tril_device(blocks)
        out["linearize"][f"K{K}"] = time_call(lambda: hopper.nlp_linearize_device(p, Zd), args.reps, args.rounds)
        out["hessian"][f"K{K}"] = time_call(lambda: hopper.nlp_hessian_device(p, Zd, lam_dyn, lam_rows), args.reps, args.rounds)
        out["emission"][f"K{K}"] = time_call(emit, args.reps, args.rounds)
        m.nlp_device(Zs, lams)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            m.nlp_device(Zs, lams)
        torch.cuda.synchronize()
        out["nlp_device_host_clock_us"][f"K{K}"] = (time.perf_counter() - t0) * 1e6 / args.reps
    Z, lam = R.problem(S, M, 0), np.random.RandomState(3).uniform(-1, 1, ncon)
    t0 = time.perf_counter()
    loc = R.local(Z, S)
    out["host_restatement_s"]["linearize_K1"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.blocks_of(loc, *R.fold_lam(lam, S, M, m.time_jump, m.time_land, 'saa'))
    out["host_restatement_s"]["hessian_blocks_K1"] = time.perf_counter() - t0

    worst = {}
    for S in (1, 2, 3, 6, 30, 65):
        m = hopper.Model(2, 'saa', 0.2, S=S, rng=np.random.RandomState(1))
        K = 3
        Zs = np.stack([R.problem(S, 2, k) for k in range(K)])
        lams = np.random.RandomState(50 + S).uniform(-1, 1, (K, m.nlp_layout()["ncon"]))
        r = m.nlp_device(Zs, lams)
        for k in range(K):
            loc = R.local(Zs[k], S)
            ref = R.tril78(R.blocks_of(loc, *R.fold_lam(lams[k], S, 2, m.time_jump, m.time_land, 'saa')))
            for name in ("defect", "d_defect", "rows", "d_rows"):
                worst[name] = max(worst.get(name, 0.0), R.rel_err(r[name][k].cpu().numpy(), loc[name]))
            worst["hess_blocks"] = max(worst.get("hess_blocks", 0.0),
                                       R.rel_err_blocks(r["hess_blocks"][k].cpu().numpy(), ref, 1))
    out["kernel_vs_restatement_max_scaled_difference"] = worst
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
