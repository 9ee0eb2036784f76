"""Measures the hopper's fp64 slip path (csrc/hopper_slip64.hip) on the GPU (nothing gates on it; bench.py is the flagship
benchmark):

  * per-call device time of rato_hopper_slip_f64 with multipliers (the slip kernel and the second stage of its sums) and
    without, of rato_hopper_slip_hess_blocks_f64, and of the whole risk group of ``Model.nlp_device`` (kernel, emission,
    Hessian share) at S = M = 30 for K = 1 and K = 6, and of the slip call at M = 5e4, C = 40 (S = 60), K = 1: device events
    around 200 back-to-back calls after a warm-up, the median of 7 rounds;
  * the fp32 path on the same inputs: the kernel call alone (rato_hopper_slip_hessian, inputs by value, per problem) on device
    events, and what a solver's callback pays for it -- the host gather of px / forces / chain, the call and the read-back --
    on the host clock, per problem;
  * the NumPy fp64 restatement (oracle/hopper.py: slip_partials, slip_hessian_sums) on the same inputs, on the host clock.

    python tools/hopper_slip_f64_bench.py [--out profiles/hopper_slip_f64_bench.json]

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


def host_clock(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hopper_slip_f64_bench.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hopper_slip_f64_bench needs a GPU: nothing here is measured on the host in its place")
    import _hopper_nlp as R
    from oracle import hopper as oh
    from riskaversetrajopt_amd import hopper

    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "sizes": {}}
    for S, M, Ks in ((30, 30, (1, 6)), (60, 50000, (1,))):
        fields = oh.sample_friction_fields(np.random.RandomState(1), M)
        m64 = hopper.Model(M, 'saa', 0.2, S=S, fields=fields, precision='f64')
        m32 = hopper.Model(M, 'saa', 0.2, S=S, fields=fields)
        ncon, r0 = m64.risk_rows_offset()
        Cn = m64.time_jump + S - m64.time_land
        o = oh.Model(*fields, method='saa', alpha=0.2, S=S)
        for K in Ks:
            rec = {}
            Zs = np.stack([R.problem(S, M, k) for k in range(K)])
            lams = np.random.RandomState(3).uniform(-1, 1, (K, ncon))
            Zd, lamd = torch.as_tensor(Zs, device=m64.device), torch.as_tensor(lams, device=m64.device)
            reps = args.reps if M <= 1000 else max(args.reps // 10, 10)
            rec["slip_f64_with_lam"] = time_call(lambda: m64.slip_device_f64(Zd, lamd, want=("h", "dh_dfz", "dh_dx")), reps, args.rounds)
            rec["slip_f64_without_lam"] = time_call(lambda: m64.slip_device_f64(Zd, None, want=("h", "dh_dfz", "dh_dx")), reps, args.rounds)
            D = m64.slip_device_f64(Zd, lamd, want=())["D"]
            add = torch.zeros((K, S + 1, 78), dtype=torch.float64, device=m64.device)
            rec["slip_hess_blocks_f64"] = time_call(lambda: m64.slip_hess_blocks_device_f64(Zd, D, add), reps, args.rounds)
            lam_s = [lams[k, r0:r0 + M * Cn].reshape(M, Cn) for k in range(K)]
            gathered = [m32.contact_inputs(Zs[k]) for k in range(K)]

            def f32_kernels():
                for k in range(K):
                    m32.slip_hessian_sums3(*gathered[k], lam_s[k])       # one launch per problem (+ the second stage, read-back)
            rec["slip_f32_hessian_call_host_clock_us"] = host_clock(f32_kernels, max(reps // 4, 5))
            if M <= 1000:
                rec["risk_group_of_nlp_device_f64"] = time_call(lambda: (m64._slip_f64(Zd, lamd), m64.slip_hess_blocks_device_f64(Zd, D, add)),
                                                                reps, args.rounds)
                rec["nlp_device_f64_host_clock_us"] = host_clock(lambda: m64.nlp_device(Zd, lamd), 50)
                rec["nlp_device_f32_host_clock_us"] = host_clock(lambda: m32.nlp_device(Zd, lamd), 50)

                def f32_callbacks():
                    for k in range(K):
                        m32.slip_risk_constraints(Zs[k])
                        m32.slip_jacobian_device(Zs[k])
                        m32.slip_hessian_blocks(Zs[k], lams[k])
                rec["risk_group_f32_facade_host_clock_us"] = host_clock(f32_callbacks, 20)
                rec["risk_group_f64_facade_host_clock_us"] = host_clock(
                    lambda: (m64._slip_f64(Zd, lamd), m64.slip_hess_blocks_device_f64(Zd, D, add)), 50)
            t0 = time.perf_counter()
            for k in range(K):
                px, forces = o.contact_inputs(Zs[k])
                o.slip_partials(px, forces)
                o.slip_hessian_sums(px, forces, lam_s[k])
            rec["numpy_fp64_restatement_s"] = time.perf_counter() - t0
            out["sizes"][f"S{S}_M{M}_C{Cn}_K{K}"] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
