"""SCP outer loop and the reference's timing protocol.

Mirrors the script-level driver of the reference (``drone_risk.py:495-540``,
``driving.py:467-529``, ``drone_times.py:509-550``): warm-up iterations, restart
from the initial guess, a FIXED number of iterations (no convergence test),
per-iteration wall-clock of "define" (linearize + assemble) and "solve" (host
QP) with cumulative times, and the L2 change of the controls."""
import os
import time

import numpy as np


def L2_error_us(us_mat, us_mat_prev):
    """drone_risk.py:471-476, driving.py:459-464 (both Model modules carry it under this name)."""
    error = np.mean(np.linalg.norm(us_mat - us_mat_prev, axis=-1))
    return error / np.mean(np.linalg.norm(us_mat, axis=-1))


def _sync():
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    except Exception:
        pass


def _finite_guard(model, check_finite):
    """Failure detection: every linearization of the run is scanned for NaN/Inf and a non-finite output raises
    ``RatoNonFiniteError`` (RATO_ENONFINITE) instead of the reference's print-and-continue (drone_risk.py:458-459)."""
    if check_finite is not None and hasattr(model, "check_finite"):
        model.check_finite = bool(check_finite)


def run_drone(model, num_scp_iters_max=60, warmup_iters=5, verbose=False, check_finite=True):
    """drone_risk.py:503-532: define once (scp_iter=2 pattern), ``warmup_iters`` throw-away
    iterations, restart, then a fixed number of update_problem/solve iterations.
    -> dict(us, t_risk, define_s, solve_s, cumulative_s, L2_error)"""
    _finite_guard(model, check_finite)
    us_prev = model.initial_guess_us_mat()
    model.define_problem(us_prev, verbose=False)
    for scp_iter in range(warmup_iters):
        model.update_problem(us_prev, scp_iter, verbose=False)
        us_prev, _ = model.solve(verbose=False)
    return _timed_qp_loop(model, model.update_problem, num_scp_iters_max, verbose)


def _timed_qp_loop(model, define, n_iters, verbose):
    """The timed loop of run_drone / run_driving (drone_risk.py:519-532, driving.py:486-513): from the initial guess, a fixed
    number of ``define(us_prev, scp_iter, verbose=False)`` / ``model.solve`` iterations with the wall-clock of each half.
    -> dict(us, t_risk, define_s, solve_s, cumulative_s, L2_error)"""
    us_prev = model.initial_guess_us_mat()
    define_s, solve_s, err = [], [], []
    t_risk = None
    for scp_iter in range(n_iters):
        _sync()
        t0 = time.perf_counter()
        define(us_prev, scp_iter, verbose=False)
        _sync()
        t1 = time.perf_counter()
        us, t_risk = model.solve(verbose=False)
        t2 = time.perf_counter()
        define_s.append(t1 - t0)
        solve_s.append(t2 - t1)
        err.append(L2_error_us(us, us_prev))
        us_prev = us
        if verbose:
            print(f"scp {scp_iter:3d}  define {t1 - t0:.4f}s  solve {t2 - t1:.4f}s  L2 {err[-1]:.3e}")
    define_s, solve_s = np.array(define_s), np.array(solve_s)
    return {"us": us_prev, "t_risk": t_risk, "define_s": define_s, "solve_s": solve_s,
            "cumulative_s": np.cumsum(define_s + solve_s), "L2_error": np.array(err)}


def run_drone_reduced(model, num_scp_iters_max=60, verbose=False, check_finite=True, native_loop=None, tol=None):
    """The SCP loop (drone_risk.py:519-532; also used for driving, driving.py:486-513) with every subproblem solved through
    ``Model.solve_reduced`` (device CVaR oracle + host master QP) — the path that scales to M = 1e5.
    "define" = device linearization (+ its small read-backs), "solve" = cutting-plane loop.
    ``native_loop`` (default: whenever the Model offers it -- the drone, one GPU, table-free oracle): the whole loop as ONE
    library call with the per-iteration clocks taken natively (``Model.scp_run_native`` -> rato_scp_run_drone); False: the
    per-iteration Python loop below, which is also the checker of the native one (same iterates bit for bit) and what the
    native call hands back to when it meets a case only the Python loop recovers.  (A driving Model offers the native loop
    too, but only when asked: ``native_loop=True`` / ``run_driving_reduced``.)
    ``tol``: stopping violation of the cutting-plane loops (default: ``solve_reduced``'s own, 1e-9)."""
    return _run_reduced(model, num_scp_iters_max, verbose, check_finite, native_loop, tol, {})


def _run_reduced(model, num_scp_iters_max, verbose, check_finite, native_loop, tol, solve_kw):
    """run_drone_reduced / run_driving_reduced; ``solve_kw``: further keywords of the per-iteration ``solve_reduced``"""
    _finite_guard(model, check_finite)
    if hasattr(model, "_lib"):                 # a device Model: its master QP must be the native one (no silent NumPy leg)
        from . import dense_qp
        dense_qp.require_native()
    us_prev = model.initial_guess_us_mat()
    if native_loop is None:                    # (a Model may offer the native loop without making it its default: driving)
        native_loop = None if getattr(model, "SCP_NATIVE_LOOP_DEFAULT", True) else False
    if native_loop is not False and not verbose and num_scp_iters_max > 0 and hasattr(model, "scp_run_native"):
        _sync()
        r = model.scp_run_native(us_prev, num_scp_iters_max, **({} if tol is None else {"tol": tol}))
        if r is not None:
            hist = r["us_hist"]
            prev = [np.asarray(us_prev, dtype=np.float64)] + list(hist[:-1])
            err = np.array([L2_error_us(u, p) for u, p in zip(hist, prev)])
            return {"us": hist[-1], "t_risk": float(r["t_risk"][-1]), "define_s": r["define_s"], "solve_s": r["solve_s"],
                    "cumulative_s": np.cumsum(r["define_s"] + r["solve_s"]), "L2_error": err, "cuts": r["cuts"],
                    "oracle_s": r["oracle_s"], "us_hist": hist,
                    "loop": "native (%s)" % getattr(model, "SCP_NATIVE_ENTRY", "rato_scp_run_drone")}
        if native_loop is True:
            raise RuntimeError("run_drone_reduced(native_loop=True): the native SCP loop does not apply to this Model / "
                               "handed back")
        model._cut_solver = None                # (a handed-back run starts over with the per-iteration loop)
    define_s, solve_s, err, cuts, oracle_s, hist = [], [], [], [], [], []
    t_risk = None
    for scp_iter in range(num_scp_iters_max):
        _sync()
        t0 = time.perf_counter()
        us, t_risk, info = model.solve_reduced(us_prev, scp_iter, **({} if tol is None else {"tol": tol}), **solve_kw)
        _sync()
        dt_total = time.perf_counter() - t0
        solve_s.append(info["oracle_s"] + info["master_s"])
        define_s.append(dt_total - solve_s[-1])
        oracle_s.append(info["oracle_s"])
        cuts.append(info["cuts"])
        err.append(L2_error_us(us, us_prev))
        hist.append(np.array(us, dtype=np.float64))
        us_prev = us
        if verbose:
            print(f"scp {scp_iter:3d}  define {define_s[-1]:.4f}s  solve {solve_s[-1]:.4f}s "
                  f"({info['cuts']} cuts, oracle {info['oracle_s']:.4f}s)  L2 {err[-1]:.3e}")
    define_s, solve_s = np.array(define_s), np.array(solve_s)
    return {"us": us_prev, "t_risk": t_risk, "define_s": define_s, "solve_s": solve_s,
            "cumulative_s": np.cumsum(define_s + solve_s), "L2_error": np.array(err), "cuts": np.array(cuts),
            "oracle_s": np.array(oracle_s), "us_hist": np.array(hist),
            "loop": "python (one define + one solve call per iteration)"}


def _default_threads():
    try:
        n = int(os.environ.get("OMP_NUM_THREADS") or 16)
    except ValueError:
        n = 16
    return max(1, min(16, n))


def _batch_error(k, code, entry="rato_scp_batch_run_drone"):
    """the exception a solo run raises for RATO status ``code``, naming problem ``k`` of the batch"""
    from . import _lib, dense_qp
    if code == _lib.RATO_ENONFINITE:
        return _lib.RatoNonFiniteError(f"SCP batch, problem {k}: non-finite sample sums / constraint values (RATO_ENONFINITE)")
    if code == _lib.RATO_EINFEASIBLE:
        return dense_qp.InfeasibleError(f"SCP batch, problem {k}: master QP infeasible")
    return _lib.RatoError(f"SCP batch, problem {k}: {entry} status {code}")


def run_drone_reduced_batch(models, num_scp_iters_max=60, tol=None, n_threads=None, on_error="raise", check_finite=True):
    """``run_drone_reduced`` for MANY drone Models at once (the reference's alpha x repeat grid, drone_risk.py:495-539): the
    SCP iterations run in lockstep in ONE library call (``drone_risk.scp_run_native_batch`` -> rato_scp_batch_run_drone) --
    per iteration one batched define, then rounds of one batched oracle round trip for every problem still cutting, the
    host masters of a round on ``n_threads`` threads (default min(16, OMP_NUM_THREADS)).  Every problem's iterates are those
    of ``run_drone_reduced(model)`` on it alone, bit for bit.  Scope: drone Models of method 'saa' sharing S and M (each
    with its own samples and alpha); anything else is a ValueError.
    -> one dict per Model with the keys of run_drone_reduced (us, us_hist, t_risk, cuts, L2_error, loop), where define_s /
    solve_s / cumulative_s are the BATCH's per-iteration clocks (lockstep has no per-problem clock), plus ``rounds`` (the
    batched oracle round trips of the whole run), ``rounds_per_iter``, and per iteration of the problem ``recycled`` (the kept
    cuts it started with) and ``slack`` (the master's slack: t_risk = VaR of the last evaluation + slack).  A problem the native loop hands back (rank-deficient master, a selection
    that gave up) is re-run alone through run_drone_reduced from the initial guess with a fresh cut solver (cold; tagged in
    ``loop``).  A problem that fails (non-finite values, infeasible master) leaves the batch while the others finish; then
    the exception class of the solo path is raised, naming the problem -- or, with on_error="return", its dict is
    {"status": RATO code, "error": exception, "done": iterations completed}."""
    from . import drone_risk
    solo = lambda m, **kw: run_drone_reduced(m, num_scp_iters_max=int(num_scp_iters_max), check_finite=check_finite, tol=tol,
                                             **kw)
    return _run_reduced_batch(drone_risk, "rato_scp_batch_run_drone", solo, lambda m: solo(m, native_loop=False), models,
                              num_scp_iters_max, tol, n_threads, on_error, check_finite)


def _run_reduced_batch(system, entry, solo, rerun, models, num_scp_iters_max, tol, n_threads, on_error, check_finite):
    """run_drone_reduced_batch / run_driving_reduced_batch.  ``system``: the module with ``_check_batch`` and
    ``scp_run_native_batch``; ``solo(model)``: the problem alone (no iterations to run); ``rerun(model)``: a handed-back
    problem alone through the per-iteration loop"""
    from . import _lib, dense_qp
    if on_error not in ("raise", "return"):
        raise ValueError(f"on_error must be 'raise' or 'return', got {on_error!r}")
    models = list(models)
    system._check_batch(models)
    dense_qp.require_native()
    iters = int(num_scp_iters_max)
    if iters <= 0:
        return [solo(m) for m in models]
    for m in models:
        _finite_guard(m, check_finite)
    us0 = np.stack([np.asarray(m.initial_guess_us_mat(), dtype=np.float64) for m in models])
    _sync()
    r = system.scp_run_native_batch(models, us0, iters, n_threads=_default_threads() if n_threads is None else int(n_threads),
                                    check_finite=bool(check_finite), **({} if tol is None else {"tol": tol}))
    define_s, solve_s = r["define_s"], r["oracle_s"] + r["master_s"]
    cumulative = np.cumsum(r["total_s"])
    out, failed = [], []
    for k, m in enumerate(models):
        code = int(r["status"][k])
        if code in (_lib.RATO_ERANK, _lib.RATO_ESELECT):
            m._cut_solver = None                       # (cold: a fresh cut solver, from the initial guess)
            try:
                d = rerun(m)
            except (_lib.RatoError, dense_qp.InfeasibleError) as e:     # the recovering loop failed too: a failed problem
                err = type(e)(f"SCP batch, problem {k} (handed back, status {code}; re-run alone): {e}")
                failed.append((k, err))
                out.append({"status": int(getattr(err, "status", code)), "error": err, "done": int(r["done"][k])})
                continue
            d["loop"] = d["loop"] + " -- handed back by the batch (status %d), re-run alone" % code
            d["rounds"] = r["rounds"]
            out.append(d)
            continue
        if code != 0:
            err = _batch_error(k, code, entry)
            failed.append((k, err))
            out.append({"status": code, "error": err, "done": int(r["done"][k])})
            continue
        hist = r["us_hist"][k]
        prev = [us0[k]] + list(hist[:-1])
        err = np.array([L2_error_us(u, p) for u, p in zip(hist, prev)])
        out.append({"us": hist[-1], "t_risk": float(r["t_risk"][k, -1]), "define_s": define_s, "solve_s": solve_s,
                    "cumulative_s": cumulative, "L2_error": err, "cuts": r["cuts"][k], "us_hist": hist,
                    "rounds": r["rounds"], "rounds_per_iter": r["rounds_per_iter"], "recycled": r["recycled"][k],
                    "slack": r["slack"][k],
                    "loop": "native batch (%s)" % entry})
    if failed and on_error == "raise":
        raise failed[0][1]
    return out


def draw_saa_batches(num_repeats=30, M=50, S=None, seed=0):
    """The sample batches of the reference's drone experiment in ITS draw order (drone_risk.py:57, :480-490):
    ``np.random.seed(seed)``, then ``sample_uncertain_parameters('saa', M)`` once per repeat.  Host only (no GPU).
    -> list of (DWs (M,S,6), masses (M,), obs_Qs (M,n_obs,3,3)), one per repeat."""
    from . import drone_params as P
    from .drone_utils import sample_uncertain_parameters
    S = P.S if S is None else int(S)
    np.random.seed(seed)
    return [sample_uncertain_parameters('saa', M=M, S=S, dt=P.T / S) for _ in range(num_repeats)]


def drone_saa_experiment(alphas=(0.05, 0.1, 0.2, 0.3), num_repeats=30, M=50, S=20, iters=60, seed=0, mc_model=None,
                         results_dir=None, n_threads=None, device='cuda:0', mc='per_alpha'):
    """The reference's drone SAA experiment (drone_risk.py:480-539, :697-725) as one call: the sample batches drawn in the
    reference's order (``draw_saa_batches``), the alpha x repeat grid solved in ONE lockstep batch
    (``run_drone_reduced_batch``; each alpha reuses the same batches), with ``mc_model`` the Monte-Carlo report per alpha
    (``monte_carlo_report``; mc='grid': all alphas in one call, ``monte_carlo_report_grid``), with ``results_dir`` the
    reference's result files drone_alpha=<alpha>_repeat=<r>.npy (us, then xs: ``save_results``).  -> dict(alphas, results [alpha][repeat] (the run_drone_reduced_batch dicts), us (A, R, S, 3),
    reports {alpha: report} (with mc_model), rounds, wall_s)"""
    from . import drone_risk
    batches = draw_saa_batches(num_repeats, M, S, seed)
    alphas = [float(a) for a in alphas]
    models = [drone_risk.Model(S, *batches[r], 'saa', a, device=device) for a in alphas for r in range(num_repeats)]
    return _saa_experiment(models, run_drone_reduced_batch, iters, n_threads, alphas, num_repeats, mc_model, results_dir,
                           "drone", mc)


def _saa_experiment(models, run_batch, iters, n_threads, alphas, num_repeats, mc_model, results_dir, name, mc='per_alpha'):
    """drone_saa_experiment / driving_saa_experiment once the alpha-major grid of ``models`` is built: ONE batched solve
    (``run_batch``), the result files <name>_alpha=<alpha>_repeat=<r>.npy and the Monte-Carlo reports"""
    if mc not in ('per_alpha', 'grid'):
        raise ValueError(f"mc must be 'per_alpha' or 'grid', got {mc!r}")
    _sync()
    t0 = time.perf_counter()
    res = run_batch(models, num_scp_iters_max=iters, n_threads=n_threads)
    _sync()
    wall = time.perf_counter() - t0
    grid = [[res[i * num_repeats + r] for r in range(num_repeats)] for i in range(len(alphas))]
    us = np.stack([np.stack([g["us"] for g in row]) for row in grid])
    out = {"alphas": alphas, "results": grid, "us": us, "rounds": res[0].get("rounds"), "wall_s": wall, "models": models}
    if results_dir is not None:
        os.makedirs(results_dir, exist_ok=True)
        for i, a in enumerate(alphas):
            for r in range(num_repeats):
                xs = models[i * num_repeats + r].us_to_state_trajectories(us[i, r])
                xs = xs.cpu().numpy() if hasattr(xs, "cpu") else np.asarray(xs)
                save_results(os.path.join(results_dir, f"{name}_alpha={a}_repeat={r}.npy"), us[i, r], xs)
    if mc_model is not None and mc == 'grid':
        out["reports"] = monte_carlo_report_grid(mc_model, us, alphas)
    elif mc_model is not None:
        out["reports"] = {a: monte_carlo_report(mc_model, list(us[i]), a) for i, a in enumerate(alphas)}
    return out


def draw_main_figure_batches(M=50, M_mc=10000, S=20, seed=0):
    """The two sample batches of the main-figure script in ITS draw order: ``np.random.seed(seed)``
    (drone_main_plot.py:26), the SAA batch of ``Model(M, 'saa', alpha)`` (:603), then the validation batch of
    ``Model(10000)`` (:632) from the SAME continuing stream -- the script does not reseed in between.  Its inline sampler
    (:92-121) draws in ``drone_utils.sample_uncertain_parameters``' order with dt = T / S.  Host only (no GPU).
    -> ((DWs, masses, obs_Qs) of the SAA batch, (DWs, masses, obs_Qs) of the validation batch)"""
    from . import drone_params as P
    from .drone_utils import sample_uncertain_parameters
    np.random.seed(seed)
    saa = sample_uncertain_parameters('saa', M=int(M), S=int(S), dt=P.T / S)
    return saa, sample_uncertain_parameters('saa', M=int(M_mc), S=int(S), dt=P.T / S)


def drone_main_figure_experiment(alpha=0.1, M=50, S=20, iters=20, M_mc=10000, seed=0, bins=100, hist_range=(-0.6, 0.4),
                                 results_dir=None, device='cuda:0'):
    """The Monte-Carlo block behind the paper's main figure (drone_main_plot.py:603-710) as one call: the two batches in
    the script's draw order (``draw_main_figure_batches``), ``iters`` iterations of the reduced SCP from the script's
    all-axes initial guess (``run_drone_reduced``; the script's own loop solves the full QP with OSQP -- no claim about
    its iterates), then on the validation batch ONE rollout with the Euclidean rows that returns the trajectories, the
    raw per-sample maxima and the row behind each (rato_drone_eval_metric), their VaR / AVaR (rato_risk_stats) and
    their histogram over ``hist_range`` (rato_histogram; the figure's axis is [-0.6, 0.4], :750).
    -> dict, all on the host: us (S,3), xs (M,S+1,6) of the SAA batch, xs_MC (M_mc,S+1,6), obs_Qs (M_mc,n_obs,3,3),
    B_satisfied_vec = constraints_vec <= OSQP_TOL + 1e-6, constraints_vec (M_mc,), percentage_safe, var_val, avar_val,
    mean, arg (M_mc,) int32 = j*S + t of each sample's maximum, hist_counts (bins + 3: below, the bins, at or above, NaN),
    hist_edges (bins + 1).
    ``percentage_safe`` keeps the reference's value under the reference's name: 1 - mean(B_satisfied_vec) (:697), i.e.
    the share of UNSAFE samples.  With ``results_dir``: drone_main_monte_carlo.npy, the script's nine arrays in its order
    (:700-710; ``load_results(path, 9)``)."""
    import torch
    from . import drone_risk, stats
    from .drone_params import OSQP_TOL
    saa, mc = draw_main_figure_batches(M, M_mc, S, seed)
    model = drone_risk.Model(S, *saa, 'saa', alpha, device=device)
    guess = model.initial_guess_us_mat
    model.initial_guess_us_mat = lambda: guess(all_axes=True)            # drone_main_plot.py:137-148
    us = np.asarray(run_drone_reduced(model, num_scp_iters_max=int(iters))["us"], dtype=np.float64)
    xs = model.us_to_state_trajectories(us)
    mc_model = drone_risk.Model(S, *mc, 'saa', alpha, device=device)
    Z, xs_MC, _, arg = mc_model.eval_device(us, want_xs=True, metric='euclidean', want_arg=True, tol=0.0)
    rec = stats.risk_stats_device(Z, alpha, thr=OSQP_TOL + 1e-6)
    counts = stats.histogram_device(Z, hist_range[0], hist_range[1], bins)
    st = dict(zip(stats._STAT_NAMES, rec.cpu().numpy().tolist()))
    if np.isnan(st["var"]):                                                 # (a selection that gave up: the recovering path)
        st = stats.risk_stats(Z, alpha, thr=OSQP_TOL + 1e-6)
    constraints_vec = Z.double().cpu().numpy()
    B = constraints_vec <= OSQP_TOL + 1e-6
    lo, hi = float(hist_range[0]), float(hist_range[1])
    out = {"us": us, "xs": xs, "xs_MC": xs_MC.permute(2, 0, 1).double().cpu().numpy(), "obs_Qs": np.asarray(mc[2]),
           "B_satisfied_vec": B, "constraints_vec": constraints_vec, "percentage_safe": 1.0 - float(np.mean(B)),
           "var_val": st["var"], "avar_val": st["cvar"], "mean": st["mean"], "arg": arg.cpu().numpy(),
           "hist_counts": counts.cpu().numpy().view(np.uint32).astype(np.int64),
           "hist_edges": lo + np.arange(int(bins) + 1, dtype=np.float64) * ((hi - lo) / int(bins))}
    if results_dir is not None:
        os.makedirs(results_dir, exist_ok=True)
        save_results(os.path.join(results_dir, "drone_main_monte_carlo.npy"), *(out[k] for k in (
            "us", "xs", "xs_MC", "obs_Qs", "B_satisfied_vec", "constraints_vec", "percentage_safe", "var_val", "avar_val")))
    return out


def run_driving(model, num_scp_iters_max=15, verbose=False, check_finite=True):
    """driving.py:474-513: two warm-up solves (scp_iter 0 and 1), restart, then a fixed number of
    define_problem/solve iterations (define re-sets the solver up at iterations 0 and 1)."""
    _finite_guard(model, check_finite)
    us_prev = model.initial_guess_us_mat()
    model.define_problem(us_prev, verbose=False)
    us, _ = model.solve()
    model.define_problem(us, 1, verbose=False)
    us, _ = model.solve()
    return _timed_qp_loop(model, model.define_problem, num_scp_iters_max, verbose)


def save_results(path, *arrays):
    """The reference's result-file convention: several ``np.save`` calls appended to ONE file
    (``us`` then ``xs``: drone_risk.py:534-539; nine arrays: drone_main_plot.py:700-710)."""
    with open(path, 'wb') as f:
        for a in arrays:
            np.save(f, np.asarray(a))


def load_results(path, n):
    """Read back ``n`` arrays written by ``save_results`` (sequential ``np.load``, drone_risk.py:704-708)."""
    with open(path, 'rb') as f:
        return [np.load(f) for _ in range(n)]


def run_driving_reduced(model, num_scp_iters_max=15, verbose=False, check_finite=True, native_loop=False, final_rows='numpy',
                        tol=None):
    """driving.py:486-513 with ``Model.solve_reduced`` subproblems (same loop as run_drone_reduced).  The defaults are the
    per-iteration Python loop with the NumPy final rows.  ``native_loop=True``: the whole loop as ONE library call
    (``Model.scp_run_native`` -> rato_scp_run_car), which computes the final rows natively (rato_car_ego_final_rows: to
    rounding, not to the bit, the NumPy ones); ``native_loop=False, final_rows='native'`` is its per-iteration checker -- the
    same iterates bit for bit -- and what a handed-back problem is repeated with."""
    if final_rows not in ('numpy', 'native'):
        raise ValueError(f"final_rows must be 'numpy' or 'native', got {final_rows!r}")
    return _run_reduced(model, num_scp_iters_max, verbose, check_finite, bool(native_loop), tol,
                        {} if final_rows == 'numpy' else {"final_rows": final_rows})


def run_driving_reduced_batch(models, num_scp_iters_max=15, tol=None, n_threads=None, on_error="raise", check_finite=True):
    """``run_driving_reduced(native_loop=True)`` for MANY driving Models at once (the reference's alpha x repeat grid,
    driving.py:467-529) in ONE library call (``driving.scp_run_native_batch`` -> rato_scp_batch_run_car): the contract and the
    result dicts of ``run_drone_reduced_batch``.  Every problem's iterates are those of its solo native run, bit for bit.
    Scope: driving Models of method 'saa' with a materialised dW sharing S, M and the parameters; anything else is a
    ValueError.  A handed-back problem is re-run alone, cold, with ``native_loop=False, final_rows='native'``."""
    from . import driving
    solo = lambda m, **kw: run_driving_reduced(m, num_scp_iters_max=int(num_scp_iters_max), check_finite=check_finite, tol=tol,
                                               **kw)
    return _run_reduced_batch(driving, "rato_scp_batch_run_car", lambda m: solo(m, native_loop=True),
                              lambda m: solo(m, native_loop=False, final_rows='native'), models, num_scp_iters_max, tol,
                              n_threads, on_error, check_finite)


def draw_driving_saa_batches(alphas, num_repeats=30, M=50, S=None, seed=0):
    """The sample batches of the reference's driving experiment in ITS draw order (driving.py:61, :470-472):
    ``np.random.seed(seed)``, then one ``Model(M, 'saa', alpha)`` -- i.e. ``driving.sample_uncertain_parameters`` -- per
    (alpha, repeat), alpha-major: every cell of the grid has samples of its own (unlike the drone's, whose alphas share the
    repeats' batches).  Host only (no GPU).  -> [alpha][repeat] of (states_init, omegas_speed, omegas_repulsive, DWs)."""
    from . import driving
    from . import driving_params as P
    S = P.S if S is None else int(S)
    np.random.seed(seed)
    return [[driving.sample_uncertain_parameters(M, 'saa', S) for _ in range(num_repeats)] for _ in alphas]


def driving_saa_experiment(alphas=(0.01, 0.02, 0.05, 0.1), num_repeats=30, M=50, S=20, iters=15, seed=0, mc_model=None,
                           results_dir=None, n_threads=None, device='cuda:0', mc='per_alpha'):
    """The reference's driving SAA experiment (driving.py:467-529, :672-700) as one call, shaped like
    ``drone_saa_experiment``: the samples of every (alpha, repeat) drawn in the reference's order
    (``draw_driving_saa_batches``), the grid solved in ONE lockstep batch (``run_driving_reduced_batch``), with ``mc_model``
    the Monte-Carlo report per alpha (mc='grid': all alphas in one call), with ``results_dir`` the reference's result files driving_alpha=<alpha>_repeat=<r>.npy
    (us, then xs).  -> dict(alphas, results [alpha][repeat], us (A, R, S, 2), reports {alpha: report} (with mc_model), rounds,
    wall_s, models)"""
    from . import driving
    alphas = [float(a) for a in alphas]
    draws = draw_driving_saa_batches(alphas, num_repeats, M, S, seed)
    models = [driving.Model(M, 'saa', a, S=S, device=device, samples=draws[i][r])
              for i, a in enumerate(alphas) for r in range(num_repeats)]
    return _saa_experiment(models, run_driving_reduced_batch, iters, n_threads, alphas, num_repeats, mc_model, results_dir,
                           "driving", mc)


def monte_carlo_report(mc_model, us_list, alpha, verbose=False):
    """The out-of-sample validation block of the reference's scripts (drone_risk.py:697-725, driving.py:672-700):
    every solution in ``us_list`` (the SAA repeats of one alpha) is evaluated on the Monte-Carlo model's fresh
    samples (M = 10000 there) -- fraction of samples that satisfy the constraints, AVaR_alpha of the max constraint
    value, control cost -- and the mean / median over the repeats are reported.  All repeats in ONE library call where the
    model has the batched entry point (drone, driving: ``Model.eval_batch_device``), one rollout kernel + one exact selection
    per solution otherwise; all on the device.  -> dict of per-solution arrays and the aggregates."""
    frac, avar, var, cost = [], [], [], []

    def _append(st, us):
        frac.append(st["frac_satisfied"])
        avar.append(st["cvar"])
        var.append(st["var"])
        cost.append(mc_model.monte_carlo_cost(us))
        if verbose:
            print("B_satisfied_vec =", frac[-1])

    batched = getattr(mc_model, "eval_batch_device", None)
    if batched is not None and len(us_list) > 1 and getattr(mc_model, "_dW", None) is not None:
        # all repeats of this alpha in ONE call (rato_*_eval_batch: one rollout launch over tiles x K, one launch of K
        # exact selections); row k is what the per-solution call below gives for solution k, to the bit
        from . import stats
        _, rec = batched(np.stack([np.asarray(us) for us in us_list]), alpha=alpha)
        rec = rec.cpu().numpy()
        names = stats._STAT_NAMES
        for k, us in enumerate(us_list):
            st = dict(zip(names, rec[k].tolist()))
            if np.isnan(st["var"]):                    # (a selection that gave up: the recovering per-solution path)
                st = mc_model.monte_carlo_statistics(us, alpha=alpha)
            _append(st, us)
        us_list = []
    for us in us_list:
        _append(mc_model.monte_carlo_statistics(us, alpha=alpha), us)
    return _mc_aggregate(frac, avar, var, cost, verbose)


def _mc_aggregate(frac, avar, var, cost, verbose=False):
    """the dict of ``monte_carlo_report`` from the per-solution values"""
    out = {"frac_satisfied": np.array(frac), "avar": np.array(avar), "var": np.array(var), "cost": np.array(cost)}
    for k in ("frac_satisfied", "avar", "cost"):
        out[k + "_mean"], out[k + "_median"] = float(np.mean(out[k])), float(np.median(out[k]))
    if verbose:
        print("percentage safe (mean) =", out["frac_satisfied_mean"])
        print("avar (mean) =", out["avar_mean"])
        print("cost (mean) =", out["cost_mean"])
        print("percentage safe (median) =", out["frac_satisfied_median"])
        print("avar (median) =", out["avar_median"])
        print("cost (median) =", out["cost_median"])
    return out


def monte_carlo_report_grid(mc_model, us_grid, alphas, verbose=False):
    """``{alpha: monte_carlo_report(mc_model, us_grid[i], alpha)}`` for the whole alpha x repeat grid ``us_grid``
    (A, R, S, n_u) in ONE ``Model.eval_batch_device(alphas=...)`` call: the A x R rollouts in one launch, then the A x R
    exact selections, every row at its own alpha, in one more (rato_risk_stats_rows; five beyond 12,288 validation samples)
    -- where the loop over ``monte_carlo_report`` makes one library call and one read-back per alpha.  Every report is the
    dict ``monte_carlo_report`` returns, to the bit while M_mc <= 12,288; beyond, mean-type entries (avar) agree to the
    order of the fp64 sums, the exactly defined ones (var, frac_satisfied) to the bit."""
    from . import stats
    us_grid = np.asarray(us_grid)
    alphas = [float(a) for a in alphas]
    A, R = us_grid.shape[:2]
    if len(alphas) != A:
        raise ValueError(f"us_grid has {A} alpha rows for {len(alphas)} alphas")
    _, rec = mc_model.eval_batch_device(us_grid.reshape((A * R,) + us_grid.shape[2:]), alphas=np.repeat(alphas, R))
    rec = rec.cpu().numpy().reshape(A, R, -1)
    reports = {}
    for i, a in enumerate(alphas):
        frac, avar, var, cost = [], [], [], []
        for r in range(R):
            st = dict(zip(stats._STAT_NAMES, rec[i, r].tolist()))
            if np.isnan(st["var"]):                    # (as monte_carlo_report: the recovering per-solution path)
                st = mc_model.monte_carlo_statistics(us_grid[i, r], alpha=a)
            frac.append(st["frac_satisfied"])
            avar.append(st["cvar"])
            var.append(st["var"])
            cost.append(mc_model.monte_carlo_cost(us_grid[i, r]))
            if verbose:
                print("B_satisfied_vec =", frac[-1])
        reports[a] = _mc_aggregate(frac, avar, var, cost, verbose)
    return reports


def driving_gaussian_tol():
    from . import driving_gaussian
    return driving_gaussian.OSQP_TOL


def _gaussian_solve_all(models, us_list, alphas_list, scp_iter, clocks=None):
    """One lockstep SCP iteration of K driving Gaussian problems: ONE K-problem linearize launch (models[0] launches: the
    kernel's parameters do not depend on alpha), then K host QPs -- or, when the models' solver is 'ipm', ONE
    ``qp_ipm.solve_batch`` launch for the K QPs.  -> ([us], [alphas_risk], [status])"""
    batched = models[0].solver == 'ipm'
    t0 = time.perf_counter()
    lin = models[0].linearize_device(np.stack(us_list), np.stack(alphas_list))
    lin = {k: v.cpu().numpy() for k, v in lin.items()}             # (the copy waits for the launch)
    t1 = time.perf_counter()
    us_out, al_out, status, sols = [], [], [], []
    for k, m in enumerate(models):
        m.define_problem(us_list[k], alphas_list[k], scp_iter, lin={key: v[k] for key, v in lin.items()})
        if not batched:
            sols.append(m.solve())
    if batched:
        _gaussian_solve_ipm(models)
        sols = [m.solution() for m in models]
    for k, m in enumerate(models):
        us, al = sols[k]
        if not (np.all(np.isfinite(us)) and np.all(np.isfinite(al))):
            # a solve that hands back no point (qp.OSQP: 'primal infeasible' -> nan): the reference prints and carries the
            # nan on (:451-452); here the problem keeps its iterate, and the status list says so
            us, al = np.array(us_list[k]), np.array(alphas_list[k])
        elif m.res.info.status != 'solved':
            # an ADMM point that missed eps (iteration cap) may sit outside the QP's own box 100 OSQP_TOL <= alpha_t <= alpha
            # by more than eps, and ppf(1 - alpha_t) does not exist for alpha_t <= 0: carry its projection onto the box
            al = np.clip(al, 100 * driving_gaussian_tol(), m.alpha)
        us_out.append(us)
        al_out.append(al)
        status.append(m.res.info.status)
    if clocks is not None:
        clocks[0].append(t1 - t0)
        clocks[1].append(time.perf_counter() - t1)
    return us_out, al_out, status


def _gaussian_solve_ipm(models):
    """the K defined problems in one ``qp_ipm.solve_batch`` call (P and q do not depend on alpha: shared); leaves ``m.res``"""
    from . import qp_ipm
    data = [m.osqp_prob.data() for m in models]
    _, _, info = res = qp_ipm.solve_batch(data[0][0], data[0][1], np.stack([d[2] for d in data]), np.stack([d[3] for d in data]),
                                          np.stack([d[4] for d in data]), models[0].osqp_prob.tol, models[0].osqp_prob.max_iter,
                                          backend=models[0].osqp_prob.backend, device=models[0].osqp_prob.device)
    for k, m in enumerate(models):
        m.res = m.osqp_prob.result(res[0][k], res[1][k], info["status"][k], int(info["iterations"][k]))


def run_driving_gaussian_batch(models, num_scp_iters_max=60, solver=None):
    """``run_driving_gaussian`` for K ``driving_gaussian.Model``s of one S in lockstep (the reference's four alphas,
    driving_gaussian.py:469-498): per iteration one K-problem launch and K host QPs ('osqp') or one K-problem QP launch ('ipm').
    ``solver``: None = the models' own (which must agree), else it is set on every model.  -> list of the result dicts."""
    S, outer = models[0].S, models[0].outer_product
    if any(m.S != S or m.outer_product != outer for m in models):
        raise ValueError("the models of a lockstep batch share S and outer_product")
    if solver is not None:
        from . import driving_gaussian
        if solver not in driving_gaussian.SOLVERS:
            raise ValueError(f"solver must be one of {driving_gaussian.SOLVERS}, got {solver!r}")
        for m in models:
            m.solver = solver
    if any(m.solver != models[0].solver for m in models):
        raise ValueError("the models of a lockstep batch share their solver")
    K = len(models)
    us_prev = [m.initial_guess_us_mat() for m in models]           # the two warm-up solves (:472-479)
    al_prev = [m.initial_guess_alphas_risk() for m in models]
    us, _, _ = _gaussian_solve_all(models, us_prev, al_prev, 0)
    _gaussian_solve_all(models, us, al_prev, 1)
    us_prev = [m.initial_guess_us_mat() for m in models]           # restart (:481-482)
    al_prev = [m.initial_guess_alphas_risk() for m in models]
    clocks, err, statuses = ([], []), [], []
    for scp_iter in range(num_scp_iters_max):
        us, al, st = _gaussian_solve_all(models, us_prev, al_prev, scp_iter, clocks)
        err.append([L2_error_us(us[k], us_prev[k]) for k in range(K)])
        statuses.append(st)
        us_prev, al_prev = us, al                                  # the alphas are carried along (:491-492)
    xs = models[0].linearize_device(np.stack(us_prev), np.stack(al_prev), want_trajectory=True)["mus"].cpu().numpy()
    define_s, solve_s = np.array(clocks[0]), np.array(clocks[1])
    err = np.array(err).reshape(num_scp_iters_max, K)
    return [{"us": us_prev[k], "alphas_risk": al_prev[k], "xs": xs[k], "L2_error": err[:, k],
             "status": [st[k] for st in statuses], "define_s": define_s, "solve_s": solve_s} for k in range(K)]


def run_driving_gaussian(model, num_scp_iters_max=60, solver=None):
    """driving_gaussian.py:471-492: two warm-up solves (scp_iter 0 and 1), restart from the initial guess, then a fixed number
    of define_problem / solve iterations with the risk allocation carried from one iteration to the next.  -> dict(us (S, 2),
    alphas_risk (S,), xs (S+1, 8) [the mean trajectory of us], L2_error per iteration, status per solve, define_s, solve_s)"""
    return run_driving_gaussian_batch([model], num_scp_iters_max, solver)[0]


def driving_gaussian_experiment(alphas=(0.01, 0.02, 0.05, 0.1), S=None, iters=60, M_mc=10000, seed=0, results_dir=None,
                                device='cuda:0', solver='osqp'):
    """The reference's driving Gaussian baseline (driving_gaussian.py:466-498) and its Monte-Carlo report (driving.py:719-739)
    as one call: the problems of all alphas in lockstep (``run_driving_gaussian_batch``), then ONE ``eval_batch_device`` call of
    a fresh ``driving.Model(M_mc)`` (drawn under ``np.random.seed(seed)``) over the solutions.  Per alpha
    percentage_safe = mean(max_t(-distance) - OSQP_TOL <= 1e-6) with the SAA model's OSQP_TOL, as the block computes it, and
    monte_carlo_cost.  With ``results_dir``: driving_gaussian_alpha=<alpha>.npy holding (us, xs).  ``solver``: 'osqp' or 'ipm'
    (``driving_gaussian.Model``).
    -> dict(alphas, results [alpha], us (A, S, 2), Z (A, M_mc) [max_t(-distance) - OSQP_TOL per sample], percentage_safe (A,),
    cost (A,), wall_s)"""
    from . import driving, driving_gaussian
    from . import driving_params as P
    S = P.S if S is None else int(S)
    alphas = [float(a) for a in alphas]
    t0 = time.perf_counter()
    models = [driving_gaussian.Model(alpha=a, S=S, device=device, solver=solver) for a in alphas]
    results = run_driving_gaussian_batch(models, iters)
    wall = time.perf_counter() - t0
    us = np.stack([r["us"] for r in results])
    np.random.seed(seed)
    mc_model = driving.Model(M_mc, S=S, device=device)
    Z, _ = mc_model.eval_batch_device(us, want_stats=False)       # Z = max_t(-distance) - OSQP_TOL (driving.py:630-638)
    Z = Z.double().cpu().numpy()
    out = {"alphas": alphas, "results": results, "us": us, "Z": Z, "percentage_safe": np.mean(Z <= 1e-6, axis=1),
           "cost": np.array([mc_model.monte_carlo_cost(u) for u in us]), "wall_s": wall}
    if results_dir is not None:
        os.makedirs(results_dir, exist_ok=True)
        for a, r in zip(alphas, results):
            save_results(os.path.join(results_dir, f"driving_gaussian_alpha={a}.npy"), r["us"], r["xs"])
    return out


def _drone_gaussian_ipm_result(model, Z, info, trajectory, callback_s, total_s):
    """the ``run_drone_gaussian`` dictionary of one ``drone_gaussian_ipm.solve_batch`` result"""
    D = 3 * model.S
    xs, Sigmas = trajectory(Z)
    return {"Z": Z, "us": model.convert_us_vec_to_us_mat(Z[:D]), "alphas_risk": Z[D:].copy(), "xs": xs, "Sigmas": Sigmas,
            "status": info["status"], "message": "interior point: " + info["status"], "nit": int(info["iterations"]),
            "nfev": int(info["factorizations"]), "constr_violation": float(info["primal_infeasibility"]),
            "optimality": float(info["dual_infeasibility"]), "fun": float(info["f"]), "callback_s": float(callback_s),
            "total_s": float(total_s), "info": info}


def run_drone_gaussian(model, Z0=None, maxiter=3000, callbacks=None, results_dir='results', solver='trust-constr', tol=1e-8,
                       backend=None, driver='host', chol='workgroup'):
    """The NLP of drone_gaussian.py:400-534 solved with ``scipy.optimize.minimize(method='trust-constr')`` -- the installed
    solver that takes the Hessian of lam . g, which is the script's ``hess_lagrange_dot_g``: the non-linear rows as a
    ``NonlinearConstraint(g, gL, gU, jac, hess)`` (6 equalities, the rest one-sided), the box on u and on the allocations as
    ``Bounds`` (the allocations with ``keep_feasible=True``: ppf(1 - a) does not exist for a <= 0), the allocation sum as a
    ``LinearConstraint``, gtol = 1e-8, xtol = 1e-10.  ``callbacks``: dict(linearize(Z) -> (g_nl, jac_nl), hessian(Z, lam) ->
    tril, trajectory(Z) -> (xs, Sigmas)), by default the model's device callbacks (one launch each); g and its Jacobian at
    the same point share one launch.  ``Z0``: the start, by default the script's (the SAA repeat-0 controls of
    ``results_dir`` and the uniform allocation).
    -> dict(Z, us (S, 3), alphas_risk, xs (S+1, 6), Sigmas (S+1, 6, 6), status, message, nit, nfev, constr_violation,
    optimality, fun, callback_s, total_s)
    ``solver='ipm'``: the same NLP by ``drone_gaussian_ipm.solve_batch`` (a batch of one; ``backend`` 'device', or
    'numpy', the default when ``callbacks`` are given; ``tol``: its E_0 tolerance) -> the same keys with status one of
    'converged' | 'max_iter' | 'line_search', nit = iterations, nfev = factorizations, constr_violation / optimality = the
    primal / dual parts of the final E_0, and ``info`` (``solve_batch``'s, with the multipliers).  ``driver``: 'host', 'device'
    or 'device_grid' (``solver='ipm'`` only: where ``solve_batch`` keeps the iterate).  ``chol``: 'workgroup' or 'grid'
    (``solver='ipm'`` on the device: which Cholesky; the result does not depend on it)."""
    from . import ipm as _ipm
    _ipm.check_chol(chol)
    if driver not in _ipm.DRIVERS:
        raise ValueError(f"driver must be 'host', 'device' or 'device_grid', got {driver!r}")
    if solver not in ('trust-constr', 'ipm'):
        raise ValueError(f"solver must be 'trust-constr' or 'ipm', got {solver!r}")
    if _ipm.on_device(driver) and solver != 'ipm':
        raise ValueError(f"driver={driver!r} is the interior-point method's: it needs solver='ipm'")
    if solver == 'ipm':
        from . import drone_gaussian_ipm
        backend = ('device' if callbacks is None else 'numpy') if backend is None else backend
        Z0 = model.initial_guess(results_dir) if Z0 is None else np.asarray(Z0, dtype=np.float64)
        clocks = {}
        t0 = time.perf_counter()
        (Z, info), = drone_gaussian_ipm.solve_batch([model], [Z0], tol=tol, max_iter=int(maxiter), backend=backend,
                                                    callbacks=None if callbacks is None else [callbacks], clocks=clocks,
                                                    driver=driver, chol=chol)
        total = time.perf_counter() - t0
        trajectory = (model.device_callbacks() if callbacks is None else callbacks)["trajectory"]
        return _drone_gaussian_ipm_result(model, Z, info, trajectory, clocks["callbacks"], total)
    from scipy.optimize import Bounds, LinearConstraint, NonlinearConstraint, minimize
    from . import drone_params as P
    cb = model.device_callbacks() if callbacks is None else callbacks
    S, nvar, n_nl = model.S, model.nvar, model.n_nl
    D = 3 * S
    Z0 = model.initial_guess(results_dir) if Z0 is None else np.asarray(Z0, dtype=np.float64)
    clock, cache = [0.0], {}
    rows, cols = np.tril_indices(nvar)
    curv = np.zeros(nvar)
    curv[:D] = np.tile(4 * model.dt * np.diag(P.R), S)

    def lin(x):
        key = x.tobytes()
        if cache.get("key") != key:
            t0 = time.perf_counter()
            cache["key"], cache["val"] = key, cb["linearize"](np.array(x, dtype=np.float64))
            clock[0] += time.perf_counter() - t0
        return cache["val"]

    def hess(x, v):
        t0 = time.perf_counter()
        tril = cb["hessian"](np.array(x, dtype=np.float64), np.asarray(v, dtype=np.float64))
        clock[0] += time.perf_counter() - t0
        H = np.zeros((nvar, nvar))
        H[rows, cols] = tril
        H[cols, rows] = tril
        return H

    g_L = np.concatenate([np.zeros(6), np.full(n_nl - 6, -np.inf)])
    nonlinear = NonlinearConstraint(lambda x: lin(x)[0], g_L, np.zeros(n_nl), jac=lambda x: lin(x)[1], hess=hess)
    lo = np.concatenate([np.full(D, float(model.u_min)), np.full(nvar - D, 1e-6)])
    hi = np.concatenate([np.full(D, float(model.u_max)), np.full(nvar - D, float(model.alpha))])
    bounds = Bounds(lo, hi, keep_feasible=np.arange(nvar) >= D)
    sum_row = np.concatenate([np.zeros(D), np.ones(nvar - D)])[None, :]
    t0 = time.perf_counter()
    res = minimize(lambda x: 0.5 * float(np.sum(curv * x * x)), Z0, method='trust-constr', jac=lambda x: curv * x,
                   hess=lambda x: np.diag(curv), bounds=bounds,
                   constraints=[nonlinear, LinearConstraint(sum_row, 0.0, float(model.alpha))],
                   options=dict(gtol=1e-8, xtol=1e-10, maxiter=int(maxiter)))
    total = time.perf_counter() - t0
    Z = np.asarray(res.x, dtype=np.float64)
    us = model.convert_us_vec_to_us_mat(Z[:D])
    xs, Sigmas = cb["trajectory"](Z)
    return {"Z": Z, "us": us, "alphas_risk": Z[D:].copy(), "xs": xs, "Sigmas": Sigmas, "status": int(res.status),
            "message": str(res.message), "nit": int(res.nit), "nfev": int(res.nfev),
            "constr_violation": float(res.constr_violation), "optimality": float(res.optimality), "fun": float(res.fun),
            "callback_s": clock[0], "total_s": total}


def drone_gaussian_experiment(alphas=(0.05, 0.1, 0.2, 0.3), S=20, results_dir='results', M_mc=10000, seed=0, maxiter=3000,
                              saa_iters=60, saa_M=50, device='cuda:0', solver='trust-constr', tol=1e-8, clocks=None,
                              driver='host', chol='workgroup'):
    """The reference's drone Gaussian baseline (drone_gaussian.py:400-534) and the third block of the drone Monte-Carlo report
    (drone_risk.py:742-761) as one call.  The start of every alpha is the SAA repeat-0 solution
    ``results_dir``/drone_alpha=<alpha>_repeat=0.npy, read where it exists and made by ``drone_saa_experiment`` (one repeat)
    where it does not; each alpha is solved by ``run_drone_gaussian`` (``solver='ipm'``: all alphas in ONE
    ``drone_gaussian_ipm.solve_batch`` call on the device, whose clocks ``clocks`` receives and whose ``driver`` is 'host',
    'device' or 'device_grid' and whose ``chol`` is 'workgroup' or 'grid') and written to drone_gaussian_alpha=<alpha>.npy as
    (us, xs); then ONE ``eval_batch_device`` call of a fresh ``drone_risk.Model`` of M_mc samples (drawn under
    ``np.random.seed(seed)``) over the solutions.  Per alpha percentage_safe = mean(max constraint <= 1e-6), as the block
    computes it, and monte_carlo_cost.
    -> dict(alphas, results [alpha] (the run_drone_gaussian dicts), status (A,), us (A, S, 3), Z (A, M_mc) [the per-sample
    maxima], percentage_safe (A,), cost (A,), wall_s)"""
    from . import drone_gaussian, drone_risk
    from . import drone_params as P
    from .drone_utils import sample_uncertain_parameters
    alphas = [float(a) for a in alphas]
    from . import ipm as _ipm
    _ipm.check_chol(chol)
    if driver not in _ipm.DRIVERS:
        raise ValueError(f"driver must be 'host', 'device' or 'device_grid', got {driver!r}")
    if _ipm.on_device(driver) and solver != 'ipm':
        raise ValueError(f"driver={driver!r} is the interior-point method's: it needs solver='ipm'")
    os.makedirs(results_dir, exist_ok=True)
    missing = [a for a in alphas if not os.path.isfile(os.path.join(results_dir, f"drone_alpha={a}_repeat=0.npy"))]
    if missing:
        drone_saa_experiment(alphas=missing, num_repeats=1, M=saa_M, S=S, iters=saa_iters, seed=seed, results_dir=results_dir,
                             device=device)
    t0 = time.perf_counter()
    if solver not in ('trust-constr', 'ipm'):
        raise ValueError(f"solver must be 'trust-constr' or 'ipm', got {solver!r}")
    results = []
    if solver == 'ipm':
        from . import drone_gaussian_ipm
        models = [drone_gaussian.Model(S, alpha=a, device=device) for a in alphas]
        ck = {} if clocks is None else clocks
        sols = drone_gaussian_ipm.solve_batch(models, tol=tol, max_iter=int(maxiter), backend='device', clocks=ck,
                                              results_dir=results_dir, driver=driver, chol=chol)
        for m, (Z, info) in zip(models, sols):
            results.append(_drone_gaussian_ipm_result(m, Z, info, m.device_callbacks()["trajectory"],
                                                      ck["callbacks"] / len(models), ck["wall"] / len(models)))
    else:
        for a in alphas:
            model = drone_gaussian.Model(S, alpha=a, device=device)
            results.append(run_drone_gaussian(model, maxiter=maxiter, results_dir=results_dir))
    for a, r in zip(alphas, results):
        save_results(os.path.join(results_dir, f"drone_gaussian_alpha={a}.npy"), r["us"], r["xs"])
    wall = time.perf_counter() - t0
    us = np.stack([r["us"] for r in results])
    np.random.seed(seed)
    mc_model = drone_risk.Model(S, *sample_uncertain_parameters('saa', M=int(M_mc), S=S, dt=P.T / S), 'saa', alphas[0],
                                device=device)
    Z, _ = mc_model.eval_batch_device(us, want_stats=False)
    Z = Z.double().cpu().numpy()[:, :int(M_mc)]
    return {"alphas": alphas, "results": results, "status": np.array([r["status"] for r in results]), "us": us, "Z": Z,
            "percentage_safe": np.mean(Z <= 1e-6, axis=1), "cost": np.array([mc_model.monte_carlo_cost(u) for u in us]),
            "wall_s": wall}


def run_hopper(model, Z0=None, tol=1e-3, max_iter=3000, backend='device', newton='dense', driver='host', chol='workgroup'):
    """The hopper script's solve block (hopper.py:642-670) for one model: ``hopper_ipm.solve_batch`` in IPOPT's place, from
    ``Z0`` (default ``model.initial_guess()``) -> dict(Z, xs (S+1, 8), us (S, 4), status, info, total_s).  status is
    'converged' only if the final error E_0 <= tol shows it.  newton: 'dense' or 'arrow' (``hopper_ipm.solve_batch``).
    ``driver``: 'host', 'device' or 'device_grid' (``ipm.solve_group_device``: the iterate stays on the device; backend='device', either
    newton, 'arrow' with a precision='f64' model).  ``chol``: 'workgroup' or 'grid' (the device Cholesky)."""
    t0 = time.perf_counter()
    Z, info = model.solve(Z0, tol=tol, max_iter=max_iter, backend=backend, newton=newton, driver=driver, chol=chol)
    xs, us = model.convert_z_to_xs_us_mats(Z)
    return {"Z": Z, "xs": xs, "us": us, "status": info["status"], "info": info, "total_s": time.perf_counter() - t0}


def hopper_result_path(results_dir, method, alpha=None):
    """hopper.py:672-680: hopper_base_results.npy / hopper_saa_alpha=<alpha>_results.npy"""
    name = "hopper_base_results.npy" if method == 'baseline' else f"hopper_saa_alpha={alpha}_results.npy"
    return os.path.join(results_dir, name)


def save_hopper_result(results_dir, model, Z):
    """xs then us in one file, as the script writes them (:672-680) -> the path"""
    os.makedirs(results_dir, exist_ok=True)
    path = hopper_result_path(results_dir, model.method, model.alpha)
    xs, us = model.convert_z_to_xs_us_mats(Z)
    save_results(path, xs, us)
    return path


def hopper_saa_start(model, xs, us):
    """the script's SAA start (:470-479): the baseline's states and controls, ys = slack = t_risk = 0"""
    from . import hopper
    Z0 = np.zeros(model.num_vars)
    nX = hopper.n_x * (model.S + 1)
    Z0[:nX] = np.asarray(xs, dtype=np.float64).reshape(-1)
    Z0[nX:nX + hopper.n_u * model.S] = np.asarray(us, dtype=np.float64).reshape(-1)
    return Z0


HOPPER_MC_REPORT = "hopper_monte_carlo_report.npy"
HOPPER_MC_REPORT_ARRAYS = ("alphas", "jump", "frac_satisfied", "var", "avar")


def _hopper_mc_alphas(alphas, K):
    """``alphas`` of ``hopper_monte_carlo_report`` -> a list of K floats / None (None, or anything <= 0: the baseline's row)"""
    al = [alphas] * K if (alphas is None or np.ndim(alphas) == 0) else list(alphas)
    if len(al) != K:
        raise ValueError(f"alphas must be a scalar or a sequence of {K} entries, got {len(al)}")
    return [None if (a is None or not float(a) > 0.0) else float(a) for a in al]


def hopper_monte_carlo_report(mc_model, Zs, alphas, verbose=False, batch=True, selection='entry'):
    """The hopper script's Monte-Carlo block (hopper.py:960-1007) for K solutions ``Zs`` (their NLP vectors; only the states and
    controls are read) on the validation fields of ``mc_model`` (a ``hopper.Model`` of M_mc samples): per solution the jumped
    distance x_S[0], the fraction of fields without slip and VaR / AVaR at the solution's alpha.  ``alphas``: a scalar or K
    entries; None (or 0, the script's ``alphas_and_base``) marks the baseline, for which the script prints no avar (:1003-1007):
    its ``var`` and ``avar`` are NaN.
    batch=True: ONE ``Model.eval_batch_device`` call (rato_hopper_eval_batch: all solutions in one launch, one selection launch
    per run of equal alphas) and one read-back of the K records beside the contact counts; a record whose VaR is NaN (a
    selection that gave up) falls back to ``Model.monte_carlo_statistics``, as ``monte_carlo_report`` does.  batch=False: the
    per-solution loop (``slip_device`` + ``stats.risk_stats`` per solution) -- the checker: every array is the same to the bit.
    selection='rows' (with batch=True): the K selections as ONE ``stats.risk_stats_rows_device`` call behind the rollouts, whatever
    the alphas are (``Model.eval_batch_device``).
    -> dict(alphas (K,) with 0.0 for the baseline, jump, frac_satisfied, var, avar (each (K,)), arg_counts (K, C) int64: over the
    samples that slip (Z > 1e-6), how often contact c -- the first that attains the maximum -- is the one; wall_s)."""
    from . import stats
    t0 = time.perf_counter()
    Zs = [np.asarray(Z, dtype=np.float64) for Z in Zs]
    K = len(Zs)
    al = _hopper_mc_alphas(alphas, K)
    px, forces = mc_model.contact_inputs_batch(Zs)
    Cn = px.shape[1]
    jump = np.array([Z[8 * mc_model.S] for Z in Zs])             # xs[-1, 0] (hopper.py:987)
    frac, var, avar = (np.full(K, np.nan) for _ in range(3))
    counts = np.zeros((K, Cn), dtype=np.int64)
    thr = np.float32(stats.SATISFIED_THRESHOLD)

    def _take(k, st):
        frac[k] = st["frac_satisfied"]
        if al[k] is not None:
            var[k], avar[k] = st["var"], st["cvar"]

    if batch:
        import torch
        Zd, rec, arg = mc_model.eval_batch_device(px, forces, alphas=al, want_arg=True, selection=selection)
        # the contact counts over the unsafe samples, on the device, so that ONE tensor comes back: [records | counts]
        unsafe = (Zd > float(thr)) & (arg >= 0)
        cnt = torch.zeros((K, Cn), dtype=torch.float64, device=Zd.device)
        cnt.scatter_add_(1, arg.clamp(min=0).long(), unsafe.double())
        back = torch.cat([rec, cnt], dim=1).cpu().numpy()
        counts[:] = np.rint(back[:, stats.N_STATS:]).astype(np.int64)
        for k in range(K):
            st = dict(zip(stats._STAT_NAMES, back[k, :stats.N_STATS].tolist()))
            if np.isnan(st["var"]):
                st = mc_model.monte_carlo_statistics(px[k], forces[k], alpha=1.0 if al[k] is None else al[k])
            _take(k, st)
    else:
        for k in range(K):
            r = mc_model.slip_device(px[k], forces[k])
            _take(k, stats.risk_stats(r["Z"], 1.0 if al[k] is None else al[k]))
            h = r["h"].cpu().numpy()                             # (C, M)
            h = np.where(np.isnan(h), -np.inf, h)
            z = h.max(axis=0)
            first = np.argmax(h, axis=0)
            counts[k] = np.bincount(first[z > thr], minlength=Cn)
    out = {"alphas": np.array([0.0 if a is None else a for a in al]), "jump": jump, "frac_satisfied": frac, "var": var,
           "avar": avar, "arg_counts": counts}
    if verbose:                                                  # hopper.py:984-1007
        for k in range(K):
            print("---------------------------")
            print("Monte-Carlo: alpha =", out["alphas"][k])
            print("jumped distance =", jump[k])
            print("B_satisfied_vec =", frac[k])
            if al[k] is not None:
                print("avar =", avar[k])
        print("---------------------------------------")
    out["wall_s"] = time.perf_counter() - t0
    return out


def save_hopper_monte_carlo_report(results_dir, report):
    """alphas, jump, frac_satisfied, var, avar of a ``hopper_monte_carlo_report`` in one file (``load_results(path, 5)``) -> path"""
    os.makedirs(results_dir, exist_ok=True)
    path = os.path.join(results_dir, HOPPER_MC_REPORT)
    save_results(path, *(report[k] for k in HOPPER_MC_REPORT_ARRAYS))
    return path


def _check_validate(validate):
    if validate not in ('solo', 'batch'):
        raise ValueError(f"validate must be 'solo' or 'batch', got {validate!r}")


def hopper_experiment(alphas=(0.05, 0.1, 0.2, 0.3, 0.5, 0.75), M=30, S=30, seed=1, results_dir=None, tol=1e-3, max_iter=3000,
                      backend='device', device='cuda:0', clocks=None, newton='dense', fields=None, driver='host',
                      chol='workgroup', M_mc=None):
    """The hopper script's two runs (hopper.py:455-680) as one call: the friction fields under ``RandomState(seed)`` (:70-74),
    the baseline from ``initial_guess()``, then every alpha of the SAA problem in ONE lockstep batch from the baseline's
    solution (:465-479).  With ``results_dir`` the files hopper_base_results.npy and hopper_saa_alpha=<a>_results.npy are
    written (xs then us, ``save_results``), whatever the status.  ``fields``: (intensities, thetas, taus), each (M, 30), in place
    of the draw; ``newton``: 'dense' or 'arrow' (``hopper_ipm.solve_batch``: 'arrow' is the one that scales with M); ``driver``:
    'host', 'device' or 'device_grid' (``ipm.solve_group_device``: the iterate stays on the device; backend='device', either newton).
    -> dict(alphas, base (the run_hopper dict), results [alpha] (dict(Z, xs, us, status, info)), status (A,) of str, wall_s)
    ``chol``: 'workgroup' or 'grid', the device Cholesky of both runs (``hopper_ipm.solve_batch``; the results do not depend on it).
    ``M_mc``: None (default) -- nothing more; an integer -- the script's Monte-Carlo block (:960-1007) on ``M_mc`` validation fields
    drawn after the model's fields under the same ``RandomState(seed)`` (the draw order of ``draw_hopper_saa_fields(1, M, M_mc,
    seed)``): ``hopper_monte_carlo_report`` of the alphas and then the baseline, the script's order, returned under
    "monte_carlo" (the validation fields under "mc_fields") and, with ``results_dir``, written to hopper_monte_carlo_report.npy
    (alphas, jump, frac_satisfied, var, avar: ``load_results(path, 5)``)."""
    from . import ipm as _ipm
    _ipm.check_chol(chol)
    from . import hopper, hopper_ipm
    alphas = [float(a) for a in alphas]
    mc_fields = None
    if M_mc is not None:
        draws, mc_fields = draw_hopper_saa_fields(1, M, int(M_mc), seed)
        if fields is None:
            fields = draws[0]
    if fields is None:
        fields = hopper.sample_friction_fields(M, np.random.RandomState(seed))
    t0 = time.perf_counter()
    base_model = hopper.Model(M, 'baseline', S=S, fields=fields, device=device, precision='f64')
    c0 = {}
    (Zb, ib), = hopper_ipm.solve_batch([base_model], tol=tol, max_iter=max_iter, backend=backend, clocks=c0,
                                        newton=newton, driver=driver, chol=chol)
    xs, us = base_model.convert_z_to_xs_us_mats(Zb)
    base = {"Z": Zb, "xs": xs, "us": us, "status": ib["status"], "info": ib}
    models = [hopper.Model(M, 'saa', a, S=S, fields=fields, device=device, precision='f64') for a in alphas]
    c1 = {}
    sols = hopper_ipm.solve_batch(models, [hopper_saa_start(m, xs, us) for m in models], tol=tol, max_iter=max_iter,
                                  backend=backend, clocks=c1, newton=newton, driver=driver, chol=chol) if models else []
    results = []
    for m, (Z, info) in zip(models, sols):
        x, u = m.convert_z_to_xs_us_mats(Z)
        results.append({"Z": Z, "xs": x, "us": u, "status": info["status"], "info": info})
    if clocks is not None:
        clocks["base"], clocks["saa"] = c0, c1
    if results_dir is not None:
        save_hopper_result(results_dir, base_model, Zb)
        for m, r in zip(models, results):
            save_hopper_result(results_dir, m, r["Z"])
    out = {"alphas": alphas, "base": base, "results": results, "status": np.array([r["status"] for r in results])}
    if mc_fields is not None:
        mc_model = hopper.Model(int(M_mc), 'saa', S=S, fields=mc_fields, device=device)
        out["monte_carlo"] = hopper_monte_carlo_report(mc_model, [r["Z"] for r in results] + [Zb], alphas + [None])
        out["mc_fields"] = mc_fields
        if results_dir is not None:
            save_hopper_monte_carlo_report(results_dir, out["monte_carlo"])
    out["wall_s"] = time.perf_counter() - t0
    return out


def draw_hopper_saa_fields(num_repeats=30, M=30, M_mc=10000, seed=1):
    """The friction fields of ``hopper_saa_experiment`` in its draw order, under ONE ``RandomState(seed)``: repeat 0 .. R-1 each
    draw ``hopper.sample_friction_fields(M, rng)`` in sequence (with the default seed repeat 0 is bitwise ``hopper_experiment``'s
    draw), then the ``M_mc`` validation fields, last.  Host only.  -> ([repeat] of (intensities, thetas, taus), each (M, 30); the
    validation triple, each (M_mc, 30))"""
    from . import hopper
    rng = np.random.RandomState(seed)
    repeats = [hopper.sample_friction_fields(M, rng) for _ in range(int(num_repeats))]
    return repeats, hopper.sample_friction_fields(int(M_mc), rng)


def hopper_saa_result_path(results_dir, alpha, repeat):
    """hopper_saa_alpha=<alpha>_repeat=<r>_results.npy"""
    return os.path.join(results_dir, f"hopper_saa_alpha={alpha}_repeat={repeat}_results.npy")


HOPPER_SAA_REPORT = "hopper_saa_grid_report.npy"
HOPPER_SAA_REPORT_ARRAYS = ("alphas", "status", "jump", "safe_fraction", "var", "avar")


def hopper_saa_experiment(alphas=(0.05, 0.1, 0.2, 0.3, 0.5, 0.75), num_repeats=30, M=30, S=30, seed=1, M_mc=10000, results_dir=None,
                          tol=1e-3, max_iter=3000, newton='dense', driver='host', device='cuda:0', clocks=None,
                          chol='workgroup', validate='solo'):
    """The hopper's SAA study over resampled terrains, shaped like ``drone_saa_experiment`` / ``driving_saa_experiment``: R draws
    of the friction fields (``draw_hopper_saa_fields``), the baseline solved once from ``initial_guess()`` (its fields are zeroed,
    so it does not depend on the draw), then all A x R SAA problems -- alpha-major, every repeat on its own fields -- in ONE
    ``hopper_ipm.solve_batch`` call (one lockstep group) from ``hopper_saa_start`` of the baseline's solution, and the script's
    Monte-Carlo validation (hopper.py:960-1007) of every solution on the ``M_mc`` validation fields: px and the contact forces
    on the contact steps (``Model.contact_inputs``), ``Model.monte_carlo_statistics`` at the problem's alpha, one solution after
    the other (validate='solo', the default) -- or all A x R solutions in ONE ``Model.eval_batch_device`` call (validate='batch':
    rato_hopper_eval_batch; the stacking is alpha-major, so the selections are A launches); every returned array is the same to
    the bit under both, any other value is a ValueError before any work.
    A problem that does not converge raises nothing: its status says so and it is validated like the others.
    -> dict(alphas, base (the run_hopper dict without total_s), results [alpha][repeat] = (Z, xs, us, status, info), status (A, R)
    of str, jump (A, R) = x_S[0], safe_fraction / var / avar (A, R), wall_s).
    With ``results_dir``: hopper_saa_alpha=<a>_repeat=<r>_results.npy per problem (xs then us, ``save_results``) and one
    hopper_saa_grid_report.npy holding, in this order, alphas (A,), status (A, R), jump, safe_fraction, var, avar (each (A, R)):
    ``load_results(path, 6)``.  ``chol``: 'workgroup' or 'grid', the device Cholesky (the results do not depend on it)."""
    from . import hopper, hopper_ipm
    from . import ipm as _ipm
    _ipm.check_chol(chol)
    _check_validate(validate)
    alphas = [float(a) for a in alphas]
    A, R = len(alphas), int(num_repeats)
    draws, mc_fields = draw_hopper_saa_fields(R, M, M_mc, seed)
    t0 = time.perf_counter()
    kw = dict(tol=tol, max_iter=max_iter, backend='device', newton=newton, driver=driver, chol=chol)
    zero = np.zeros((M, hopper.num_mu_features))                 # what Model makes of any baseline's fields
    base_model = hopper.Model(M, 'baseline', S=S, fields=(zero, zero, zero), device=device, precision='f64')
    c0, c1 = {}, {}
    (Zb, ib), = hopper_ipm.solve_batch([base_model], clocks=c0, **kw)
    xs, us = base_model.convert_z_to_xs_us_mats(Zb)
    base = {"Z": Zb, "xs": xs, "us": us, "status": ib["status"], "info": ib}
    models = [hopper.Model(M, 'saa', a, S=S, fields=draws[r], device=device, precision='f64') for a in alphas for r in range(R)]
    sols = hopper_ipm.solve_batch(models, [hopper_saa_start(m, xs, us) for m in models], clocks=c1, **kw) if models else []
    mc_model = hopper.Model(int(M_mc), 'saa', S=S, fields=mc_fields, device=device)
    results = [[None] * R for _ in alphas]
    status = np.empty((A, R), dtype='U16')
    jump, safe, var, avar = (np.zeros((A, R)) for _ in range(4))
    for k, (m, (Z, info)) in enumerate(zip(models, sols)):
        i, r = divmod(k, R)
        x, u = m.convert_z_to_xs_us_mats(Z)
        results[i][r] = (Z, x, u, info["status"], info)
        status[i, r], jump[i, r] = info["status"], x[-1, 0]
        if validate == 'solo':
            px, forces = m.contact_inputs(Z)
            st = mc_model.monte_carlo_statistics(px, forces, alpha=m.alpha)
            safe[i, r], var[i, r], avar[i, r] = st["frac_satisfied"], st["var"], st["cvar"]
    if validate == 'batch' and models:
        from . import stats
        inputs = [m.contact_inputs(Z) for m, (Z, _) in zip(models, sols)]
        _, rec = mc_model.eval_batch_device(np.stack([p for p, _ in inputs]), np.stack([f for _, f in inputs]),
                                            alphas=[m.alpha for m in models])
        rec = rec.cpu().numpy()
        for k, m in enumerate(models):
            st = dict(zip(stats._STAT_NAMES, rec[k].tolist()))
            if np.isnan(st["var"]):                    # (a selection that gave up: the recovering per-solution path)
                st = mc_model.monte_carlo_statistics(*inputs[k], alpha=m.alpha)
            i, r = divmod(k, R)
            safe[i, r], var[i, r], avar[i, r] = st["frac_satisfied"], st["var"], st["cvar"]
    if clocks is not None:
        clocks["base"], clocks["saa"] = c0, c1
    out = {"alphas": alphas, "base": base, "results": results, "status": status, "jump": jump, "safe_fraction": safe, "var": var,
           "avar": avar, "wall_s": time.perf_counter() - t0}
    if results_dir is not None:
        os.makedirs(results_dir, exist_ok=True)
        for i, a in enumerate(alphas):
            for r in range(R):
                save_results(hopper_saa_result_path(results_dir, a, r), results[i][r][1], results[i][r][2])
        save_results(os.path.join(results_dir, HOPPER_SAA_REPORT), np.asarray(alphas), *(out[k] for k in HOPPER_SAA_REPORT_ARRAYS[1:]))
    return out
