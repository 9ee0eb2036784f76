"""GPU: the L3/L4 boundary on the device path — sparse QP rows from the HIP linearization vs the
oracle's, and SCP iterates (device linearization) vs SCP iterates (fp64 oracle linearization) with
the same host QP solver: the north star's "SCP iterates matching reference to 1e-5"."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _drone(M, S, alpha=0.2, method='saa', seed=0):
    from oracle import drone as od
    from riskaversetrajopt_amd import drone_risk
    DWs, masses, Q = od.sample_uncertain_parameters(np.random.RandomState(seed), method, M=M, S=S)
    return od.Model(S, DWs, masses, Q, method, alpha), drone_risk.Model(S, DWs, masses, Q, method, alpha)


def _car(M, S, alpha=0.1, method='saa', seed=0):
    from oracle import driving as ocar
    from riskaversetrajopt_amd import driving
    samples = ocar.sample_uncertain_parameters(np.random.RandomState(seed), M, method, S)
    return ocar.Model(*samples, method=method, alpha=alpha), driving.Model(M, method, alpha, S=S, samples=samples)


def graze(S):
    t = np.arange(S)[:, None]
    return np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)]) * (20.0 / S)


@pytest.mark.parametrize("method", ["saa", "baseline"])
@pytest.mark.parametrize("scp_iter", [0, 2])
def test_drone_sparse_rows_vs_oracle(method, scp_iter):
    from tests._oracle_qp import DroneOracleQP
    S, M = 20, 37
    o, d = _drone(M, S, method=method)
    us = graze(S)
    A, l, u = d.get_constraints_coeffs(us, scp_iter)
    Ao, lo, uo = DroneOracleQP(o).get_constraints_coeffs(us, scp_iter)
    assert A.shape == Ao.shape and np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
    scale = np.abs(Ao.data).max()
    assert np.max(np.abs(A.data - Ao.data)) < 2e-5 * scale
    fin = np.isfinite(lo)
    np.testing.assert_array_equal(np.isfinite(l), fin)
    np.testing.assert_allclose(l[fin], lo[fin], rtol=1e-5, atol=2e-5)
    fin = np.isfinite(uo)
    np.testing.assert_allclose(u[fin], uo[fin], rtol=1e-4, atol=5e-6)
    P, q = d.get_objective_coeffs()
    Po, qo = DroneOracleQP(o).get_objective_coeffs()
    assert (P != Po).nnz == 0 and np.array_equal(q, qo)
    Ad, low, up = d.get_all_constraints_coeffs_all(us)
    Ado, lowo, upo = o.get_all_constraints_coeffs_all(us)
    assert Ad.shape == Ado.shape and np.array_equal(Ad != 0, Ado != 0)


def test_driving_sparse_rows_vs_oracle():
    from tests._oracle_qp import DrivingOracleQP
    S, M = 20, 19
    o, d = _car(M, S)
    t = np.arange(S)[:, None]
    us = np.hstack([0.4 * np.cos(0.4 * t) - 0.2, 0.05 * np.sin(0.35 * t) + 0.01])
    for scp_iter in (0, 1):
        A, l, u = d.get_constraints_coeffs(us, scp_iter)
        Ao, lo, uo = DrivingOracleQP(o).get_constraints_coeffs(us, scp_iter)
        assert np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
        assert np.max(np.abs(A.data - Ao.data)) < 1e-4 * np.abs(Ao.data).max()
        fin = np.isfinite(uo)
        np.testing.assert_allclose(u[fin], uo[fin], rtol=1e-4, atol=2e-4)


def test_drone_scp_iterates_match_oracle_path():
    from riskaversetrajopt_amd import scp
    from tests._oracle_qp import DroneOracleQP
    S, M = 20, 30
    o, d = _drone(M, S, alpha=0.2)
    ref = scp.run_drone(DroneOracleQP(o), num_scp_iters_max=25, warmup_iters=1)
    out = scp.run_drone(d, num_scp_iters_max=25, warmup_iters=1)
    assert ref["L2_error"][-1] < 1e-5 and out["L2_error"][-1] < 1e-5          # both converge
    # North star: "SCP iterates matching reference to 1e-5".  Converged iterates agree to 1e-5 ABSOLUTE on controls
    # bounded by u_max = 10 (measured on MI355X, tools/scp_tol.py: 1e-7 .. 6e-7 over the last five iterations for
    # M = 30 and M = 50; both legs polished).  Along the path the difference is below 1e-6 except at the one iteration
    # where the CVaR rows are switched on (scp_iter = 2, drone_risk.py:413-417): there the subproblem's optimiser is
    # ill-conditioned in the linearization and one step differs by up to 1.2e-2 before contracting again.
    np.testing.assert_allclose(out["us"], ref["us"], rtol=0, atol=1e-5)
    assert abs(out["t_risk"] - ref["t_risk"]) < 1e-5
    # Monte-Carlo validation on fresh samples through the device path (drone_risk.py:643-725)
    from oracle import drone as od
    from riskaversetrajopt_amd import drone_risk
    DWs, masses, Q = od.sample_uncertain_parameters(np.random.RandomState(123), 'saa', M=10000, S=S)
    mc = drone_risk.Model(S, DWs, masses, Q, 'saa', 0.2)
    st = mc.monte_carlo_statistics(out["us"], alpha=0.2)
    assert 0.0 <= st["frac_satisfied"] <= 1.0 and st["cvar"] >= st["var"]
    assert st["cvar"] < 0.5                 # out-of-sample AVaR stays near the constraint level


def test_driving_scp_iterates_match_oracle_path():
    from riskaversetrajopt_amd import scp
    from tests._oracle_qp import DrivingOracleQP
    S, M = 20, 16
    o, d = _car(M, S, alpha=0.1)
    ref = scp.run_driving(DrivingOracleQP(o), num_scp_iters_max=10)
    out = scp.run_driving(d, num_scp_iters_max=10)
    # 1e-5 absolute on controls bounded by u_max = 100 (measured: 6e-8 at the last iteration, <= 1.4e-6 along the
    # whole path for M = 16; tools/scp_tol.py)
    np.testing.assert_allclose(out["us"], ref["us"], rtol=0, atol=1e-5)
    assert abs(out["t_risk"] - ref["t_risk"]) < 1e-5
    assert np.all(np.isfinite(out["define_s"])) and out["cumulative_s"][-1] > 0


@pytest.mark.parametrize("method", ["saa", "baseline"])
def test_device_emitted_csc_values_match_host_assembly(method):
    """rato_emit_csc_values + cached pattern == host assembly (same pattern; values to fp32 rounding)."""
    S, M = 20, 130
    _, d = _drone(M, S, method=method)
    for scp_iter, scale in ((0, 1.0), (2, 1.0), (5, 0.7)):
        us = graze(S) * scale
        A, l, u = d.get_constraints_coeffs(us, scp_iter)
        Ah, lh, uh = d.get_constraints_coeffs_host(us, scp_iter)
        assert np.array_equal(A.indptr, Ah.indptr) and np.array_equal(A.indices, Ah.indices)
        np.testing.assert_allclose(A.data, Ah.data, rtol=3e-7, atol=1e-30)
        np.testing.assert_allclose(l, lh, rtol=1e-12, atol=0)
        np.testing.assert_allclose(u, uh, rtol=3e-7, atol=1e-12)
    assert d._fast.ok
    _, c = _car(70, 20, method=method)
    t = np.arange(20)[:, None]
    us = np.hstack([0.4 * np.cos(0.4 * t) - 0.2, 0.05 * np.sin(0.35 * t) + 0.01])
    for scp_iter in (0, 1, 3):
        A, l, u = c.get_constraints_coeffs(us, scp_iter)
        Ah, lh, uh = c.get_constraints_coeffs_host(us, scp_iter)
        assert np.array_equal(A.indptr, Ah.indptr) and np.array_equal(A.indices, Ah.indices)
        np.testing.assert_allclose(A.data, Ah.data, rtol=3e-7, atol=1e-30)
        np.testing.assert_allclose(u, uh, rtol=3e-7, atol=1e-12)


def test_reduced_cutting_plane_solve_equals_full_qp():
    """Eliminating y_i / t and solving in (u, slack) by CVaR cuts gives the optimum of the reference's QP."""
    S, M = 20, 40
    _, d = _drone(M, S, alpha=0.2)
    us_prev = graze(S) * 0.5
    from riskaversetrajopt_amd import scp
    # (a) at an arbitrary iterate: the reduced solution lifts to a FEASIBLE point of the reference's full QP
    #     (y_i = max(-slack, m_i - t), t = VaR + slack) with the same objective -> it is the full QP's optimum,
    #     because the master only ever holds valid cuts (outer approximation).
    A, l, u = d.get_constraints_coeffs(us_prev, 2)
    Pm, q = d.get_objective_coeffs()
    us_red, t_red, info = d.solve_reduced(us_prev, 2)
    assert info["cuts"] >= 1 and info["status"] == 'solved'
    nU = 3 * S
    rows = (A[7 + M:7 + M + M * 3 * S, :nU] @ us_red.reshape(-1) - u[7 + M:7 + M + M * 3 * S]) / 0.01   # (G_i u - g_up_i)_r
    m_i = rows.reshape(M, 3 * S).max(axis=1)
    y = np.maximum(-info["slack"], m_i - t_red)
    z = np.concatenate([us_red.reshape(-1), y, [info["slack"], t_red]])
    Az = A @ z
    # tolerance: A / u carry the fp32 rounding of the products W * Phi and of g_up = -g + G u_k (|g_up| ~ 1e2), which
    # the oracle's delta form g + G (u - u_k) does not; the CVaR sum row adds M of those differences
    tol_rows = np.full(A.shape[0], 2e-5)
    tol_rows[6] = 1e-5 * M * max(1.0, np.abs(m_i).max())
    assert np.all(Az <= u + tol_rows) and np.all(Az >= l - tol_rows), (np.max(Az - u), np.max(l - Az))
    # (b) along the SCP path (where the full QP is well conditioned) both solves give the same iterate
    start = scp.run_drone(d, num_scp_iters_max=4, warmup_iters=0)["us"]
    d.update_problem(start, 4)
    us_full, t_full = d.solve(verbose=False)
    assert d.res.info.status == 'solved'
    us_red2, t_red2, info2 = d.solve_reduced(start, 4)
    np.testing.assert_allclose(us_red2, us_full, rtol=0, atol=1e-5)
    assert abs(t_red2 - t_full) < 1e-5 and abs(info2["slack"] - d.res.x[-2]) < 1e-5
    # scp_iter < 2: every CVaR row is relaxed away (drone_risk.py:413-417; y, t are then free and the full QP
    # is degenerate), what remains is the minimum-effort control meeting the final constraints
    us_red0, _, info0 = d.solve_reduced(us_prev, 0)
    F, f = A[:6, :3 * S].toarray(), l[:6]
    Pu = Pm[:3 * S, :3 * S].toarray()
    K = np.block([[Pu, F.T], [F, np.zeros((6, 6))]])
    sol = np.linalg.solve(K, np.concatenate([np.zeros(3 * S), f]))
    assert info0["cuts"] == 0 and np.all(np.abs(sol[:3 * S]) < 10)
    np.testing.assert_allclose(us_red0.reshape(-1), sol[:3 * S], rtol=0, atol=1e-6)
    # ... and the slack sits at the minimiser of its penalty: the relaxation covers its row too (:413-417)
    assert abs(info0["slack"] + 1.0) < 1e-9 and info0["t_risk"] == 0.0
    d.update_problem(us_prev, 0)
    d.solve(verbose=False)
    assert abs(d.res.x[-2] + 1.0) < 1e-6
    np.testing.assert_allclose(d.res.x[:3 * S], us_red0.reshape(-1), rtol=0, atol=1e-6)


def test_reduced_scp_matches_full_scp_and_scales():
    from riskaversetrajopt_amd import scp
    S, M = 20, 30
    o, d = _drone(M, S, alpha=0.2)
    full = scp.run_drone(d, num_scp_iters_max=15, warmup_iters=0)
    _, d2 = _drone(M, S, alpha=0.2)
    red = scp.run_drone_reduced(d2, num_scp_iters_max=15)
    # North star: "SCP iterates matching reference to 1e-5" on the path the benchmark times (generators-only
    # linearization, Jacobian-free fp64 oracle in delta form, recycled cuts)
    np.testing.assert_allclose(red["us"], full["us"], rtol=0, atol=1e-5)
    assert abs(red["t_risk"] - full["t_risk"]) < 1e-5
    # ... and against the fp64 oracle's linearization through the full QP (the "reference" leg)
    from tests._oracle_qp import DroneOracleQP
    ref = scp.run_drone(DroneOracleQP(o), num_scp_iters_max=15, warmup_iters=0)
    np.testing.assert_allclose(red["us"], ref["us"], rtol=0, atol=1e-5)
    # a batch no host QP could take (3e6 rows): the reduced path still converges
    _, big = _drone(20000, S, alpha=0.1, seed=3)
    out = scp.run_drone_reduced(big, num_scp_iters_max=8)
    assert np.isfinite(out["us"]).all() and out["L2_error"][-1] < 0.05
    st = big.monte_carlo_statistics(out["us"], alpha=0.1)
    assert st["cvar"] < 0.1          # in-sample CVaR of the (nonlinear) constraint is near/below 0


def test_driving_reduced_scp_matches_full_scp():
    from riskaversetrajopt_amd import scp
    S, M = 20, 16
    _, d = _car(M, S, alpha=0.1)
    full = scp.run_driving(d, num_scp_iters_max=10)
    _, d2 = _car(M, S, alpha=0.1)
    red = scp.run_driving_reduced(d2, num_scp_iters_max=10)
    np.testing.assert_allclose(red["us"], full["us"], rtol=0, atol=1e-5)
    assert abs(red["t_risk"] - full["t_risk"]) < 1e-5
    assert red["cuts"][0] == 0 and red["cuts"][1:].max() >= 1
    _, big = _car(30000, S, alpha=0.05, seed=2)
    out = scp.run_driving_reduced(big, num_scp_iters_max=6)
    assert np.isfinite(out["us"]).all()
    st = big.monte_carlo_statistics(out["us"], alpha=0.05)
    assert st["cvar"] < 0.2


@pytest.mark.parametrize("S,M", [(20, 300), (50, 1000), (2, 5), (125, 70)])
def test_rowmax_implicit_matches_explicit_and_oracle(S, M):
    """m_i(u) = max_r (G_i u - g_up_i)_r from the step-Jacobian table (O(S) recursion, no Jacobian read) ==
    the same from the packed Jacobian == the fp64 oracle's dense g_obs_du @ u."""
    import ctypes as C
    import torch
    from riskaversetrajopt_amd import _lib
    o, d = _drone(M, S)
    us = graze(S)
    r = d.linearize_device(us, want_A22=True)
    assert r["A22"].shape == (S, 2, M)
    rng = np.random.RandomState(4)
    u_new = us + 0.3 * rng.randn(S, 3)
    u_dev = torch.as_tensor(u_new, dtype=torch.float64, device=r["G"].device).contiguous()
    lib = d._lib
    ld = r["_g_up"].shape[-1]
    dW, mass, Qsym, _ = d._inputs(None)
    out = {}
    for name in ("explicit", "implicit"):
        m = torch.empty(M, dtype=torch.float32, device=u_dev.device)
        a = torch.empty(M, dtype=torch.int32, device=u_dev.device)
        if name == "explicit":
            _lib.check(lib.rato_saa_rowmax(_lib.ptr(r["G"]), _lib.ptr(r["_W"]), r["tile"], 3, S, M, ld,
                                           _lib.ptr(r["_g_up"]), -1.0, _lib.ptr(u_dev), 3, _lib.ptr(m), _lib.ptr(a),
                                           _lib.current_stream()), "rato_saa_rowmax")
        else:
            p = d._params(M, ld)
            _lib.check(lib.rato_drone_rowmax_implicit(C.byref(p), _lib.ptr(mass), _lib.ptr(r["_A22"]), 2,
                                                      _lib.ptr(r["_W"]), _lib.ptr(r["_g_up"]), -1.0, _lib.ptr(u_dev),
                                                      _lib.ptr(m), _lib.ptr(a), _lib.current_stream()),
                       "rato_drone_rowmax_implicit")
        out[name] = (m.cpu().numpy().astype(np.float64), a.cpu().numpy())
    # oracle: dense fp64 rows
    _, _, _, gdu_o, gup_o = o.get_all_constraints_coeffs(us)                  # (M,3,S,3S), (M,3,S)
    rows = (gdu_o.reshape(M, 3 * S, 3 * S) @ u_new.reshape(-1)) - gup_o.reshape(M, 3 * S)
    m_o, a_o = rows.max(axis=1), rows.argmax(axis=1)
    scale = max(1.0, np.abs(rows).max())
    for name in ("explicit", "implicit"):
        m, a = out[name]
        assert np.max(np.abs(m - m_o)) < 2e-4 * scale, (name, np.max(np.abs(m - m_o)))
        srt = np.sort(rows, axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > 1e-3 * scale if S * 3 > 1 else np.ones(M, bool)
        assert np.array_equal(a[clear], a_o[clear]), name
    assert np.max(np.abs(out["implicit"][0] - out["explicit"][0])) < 2e-5 * scale


def test_reduced_solve_implicit_equals_explicit_oracle_path():
    from riskaversetrajopt_amd import scp
    S, M = 20, 2000
    _, d = _drone(M, S, alpha=0.1, seed=5)
    start = scp.run_drone_reduced(d, num_scp_iters_max=6)["us"]      # a point on the SCP path (slack ~ 0)
    us_i, t_i, info_i = d.solve_reduced(start, 6, implicit=True)
    us_e, t_e, info_e = d.solve_reduced(start, 6, implicit=False)
    assert info_i["status"] == info_e["status"] == 'solved' and info_i["cuts"] >= 1
    assert info_i["slack"] < 1e-3
    np.testing.assert_allclose(us_i, us_e, rtol=0, atol=1e-5)
    assert abs(t_i - t_e) < 1e-5 and abs(info_i["slack"] - info_e["slack"]) < 1e-6
    us_r, t_r, info_r = d.solve_reduced(start, 6, delta=False)        # the reference's form G u - g_up (fp32 g_up)
    np.testing.assert_allclose(us_r, us_i, rtol=0, atol=5e-5)
    # far from the path (huge slack) the optimum is flat in u: same objective, not the same u
    far = graze(S) * 0.7
    _, _, fi = d.solve_reduced(far, 3, implicit=True)
    _, _, fe = d.solve_reduced(far, 3, implicit=False)
    Pd, q = d._cut_solver.P.toarray(), d._cut_solver.q
    obj = lambda f: (lambda z: 0.5 * z @ Pd @ z + q @ z)(np.concatenate([f["us"].reshape(-1), [f["slack"]]]))
    assert abs(obj(fi) - obj(fe)) < 1e-6 * abs(obj(fe))


def test_recycled_cuts_are_valid_and_do_not_change_the_iterates():
    """Cuts kept from one SCP iteration and re-linearized against the next one (rato_saa_tail_rows_batch) are
    valid lower bounds of the new CVaR function, tight where nothing changed, and leave the SCP path unchanged."""
    from riskaversetrajopt_amd import scp
    S, M = 20, 3000
    _, d = _drone(M, S, alpha=0.1, seed=7)
    start = scp.run_drone_reduced(d, num_scp_iters_max=5)["us"]
    us1, _, info1 = d.solve_reduced(start, 5)
    cs = d._cut_solver
    assert cs.recycle and len(cs.keep) >= 1
    # (the table-free oracle keeps no linearization at all: nothing but the samples and u_k stands behind the kept cuts)
    r = {"G": None, "_W": None, "tile": 64, "_g_up": None}
    assert cs.rollout is not None and cs.u_lin is not None
    rows, rhs = cs.relinearize_kept_cuts(r["G"], r["_W"], r["tile"], r["_g_up"])
    assert rows.shape == (len(cs.keep), 3 * S) and np.all(rows.reshape(-1, S, 3)[:, :, 2] == 0)
    rng = np.random.RandomState(1)
    best_at_solution = -np.inf
    for trial in range(6):
        u = us1.reshape(-1) + (0.0 if trial == 0 else 0.05) * rng.randn(3 * S)
        phi, _, _ = cs.evaluate(r["G"], r["_W"], r["tile"], r["_g_up"], u)
        lower = rows @ u - rhs
        assert np.all(lower <= phi + 1e-9 * max(1.0, abs(phi))), (trial, lower.max(), phi)      # valid cuts (fp64)
        if trial == 0:
            best_at_solution = lower.max() - phi
    assert abs(best_at_solution) < 1e-8                  # ... and tight at the point they were generated around
    # a different linearization point, the reference's form of the rows (g_up, no u_k): still valid
    r2 = d.linearize_device(start * 0.9, want_A22=True)
    cs.rollout = None                                    # (the table-free form has no reference form: tables from here on)
    cs.set_linearization_point(None)
    rows2, rhs2 = cs.relinearize_kept_cuts(r2["G"], r2["_W"], r2["tile"], r2["_g_up"])
    cs.implicit = (d._params(M, r2["_g_up"].shape[-1]), d._inputs(None)[1], r2["_A22"], 2)
    for trial in range(4):
        u = us1.reshape(-1) + 0.05 * rng.randn(3 * S)
        phi, _, _ = cs.evaluate(r2["G"], r2["_W"], r2["tile"], r2["_g_up"], u)
        # explicit rows (fp32 products W * Phi) against rows regenerated from A22: equal to fp32 rounding of Phi
        assert np.all(rows2 @ u - rhs2 <= phi + 2e-5 * max(1.0, abs(phi)))
    # same SCP path with and without recycling
    _, da = _drone(M, S, alpha=0.1, seed=7)
    _, db = _drone(M, S, alpha=0.1, seed=7)
    a = scp.run_drone_reduced(da, num_scp_iters_max=12)
    db.solve_reduced(db.initial_guess_us_mat(), 0)       # creates the solver
    db._cut_solver.recycle = False
    b = scp.run_drone_reduced(db, num_scp_iters_max=12)
    np.testing.assert_allclose(a["us"], b["us"], rtol=0, atol=1e-5)
    assert a["cuts"][-3:].sum() <= b["cuts"][-3:].sum()


@pytest.mark.parametrize("S,M", [(20, 300), (50, 1000), (2, 5), (125, 70)])
def test_generators_only_linearization_matches_the_jacobian_kernel(S, M):
    """rato_drone_linearize_generators (A22, W, g_up, Z, sums; no Jacobian entries) == the same quantities of the
    row-parallel Jacobian kernel, and the rows regenerated from A22 (rato_drone_tail_rows_implicit) == the rows read
    from Phi (rato_saa_tail_rows_batch)."""
    import ctypes as C
    import torch
    from riskaversetrajopt_amd import _lib, stats
    o, d = _drone(M, S)
    us = graze(S)
    full = d.linearize_device(us, want_A22=True)
    gen = d.linearize_generators_device(us)
    assert gen["G"] is None and gen["A22"].shape == (S, 3, M)
    # (the generators' table holds the complement 1 - a22, the row kernel's a22 itself)
    np.testing.assert_allclose(1.0 - gen["A22"][:, :2].double().cpu().numpy(), full["A22"].double().cpu().numpy(),
                               rtol=1e-6, atol=1e-7)
    Wf = full["W"].cpu().numpy()                     # W = -(Q+Q')(p - o): |Q| ~ 1e2..1e3 amplifies the last-bit
    np.testing.assert_allclose(gen["W"].cpu().numpy(), Wf, rtol=1e-5, atol=2e-5 * np.abs(Wf).max())   # differences of p
    np.testing.assert_allclose(gen["g_up"].cpu().numpy(), full["g_up"].cpu().numpy(), rtol=5e-5, atol=2e-4)
    np.testing.assert_allclose(gen["Z"].cpu().numpy(), full["Z"].cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(gen["sums"].cpu().numpy(), full["sums"].cpu().numpy(), rtol=2e-5, atol=2e-3)
    _, _, _, _, gup_o = o.get_all_constraints_coeffs(us)
    np.testing.assert_allclose(gen["g_up"].permute(2, 0, 1).cpu().numpy(), gup_o, rtol=5e-5, atol=2e-4)
    # the generators kernel computes in fp64 and rounds its outputs once: against the fp64 oracle its constraint values
    # carry the rounding of the fp32 INPUTS (noise, masses, Q) and of the output, not 50 fp32 Euler steps
    xs_o = o.us_to_state_trajectories(us)
    g_o = o.obstacle_avoidance_constraints(xs_o, np.asarray(o.obs_Qs))                             # (M, 3, S)
    g_gen = d.linearize_generators_device(us, rows_out=1)["g_up"].permute(2, 0, 1).cpu().numpy().astype(np.float64)
    g_row = d.linearize_device(us, rows_out=1)["g_up"].permute(2, 0, 1).cpu().numpy().astype(np.float64)
    e_gen, e_row = np.abs(g_gen - g_o).max(), np.abs(g_row - g_o).max()
    print(f"S={S} M={M}: max |g - g_oracle|: generators kernel (fp64 arithmetic) {e_gen:.2e}, row kernel (fp32) {e_row:.2e}, "
          f"max |g| {np.abs(g_o).max():.1f}")
    np.testing.assert_allclose(g_gen, g_o, rtol=1e-6, atol=5e-6)
    if S < 2:
        return
    # rows of tail samples: implicit (from A22) vs explicit (from Phi), K = 3 synthetic cuts
    lib, dev = d._lib, gen["_W"].device
    ld, K, nw = gen["_g_up"].shape[-1], 3, 2 * (S - 1)
    rng = np.random.RandomState(8)
    m_base = torch.as_tensor(rng.randn(K, M).astype(np.float32), device=dev)
    arg_base = torch.as_tensor(rng.randint(0, 3 * S, size=(K, M)).astype(np.int32), device=dev)
    stats_base = torch.zeros((K, stats.N_STATS), dtype=torch.float64, device=dev)
    for k in range(K):
        stats.risk_stats_device(m_base[k], 0.2, out=stats_base[k])
    slots = torch.as_tensor(np.array([2, 0, 1], dtype=np.int32), device=dev)
    nblk = (M + 255) // 256
    pa = torch.zeros((nblk, K, nw + 1), dtype=torch.float64, device=dev)
    pb = torch.zeros((nblk, K, nw + 1), dtype=torch.float64, device=dev)
    p = d._params(M, ld)
    mass = d._inputs(None)[1]
    _lib.check(lib.rato_drone_tail_rows_implicit(C.byref(p), _lib.ptr(mass), _lib.ptr(gen["_A22"]), 3, _lib.ptr(gen["_W"]),
                                                 _lib.ptr(gen["_g_up"]), _lib.ptr(m_base), _lib.ptr(arg_base),
                                                 _lib.ptr(stats_base), stats.N_STATS, _lib.ptr(slots), K, 0.2 * M, _lib.ptr(pa),
                                                 _lib.current_stream()), "rato_drone_tail_rows_implicit")
    _lib.check(lib.rato_saa_tail_rows_batch(_lib.ptr(full["G"]), _lib.ptr(full["_W"]), ld, full["tile"], 3, S, M,
                                            _lib.ptr(full["_g_up"]), _lib.ptr(m_base), _lib.ptr(arg_base),
                                            _lib.ptr(stats_base), stats.N_STATS, _lib.ptr(slots), K, 0.2 * M, _lib.ptr(pb),
                                            _lib.current_stream()), "rato_saa_tail_rows_batch")
    a, b = pa.sum(0).cpu().numpy(), pb.sum(0).cpu().numpy()
    # rows regenerated in fp64 from the fp32 A22 table against the stored fp32 Phi: equal to the rounding of Phi
    np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-6 * max(1.0, np.abs(b).max()))
    np.testing.assert_allclose(stats.sum_partials(pa.view(nblk, -1)).cpu().numpy().reshape(K, nw + 1), a, rtol=1e-13, atol=1e-13)


def test_monte_carlo_report_matches_oracle():
    """scp.monte_carlo_report (drone_risk.py:697-725): per-solution fraction safe / AVaR / cost on fresh samples
    and their mean / median over the repeats, against the oracle's Monte-Carlo functions."""
    from oracle import drone as od, stats as ostats
    from riskaversetrajopt_amd import drone_risk, scp
    S, M, alpha = 20, 2000, 0.1
    DWs, masses, Q = od.sample_uncertain_parameters(np.random.RandomState(77), 'saa', M=M, S=S)
    o = od.Model(S, DWs, masses, Q, 'saa', alpha)
    d = drone_risk.Model(S, DWs, masses, Q, 'saa', alpha)
    us_list = [graze(S) * f for f in (0.2, 0.6, 1.0)]
    rep = scp.monte_carlo_report(d, us_list, alpha)
    for i, us in enumerate(us_list):
        ok, Z = o.monte_carlo_no_collisions_constraint_verification(us)
        near = np.sum(np.abs(Z - 1e-6) < 1e-4) / M
        assert abs(rep["frac_satisfied"][i] - ok.mean()) <= near + 1e-12
        assert abs(rep["avar"][i] - ostats.monte_carlo_avar(Z, alpha)) < 2e-4 * max(1.0, abs(rep["avar"][i]))
        assert abs(rep["cost"][i] - o.monte_carlo_cost(us)) < 1e-9 * max(1.0, rep["cost"][i])
    assert rep["avar_median"] == np.median(rep["avar"]) and rep["cost_mean"] == np.mean(rep["cost"])
    # the report went through ONE batched call (Model.eval_batch_device); solution by solution it must be the same numbers
    for i, us in enumerate(us_list):
        st = d.monte_carlo_statistics(us, alpha=alpha)
        assert st["var"] == rep["var"][i] and st["frac_satisfied"] == rep["frac_satisfied"][i]
        assert abs(st["cvar"] - rep["avar"][i]) <= 1e-12 * max(1.0, abs(st["cvar"]))
    one = scp.monte_carlo_report(d, us_list[:1], alpha)                # (a single solution: the per-solution path)
    assert one["var"][0] == rep["var"][0]


def test_device_emitted_csc_values_with_padded_tiles():
    """the same check where the packed Jacobian's tiles are >= 1 MiB and therefore start on 2 MiB boundaries
    (driving S = 70: 1.2 MB per 64-sample tile, three tiles): CSC emission and the cutting-plane oracle read the layout
    the linearize kernel wrote"""
    S, M = 70, 130
    _, c = _car(M, S)
    t = np.arange(S)[:, None]
    us = np.hstack([0.4 * np.cos(0.4 * t) - 0.2, 0.05 * np.sin(0.35 * t) + 0.01]) * (20.0 / S)
    r = c.linearize_device(us)
    assert r["G"].stride(0) > r["G"][0].numel()                       # padded
    for scp_iter in (0, 2):
        A, l, u = c.get_constraints_coeffs(us, scp_iter)
        Ah, lh, uh = c.get_constraints_coeffs_host(us, scp_iter)
        assert np.array_equal(A.indptr, Ah.indptr) and np.array_equal(A.indices, Ah.indices)
        np.testing.assert_allclose(A.data, Ah.data, rtol=3e-7, atol=1e-30)
        np.testing.assert_allclose(u, uh, rtol=3e-7, atol=1e-12)


@pytest.mark.parametrize("system,M", [("drone", 12), ("driving", 12)])
def test_reduced_baseline_scp_matches_full_qp_scp(system, M):
    """method='baseline' (drone_risk.py:303-325, driving.py:320-329) through solve_reduced: the M R_s hard rows as the
    one constraint max_i m_i(u) <= -pad / kappa (row generation with the CVaR oracle at a one-sample tail)."""
    from riskaversetrajopt_amd import scp
    S = 20
    if system == "drone":
        _, d = _drone(M, S, alpha=0.2, method='baseline')
        full = scp.run_drone(d, num_scp_iters_max=10, warmup_iters=0)
        _, d2 = _drone(M, S, alpha=0.2, method='baseline')
        red = scp.run_drone_reduced(d2, num_scp_iters_max=10)
    else:
        _, d = _car(M, S, alpha=0.1, method='baseline')
        full = scp.run_driving(d, num_scp_iters_max=8)
        _, d2 = _car(M, S, alpha=0.1, method='baseline')
        red = scp.run_driving_reduced(d2, num_scp_iters_max=8)
    np.testing.assert_allclose(red["us"], full["us"], rtol=0, atol=1e-5)
    assert red["cuts"].sum() >= 1 and red["t_risk"] == 0.0
    # the rows the reference builds for 'baseline' (pinned by reference execution: ref_*_S20_M16.npz) are satisfied
    A, l, u = d.get_constraints_coeffs(red["us"], 5)
    nU = A.shape[1] - M - 2
    Au = A[:, :nU] @ red["us"].reshape(-1)
    fin = np.isfinite(u)
    assert np.all(Au[fin] <= u[fin] + 2e-5)


@pytest.mark.parametrize("system,M,alpha,S", [("drone", 200, 0.1, 20), ("drone", 10000, 0.05, 20), ("driving", 200, 0.1, 20),
                                              ("driving", 10000, 0.05, 20), ("drone", 3000, 0.1, 50), ("driving", 3000, 0.05, 40),
                                              # horizons whose x no longer fits the kernel arguments of the one-call round
                                              # trip (S n_u > 192: it is uploaded instead) and ragged sample counts
                                              ("drone", 301, 0.1, 70), ("driving", 333, 0.1, 100)])
def test_reduced_subproblems_device_vs_fp64_host_oracle(system, M, alpha, S):
    """The benchmarked path (device linearization in fp32, device cut oracle) against the SAME algorithm run entirely
    in fp64 on the fp64 oracle's linearization (tests/_host_cuts.py; its equality with the reference's full QP is a CPU
    test, tests/test_reduced_host.py) -- at batch sizes beyond what a host QP solves reliably.  Every subproblem of the
    SCP path is solved by both from the SAME iterate (the fp64 leg's), so that each comparison is one subproblem, not
    the accumulated drift of two sequences."""
    from tests._host_cuts import DroneReducedOracle, DrivingReducedOracle
    # (S = 50 / 40: the horizons of the BASELINE configurations, at the largest M whose dense fp64 rows the host holds)
    if system == "drone":
        o, d = _drone(M, S, alpha=alpha, seed=11)
        h, iters = DroneReducedOracle(o), (12 if S == 20 else 8)
    else:
        o, d = _car(M, S, alpha=alpha, seed=11)
        h, iters = DrivingReducedOracle(o), (8 if S == 20 else 6)
    us = h.initial_guess_us_mat()
    du, dt_ = [], []
    for k in range(iters):
        ud, td, _ = d.solve_reduced(us, k)
        uh, th, _ = h.solve_reduced(us, k)
        du.append(np.abs(ud - uh).max())
        dt_.append(abs(td - th))
        us = uh
    print(system, M, "per-subproblem max |du|:", " ".join("%.1e" % v for v in du), "| |dt_risk|:",
          " ".join("%.1e" % v for v in dt_))
    # every subproblem, the one where the CVaR rows switch on included (its step from the linearization point is O(1):
    # with fp32 linearization tables in the rows it reached 2.4e-5 in u at S = 50; the drone oracle now re-runs the
    # rollout in fp64 from the samples, and the last evaluated cut joins the master before it returns)
    assert max(du) < 1e-5 and max(dt_) < 1e-5


@pytest.mark.parametrize("system,M,alpha,iters", [("drone", 200, 0.1, 40), ("driving", 200, 0.1, 10)])
def test_reduced_scp_device_vs_fp64_host_oracle(system, M, alpha, iters):
    """... and the two free-running SCP sequences end at the same controls (1e-5)."""
    from riskaversetrajopt_amd import scp
    from tests._host_cuts import DroneReducedOracle, DrivingReducedOracle
    S = 20
    if system == "drone":
        o, d = _drone(M, S, alpha=alpha, seed=11)
        ref = scp.run_drone_reduced(DroneReducedOracle(o), num_scp_iters_max=iters)
        out = scp.run_drone_reduced(d, num_scp_iters_max=iters)
    else:
        o, d = _car(M, S, alpha=alpha, seed=11)
        ref = scp.run_driving_reduced(DrivingReducedOracle(o), num_scp_iters_max=iters)
        out = scp.run_driving_reduced(d, num_scp_iters_max=iters)
    print(system, M, "max |du| %.2e  |dt_risk| %.2e  L2 %.1e / %.1e" %
          (np.abs(out["us"] - ref["us"]).max(), abs(out["t_risk"] - ref["t_risk"]), out["L2_error"][-1], ref["L2_error"][-1]))
    np.testing.assert_allclose(out["us"], ref["us"], rtol=0, atol=1e-5)
    assert abs(out["t_risk"] - ref["t_risk"]) < 1e-5


def _device_cut_data(cs):
    """(weights, arg-max rows) of every ring slot the last solve gave a multiplier to, from the device rings: the tail
    rule of rato_saa_tail_rows_batch (1 above t = out[10], lambda on ties)"""
    out = {}
    for slot, lam in cs_last_cuts(cs):
        m = cs.ring_m[slot].double().cpu().numpy()
        arg = cs.ring_arg[slot].cpu().numpy()
        st = cs.ring_res[slot].cpu().numpy()
        t, n_gt, n_eq = np.float32(st[10]), st[8], st[9]
        lam_tie = min(max((cs.alphaM - n_gt) / n_eq, 0.0), 1.0) if n_eq > 0 else 0.0
        m32 = m.astype(np.float32)
        out[slot] = ((m32 > t) * 1.0 + (m32 == t) * lam_tie, arg)
    return out


def cs_last_cuts(cs):
    return [(sl, lam) for sl, lam in cs._last_info["multipliers"]["cuts"] if lam > 0.0]


@pytest.mark.parametrize("system,M,alpha", [("drone", 200, 0.1), ("drone", 1000, 0.05), ("driving", 200, 0.1),
                                            ("driving", 1000, 0.05)])
def test_device_reduced_solution_satisfies_the_kkt_conditions_of_the_full_qp(system, M, alpha):
    """The device-linearized reduced solution against the FULL QP assembled (reference layout, host fp64 arithmetic)
    from the same device linearization: lifted to (u, y, slack, t), with the master's multipliers spread over the
    full QP's rows, it meets primal feasibility / stationarity / dual signs / complementarity -- the optimum of the
    reference's QP without relying on a host solver that cannot take this M (tests/test_reduced_host.py has the same
    certificate in pure fp64).  Explicit Jacobian (products), reference form of the rows: exactly the numbers A holds."""
    from tests._host_cuts import kkt_certificate
    S = 20
    if system == "drone":
        _, d = _drone(M, S, alpha=alpha, seed=21)
        kw, n_c, n_u, R, kappa, first = dict(implicit=False, generators_only=False, delta=False, factored=False), 6, 3, 3, 0.01, 2
    else:
        _, d = _car(M, S, alpha=alpha, seed=21)
        kw, n_c, n_u, R, kappa, first = dict(delta=False), 4, 2, 1, 1.0, 1
    P, q = d.get_objective_coeffs()
    us = d.initial_guess_us_mat()
    worst = {}
    for it in range(6):
        nxt, _, info = d.solve_reduced(us, it, tol=1e-10, **kw)
        if it >= first:
            d._cut_solver._last_info = info
            if system == "drone":       # the full QP from the very buffers this solve read (another launch of another
                from riskaversetrajopt_amd import assemble      # kernel variant rounds its sample sums differently)
                r = d._lin_buffers
                A, l, u = assemble.saa_constraints(
                    d.expand_final_du(r["du_sum"].cpu().numpy(), 1.0 / M), r["rhs_sum"].cpu().numpy() / M,
                    d.packed_jacobian(r).double().cpu().numpy(), r["g_up"].double().cpu().numpy(), n_u=3, S=S, M=M,
                    alpha=alpha, method='saa', kappa=0.01, baseline_pad=0.0, u_min=d.u_min, u_max=d.u_max, relax=None)
            else:
                A, l, u = d.get_constraints_coeffs_host(us, it)
            c = kkt_certificate(A, l, u, P, q, info, _device_cut_data(d._cut_solver), n_c=n_c, n_u=n_u, S=S, M=M, R=R,
                                kappa=kappa, alphaM=d._cut_solver.alphaM, saa=True, u_max=None)
            scale = max(1.0, c["multiplier_scale"])
            for k in ("primal", "stationarity", "dual_sign", "complementarity"):
                worst[k] = max(worst.get(k, 0.0), c[k] / (1.0 if k == "primal" else scale))
        us = nxt
    print(system, M, "KKT residuals (relative to the multiplier scale):", {k: "%.1e" % v for k, v in worst.items()})
    assert worst["primal"] < 1e-7 and worst["stationarity"] < 1e-8 and worst["dual_sign"] < 1e-8 \
        and worst["complementarity"] < 1e-8


@pytest.mark.parametrize("S,M", [(20, 300), (50, 1000), (2, 5), (125, 70)])
def test_rollout_form_of_the_oracle(S, M):
    """rato_drone_rowmax_rollout / rato_drone_tail_rows_rollout (the oracle re-runs the rollout at u_k in fp64 from the
    samples, no linearization table) against (a) the fp64 oracle's dense rows g + G (u - u_k) on the SAME fp32-rounded
    samples -- what is left is fp64 rounding -- and (b) the table form (generators + rato_drone_*_implicit)."""
    import ctypes as C
    import torch
    from oracle import drone as od
    from riskaversetrajopt_amd import _lib, drone_risk, stats
    DWs, masses, Q = od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=M, S=S)
    r32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    DWs, masses, Q = r32(DWs), r32(masses), r32(Q)       # the device holds fp32 samples: give the oracle the same numbers
    o = od.Model(S, DWs, masses, Q, 'saa', 0.2)
    d = drone_risk.Model(S, DWs, masses, Q, 'saa', 0.2)
    uk = graze(S)
    rng = np.random.RandomState(4)
    x = 0.3 * rng.randn(S, 3)
    dev = d.device
    lib = d._lib
    dW, mass, Qsym, _ = d._inputs(None)
    ld = mass.numel()
    p = d._params(M, ld)
    uk_d = torch.as_tensor(uk, dtype=torch.float64, device=dev).contiguous()
    x_d = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    m = torch.empty(M, dtype=torch.float32, device=dev)
    a = torch.empty(M, dtype=torch.int32, device=dev)
    _lib.check(lib.rato_drone_rowmax_rollout(C.byref(p), _lib.ptr(uk_d), _lib.ptr(dW), _lib.ptr(mass), _lib.ptr(Qsym),
                                             _lib.ptr(x_d), _lib.ptr(m), _lib.ptr(a), _lib.current_stream()), "rowmax_rollout")
    # (a) fp64 oracle: rows = g + G x
    _, _, _, gdu_o, gup_o = o.get_all_constraints_coeffs(uk)
    G = gdu_o.reshape(M, 3 * S, 3 * S)
    g = -(gup_o.reshape(M, 3 * S) - G @ uk.reshape(-1))
    rows = g + G @ x.reshape(-1)
    m_o, a_o = rows.max(axis=1), rows.argmax(axis=1)
    scale = max(1.0, np.abs(rows).max())
    md = m.double().cpu().numpy()
    print(f"S={S} M={M}: rollout oracle vs fp64 rows: max |dm| {np.abs(md - m_o).max():.2e} (rows up to {scale:.1f}; "
          f"fp32 rounding of the OUTPUT alone is {np.abs(m_o.astype(np.float32).astype(np.float64) - m_o).max():.2e})")
    # the constants of rato_drone_params are floats (k_p = 0.05f is 1.5e-8 away from 0.05): 1e-9 of the rows' scale on
    # top of the final rounding of m to fp32
    assert np.all(np.abs(md - m_o) <= 6.0e-8 * np.abs(m_o) + 2e-9 * scale)             # exact up to the final rounding ...
    srt = np.sort(rows, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-8 * scale if 3 * S > 1 else np.ones(M, bool)
    assert np.array_equal(a.cpu().numpy()[clear], a_o[clear])                        # ... and the same arg-max rows
    if S < 2:
        return
    # the cut: tail weights from the statistics of m, sums of the arg-max rows and of their offsets
    st = torch.zeros(stats.N_STATS, dtype=torch.float64, device=dev)
    stats.risk_stats_device(m, 0.2, out=st)
    nblk, nc = (M + 255) // 256, 2 * (S - 1) + 1
    part = torch.zeros((nblk, nc), dtype=torch.float64, device=dev)
    _lib.check(lib.rato_drone_tail_rows_rollout(C.byref(p), _lib.ptr(uk_d), _lib.ptr(dW), _lib.ptr(mass), _lib.ptr(Qsym),
                                                _lib.ptr(m), _lib.ptr(a), _lib.ptr(st), stats.N_STATS, None, 1, 0.2 * M,
                                                _lib.ptr(part), _lib.current_stream()), "tail_rows_rollout")
    sums = part.sum(0).cpu().numpy()
    sth = st.cpu().numpy()
    t, n_gt, n_eq = np.float32(sth[10]), sth[8], sth[9]
    lam = min(max((0.2 * M - n_gt) / n_eq, 0.0), 1.0) if n_eq > 0 else 0.0
    m32 = md.astype(np.float32)
    w = (m32 > t) * 1.0 + (m32 == t) * lam
    arg_h = a.cpu().numpy()
    idx = np.arange(M)
    grad_o = (w[:, None] * G[idx, arg_h]).sum(axis=0).reshape(S, 3)[:S - 1, :2].reshape(-1)
    off_o = float(w @ g[idx, arg_h])
    np.testing.assert_allclose(sums[:nc - 1], grad_o, rtol=1e-7, atol=1e-8 * max(1.0, np.abs(grad_o).max()))
    np.testing.assert_allclose(sums[nc - 1], off_o, rtol=1e-7, atol=1e-8 * float(w @ np.abs(g[idx, arg_h]) + 1.0))
    # (b) the table form on the same linearization: equal to the rounding of its fp32 tables
    gen = d.linearize_generators_device(uk, rows_out=1)
    m_t = torch.empty(M, dtype=torch.float32, device=dev)
    a_t = torch.empty(M, dtype=torch.int32, device=dev)
    _lib.check(lib.rato_drone_rowmax_implicit(C.byref(p), _lib.ptr(mass), _lib.ptr(gen["_A22"]), 3, _lib.ptr(gen["_W"]),
                                              _lib.ptr(gen["_g_up"]), 1.0, _lib.ptr(x_d), _lib.ptr(m_t), _lib.ptr(a_t),
                                              _lib.current_stream()), "rowmax_implicit")
    np.testing.assert_allclose(m_t.double().cpu().numpy(), md, rtol=0, atol=2e-6 * scale)


@pytest.mark.parametrize("S,M", [(20, 300), (40, 1000), (2, 5), (90, 70)])
def test_driving_rollout_form_of_the_oracle(S, M):
    """rato_car_rowmax_rollout / rato_car_tail_rows_rollout (ego tables folded per workgroup and the pedestrian re-rolled
    per sample, all in fp64, no Jacobian) against (a) the fp64 oracle's dense rows g + G (u - u_k) on the SAME
    fp32-rounded samples and (b) the explicit form (packed Jacobian of the row kernel + rato_saa_rowmax); and the
    host-folded final rows against the oracle's."""
    import ctypes as C
    import torch
    from oracle import driving as ocar
    from riskaversetrajopt_amd import _lib, driving, stats
    r32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    samples = [r32(a) for a in ocar.sample_uncertain_parameters(np.random.RandomState(0), M, 'saa', S)]
    alpha = 0.2
    o = ocar.Model(*samples, method='saa', alpha=alpha)
    d = driving.Model(M, 'saa', alpha, S=S, samples=samples)
    t = np.arange(S)[:, None]
    uk = np.hstack([0.4 * np.cos(0.3 * t) + 0.1, 0.03 * np.sin(0.5 * t) + 0.004]) * (20.0 / S)
    x = 0.3 * np.random.RandomState(4).randn(S, 2) * np.array([1.0, 0.05])
    dev, lib = d.device, d._lib
    dW, x0, ws, wr = d._dW, d._x0, d._ws, d._wr
    p = d._params(M)
    uk_d = torch.as_tensor(uk, dtype=torch.float64, device=dev).contiguous()
    x_d = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    m = torch.empty(M, dtype=torch.float32, device=dev)
    a = torch.empty(M, dtype=torch.int32, device=dev)
    _lib.check(lib.rato_car_rowmax_rollout(C.byref(p), _lib.ptr(uk_d), _lib.ptr(dW), _lib.ptr(x0), _lib.ptr(ws), _lib.ptr(wr),
                                           _lib.ptr(x_d), _lib.ptr(m), _lib.ptr(a), _lib.current_stream()), "rowmax_rollout")
    fdu_o, flo_o, _, gdu_o, gup_o = o.get_all_constraints_coeffs(uk)
    G = gdu_o.reshape(M, S, 2 * S)
    g = -(gup_o.reshape(M, S) - G @ uk.reshape(-1))
    rows = g + G @ x.reshape(-1)
    m_o, a_o = rows.max(axis=1), rows.argmax(axis=1)
    scale = max(1.0, np.abs(rows).max())
    md = m.double().cpu().numpy()
    print(f"S={S} M={M}: driving rollout oracle vs fp64 rows: max |dm| {np.abs(md - m_o).max():.2e} (rows up to {scale:.1f}; "
          f"fp32 rounding of the OUTPUT alone is {np.abs(m_o.astype(np.float32).astype(np.float64) - m_o).max():.2e})")
    assert np.all(np.abs(md - m_o) <= 6.0e-8 * np.abs(m_o) + 2e-9 * scale)             # exact up to the final rounding ...
    srt = np.sort(rows, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-8 * scale
    assert np.array_equal(a.cpu().numpy()[clear], a_o[clear])                        # ... and the same arg-max rows
    # final rows (sample independent), folded on the host in fp64
    fdu, frhs = d.ego_final_rows(uk)
    np.testing.assert_allclose(fdu, fdu_o[0], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(frhs, flo_o[0], rtol=1e-12, atol=1e-12)
    # the cut
    st = torch.zeros(stats.N_STATS, dtype=torch.float64, device=dev)
    stats.risk_stats_device(m, alpha, out=st)
    nblk, nc = (M + 255) // 256, 2 * (S - 1) + 1
    part = torch.zeros((nblk, nc), dtype=torch.float64, device=dev)
    _lib.check(lib.rato_car_tail_rows_rollout(C.byref(p), _lib.ptr(uk_d), _lib.ptr(dW), _lib.ptr(x0), _lib.ptr(ws),
                                              _lib.ptr(wr), _lib.ptr(m), _lib.ptr(a), _lib.ptr(st), stats.N_STATS, None, 1,
                                              alpha * M, _lib.ptr(part), _lib.current_stream()), "tail_rows_rollout")
    sums = part.sum(0).cpu().numpy()
    sth = st.cpu().numpy()
    tq, n_gt, n_eq = np.float32(sth[10]), sth[8], sth[9]
    lam = min(max((alpha * M - n_gt) / n_eq, 0.0), 1.0) if n_eq > 0 else 0.0
    m32 = md.astype(np.float32)
    w = (m32 > tq) * 1.0 + (m32 == tq) * lam
    arg_h = a.cpu().numpy()
    idx = np.arange(M)
    grad_full = (w[:, None] * G[idx, arg_h]).sum(axis=0).reshape(S, 2)
    assert np.all(grad_full[S - 1] == 0.0)                          # u_{S-1} enters no row
    grad_o = grad_full[:S - 1].reshape(-1)
    off_o = float(w @ g[idx, arg_h])
    np.testing.assert_allclose(sums[:nc - 1], grad_o, rtol=1e-7, atol=1e-8 * max(1.0, np.abs(grad_o).max()))
    np.testing.assert_allclose(sums[nc - 1], off_o, rtol=1e-7, atol=1e-8 * float(w @ np.abs(g[idx, arg_h]) + 1.0))
    # (b) the explicit form on the same linearization point: equal to the rounding of the fp32 Jacobian
    r = d.linearize_device(uk, rows_out=1)
    m_t = torch.empty(M, dtype=torch.float32, device=dev)
    a_t = torch.empty(M, dtype=torch.int32, device=dev)
    _lib.check(lib.rato_saa_rowmax(_lib.ptr(r["G"]), None, r["tile"], 1, S, M, M, _lib.ptr(r["g_up"]), 1.0, _lib.ptr(x_d), 2,
                                   _lib.ptr(m_t), _lib.ptr(a_t), _lib.current_stream()), "rowmax")
    np.testing.assert_allclose(m_t.double().cpu().numpy(), md, rtol=0, atol=1e-5 * scale)


def test_driving_reduced_solve_rollout_equals_explicit():
    """one subproblem of the driving SCP from the same iterate: table-free oracle against the packed-Jacobian oracle"""
    o, d = _car(1500, 30, alpha=0.1, seed=3)
    us = np.zeros((30, 2)) + 1e-2
    for it in range(3):
        d._cut_solver = None
        u_r, t_r, info_r = d.solve_reduced(us, it, rollout=True)
        d._cut_solver = None
        u_e, t_e, info_e = d.solve_reduced(us, it, rollout=False)
        print("iteration %d: |du| %.2e |dt| %.2e cuts %d / %d" % (it, np.abs(u_r - u_e).max(), abs(t_r - t_e),
                                                                    info_r["cuts"], info_e["cuts"]))
        np.testing.assert_allclose(u_r, u_e, rtol=0, atol=1e-5)
        assert abs(t_r - t_e) < 1e-5
        us = u_r


@pytest.mark.parametrize("system", ["drone", "driving"])
def test_one_call_round_trip_equals_the_stepwise_calls(system):
    """rato_cut_oracle_rollout (x in the kernel arguments, rowmax, selection, cut sums, read-back, synchronisation in one
    library call) against the same round trip issued call by call through device memory: identical m values, arg-max
    rows, statistics and cut sums."""
    import torch
    from riskaversetrajopt_amd import stats
    if system == "drone":
        o, d = _drone(13000, 30, alpha=0.1, seed=5)           # (> 12,288 samples: the one-launch selection across workgroups)
    else:
        o, d = _car(13000, 30, alpha=0.1, seed=5)
    us = d.initial_guess_us_mat()
    for it in range(3):
        us, _, _ = d.solve_reduced(us, it)                    # leaves a solver with the table-free oracle configured
    cs = d._cut_solver
    assert cs.rollout is not None and cs.world == 1
    rng = np.random.RandomState(2)
    u = np.asarray(us, dtype=np.float64).reshape(-1) + 0.05 * rng.randn(cs.nU)
    phi, t, g = cs.evaluate(None, None, 0, None, u, slot=3)
    one = (cs.ring_m[3].clone(), cs.ring_arg[3].clone(), cs.ring_res[3].clone())
    sign, x0 = cs._form()
    cs._evaluate_stepwise(None, None, 0, None, np.ascontiguousarray(u - x0), sign, cs.ring_m[4], cs.ring_arg[4], cs.ring_res[4])
    assert torch.equal(one[0], cs.ring_m[4]) and torch.equal(one[1], cs.ring_arg[4])
    assert torch.equal(one[2], cs.ring_res[4])
    r = cs.res_host.numpy()
    assert np.array_equal(r, one[2].cpu().numpy()) and np.isfinite(phi) and t == r[0]
    # a selection that gives up (here: an unclean workspace) is recovered inside evaluate: same cut
    if cs.M > 12288:
        cs.ws.view(torch.int32)[100] = 7
        phi2, t2, g2 = cs.evaluate(None, None, 0, None, u, slot=5)
        assert t2 == t and abs(phi2 - phi) <= 1e-12 * max(1.0, abs(phi)) and np.allclose(g2, g, rtol=1e-12, atol=1e-15)


def _bench_batch(system):
    """The batch bench.py's SCP blocks run on (device Philox sampler, seed 7; drone M = 1e5, S = 50, alpha = 0.1 /
    driving M = 1e5, S = 40, alpha = 0.05) -> (device Model, fp64 oracle Model holding the SAME fp32 numbers)."""
    if system == "drone":
        from oracle import drone as od
        from riskaversetrajopt_amd import drone_risk, drone_utils
        M, S, alpha = 100000, 50, 0.1
        dW, mass, Qsym = drone_utils.sample_uncertain_parameters_device(M, S, seed=7)
        d = drone_risk.Model.from_device(S, dW, mass, Qsym, 'saa', alpha, M=M)
        DWs = np.zeros((M, S, 6))
        DWs[:, :, 3:6] = dW[:, :, :M].permute(2, 0, 1).double().cpu().numpy()
        Qs = Qsym[:, :, :M].double().cpu().numpy()                  # [obs][(Q00, Q01 + Q10, Q11)][M]
        Q = np.zeros((M, 3, 3, 3))
        Q[:, :, 0, 0], Q[:, :, 0, 1], Q[:, :, 1, 1] = Qs[:, 0].T, Qs[:, 1].T, Qs[:, 2].T
        return d, od.Model(S, DWs, mass[:M].double().cpu().numpy(), Q, 'saa', alpha)
    from oracle import driving as ocar
    from riskaversetrajopt_amd import driving
    M, S, alpha = 100000, 40, 0.05
    dW, x0, ws, wr = driving.sample_uncertain_parameters_device(M, S, seed=7)
    d = driving.Model.from_device(S, dW, x0, ws, wr, 'saa', alpha)
    DWs = np.zeros((M, S, 8))
    DWs[:, :, 6:8] = dW.permute(2, 0, 1).double().cpu().numpy()
    x0h = np.repeat(ocar.state_init[None, :], M, axis=0)
    x0h[:, 4:8] = x0.t().double().cpu().numpy()
    return d, ocar.Model(x0h, ws.double().cpu().numpy(), wr.double().cpu().numpy(), DWs, method='saa', alpha=alpha)


@pytest.mark.parametrize("system", ["drone", "driving"])
def test_reduced_subproblems_at_the_benchmarked_size(system):
    """North star: "SCP iterates matching reference to 1e-5" AT THE SIZE THE METRIC IS QUOTED ON.  bench.py's own
    batch (M = 1e5; drone S = 50, driving S = 40): every subproblem of the SCP path solved by the benchmarked device
    path (fp32 samples, table-free fp64 device oracle, recycled cuts, tol 1e-8) and by the all-fp64 leg on the
    oracle's streaming C cut oracle (oracle/saa_oracle.c: every sample's dense linearization formed in the reference's
    shapes, rows G u - g_up of drone_risk.py:357-364 / driving.py:358-363; == the dense NumPy leg == the reference's
    full QP on the CPU, tests/test_reduced_host.py), from the SAME iterate -- the subproblems where the CVaR rows switch
    on (the worst ones) included."""
    from tests._host_cuts import DroneStreamingOracle, DrivingStreamingOracle
    d, o = _bench_batch(system)
    h = (DroneStreamingOracle if system == "drone" else DrivingStreamingOracle)(o)
    iters = 9 if system == "drone" else 7
    us = h.initial_guess_us_mat()
    du, dtr, cuts = [], [], []
    for k in range(iters):
        ud, td, idv = d.solve_reduced(us, k)
        uh, th, ih = h.solve_reduced(us, k)
        du.append(np.abs(ud - uh).max())
        dtr.append(abs(td - th))
        cuts.append((idv["cuts"], ih["cuts"]))
        us = uh
    print(system, "M=1e5 per-subproblem max |du|:", " ".join("%.1e" % v for v in du), "| |dt_risk|:",
          " ".join("%.1e" % v for v in dtr), "| cuts (device, fp64):", cuts)
    assert max(du) < 1e-5 and max(dtr) < 1e-5


@pytest.mark.parametrize("system,M,S,alpha,method", [("drone", 2000, 20, 0.1, "saa"), ("drone", 3001, 50, 0.05, "saa"),
                                                     ("driving", 2000, 20, 0.1, "saa"), ("driving", 3001, 40, 0.05, "saa"),
                                                     ("drone", 64, 20, 0.2, "baseline"), ("driving", 64, 20, 0.1, "baseline")])
def test_native_cut_loop_equals_the_python_loop_bitwise(system, M, S, alpha, method):
    """rato_cut_solve (csrc/cutloop.hip: the cutting-plane loop of a subproblem as one library call -- what bench.py's SCP
    blocks time) against cvar_cuts.CvarCutSolver._solve (the Python loop every parity test of this file was established
    on): same master, same oracle round trips, exactly rounded inner products on both sides -> the free-running SCP
    sequences agree BIT FOR BIT, iterate by iterate, with the same cut counts, keep lists and multipliers."""
    mk = (lambda: _drone(M, S, alpha=alpha, method=method, seed=3)[1]) if system == "drone" else \
         (lambda: _car(M, S, alpha=alpha, method=method, seed=3)[1])
    a, b = mk(), mk()
    us_a = us_b = a.initial_guess_us_mat()
    iters = 10 if system == "drone" else 7
    for k in range(iters):
        us_a, t_a, ia = a.solve_reduced(us_a, k)
        if b.__dict__.get("_cut_solver") is not None:
            b._cut_solver.use_native_loop = False
        else:                                     # the solver is created by the first call: switch it before any loop runs
            import os
            os.environ["RATO_PY_CUT_LOOP"] = "1"
        try:
            us_b, t_b, ib = b.solve_reduced(us_b, k)
        finally:
            import os
            os.environ.pop("RATO_PY_CUT_LOOP", None)
        b._cut_solver.use_native_loop = False
        assert ia["loop"] == "native" and ib["loop"] == "python"
        assert np.array_equal(us_a, us_b), (k, np.abs(us_a - us_b).max())
        assert t_a == t_b and ia["slack"] == ib["slack"] and ia["cuts"] == ib["cuts"] and ia["status"] == ib["status"]
        assert a._cut_solver.keep == b._cut_solver.keep and a._cut_solver.idle == b._cut_solver.idle
        ma, mb = ia["multipliers"], ib["multipliers"]
        assert ma["cuts"] == mb["cuts"] and ma["slack"] == mb["slack"] and ma["uncertified_cuts"] == mb["uncertified_cuts"]
        flat = lambda bs: sorted((int(i), float(sg), float(la)) for idx, sg, lam in bs for i, la in zip(idx, lam))
        assert flat(ma["bounds"]) == flat(mb["bounds"])


@pytest.mark.parametrize("system,M,alpha", [("drone", 200, 0.1), ("drone", 1000, 0.05), ("driving", 200, 0.1),
                                            ("driving", 1000, 0.05)])
def test_matrix_free_certificate_agrees_with_the_full_qp_certificate(system, M, alpha):
    """certificate.certify (sums over the samples formed on the device: what bench.py reports at M = 1e5) against
    tests/_host_cuts.kkt_certificate on the reference-layout QP that the fp64 ORACLE assembles from the same fp32-rounded
    samples -- the benchmarked path (table-free oracle, native loop).  Both certify the same lifted point: their
    residuals are small together."""
    from tests._host_cuts import kkt_certificate
    from tests._oracle_qp import DroneOracleQP, DrivingOracleQP
    S = 20
    r32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    if system == "drone":
        from oracle import drone as od
        from riskaversetrajopt_amd import drone_risk
        DWs, masses, Q = (r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(21), 'saa', M=M, S=S))
        o, d = od.Model(S, DWs, masses, Q, 'saa', alpha), drone_risk.Model(S, DWs, masses, Q, 'saa', alpha)
        oq, n_c, n_u, R, kappa, first = DroneOracleQP(o), 6, 3, 3, 0.01, 2
    else:
        from oracle import driving as ocar
        from riskaversetrajopt_amd import driving
        samples = tuple(r32(a) for a in ocar.sample_uncertain_parameters(np.random.RandomState(21), M, 'saa', S))
        o, d = ocar.Model(*samples, method='saa', alpha=alpha), driving.Model(M, 'saa', alpha, S=S, samples=samples)
        oq, n_c, n_u, R, kappa, first = DrivingOracleQP(o), 4, 2, 1, 1.0, 1
    P, q = oq.get_objective_coeffs()
    us = d.initial_guess_us_mat()
    worst_dev, worst_host = {}, {}
    for it in range(6):
        nxt, _, info = d.solve_reduced(us, it, tol=1e-10)
        if it >= first:
            d._cut_solver._last_info = info
            cut_data = _device_cut_data(d._cut_solver)                 # (before certify overwrites the scratch slot)
            c = d.certify_reduced(info)
            A, l, u = oq.get_constraints_coeffs(us, it)
            hc = kkt_certificate(A, l, u, P, q, info, cut_data, n_c=n_c, n_u=n_u, S=S, M=M, R=R, kappa=kappa,
                                 alphaM=d._cut_solver.alphaM, saa=True, u_max=None)
            hs = max(1.0, hc["multiplier_scale"])
            for k in ("primal", "stationarity", "dual_sign", "complementarity"):
                worst_dev[k] = max(worst_dev.get(k, 0.0), c[k])
                worst_host[k] = max(worst_host.get(k, 0.0), hc[k] / (1.0 if k == "primal" else hs))
        us = nxt
    print(system, M, "matrix-free:", {k: "%.1e" % v for k, v in worst_dev.items()},
          "| full QP (fp64 oracle rows):", {k: "%.1e" % v for k, v in worst_host.items()})
    # the device rows equal the fp64 oracle's up to the rounding of m to fp32 (6e-8 of |m| <= 1): both certificates see it
    for k in ("primal", "stationarity", "dual_sign", "complementarity"):
        assert worst_dev[k] < 1e-7, (k, worst_dev)
        assert worst_host[k] < 2e-6, (k, worst_host)


@pytest.mark.parametrize("system", ["drone", "driving"])
def test_kkt_certificate_at_the_benchmarked_size(system):
    """the reduced solution of every subproblem with CVaR rows on bench.py's own batch (M = 1e5)
    satisfies the KKT conditions of the reference-layout QP (1.5e7 rows) to 1e-7 -- matrix-free, on the device."""
    d, _ = _bench_batch(system)
    first = 2 if system == "drone" else 1
    us = d.initial_guess_us_mat()
    worst = {}
    for it in range(first + 6):
        nxt, _, info = d.solve_reduced(us, it)
        if it >= first:
            c = d.certify_reduced(info)
            for k in ("primal", "stationarity", "dual_sign", "complementarity"):
                worst[k] = max(worst.get(k, 0.0), c[k])
        us = nxt
    print(system, "M=1e5 KKT residuals:", {k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) < 1e-7, worst


@pytest.mark.parametrize("system,bound", [("drone", 0.12), ("driving", 0.15)])
def test_reduced_subproblems_with_controls_pinned_at_their_bounds(system, bound):
    """|u| <= u_max (drone_risk.py:221-237, driving.py:243-258) ACTIVE: with the bound pulled inside the unconstrained
    solution, several controls sit at +-u_max; the lazily entering bound rows of the native loop against the fp64 leg
    (same iterate, every subproblem), and the bound multipliers in the KKT certificate of the full QP."""
    from tests._host_cuts import DroneReducedOracle, DrivingReducedOracle
    M, S = 200, 20
    if system == "drone":
        o, d = _drone(M, S, alpha=0.1, seed=11)
        h, iters, first = DroneReducedOracle(o), 5, 2
    else:
        o, d = _car(M, S, alpha=0.1, seed=11)
        h, iters, first = DrivingReducedOracle(o), 5, 1
    d.u_max, d.u_min = bound, -bound
    h.cs.u_max, h.cs.u_min = bound, -bound
    us = h.initial_guess_us_mat()
    pinned = 0
    for k in range(iters):
        ud, td, idv = d.solve_reduced(us, k)
        uh, th, ih = h.solve_reduced(us, k)
        assert idv["loop"] == "native" and np.abs(ud).max() <= bound + 1e-9
        assert np.abs(ud - uh).max() < 1e-5 and abs(td - th) < 1e-5, (k, np.abs(ud - uh).max())
        at_bound = np.abs(np.abs(ud) - bound) < 1e-9
        assert np.array_equal(at_bound, np.abs(np.abs(uh) - bound) < 1e-9)
        if k >= first:
            n_mult = sum(int((np.asarray(la) > 0).sum()) for _, _, la in idv["multipliers"]["bounds"])
            assert n_mult <= at_bound.sum()
            c = d.certify_reduced(idv)
            assert max(c["primal"], c["stationarity"], c["dual_sign"], c["complementarity"]) < 1e-7, c
            pinned = max(pinned, int(at_bound.sum()))
        us = uh
    print(system, "controls pinned at the bound:", pinned)
    assert pinned >= 3


@pytest.mark.parametrize("M,S,alpha,method,iters", [(3001, 30, 0.1, "saa", 14), (13000, 50, 0.05, "saa", 9),
                                                    (64, 20, 0.2, "baseline", 8)])
def test_native_scp_loop_equals_the_per_iteration_loop_bitwise(M, S, alpha, method, iters):
    """rato_scp_run_drone (the whole reduced SCP as ONE library call, what bench.py's SCP block times) against
    scp.run_drone_reduced's Python loop (one rato_cut_define_drone + one rato_cut_solve per iteration, a device
    synchronisation on both sides of each): the same iterates bit for bit, iteration by iteration, the same cut counts and
    t_risk, the same kept cuts at the end -- and a solve_reduced that follows continues identically on both."""
    from riskaversetrajopt_amd import scp
    a, b = _drone(M, S, alpha=alpha, method=method, seed=4)[1], _drone(M, S, alpha=alpha, method=method, seed=4)[1]
    ra = scp.run_drone_reduced(a, num_scp_iters_max=iters)
    rb = scp.run_drone_reduced(b, num_scp_iters_max=iters, native_loop=False)
    assert ra["loop"].startswith("native") and rb["loop"].startswith("python")
    assert ra["us_hist"].shape == rb["us_hist"].shape == (iters, S, 3)
    for k in range(iters):
        assert np.array_equal(ra["us_hist"][k], rb["us_hist"][k]), (k, np.abs(ra["us_hist"][k] - rb["us_hist"][k]).max())
    assert np.array_equal(ra["cuts"], rb["cuts"]) and np.array_equal(ra["L2_error"], rb["L2_error"])
    assert ra["t_risk"] == rb["t_risk"] and np.array_equal(ra["us"], rb["us"])
    assert a._cut_solver.keep == b._cut_solver.keep and a._cut_solver.idle == b._cut_solver.idle
    assert (ra["define_s"] > 0).all() and (ra["solve_s"] > 0).all() and np.all(np.diff(ra["cumulative_s"]) > 0)
    ua, ta, ia = a.solve_reduced(ra["us"], iters)
    ub, tb, ib = b.solve_reduced(rb["us"], iters)
    assert np.array_equal(ua, ub) and ta == tb and ia["cuts"] == ib["cuts"]


def test_native_scp_loop_edge_iteration_counts():
    """one iteration (no CVaR rows yet: the relaxed subproblem only), three (the first CVaR subproblem), and zero (nothing
    runs: the initial guess comes back) -- the native loop and the per-iteration loop agree on each"""
    from riskaversetrajopt_amd import scp
    for iters in (1, 3, 0):
        a, b = _drone(500, 20, alpha=0.1, seed=2)[1], _drone(500, 20, alpha=0.1, seed=2)[1]
        ra = scp.run_drone_reduced(a, num_scp_iters_max=iters)
        rb = scp.run_drone_reduced(b, num_scp_iters_max=iters, native_loop=False)
        assert np.array_equal(np.asarray(ra["us"]), np.asarray(rb["us"])) and len(ra["define_s"]) == len(rb["define_s"]) == iters
        assert np.array_equal(ra["cuts"], rb["cuts"])
        if iters:
            assert ra["loop"].startswith("native") and np.array_equal(ra["us_hist"], rb["us_hist"])


def test_a_define_that_is_never_solved_does_not_leak_into_the_next_one():
    """ADVICE r5 (csrc/cutloop.hip): rato_cut_define_drone arms the pinned words of the kept cuts' sums and launches their
    re-linearization; a second define without a solve in between used to re-arm the words while the first launch could
    still write into them -- the next solve's wait would then be satisfied by the OLD launch's sums.  Two defines in a row
    (the first at another point) followed by one solve must give exactly what one define + one solve give."""
    import ctypes as C
    from riskaversetrajopt_amd import _lib

    def prepared():
        d = _drone(4000, 30, alpha=0.1, seed=9)[1]
        us = d.initial_guess_us_mat()
        for k in range(4):
            us, _, _ = d.solve_reduced(us, k)             # leaves kept cuts behind
        return d, us
    (a, us_a), (b, us_b) = prepared(), prepared()
    assert np.array_equal(us_a, us_b) and len(a._cut_solver.keep) > 0
    # b: an abandoned define at a shifted point first
    cs = b._cut_solver
    buf = b._native_define_buffers(cs)
    h, out = cs._native_solver(), cs._keep_arrays()
    other = np.ascontiguousarray(us_b * 1.05 + 0.01, dtype=np.float64)
    rc = b._lib.rato_cut_define_drone(h, other.ctypes.data, buf["us_host"].data_ptr(), buf["us_dev"].data_ptr(),
                                      buf["A22"].data_ptr(), None, 0, buf["part"].data_ptr(), buf["sums_host"].data_ptr(), None,
                                      None, out["keep"].ctypes.data, len(cs.keep), _lib.current_stream())
    assert rc == 0
    ua, ta, ia = a.solve_reduced(us_a, 4)
    ub, tb, ib = b.solve_reduced(us_b, 4)
    assert np.array_equal(ua, ub) and ta == tb and ia["cuts"] == ib["cuts"] and ia["loop"] == ib["loop"] == "native"


def test_native_solver_is_rebuilt_when_its_parameter_struct_changes_in_place():
    """ADVICE r5 (cvar_cuts.py): rato_cut_solver holds the rollout parameters BY VALUE; the cached handle must not survive
    an in-place edit of the Python-side struct (same object, other bytes), nor a change of keep_max."""
    d = _drone(600, 20, alpha=0.1, seed=1)[1]
    us = d.initial_guess_us_mat()
    for k in range(3):
        us, _, _ = d.solve_reduced(us, k)
    cs = d._cut_solver
    h1 = cs._native_solver()
    assert cs._native_solver().value == h1.value            # unchanged inputs: the cached handle
    p = cs.rollout[1]
    p.drag64 = p.drag64 * (1.0 + 1e-9)                      # in place: same Python object
    h2 = cs._native_solver()
    assert cs._native[3][3] == bytes(p) and (h2.value != h1.value or cs._native[0][1] == bytes(p))
    key_before = cs._native[0]
    cs.keep_max = cs.keep_max - 1
    cs._native_solver()
    assert cs._native[0] != key_before


def test_bad_kept_cut_arguments_are_rejected_before_any_launch():
    """rato_cut_begin and rato_cut_define_drone share one validation of the kept cuts (csrc/cutloop.hip: keep_args_ok): a
    count beyond keep_max, a negative count, a count without slots and a slot that is the ring's scratch slot (cap - 1) are
    each RATO_EINVAL, answered before anything is staged or launched -- the solver's state is untouched and the next
    solve_reduced gives the iterate of a twin Model that never saw the bad calls, to the bit.  M = 50, S = 20 (the
    reference's size: one sample block, inputs staged through kernel arguments); two relaxed iterations, then two with the
    CVaR rows, leave kept cuts behind."""
    from riskaversetrajopt_amd import _lib
    RATO_EINVAL = -1                                          # rato_saa.h

    def prepared():
        d = _drone(50, 20, alpha=0.1, seed=4)[1]
        us = d.initial_guess_us_mat()
        for k in range(4):
            us, _, _ = d.solve_reduced(us, k)
        return d, us
    (a, us_a), (b, us_b) = prepared(), prepared()
    cs = a._cut_solver
    assert np.array_equal(us_a, us_b) and len(cs.keep) > 0 and cs.S >= 2
    buf = a._native_define_buffers(cs)
    h, out = cs._native_solver(), cs._keep_arrays()
    K = len(cs.keep)
    u = np.ascontiguousarray(us_a, dtype=np.float64)
    good = out["keep"].copy()
    scratch = good.copy()
    scratch[K - 1] = cs.cap - 1
    state = lambda: (cs._native[0], cs._native[1].value, list(cs.keep), dict(cs.idle), cs._relin_pending,
                     out["keep"].tolist(), out["idle"].tolist(), out["n_keep"].value, cs.u_lin.tolist())
    before = state()
    st = _lib.current_stream()
    for keep, n_keep in ((good, cs.keep_max + 1), (good, -1), (None, 1), (scratch, K)):
        kp = None if keep is None else keep.ctypes.data
        assert a._lib.rato_cut_begin(h, u.ctypes.data, kp, n_keep, st) == RATO_EINVAL
        assert state() == before
        rc = a._lib.rato_cut_define_drone(h, u.ctypes.data, buf["us_host"].data_ptr(), buf["us_dev"].data_ptr(),
                                          buf["A22"].data_ptr(), None, 0, buf["part"].data_ptr(), buf["sums_host"].data_ptr(),
                                          None, None, kp, n_keep, st)
        assert rc == RATO_EINVAL
        assert state() == before
    ua, ta, ia = a.solve_reduced(us_a, 4)
    ub, tb, ib = b.solve_reduced(us_b, 4)
    assert np.array_equal(ua, ub) and ta == tb and ia["cuts"] == ib["cuts"] and ia["loop"] == ib["loop"] == "native"
