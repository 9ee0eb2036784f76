"""CPU: ``qp_ipm.solve_batch(backend='numpy')``, the host twin of csrc/qp_ipm.hip -- the same algorithm, presolve included.

Every accepted solution is judged by KKT residuals recomputed here in NumPy fp64 from the returned (z, y) and the ORIGINAL
(un-presolved) data: primal violation and stationarity with the stop rule's scaling, complementarity as
max_i(|y_i^+ (u_i - a_i'z)|, |y_i^- (a_i'z - l_i)|), each <= 2 tol (the 2 covers the re-summation in another order, ~1e-13
of the scale)."""
import numpy as np
import pytest

import _qp_ipm as H
from riskaversetrajopt_amd import qp_ipm

TOL = H.TOL
INF = np.inf


def solve1(P, q, A, l, u, **kw):
    Z, Y, info = qp_ipm.solve_batch(np.asarray(P, dtype=float), np.asarray(q, dtype=float), np.asarray(A, dtype=float)[None],
                                    np.asarray(l, dtype=float)[None], np.asarray(u, dtype=float)[None], backend='numpy', **kw)
    return Z[0], Y[0], {k: v[0] for k, v in info.items()}


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,u", [(-INF, INF), (-INF, 0.5), (-INF, 3.0), (1.5, INF), (-3.0, INF), (0.2, 0.6), (1.5, 4.0),
                                 (-4.0, -2.0), (0.7, 0.7), (np.nan, 0.5), (1.5, np.nan)])
def test_scalar_qp_with_every_combination_of_sides(l, u):
    """min 1/2 2 z^2 - 2 z (free optimum z = 1) under l <= 1.0 z <= u: z* = clip(1, l, u)"""
    P, q, A = [[2.0]], [-2.0], [[1.0]]
    z, y, info = solve1(P, q, A, [l], [u])
    lo, up = (-INF if np.isnan(l) else l), (INF if np.isnan(u) else u)
    assert info["status"] == "solved" and info["iterations"] <= H.ITER_CAP
    H.assert_kkt(P, q, A, [l], [u], z, y, what=f"scalar [{l}, {u}]")
    # 2 (z - 1) + y = 0 and the residual limits: |z - z*| <= (stationarity + |y - y*|) / 2, far below 1e-6
    assert abs(z[0] - np.clip(1.0, lo, up)) <= 1e-6
    if up < 1.0:
        assert y[0] > 0.0                                       # active upper side: OSQP's sign
    if lo > 1.0:
        assert y[0] < 0.0


@pytest.mark.parametrize("n", [3, 10, 61])
def test_separable_box_qp(n):
    """z* = clip(-q / p, l, u) with coordinates active below, active above and free; the active ones sit 0.5 inside the
    infeasible side, so |y*| >= 0.5 p >= 0.5 and |z - z*| <= 2 tol (1 + |z|) on them, (2 tol scale) / p on the free ones"""
    P, q, A, l, u, zs = H.box_qp(n, seed=n)
    z, y, info = solve1(P, q, A, l, u)
    assert info["status"] == "solved" and info["iterations"] <= H.ITER_CAP
    H.assert_kkt(P, q, A, l, u, z, y, what=f"box n={n}")
    assert np.max(np.abs(z - zs)) <= 1e-6
    kind = np.arange(n) % 3
    assert np.all(y[kind == 1] < 0.0) and np.all(y[kind == 2] > 0.0) and np.max(np.abs(y[kind == 0]), initial=0.0) <= 1e-6


@pytest.mark.parametrize("n,m", [(2, 1), (10, 4), (33, 12), (61, 20)])
def test_equality_only_qp_against_a_dense_kkt_solve(n, m):
    """the KKT matrix [[P, A'], [A, 0]] has lambda_min(P) >= 1 and random full-rank A: its solve is exact to ~1e-12; the
    solver's point has residuals <= tol scale, so the distance is <= cond tol scale -- 1e-5 is asserted, cond <= 1e2 here"""
    P, q, A, l, u, zs, ys = H.equality_qp(n, m, seed=100 + n)
    z, y, info = solve1(P, q, A, l, u)
    assert info["status"] == "solved" and info["iterations"] <= H.ITER_CAP
    H.assert_kkt(P, q, A, l, u, z, y, what=f"equality n={n} m={m}")
    assert np.max(np.abs(z - zs)) <= 1e-5 and np.max(np.abs(y - ys)) <= 1e-5


# ---- constructed QPs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,seed", [(1, 1, 0), (2, 3, 1), (5, 0, 2), (12, 30, 3), (31, 40, 4), (61, 85, 5), (64, 130, 6)])
def test_constructed_qp_recovers_the_designed_solution(n, m, seed):
    """``_qp_ipm.constructed``: z*, active set, |y*| >= 1e-2, lambda_min(P) >= 1, inactive sides at a margin >= 0.1.  The bound on
    |z - z*| is ``_qp_ipm.constructed_bound`` (derived in its docstring from tol, lambda_min and the stop rule alone)."""
    P, q, A, l, u, zs, ys = H.constructed(n, m, seed)
    z, y, info = solve1(P, q, A, l, u)
    assert info["status"] == "solved" and info["iterations"] <= H.ITER_CAP
    H.assert_kkt(P, q, A, l, u, z, y, what=f"constructed n={n} m={m}")
    bound = H.constructed_bound(P, A, zs)
    print(f"|z - z*| = {np.max(np.abs(z - zs)):.3e}, bound {bound:.3e}")
    assert np.max(np.abs(z - zs)) <= bound
    assert np.all(np.sign(y[np.abs(ys) > 0]) == np.sign(ys[np.abs(ys) > 0]))


# ---- designs that reach the retry ladder ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1e-11, 1e-7, 1e-3])
@pytest.mark.parametrize("n,m,j", [(70, 85, 0), (70, 85, 31), (70, 85, 32), (70, 85, 69), (33, 40, 32), (130, 85, 96)])
def test_saddle_takes_the_designed_number_of_rungs(n, m, j, c):
    """``_qp_ipm.saddle``: pivot j is exactly -c + delta_w, so every iteration factors RUNGS[c] times -- a count the design fixes,
    not rounding.  z_j stays exactly 0 and the other variables solve ``constructed``'s QP.  Here (70 x 85): 13 to 16 iterations."""
    P, q, A, l, u, zs, _, keep = H.saddle(n, m, j, c, 1000 * n + 10 * m + j)
    z, y, info = qp_ipm.solve_numpy(P, q, A, l, u, TOL, 100)            # past the presolve, as the device test goes
    print(f"saddle n={n} m={m} j={j} c={c}: {info['status']} in {info['iterations']} iterations, {info['factorizations']} factorizations")
    assert info["status"] == "solved" and 0 < info["iterations"] <= H.ITER_CAP
    assert info["factorizations"] == H.RUNGS[c] * info["iterations"]
    assert z[j] == 0.0
    H.assert_kkt(P, q, A, l, u, z, y, what=f"saddle n={n} m={m} j={j} c={c}")
    assert np.max(np.abs(z[keep] - zs[keep])) <= H.constructed_bound(P[np.ix_(keep, keep)], A[:, keep], zs[keep])
    pre = qp_ipm.presolve(P, q, A, l, u)                                # the presolve would drop nothing here
    assert pre["cols"].size == n and pre["rows"].size == m


@pytest.mark.parametrize("j", [0, 31, 32, 69])
def test_saddle_beyond_the_last_rung_exhausts_the_ladder(j):
    """c = 1e13 is above the 13th rung (1e-12 x 100^12 ~ 1e12): 'numerical' with 0 iterations, 13 factorizations, z the start"""
    P, q, A, l, u, _, _, _ = H.saddle(70, 85, j, 1e13, 1000 * 70 + 10 * 85 + j)
    z, y, info = qp_ipm.solve_numpy(P, q, A, l, u, TOL, 100)
    assert H.rung(qp_ipm.MAX_RETRIES) < 1e13
    assert info["status"] == "numerical" and info["iterations"] == 0 and info["factorizations"] == qp_ipm.MAX_RETRIES + 1 == 13
    assert np.all(z == 0.0) and np.all(np.isfinite(y))


def test_rungs_are_what_the_design_says():
    """RUNGS[c] counts the attempts up to the first whose pivot -c + delta_w is positive (all 13 when none is), for the deltas
    both backends compute (1e-12 multiplied by 100.0 in fp64); no rung lies within a factor 2 of c, so rounding cannot decide"""
    attempts = qp_ipm.MAX_RETRIES + 1
    for c, rungs in H.RUNGS.items():
        failing = sum(not (-c + H.rung(k) > 0.0) for k in range(attempts))
        assert min(failing + 1, attempts) == rungs
        assert all(not (0.5 < H.rung(k) / c < 2.0) for k in range(attempts))


@pytest.mark.parametrize("n,r,m,scale", H.DEFICIENT)
def test_deficient_reaches_the_ladder_by_rounding(n, r, m, scale):
    """``_qp_ipm.deficient``: Kc0 has rank r, the n - r surplus pivots are rounding noise.  The solution is not unique, so the
    KKT residuals judge it.  Here: 18 factorizations in 11 iterations (33, 10, 20, 1), 48 in 17 (65, 20, 40, 1e4), 72 in 20
    (70, 35, 50, 1e6)."""
    P, q, A, l, u = H.deficient(n, r, m, n, scale)
    assert np.linalg.matrix_rank(P) == r
    z, y, info = qp_ipm.solve_numpy(P, q, A, l, u, TOL, 100)
    print(f"deficient n={n} r={r} m={m} scale={scale:g}: {info['status']}, {info['factorizations']} factorizations in "
          f"{info['iterations']} iterations")
    assert info["status"] == "solved" and info["iterations"] <= H.ITER_CAP
    H.assert_kkt(P, q, A, l, u, z, y, what=f"deficient n={n} r={r}")
    assert info["factorizations"] > info["iterations"]
    if scale > 1.0:
        assert info["factorizations"] >= 2 * info["iterations"]


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("n,m", [(256, 384), (255, 383), (256, 0), (1, 384)])
def test_constructed_qp_at_the_entry_points_largest_shapes(n, m, k):
    """the shapes tests/test_gpu_qp_ipm_paths.py runs on the device, both seeds: 18, 19, 1 and 9 iterations here at k = 0,
    18, 17, 1 and 6 at k = 1"""
    P, q, A, l, u, zs, _ = H.constructed(n, m, 1000 * n + 10 * m + k)
    z, y, info = qp_ipm.solve_numpy(P, q, A.reshape(m, n), l, u, TOL, 100)
    print(f"n={n} m={m} k={k}: {info['status']} in {info['iterations']} iterations, {info['factorizations']} factorizations")
    assert info["status"] == "solved" and info["iterations"] <= H.ITER_CAP
    H.assert_kkt(P, q, A.reshape(m, n), l, u, z, y, what=f"constructed n={n} m={m}")
    assert np.max(np.abs(z - zs)) <= H.constructed_bound(P, A.reshape(m, n), zs)


def test_unreachable_tolerance_runs_into_max_iter_and_the_hard_cap():
    """``_qp_ipm.CAP_QP`` at tol = 1e-17: the iterates stay finite and the stop rule is never met, so the solve ends 'max_iter'
    at exactly max_iter iterations -- 150 for 150, 200 for 200, and 200 again for 10**6 (HARD_CAP), with the bytes of 200"""
    P, q, A, l, u, _, _ = H.constructed(*H.CAP_QP)
    runs = {mi: qp_ipm.solve_numpy(P, q, A, l, u, H.CAP_TOL, mi) for mi in (150, 200, 10 ** 6)}
    for mi, (z, y, info) in runs.items():
        print(f"max_iter={mi}: {info['status']} in {info['iterations']} iterations, {info['factorizations']} factorizations")
        assert info["status"] == "max_iter" and info["iterations"] == min(mi, qp_ipm.HARD_CAP) and np.all(np.isfinite(z))
    assert qp_ipm.HARD_CAP == 200
    assert runs[10 ** 6][0].tobytes() == runs[200][0].tobytes() and runs[10 ** 6][1].tobytes() == runs[200][1].tobytes()
    assert runs[150][0].tobytes() != runs[200][0].tobytes()          # the last 50 iterations move the point: the cap is what binds


# ---- the driving Gaussian QPs ------------------------------------------------------------------------------------------------------
def driving_cases():
    cases = [(20, 0.05, name) for name in ("scp_iter0", "warmup1")]            # the warm-up pair at S = 20
    cases += [(40, 0.01, "main1")]                                             # where recomputed slacks went NaN
    cases += [(5, a, "main1") for a in H.ALPHAS]
    return cases


@pytest.mark.parametrize("S,alpha,name", driving_cases())
def test_driving_qp_is_solved_within_the_iteration_cap(S, alpha, name):
    qp = dict(H.warmup_qps(S, alpha))[name]
    z, y, info = H.twin_solve(qp)
    print(f"S={S} alpha={alpha} {name}: {info}")
    assert info["status"] == "solved" and info["iterations"] <= H.ITER_CAP
    H.assert_kkt(*qp, z, y, what=f"driving S={S} alpha={alpha} {name}")
    if name == "scp_iter0":                                                     # the relaxed rows: what the presolve is for
        assert np.all(y[8:4 + S] == 0.0) and z[-1] == 0.0


@pytest.mark.parametrize("S", [5, 20])
@pytest.mark.parametrize("alpha", H.ALPHAS)
def test_scp_through_the_twin_converges(S, alpha):
    r = H.twin_scp(S, alpha)
    print(f"S={S} alpha={alpha}: final L2 step {r['L2'][-1]:.3e}, iterations per solve {min(r['iterations'])}..{max(r['iterations'])}")
    assert r["status"] == ["solved"] * 60
    assert max(r["iterations"]) <= H.ITER_CAP
    assert r["L2"][-1] <= 1e-5


# ---- statuses ------------------------------------------------------------------------------------------------------------------
def test_infeasible_rows_end_not_solved_with_finite_iteration_counts():
    z, y, info = solve1(np.eye(2), np.zeros(2), [[1.0, 0.0], [1.0, 0.0]], [-INF, 1.0], [-1.0, INF])   # z0 <= -1 and z0 >= 1
    assert info["status"] in ("max_iter", "numerical")
    assert 0 <= info["iterations"] <= 100 and 0 < info["factorizations"] <= 13 * 101


def test_nan_in_the_matrix_is_invalid():
    z, y, info = solve1(np.eye(2), np.zeros(2), [[1.0, np.nan]], [0.0], [1.0])
    assert info["status"] == "invalid" and info["iterations"] == 0
    assert np.all(np.isnan(z)) and np.all(np.isnan(y))
    assert solve1(np.eye(2), np.zeros(2), [[1.0, 1.0]], [2.0], [1.0])[2]["status"] == "invalid"          # l > u


def test_zero_row_with_a_positive_lower_bound_is_infeasible_without_a_solve():
    z, y, info = solve1(np.eye(2), np.zeros(2), [[0.0, 0.0], [1.0, 0.0]], [1.0, 0.0], [2.0, 1.0])
    assert info["status"] == "infeasible" and info["iterations"] == 0 and info["factorizations"] == 0


def test_presolve_maps_back_removed_rows_and_columns():
    P = np.diag([1.0, 0.0, 2.0])
    A = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 1.0]])
    l, u = np.array([0.5, np.nan, -INF, -INF]), np.array([INF, 0.0, INF, 5.0])
    z, y, info = solve1(P, [-0.2, 0.0, -2.0], A, l, u)
    assert info["status"] == "solved"
    H.assert_kkt(P, [-0.2, 0.0, -2.0], A, l, u, z, y, what="presolve")
    assert z[1] == 0.0 and y[1] == 0.0 and y[2] == 0.0            # the empty column, the zero row, the row without sides
    assert abs(z[0] - 0.5) <= 1e-6 and abs(z[2] - 1.0) <= 1e-6 and y[0] < 0.0


def test_batch_equals_the_solo_runs_bitwise():
    Pa, qa, Aa, la, ua, _, _ = H.constructed(6, 8, 11)
    Pb, qb, Ab, lb, ub, _, _ = H.constructed(6, 8, 12)
    Ac = Aa.copy()
    Ac[1] = Ac[0]
    lc, uc = la.copy(), ua.copy()
    lc[0], uc[0], lc[1], uc[1] = -INF, -1.0, 1.0, INF             # a_0'z <= -1 and a_0'z >= 1
    P, q = np.stack([Pa, Pb, Pa]), np.stack([qa, qb, qa])
    A, l, u = np.stack([Aa, Ab, Ac]), np.stack([la, lb, lc]), np.stack([ua, ub, uc])
    Z, Y, info = qp_ipm.solve_batch(P, q, A, l, u, backend='numpy')
    assert info["status"][:2] == ["solved", "solved"] and info["status"][2] in ("max_iter", "numerical")
    for k in range(3):
        z, y, i1 = solve1(P[k], q[k], A[k], l[k], u[k])
        assert z.tobytes() == Z[k].tobytes() and y.tobytes() == Y[k].tobytes()
        assert i1["status"] == info["status"][k] and i1["iterations"] == info["iterations"][k]


def test_ipm_object_has_the_osqp_result_shape():
    import scipy.sparse as sp
    P, q, A, l, u, zs, _ = H.constructed(5, 7, 21)
    prob = qp_ipm.IPM(backend='numpy')
    prob.setup(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u, tol=TOL)
    res = prob.solve()
    assert res.info.status == "solved" and res.x.shape == (5,) and res.y.shape == (7,)
    prob.update(l=l - 1.0, u=u + 1.0)
    prob.update(Ax=sp.csc_matrix(A).data)
    res2 = prob.solve()
    assert res2.info.status == "solved" and np.max(np.abs(res.x - zs)) <= H.constructed_bound(P, A, zs)


def test_solver_keyword_is_appended_with_todays_default():
    import inspect
    from riskaversetrajopt_amd import driving_gaussian, scp
    assert list(inspect.signature(driving_gaussian.Model.__init__).parameters)[-1] == "solver"
    assert inspect.signature(driving_gaussian.Model.__init__).parameters["solver"].default == "osqp"
    for fn, dflt in ((scp.run_driving_gaussian, None), (scp.run_driving_gaussian_batch, None),
                     (scp.driving_gaussian_experiment, "osqp")):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "solver" and p["solver"].default == dflt
