"""Shared by tests/test_qp_ipm_cpu.py and tests/test_gpu_qp_ipm.py: the KKT residual check on the ORIGINAL data, QP
constructions with known solutions, the driving Gaussian QPs built on the CPU (tests/_car_gaussian.linearize +
driving_gaussian.constraints_coeffs) and the SCP through the host twin (computed once per session, never modified)."""
import functools

import numpy as np

import _car_gaussian as R
from riskaversetrajopt_amd import driving_gaussian as DG
from riskaversetrajopt_amd import driving_params as DP
from riskaversetrajopt_amd import qp_ipm, scp

TOL = 1e-8
ALPHAS = (0.01, 0.02, 0.05, 0.1)
ITER_CAP = 40                       # the prototype needed <= 25; 40 keeps a stalled method from passing


def kkt_residuals(P, q, A, l, u, z, y):
    """(primal, stationarity, complementarity), the first two divided by the stop rule's scales, recomputed in fp64 from
    (z, y) and the un-presolved data; NaN bounds are absent sides."""
    P, q, A = np.asarray(P, dtype=np.float64), np.asarray(q, dtype=np.float64), np.asarray(A, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        l = np.where(np.isnan(l), -np.inf, np.asarray(l, dtype=np.float64))
        u = np.where(np.isnan(u), np.inf, np.asarray(u, dtype=np.float64))
    Az, Pz = A @ z, P @ z
    eq = np.isfinite(l) & (l == u)
    viol = np.max(np.maximum(np.maximum(l - Az, Az - u), 0.0), initial=0.0)
    primal = viol / (1.0 + np.max(np.abs(Az), initial=0.0))
    ATyI = A.T @ np.where(eq, 0.0, y)
    stat = np.max(np.abs(Pz + q + A.T @ y)) / (1.0 + max(np.max(np.abs(Pz)), np.max(np.abs(q)), np.max(np.abs(ATyI))))
    with np.errstate(invalid="ignore"):
        cu = np.where(np.isfinite(u), np.maximum(y, 0.0) * np.where(np.isfinite(u), u - Az, 0.0), 0.0)
        cl = np.where(np.isfinite(l), np.maximum(-y, 0.0) * np.where(np.isfinite(l), Az - l, 0.0), 0.0)
    cu, cl = np.where(eq, 0.0, cu), np.where(eq, 0.0, cl)
    # a multiplier pushing against an absent side is a stationarity error no scale forgives
    wrong = np.max(np.where(~np.isfinite(u), np.maximum(y, 0.0), 0.0) + np.where(~np.isfinite(l), np.maximum(-y, 0.0), 0.0),
                   initial=0.0)
    comp = max(np.max(np.abs(cu), initial=0.0), np.max(np.abs(cl), initial=0.0), wrong)
    return float(primal), float(stat), float(comp)


def assert_kkt(P, q, A, l, u, z, y, tol=TOL, what=""):
    r = kkt_residuals(P, q, A, l, u, z, y)
    print(f"kkt {what}: primal {r[0]:.3e} stationarity {r[1]:.3e} complementarity {r[2]:.3e}")
    assert max(r) <= 2.0 * tol, (what, r)


# ---- constructed QPs ---------------------------------------------------------------------------------------------------------
LAMBDA_MIN, Y_MIN, MARGIN = 1.0, 1e-2, 0.1


def constructed(n, m, seed, n_eq=None):
    """A QP with a known solution: z*, an active set with multipliers |y*| >= Y_MIN, P with lambda_min >= LAMBDA_MIN,
    q = -P z* - A'y*, inactive sides at a margin >= MARGIN.  At most n rows are active (equalities included) and the active
    rows are linearly independent (random), so (z*, y*) is the unique KKT pair.  -> P, q, A, l, u, z*, y*"""
    rng = np.random.RandomState(seed)
    z = rng.uniform(-1.0, 1.0, n)
    B = rng.uniform(-1.0, 1.0, (n, n)) / np.sqrt(n)
    P = B @ B.T + LAMBDA_MIN * np.eye(n)
    P = (P + P.T) / 2
    A = rng.uniform(-1.0, 1.0, (m, n))
    n_act = min(m, max(n // 2, 1)) if m else 0
    n_eq = min(n_act // 3, n_act) if n_eq is None else min(n_eq, n_act)
    act = rng.permutation(m)[:n_act]
    y = np.zeros(m)
    y[act] = rng.uniform(Y_MIN, 2.0, n_act) * rng.choice([-1.0, 1.0], n_act)
    Az = A @ z
    l, u = Az - rng.uniform(MARGIN, 1.0, m), Az + rng.uniform(MARGIN, 1.0, m)
    one_sided = rng.uniform(size=m) < 0.3
    for i in range(m):
        if one_sided[i] and y[i] == 0.0:
            if rng.uniform() < 0.5:
                l[i] = -np.inf
            else:
                u[i] = np.inf
    for j, i in enumerate(act):
        if j < n_eq:
            l[i] = u[i] = Az[i]
        elif y[i] > 0:
            u[i] = Az[i]
            if one_sided[i]:
                l[i] = -np.inf
        else:
            l[i] = Az[i]
            if one_sided[i]:
                u[i] = np.inf
    q = -P @ z - A.T @ y
    return P, q, A, l, u, z, y


def constructed_bound(P, A, z, tol=TOL):
    """|z - z*|_inf for a point that passes the solver's stop rule on a ``constructed`` QP, from the design's constants alone.
    With e = z - z*, strong convexity gives  lambda_min |e|^2 <= e'P e = e'(r_d - A'(y - y*)),  r_d the stationarity residual.
    The multiplier term is  -sum_i (y_i - y*_i) a_i'e:  on a row active at the upper side (a_i'z* = u_i, y*_i > 0) it is
    <= y_i (u_i - a_i'z) + y*_i (a_i'z - u_i) <= comp + |y*_i| viol, likewise below; on an inactive row (y*_i = 0) it is
    y_i^+ (a_i'z* - a_i'z) <= comp - y_i^+ (margin - viol) <= comp.  With the stop rule  |r_d|_inf <= tol s_d,  viol <= tol s_p
    and every product  lam |gap| <= tol  (so comp <= tol on every row):
        lambda_min |e|_2^2 <= sqrt(n) tol s_d |e|_2 + m (2 tol + 2 y_max tol s_p)
    which is solved for |e|_2 >= |e|_inf.  The scales s_d, s_p are taken at z* with a factor 2 for the iterate (|e| << 1),
    y_max = 2 max |y*| likewise (|y - y*| is small once |e| is: the active rows are independent)."""
    n, m = z.size, A.shape[0]
    s_p = 2.0 * (1.0 + np.max(np.abs(A @ z), initial=0.0))
    s_d = 2.0 * (1.0 + max(np.max(np.abs(P @ z)), np.max(np.abs(P)) * n + 4.0 * np.sum(np.abs(A), axis=0).max(initial=0.0)))
    y_max = 4.0
    b, c = np.sqrt(n) * tol * s_d, m * (2.0 * tol + 2.0 * y_max * tol * s_p)
    return (b + np.sqrt(b * b + 4.0 * LAMBDA_MIN * c)) / (2.0 * LAMBDA_MIN)


# ---- designs that reach the retry ladder (delta_w x 100 while a pivot fails) ------------------------------------------------------
RUNGS = {1e-11: 2, 1e-7: 4, 1e-3: 6, 1e13: qp_ipm.MAX_RETRIES + 1}   # saddle's c -> factorization attempts per iteration


def rung(k):
    """delta_w of attempt k (0-based) as both backends compute it: 1e-12 multiplied k times by 100.0 in fp64"""
    dw = qp_ipm.DELTA_W0
    for _ in range(k):
        dw *= qp_ipm.DELTA_W_GROWTH
    return dw


def saddle(n, m, j, c, seed):
    """``constructed(n - 1, m, seed)`` on every variable but j, and variable j decoupled with negative curvature: P[j, j] = -c,
    the rest of row and column j of P zero, q[j] = 0, A[:, j] = 0.  Pivot j of Kc0 + delta_w I has only exact zeros to subtract,
    so it is exactly -c + delta_w in any summation order, with or without FMA: the factorization fails at pivot j on every rung
    with delta_w <= c and the number of attempts per iteration is RUNGS[c] by design.  Row j of every right-hand side is
    c z_j = 0, so dz_j and z_j stay exactly 0 and the other variables see ``constructed``'s QP (plus delta_w, which the
    refinement removes).  Non-convex, so outside the solver's contract, not outside its handling.
    -> P, q, A, l, u, z* (z*[j] = 0), y*, keep (the n - 1 indices of the constructed part)"""
    P0, q0, A0, l, u, z0, y = constructed(n - 1, m, seed)
    keep = np.delete(np.arange(n), j)
    P, q, A, z = np.zeros((n, n)), np.zeros(n), np.zeros((m, n)), np.zeros(n)
    P[np.ix_(keep, keep)] = P0
    P[j, j] = -c
    q[keep], A[:, keep], z[keep] = q0, A0, z0
    return P, q, A, l, u, z, y, keep


DEFICIENT = [(33, 10, 20, 1.0), (65, 20, 40, 1e4), (70, 35, 50, 1e6)]          # (n, r, m, scale); seed = n


def deficient(n, r, m, seed, scale=1.0):
    """P = scale B B' with B (n, r) and A = C B': Kc0 = B (scale I + C'D C) B' has rank r exactly, and its n - r surplus pivots
    are rounding noise of either sign, of the order eps scale (and eps |D| late in the solve) against delta_w = 1e-12: the
    ladder is reached by rounding.  z* is feasible, about r / 2 rows are active with multipliers |y*| >= Y_MIN, the others keep a
    margin >= MARGIN, q = -P z* - A'y* (in the range of B, so the QP is bounded).  The solution is NOT unique (z* + null(B') is
    optimal): judge a result by ``assert_kkt`` only.  -> P, q, A, l, u"""
    rng = np.random.RandomState(seed)
    B = rng.uniform(-1.0, 1.0, (n, r)) / np.sqrt(r)
    C = rng.uniform(-1.0, 1.0, (m, r))
    P = scale * (B @ B.T)
    P = (P + P.T) / 2
    A = C @ B.T
    z = rng.uniform(-1.0, 1.0, n)
    n_act = min(m, max(r // 2, 1))
    act = rng.permutation(m)[:n_act]
    y = np.zeros(m)
    y[act] = rng.uniform(Y_MIN, 2.0, n_act) * rng.choice([-1.0, 1.0], n_act)
    Az = A @ z
    l, u = Az - rng.uniform(MARGIN, 1.0, m), Az + rng.uniform(MARGIN, 1.0, m)
    u[act] = np.where(y[act] > 0, Az[act], u[act])
    l[act] = np.where(y[act] < 0, Az[act], l[act])
    return P, -P @ z - A.T @ y, A, l, u


# An input that runs into the iteration cap: a tolerance below what fp64 residuals can reach (the dual residual stalls near
# 1e-10, the primal near 1e-15) on a QP whose iterates stay finite for 200 iterations, so the only exit left is max_iter.
CAP_QP, CAP_TOL = (33, 65, 33065), 1e-17


def box_qp(n, seed):
    """separable: diagonal P >= 1, A = I, some coordinates active below, some above, some free: z* = clip(-q / p, l, u)"""
    rng = np.random.RandomState(seed)
    p = rng.uniform(1.0, 3.0, n)
    free = rng.uniform(-1.0, 1.0, n)                                 # -q / p
    kind = np.arange(n) % 3                                          # 0 free, 1 active below, 2 active above
    l = np.where(kind == 1, free + 0.5, free - 0.5)
    u = np.where(kind == 2, free - 0.5, free + 0.5)
    l = np.where(kind == 2, u - 1.0, l)
    u = np.where(kind == 1, l + 1.0, u)
    return np.diag(p), -p * free, np.eye(n), l, u, np.clip(free, l, u)


def equality_qp(n, m, seed):
    """equality rows only, against a dense KKT solve"""
    rng = np.random.RandomState(seed)
    B = rng.uniform(-1.0, 1.0, (n, n)) / np.sqrt(n)
    P = B @ B.T + np.eye(n)
    A = rng.uniform(-1.0, 1.0, (m, n))
    b, q = rng.uniform(-1.0, 1.0, m), rng.uniform(-1.0, 1.0, n)
    sol = np.linalg.solve(np.block([[P, A.T], [A, np.zeros((m, m))]]), np.concatenate([-q, b]))
    return P, q, A, b, b.copy(), sol[:n], sol[n:]


# ---- the driving Gaussian QPs, on the CPU ---------------------------------------------------------------------------------------
def driving_qp(S, alpha, us, alphas_risk, scp_iter):
    """-> dense (P, q, A, l, u) of define_problem (car/driving_gaussian.py:428-449) at (us, alphas_risk)"""
    lin = R.linearize(us, alphas_risk)
    A, l, u = DG.constraints_coeffs(lin, us, alphas_risk, scp_iter, alpha)
    P, q = DG.objective_coeffs(S, DP.T / S)
    return P.toarray(), q, A.toarray(), l, u


def split(S, z):
    return np.reshape(z[:2 * S], (2, S), 'F').T.copy(), z[2 * S:-1].copy()


def guess(S, alpha):
    return np.zeros((S, 2)) + 1e-2, (alpha / S) * np.ones(S)


def twin_solve(qp):
    P, q, A, l, u = qp
    Z, Y, info = qp_ipm.solve_batch(P, q, A[None], l[None], u[None], TOL, 100, backend='numpy')
    return Z[0], Y[0], {k: v[0] for k, v in info.items()}


@functools.lru_cache(maxsize=None)
def warmup_qps(S, alpha):
    """the QPs of the two warm-up solves (scp_iter 0 and 1) and the main loop's iteration 1 (linearized at iteration 0's solution,
    which is the first warm-up's): [(name, qp)]"""
    us0, al0 = guess(S, alpha)
    qp0 = driving_qp(S, alpha, us0, al0, 0)
    z, _, info = twin_solve(qp0)
    assert info["status"] == "solved"
    us1, al1 = split(S, z)
    return [("scp_iter0", qp0), ("warmup1", driving_qp(S, alpha, us1, al0, 1)), ("main1", driving_qp(S, alpha, us1, al1, 1))]


@functools.lru_cache(maxsize=None)
def twin_scp(S, alpha, iters=60):
    """The main loop of run_driving_gaussian (car/driving_gaussian.py:481-492) through the host twin with the define step of
    ``_car_gaussian.linearize``.  -> dict(us, alphas_risk, L2 (iters,), status [iters], iterations [iters])"""
    us, al = guess(S, alpha)
    L2, status, its = [], [], []
    for it in range(iters):
        z, _, info = twin_solve(driving_qp(S, alpha, us, al, it))
        status.append(info["status"])
        its.append(int(info["iterations"]))
        if info["status"] != "solved" or not np.all(np.isfinite(z)):
            break
        us_new, al = split(S, z)
        L2.append(float(scp.L2_error_us(us_new, us)))
        us = us_new
    return {"us": us, "alphas_risk": al, "L2": np.array(L2), "status": status, "iterations": its}
