"""Test helper (host only, NumPy): designed master QPs for csrc/master.hip and two references that share nothing with its
NNLS formulation.

    min 1/2 z' diag(p) z + q'z   s.t.  A z = b,   R_j z <= r_j

  * ``enumerate_reference`` (r <= 10 rows): every active set W of the rows, the KKT system of (P, A, R_W) solved in fp64, the
    set that is primal and dual feasible kept.  The thresholds are relative to each row's own scale, 1e-9 (|R_j| |z| + |r_j|):
    one threshold for all rows, 1e-9 (1 + max |r|), accepts a violated small row next to a right-hand side of 1e9.
  * ``certificate`` (any length): the KKT conditions of a returned (z, lam) -- P is positive, so a clean certificate means the
    unique minimiser.
``healthy_designs`` / ``vanishing_designs`` / ``loose_designs`` / ``churn_design`` are the problems tests/test_master_qp.py
runs, each with the row counts at which it solves; ``write_sequence`` / ``write_nnls`` / ``flat_sequence`` are the file format
of tests/host/master_host.hip.  Checker only: nothing in the package imports this."""
import itertools
from dataclasses import dataclass

import numpy as np

EINFEASIBLE = -4


# ---- references ----------------------------------------------------------------------------------------------------------
def enumerate_reference(pd, q, A, b, R, r):
    """-> (z, mu (one multiplier per row)) of the minimiser, or None when no active set gives a feasible point"""
    n, m, nr = len(q), len(b), len(r)
    assert nr <= 10
    Rn = np.linalg.norm(R, axis=1) if nr else np.zeros(0)
    best = None
    for k in range(0, min(nr, n - m) + 1):
        for W in itertools.combinations(range(nr), k):
            W = list(W)
            Cm = np.vstack([A, R[W]])
            d = np.concatenate([b, r[W]])
            mc = m + k
            # a dependent active set (duplicate rows, a row in the span of A) has no KKT system of its own: its multipliers
            # are not defined, and a smaller set describes the same point
            if mc:
                sv = np.linalg.svd(Cm / np.maximum(np.linalg.norm(Cm, axis=1, keepdims=True), 1e-300), compute_uv=False)
                if mc > n or sv[-1] <= 1e-10 * sv[0]:
                    continue
            K = np.block([[np.diag(pd), Cm.T], [Cm, np.zeros((mc, mc))]])
            rhs = np.concatenate([-q, d])
            try:
                sol = np.linalg.solve(K, rhs)
            except np.linalg.LinAlgError:
                continue
            if not np.all(np.isfinite(sol)):
                continue
            # a dependent active set (duplicate rows, a row in the span of A) that LAPACK did not flag: its residual shows it
            if np.abs(K @ sol - rhs).max() > 1e-9 * (np.abs(K) @ np.abs(sol) + np.abs(rhs)).max():
                continue
            z, mu = sol[:n], sol[n + m:]
            g = np.abs(pd * z + q).max()
            if nr and np.any(R @ z - r > 1e-9 * (Rn * np.linalg.norm(z) + np.abs(r))):
                continue
            if np.any(mu * Rn[W] < -1e-9 * max(g, 1e-300)):
                continue
            f = 0.5 * z @ (pd * z) + q @ z
            if best is None or f < best[0]:
                full = np.zeros(nr)
                full[W] = mu
                best = (f, z, full)
    return None if best is None else (best[1], best[2])


def certificate(pd, q, A, b, R, r, z, lam):
    """KKT residuals of (z, lam), each relative to the scale of its own terms -> dict(eq, viol, lam_min, comp, stat)"""
    zn = np.linalg.norm(z)
    out = {"eq": 0.0, "viol": 0.0, "lam_min": 0.0, "comp": 0.0}
    if len(b):
        out["eq"] = float(np.max(np.abs(A @ z - b) / (np.linalg.norm(A, axis=1) * zn + np.abs(b) + 1e-300)))
    g = pd * z + q
    gs = max(np.abs(g).max(), 1e-300)
    if len(r):
        Rn = np.linalg.norm(R, axis=1)
        scale = Rn * zn + np.abs(r) + 1e-300
        s = R @ z - r
        out["viol"] = float(np.max(s / scale))
        out["lam_min"] = float(np.min(lam * Rn) / gs)
        out["comp"] = float(np.max(np.abs(lam * s)) / (gs * max(zn, 1.0)))
        g = g + R.T @ lam
    if len(b):
        g = g - A.T @ np.linalg.lstsq(A.T, g, rcond=None)[0]
    out["stat"] = float(np.abs(g).max() / gs)
    return out


def certificate_worst(c):
    """the largest breach of the certificate (<= 0 parts count as clean)"""
    return max(c["eq"], c["viol"], -c["lam_min"], c["comp"], c["stat"])


# ---- designs -------------------------------------------------------------------------------------------------------------
@dataclass
class Design:
    name: str
    pd: np.ndarray
    q: np.ndarray
    A: np.ndarray
    b: np.ndarray
    R: np.ndarray
    r: np.ndarray
    chunks: tuple                 # the row counts at which the sequence solves
    kind: str = "healthy"         # healthy / vacuous / loose / infeasible
    without: tuple = ()           # rows that must not change the solution (vacuous, loose)


def _base(seed, n, m_eq, nr, slack=0.3):
    rng = np.random.RandomState(seed)
    pd, q = 1.0 + rng.rand(n), rng.randn(n)
    A, xf = rng.randn(m_eq, n), rng.randn(n)
    R = rng.randn(nr, n)
    return rng, pd, q, A, A @ xf, R, R @ xf + slack * rng.rand(nr), xf


def _eq_minimiser(pd, q, A, b):
    n, m = len(q), len(b)
    K = np.block([[np.diag(pd), A.T], [A, np.zeros((m, m))]])
    return np.linalg.solve(K, np.concatenate([-q, b]))[:n]


def healthy_designs():
    out = []
    rng, pd, q, A, b, R, r, xf = _base(0, 12, 3, 8)
    out.append(Design("plain, active rows", pd, q, A, b, R, r, (1, 4, 8)))
    z0 = _eq_minimiser(pd, q, A, b)
    out.append(Design("plain, no active row", pd, q, A, b, R, R @ z0 + 1.0 + rng.rand(8), (3, 8)))
    rng, pd, q, A, b, R, r, xf = _base(1, 10, 1, 8)
    out.append(Design("m_eq = 1", pd, q, A, b, R, r, (2, 5, 8)))
    rng, pd, q, A, b, R, r, xf = _base(2, 9, 8, 3)
    out.append(Design("m_eq = n - 1", pd, q, A, b, R[:2], r[:2], (1, 2)))
    rng, pd, q, A, b, R, r, xf = _base(3, 12, 3, 8)
    sc = 10.0 ** np.array([-8, 8, -3, 0, 5, -6, 2, 7])
    out.append(Design("rows scaled 1e-8 .. 1e8", pd, q, A, b, R * sc[:, None], r * sc, (4, 8)))
    # an optimum far out: the rows push |v| to ~1e3, then ~1e6: sigma is rescaled upwards twice inside one master.  (Downwards
    # it cannot go: rows are only ever added, so |v| of one master never shrinks.)
    rng, pd, q, A, b, R, r, xf = _base(4, 12, 3, 6)
    r_far = r - np.array([0.0, 0.0, 1e3, 1e3, 1e6, 1e6])
    out.append(Design("far out: |v| ~ 1, 1e3, 1e6", pd, q, A, b, R, r_far, (2, 4, 6)))
    out.append(Design("far out from the first solve: |v| ~ 1e6", pd, q * 1e6, A, b * 1e3, R, r, (2, 6)))
    rng, pd, q, A, b, R, r, xf = _base(5, 12, 3, 5)
    out.append(Design("exact duplicate rows", pd, q, A, b, np.vstack([R, R]), np.concatenate([r, r]), (5, 7, 10)))
    rng, pd, q, A, b, R, r, xf = _base(6, 8, 3, 10, slack=0.2)
    out.append(Design("more rows than n - m_eq + 1", pd, q, A, b, R, r, (5, 10)))
    rng, pd, q, A, b, R, r, xf = _base(7, 24, 6, 10)
    out.append(Design("n = 24", pd * np.where(np.arange(24) == 23, 1e4, 1.0), q, A, b, R, r, (3, 6, 10)))
    return out


def vanishing_designs():
    """a row that vanishes in the null space of the equalities, in the middle of seven ordinary rows: an exact combination of
    equality rows, and an all-zero row, each once with slack 1 (vacuous) and once violated by 1 (nothing is feasible)"""
    out = []
    rng, pd, q, A, b, R, r, xf = _base(0, 12, 3, 7)
    comb = np.array([0.7, -1.3, 0.0])
    for name, row, rhs0 in (("combination of equality rows", comb @ A, float(comb @ b)), ("all-zero row", np.zeros(12), 0.0)):
        for slack, kind in ((1.0, "vacuous"), (-1.0, "infeasible")):
            R2 = np.vstack([R[:3], row, R[3:]])
            r2 = np.concatenate([r[:3], [rhs0 + slack], r[3:]])
            out.append(Design(f"vanishing: {name}, slack {slack:+g}", pd, q, A, b, R2, r2, (3, 4, 8), kind, without=(3,)))
    row = A[0].copy()                        # the issue's own probe: A_eq[0] with right-hand side b_eq[0] + 1, as the last row
    out.append(Design("vanishing: A_eq[0] <= b_eq[0] + 1 as the eighth row", pd, q, A, b, np.vstack([R, row]),
                      np.concatenate([r, [b[0] + 1.0]]), (7, 8), "vacuous", without=(7,)))
    return out


LOOSE_OFFSETS = (1e6, 1e9, 1e12, 1e15, 1e18)


def loose_designs():
    out = []
    rng, pd, q, A, b, R, r, xf = _base(0, 12, 3, 8)
    for off in LOOSE_OFFSETS:
        r2 = r.copy()
        r2[7] = R[7] @ xf + off * np.linalg.norm(R[7])
        out.append(Design(f"loose row, offset {off:g}", pd, q, A, b, R, r2, (8,), "loose", without=(7,)))
        order = np.array([7, 0, 1, 2, 3, 4, 5, 6])   # ... and as the FIRST row, before anything else sets the scale
        out.append(Design(f"loose row first, offset {off:g}", pd, q, A, b, R[order], r2[order], (1, 4, 8), "loose", without=(0,)))
    return out


def churn_design(n_solves=300):
    """one new row per solve: tangent planes  d_k . (z - z0) >= rho_k  of a slowly growing ball around the equality-constrained
    minimiser z0, directions inside a cone (so the rows stay feasible): the optimum slides over the ball and the passive set
    of the NNLS turns over -- more than FACTOR_REFRESH = 96 updates and downdates of the kept factor"""
    rng = np.random.RandomState(8)
    n, m = 10, 2
    pd, q = 1.0 + rng.rand(n), rng.randn(n)
    A = rng.randn(m, n)
    b = A @ rng.randn(n)
    z0 = _eq_minimiser(pd, q, A, b)
    Nn = np.linalg.svd(A)[2][m:].T                                 # null-space basis (n x 8)
    axis = Nn @ rng.randn(n - m)
    axis /= np.linalg.norm(axis)
    rows, rhs = [], []
    for k in range(n_solves):
        d = Nn @ rng.randn(n - m)
        d -= (d @ axis) * axis
        d = axis + 0.9 * d / np.linalg.norm(d)
        d /= np.linalg.norm(d)
        rho = 1.0 + 0.01 * k
        rows.append(-d)
        rhs.append(-(rho + d @ z0))
    return Design("churn", pd, q, A, b, np.array(rows), np.array(rhs), tuple(range(1, n_solves + 1)))


# ---- the file format of tests/host/master_host.hip ---------------------------------------------------------------------------
def write_sequence(path, d):
    """int64 [0, n, m_eq, rows, solves]; p, q [n]; A [m_eq][n]; b [m_eq]; R [rows][n]; r [rows]; int64 chunks [solves]"""
    n, m, nr = len(d.q), len(d.b), len(d.r)
    with open(path, "wb") as f:
        np.array([0, n, m, nr, len(d.chunks)], dtype=np.int64).tofile(f)
        for a in (d.pd, d.q, d.A, d.b, d.R, d.r):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        np.array(d.chunks, dtype=np.int64).tofile(f)


def write_nnls(path, A, b, passive, maxiter):
    """int64 [1, m, n, maxiter]; A column-major [n][m]; b [m]; int64 passive [n]"""
    m, n = A.shape
    with open(path, "wb") as f:
        np.array([1, m, n, maxiter], dtype=np.int64).tofile(f)
        np.asfortranarray(A, dtype=np.float64).T.tofile(f)
        np.ascontiguousarray(b, dtype=np.float64).tofile(f)
        np.asarray(passive, dtype=np.int64).tofile(f)


def flat_sequence(create_status, solves, n, nr):
    """what the host program writes for a sequence: create status, then per solve [status, rows, z (n), lam (rows total)]"""
    out = [float(create_status)]
    for st, rows, z, lam in solves:
        pad = np.zeros(nr)
        pad[:len(lam)] = lam
        out += [float(st), float(rows)] + list(z) + list(pad)
    return np.array(out)
