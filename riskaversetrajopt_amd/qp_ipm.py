"""Batched dense convex QP solver: a Mehrotra predictor-corrector interior-point method that solves K small QPs to
completion in ONE launch (csrc/qp_ipm.hip: rato_qp_ipm_batch_f64, one workgroup per problem, fp64).  It serves the QPs of the
driving Gaussian baseline (car/driving_gaussian.py:428-456), which are small (n = 3S + 1, m = 4S + 5) and badly scaled for a
first-order method: an allocation at its lower bound has dg/dalpha ~ -1e5 against O(1) control columns and no cost.

  min 1/2 z'P z + q'z   s.t.   l <= A z <= u          (dense P symmetric PSD, dense A; +-inf = side absent; l == u: equality)

Method.  Rows with l == u are equalities E with multiplier y_E; every other row has slacks s_l = A z - l,
s_u = u - A z (iterates of their own, never recomputed from A z) and multipliers lam_l, lam_u > 0; y_I = lam_u - lam_l.
  residuals   r_d = P z + q + A'y,  r_E = A_E z - l_E,  r_l = (A z - l) - s_l,  r_u = (u - A z) - s_u,  mu = mean(s lam)
  condensed   (P + delta_w I + A_I' D A_I + A_E' A_E / delta_c) dz = -r_d - A'g,     D = lam_l / s_l + lam_u / s_u,
              g_I = (c_u - lam_u r_u) / s_u - (c_l - lam_l r_l) / s_l,  g_E = r_E / delta_c,  delta_c = 1e-10
              ds_l = A dz + r_l,  ds_u = -A dz + r_u,  dlam = (c - lam ds) / s,  dy_E = (A_E dz + r_E) / delta_c
  delta_w = 1e-12, x 100 while the Cholesky fails (at most 12 times); two refinement steps against the matrix without delta_w
  Mehrotra: affine step (c = -s lam), sigma = (mu_aff / mu)^3, corrector c = max(sigma mu, 1e-2 tol) - s lam - ds_aff dlam_aff,
  fraction to the boundary max(0.995, 1 - mu), separate primal and dual step lengths.  The floor on the target: once mu is far
  below tol there is nothing to gain from shrinking it, and a lot to lose -- on the S = 40, alpha = 0.01, SCP-iteration-1 QP
  the dual residual stood at 0.97 tol when mu was 3e-15; one more iteration took mu to 6e-25 and D to 1e23, the Cholesky
  failed through the whole ladder.  With the floor the same QP ends with the dual residual at 3e-11 for every tol tried.
  stop: max(|r_E|, |r_l|, |r_u|) <= tol (1 + |A z|_inf), |r_d|_inf <= tol (1 + max(|P z|, |q|, |A_I'y_I|)_inf), mu <= tol and
  max_i(lam_l |A z - l|, lam_u |u - A z|)_i <= tol: the mean mu bounds no single product (a 61-variable box QP met mu <= 1e-8
  with one product at 2e-7), and the per-row products are what a KKT check of the returned point sees.

``backend='numpy'`` is the same algorithm on the host (the CPU-testable twin); both backends share one host presolve.
"""
import numpy as np

STATUSES = ("solved", "max_iter", "numerical", "invalid")      # the kernel's status codes 0..3; the presolve adds 'infeasible'
DELTA_C = 1e-10
DELTA_W0, DELTA_W_GROWTH, MAX_RETRIES = 1e-12, 100.0, 12
MU_FLOOR = 1e-2                                                 # the corrector's target is max(sigma mu, MU_FLOOR tol)
HARD_CAP = 200                                                  # iterations, whatever max_iter says (the kernel's own cap)
MAX_N, MAX_M = 256, 384                                         # rato_qp_ipm_batch_f64's limits (n <= 193, m <= 261 at S = 64)
INFO_WORDS = 8


# ---- presolve (host, shared by both backends) -----------------------------------------------------------------------------
def presolve(P, q, A, l, u):
    """One problem.  NaN bounds are read as absent (as ``qp.OSQP`` does); rows with no finite side are removed; structurally
    zero rows are removed after checking l <= 0 <= u (else the QP is infeasible); columns that are empty in P, q and every
    kept row are fixed at 0.  -> dict(status 'ok' | 'infeasible', rows, cols [kept indices], P, q, A, l, u [reduced])"""
    l = np.where(np.isnan(l), -np.inf, l)
    u = np.where(np.isnan(u), np.inf, u)
    zero_row = ~np.any(A != 0.0, axis=1) if A.shape[0] else np.zeros(0, dtype=bool)
    if np.any(zero_row & ((l > 0.0) | (u < 0.0))):
        return {"status": "infeasible"}
    keep_r = ~zero_row & (np.isfinite(l) | np.isfinite(u) | (l > u))        # (l = +inf or u = -inf: left for 'invalid')
    rows = np.flatnonzero(keep_r)
    Ar = A[rows]
    used = np.any(P != 0.0, axis=0) | np.any(P != 0.0, axis=1) | (q != 0.0)
    if rows.size:
        used |= np.any(Ar != 0.0, axis=0)
    cols = np.flatnonzero(used)
    return {"status": "ok", "rows": rows, "cols": cols, "P": np.ascontiguousarray(P[np.ix_(cols, cols)]),
            "q": np.ascontiguousarray(q[cols]), "A": np.ascontiguousarray(Ar[:, cols]), "l": l[rows], "u": u[rows]}


# ---- the host twin ----------------------------------------------------------------------------------------------------------
def _step_length(s, ds):
    """largest a in [0, inf] with s + a ds >= 0 (inf when no entry of ds is negative)"""
    neg = ds < 0.0
    return float(np.min(-s[neg] / ds[neg])) if np.any(neg) else np.inf


def solve_numpy(P, q, A, l, u, tol=1e-8, max_iter=100):
    """One presolved problem on the host: the kernel's algorithm step by step.  -> (z, y, info dict)"""
    n, m = q.size, l.size
    info = {"status": "invalid", "iterations": 0, "factorizations": 0, "pres": np.nan, "dres": np.nan, "mu": np.nan, "comp": np.nan}
    bad = not (np.all(np.isfinite(P)) and np.all(np.isfinite(q)) and np.all(np.isfinite(A)))
    bad = bad or np.any(np.isnan(l)) or np.any(np.isnan(u)) or np.any(l > u) or np.any(l == np.inf) or np.any(u == -np.inf)
    if bad:
        return np.full(n, np.nan), np.full(m, np.nan), info
    max_iter = min(int(max_iter), HARD_CAP)
    hasl, hasu = np.isfinite(l), np.isfinite(u)
    eq = hasl & hasu & (l == u)
    hasl, hasu = hasl & ~eq, hasu & ~eq
    nsides = int(hasl.sum() + hasu.sum())
    lf, uf = np.where(np.isfinite(l), l, 0.0), np.where(np.isfinite(u), u, 0.0)
    # start: z = 0, w = A z = 0 moved inside its bounds
    two = hasl & hasu
    mar_l = np.where(two, np.minimum(0.1 * (uf - lf), 1e-2 * np.maximum(1.0, np.abs(lf))), 1e-2 * np.maximum(1.0, np.abs(lf)))
    mar_u = np.where(two, mar_l, 1e-2 * np.maximum(1.0, np.abs(uf)))
    w0 = np.zeros(m)
    w0 = np.where(hasl, np.maximum(w0, lf + mar_l), w0)
    w0 = np.where(hasu, np.minimum(w0, uf - mar_u), w0)
    z = np.zeros(n)
    sl, su = np.where(hasl, w0 - lf, 1.0), np.where(hasu, uf - w0, 1.0)
    ll = np.where(hasl, np.clip(1.0 / sl, 1e-2, 1e4), 0.0)
    lu = np.where(hasu, np.clip(1.0 / su, 1e-2, 1e4), 0.0)          # on E rows lu carries y_E (signed), 0 at the start
    q_inf = float(np.max(np.abs(q)))
    status, it = "max_iter", 0
    pres = dres = mu = comp = np.nan
    with np.errstate(all="ignore"):
        while True:
            Az, Pz = A @ z, P @ z
            yI = np.where(eq, 0.0, lu - ll)
            yE = np.where(eq, lu, 0.0)
            aI, aE = A.T @ yI, A.T @ yE
            rd = Pz + q + (aI + aE)
            rl = np.where(hasl, (Az - lf) - sl, 0.0)
            ru = np.where(hasu, (uf - Az) - su, 0.0)
            rE = np.where(eq, Az - lf, 0.0)
            mu = float((np.sum(np.where(hasl, sl * ll, 0.0)) + np.sum(np.where(hasu, su * lu, 0.0))) / nsides) if nsides else 0.0
            pres = float(max(np.max(np.abs(rl), initial=0.0), np.max(np.abs(ru), initial=0.0), np.max(np.abs(rE), initial=0.0)))
            dres = float(np.max(np.abs(rd)))
            comp = float(max(np.max(np.where(hasl, ll * np.abs(Az - lf), 0.0), initial=0.0),
                             np.max(np.where(hasu, lu * np.abs(uf - Az), 0.0), initial=0.0)))
            if not (np.isfinite(pres) and np.isfinite(dres) and np.isfinite(mu) and np.isfinite(comp)):
                status = "numerical"
                break
            if (pres <= tol * (1.0 + np.max(np.abs(Az), initial=0.0)) and mu <= tol and comp <= tol and
                    dres <= tol * (1.0 + max(float(np.max(np.abs(Pz))), q_inf, float(np.max(np.abs(aI)))))):
                status = "solved"
                break
            if it >= max_iter:
                break
            # the condensed matrix and its factor
            D = np.where(eq, 1.0 / DELTA_C, np.where(hasl, ll / sl, 0.0) + np.where(hasu, lu / su, 0.0))
            K0 = P + A.T @ (D[:, None] * A)
            K0 = np.tril(K0) + np.tril(K0, -1).T
            dw, Lf = DELTA_W0, None
            for _ in range(MAX_RETRIES + 1):
                info["factorizations"] += 1
                try:
                    Lf = np.linalg.cholesky(K0 + dw * np.eye(n))
                    if np.all(np.isfinite(Lf)):
                        break
                    Lf = None
                except np.linalg.LinAlgError:
                    Lf = None
                dw *= DELTA_W_GROWTH
            if Lf is None:
                status = "numerical"
                break

            def kkt(cl, cu):
                g = np.where(eq, rE / DELTA_C, 0.0)
                g = g + np.where(hasu, (cu - lu * ru) / su, 0.0) - np.where(hasl, (cl - ll * rl) / sl, 0.0)
                rhs = -rd - A.T @ g
                solve = lambda b: np.linalg.solve(Lf.T, np.linalg.solve(Lf, b))
                dz = solve(rhs)
                for _ in range(2):
                    dz = dz + solve(rhs - K0 @ dz)
                dAz = A @ dz
                dsl, dsu = np.where(hasl, dAz + rl, 0.0), np.where(hasu, -dAz + ru, 0.0)
                dll = np.where(hasl, (cl - ll * dsl) / sl, 0.0)
                dlu = np.where(eq, (dAz + rE) / DELTA_C, np.where(hasu, (cu - lu * dsu) / su, 0.0))
                return dz, dsl, dsu, dll, dlu

            def lengths(dsl, dsu, dll, dlu):
                ap = min(_step_length(sl[hasl], dsl[hasl]), _step_length(su[hasu], dsu[hasu]))
                ad = min(_step_length(ll[hasl], dll[hasl]), _step_length(lu[hasu], dlu[hasu]))
                return ap, ad
            dz, dsl, dsu, dll, dlu = kkt(-sl * ll, -su * lu)
            ap, ad = lengths(dsl, dsu, dll, dlu)
            ap, ad = min(1.0, ap), min(1.0, ad)
            sigma = 0.0
            if nsides and mu > 0.0:
                mu_aff = (np.sum(np.where(hasl, (sl + ap * dsl) * (ll + ad * dll), 0.0)) +
                          np.sum(np.where(hasu, (su + ap * dsu) * (lu + ad * dlu), 0.0))) / nsides
                r = mu_aff / mu
                sigma = float(r * r * r)
            tgt = max(sigma * mu, MU_FLOOR * tol)
            dz, dsl, dsu, dll, dlu = kkt(tgt - sl * ll - dsl * dll, tgt - su * lu - dsu * dlu)
            ap, ad = lengths(dsl, dsu, dll, dlu)
            tau = max(0.995, 1.0 - mu)
            ap, ad = min(1.0, tau * ap), min(1.0, tau * ad)
            if not (np.isfinite(ap) and np.isfinite(ad) and np.all(np.isfinite(dz)) and np.all(np.isfinite(dlu))
                    and np.all(np.isfinite(dll))):
                status = "numerical"
                break
            z = z + ap * dz
            sl, su = np.where(hasl, sl + ap * dsl, sl), np.where(hasu, su + ap * dsu, su)
            ll = np.where(hasl, ll + ad * dll, ll)
            lu = np.where(hasu | eq, lu + ad * dlu, lu)
            it += 1
    info.update(status=status, iterations=it, pres=pres, dres=dres, mu=mu, comp=comp)
    return z, np.where(eq, lu, lu - ll), info


# ---- the device backend --------------------------------------------------------------------------------------------------
def workspace_bytes(K, n, m):
    from . import _lib
    return int(_lib.load().rato_qp_ipm_workspace_bytes(int(K), int(n), int(m)))


class DeviceBatch:
    """K presolved problems of one shape on the device: ``launch()`` is ONE rato_qp_ipm_batch_f64 call on the current stream
    (stream-ordered, no allocation, repeatable: every launch is a cold start), ``fetch()`` copies (Z, Y, info) back.
    P (K, n, n) / q (K, n) -- or (n, n) / (n,) with ``shared_objective`` (stride 0) --, A (K, m, n), l, u (K, m): host arrays.
    ``lda`` > n pads A's rows with NaN; the outputs are pre-filled with NaN."""

    def __init__(self, P, q, A, l, u, tol=1e-8, max_iter=100, device="cuda:0", lda=None, shared_objective=False):
        import torch
        from . import _lib
        self._lib, self._L = _lib.load(), _lib
        K, m = l.shape
        n = q.shape[-1]
        self.K, self.n, self.m, self.dev = K, n, m, torch.device(device)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.dev)
        self.lda = n if lda is None else int(lda)
        self.mm = max(m, 1)
        Ap = np.full((K, self.mm, self.lda), np.nan)
        Ap[:, :m, :n] = A
        self.P, self.q, self.A, self.l, self.u = t(P), t(q), t(Ap), t(l.reshape(K, m)), t(u.reshape(K, m))
        self.strideP, self.strideq = (0, 0) if shared_objective else (n * n, n)
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=self.dev)
        self.Z, self.Y, self.info = nan(K, n), nan(K, self.mm), nan(K, INFO_WORDS)
        self.nbytes = workspace_bytes(K, n, m)
        self.work = torch.empty(max(self.nbytes // 8, 1), dtype=torch.float64, device=self.dev)
        self.tol, self.max_iter = float(tol), int(max_iter)

    def launch(self):
        import torch
        p = self._L.ptr
        with torch.cuda.device(self.dev):
            self._L.check(self._lib.rato_qp_ipm_batch_f64(
                self.K, self.n, self.m, p(self.P), self.strideP, p(self.q), self.strideq, p(self.A), self.lda, self.mm * self.lda,
                p(self.l), p(self.u), self.m, self.tol, self.max_iter, p(self.Z), self.n, p(self.Y), self.mm, p(self.info),
                p(self.work), self.nbytes, self._L.current_stream()), "rato_qp_ipm_batch_f64")
        return self

    def fetch(self):
        return self.Z.cpu().numpy(), self.Y.cpu().numpy()[:, :self.m], self.info.cpu().numpy()


def solve_device(P, q, A, l, u, tol=1e-8, max_iter=100, device="cuda:0", lda=None, shared_objective=False):
    """``DeviceBatch(...).launch().fetch()`` -> (Z (K, n), Y (K, m), info (K, INFO_WORDS)) as host arrays"""
    return DeviceBatch(P, q, A, l, u, tol, max_iter, device, lda, shared_objective).launch().fetch()


# ---- the public call --------------------------------------------------------------------------------------------------------
def _dense(M):
    return np.asarray(M.toarray() if hasattr(M, "toarray") else M, dtype=np.float64)


def solve_batch(P, q, A, l, u, tol=1e-8, max_iter=100, backend='device', device="cuda:0"):
    """K QPs: P (K, n, n) or (n, n) [shared], q (K, n) or (n,) [shared], A (K, m, n), l, u (K, m).  The presolve runs per problem
    on the host; the problems that are left are grouped by the shape it leaves (the K problems of one SCP iteration share it)
    and each group is ONE launch ('device') or a host loop ('numpy').
    -> (Z (K, n), Y (K, m), info): y with OSQP's sign (y > 0 on an active upper side, y < 0 on an active lower side), 0 on
    removed rows; info = dict(status [K] of 'solved' | 'max_iter' | 'numerical' | 'invalid' | 'infeasible', iterations,
    factorizations (K,) int, pres, dres, mu, comp (K,))"""
    if backend not in ("device", "numpy"):
        raise ValueError(f"backend must be 'device' or 'numpy', got {backend!r}")
    A, l, u = _dense(A), np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)
    P, q = _dense(P), np.asarray(q, dtype=np.float64)
    if A.ndim != 3 or l.shape != A.shape[:2] or u.shape != l.shape:
        raise ValueError(f"A must be (K, m, n) and l, u (K, m), got {A.shape}, {l.shape}, {u.shape}")
    K, m, n = A.shape
    shared = P.ndim == 2
    if (P.shape != ((n, n) if shared else (K, n, n))) or q.shape != ((n,) if q.ndim == 1 else (K, n)) or (q.ndim == 1) != shared:
        raise ValueError(f"P must be (n, n) with q (n,), or (K, n, n) with q (K, n), got {P.shape}, {q.shape}")
    Z, Y = np.zeros((K, n)), np.zeros((K, m))
    info = {"status": [None] * K, "iterations": np.zeros(K, dtype=np.int64), "factorizations": np.zeros(K, dtype=np.int64),
            "pres": np.full(K, np.nan), "dres": np.full(K, np.nan), "mu": np.full(K, np.nan), "comp": np.full(K, np.nan)}
    groups = {}
    for k in range(K):
        pre = presolve(P if shared else P[k], q if shared else q[k], A[k], l[k], u[k])
        if pre["status"] == "infeasible":
            info["status"][k] = "infeasible"
            Z[k], Y[k] = np.nan, np.nan
        elif pre["cols"].size == 0:                                # nothing left to decide: z = 0
            info["status"][k] = "solved"
            info["pres"][k] = info["dres"][k] = info["mu"][k] = info["comp"][k] = 0.0
        else:
            groups.setdefault((tuple(pre["cols"]), pre["rows"].size), []).append((k, pre))
    for (cols, mr), members in groups.items():
        nr = len(cols)
        if backend == "numpy":
            sols = [solve_numpy(p["P"], p["q"], p["A"], p["l"], p["u"], tol, max_iter) for _, p in members]
        else:
            if nr > MAX_N or mr > MAX_M:
                raise ValueError(f"rato_qp_ipm_batch_f64 takes n <= {MAX_N} and m <= {MAX_M}, got {nr}, {mr}")
            Pg = members[0][1]["P"] if shared else np.stack([p["P"] for _, p in members])
            qg = members[0][1]["q"] if shared else np.stack([p["q"] for _, p in members])
            Zg, Yg, ig = solve_device(Pg, qg, np.stack([p["A"] for _, p in members]).reshape(len(members), mr, nr),
                                      np.stack([p["l"] for _, p in members]), np.stack([p["u"] for _, p in members]),
                                      tol, max_iter, device, shared_objective=shared)
            sols = [(Zg[i], Yg[i], {"status": STATUSES[int(ig[i, 0])], "iterations": int(ig[i, 1]),
                                    "factorizations": int(ig[i, 2]), "pres": ig[i, 3], "dres": ig[i, 4], "mu": ig[i, 5],
                                    "comp": ig[i, 7]})
                    for i in range(len(members))]
        for (k, p), (zk, yk, ik) in zip(members, sols):
            Z[k, p["cols"]], Y[k, p["rows"]] = zk, yk
            if not np.all(np.isfinite(zk)):
                Z[k], Y[k] = np.nan, np.nan
            for key in ("iterations", "factorizations", "pres", "dres", "mu", "comp"):
                info[key][k] = ik[key]
            info["status"][k] = ik["status"]
    return Z, Y, info


# ---- the qp.OSQP-shaped object ``driving_gaussian.Model`` holds -----------------------------------------------------------------
class _Info:
    status = "unsolved"
    iter = 0


class _Result:
    def __init__(self, x, y, status, iterations):
        self.x, self.y, self.info = x, y, _Info()
        self.info.status, self.info.iter = status, iterations


class IPM:
    """``setup(P, q, A, l, u)`` / ``update(l=, u=, Ax=)`` / ``solve()`` with ``qp.OSQP``'s result shape (``res.x``, ``res.y``,
    ``res.info.status``).  Every solve is a cold start from z = 0; ``data()`` hands the dense problem to a batched caller."""

    def __init__(self, backend='device', device="cuda:0"):
        self.backend, self.device = backend, device

    def setup(self, P=None, q=None, A=None, l=None, u=None, tol=1e-8, max_iter=100, **_ignored):
        import scipy.sparse as sp
        self._A = sp.csc_matrix(A).astype(np.float64)               # the pattern ``update(Ax=)`` refers to
        self._P, self._q = _dense(P), np.asarray(q, dtype=np.float64).copy()
        self._l, self._u = np.asarray(l, dtype=np.float64).copy(), np.asarray(u, dtype=np.float64).copy()
        self.tol, self.max_iter = float(tol), int(max_iter)
        return self

    def update(self, l=None, u=None, Ax=None):
        if l is not None:
            self._l = np.asarray(l, dtype=np.float64).copy()
        if u is not None:
            self._u = np.asarray(u, dtype=np.float64).copy()
        if Ax is not None:
            Ax = np.asarray(Ax, dtype=np.float64)
            if Ax.shape != self._A.data.shape:
                raise ValueError(f"Ax must hold the {self._A.data.size} values of the set-up pattern, got {Ax.shape}")
            self._A.data = Ax.copy()

    def data(self):
        return self._P, self._q, self._A.toarray(), self._l, self._u

    def result(self, x, y, status, iterations=0):
        self.res = _Result(x, y, status, iterations)
        return self.res

    def solve(self):
        P, q, A, l, u = self.data()
        Z, Y, info = solve_batch(P, q, A[None], l[None], u[None], self.tol, self.max_iter, self.backend, self.device)
        return self.result(Z[0], Y[0], info["status"][0], int(info["iterations"][0]))
