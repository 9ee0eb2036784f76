"""The lockstep primal-dual interior-point method, model-independent: ``hopper_ipm`` and ``drone_gaussian_ipm``
run it on backends of their own.

  min f(z)  s.t.  gL <= g(z) <= gU,  xL <= z <= xU

Rows with gL == gU are equalities E; every other row I gets a slack, g_I(z) - s = 0, gL_I <= s <= gU_I.  v = (z, s).  A bound
with |b| >= 1e14 is absent; present bounds are relaxed outward by 1e-8 max(1, |b|) (IPOPT's bound_relax_factor).  The objective
is scaled by sf = min(1, 100 / max |grad f(Z0)|).

Newton step, condensed.  With Sigma = zl / (v - vL) + zu / (vU - v), eliminating s and y_I:
  Kc = W + diag(Sigma_z) + delta_w I + J_I' diag(Sigma_s) J_I + (1 / delta_c) J_E' J_E
  Kc dz = -r_z - J' w,   w = d c + (r_s on I, 0 on E),   d = (Sigma_s on I, 1 / delta_c on E)
  dy_E = (J_E dz + c_E) / delta_c,   ds = J_I dz + c_I,   dy_I = Sigma_s ds + r_s
delta_c = 1e-8 mu^(1/4) is always on (it tolerates redundant rows); delta_w = 0, 1e-4, then x 8 until the Cholesky of Kc
succeeds: Kc positive definite <=> the regularised KKT matrix has the right inertia, so the factorization is the inertia test.
Two steps of iterative refinement follow against the system with the equality block NOT condensed (unknowns dz, dy_E),
re-using the factor.

The driver (``Problem``, ``newton_steps``, ``solve_group``, ``solve_groups``) knows a model through num_vars, gL_gU(),
x_bounds(), f, grad_f and a backend through name, clock, eval_full / eval_g / matvec / tmatvec / factor / solve /
hess_apply(idx, X) -> [W x].  It, the line search and the O(n + m) vector algebra run on the host per problem, so a problem's
iterates do not depend on what else is in the batch.  ``Backend`` / ``DeviceBase`` hold what the backends have in common: the
clocks, the Cholesky on the host and on the device (``chol_factor`` / ``chol_solve``: csrc/chol.hip, or csrc/chol_grid.hip
with ``chol='grid'``: the same bits from launches spread over the device), uploads and row selection,
and ``factor`` / ``solve`` (``DeviceBase``: ``factor_t`` / ``solve_t`` too) on the normal matrix a subclass provides:
``normal_matrix_host(i, d, diag)`` on the host, ``normal_matrix(idx, D, diags)`` / ``normal_matrix_t(d, diag, out=)`` on the device.

``solve_group_device`` (``driver='device'``) is the same method with the iterate on the device: ``DeviceState``
holds the state of the K problems in HBM, the vector algebra above is csrc/ipm_driver.hip, and the host keeps the branches
it needs a read-back for: who is still running, the delta_w ladder, who is still searching.  There the objective is
sf (1/2 sum curv z^2 + lin . z): the model gives ``curv`` and, if it has a linear part, ``lin`` (both (n,)).
``driver='device_grid'`` is the same driver with that vector algebra spread over the rows of a problem
(csrc/ipm_driver_grid.hip, ``DeviceState(vec='grid')``): the same bits from more launches, for problems of many thousands of rows.
"""
import contextlib
import functools
import time

import numpy as np

ABSENT = 1e14
STATUSES = ("converged", "max_iter", "line_search")


# ---- the Cholesky (csrc/chol.hip) --------------------------------------------------------------------------------------------
def chol_panel_width():
    from . import _lib
    return int(_lib.load().rato_chol_panel_width())


CHOL_METHODS = ("workgroup", "grid")


def check_chol(method, what="chol"):
    """-> method, one of CHOL_METHODS; anything else is a ValueError (raised before any device call)"""
    if method not in CHOL_METHODS:
        raise ValueError(f"{what} must be one of {CHOL_METHODS}, got {method!r}")
    return method


def chol_grid_work(n, K, device):
    """the scratch ``chol_factor(method='grid')`` needs for K problems of size n: a device fp64 tensor of
    K * rato_chol_grid_work_doubles(n) doubles (contents irrelevant; empty when the query returns 0)"""
    import torch
    from . import _lib
    return torch.empty(int(K) * int(_lib.load().rato_chol_grid_work_doubles(int(n))), dtype=torch.float64, device=device)


def chol_factor(A, method='workgroup', work=None):
    """rato_chol_factor_batch_f64 in place on a device fp64 tensor A (K, n, lda) (row-major lower triangle; lda >= n)
    -> info (K,) int32 device tensor: 0, or j + 1 for the first pivot j that is not positive and finite.
    method='grid': rato_chol_factor_grid_batch_f64 (csrc/chol_grid.hip), bitwise the same L, on ``work`` (``chol_grid_work``;
    None = allocated here)"""
    import torch
    from . import _lib
    check_chol(method, "method")
    if A.dim() != 3 or A.dtype != torch.float64 or not A.is_cuda or not A.is_contiguous() or A.shape[2] < A.shape[1] or A.shape[1] < 1:
        raise ValueError(f"A must be a contiguous device float64 tensor (K, n, lda >= n), got {tuple(A.shape)}")
    info = torch.empty(A.shape[0], dtype=torch.int32, device=A.device)
    if method == 'grid':
        lib = _lib.load()
        need = A.shape[0] * int(lib.rato_chol_grid_work_doubles(A.shape[1]))
        if work is None:
            work = torch.empty(need, dtype=torch.float64, device=A.device)
        elif work.dtype != torch.float64 or work.device != A.device or not work.is_contiguous() or work.numel() < need:
            raise ValueError(f"work must be a contiguous float64 tensor of at least {need} doubles on {A.device}")
        with torch.cuda.device(A.device):
            _lib.check(lib.rato_chol_factor_grid_batch_f64(_lib.ptr(A), A.shape[1], A.shape[2], A.shape[0], _lib.ptr(info),
                                                           _lib.ptr(work) if need else None, _lib.current_stream()),
                       "rato_chol_factor_grid_batch_f64")
        return info
    with torch.cuda.device(A.device):
        _lib.check(_lib.load().rato_chol_factor_batch_f64(_lib.ptr(A), A.shape[1], A.shape[2], A.shape[0], _lib.ptr(info),
                                                          _lib.current_stream()), "rato_chol_factor_batch_f64")
    return info


def chol_solve(L, B, method='workgroup'):
    """rato_chol_solve_batch_f64: L (K, n, lda) as chol_factor leaves it, B (K, nrhs, ldb >= n) device fp64, solved in place.
    method='grid': rato_chol_solve_grid_batch_f64, bitwise the same X"""
    import torch
    from . import _lib
    check_chol(method, "method")
    if L.dim() != 3 or B.dim() != 3 or L.dtype != torch.float64 or B.dtype != torch.float64 or not (L.is_contiguous() and B.is_contiguous()) \
            or B.shape[0] != L.shape[0] or B.shape[2] < L.shape[1] or L.shape[2] < L.shape[1] or L.device != B.device or not L.is_cuda:
        raise ValueError("chol_solve: L (K, n, lda >= n) and B (K, nrhs, ldb >= n) contiguous device float64 tensors")
    name = "rato_chol_solve_grid_batch_f64" if method == 'grid' else "rato_chol_solve_batch_f64"
    with torch.cuda.device(L.device):
        _lib.check(getattr(_lib.load(), name)(_lib.ptr(L), L.shape[1], L.shape[2], L.shape[0], _lib.ptr(B), B.shape[1],
                                              B.shape[2], _lib.current_stream()), name)
    return B


# ---- what every backend repeats ------------------------------------------------------------------------------------------------
class Backend:
    """the clocks of a backend, and the host's Cholesky: factors kept per problem in ``self.L``"""

    def __init__(self, *more_clocks):
        self.clock = dict.fromkeys(("callbacks", "normal", "factor", "solve") + more_clocks, 0.0)
        self.L = {}

    @contextlib.contextmanager
    def timed(self, key):
        """adds the seconds spent in the block to clock[key]"""
        t0 = time.perf_counter()
        yield
        self.clock[key] += time.perf_counter() - t0

    def factor_host(self, i, Kc, ok=True):
        """the Cholesky factor of Kc as problem i's L -> 0, or 1 when ``ok`` is false or Kc is not finite and positive definite"""
        ok = ok and bool(np.all(np.isfinite(Kc)))
        if ok:
            try:
                self.L[i] = np.linalg.cholesky(Kc)
            except np.linalg.LinAlgError:
                ok = False
        return 0 if ok else 1

    def solve_host(self, i, b):
        from scipy.linalg import solve_triangular
        return solve_triangular(self.L[i], solve_triangular(self.L[i], b, lower=True), lower=True, trans='T')

    def factor(self, idx, D, diags):
        """one problem after the other: ``normal_matrix_host(i, d, diag)`` -> Kc (n, n), the subclass's, then its Cholesky"""
        info = []
        for i, d, dg in zip(idx, D, diags):
            with self.timed("normal"):
                Kc = self.normal_matrix_host(i, d, dg)
            with self.timed("factor"):
                info.append(self.factor_host(i, Kc))
        return info

    def solve(self, idx, B):
        with self.timed("solve"):
            return [self.solve_host(i, b) for i, b in zip(idx, B)]


class DeviceBase(Backend):
    """what the device backends share: the uploads, ``slot`` (problem -> row of the current value arrays) and the Cholesky on
    the device with the factors of all ``n_all`` problems of the group kept in one tensor.  ``factor`` / ``solve`` / ``factor_t``
    stand on the subclass's ``normal_matrix(idx, D, diags)`` and ``normal_matrix_t(d, diag, out=)`` -> Kc (K, n, lda)."""

    def __init__(self, dev, n_all, *more_clocks, chol='workgroup'):
        import torch
        super().__init__(*more_clocks)
        self.torch, self.dev, self.n_all = torch, dev, n_all
        self.slot, self.L, self.Kc = {}, None, None
        self.chol, self.chol_work = check_chol(chol), None

    def chol_factor(self, Kc):
        """``chol_factor`` by the backend's method; the grid form's scratch is allocated once, for n_all problems of Kc's n"""
        if self.chol != 'grid':
            return chol_factor(Kc)
        if self.chol_work is None:
            self.chol_work = chol_grid_work(Kc.shape[1], max(self.n_all, Kc.shape[0]), self.dev)
        return chol_factor(Kc, method='grid', work=self.chol_work)

    def chol_solve(self, L, B):
        return chol_solve(L, B) if self.chol != 'grid' else chol_solve(L, B, method='grid')

    def _sync(self):
        self.torch.cuda.synchronize(self.dev)

    def _up(self, rows):
        return self.torch.as_tensor(np.ascontiguousarray(np.stack(rows), dtype=np.float64), device=self.dev)

    def _rows(self, idx, *tensors):
        """the rows of the value arrays that hold the listed problems, in place when they are all of them in order"""
        rows = [self.slot[i] for i in idx]
        if rows == list(range(tensors[0].shape[0])):
            return tensors
        sel = self.torch.as_tensor(rows, device=self.dev)
        return tuple(t.index_select(0, sel).contiguous() for t in tensors)

    def factor_device(self, idx, Kc):
        """factors Kc (K, n, lda) in place and keeps it as the listed problems' L -> info as a list"""
        torch = self.torch
        info = self.chol_factor(Kc)
        if self.L is None:
            self.L = torch.empty((self.n_all,) + tuple(Kc.shape[1:]), dtype=torch.float64, device=self.dev)
        self.L[torch.as_tensor(list(idx), device=self.dev)] = Kc
        return [int(v) for v in info.cpu().numpy()]

    def solve_device(self, idx, B):
        """L L' x = b for the listed problems from their kept factors, B host vectors -> (K, n) host array"""
        L = self.L.index_select(0, self.torch.as_tensor(list(idx), device=self.dev))
        b = self._up(B)[:, None, :].contiguous()
        self.chol_solve(L, b)
        return b[:, 0].cpu().numpy()

    def factor(self, idx, D, diags):
        with self.timed("normal"):
            Kc = self.normal_matrix(idx, D, diags)
            self._sync()
        with self.timed("factor"):
            return self.factor_device(idx, Kc)

    def solve(self, idx, B):
        with self.timed("solve"):
            return list(self.solve_device(idx, B))

    # ---- for the driver on the device (``solve_group_device``): launches are not waited for
    sync_clocks = False

    @contextlib.contextmanager
    def timed_t(self, key):
        """``timed`` around asynchronous launches: the clock holds the time to launch, or, with ``sync_clocks`` set (the
        per-iteration split of a measurement), the time until the device has finished the block"""
        t0 = time.perf_counter()
        yield
        if self.sync_clocks:
            self._sync()
        self.clock[key] = self.clock.get(key, 0.0) + time.perf_counter() - t0

    def factor_all(self, Kc):
        """factors Kc (K, n, lda) of the whole group in place and keeps it as L -> info (K,) int32 device tensor"""
        with self.timed_t("factor"):
            info = self.chol_factor(Kc)
            self.L = Kc
        return info

    def factor_t(self, d, diag):
        """the normal matrix of the whole group into the kept ``self.Kc``, factored in place -> info (K,) device tensor"""
        with self.timed_t("normal"):
            self.Kc = self.normal_matrix_t(d, diag, out=self.Kc)
        return self.factor_all(self.Kc)

    def solve_t(self, B):
        """L L' x = b in place on B (K, ld >= n), a device tensor, from the factors ``factor_all`` kept"""
        with self.timed_t("solve"):
            self.chol_solve(self.L, B[:, None, :])
        return B


# ---- the method ------------------------------------------------------------------------------------------------------------
class Problem:
    """one problem's iterate and constants (host, fp64)"""

    def __init__(self, model, Z0, g0, tol):
        self.model, self.tol = model, float(tol)
        n = self.n = model.num_vars
        gL, gU = model.gL_gU()
        xL, xU = model.x_bounds()
        self.m = gL.size
        self.E = gL == gU
        self.I = ~self.E
        self.gE = gL[self.E]
        vL, vU = np.concatenate([xL, gL[self.I]]), np.concatenate([xU, gU[self.I]])
        self.hasL, self.hasU = np.abs(vL) < ABSENT, np.abs(vU) < ABSENT
        vL = np.where(self.hasL, vL - 1e-8 * np.maximum(1.0, np.abs(vL)), -np.inf)
        vU = np.where(self.hasU, vU + 1e-8 * np.maximum(1.0, np.abs(vU)), np.inf)
        self.vL, self.vU = vL, vU
        v = np.concatenate([np.asarray(Z0, dtype=np.float64), g0[self.I]])
        with np.errstate(invalid='ignore'):
            width = np.where(self.hasL & self.hasU, 1e-2 * (vU - vL), np.inf)
        fin = lambda b, has: np.where(has, b, 0.0)
        pL = np.minimum(1e-2 * np.maximum(1.0, np.abs(fin(vL, self.hasL))), width)
        pU = np.minimum(1e-2 * np.maximum(1.0, np.abs(fin(vU, self.hasU))), width)
        v = np.where(self.hasL, np.maximum(v, fin(vL, self.hasL) + pL), v)
        v = np.where(self.hasU, np.minimum(v, fin(vU, self.hasU) - pU), v)
        self.v = v
        self.zl, self.zu = self.hasL.astype(np.float64), self.hasU.astype(np.float64)
        self.y = np.zeros(self.m)
        self.mu, self.nu, self.dw = 0.1, 0.0, 0.0
        gf = model.grad_f(Z0)
        self.sf = min(1.0, 100.0 / max(np.max(np.abs(gf)), 1e-300))
        self.done, self.status = False, None
        self.iterations = self.factorizations = 0
        self.E0 = self.prim = self.dual = np.inf

    @property
    def z(self):
        return self.v[:self.n]

    def residuals(self, g, JTy):
        """c (m,), the dual residual of (z, s), and E_mu as a function of mu"""
        n = self.n
        c = np.empty(self.m)
        c[self.E] = g[self.E] - self.gE
        c[self.I] = g[self.I] - self.v[n:]
        self.gradf = self.sf * self.model.grad_f(self.z)
        rz = self.gradf + JTy - self.zl[:n] + self.zu[:n]
        rs = -self.y[self.I] - self.zl[n:] + self.zu[n:]
        self.c, self.JTy = c, JTy
        self.dual = max(np.max(np.abs(rz)), np.max(np.abs(rs)) if rs.size else 0.0)
        self.prim = np.max(np.abs(c))
        with np.errstate(invalid='ignore'):
            self.dL, self.dU = self.v - self.vL, self.vU - self.v
        self.cl = np.where(self.hasL, self.zl * np.where(self.hasL, self.dL, 0.0), 0.0)
        self.cu = np.where(self.hasU, self.zu * np.where(self.hasU, self.dU, 0.0), 0.0)

    def error(self, mu):
        comp = 0.0
        if np.any(self.hasL):
            comp = max(comp, np.max(np.abs(self.cl[self.hasL] - mu)))
        if np.any(self.hasU):
            comp = max(comp, np.max(np.abs(self.cu[self.hasU] - mu)))
        return max(self.dual, self.prim, comp)

    def barrier(self, v):
        with np.errstate(invalid='ignore', divide='ignore'):
            return -self.mu * (np.sum(np.log((v - self.vL)[self.hasL])) + np.sum(np.log((self.vU - v)[self.hasU])))

    def c_of(self, g, v):
        c = np.empty(self.m)
        c[self.E] = g[self.E] - self.gE
        c[self.I] = g[self.I] - v[self.n:]
        return c

    def prepare_step(self):
        """Sigma, the barrier gradient, the row weights d and the vector w of the condensed right-hand side"""
        n, mu = self.n, self.mu
        iL, iU = 1.0 / np.where(self.hasL, self.dL, np.inf), 1.0 / np.where(self.hasU, self.dU, np.inf)
        self.Sigma = self.zl * iL + self.zu * iU
        self.gbar = -mu * iL + mu * iU                               # the barrier's gradient in v
        self.rz = self.gradf + self.JTy + self.gbar[:n]
        self.rs = -self.y[self.I] + self.gbar[n:]
        self.dc = 1e-8 * mu ** 0.25
        d = np.empty(self.m)
        d[self.E] = 1.0 / self.dc
        d[self.I] = self.Sigma[n:]
        self.d = d
        w = d * self.c
        w[self.I] += self.rs
        self.w = w


def newton_steps(be, idx, ps, refine=2):
    """the condensed Newton step of the listed problems (``Problem.prepare_step`` done) on backend ``be``: fills p.dv (n + nI)
    and p.dy (m).  A failed factorization is redone with the next delta_w; returns False for a problem where none succeeded."""
    JTw = be.tmatvec(idx, [p.w for p in ps])
    for p, t in zip(ps, JTw):
        p.rhs = -(p.rz + t)
        p.dw, p.fact_ok = 0.0, False
    todo = list(range(len(ps)))
    for _ in range(60):
        info = be.factor([idx[k] for k in todo], [ps[k].d for k in todo], [ps[k].Sigma[:ps[k].n] + ps[k].dw for k in todo])
        nxt = []
        for k, bad in zip(todo, info):
            ps[k].factorizations += 1
            if bad:
                ps[k].dw = 1e-4 if ps[k].dw == 0.0 else 8.0 * ps[k].dw
                nxt.append(k)
            else:
                ps[k].fact_ok = True
        todo = nxt
        if not todo:
            break
    good = [k for k in range(len(ps)) if ps[k].fact_ok]
    if not good:
        return [False] * len(ps)
    gi, gp = [idx[k] for k in good], [ps[k] for k in good]
    for p, x in zip(gp, be.solve(gi, [p.rhs for p in gp])):
        p.dz = x
    for it in range(refine + 1):
        Jdz = be.matvec(gi, [p.dz for p in gp])
        for p, jd in zip(gp, Jdz):
            p.Jdz = jd
            lin = jd + p.c
            if it == 0:
                p.dyE = lin[p.E] / p.dc
        if it == refine:
            break
        Q = []
        for p in gp:
            lin = p.Jdz + p.c
            p.r2 = -lin[p.E] + p.dc * p.dyE                        # the equality block's residual, kept apart from dz's
            q = np.empty(p.m)
            q[p.I] = p.Sigma[p.n:] * lin[p.I] + p.rs
            q[p.E] = p.dyE - p.r2 / p.dc
            Q.append(q)
        JTq = be.tmatvec(gi, Q)
        Wdz = be.hess_apply(gi, [p.dz for p in gp])
        R = [-(p.rz + h + (p.Sigma[:p.n] + p.dw) * p.dz + t) for p, h, t in zip(gp, Wdz, JTq)]
        ez = be.solve(gi, R)
        Jez = be.matvec(gi, ez)
        for p, e, je in zip(gp, ez, Jez):
            p.dz = p.dz + e
            p.dyE = p.dyE + (je[p.E] - p.r2) / p.dc
    for p in gp:
        ds = p.Jdz[p.I] + p.c[p.I]
        p.dv = np.concatenate([p.dz, ds])
        dy = np.empty(p.m)
        dy[p.E] = p.dyE
        dy[p.I] = p.Sigma[p.n:] * ds + p.rs
        p.dy = dy
    return [p.fact_ok for p in ps]


def kkt_residual(p, J, W):
    """relative residual of (p.dv, p.dy) in the UNCONDENSED regularised KKT system (unknowns dz, ds, dy_E, dy_I) with dense J
    (m, n) and W (n, n):  max |K x - b| / max |b|"""
    n = p.n
    dz, ds, dy = p.dv[:n], p.dv[n:], p.dy
    JE, JI = J[p.E], J[p.I]
    r1 = (W @ dz + (p.Sigma[:n] + p.dw) * dz + JE.T @ dy[p.E] + JI.T @ dy[p.I]) + p.rz
    r2 = p.Sigma[n:] * ds - dy[p.I] + p.rs
    r3 = JE @ dz - p.dc * dy[p.E] + p.c[p.E]
    r4 = JI @ dz - ds + p.c[p.I]
    b = np.concatenate([p.rz, p.rs, p.c[p.E], p.c[p.I]])
    return float(np.max(np.abs(np.concatenate([r1, r2, r3, r4]))) / np.max(np.abs(b)))


def _max_step(x, dx, has, tau):
    """largest alpha in (0, 1] with x + alpha dx >= (1 - tau) x (x: distances to a bound or multipliers, all positive)"""
    m = has & (dx < 0)
    if not np.any(m):
        return 1.0
    return float(min(1.0, np.min(-tau * x[m] / dx[m])))


def _print_iteration(it, rows):
    """the verbose line of both drivers; a row: (mu, E0, prim, dual, alpha, dw) of one problem"""
    print("it %4d " % it + " | ".join("mu %.1e E0 %.2e pr %.1e du %.1e a %.1e dw %.0e" % tuple(r) for r in rows))


def _results(ps, be, **more):
    """what both drivers return: [(Z, info)] of the ended Problems; one that never ended ran out of iterations"""
    out = []
    for p in ps:
        if p.status is None:
            p.status = "max_iter"
        info = dict(status=p.status, iterations=p.iterations, factorizations=p.factorizations, E0=float(p.E0),
                    primal_infeasibility=float(p.prim), dual_infeasibility=float(p.dual), f=p.model.f(p.z), mu=p.mu, sf=p.sf,
                    y=p.y.copy(), zl=p.zl.copy(), zu=p.zu.copy(), s=p.v[p.n:].copy(), backend=be.name, **more)
        out.append((p.z.copy(), info))
    return out


def solve_group(models, Z0s, tol, max_iter, be, verbose):
    K = len(models)
    all_idx = list(range(K))
    g0 = be.eval_g(all_idx, [np.asarray(Z, dtype=np.float64) for Z in Z0s])
    ps = [Problem(m, Z, g, tol) for m, Z, g in zip(models, Z0s, g0)]
    for it in range(max_iter + 1):
        idx = [i for i in all_idx if not ps[i].done]
        if not idx:
            break
        act = [ps[i] for i in idx]
        G = be.eval_full(idx, [p.z.copy() for p in act], [p.y for p in act], [p.sf for p in act])
        JTy = be.tmatvec(idx, [p.y for p in act])
        for p, g, t in zip(act, G, JTy):
            p.g = g
            p.residuals(g, t)
            p.E0 = p.error(0.0)
            if not np.isfinite(p.E0):
                p.done, p.status = True, "line_search"
            elif p.E0 <= tol:
                p.done, p.status = True, "converged"
            elif it == max_iter:
                p.done, p.status = True, "max_iter"
            else:
                while p.error(p.mu) <= 10.0 * p.mu and p.mu > tol / 10.0:
                    p.mu = max(tol / 10.0, min(0.2 * p.mu, p.mu ** 1.5))
                    p.nu = 0.0
                p.prepare_step()
        pairs = [(i, p) for i, p in zip(idx, act) if not p.done]
        if not pairs:
            continue
        idx, act = [i for i, _ in pairs], [p for _, p in pairs]
        ok = newton_steps(be, idx, act)
        search = []
        gi = [i for i, good in zip(idx, ok) if good]
        Wdv = dict(zip(gi, be.hess_apply(gi, [p.dv[:p.n] for p, good in zip(act, ok) if good]))) if gi else {}
        for i, p, good in zip(idx, act, ok):
            if not good:
                p.done, p.status = True, "line_search"
                continue
            n, mu = p.n, p.mu
            tau = max(0.99, 1.0 - mu)
            dv = p.dv
            iL, iU = 1.0 / np.where(p.hasL, p.dL, np.inf), 1.0 / np.where(p.hasU, p.dU, np.inf)
            p.dzl = np.where(p.hasL, mu * iL - p.zl - p.zl * iL * dv, 0.0)
            p.dzu = np.where(p.hasU, mu * iU - p.zu + p.zu * iU * dv, 0.0)
            p.a_max = min(_max_step(np.where(p.hasL, p.dL, 1.0), dv, p.hasL, tau),
                          _max_step(np.where(p.hasU, p.dU, 1.0), -dv, p.hasU, tau))
            p.a_dual = min(_max_step(p.zl, p.dzl, p.hasL, tau), _max_step(p.zu, p.dzu, p.hasU, tau))
            c1 = float(np.sum(np.abs(p.c)))
            Dbar = float(p.gradf @ dv[:n] + p.gbar @ dv)
            quad = float(dv[:n] @ Wdv[i] + np.sum(p.Sigma * dv * dv) + p.dw * (dv[:n] @ dv[:n]))
            if c1 > 0.0:
                nu_trial = (Dbar + 0.5 * max(quad, 0.0)) / (0.9 * c1)
                if p.nu < nu_trial:
                    p.nu = nu_trial + 1.0
            p.Dphi = min(Dbar - p.nu * c1, 0.0)
            p.phi = p.sf * p.model.f(p.z) + p.barrier(p.v) + p.nu * c1
            p.alpha, p.trials, p.accepted = p.a_max, 0, False
            search.append((i, p))
        while search:
            trial_v = [p.v + p.alpha * p.dv for _, p in search]
            Gt = be.eval_g([i for i, _ in search], [v[:p.n].copy() for v, (_, p) in zip(trial_v, search)])
            nxt = []
            for (i, p), v, g in zip(search, trial_v, Gt):
                phi_t = p.sf * p.model.f(v[:p.n]) + p.barrier(v) + p.nu * float(np.sum(np.abs(p.c_of(g, v))))
                p.trials += 1
                if np.isfinite(phi_t) and phi_t <= p.phi + 1e-8 * p.alpha * p.Dphi + 10.0 * np.finfo(float).eps * abs(p.phi):
                    p.v = v
                    p.y = p.y + p.alpha * p.dy
                    p.zl = p.zl + p.a_dual * p.dzl
                    p.zu = p.zu + p.a_dual * p.dzu
                    with np.errstate(invalid='ignore'):
                        dL, dU = np.where(p.hasL, p.v - p.vL, 1.0), np.where(p.hasU, p.vU - p.v, 1.0)
                    p.zl = np.where(p.hasL, np.clip(p.zl, p.mu / dL / 1e10, 1e10 * p.mu / dL), 0.0)   # kappa_Sigma
                    p.zu = np.where(p.hasU, np.clip(p.zu, p.mu / dU / 1e10, 1e10 * p.mu / dU), 0.0)
                    p.iterations += 1
                elif p.trials >= 40:
                    p.done, p.status = True, "line_search"
                else:
                    p.alpha *= 0.5
                    nxt.append((i, p))
            search = nxt
        if verbose:
            _print_iteration(it, [(p.mu, p.E0, p.prim, p.dual, getattr(p, "alpha", 0.0), p.dw) for p in act])
    return _results(ps, be)


# ---- the driver on the device (csrc/ipm_driver.hip) -----------------------------------------------------------------
DRIVERS = ("host", "device", "device_grid")
VECS = ("workgroup", "grid")
VEC_OF_DRIVER = {"device": "workgroup", "device_grid": "grid"}       # the form of the driver's own vector kernels (§7.al)


def on_device(driver):
    """whether ``driver`` keeps the iterate on the device ('device', or 'device_grid': the same with its vector kernels
    spread over the rows, csrc/ipm_driver_grid.hip)"""
    return driver in VEC_OF_DRIVER


def check_driver(driver, backend):
    if driver not in DRIVERS:
        raise ValueError(f"driver must be 'host', 'device' or 'device_grid', got {driver!r}")
    if on_device(driver) and backend != 'device':
        raise ValueError(f"driver={driver!r} keeps the iterate on the device: it needs backend='device', got {backend!r}")


def g_rows(n, g0, J1, z, out=None):
    """rato_ipm_g_rows_f64 on device fp64 tensors: g0 (K, m0), the shared block J1 (m1, ld1 >= n), z (K, ldz >= n)
    -> g (K, m0 + m1) = (g0, J1 z)"""
    import torch
    from . import _lib
    K, m0, m1 = z.shape[0], g0.shape[1], J1.shape[0]
    g = torch.empty((K, m0 + m1), dtype=torch.float64, device=z.device) if out is None else out
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().rato_ipm_g_rows_f64(K, n, _lib.ptr(g0), m0, g0.shape[1], _lib.ptr(J1), m1, J1.shape[1], _lib.ptr(z),
                                                   z.shape[1], _lib.ptr(g), g.shape[1], _lib.current_stream()), "rato_ipm_g_rows_f64")
    return g


class DeviceState:
    """The iterates, constants and work vectors of K problems of one shape as rows of device arrays (rato_ipm_state of
    include/rato_saa.h), built from host ``Problem``s and downloadable back into them.  Vectors of length nv = n + nI or n lie in
    (K, ldv) arrays, vectors over the m rows in (K, ldm) arrays; ``rs`` / ``dyE`` / ``r2``, which the host keeps packed over the
    inequality / equality rows, are spread over the rows.  Whatever of a Problem's work vectors exists is uploaded too, so a
    phase can be run from any host state.  ``fill`` is what the padding and the work vectors that do not exist yet hold.
    The methods are the kernels: ``residuals``, ``newton``, ``step_setup``, ``trial``, ``accept``; ``record()`` reads the
    (K, RATO_IPM_REC) scalars back -- the only read-back an iteration needs.  ``vec``: 'workgroup' (csrc/ipm_driver.hip, one
    workgroup per problem) or 'grid' (csrc/ipm_driver_grid.hip, DESIGN §7.al: the rows spread over the device, bitwise the
    same state after every method; its scratch, ``work``, is allocated here once)."""
    NV = ("v", "zl", "zu", "vL", "vU", "Sigma", "gbar", "dv", "dzl", "dzu", "vt")
    N = ("curv", "lin", "gradf", "rz", "dz", "ez")
    M = ("y", "gL", "c", "d", "w", "rs", "dyE", "r2", "q", "dy")
    SCALARS = ("mu", "nu", "dw", "dc", "tol", "E0", "prim", "dual", "a_max", "a_dual", "Dphi", "phi", "alpha", "sf")

    def __init__(self, ps, dev, ldv=None, ldm=None, fill=np.nan, vec='workgroup'):
        import torch
        from . import _lib
        if vec not in VECS:
            raise ValueError(f"vec must be 'workgroup' or 'grid', got {vec!r}")
        self.vec = vec
        p0 = ps[0]
        self.K, self.n, self.m, self.nI = len(ps), p0.n, p0.m, int(np.sum(p0.I))
        self.nv = self.n + self.nI
        if any(p.n != p0.n or p.m != p0.m or not np.array_equal(p.E, p0.E) for p in ps):
            raise ValueError("the problems of a DeviceState share n, m and the equality rows")
        self.ldv, self.ldm = self.nv if ldv is None else int(ldv), self.m if ldm is None else int(ldm)
        if self.ldv < self.nv or self.ldm < self.m:
            raise ValueError("ldv >= n + nI and ldm >= m")
        self.torch, self.dev, self.lib = torch, torch.device(dev), _lib
        self.E, self.I = p0.E.copy(), p0.I.copy()
        slack = np.full(self.m, -1, dtype=np.int32)
        slack[self.I] = np.arange(self.nI, dtype=np.int32)
        self.row_slack = torch.as_tensor(slack, device=self.dev)
        host = {k: np.full((self.K, self.ldv), fill) for k in self.NV + self.N}
        host.update({k: np.full((self.K, self.ldm), fill) for k in self.M})
        rec = np.zeros((self.K, _lib.IPM_REC))
        F = {k: i for i, k in enumerate(_lib.IPM_FIELDS)}
        for k, p in enumerate(ps):
            for name in self.NV + self.N + self.M:
                a = self._host_vector(p, name)
                if a is not None:
                    host[name][k, :a.size] = a
            for name in self.SCALARS:
                if hasattr(p, name):
                    rec[k, F[name]] = float(getattr(p, name))
            rec[k, F["iterations"]] = p.iterations
            rec[k, F["trials"]] = getattr(p, "trials", 0)
            rec[k, F["status"]] = STATUSES.index(p.status) if p.done else _lib.IPM_RUNNING
        for name, a in host.items():
            setattr(self, name, torch.as_tensor(a, device=self.dev))
        self.diag = torch.full((self.K, self.n), float(fill), dtype=torch.float64, device=self.dev)
        self.rec = torch.as_tensor(rec, device=self.dev)
        self.F = F
        fields = [k for k, _ in _lib.IpmState._fields_]              # the struct's pointers follow ldm, named as the tensors are
        self.c_state = _lib.IpmState(self.K, self.n, self.nI, self.m, self.ldv, self.ldm,
                                     *[getattr(self, k).data_ptr() for k in fields[fields.index("ldm") + 1:]])
        self.work = None
        if vec == 'grid':
            size = _lib.load().rato_ipm_grid_work_doubles(self.n, self.nI, self.m, self.K)
            self.work = torch.empty(size, dtype=torch.float64, device=self.dev)

    def _host_vector(self, p, name):
        """what a Problem holds of the named device vector, in the device's layout, or None"""
        if name == "curv":
            return np.asarray(p.model.curv, dtype=np.float64)
        if name == "lin":                                            # f = sf (1/2 sum curv z^2 + lin . z); a model without one: zeros
            lin = getattr(p.model, "lin", None)
            return np.zeros(self.n) if lin is None else np.asarray(lin, dtype=np.float64)
        if name == "gL":
            return np.asarray(p.model.gL_gU()[0], dtype=np.float64)
        a = getattr(p, name, None)
        if a is None:
            return None
        a = np.asarray(a, dtype=np.float64)
        if name in ("rs", "dyE", "r2"):
            full = np.zeros(self.m)
            full[self.I if name == "rs" else self.E] = a
            return full
        return a

    def download(self, ps):
        """the device's state into the host Problems: the iterate, the scalars and every work vector"""
        rec = self.record()
        const = ("curv", "lin", "gL", "vL", "vU")
        get = {k: getattr(self, k).cpu().numpy() for k in self.NV + self.N + self.M if k not in const}
        for k, p in enumerate(ps):
            for name, a in get.items():
                length = self.nv if name in self.NV else self.n if name in self.N else self.m
                a = a[k, :length].copy()
                if name in ("rs", "dyE", "r2"):
                    a = a[self.I if name == "rs" else self.E]
                setattr(p, name, a)
            for name in self.lib.IPM_FIELDS:
                if name not in ("status", "iterations", "trials", "tol", "sf"):
                    setattr(p, name, float(rec[k, self.F[name]]))
            p.iterations, p.trials = int(rec[k, self.F["iterations"]]), int(rec[k, self.F["trials"]])
            code = int(rec[k, self.F["status"]])
            p.done, p.status = code != self.lib.IPM_RUNNING, None if code == self.lib.IPM_RUNNING else STATUSES[code]
            with np.errstate(invalid='ignore'):
                p.dL, p.dU = p.v - p.vL, p.vU - p.v

    def record(self):
        return self.rec.cpu().numpy()

    def z(self, of="v"):
        """the z part of ``v`` (or ``vt``) as a contiguous (K, n) tensor (a copy on the device)"""
        return getattr(self, of)[:, :self.n].contiguous()

    own_clock = None             # a dict while ``vector_clock()`` measures: every call is then waited for

    @staticmethod
    def launches(vec, name, args):
        """the kernel launches of one call (include/rato_saa.h: the grid form's count per entry point)"""
        if vec == 'workgroup':
            return 1
        if name == "rato_ipm_newton":
            return 1 if args[0] != 1 else 2 if args[-1] < 60 else 1  # RATO_IPM_PHASE_LADDER: rows and finish; finish alone at 60
        return {"rato_ipm_residuals": 3, "rato_ipm_step_setup": 3, "rato_ipm_trial": 1, "rato_ipm_accept": 4}[name]

    def _call(self, name, *args):
        """the entry point ``name`` ('rato_ipm_residuals', ...) in this state's form -> None; raises on a status"""
        lib, clock = self.lib, DeviceState.own_clock
        full, more = (name + "_grid_f64", (lib.ptr(self.work), self.work.numel())) if self.vec == 'grid' else (name + "_f64", ())
        with self.torch.cuda.device(self.dev):
            if clock is not None:
                self.torch.cuda.synchronize(self.dev)
                t0 = time.perf_counter()
            lib.check(getattr(lib.load(), full)(self.c_state, *args, *more, lib.current_stream()), full)
            if clock is not None:
                self.torch.cuda.synchronize(self.dev)
                clock["seconds"] += time.perf_counter() - t0
                clock["calls"] += 1
                clock["launches"] += self.launches(self.vec, name, args)

    def _ld(self, t):
        return 0 if t is None else t.shape[1]

    def residuals(self, g, JTy, last=False):
        self._call("rato_ipm_residuals", self.lib.ptr(g), self._ld(g), self.lib.ptr(JTy), self._ld(JTy), int(last))

    def newton(self, phase, a=None, b=None, info=None, flag=0):
        lib = self.lib
        self._call("rato_ipm_newton", lib.IPM_PHASES[phase], lib.ptr(a), self._ld(a), lib.ptr(b), self._ld(b), lib.ptr(info), int(flag))

    def step_setup(self, Hdv):
        self._call("rato_ipm_step_setup", self.lib.ptr(Hdv), self._ld(Hdv))

    def trial(self):
        self._call("rato_ipm_trial")

    def accept(self, gt):
        self._call("rato_ipm_accept", self.lib.ptr(gt), self._ld(gt))


@contextlib.contextmanager
def vector_clock():
    """For the profiles (tools/hopper_solve_bench.py --vec): inside, every ``DeviceState`` call is preceded and followed by a
    device-wide wait and timed -> the dict it fills: ``seconds`` in the driver's own vector kernels, their ``calls`` and
    ``launches``.  The waits make the solve slower; nothing else changes."""
    clock = dict(seconds=0.0, calls=0, launches=0)
    DeviceState.own_clock = clock
    try:
        yield clock
    finally:
        DeviceState.own_clock = None


def newton_steps_device(be, st, run, fact, refine=2):
    """``newton_steps`` on a DeviceState for the running problems (``run``: their numbers); every launch serves the whole batch
    and a problem that is not running is skipped inside it.  The delta_w ladder stays the host's decision on the
    factorization's info; ``fact`` counts a problem's factorizations.  -> the problems that are still running"""
    with be.timed_t("matvec"):
        st.newton("rhs", be.tmatvec_t(st.w))
    todo = list(run)
    for attempt in range(60):
        info = be.factor_t(st.d, st.diag)
        with be.timed_t("factor"):
            bad = info.cpu().numpy()
        for k in todo:
            fact[k] += 1
        todo = [k for k in todo if bad[k]]
        if not todo:
            break
        st.newton("ladder", info=info, flag=attempt + 1)              # the 60th failure ends the problem: 'line_search'
    run = [k for k in run if k not in todo]
    if not run:
        return run
    be.solve_t(st.dz)
    for it in range(refine + 1):
        with be.timed_t("matvec"):
            Jdz = be.matvec_t(st.dz)
            if it == refine:
                break
            st.newton("q", Jdz, flag=it == 0)
            JTq, Wdz = be.tmatvec_t(st.q), be.hess_apply_t(st.dz)
            st.newton("r", Wdz, JTq)
        be.solve_t(st.ez)
        with be.timed_t("matvec"):
            st.newton("update", be.matvec_t(st.ez))
    st.newton("finish", Jdz)
    return run


def solve_group_device(models, Z0s, tol, max_iter, be, verbose, driver='device'):
    """``solve_group`` with the iterate on the device: the Problems are made on the host once (bound relaxation, the push into
    the interior, sf), uploaded as a ``DeviceState``, and every lockstep iteration is a chain of K-problem launches; the host
    reads back the scalar record after the residual phase and after each line-search trial, and the info of each
    factorization.  A problem that has ended stays in the launches and is skipped inside them.  ``be`` serves device tensors:
    eval_full_t / eval_g_t / matvec_t / tmatvec_t / hess_apply_t / factor_t / solve_t.  -> [(Z, info)] as ``solve_group``'s,
    with info["driver"] = ``driver``: 'device', or 'device_grid' for the vector kernels' grid form (``DeviceState(vec='grid')``),
    which changes no bit of the result."""
    from . import _lib
    K = len(models)
    g0 = be.eval_g(list(range(K)), [np.asarray(Z, dtype=np.float64) for Z in Z0s])
    ps = [Problem(m, Z, g, tol) for m, Z, g in zip(models, Z0s, g0)]
    st = DeviceState(ps, be.dev, vec=VEC_OF_DRIVER[driver])
    fact = [0] * K
    STATUS, SEARCHING = st.F["status"], st.F["searching"]
    for it in range(max_iter + 1):
        with be.timed_t("callbacks"):
            g = be.eval_full_t(st.z(), st.y)
        with be.timed_t("matvec"):
            JTy = be.tmatvec_t(st.y)
        st.residuals(g, JTy, it == max_iter)
        with be.timed_t("readback"):
            rec = st.record()
        run = [k for k in range(K) if rec[k, STATUS] == _lib.IPM_RUNNING]
        if run:
            run = newton_steps_device(be, st, run, fact)
        if run:
            with be.timed_t("matvec"):
                st.step_setup(be.hess_apply_t(st.dv))
            while True:
                st.trial()
                with be.timed_t("callbacks"):
                    gt = be.eval_g_t(st.z("vt"))
                st.accept(gt)
                with be.timed_t("readback"):
                    rec = st.record()
                if not np.any((rec[:, STATUS] == _lib.IPM_RUNNING) & (rec[:, SEARCHING] == 1.0)):
                    break
        if verbose:
            _print_iteration(it, rec[:, [st.F[f] for f in ("mu", "E0", "prim", "dual", "alpha", "dw")]])
        if not np.any(rec[:, STATUS] == _lib.IPM_RUNNING):
            break
    st.download(ps)
    for p, nf in zip(ps, fact):
        p.factorizations = nf                                        # the device's record does not count them: the host did
    return _results(ps, be, driver=driver)


def solve_groups(groups, setup, Z0s, tol, max_iter, verbose, clocks, driver='host'):
    """what a ``solve_batch`` ends with: the groups (lists of problem numbers) one after the other, each by ``solve_group``
    (``driver='device'`` / ``'device_grid'``: ``solve_group_device``) on the (models, backend) ``setup(members)`` makes -> [(Z, info)] in the
    problems' order.  ``clocks`` (a dict, or None) receives the sums of the backends' clocks and the wall clock."""
    out = [None] * sum(len(members) for members in groups)
    t0 = time.perf_counter()
    run = functools.partial(solve_group_device, driver=driver) if on_device(driver) else solve_group
    for members in groups:
        models, be = setup(members)
        for i, r in zip(members, run(models, [Z0s[i] for i in members], tol, max_iter, be, verbose)):
            out[i] = r
        if clocks is not None:
            for k, v in be.clock.items():
                clocks[k] = clocks.get(k, 0.0) + v
    if clocks is not None:
        clocks["wall"] = clocks.get("wall", 0.0) + time.perf_counter() - t0
    return out
