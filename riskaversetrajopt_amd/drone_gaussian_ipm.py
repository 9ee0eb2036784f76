"""Batched interior-point solve of the drone Gaussian baseline's NLP (drone/drone_gaussian.py:400-534: what the script hands
to IPOPT), by the method of ``ipm`` (``Problem``, ``newton_steps``, ``solve_group``: DESIGN §7.ad, §7.ae).

Formulation.  The script's g is (the n_nl non-linear rows, z itself, the allocation sum).  The nvar identity rows are bounds on
z, intersected with x_L / x_U = -+1000:  u in [u_min, u_max], allocations in [1e-6, alpha] -- the same feasible set, and every
trial point keeps its allocations strictly inside (0, alpha), where ppf(1 - a) exists.  That leaves m = n_nl + 1 rows: 6
equalities, n_nl - 6 rows bounded above by 0, the sum row in [0, alpha].  f = sum 2 dt R_ii u^2 has a diagonal Hessian, which
the host folds into the diagonal term of the condensed matrix and adds to W x.

The constraint matrix is dense: J = [jac_nl; the sum row] (m x nvar).  Two backends do the step:
  'device'  one ``linearize_device`` and one ``hessian_device`` call per iteration for the active problems, then
            rato_dense_normal_matrix_f64 / rato_chol_factor_batch_f64 / rato_chol_solve_batch_f64 / rato_dense_matvec_f64 /
            rato_dense_tmatvec_f64 / rato_tril_symv_f64 (csrc/drone_gaussian_ipm.hip, csrc/chol.hip) on jac_nl and the
            packed Hessian where they lie.  Up go the points, the multipliers (K, n_nl), d, the diagonals and the vectors;
            down come g_nl, the matvec results, the factorization's info and the solutions.  jac_nl, the packed Hessian and
            Kc / L never leave the device.
  'numpy'   the whole step on the host on injected (or the model's) callbacks dict(linearize, hessian).
alpha enters only the host-side bounds, so the problems of one S form a group whatever their alpha.  A backend here is its
callbacks, its products and its normal matrix (``normal_matrix_host``; ``normal_matrix`` / ``normal_matrix_t`` on the device):
factor and solve, on lists and on tensors, are ``ipm.Backend``'s / ``ipm.DeviceBase``'s.
"""
import numpy as np

from . import drone_params as P
from . import ipm as _ipm

STATUSES = _ipm.STATUSES
X_BOUND = 1000.0                                                 # the script's x_L / x_U (:446-447)


class Nlp:
    """what ``ipm.Problem`` reads of a model: num_vars, gL_gU() on the m = n_nl + 1 rows, x_bounds(), f, grad_f"""

    def __init__(self, model):
        from . import drone_gaussian as dg
        self.model, self.S, self.alpha = model, model.S, float(model.alpha)
        self.num_vars, self.n_nl, self.D = model.nvar, model.n_nl, dg.n_u * model.S
        self.curv = np.zeros(model.nvar)
        self.curv[:self.D] = np.tile(4 * model.dt * np.diag(P.R), model.S)          # f = 1/2 sum curv z^2 = sum 2 dt R_ii u^2
        self.alpha_min = dg.ALPHA_MIN

    def f(self, Z):
        Z = np.asarray(Z, dtype=np.float64)
        return 0.5 * float(np.sum(self.curv * Z * Z))

    def grad_f(self, Z):
        return self.curv * np.asarray(Z, dtype=np.float64)

    def gL_gU(self):
        gL = np.concatenate([np.zeros(6), np.full(self.n_nl - 6, -1e15), [0.0]])
        gU = np.concatenate([np.zeros(self.n_nl), [self.alpha]])
        return gL, gU

    def x_bounds(self):
        n, D = self.num_vars, self.D
        lo = np.concatenate([np.full(D, float(self.model.u_min)), np.full(n - D, self.alpha_min)])
        hi = np.concatenate([np.full(D, float(self.model.u_max)), np.full(n - D, self.alpha)])
        return np.maximum(lo, -X_BOUND), np.minimum(hi, X_BOUND)

    def g(self, Z, g_nl):
        return np.concatenate([g_nl, [np.sum(np.asarray(Z)[self.D:])]])

    def sum_row(self):
        return np.concatenate([np.zeros(self.D), np.ones(self.num_vars - self.D)])


def unpack_tril(tril, n):
    r, c = np.tril_indices(n)
    H = np.zeros((n, n))
    H[r, c] = tril
    H[c, r] = tril
    return H


def normal_matrix_host(J, d, hess_tril=None, diag=None):
    """the NumPy twin of rato_dense_normal_matrix_f64: unpack(hess_tril) + diag(diag) + J' diag(d) J, J (m, n) -> (n, n)"""
    J = np.asarray(J, dtype=np.float64)
    Kc = (J.T * np.asarray(d, dtype=np.float64)) @ J             # the factorization reads the lower triangle alone
    if hess_tril is not None:
        Kc = Kc + unpack_tril(hess_tril, J.shape[1])
    if diag is not None:
        Kc = Kc + np.diag(np.asarray(diag, dtype=np.float64))
    return Kc


# ---- backends ----------------------------------------------------------------------------------------------------------------
class NumpyBackend(_ipm.Backend):
    """the whole step on the host.  ``callbacks[i]`` serves nlps[i]: dict(linearize(Z) -> (g_nl, jac_nl), hessian(Z, lam) -> tril)"""
    name = "numpy"

    def __init__(self, nlps, callbacks=None):
        super().__init__("matvec")
        self.nlps = nlps
        self.cb = [p.model.device_callbacks() for p in nlps] if callbacks is None else list(callbacks)
        self.st = None
        self.J, self.hess, self.sf = {}, {}, {}

    def eval_full(self, idx, Zs, lams, sfs):
        with self.timed("callbacks"):
            out = []
            for i, Z, lam, sf in zip(idx, Zs, lams, sfs):
                nlp = self.nlps[i]
                g_nl, jac_nl = self.cb[i]["linearize"](np.asarray(Z, dtype=np.float64))
                self.J[i] = np.vstack([np.asarray(jac_nl, dtype=np.float64), nlp.sum_row()[None, :]])
                self.hess[i] = np.asarray(self.cb[i]["hessian"](np.asarray(Z, dtype=np.float64),
                                                                np.asarray(lam, dtype=np.float64)[:nlp.n_nl]), dtype=np.float64)
                self.sf[i] = float(sf)
                out.append(nlp.g(Z, np.asarray(g_nl, dtype=np.float64)))
        return out

    def eval_g(self, idx, Zs):
        with self.timed("callbacks"):
            out = [self.nlps[i].g(Z, np.asarray(self.cb[i]["linearize"](np.asarray(Z, dtype=np.float64))[0], dtype=np.float64))
                   for i, Z in zip(idx, Zs)]
        return out

    def set_values(self, J, hess, sfs):
        """install dense J (K, m, n), packed Hessians (K, n (n + 1) / 2) and objective scales as the current evaluation of
        problems 0 .. K-1 (what eval_full leaves)"""
        for i, (j, h, sf) in enumerate(zip(J, hess, sfs)):
            self.J[i], self.hess[i], self.sf[i] = np.asarray(j, dtype=np.float64), np.asarray(h, dtype=np.float64), float(sf)

    def hess_apply(self, idx, X):
        return [unpack_tril(self.hess[i], x.size) @ x + self.sf[i] * self.nlps[i].curv * x for i, x in zip(idx, X)]

    def matvec(self, idx, X):
        with self.timed("matvec"):
            out = [self.J[i] @ x for i, x in zip(idx, X)]
        return out

    def tmatvec(self, idx, W):
        with self.timed("matvec"):
            out = [self.J[i].T @ w for i, w in zip(idx, W)]
        return out

    def normal_matrix_host(self, i, d, diag):
        return normal_matrix_host(self.J[i], d, self.hess[i], diag + self.sf[i] * self.nlps[i].curv)


def _check(t, name, dims=None):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or \
            (dims is not None and t.dim() != dims):
        raise ValueError(f"{name} must be a contiguous device float64 tensor" + (f" of {dims} dimensions" if dims else ""))
    return t


def dense_tile_width():
    from . import _lib
    return int(_lib.load().rato_dense_tile_width())


def _blocks(J0, J1, n):
    """the two row blocks as the ABI takes them: J0 (K, m0, ld0), J1 None | (m1, ld1) shared | (K, m1, ld1) per problem"""
    from . import _lib
    _check(J0, "J0", 3)
    K, m0, ld0 = J0.shape
    if J1 is None:
        return K, (_lib.ptr(J0), m0, ld0, None, 0, n, 0), m0
    _check(J1, "J1")
    if J1.dim() == 2:
        m1, ld1, stride1 = J1.shape[0], J1.shape[1], 0
    elif J1.dim() == 3 and J1.shape[0] == K:
        m1, ld1, stride1 = J1.shape[1], J1.shape[2], J1.shape[1] * J1.shape[2]
    else:
        raise ValueError("J1 must be (m1, ld1) or (K, m1, ld1)")
    return K, (_lib.ptr(J0), m0, ld0, _lib.ptr(J1) if m1 else None, m1, ld1, stride1), m0 + m1


def dense_normal_matrix(n, J0, J1, d, hess_tril=None, diag=None, out=None):
    """rato_dense_normal_matrix_f64 on device fp64 tensors: J0 (K, m0, ld0 >= n), J1 as ``_blocks`` takes it, d (K, ldd >= m),
    hess_tril (K, n (n + 1) / 2) or None, diag (K, n) or None -> Kc (K, n, lda) (``out``, or a fresh (K, n, n) tensor whose strict
    upper triangle is not written)"""
    import torch
    from . import _lib
    K, blk, m = _blocks(J0, J1, n)
    _check(d, "d", 2)
    if hess_tril is not None and tuple(_check(hess_tril, "hess_tril", 2).shape) != (K, n * (n + 1) // 2):
        raise ValueError("hess_tril must be (K, n (n + 1) / 2)")
    if diag is not None and tuple(_check(diag, "diag", 2).shape) != (K, n):
        raise ValueError("diag must be (K, n)")
    Kc = torch.empty((K, n, n), dtype=torch.float64, device=J0.device) if out is None else _check(out, "out", 3)
    if d.shape[0] != K or tuple(Kc.shape[:2]) != (K, n):
        raise ValueError("d must be (K, ldd) and out (K, n, lda)")
    with torch.cuda.device(J0.device):
        _lib.check(_lib.load().rato_dense_normal_matrix_f64(K, n, Kc.shape[2], *blk, _lib.ptr(d), d.shape[1], _lib.ptr(hess_tril),
                                                            _lib.ptr(diag), _lib.ptr(Kc), _lib.current_stream()),
                   "rato_dense_normal_matrix_f64")
    return Kc


def _mv(name, n, J0, J1, x, n_out_of):
    import torch
    from . import _lib
    K, blk, m = _blocks(J0, J1, n)
    _check(x, "x", 2)
    if x.shape[0] != K:
        raise ValueError("the vector must be (K, ld)")
    out = torch.empty((K, n_out_of(m)), dtype=torch.float64, device=J0.device)
    with torch.cuda.device(J0.device):
        _lib.check(getattr(_lib.load(), name)(K, n, *blk, _lib.ptr(x), x.shape[1], _lib.ptr(out), out.shape[1],
                                              _lib.current_stream()), name)
    return out


def dense_matvec(n, J0, J1, x):
    """rato_dense_matvec_f64: x (K, ldx >= n) -> J x (K, m)"""
    return _mv("rato_dense_matvec_f64", n, J0, J1, x, lambda m: m)


def dense_tmatvec(n, J0, J1, w):
    """rato_dense_tmatvec_f64: w (K, ldw >= m) -> J' w (K, n)"""
    return _mv("rato_dense_tmatvec_f64", n, J0, J1, w, lambda m: n)


def tril_symv(n, hess_tril, x):
    """rato_tril_symv_f64: hess_tril (K, n (n + 1) / 2), x (K, ldx >= n) -> H x (K, n)"""
    import torch
    from . import _lib
    _check(hess_tril, "hess_tril", 2), _check(x, "x", 2)
    K = x.shape[0]
    if tuple(hess_tril.shape) != (K, n * (n + 1) // 2):
        raise ValueError("hess_tril must be (K, n (n + 1) / 2)")
    out = torch.empty((K, n), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().rato_tril_symv_f64(K, n, _lib.ptr(hess_tril), _lib.ptr(x), x.shape[1], _lib.ptr(out), n,
                                                  _lib.current_stream()), "rato_tril_symv_f64")
    return out


class DeviceBackend(_ipm.DeviceBase):
    """the step on the MI355X for the problems of one group (same S; alpha may differ).  Every call serves the listed problems
    in ONE launch each; nothing a kernel computes for a problem depends on the others."""
    name = "device"

    def __init__(self, nlps, chol='workgroup'):
        self.nlps = nlps
        self.m0 = nlps[0].model
        self.m0._handle()
        super().__init__(self.m0.device, len(nlps), "matvec", chol=chol)
        self.n, self.n_nl = nlps[0].num_vars, nlps[0].n_nl
        self.st = None
        self.sum_row = self.torch.as_tensor(nlps[0].sum_row()[None, :].copy(), device=self.dev)
        self.sf = {}
        self.jac = self.hess = None

    def _g(self, idx, Zs, g_nl):
        g_nl = g_nl.cpu().numpy()
        return [self.nlps[i].g(Z, g_nl[k]) for k, (i, Z) in enumerate(zip(idx, Zs))]

    def eval_full(self, idx, Zs, lams, sfs):
        with self.timed("callbacks"):
            with self.torch.cuda.device(self.dev):
                Zd = self._up(Zs)
                r = self.m0.linearize_device(Zd)
                self.hess = self.m0.hessian_device(Zd, self._up([np.asarray(l)[:self.n_nl] for l in lams]))
            self.jac = r["jac_nl"]
            self.slot = {i: k for k, i in enumerate(idx)}
            for i, sf in zip(idx, sfs):
                self.sf[i] = float(sf)
            out = self._g(idx, Zs, r["g_nl"])
        return out

    def eval_g(self, idx, Zs):
        with self.timed("callbacks"):
            with self.torch.cuda.device(self.dev):
                out = self._g(idx, Zs, self.m0.linearize_device(self._up(Zs))["g_nl"])
        return out

    def set_values(self, J, hess, sfs):
        """install dense J (K, m, n) (its last row is the sum row), packed Hessians (K, n (n + 1) / 2) and objective scales as
        the current evaluation of problems 0 .. K-1 (what eval_full leaves)"""
        J = np.asarray(J, dtype=np.float64)
        self.jac, self.hess = self._up(list(J[:, :self.n_nl])), self._up(list(hess))
        self.slot = {i: i for i in range(J.shape[0])}
        self.sf = {i: float(sf) for i, sf in enumerate(sfs)}

    def _sel(self, idx):
        return self._rows(idx, self.jac, self.hess)

    def hess_apply(self, idx, X):
        with self.timed("matvec"):
            out = tril_symv(self.n, self._sel(idx)[1], self._up(X)).cpu().numpy()
        return [o + self.sf[i] * self.nlps[i].curv * x for i, o, x in zip(idx, out, X)]

    def matvec(self, idx, X):
        with self.timed("matvec"):
            out = list(dense_matvec(self.n, self._sel(idx)[0], self.sum_row, self._up(X)).cpu().numpy())
        return out

    def tmatvec(self, idx, W):
        with self.timed("matvec"):
            out = list(dense_tmatvec(self.n, self._sel(idx)[0], self.sum_row, self._up(W)).cpu().numpy())
        return out

    def normal_matrix(self, idx, D, diags, out=None):
        """-> Kc (K, n, lda) device tensor, the objective's curvature folded into the diagonal"""
        jac, hess = self._sel(idx)
        dg = self._up([g + self.sf[i] * self.nlps[i].curv for i, g in zip(idx, diags)])
        return dense_normal_matrix(self.n, jac, self.sum_row, self._up(D), hess, dg, out=out)

    # ---- the same on device tensors, for ``ipm.solve_group_device``: every call serves the whole group, takes and returns
    # (K, ld) tensors and waits for nothing.  ``factor_t`` and ``solve_t`` are DeviceBase's, as are ``factor`` and ``solve``.
    def eval_full_t(self, Z, Y):
        """Z (K, n) and the multipliers Y (K, ld >= m) -> g (K, m); leaves jac_nl and the packed Hessian of Y . g for the calls below"""
        with self.torch.cuda.device(self.dev):
            r = self.m0.linearize_device(Z)
            self.hess = self.m0.hessian_device(Z, Y[:, :self.n_nl].contiguous())
        self.jac = r["jac_nl"]
        self.slot = {i: i for i in range(Z.shape[0])}
        return _ipm.g_rows(self.n, r["g_nl"], self.sum_row, Z)

    def eval_g_t(self, Z):
        with self.torch.cuda.device(self.dev):
            g_nl = self.m0.linearize_device(Z)["g_nl"]
        return _ipm.g_rows(self.n, g_nl, self.sum_row, Z)

    def matvec_t(self, X):
        return dense_matvec(self.n, self.jac, self.sum_row, X)

    def tmatvec_t(self, W):
        return dense_tmatvec(self.n, self.jac, self.sum_row, W)

    def hess_apply_t(self, X):
        """W x of the constraints' part alone: the objective's sf curv x is added where the result is used (csrc/ipm_driver.hip)"""
        return tril_symv(self.n, self.hess, X)

    def normal_matrix_t(self, d, diag, out=None):
        """d (K, ld >= m), diag (K, n) with the objective's curvature already in it -> Kc (K, n, lda)"""
        return dense_normal_matrix(self.n, self.jac, self.sum_row, d, self.hess, diag, out=out)


# ---- the solve -------------------------------------------------------------------------------------------------------------
def lagrange(nlp, info):
    """the multipliers in the script's row order (ncon): the non-linear rows' y, zu_j - zl_j for the identity row j, the sum
    row's y.  With J_script = ``ipopt_callbacks()``'s Jacobian: sf grad f + J_script' lagrange is the dual residual."""
    n, n_nl = nlp.num_vars, nlp.n_nl
    return np.concatenate([info["y"][:n_nl], info["zu"][:n] - info["zl"][:n], info["y"][n_nl:]])


def make_backend(nlps, backend, callbacks=None, chol='workgroup'):
    return DeviceBackend(nlps, chol=chol) if backend == 'device' else NumpyBackend(nlps, callbacks)


def solve_batch(models, Z0s=None, tol=1e-8, max_iter=3000, backend='device', callbacks=None, verbose=False, clocks=None,
                results_dir='results', driver='host', chol='workgroup'):
    """Solve the models' NLPs in lockstep -> list of (Z, info), in the models' order.  Models of one S form a group that moves
    through the K-problem kernels together (alpha may differ inside it: it enters only the host-side bounds), the groups one
    after the other.  A problem that has ended leaves the launches, a failed factorization is redone for the failed problems
    alone, and a problem's Z is bitwise what its own K = 1 run returns.
      Z0s        starting points (default: ``model.initial_guess(results_dir)``, the script's)
      backend    'device' (csrc/drone_gaussian_ipm.hip) or 'numpy' (the step on the host)
      callbacks  backend='numpy' only: one dict(linearize, hessian) per model, as ``run_drone_gaussian(callbacks=...)`` takes
      clocks     a dict that receives the seconds spent in callbacks / normal / factor / solve / matvec, the wall clock and
                 host = the rest (the driver's vector algebra and line-search bookkeeping)
      driver     'host' (``ipm.solve_group``: the iterate and the vector algebra on the host) or 'device'
                 (``ipm.solve_group_device``, backend='device' only: the iterate stays on the device, csrc/ipm_driver.hip, and
                 the clocks hold the time to launch; info["driver"] = 'device'), or 'device_grid': 'device' with the driver's
                 own vector kernels spread over the rows (csrc/ipm_driver_grid.hip, DESIGN §7.al: the same bits)
      chol       'workgroup' (csrc/chol.hip) or 'grid' (csrc/chol_grid.hip: the same bits from launches spread over the device);
                 backend='numpy' ignores it
    info: status ('converged' | 'max_iter' | 'line_search'), iterations, factorizations, E0, primal_infeasibility,
    dual_infeasibility, f, mu, sf (the objective scale), the final multipliers y (m = n_nl + 1), zl, zu (nvar + the slacks), the
    slacks s, and lagrange (ncon) in the script's row order."""
    if backend not in ('device', 'numpy'):
        raise ValueError(f"backend must be 'device' or 'numpy', got {backend!r}")
    _ipm.check_driver(driver, backend)
    _ipm.check_chol(chol)
    if callbacks is not None and backend != 'numpy':
        raise ValueError("callbacks are the numpy backend's")
    models = list(models)
    if callbacks is not None and len(callbacks) != len(models):
        raise ValueError("callbacks must hold one dict(linearize, hessian) per model")
    Z0s = [m.initial_guess(results_dir) for m in models] if Z0s is None else [np.asarray(Z, dtype=np.float64) for Z in Z0s]
    if len(Z0s) != len(models) or any(Z.shape != (m.nvar,) for Z, m in zip(Z0s, models)):
        raise ValueError("Z0s must hold one (nvar,) vector per model")
    groups = {}
    for i, m in enumerate(models):
        groups.setdefault((m.S, str(m.device)) if backend == 'device' else (m.S,), []).append(i)
    nlps = {}

    def setup(members):
        group = [Nlp(models[i]) for i in members]
        nlps.update(zip(members, group))
        return group, make_backend(group, backend, None if callbacks is None else [callbacks[i] for i in members],
                                   chol=chol)

    spent = None if clocks is None else {}
    out = _ipm.solve_groups(list(groups.values()), setup, Z0s, tol, max_iter, verbose, spent, driver=driver)
    for i, (Z, info) in enumerate(out):
        info["lagrange"] = lagrange(nlps[i], info)
    if clocks is not None:
        spent["host"] = spent["wall"] - sum(v for k, v in spent.items() if k != "wall")
        for k, v in spent.items():
            clocks[k] = clocks.get(k, 0.0) + v
    return out
