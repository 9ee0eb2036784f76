"""Shared pieces of the hopper interior-point tests: the solver's callbacks served by the fp64 restatement
(tests/_hopper_nlp.py + oracle/hopper.py), independent of the package's kernels, and the check of a returned solution that
uses nothing of the solver's own bookkeeping."""
import numpy as np

from oracle import hopper as oh
from riskaversetrajopt_amd import hopper
import _hopper_nlp as R

S_SMALL, M_SMALL = 6, 4
TOL = 1e-3


def fields(M, seed=1):
    return oh.sample_friction_fields(np.random.RandomState(seed), M)


class RestatementCallbacks:
    """g, the Jacobian's values on ``nlp_layout()``'s fixed pattern and the Hessian's step blocks from the restatement"""

    def __init__(self, model, flds):
        self.m, self.fields = model, flds
        lay = model.nlp_layout()
        self.rows = np.asarray(lay["jac_indices"], dtype=np.int64)
        self.cols = np.repeat(np.arange(lay["nvar"]), np.diff(lay["jac_indptr"]))
        assert (model.time_jump, model.time_land) == oh.phase_times(model.S)

    def _args(self):
        return self.m.S, self.m.M, self.m.method, self.m.alpha, self.fields

    def g(self, Z):
        return R.g_full(np.asarray(Z), *self._args())

    def jac_dense(self, Z):
        return R.jac_dense(np.asarray(Z), *self._args())

    def jac_values(self, Z):
        return self.jac_dense(Z)[self.rows, self.cols]

    def hess_blocks(self, Z, lam, obj_factor):
        return R.tril78(R.hess_blocks_full(np.asarray(Z), np.asarray(lam), *self._args(), obj_factor=obj_factor))


def host_model(method, alpha, S=S_SMALL, M=M_SMALL):
    return hopper.Model.host_only(M, method=method, alpha=alpha, S=S)


def check_solution(model, flds, Z, info, tol=TOL):
    """On the restatement: g within [gL - tol, gU + tol], the bounds hold, and E_0 recomputed from the returned multipliers is
    <= tol.  -> the recomputed E_0"""
    S, M = model.S, model.M
    tj, tl = oh.phase_times(S)
    g = R.g_full(Z, S, M, model.method, model.alpha, flds)
    J = R.jac_dense(Z, S, M, model.method, model.alpha, flds)
    gL, gU = R.bounds_g(S, M, tj, tl, model.method)
    xL, xU = R.bounds_x(S, M)
    assert np.all(g >= gL - tol) and np.all(g <= gU + tol), (np.max(gL - g), np.max(g - gU))
    assert np.all(Z >= xL - 1e-8 * np.maximum(1, np.abs(xL))) and np.all(Z <= xU + 1e-8 * np.maximum(1, np.abs(xU)))
    E = gL == gU
    I = ~E
    y, zl, zu, s, sf = info["y"], info["zl"], info["zu"], info["s"], info["sf"]
    n = Z.size
    relax = lambda b, sign: b + sign * 1e-8 * np.maximum(1.0, np.abs(b))
    vL, vU = relax(np.concatenate([xL, gL[I]]), -1), relax(np.concatenate([xU, gU[I]]), +1)
    hasL, hasU = np.abs(vL) < 1e14, np.abs(vU) < 1e14
    v = np.concatenate([Z, s])
    assert np.all(zl >= 0) and np.all(zu >= 0) and not np.any(zl[~hasL]) and not np.any(zu[~hasU])
    assert np.all(v[hasL] > vL[hasL]) and np.all(v[hasU] < vU[hasU])
    dual_z = sf * R.grad_objective(Z, S) + J.T @ y - zl[:n] + zu[:n]
    dual_s = -y[I] - zl[n:] + zu[n:]
    c = np.concatenate([g[E] - gL[E], g[I] - s])
    comp = max(np.max(zl[hasL] * (v - vL)[hasL]), np.max(zu[hasU] * (vU - v)[hasU]))
    E0 = max(np.max(np.abs(dual_z)), np.max(np.abs(dual_s)), np.max(np.abs(c)), comp)
    assert E0 <= tol, (E0, np.max(np.abs(dual_z)), np.max(np.abs(dual_s)), np.max(np.abs(c)), comp)
    return E0


def newton_residual(be, model, flds, S, M, seed=0):
    """One Newton step of backend ``be`` (holding ``model`` as its problem 0) at a designed interior iterate: the perturbed
    point ``_hopper_nlp.problem(S, M, seed)`` pushed inside the bounds, seeded multipliers of mixed sign, mu = 0.1.
    -> (relative residual in the uncondensed regularised KKT system built from the restatement's dense J and W, delta_w)"""
    from riskaversetrajopt_amd import ipm
    Z0 = R.problem(S, M, seed)
    p = ipm.Problem(model, Z0, be.eval_g([0], [Z0])[0], TOL)
    rng = np.random.RandomState(400 + S)
    p.y = rng.uniform(-1, 1, p.m)
    p.zl, p.zu = p.zl * rng.uniform(0.5, 2.0, p.zl.size), p.zu * rng.uniform(0.5, 2.0, p.zu.size)
    g, = be.eval_full([0], [p.z.copy()], [p.y], [p.sf])
    p.residuals(g, be.tmatvec([0], [p.y])[0])
    p.prepare_step()
    assert ipm.newton_steps(be, [0], [p]) == [True]
    J = R.jac_dense(p.z, S, M, model.method, model.alpha, flds)
    W = R.dense_from_blocks(R.hess_blocks_full(p.z, p.y, S, M, model.method, model.alpha, flds, obj_factor=p.sf), S, p.n)
    return ipm.kkt_residual(p, J, W), p.dw


def warm_start(model, Zbase):
    """the script's SAA start (:465-479): the baseline's states and controls, ys = slack = t_risk = 0"""
    Z0 = np.zeros(model.num_vars)
    k = hopper.n_x * (model.S + 1) + hopper.n_u * model.S
    Z0[:k] = Zbase[:k]
    return Z0


# ---- the product map's cases and references (CPU and GPU tests) -------------------------------------------------------------
U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def map_cases():
    cases = []
    for S in (1, 2, 6):
        for M in (1, 4):
            for method in ('baseline', 'saa'):
                cases.append((S, M, method, None))
    for S, ph in ((2, (1, 1)), (6, (3, 3)), (6, (0, 0)), (2, (0, 2)), (6, (0, 6))):      # empty flight; empty contact
        for method in ('baseline', 'saa'):
            cases.append((S, 4, method, ph))
    return cases


def designed_values(st, seed):
    """values on the fixed pattern with exact zeros among them, and weights from 1e-8 to 1e8"""
    rng = np.random.RandomState(seed)
    vals = rng.uniform(-2, 2, st["nnz"]) * 10.0 ** rng.randint(-3, 4, st["nnz"])
    vals[rng.rand(st["nnz"]) < 0.15] = 0.0
    d = 10.0 ** rng.uniform(-8, 8, st["ncon"])
    return vals, d


def dense_reference(st, vals, d):
    """J' D J and sum |terms| from dense extended-precision NumPy, and the number of triples per entry"""
    J = np.zeros((st["ncon"], st["n"]), dtype=np.longdouble)
    J[st["rows"], st["cols"]] = vals
    D = d.astype(np.longdouble)[:, None]
    T = np.zeros((st["n"], st["n"]), dtype=np.int64)
    np.add.at(T.reshape(-1), st["ent_keys"], np.diff(st["ptr"]))
    return J.T @ (D * J), np.abs(J).T @ (D * np.abs(J)), T
