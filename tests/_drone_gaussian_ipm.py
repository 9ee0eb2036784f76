"""Shared by the drone Gaussian interior-point tests: the independent check of a returned point on the fp64 restatement
(tests/_drone_gaussian.py), the designed buffers of the dense kernels and their extended-precision references."""
import functools

import numpy as np

import _drone_gaussian as R
from riskaversetrajopt_amd import drone_gaussian as dg
from riskaversetrajopt_amd import drone_params as P

LD = np.longdouble
U = 2.0 ** -53
TOL = 1e-8
CASES = {3: (0.05, 0.3), 5: (0.1, 0.3)}                          # S -> the alphas of one batch


def gamma(k):
    return k * U / (1.0 - k * U)


def curvature(S):
    c = np.zeros(R.sizes(S)[0])
    c[:3 * S] = np.tile(4 * (P.T / S) * np.diag(P.R), S)
    return c


def bounds(S, alpha):
    """-> (zL, zU) of z, (gL, gU) of the m = n_nl + 1 rows (non-linear rows, then the allocation sum), stated apart from the solver"""
    nvar, n_nl = R.sizes(S)
    D = 3 * S
    zL = np.concatenate([np.full(D, -float(P.u_max)), np.full(nvar - D, 1e-6)])
    zU = np.concatenate([np.full(D, float(P.u_max)), np.full(nvar - D, alpha)])
    gL = np.concatenate([np.zeros(6), np.full(n_nl - 6, -np.inf), [0.0]])
    gU = np.concatenate([np.zeros(n_nl), [alpha]])
    return (zL, zU), (gL, gU)


def check_solution(S, alpha, Z, info, tol=TOL):
    """Re-evaluates the returned point with ``_drone_gaussian.evaluate`` and without the solver's bookkeeping: E_0 from
    (Z, s, y, zl, zu) <= tol, |g_eq| <= tol, the inequality rows and the sum row hold to tol, z inside the relaxed bounds.
    -> dict(E0, dual (the z part of the dual residual, a vector))"""
    nvar, n_nl = R.sizes(S)
    D = 3 * S
    (zL, zU), (gL, gU) = bounds(S, alpha)
    y, zl, zu, s, sf = info["y"], info["zl"], info["zu"], info["s"], info["sf"]
    assert y.shape == (n_nl + 1,) and s.shape == (n_nl + 1 - 6,) and zl.shape == zu.shape == (nvar + s.size,)
    ev = R.evaluate(Z, S)
    g = np.concatenate([ev["g_nl"], [np.sum(Z[D:])]])
    J = np.vstack([ev["jac_nl"], np.concatenate([np.zeros(D), np.ones(nvar - D)])[None, :]])
    assert np.max(np.abs(g[:6])) <= tol, np.max(np.abs(g[:6]))
    assert np.all(g[6:] <= gU[6:] + tol) and g[-1] >= gL[-1] - tol, (np.max(g[6:] - gU[6:]), g[-1])
    relax = lambda b, sign: b + sign * 1e-8 * np.maximum(1.0, np.abs(b))
    assert np.all(Z >= relax(zL, -1)) and np.all(Z <= relax(zU, +1))
    E = gL == gU
    I = ~E
    with np.errstate(invalid='ignore'):
        vL, vU = relax(np.concatenate([zL, gL[I]]), -1), relax(np.concatenate([zU, gU[I]]), +1)
    hasL, hasU = np.isfinite(vL), np.isfinite(vU)
    v = np.concatenate([Z, s])
    assert np.all(zl >= 0) and np.all(zu >= 0) and not np.any(zl[~hasL]) and not np.any(zu[~hasU])
    assert np.all(v[hasL] > vL[hasL]) and np.all(v[hasU] < vU[hasU])
    dual_z = sf * curvature(S) * Z + J.T @ y - zl[:nvar] + zu[:nvar]
    dual_s = -y[I] - zl[nvar:] + zu[nvar:]
    c = np.concatenate([g[E] - gL[E], g[I] - s])
    comp = max(np.max(zl[hasL] * (v - vL)[hasL]), np.max(zu[hasU] * (vU - v)[hasU]))
    E0 = max(np.max(np.abs(dual_z)), np.max(np.abs(dual_s)), np.max(np.abs(c)), comp)
    assert E0 <= tol, (E0, np.max(np.abs(dual_z)), np.max(np.abs(dual_s)), np.max(np.abs(c)), comp)
    return dict(E0=E0, dual=dual_z)


def models(S, alphas):
    return [dg.Model(S, alpha=a) for a in alphas]


def starts(S, alphas):
    return [R.start_point(S, a) for a in alphas]


def host_callbacks(S, alphas):
    return [R.callbacks(S, a) for a in alphas]


@functools.lru_cache(maxsize=None)
def numpy_solutions(S, max_iter=300):
    """the NumPy backend on the restatement's callbacks, the batch of CASES[S] -> [(Z, info)] (computed once; do not modify)"""
    from riskaversetrajopt_amd import drone_gaussian_ipm as ipm
    a = CASES[S]
    return ipm.solve_batch(models(S, a), starts(S, a), tol=TOL, max_iter=max_iter, backend='numpy', callbacks=host_callbacks(S, a))


# ---- designed buffers of the dense kernels ---------------------------------------------------------------------------------
def graded(rng, shape, signed=True):
    """values graded over 12 orders of magnitude: 10^U(-6, 6), with a random sign"""
    v = 10.0 ** rng.uniform(-6.0, 6.0, shape)
    return v * rng.choice([-1.0, 1.0], shape) if signed else v


@functools.lru_cache(maxsize=None)
def designed(n, m0, m1, per_problem, K=3):
    """-> dict(J0 (K, m0, n), J1 (m1, n) | (K, m1, n) | None, d (K, m), hess (K, n (n + 1) / 2), diag (K, n), x (K, n), w (K, m),
    J [k] (m, n) the stacked matrix).  Computed once per shape; do not modify."""
    rng = np.random.RandomState(1000 * n + 10 * m0 + m1 + (5 if per_problem else 0))
    m = m0 + m1
    J0 = graded(rng, (K, m0, n))
    J1 = None if m1 == 0 else graded(rng, (K, m1, n) if per_problem else (m1, n))
    d = graded(rng, (K, m), signed=False)
    J = [J0[k] if m1 == 0 else np.vstack([J0[k], J1[k] if per_problem else J1]) for k in range(K)]
    return dict(J0=J0, J1=J1, d=d, hess=graded(rng, (K, n * (n + 1) // 2)), diag=graded(rng, (K, n), signed=False),
                x=graded(rng, (K, n)), w=graded(rng, (K, m)), J=J, m=m)


def unpack(tril, n):
    r, c = np.tril_indices(n)
    H = np.zeros((n, n), dtype=tril.dtype)
    H[r, c] = tril
    H[c, r] = tril
    return H


@functools.lru_cache(maxsize=None)
def jdj_reference(n, m0, m1, per_problem, K=3):
    """J' diag(d) J and sum_r |J_ra d_r J_rb| per entry in np.longdouble -> [(ref, mag)] per problem"""
    des = designed(n, m0, m1, per_problem, K)
    out = []
    for k in range(K):
        Jl, dl = des["J"][k].astype(LD), des["d"][k].astype(LD)
        out.append(((Jl.T * dl) @ Jl, (np.abs(Jl).T * dl) @ np.abs(Jl)))
    return out


def normal_reference(n, m0, m1, per_problem, k, with_hess, with_diag=True):
    """-> (Kc, bound) in np.longdouble: the exact value and gamma_(m + 3) sum |terms| per entry"""
    des = designed(n, m0, m1, per_problem)
    ref, mag = jdj_reference(n, m0, m1, per_problem)[k]
    if with_hess:
        H = unpack(des["hess"][k].astype(LD), n)
        ref, mag = ref + H, mag + np.abs(H)
    if with_diag:
        g = np.diag(des["diag"][k].astype(LD))
        ref, mag = ref + g, mag + g
    return ref, gamma(des["m"] + 3) * mag


def padded(a, ld):
    """the array with its last axis widened to ld, NaN in the padding"""
    a = np.asarray(a, dtype=np.float64)
    out = np.full(a.shape[:-1] + (ld,), np.nan)
    out[..., :a.shape[-1]] = a
    return out
