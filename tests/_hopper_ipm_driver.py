"""Shared by the tests of the hopper solve under the interior-point driver on the device (test_hopper_ipm_driver_cpu.py,
test_gpu_hopper_ipm_driver.py): the designed batches of tests/_ipm_driver.py with a linear objective term, the host driver's
branches on them with one comparison log per problem, np.longdouble references of the places ``lin`` enters in
csrc/ipm_driver.hip, and the pieces of the hopper's g as designed host arrays.

The objective is f = sf (1/2 sum curv z^2 + sum lin z).  ``lin`` enters gradf = sf (curv z + lin) -- hence rz, dual, E0 and,
through gradf, Dbar -- and the two objective values (the step setup's record, phi_t).  Bounds (Higham §3.1, as in
tests/_ipm_driver.py): each formula of _ipm_driver.ref_* gains one rounding (the addition of the linear term, fused or not) and
the linear term's magnitude among its |terms|: sf |lin| in a gradient, |lin| |z| in an objective."""
import functools

import numpy as np

import _ipm_driver as D
from _drone_gaussian_ipm import LD, gamma

SHAPES = [(1, 0, 1), (5, 2, 3), (65, 7, 0), (300, 10, 700)]
PATTERN = "mixed"


class QuadLin(D.Quad):
    """``_ipm_driver.Quad`` plus a linear term: f = 1/2 sum curv z^2 + lin . z"""

    def __init__(self, quad, lin):
        super().__init__(quad.curv, quad.gL, quad.gU, quad.xL, quad.xU)
        self.lin = lin

    def f(self, Z):
        Z = np.asarray(Z, dtype=np.float64)
        return 0.5 * float(np.sum(self.curv * Z * Z)) + float(np.sum(self.lin * Z))

    def grad_f(self, Z):
        return self.curv * np.asarray(Z, dtype=np.float64) + self.lin


@functools.lru_cache(maxsize=None)
def designed_lin(n, mE, mI):
    """``_ipm_driver.designed(n, mE, mI, 'mixed')`` with the models rebuilt as QuadLin: lin graded over 12 orders of magnitude (7,
    up to 10, in the converged problem, as every other value there), of mixed sign, a fifth of it exactly zero; J'y shifted by
    -sf lin, so the designed residuals stay the designed ones.  A new dict: the cached design is not touched.  Computed once
    per shape; do not modify."""
    des = D.designed(n, mE, mI, PATTERN)
    rng = np.random.RandomState(104729 + 7919 * n + 101 * mE + 13 * mI)
    models, JTy = [], des["JTy"].copy()
    for k, kind in enumerate(D.KINDS):
        top = 1.0 if kind == "converged" else 6.0
        lin = 10.0 ** rng.uniform(-6.0, top, n) * rng.choice([-1.0, 1.0], n)
        lin[rng.rand(n) < 0.2] = 0.0
        if n > 1:
            lin[0] = 10.0 ** top                                     # the largest magnitude is present
        models.append(QuadLin(des["models"][k], lin))
        JTy[k] = JTy[k] - des["state"][k]["sf"] * lin
    out = dict(des)
    out.update(models=models, JTy=JTy)
    return out


def host_chain(des):
    """``_ipm_driver.host_chain`` with one comparison log per problem -> (ps, passes, accepted [2 rounds], logs [K])"""
    from riskaversetrajopt_amd import ipm
    logs = [D.Log() for _ in range(D.K)]
    ps = D.problems(des)
    passes = [D.host_residual_phase(p, des["g"][k], des["JTy"][k], False, logs[k]) for k, p in enumerate(ps)]
    run = [k for k, p in enumerate(ps) if not p.done]
    assert ipm.newton_steps(D.Scripted(des), run, [ps[k] for k in run]) == [True] * len(run)
    for k in run:
        ps[k].dv = des["dv"][k].copy()                               # the designed step takes over from here
        D.host_step_setup(ps[k], des["Hdv"][k][:ps[k].n] + ps[k].sf * ps[k].model.curv * ps[k].dv[:ps[k].n], logs[k])
    accepted = []
    for r in range(2):
        for k in run:
            if not ps[k].accepted and not ps[k].done:
                ps[k].vt = ps[k].v + ps[k].alpha * ps[k].dv
        G = D.trial_g(des, ps, r)
        accepted.append([k for k in run if not ps[k].accepted and not ps[k].done and D.host_trial(ps[k], G[k], logs[k])])
    return ps, passes, accepted, logs


def decided(log):
    """every finite comparison of the log keeps the relative distance ``_ipm_driver.MARGIN`` between its two sides: the device,
    which rounds in another order, must decide as the host did"""
    return all(margin >= D.MARGIN for _, margin in log.margins())


# ---- np.longdouble references: name -> (value, bound) ---------------------------------------------------------------------------
def _gradf(p, s):
    v, curv, lin = D._ld(s["v"][:p.n], p.model.curv, p.model.lin)
    sf = LD(s["sf"])
    return sf * (curv * v + lin), sf * (np.abs(curv * v) + np.abs(lin))


def ref_residuals(p, s, g, JTy):
    """``_ipm_driver.ref_residuals`` with the linear term: gradf, prim, dual, E0"""
    n = p.n
    v, zl, zu, y, gl, jt = D._ld(s["v"], s["zl"], s["zu"], s["y"], g, JTy)
    gE = p.gE.astype(LD)
    c, cm = np.empty(p.m, dtype=LD), np.empty(p.m, dtype=LD)
    c[p.E], cm[p.E] = gl[p.E] - gE, np.abs(gl[p.E]) + np.abs(gE)
    c[p.I], cm[p.I] = gl[p.I] - v[n:], np.abs(gl[p.I]) + np.abs(v[n:])
    gf, gfm = _gradf(p, s)
    out = {"gradf": (gf, gamma(4) * gfm)}
    rz, rzb = gf + jt - zl[:n] + zu[:n], gamma(7) * (gfm + np.abs(jt) + zl[:n] + zu[:n])
    rs, rsb = -y[p.I] - zl[n:] + zu[n:], gamma(3) * (np.abs(y[p.I]) + zl[n:] + zu[n:])
    dL, dU, _, _ = D._dist(p, s["v"])
    cl, clb = np.where(p.hasL, zl * dL, 0), gamma(3) * np.where(p.hasL, zl * np.abs(dL), 0)
    cu, cub = np.where(p.hasU, zu * dU, 0), gamma(3) * np.where(p.hasU, zu * np.abs(dU), 0)
    mx = lambda a: np.max(np.abs(a)) if a.size else LD(0)
    prim, dual = mx(c), max(mx(rz), mx(rs))
    out["prim"], out["dual"] = (prim, mx(gamma(2) * cm)), (dual, max(mx(rzb), mx(rsb)))
    out["E0"] = (max(prim, dual, mx(cl), mx(cu)), max(mx(gamma(2) * cm), mx(rzb), mx(rsb), mx(clb), mx(cub)))
    return out


def ref_rz(p, s, mu, JTy):
    """the rz of prepare_step: gradf + J'y + gbar_z, from the state and the device's mu"""
    n = p.n
    jt, = D._ld(JTy)
    _, _, iL, iU = D._dist(p, s["v"])
    mu = LD(mu)
    gb, gm = (-mu * iL + mu * iU)[:n], (mu * np.abs(iL) + mu * np.abs(iU))[:n]
    gf, gfm = _gradf(p, s)
    return gf + jt + gb, gamma(13) * (gfm + np.abs(jt) + gm)


def _objective(p, v):
    vl, curv, lin = D._ld(np.asarray(v)[:p.n], p.model.curv, p.model.lin)
    return 0.5 * np.sum(curv * vl * vl) + np.sum(lin * vl), 0.5 * np.sum(curv * vl * vl) + np.sum(np.abs(lin * vl))


def ref_objective(p, v):
    ob, mag = _objective(p, v)
    return ob, gamma(p.n + 4) * mag


def ref_phi(dev):
    """phi from the device's own objective, barrier, nu and c1 (``dev`` downloaded after the step setup)"""
    sf, ob, bar, nu, c1 = LD(dev.sf), LD(dev.objective), LD(dev.barrier), LD(dev.nu), LD(dev.c1)
    return sf * ob + bar + nu * c1, gamma(5) * (sf * abs(ob) + abs(bar) + nu * c1)


def ref_phi_t(p, dev, vt, gt):
    """``_ipm_driver.ref_phi_t`` with the linear term, from the device's own vt"""
    n = p.n
    vtl, g = D._ld(vt, gt)
    mu, nu, sf = LD(dev.mu), LD(dev.nu), LD(dev.sf)
    gE = p.gE.astype(LD)
    ct = np.concatenate([np.abs(g[p.E] - gE), np.abs(g[p.I] - vtl[n:])])
    ctm = np.concatenate([np.abs(g[p.E]) + np.abs(gE), np.abs(g[p.I]) + np.abs(vtl[n:])])
    c1, c1b = np.sum(ct), gamma(p.m + 1) * np.sum(ctm)
    ob, mag = _objective(p, vt)
    obb = gamma(n + 4) * mag
    bar, barb = D._barrier(p, vt, dev.mu)
    return sf * ob + bar + nu * c1, sf * obb + barb + nu * c1b + gamma(5) * (sf * abs(ob) + abs(bar) + nu * c1)


# ---- the hopper's g from designed pieces ---------------------------------------------------------------------------------------
def g_pieces(model, K, seed, alphas):
    """designed host inputs of rato_hopper_g_f64 for K problems of ``model``'s shape: Z (K, nvar), defect (K, S, 8), rows
    (K, S+1, 2), slip_rows (K, M C) in the rows' order i C + c, of mixed sign and graded over six orders, and malpha (K,)"""
    rng = np.random.RandomState(seed)
    lay = model.nlp_layout()
    S, M, Cn = model.S, model.M, lay["C"]
    val = lambda *shape: rng.uniform(-2, 2, shape) * 10.0 ** rng.randint(-3, 4, shape)
    return dict(Z=val(K, lay["nvar"]), defect=val(K, S, 8), rows=val(K, S + 1, 2), slip_rows=val(K, M * Cn),
                malpha=np.array([M * float(a) for a in alphas]))


def g_sum_row(model, Z, malpha):
    """the SAA group's sum row M alpha t + sum ys in longdouble -> (value, sum |terms|)"""
    from riskaversetrajopt_amd import hopper
    nX, nU = hopper.n_x * (model.S + 1), hopper.n_u * model.S
    ys, t = D._ld(Z[nX + nU:-2], Z[-1])
    return LD(malpha) * t + np.sum(ys), abs(LD(malpha) * t) + np.sum(np.abs(ys))
