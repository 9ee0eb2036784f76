"""The arrowhead Newton step of the hopper's interior-point solve (``hopper_ipm.solve_batch(newton='arrow')``): the
same step as the dense one for any M.  The M variables ys enter Kc only through E = diag(e) + d_0 1 1' and one row each of B, so
they are eliminated exactly and the Cholesky factors the core's Schur complement (8(S+1) + 4S + 2 columns) -- the same inertia
test, since e > 0.  ``ArrowDeviceBackend`` does the work over the samples with csrc/hopper_arrow.hip on the partials
rato_hopper_slip_f64 leaves and the deterministic rows with ``hopper_ipm``'s ``normal_matrix`` / ``csc_matvec`` / ``csc_tmatvec`` on
the core's pattern; ``ArrowNumpyBackend`` is its host twin.  Both keep their own factor and solve (the elimination).  The
evaluation itself is ``hopper.Model``'s: ``ArrowDeviceBackend._evaluate`` is a call sequence over its stages that keeps the slip
partials, and g, W x and the group's constants are ``hopper_ipm.HopperDeviceBase``'s.
``ArrowDeviceBackend`` has one step, written on device tensors with every line between two launches a kernel of
csrc/hopper_arrow.hip: the ``*_t`` methods (``driver='device'``) run it on the group's arrays where they lie, and
the list methods (``driver='host'``) upload the listed problems' vectors, run it on those problems' rows and download the result.
"""
import contextlib

import numpy as np

from . import hopper as _h
from . import ipm as _ipm
from .hopper_ipm import (HopperDeviceBase, ModelCallbacks, _hess_apply, _pattern_maps, arrow_einv, arrow_kkbeta, arrow_rhsfix, arrow_scale,
                         arrow_tfix, csc_matvec, csc_tmatvec, normal_matrix, normal_matrix_host, scatter_rows, upload_maps)


def arrow_structure(model):
    """Host-only index lists of the arrowhead step; nothing in it grows faster than O(M C).  z = (core, y): the core
    c = (xs, us, slack, t_risk) has n_c = 8(S+1) + 4S + 2 columns, y = ys has M.
      n, nc, ncon, M, C, saa, q = 5C + 2, r0 (g index of the slip row of sample 0, contact 0), rr (the sum row; -1: baseline)
      core_z (nc,)       z index of a core column;  y0: z index of y_0
      qcol (q,), qz (q,) core / z index of the touched columns: per contact (x0, x2, x3, fx, fz) of its step, then slack, t_risk
      det                ``_pattern_maps`` of the deterministic rows on the core columns (value index = position in
                         ``nlp_layout()``'s det values; ent_of is n_c x n_c whatever M is)
      det_rows, det_cols_z   the deterministic pattern as coordinate lists in z numbering
      pos_det, pos_slip  where the two value arrays lie in the full pattern (the NumPy twin splits injected values with them)
      inv_qz (n,), inv_core_z (n,), inv_qcol (nc,)   the inverse maps of qz, core_z and qcol (-1: the column has no target): what
                         rato_scatter_f64 takes to gather x[qz], z[core_z] and xc[qcol] on the device"""
    st = getattr(model, "_ipm_arrow", None)
    if st is not None:
        return st
    lay = model.nlp_layout()
    S, M, Cn, n, ncon = model.S, model.M, lay["C"], lay["nvar"], lay["ncon"]
    if Cn < 1:
        raise ValueError("newton='arrow' needs at least one contact step; use newton='dense'")
    saa = model.method != 'baseline'
    nXU = _h.n_x * (S + 1) + _h.n_u * S
    nc = nXU + 2
    det_indptr = np.asarray(lay["det_indptr"], dtype=np.int64)
    assert det_indptr[nXU] == det_indptr[n - 2]                    # no deterministic row touches a y column
    det = _pattern_maps(lay["det_indices"], np.concatenate([det_indptr[:nXU], det_indptr[n - 2:]]), nc, ncon, S)
    core_z = np.concatenate([np.arange(nXU), [n - 2, n - 1]]).astype(np.int64)
    steps = model.contact_steps()
    nX = _h.n_x * (S + 1)
    qcol = np.concatenate([np.stack([_h.n_x * steps, _h.n_x * steps + 2, _h.n_x * steps + 3, nX + _h.n_u * steps + 2,
                                     nX + _h.n_u * steps + 3], axis=1).reshape(-1), [nc - 2, nc - 1]]).astype(np.int64)
    r_ncon, r0 = model.risk_rows_offset()
    assert r_ncon == ncon
    st = dict(n=n, nc=nc, ncon=ncon, M=M, C=Cn, saa=saa, q=5 * Cn + 2, r0=int(r0), rr=int(r0 - M - 1) if saa else -1, y0=nXU,
              core_z=core_z, qcol=qcol, qz=core_z[qcol], det=det, det_rows=np.asarray(lay["det_indices"], dtype=np.int64),
              det_cols_z=np.repeat(np.arange(n, dtype=np.int64), np.diff(det_indptr)), det_indptr_z=det_indptr,
              pos_det=np.asarray(lay["pos_det"]), pos_slip=np.asarray(lay["pos_slip"]),
              hess=dict(n=n, block_vars=det["block_vars"].copy()))
    st["hess"]["block_vars"][st["hess"]["block_vars"] == nc] = n
    for name, fwd, size in (("inv_qz", st["qz"], n), ("inv_core_z", core_z, n), ("inv_qcol", qcol, nc)):
        assert np.unique(fwd).size == fwd.size
        inv = -np.ones(size, dtype=np.int64)
        inv[fwd] = np.arange(fwd.size)
        st[name] = inv
    model._ipm_arrow = st
    return st


def arrow_terms(st, dx, dfz, d, ydiag, malpha):
    """The sample block of one problem on the host.  dx (C, 3, M), dfz (C, M) the slip partials, d (ncon,), ydiag (M,) = Sigma_y +
    delta_w, malpha = M alpha.  -> dict(e (M,), Bq (M, q) = B_s on the touched columns, A (q, q) the slip rows' own share, T (q, q)
    what is added to the core's matrix, d0, beta, k, s): E = diag(e) + d0 1 1', B = B_s + beta 1 e_t'."""
    M, Cn, q, r0, saa = st["M"], st["C"], st["q"], st["r0"], st["saa"]
    dic = d[r0:r0 + M * Cn].reshape(M, Cn)
    g = np.stack([dx[:, 0].T, dx[:, 1].T, dx[:, 2].T, np.ones((M, Cn)), dfz.T], axis=2)            # (M, C, 5)
    dsum = dic.sum(axis=1)
    Bq = np.zeros((M, q))
    Bq[:, :5 * Cn] = (-dic[:, :, None] * g).reshape(M, 5 * Cn)
    Bq[:, 5 * Cn] = dsum
    A = np.zeros((q, q))
    tq = 5 * Cn + 1
    for c in range(Cn):
        N = np.zeros((M, q))
        N[:, 5 * c:5 * c + 5] = g[:, c]
        N[:, 5 * Cn] = -1.0
        if saa:
            N[:, tq] = -1.0
        A += N.T @ (dic[:, c, None] * N)
    if not saa:
        return dict(e=ydiag.copy(), Bq=None, A=A, T=A, d0=0.0, beta=0.0, k=0.0, s=0.0)
    Bq[:, tq] = dsum
    e = ydiag + d[st["rr"] + 1:st["rr"] + 1 + M] + dsum
    u = 1.0 / e
    d0 = float(d[st["rr"]])
    beta = d0 * malpha
    G, w, s = Bq.T @ (u[:, None] * Bq), Bq.T @ u, float(np.sum(u))
    k = d0 / (1.0 + d0 * s)
    et = np.zeros(q)
    et[tq] = 1.0
    v = w + beta * s * et
    T = A - (G + beta * (np.outer(w, et) + np.outer(et, w)) + beta * beta * s * np.outer(et, et)) + k * np.outer(v, v)
    T[tq, tq] += d0 * malpha * malpha
    return dict(e=e, Bq=Bq, A=A, T=T, d0=d0, beta=beta, k=k, s=s)


def _risk_matvec(st, dx, dfz, malpha, x, out):
    """out[risk rows] = J_risk x from the partials (x in z numbering)"""
    M, Cn, r0 = st["M"], st["C"], st["r0"]
    xq = x[st["qz"]]
    h = np.einsum("cjm,cj->mc", dx, xq[:5 * Cn].reshape(Cn, 5)[:, :3]) + xq[3:5 * Cn:5][None, :] + dfz.T * xq[4:5 * Cn:5][None, :]
    h = h - xq[5 * Cn]
    if st["saa"]:
        xy = x[st["y0"]:st["y0"] + M]
        h = h - xq[5 * Cn + 1] - xy[:, None]
        out[st["rr"]] = malpha * xq[5 * Cn + 1] + np.sum(xy)
        out[st["rr"] + 1:st["rr"] + 1 + M] = -xy
    out[r0:r0 + M * Cn] = h.reshape(-1)
    return out


def _risk_tmatvec(st, dx, dfz, malpha, w, out):
    """out += J_risk' w from the partials (out in z numbering)"""
    M, Cn, r0 = st["M"], st["C"], st["r0"]
    wic = w[r0:r0 + M * Cn].reshape(M, Cn)
    cols = np.empty((Cn, 5))
    cols[:, :3] = np.einsum("cjm,mc->cj", dx, wic)
    cols[:, 3] = wic.sum(axis=0)
    cols[:, 4] = np.einsum("cm,mc->c", dfz, wic)
    tot = -np.sum(cols[:, 3])
    add = np.concatenate([cols.reshape(-1), [tot, 0.0]])
    if st["saa"]:
        add[5 * Cn + 1] = malpha * w[st["rr"]] + tot
        out[st["y0"]:st["y0"] + M] = w[st["rr"]] - w[st["rr"] + 1:st["rr"] + 1 + M] - wic.sum(axis=1)
    out[st["qz"]] += add
    return out


class ArrowNumpyBackend(_ipm.Backend):
    """The arrowhead step on the host: the same elimination as ``ArrowDeviceBackend``, from injected callbacks (or the Model's,
    one problem at a time).  ``callbacks[i]`` as for ``NumpyBackend``; of jac_values only the deterministic values and the slip
    partials dh/d(x0, x2, x3), dh/dfz are kept.  After ``factor``, ``parts[i]`` holds Shat (nc, nc) with ``arrow_terms``' pieces."""
    name, newton = "numpy", "arrow"

    def __init__(self, models, callbacks=None):
        self.models = models
        self.cb = [ModelCallbacks(m) for m in models] if callbacks is None else list(callbacks)
        super().__init__()
        self.st = arrow_structure(models[0])
        self.det, self.dx, self.dfz, self.hess, self.parts = {}, {}, {}, {}, {}

    def _malpha(self, i):
        return self.st["M"] * float(self.models[i].alpha)

    def set_values(self, i, vals, hess):
        """install Jacobian values on the full CSC pattern and step blocks as problem i's current evaluation"""
        st = self.st
        M, Cn = st["M"], st["C"]
        vals = np.asarray(vals, dtype=np.float64)
        slip = vals[st["pos_slip"]]
        self.det[i] = vals[st["pos_det"]]
        self.dx[i] = slip[:3 * Cn * M].reshape(Cn, 3, M).copy()
        self.dfz[i] = slip[3 * Cn * M:5 * Cn * M].reshape(Cn, 2, M)[:, 1].copy()
        self.hess[i] = np.asarray(hess, dtype=np.float64)

    def eval_full(self, idx, Zs, lams, sfs):
        with self.timed("callbacks"):
            out = []
            for i, Z, lam, sf in zip(idx, Zs, lams, sfs):
                self.set_values(i, self.cb[i].jac_values(Z), self.cb[i].hess_blocks(Z, lam, sf))
                out.append(np.asarray(self.cb[i].g(Z), dtype=np.float64))
        return out

    def eval_g(self, idx, Zs):
        with self.timed("callbacks"):
            return [np.asarray(self.cb[i].g(Z), dtype=np.float64) for i, Z in zip(idx, Zs)]

    def hess_apply(self, idx, X):
        return [_hess_apply(self.st["hess"], self.hess[i], x) for i, x in zip(idx, X)]

    def matvec(self, idx, X):
        st = self.st
        out = []
        for i, x in zip(idx, X):
            o = np.bincount(st["det_rows"], weights=self.det[i] * x[st["det_cols_z"]], minlength=st["ncon"])
            out.append(_risk_matvec(st, self.dx[i], self.dfz[i], self._malpha(i), x, o))
        return out

    def tmatvec(self, idx, W):
        st = self.st
        out = []
        for i, w in zip(idx, W):
            o = np.bincount(st["det_cols_z"], weights=self.det[i] * w[st["det_rows"]], minlength=st["n"])
            out.append(_risk_tmatvec(st, self.dx[i], self.dfz[i], self._malpha(i), w, o))
        return out

    def factor(self, idx, D, diags):
        st = self.st
        info = []
        for i, d, dg in zip(idx, D, diags):
            with self.timed("normal"):
                Sh = normal_matrix_host(st["det"], self.det[i], d, self.hess[i], dg[st["core_z"]])
                P = arrow_terms(st, self.dx[i], self.dfz[i], d, dg[st["y0"]:st["y0"] + st["M"]], self._malpha(i))
                Sh[np.ix_(st["qcol"], st["qcol"])] += P["T"]
                P["Shat"] = Sh
                self.parts[i] = P
            with self.timed("factor"):
                info.append(self.factor_host(i, Sh, bool(np.all(P["e"] > 0.0))))
        return info

    def solve(self, idx, B):
        st = self.st
        with self.timed("solve"):
            out = []
            for i, b in zip(idx, B):
                P = self.parts[i]
                u = 1.0 / P["e"]
                einv = (lambda v: u * (v - P["k"] * (u @ v))) if st["saa"] else (lambda v: u * v)
                rc, ry = b[st["core_z"]].copy(), b[st["y0"]:st["y0"] + st["M"]]
                t = einv(ry)
                if st["saa"]:
                    bt = P["Bq"].T @ t
                    bt[-1] += P["beta"] * np.sum(t)
                    rc[st["qcol"]] -= bt
                xc = self.solve_host(i, rc)
                if st["saa"]:
                    ry = ry - (P["Bq"] @ xc[st["qcol"]] + P["beta"] * xc[-1])
                x = np.empty(st["n"])
                x[st["core_z"]] = xc
                x[st["y0"]:st["y0"] + st["M"]] = einv(ry)
                out.append(x)
        return out


class ArrowDeviceBackend(HopperDeviceBase):
    """The arrowhead step on the MI355X (csrc/hopper_arrow.hip on the partials rato_hopper_slip_f64 leaves in HBM; the core
    through ``hopper_ipm.normal_matrix`` on the deterministic pattern and the Cholesky of ``ipm.DeviceBase``).  Its evaluation
    is the stages of ``hopper.Model`` with the slip partials kept: neither the slip CSC values nor the tril-packed Hessian are
    ever formed, and nothing in it grows faster than O(M C).  What travels per call of a list method is the vectors the driver
    works on, up and down once; the ``*_t`` methods (the driver on the device) move nothing."""
    newton = "arrow"

    def __init__(self, models, chol='workgroup'):
        import torch
        from . import _lib
        self._lib, self.lib = _lib, _lib.load()
        super().__init__(models, "reduction", "assembly", "products", chol=chol)
        st = self.st = arrow_structure(self.m0)
        self.hess_st = st["hess"]
        self.maps = upload_maps(st["det"], self.dev, to_col=st["core_z"], col_ptr=st["det_indptr_z"])     # x and J'w in z numbering
        self.maps["qcol"] = torch.as_tensor(np.ascontiguousarray(st["qcol"], dtype=np.int32), device=self.dev)
        self.nch = int(self.lib.rato_hopper_arrow_nchunks(st["M"]))
        self.npart = int(self.lib.rato_hopper_arrow_npart(st["C"]))
        if self.nch < 1 or self.npart < 1:
            raise ValueError(f"newton='arrow' on the device serves 1 <= C <= 50 contact steps, got C = {st['C']}")
        self.vals0 = self.dx = self.dfz = None
        n_all = len(models)
        self.e, self.d = self._empty(n_all, st["M"]), self._empty(n_all, st["ncon"])     # what a factorization keeps, by problem
        self.kk, self.beta, self.d_t = self._empty(n_all), self._empty(n_all), None       # number (d_t: the device driver's d)

    def _empty(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.dev)

    def _evaluate(self, Z, Y, add, idx):
        """the stages of ``hopper.Model`` on device tensors Z (K, >= n) and Y (K, ld >= ncon) for the listed problems (None: the
        whole group): leaves the deterministic rows' values, the slip partials and the step blocks of hess(Y . g) + add (``add``:
        a scratch buffer, used in place) -> (defect, rows, slip_h), what g is assembled from"""
        m0 = self.m0
        lin = _h.nlp_linearize_device(m0._slip_params(), Z)
        self.vals0 = m0.det_jacobian_values(lin, Z.shape[0])
        slip = m0.slip_device_f64(Z, Y[:, :self.st["ncon"]], want=("h", "dh_dfz", "dh_dx"), fields=self.fields.of(idx))
        self.dx, self.dfz = slip["dh_dx"], slip["dh_dfz"]
        self.hessd = m0.hess_blocks_device(Z, Y, add, slip["D"], in_place=True)
        return lin["defect"], lin["rows"], slip["h"]

    # ---- the arrow step, written once on device tensors and served to both drivers.  Each function takes the arrays it reads
    # (``vals`` = (vals0, dx, dfz, hessd) of its K problems, malpha (K,)), what a factorization keeps (e (K, M), d (K, ld >= ncon),
    # kk and beta (K,), the factor L) and work buffers ``w`` for K problems; vectors are (K, ld) tensors where they lie.  Nothing
    # here waits or moves anything to the host: a line between two launches is an ``arrow_*`` binding of ``hopper_ipm``, a gather
    # or scatter between z numbering, core numbering and the touched columns rato_scatter_f64 with ``arrow_structure``'s maps.
    def _call(self, name, *args):
        with self.torch.cuda.device(self.dev):
            self._lib.check(getattr(self.lib, name)(*args, self._lib.current_stream()), name)

    def _buffers(self, K):
        """the step's work buffers for K problems"""
        st = self.st
        M, q, nc = st["M"], st["q"], st["nc"]
        return dict(xq=self._empty(K, q), xy=self._empty(K, M), yout=self._empty(K, M), dg=self._empty(K, nc), yd=self._empty(K, M),
                    rc=self._empty(K, nc), ry=self._empty(K, M), t=self._empty(K, M), rem=self._empty(K, M), addc=self._empty(K),
                    part1=self._empty(self.nch, K), red1=self._empty(K), partc=self._empty(self.nch, K, 5 * st["C"] + 1),
                    redc=self._empty(K, 5 * st["C"] + 1), partr=self._empty(self.nch, K, self.npart),
                    redr=self._empty(K, self.npart))

    def _work(self):
        """the work buffers of the group and the uploaded maps, made once"""
        w = getattr(self, "_w", None)
        if w is None:
            st, K, torch = self.st, self.n_all, self.torch
            up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
            w = self._w = dict(
                self._buffers(K), add=self._empty(K, self.m0.S + 1, _h.n_pairs), qz=up(st["qz"], np.int32), core_z=up(st["core_z"], np.int64),
                inv_qz=up(st["inv_qz"], np.int64), inv_core_z=up(st["inv_core_z"], np.int64), inv_qcol=up(st["inv_qcol"], np.int64))
        return w

    def _jx(self, X, vals, malpha, w):
        """X (K, ld >= n) -> J x (K, ncon)"""
        st, p = self.st, self._lib.ptr
        M, Cn, n, K = st["M"], st["C"], st["n"], X.shape[0]
        v0, dx, dfz, _ = vals
        out = csc_matvec(st, self.maps, v0, None, X)                    # the deterministic rows; the risk rows below
        xq = scatter_rows(X, n, w["inv_qz"], w["xq"], st["q"])
        xy = w["xy"].copy_(X[:, st["y0"]:st["y0"] + M])
        self._call("rato_hopper_arrow_rows_f64", K, M, Cn, int(st["saa"]), 0, p(dx), p(dfz), p(xq), p(xy), None, 0, st["r0"], None,
                   p(out), st["ncon"], p(w["part1"]), p(w["red1"]))
        if st["saa"]:
            arrow_scale(malpha, X, n - 1, w["red1"], out, st["rr"])
        return out

    def _jtw(self, W, vals, malpha, w):
        """W (K, ld >= ncon) -> J' w (K, n)"""
        st, p = self.st, self._lib.ptr
        M, Cn, K = st["M"], st["C"], W.shape[0]
        v0, dx, dfz, _ = vals
        out = csc_tmatvec(st, self.maps, v0, None, W)
        self._call("rato_hopper_arrow_cols_f64", K, M, Cn, int(st["saa"]), 0, p(dx), p(dfz), p(W), W.shape[1], st["r0"], None,
                   p(w["yout"]), p(w["partc"]), p(w["redc"]))
        arrow_tfix(M, Cn, st["saa"], st["n"], w["qz"], w["redc"], malpha, W, st["rr"], w["yout"], out)
        return out

    def _schur(self, d, diag, vals, malpha, e, kk, beta, out, w):
        """d (K, ld >= ncon) and diag (K, n) -> the core's Schur complement (K, nc, lda), lower triangle, written into ``out`` (a
        contiguous (K, nc, lda >= nc) tensor; None: a new one): normal_matrix on the core pattern, reduce, assemble.  Fills e
        (K, M) and, with SAA, kk and beta (K,)."""
        st, mp, p = self.st, self.maps, self._lib.ptr
        M, Cn, nc, K = st["M"], st["C"], st["nc"], d.shape[0]
        v0, dx, dfz, hs = vals
        with self.timed_t("normal"):
            dg = scatter_rows(diag, st["n"], w["inv_core_z"], w["dg"], nc)
            yd = w["yd"].copy_(diag[:, st["y0"]:st["y0"] + M])
            Kc = normal_matrix(nc, st["ncon"], mp, v0, None, d, hs, dg, out=out)   # the deterministic rows' J'DJ + W + the diagonal
        with self.timed_t("reduction"):
            self._call("rato_hopper_arrow_reduce_f64", K, M, Cn, int(st["saa"]), p(dx), p(dfz), p(d), d.shape[1], st["r0"], p(yd),
                       p(e), p(w["partr"]), p(w["redr"]))
        with self.timed_t("assembly"):
            self._call("rato_hopper_arrow_assemble_f64", K, M, Cn, int(st["saa"]), nc, Kc.shape[2], p(mp["qcol"]), p(w["redr"]),
                       p(d), d.shape[1], st["r0"], p(malpha), p(Kc))
            if st["saa"]:
                arrow_kkbeta(Cn, d, st["rr"], w["redr"], malpha, kk, beta)
        return Kc

    def _einv(self, e, kk, v, out, w):
        """E^-1 v = u o (v - kk (u'v)), u = 1 / e, for v and out (K, >= M)"""
        p = self._lib.ptr
        if not self.st["saa"]:
            return arrow_einv(e, v, None, None, out)
        self._call("rato_hopper_arrow_edot_f64", v.shape[0], self.st["M"], p(e), p(v), p(w["part1"]), p(w["red1"]))
        return arrow_einv(e, v, kk, w["red1"], out)

    def _solve(self, B, vals, kept, w):
        """the elimination in place on B (K, ld >= n) in z numbering, from what the factorization kept"""
        st, p = self.st, self._lib.ptr
        M, Cn, nc, n, K, y0 = st["M"], st["C"], st["nc"], st["n"], B.shape[0], st["y0"]
        (_, dx, dfz, _), (e, d, kk, beta, L) = vals, kept
        rc = scatter_rows(B, n, w["inv_core_z"], w["rc"], nc)
        ry = w["ry"].copy_(B[:, y0:y0 + M])
        if st["saa"]:
            t = self._einv(e, kk, ry, w["t"], w)
            self._call("rato_hopper_arrow_cols_f64", K, M, Cn, 1, 1, p(dx), p(dfz), p(d), d.shape[1], st["r0"], p(t), None,
                       p(w["partc"]), p(w["redc"]))
            arrow_rhsfix(Cn, nc, self.maps["qcol"], w["redc"], beta, rc)
        self.chol_solve(L, rc[:, None, :])
        if st["saa"]:
            xq = scatter_rows(rc, nc, w["inv_qcol"], w["xq"], st["q"])
            arrow_scale(beta, rc, nc - 1, None, w["addc"], 0)
            self._call("rato_hopper_arrow_rows_f64", K, M, Cn, 1, 1, p(dx), p(dfz), p(xq), p(ry), p(d), d.shape[1], st["r0"],
                       p(w["addc"]), p(w["rem"]), M, None, None)                   # r_y - B x_c
            ry = w["rem"]
        self._einv(e, kk, ry, B[:, y0:y0 + M], w)
        scatter_rows(rc, nc, w["core_z"], B, n)
        return B

    # ---- the list methods (the driver on the host): upload the listed problems' vectors, take their rows of the arrays, run the
    # step, write what is kept back under the problems' numbers, download.  The clocks end in a device-wide wait.
    def _vals(self):
        return self.vals0, self.dx, self.dfz, self.hessd

    def _listed(self, idx, *kept):
        """-> (vals, malpha, w, *kept) of the listed problems: their rows of the value arrays by ``slot``, of malpha and of the
        ``kept`` arrays by problem number, and work buffers for them -- the group's own arrays when everyone is listed in order"""
        w = self._work()
        vals = self._rows(idx, *self._vals())
        if list(idx) == list(range(self.n_all)):
            return (vals, self.malpha, w) + kept
        sel = self.torch.as_tensor(list(idx), device=self.dev)
        take = lambda t: t.index_select(0, sel)
        return (vals, take(self.malpha), dict(w, **self._buffers(len(idx)))) + tuple(take(t) for t in kept)

    @contextlib.contextmanager
    def _waited(self):
        """``timed_t`` with a device-wide wait behind every block, whatever the class's ``sync_clocks`` says"""
        self.sync_clocks = True
        try:
            yield
        finally:
            del self.sync_clocks

    def matvec(self, idx, X):
        with self.timed("products"):
            return list(self._jx(self._up(X), *self._listed(idx)).cpu().numpy())

    def tmatvec(self, idx, W):
        with self.timed("products"):
            return list(self._jtw(self._up(W), *self._listed(idx)).cpu().numpy())

    def _schur_listed(self, idx, D, diags, out=None):
        """``_schur`` of the listed problems into arrays of their own -> (Shat, e, d, kk, beta, w), all on the device"""
        K = len(idx)
        vals, malpha, w = self._listed(idx)
        d, e, kk, beta = self._up(D), self._empty(K, self.st["M"]), self._empty(K), self._empty(K)
        with self._waited():
            Sh = self._schur(d, self._up(diags), vals, malpha, e, kk, beta, out, w)
        return Sh, e, d, kk, beta, w

    def schur(self, idx, D, diags, out=None):
        """-> (Shat (K, nc, lda) device tensor, lower triangle; e (K, M) and d (K, ncon) device; red (K, n_part) and d on the
        host): the core's Schur complement of the listed problems (``out``: a contiguous (K, nc, lda >= nc) tensor to write into).
        Nothing that is kept changes."""
        Sh, e, d, _, _, w = self._schur_listed(idx, D, diags, out)
        return Sh, e, d, w["redr"].cpu().numpy(), np.stack(D)

    def factor(self, idx, D, diags):
        Sh, e, d, kk, beta, _ = self._schur_listed(idx, D, diags)
        with self.timed("factor"):
            info = self.factor_device(idx, Sh)
            sel = self.torch.as_tensor(list(idx), device=self.dev)
            self.e[sel], self.d[sel], self.kk[sel], self.beta[sel] = e, d, kk, beta
        return info

    def solve(self, idx, B):
        with self.timed("solve"):
            vals, _, w, *kept = self._listed(idx, self.e, self.d, self.kk, self.beta, self.L)
            return list(self._solve(self._up(B), vals, kept, w).cpu().numpy())

    # ---- the same on device tensors, for ``ipm.solve_group_device``: every call serves the whole group where its
    # arrays lie, takes and returns (K, ld) tensors, waits for nothing and moves nothing to the host
    def eval_full_t(self, Z, Y):
        """the base's, with the group's kept ``add`` buffer zeroed as the scratch the slip share goes into"""
        return super().eval_full_t(Z, Y, self._work()["add"].zero_())

    def matvec_t(self, X):
        """X (K, ld >= n) -> J x (K, ncon)"""
        with self.timed_t("products"):
            return self._jx(X, self._vals(), self.malpha, self._work())

    def tmatvec_t(self, W):
        """W (K, ld >= ncon) -> J' w (K, n)"""
        with self.timed_t("products"):
            return self._jtw(W, self._vals(), self.malpha, self._work())

    def factor_t(self, d, diag):
        """d (K, ld >= ncon) and diag (K, n) with the objective's curvature already in it: the core's Schur complement into the
        kept ``self.Kc``, factored in place -> info (K,) int32 device tensor.  e, kk and beta stay on the device; ``d`` is kept by
        reference for ``solve_t``."""
        self.Kc = self._schur(d, diag, self._vals(), self.malpha, self.e, self.kk, self.beta, self.Kc, self._work())
        self.d_t = d
        return self.factor_all(self.Kc)

    def solve_t(self, B):
        """the elimination in place on B (K, ld >= n) in z numbering, from what ``factor_t`` kept"""
        with self.timed_t("solve"):
            return self._solve(B, self._vals(), (self.e, self.d_t, self.kk, self.beta, self.L), self._work())
