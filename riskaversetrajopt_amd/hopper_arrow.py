"""The arrowhead Newton step of the hopper's interior-point solve (``hopper_ipm.solve_batch(newton='arrow')``): the
same step as the dense one for any M.  The M variables ys enter Kc only through E = diag(e) + d_0 1 1' and one row each of B, so
they are eliminated exactly and the Cholesky factors the core's Schur complement (8(S+1) + 4S + 2 columns) -- the same inertia
test, since e > 0.  ``ArrowDeviceBackend`` does the work over the samples with csrc/hopper_arrow.hip on the partials
rato_hopper_slip_f64 leaves and the deterministic rows with ``hopper_ipm``'s ``normal_matrix`` / ``csc_matvec`` / ``csc_tmatvec`` on
the core's pattern; ``ArrowNumpyBackend`` is its host twin.  Both keep their own factor and solve (the elimination).
Under ``driver='device'`` ``ArrowDeviceBackend`` serves device tensors: its ``*_t`` methods do the same step
without a read-back, the host-side fix-ups of the list methods being kernels of csrc/hopper_arrow.hip.
"""
import time

import numpy as np

from . import hopper as _h
from . import ipm as _ipm
from .hopper_ipm import (GroupFields, ModelCallbacks, _hess_apply, _obj_add, _pattern_maps, arrow_einv, arrow_kkbeta, arrow_rhsfix, arrow_scale,
                         arrow_tfix, assemble_g, csc_matvec, csc_tmatvec, normal_matrix, normal_matrix_host, scatter_rows,
                         upload_maps)


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


class ArrowDeviceBackend(_ipm.DeviceBase):
    """The arrowhead step on the MI355X for the problems of one group (csrc/hopper_arrow.hip on the partials rato_hopper_slip_f64
    leaves in HBM; the core through ``hopper_ipm.normal_matrix`` on the deterministic pattern and the Cholesky of ``ipm.DeviceBase``).
    eval_full keeps the partials: neither the slip CSC values nor the tril-packed Hessian are ever formed.  What travels to the
    host per call of a list method is the vectors the driver works on and O(q) sums; the ``*_t`` methods (the driver on the
    device) move nothing.  The group's models may hold friction fields of their own (``hopper_ipm.GroupFields``)."""
    name, newton = "device", "arrow"

    def __init__(self, models, chol='workgroup'):
        import torch
        from . import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.models = models
        m0 = self.m0 = models[0]
        if any(m.precision != 'f64' for m in models):
            raise ValueError("the device backend needs Model(..., precision='f64')")
        super().__init__(m0.device, len(models), "reduction", "assembly", "products", chol=chol)
        st = self.st = arrow_structure(m0)
        lay = m0.nlp_layout()
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
        self.maps = upload_maps(st["det"], self.dev, to_col=st["core_z"], col_ptr=st["det_indptr_z"])     # x and J'w in z numbering
        self.maps.update(qcol=up(st["qcol"], np.int32), map_defect=up(lay["map_defect"], np.int64),
                         map_rows=up(lay["map_rows"], np.int64), scale_rows=up(lay["scale_rows"], np.float64),
                         det_const=up(lay["det_const"], np.float64))
        self.params = _h.nlp_params(m0.S, m0.time_jump, m0.time_land, m0.dt)
        self.nch = int(self.lib.rato_hopper_arrow_nchunks(st["M"]))
        self.npart = int(self.lib.rato_hopper_arrow_npart(st["C"]))
        if self.nch < 1 or self.npart < 1:
            raise ValueError(f"newton='arrow' on the device serves 1 <= C <= 50 contact steps, got C = {st['C']}")
        self.vals0 = self.dx = self.dfz = self.hessd = self.hess_host = None
        self.fields = GroupFields(models)
        n_all = len(models)
        self.e, self.d = self._empty(n_all, st["M"]), self._empty(n_all, st["ncon"])
        self.kk, self.beta = np.zeros(n_all), np.zeros(n_all)

    def _empty(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.dev)

    def _malpha(self, idx):
        return np.array([self.st["M"] * float(self.models[i].alpha) for i in idx])

    def _g_rows(self, idx, Zs, lin, h):
        defect, rows = lin["defect"].cpu().numpy(), lin["rows"].cpu().numpy()
        slip = np.ascontiguousarray(h.cpu().numpy().transpose(0, 2, 1)).reshape(len(idx), -1)          # row order i C + c
        return [assemble_g(self.models[i], np.asarray(Z), defect[k], rows[k], slip[k]) for k, (i, Z) in enumerate(zip(idx, Zs))]

    def eval_full(self, idx, Zs, lams, sfs):
        with self.timed("callbacks"):
            m0, mp, K = self.m0, self.maps, len(idx)
            Zd, lamd = self._up(Zs), self._up(lams)
            lin = _h.nlp_linearize_device(self.params, Zd)
            jac = mp["det_const"][None].repeat(K, 1).contiguous()
            _h.scatter_f64(lin["d_defect"].view(K, -1), mp["map_defect"], jac)
            _h.scatter_f64(lin["d_rows"].view(K, -1), mp["map_rows"], jac, mp["scale_rows"])
            slip = m0.slip_device_f64(Zd, lamd, want=("h", "dh_dfz", "dh_dx"), fields=self.fields.of(idx))
            add = self._up([_obj_add(m0, sf) for sf in sfs])
            m0.slip_hess_blocks_device_f64(Zd, slip["D"], add)
            lam_dyn, lam_rows = m0.fold_multipliers(np.stack(lams))
            self.hessd = _h.nlp_hessian_device(self.params, Zd, self._up(list(lam_dyn)), self._up(list(lam_rows)), add)
            self.vals0, self.dx, self.dfz = jac, slip["dh_dx"], slip["dh_dfz"]
            self.slot = {i: k for k, i in enumerate(idx)}
            self.hess_host = self.hessd.cpu().numpy()
            out = self._g_rows(idx, Zs, lin, slip["h"])
        return out

    def eval_g(self, idx, Zs):
        with self.timed("callbacks"):
            Zd = self._up(Zs)
            lin = _h.nlp_linearize_device(self.params, Zd, want=("defect", "rows"))
            out = self._g_rows(idx, Zs, lin, self.m0.slip_device_f64(Zd, want=("h",), fields=self.fields.of(idx))["h"])
        return out

    def hess_apply(self, idx, X):
        return [_hess_apply(self.st["hess"], self.hess_host[self.slot[i]], x) for i, x in zip(idx, X)]

    def _sel(self, idx):
        return self._rows(idx, self.vals0, self.dx, self.dfz, self.hessd)

    def _call(self, name, *args):
        with self.torch.cuda.device(self.dev):
            self._lib.check(getattr(self.lib, name)(*args, self._lib.current_stream()), name)

    def matvec(self, idx, X):
        with self.timed("products"):
            st, p = self.st, self._lib.ptr
            M, Cn, K = st["M"], st["C"], len(idx)
            v0, dx, dfz, _ = self._sel(idx)
            xh = np.stack(X)
            x = self._up(X)
            out = csc_matvec(st, self.maps, v0, None, x)                # the deterministic rows; the risk rows below
            xq, xy = self._up(list(xh[:, st["qz"]])), x[:, st["y0"]:st["y0"] + M].contiguous()
            part, red = self._empty(self.nch, K), self._empty(K)
            self._call("rato_hopper_arrow_rows_f64", K, M, Cn, int(st["saa"]), 0, p(dx), p(dfz), p(xq), p(xy), None, 0, st["r0"],
                       None, p(out), st["ncon"], p(part), p(red))
            o = out.cpu().numpy()
            if st["saa"]:
                o[:, st["rr"]] = self._malpha(idx) * xh[:, st["n"] - 1] + red.cpu().numpy()
        return list(o)

    def _cols(self, mode, dx, dfz, w, t, yout):
        """rato_hopper_arrow_cols_f64 -> (K, 5C + 1) host"""
        st, p = self.st, self._lib.ptr
        K = w.shape[0]
        part, red = self._empty(self.nch, K, 5 * st["C"] + 1), self._empty(K, 5 * st["C"] + 1)
        self._call("rato_hopper_arrow_cols_f64", K, st["M"], st["C"], int(st["saa"]), mode, p(dx), p(dfz), p(w), w.shape[1], st["r0"],
                   p(t), p(yout), p(part), p(red))
        return red.cpu().numpy()

    def _minus_fx_total(self, red):
        """-sum_c of the fx column sums (the slack and t_risk columns hold -1 in every slip row), contacts ascending one
        problem-wise addition at a time: np.sum over an axis of a (K, C) array picks its order by K"""
        tot = np.zeros(red.shape[0])
        for c in range(self.st["C"]):
            tot -= red[:, 5 * c + 3]
        return tot

    def tmatvec(self, idx, W):
        with self.timed("products"):
            st = self.st
            M, Cn, K = st["M"], st["C"], len(idx)
            v0, dx, dfz, _ = self._sel(idx)
            wh = np.stack(W)
            w = self._up(W)
            out = csc_tmatvec(st, self.maps, v0, None, w)
            yout = self._empty(K, M)
            red = self._cols(0, dx, dfz, w, None, yout)
            o = out.cpu().numpy()
            tot = self._minus_fx_total(red)
            o[:, st["qz"][:5 * Cn]] += red[:, :5 * Cn]
            o[:, st["n"] - 2] += tot
            if st["saa"]:
                o[:, st["n"] - 1] += self._malpha(idx) * wh[:, st["rr"]] + tot
                o[:, st["y0"]:st["y0"] + M] = yout.cpu().numpy()
        return list(o)

    def schur(self, idx, D, diags, out=None):
        """-> (Shat (K, nc, lda) device tensor, lower triangle; e (K, M) and d (K, ncon) device; red (K, n_part) and d on the
        host): the core's Schur complement of the listed problems (``out``: a contiguous (K, nc, lda >= nc) tensor to write into)"""
        st, mp, p = self.st, self.maps, self._lib.ptr
        M, Cn, nc, K = st["M"], st["C"], st["nc"], len(idx)
        v0, dx, dfz, hs = self._sel(idx)
        dh = np.stack(D)
        d, dgh = self._up(D), np.stack(diags)
        dg, yd = self._up(list(dgh[:, st["core_z"]])), self._up(list(dgh[:, st["y0"]:st["y0"] + M]))
        t0 = time.perf_counter()
        Sh = normal_matrix(nc, st["ncon"], mp, v0, None, d, hs, dg, out=out)       # the deterministic rows' J'DJ + W + the diagonal
        self._sync()
        t1 = time.perf_counter()
        e, part, red = self._empty(K, M), self._empty(self.nch, K, self.npart), self._empty(K, self.npart)
        self._call("rato_hopper_arrow_reduce_f64", K, M, Cn, int(st["saa"]), p(dx), p(dfz), p(d), st["ncon"], st["r0"], p(yd), p(e),
                   p(part), p(red))
        self._sync()
        t2 = time.perf_counter()
        ma = self._up([self._malpha(idx)])[0].contiguous()
        self._call("rato_hopper_arrow_assemble_f64", K, M, Cn, int(st["saa"]), nc, Sh.shape[2], p(mp["qcol"]), p(red), p(d),
                   st["ncon"], st["r0"], p(ma), p(Sh))
        self._sync()
        t3 = time.perf_counter()
        self.clock["normal"] += t1 - t0
        self.clock["reduction"] += t2 - t1
        self.clock["assembly"] += t3 - t2
        return Sh, e, d, red.cpu().numpy(), dh

    def factor(self, idx, D, diags):
        torch, st = self.torch, self.st
        Sh, e, d, red, dh = self.schur(idx, D, diags)
        t1 = time.perf_counter()
        info = self.factor_device(idx, Sh)
        sel = torch.as_tensor(list(idx), device=self.dev)
        self.e[sel], self.d[sel] = e, d
        if st["saa"]:
            q = st["q"]
            s = red[:, q * (q + 1) // 2 + 2 * q]
            d0 = dh[:, st["rr"]]
            self.kk[list(idx)] = d0 / (1.0 + d0 * s)
            self.beta[list(idx)] = d0 * self._malpha(idx)
        self.clock["factor"] += time.perf_counter() - t1
        return info

    def _einv(self, e, v, kk):
        """E^-1 v for (K, M) device tensors: u o (v - k (u'v))"""
        p = self._lib.ptr
        K, M = v.shape
        kappa = np.zeros(K)
        if self.st["saa"]:
            part, red = self._empty(self.nch, K), self._empty(K)
            self._call("rato_hopper_arrow_edot_f64", K, M, p(e), p(v), p(part), p(red))
            kappa = kk * red.cpu().numpy()
        out, kap = self._empty(K, M), self._up([kappa])[0].contiguous()   # kap stays referenced until the launch is queued
        self._call("rato_hopper_arrow_eapply_f64", K, M, p(e), p(v), p(kap), p(out))
        return out

    def solve(self, idx, B):
        with self.timed("solve"):
            st, p = self.st, self._lib.ptr
            M, Cn, K, q = st["M"], st["C"], len(idx), st["q"]
            rows = [self.slot[i] for i in idx]
            sel = self.torch.as_tensor(list(idx), device=self.dev)
            ssel = self.torch.as_tensor(rows, device=self.dev)
            e, d = self.e.index_select(0, sel), self.d.index_select(0, sel)
            dx, dfz = self.dx.index_select(0, ssel), self.dfz.index_select(0, ssel)
            kk, beta = self.kk[list(idx)], self.beta[list(idx)]
            bh = np.stack(B)
            rc = bh[:, st["core_z"]].copy()
            ry = self._up(list(bh[:, st["y0"]:st["y0"] + M]))
            if st["saa"]:
                t = self._einv(e, ry, kk)
                red = self._cols(1, dx, dfz, d, t, None)
                tot = self._minus_fx_total(red)
                rc[:, st["qcol"][:5 * Cn]] -= red[:, :5 * Cn]
                rc[:, -2] -= tot
                rc[:, -1] -= tot + beta * red[:, 5 * Cn]
            xch = self.solve_device(idx, list(rc))
            if st["saa"]:
                rem = self._empty(K, M)                                    # r_y - B x_c
                xq, addc = self._up(list(xch[:, st["qcol"]])), self._up([beta * xch[:, -1]])[0].contiguous()
                self._call("rato_hopper_arrow_rows_f64", K, M, Cn, 1, 1, p(dx), p(dfz), p(xq), p(ry), p(d), st["ncon"], st["r0"],
                           p(addc), p(rem), M, None, None)
                ry = rem
            ry = self._einv(e, ry, kk)
            out = np.empty((K, st["n"]))
            out[:, st["core_z"]] = xch
            out[:, st["y0"]:st["y0"] + M] = ry.cpu().numpy()
        return list(out)

    # ---- the same on device tensors, for ``ipm.solve_group_device``: every call serves the whole group, takes and
    # returns (K, ld) tensors, waits for nothing and moves nothing to the host.  What the list methods fix up on the host is done
    # by the ``arrow_*`` bindings of ``hopper_ipm`` (bitwise the host's lines); gathers and scatters between z numbering, core
    # numbering and the touched columns go through rato_scatter_f64 with the maps of ``arrow_structure``.
    def _work(self):
        """the work buffers of the group and the uploaded maps, made once"""
        w = getattr(self, "_w", None)
        if w is None:
            st, K, torch = self.st, self.n_all, self.torch
            M, q, nc = st["M"], st["q"], st["nc"]
            up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
            w = self._w = dict(
                xq=self._empty(K, q), xy=self._empty(K, M), yout=self._empty(K, M), dg=self._empty(K, nc), yd=self._empty(K, M),
                rc=self._empty(K, nc), ry=self._empty(K, M), t=self._empty(K, M), rem=self._empty(K, M), addc=self._empty(K),
                part1=self._empty(self.nch, K), red1=self._empty(K), partc=self._empty(self.nch, K, 5 * st["C"] + 1),
                redc=self._empty(K, 5 * st["C"] + 1), partr=self._empty(self.nch, K, self.npart), redr=self._empty(K, self.npart),
                kk=self._empty(K), beta=self._empty(K), malpha=self._up([self._malpha(range(K))])[0].contiguous(),
                add=self._empty(K, self.m0.S + 1, _h.n_pairs), qz=up(st["qz"], np.int32), core_z=up(st["core_z"], np.int64),
                inv_qz=up(st["inv_qz"], np.int64), inv_core_z=up(st["inv_core_z"], np.int64), inv_qcol=up(st["inv_qcol"], np.int64))
        return w

    def _g_t(self, Z, lin, h):
        m0, st = self.m0, self.st
        return _h.g_device(m0._slip_params(), st["M"], st["saa"], Z, lin["defect"], lin["rows"], h, (1, st["M"]),
                           self._work()["malpha"])

    def eval_full_t(self, Z, Y):
        """Z (K, n) and the multipliers Y (K, ld >= ncon), read where they lie -> g (K, ncon); leaves the deterministic rows'
        values, the slip partials and the step blocks of hess(Y . g) for the calls below.  The objective's curvature is NOT in the
        blocks: the driver's diagonal carries it."""
        m0, mp, w, K = self.m0, self.maps, self._work(), Z.shape[0]
        lin = _h.nlp_linearize_device(self.params, Z)
        jac = mp["det_const"][None].repeat(K, 1).contiguous()
        _h.scatter_f64(lin["d_defect"].view(K, -1), mp["map_defect"], jac)
        _h.scatter_f64(lin["d_rows"].view(K, -1), mp["map_rows"], jac, mp["scale_rows"])
        slip = m0.slip_device_f64(Z, Y[:, :self.st["ncon"]], want=("h", "dh_dfz", "dh_dx"), fields=self.fields.of())
        add = w["add"].zero_()
        m0.slip_hess_blocks_device_f64(Z, slip["D"], add)
        lam_dyn, lam_rows = m0.fold_multipliers_device(Y)
        self.hessd = _h.nlp_hessian_device(self.params, Z, lam_dyn, lam_rows, add)
        self.vals0, self.dx, self.dfz = jac, slip["dh_dx"], slip["dh_dfz"]
        self.slot = {i: i for i in range(K)}
        return self._g_t(Z, lin, slip["h"])

    def eval_g_t(self, Z):
        lin = _h.nlp_linearize_device(self.params, Z, want=("defect", "rows"))
        return self._g_t(Z, lin, self.m0.slip_device_f64(Z, want=("h",), fields=self.fields.of())["h"])

    def hess_apply_t(self, X):
        """W x of the constraints' part alone (K, n)"""
        return _h.block_symv(self.m0.S, self.hessd, X, self.st["n"])

    def matvec_t(self, X):
        """X (K, ld >= n) -> J x (K, ncon)"""
        with self.timed_t("products"):
            st, w, p = self.st, self._work(), self._lib.ptr
            M, Cn, n, K = st["M"], st["C"], st["n"], X.shape[0]
            out = csc_matvec(st, self.maps, self.vals0, None, X)
            xq = scatter_rows(X, n, w["inv_qz"], w["xq"], st["q"])
            xy = w["xy"].copy_(X[:, st["y0"]:st["y0"] + M])
            self._call("rato_hopper_arrow_rows_f64", K, M, Cn, int(st["saa"]), 0, p(self.dx), p(self.dfz), p(xq), p(xy), None, 0,
                       st["r0"], None, p(out), st["ncon"], p(w["part1"]), p(w["red1"]))
            if st["saa"]:
                arrow_scale(w["malpha"], X, n - 1, w["red1"], out, st["rr"])
        return out

    def tmatvec_t(self, W):
        """W (K, ld >= ncon) -> J' w (K, n)"""
        with self.timed_t("products"):
            st, w, p = self.st, self._work(), self._lib.ptr
            M, Cn, K = st["M"], st["C"], W.shape[0]
            out = csc_tmatvec(st, self.maps, self.vals0, None, W)
            self._call("rato_hopper_arrow_cols_f64", K, M, Cn, int(st["saa"]), 0, p(self.dx), p(self.dfz), p(W), W.shape[1], st["r0"],
                       None, p(w["yout"]), p(w["partc"]), p(w["redc"]))
            arrow_tfix(M, Cn, st["saa"], st["n"], w["qz"], w["redc"], w["malpha"], W, st["rr"], w["yout"], out)
        return out

    def factor_t(self, d, diag):
        """d (K, ld >= ncon) and diag (K, n) with the objective's curvature already in it: the core's Schur complement into the
        kept ``self.Kc`` (normal_matrix on the core pattern, reduce, assemble), factored in place -> info (K,) int32 device tensor.
        e, kk and beta stay on the device; ``d`` is kept by reference for ``solve_t``."""
        st, mp, w, p = self.st, self.maps, self._work(), self._lib.ptr
        M, Cn, nc, K = st["M"], st["C"], st["nc"], d.shape[0]
        with self.timed_t("normal"):
            dg = scatter_rows(diag, st["n"], w["inv_core_z"], w["dg"], nc)
            yd = w["yd"].copy_(diag[:, st["y0"]:st["y0"] + M])
            self.Kc = normal_matrix(nc, st["ncon"], mp, self.vals0, None, d, self.hessd, dg, out=self.Kc)
        with self.timed_t("reduction"):
            self._call("rato_hopper_arrow_reduce_f64", K, M, Cn, int(st["saa"]), p(self.dx), p(self.dfz), p(d), d.shape[1], st["r0"],
                       p(yd), p(self.e), p(w["partr"]), p(w["redr"]))
        with self.timed_t("assembly"):
            self._call("rato_hopper_arrow_assemble_f64", K, M, Cn, int(st["saa"]), nc, self.Kc.shape[2], p(mp["qcol"]), p(w["redr"]),
                       p(d), d.shape[1], st["r0"], p(w["malpha"]), p(self.Kc))
            if st["saa"]:
                arrow_kkbeta(Cn, d, st["rr"], w["redr"], w["malpha"], w["kk"], w["beta"])
            self.d_t = d
        return self.factor_all(self.Kc)

    def _einv_t(self, v, out):
        """E^-1 v for (K, >= M) device tensors into ``out``: kappa is formed on the device"""
        w, p = self._work(), self._lib.ptr
        K, M = v.shape[0], self.st["M"]
        if not self.st["saa"]:
            return arrow_einv(self.e, v, None, None, out)
        self._call("rato_hopper_arrow_edot_f64", K, M, p(self.e), p(v), p(w["part1"]), p(w["red1"]))
        return arrow_einv(self.e, v, w["kk"], w["red1"], out)

    def solve_t(self, B):
        """the elimination in place on B (K, ld >= n) in z numbering, from what ``factor_t`` kept"""
        with self.timed_t("solve"):
            st, w, p = self.st, self._work(), self._lib.ptr
            M, Cn, nc, n, K, y0 = st["M"], st["C"], st["nc"], st["n"], B.shape[0], st["y0"]
            d = self.d_t
            rc = scatter_rows(B, n, w["inv_core_z"], w["rc"], nc)
            ry = w["ry"].copy_(B[:, y0:y0 + M])
            if st["saa"]:
                t = self._einv_t(ry, w["t"])
                self._call("rato_hopper_arrow_cols_f64", K, M, Cn, 1, 1, p(self.dx), p(self.dfz), p(d), d.shape[1], st["r0"], p(t),
                           None, p(w["partc"]), p(w["redc"]))
                arrow_rhsfix(Cn, nc, self.maps["qcol"], w["redc"], w["beta"], rc)
            self.chol_solve(self.L, rc[:, None, :])
            if st["saa"]:
                xq = scatter_rows(rc, nc, w["inv_qcol"], w["xq"], st["q"])
                arrow_scale(w["beta"], rc, nc - 1, None, w["addc"], 0)
                self._call("rato_hopper_arrow_rows_f64", K, M, Cn, 1, 1, p(self.dx), p(self.dfz), p(xq), p(ry), p(d), d.shape[1],
                           st["r0"], p(w["addc"]), p(w["rem"]), M, None, None)
                ry = w["rem"]
            self._einv_t(ry, B[:, y0:y0 + M])
            scatter_rows(rc, nc, w["core_z"], B, n)
        return B
