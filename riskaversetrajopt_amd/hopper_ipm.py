"""Batched primal-dual interior-point solver for the hopper NLP (hopper/hopper.py:486-669: what the script hands to IPOPT).

  min f(z)  s.t.  gL <= g(z) <= gU,  xL <= z <= xU          (``hopper.Model.ipopt_callbacks()``)

Rows with gL == gU are equalities E; every other row I gets a slack, g_I(z) - s = 0, gL_I <= s <= gU_I.  v = (z, s).  A bound
with |b| >= 1e14 is absent; present bounds are relaxed outward by 1e-8 max(1, |b|) (IPOPT's bound_relax_factor: the constant
row ``0 <= 0`` of the SAA group becomes harmless).  The objective is scaled by sf = min(1, 100 / max |grad f(Z0)|).

Newton step, condensed.  With Sigma = zl / (v - vL) + zu / (vU - v), eliminating s and y_I:
  Kc = W + diag(Sigma_z) + delta_w I + J_I' diag(Sigma_s) J_I + (1 / delta_c) J_E' J_E
  Kc dz = -r_z - J' w,   w = d c + (r_s on I, 0 on E),   d = (Sigma_s on I, 1 / delta_c on E)
  dy_E = (J_E dz + c_E) / delta_c,   ds = J_I dz + c_I,   dy_I = Sigma_s ds + r_s
delta_c = 1e-8 mu^(1/4) is always on (it tolerates the script's redundant rows); delta_w = 0, 1e-4, then x 8 until the Cholesky
of Kc succeeds: Kc positive definite <=> the regularised KKT matrix has the right inertia, so the factorization is the
inertia test.  Two steps of iterative refinement follow against the system with the equality block NOT condensed (unknowns
dz, dy_E), re-using the factor.

Two backends do the step: 'device' (csrc/hopper_ipm.hip: rato_normal_matrix_f64, rato_chol_factor_batch_f64,
rato_chol_solve_batch_f64, rato_csc_matvec_f64 / rato_csc_tmatvec_f64 on the values ``Model.nlp_device`` leaves in HBM, K
problems per launch) and 'numpy' (the whole step on the host, callbacks injected or taken one problem at a time from the
Model): the driver, the line search and the O(n + m) vector algebra are shared and run on the host per problem, so a problem's
iterates do not depend on what else is in the batch.

newton='arrow'  is the same step for any M: the M variables ys enter Kc only through E = diag(e) + d_0 1 1' and one
row each of B, so they are eliminated exactly and the Cholesky factors the core's Schur complement (8(S+1) + 4S + 2 columns)
-- the same inertia test, since e > 0.  ``ArrowDeviceBackend`` does the work over the samples with csrc/hopper_arrow.hip on the
partials rato_hopper_slip_f64 leaves, ``ArrowNumpyBackend`` is its host twin; newton='dense' (the default) is the step above.

The driver (``Problem``, ``newton_steps``, ``_solve_group``) knows a model through num_vars, gL_gU(), x_bounds(), f, grad_f and a
backend through eval_full / eval_g / matvec / tmatvec / factor / solve / hess_apply(idx, X) -> [W x]: ``drone_gaussian_ipm`` runs
it on dense backends of its own.
"""
import time

import numpy as np

from . import hopper as _h

ABSENT = 1e14
STATUSES = ("converged", "max_iter", "line_search")


# ---- fixed structure, built once next to nlp_layout() ------------------------------------------------------------------------
def structure(model):
    """Host-only index lists on ``model.nlp_layout()``'s fixed CSC pattern of jac_g (value index = position in jac_indices):
      n, ncon, nnz, rows, cols              the pattern as coordinate lists
      row_ptr, row_idx, row_col             the row list: row r holds the values row_idx[row_ptr[r]:row_ptr[r+1]] (columns ascending)
      ent_keys (a n + b, b <= a), ent_of    the structural lower-triangle entries of J'J + W + diagonal; ent_of [n n]: entry or -1
      ptr, tri_a, tri_b, tri_r, tri_ent     the product map: per entry the triples (value index of J_ra, of J_rb, row r) sorted by r
      hess_src [n_ent]                      where the entry lies in the step blocks (S+1, 78) flattened, or -1
      diag_ent [n]                          the entry of (a, a)
      to_cat [nnz]                          full value index -> index in the (deterministic, slip) concatenation the device holds
      block_vars (S+1, 12)                  z index of the local variables of a step block (n for the missing u of block S)"""
    st = getattr(model, "_ipm_structure", None)
    if st is not None:
        return st
    lay = model.nlp_layout()
    st = _pattern_maps(lay["jac_indices"], lay["jac_indptr"], lay["nvar"], lay["ncon"], model.S)
    to_cat = np.empty(st["nnz"], dtype=np.int64)
    to_cat[lay["pos_det"]] = np.arange(lay["pos_det"].size)
    to_cat[lay["pos_slip"]] = lay["pos_det"].size + np.arange(lay["pos_slip"].size)
    st.update(to_cat=to_cat, n_det=int(lay["pos_det"].size), n_slip=int(lay["pos_slip"].size))
    model._ipm_structure = st
    return st


def _pattern_maps(jac_indices, jac_indptr, n, ncon, S):
    """the index lists of ``structure`` for a CSC pattern with n columns whose first 8(S+1) + 4S are the step blocks' variables"""
    rows = np.asarray(jac_indices, dtype=np.int64)
    indptr = np.asarray(jac_indptr, dtype=np.int64)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    nnz = rows.size
    order = np.lexsort((cols, rows))
    row_idx, row_col = order, cols[order]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ncon))]).astype(np.int64)
    rl = np.diff(row_ptr)
    A, B, R, IA, IB = [], [], [], [], []
    for L in np.unique(rl[rl > 0]):
        rs = np.flatnonzero(rl == L)
        base = row_ptr[rs][:, None] + np.arange(L)[None, :]
        cidx, vidx = row_col[base], row_idx[base]
        i, j = np.tril_indices(L)
        A.append(cidx[:, i].ravel()), B.append(cidx[:, j].ravel())
        IA.append(vidx[:, i].ravel()), IB.append(vidx[:, j].ravel())
        R.append(np.repeat(rs, i.size))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    A, B, R, IA, IB = (cat(x) for x in (A, B, R, IA, IB))
    tr, tc = np.tril_indices(_h.n_l)
    bv = np.stack([_h.block_variables(S, t) for t in range(S + 1)])
    gr, gc = bv[:, tr], bv[:, tc]
    ok = (gr >= 0) & (gc >= 0)
    hkeys, hsrc = (gr * n + gc)[ok], np.flatnonzero(ok.reshape(-1))
    dkeys = np.arange(n, dtype=np.int64) * (n + 1)
    ent_keys = np.unique(np.concatenate([A * n + B, hkeys, dkeys]))
    tri_ent = np.searchsorted(ent_keys, A * n + B)
    o = np.lexsort((R, tri_ent))
    tri_ent, R, IA, IB = tri_ent[o], R[o], IA[o], IB[o]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(tri_ent, minlength=ent_keys.size))]).astype(np.int64)
    hess_src = -np.ones(ent_keys.size, dtype=np.int64)
    hess_src[np.searchsorted(ent_keys, hkeys)] = hsrc
    ent_of = -np.ones(n * n, dtype=np.int64)
    ent_of[ent_keys] = np.arange(ent_keys.size)
    return dict(n=n, ncon=ncon, nnz=nnz, rows=rows, cols=cols, indptr=indptr, row_ptr=row_ptr, row_idx=row_idx, row_col=row_col,
                ent_keys=ent_keys, ent_of=ent_of, ptr=ptr, tri_a=IA, tri_b=IB, tri_r=R, tri_ent=tri_ent, hess_src=hess_src,
                diag_ent=np.searchsorted(ent_keys, dkeys), block_vars=np.where(bv >= 0, bv, n))


def product_map(model):
    """the product map of ``structure(model)`` alone: dict(n, ent_a, ent_b, ptr, tri_a, tri_b, tri_r)"""
    st = structure(model)
    return dict(n=st["n"], ent_a=st["ent_keys"] // st["n"], ent_b=st["ent_keys"] % st["n"], ptr=st["ptr"], tri_a=st["tri_a"],
                tri_b=st["tri_b"], tri_r=st["tri_r"])


def normal_matrix_host(st, vals, d, hess=None, diag=None):
    """Kc = J' diag(d) J (+ the step blocks ``hess`` (S+1, 78), + diag) through the product map: each structural entry sums
    its triples in row order.  vals (nnz,) on the full CSC pattern.  -> dense symmetric (n, n)"""
    n = st["n"]
    terms = (vals[st["tri_a"]] * d[st["tri_r"]]) * vals[st["tri_b"]]
    ev = np.bincount(st["tri_ent"], weights=terms, minlength=st["ent_keys"].size)
    if hess is not None:
        hs = st["hess_src"]
        ev = ev + np.where(hs >= 0, np.asarray(hess).reshape(-1)[np.maximum(hs, 0)], 0.0)
    if diag is not None:
        ev[st["diag_ent"]] += diag
    Kc = np.zeros(n * n)
    Kc[st["ent_keys"]] = ev
    Kc = Kc.reshape(n, n)
    return Kc + np.tril(Kc, -1).T


def _hess_apply(st, blocks, x):
    """W x with W given as its step blocks (S+1, 78); the blocks hold disjoint variables"""
    tr, tc = np.tril_indices(_h.n_l)
    Bf = np.zeros((blocks.shape[0], _h.n_l, _h.n_l))
    Bf[:, tr, tc] = blocks
    Bf[:, tc, tr] = blocks
    xp = np.append(x, 0.0)
    yb = np.einsum("tab,tb->ta", Bf, xp[st["block_vars"]])
    out = np.zeros(st["n"] + 1)
    out[st["block_vars"]] = yb
    return out[:-1]


def _obj_add(model, sf):
    """sf hess_f as step blocks (S+1, 78): 2 R on u0 and u1, R = 1 (:443-448)"""
    tr, tc = np.tril_indices(_h.n_l)
    add = np.zeros((model.S + 1, _h.n_pairs))
    add[:model.S, np.flatnonzero((tr == tc) & ((tr == _h.n_x) | (tr == _h.n_x + 1)))] = 2.0 * sf
    return add


# ---- backends ----------------------------------------------------------------------------------------------------------------
class ModelCallbacks:
    """the numpy backend's default callbacks: the Model's own device callbacks, one problem at a time"""

    def __init__(self, model):
        self.m = model

    def g(self, Z):
        return self.m.g(Z)

    def jac_values(self, Z):
        return np.asarray(self.m.jac_g(Z).data, dtype=np.float64)

    def hess_blocks(self, Z, lam, obj_factor):
        return self.m._hess_device(Z, lam, obj_factor)["hess_blocks"][0].cpu().numpy()


class NumpyBackend:
    """the whole step on the host.  ``callbacks[i]`` serves models[i]: g(Z) (ncon,), jac_values(Z) (nnz,) on the full CSC
    pattern, hess_blocks(Z, lam, obj_factor) (S+1, 78)"""
    name = "numpy"

    def __init__(self, models, callbacks=None):
        self.models = models
        self.cb = [ModelCallbacks(m) for m in models] if callbacks is None else list(callbacks)
        self.st = structure(models[0])
        self.vals, self.hess, self.L = {}, {}, {}
        self.clock = dict(callbacks=0.0, normal=0.0, factor=0.0, solve=0.0)

    def eval_full(self, idx, Zs, lams, sfs):
        t0 = time.perf_counter()
        out = []
        for i, Z, lam, sf in zip(idx, Zs, lams, sfs):
            self.vals[i] = np.asarray(self.cb[i].jac_values(Z), dtype=np.float64)
            self.hess[i] = np.asarray(self.cb[i].hess_blocks(Z, lam, sf), dtype=np.float64)
            out.append(np.asarray(self.cb[i].g(Z), dtype=np.float64))
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

    def eval_g(self, idx, Zs):
        t0 = time.perf_counter()
        out = [np.asarray(self.cb[i].g(Z), dtype=np.float64) for i, Z in zip(idx, Zs)]
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

    def hess_blocks(self, i):
        return self.hess[i]

    def hess_apply(self, idx, X):
        return [_hess_apply(self.st, self.hess[i], x) for i, x in zip(idx, X)]

    def matvec(self, idx, X):
        st = self.st
        return [np.bincount(st["rows"], weights=self.vals[i] * x[st["cols"]], minlength=st["ncon"]) for i, x in zip(idx, X)]

    def tmatvec(self, idx, W):
        st = self.st
        return [np.bincount(st["cols"], weights=self.vals[i] * w[st["rows"]], minlength=st["n"]) for i, w in zip(idx, W)]

    def factor(self, idx, D, diags):
        info = []
        for i, d, dg in zip(idx, D, diags):
            t0 = time.perf_counter()
            Kc = normal_matrix_host(self.st, self.vals[i], d, self.hess[i], dg)
            t1 = time.perf_counter()
            ok = bool(np.all(np.isfinite(Kc)))
            if ok:
                try:
                    self.L[i] = np.linalg.cholesky(Kc)
                except np.linalg.LinAlgError:
                    ok = False
            self.clock["normal"] += t1 - t0
            self.clock["factor"] += time.perf_counter() - t1
            info.append(0 if ok else 1)
        return info

    def solve(self, idx, B):
        from scipy.linalg import solve_triangular
        t0 = time.perf_counter()
        out = [solve_triangular(self.L[i], solve_triangular(self.L[i], b, lower=True), lower=True, trans='T')
               for i, b in zip(idx, B)]
        self.clock["solve"] += time.perf_counter() - t0
        return out


def assemble_g(model, Z, defect, rows, slip_rows):
    """g in the script's order (:491-514) from what ``nlp_device`` leaves for one problem (host arrays)"""
    lay = model.nlp_layout()
    xs, us = model.convert_z_to_xs_us_mats(Z)
    stt, tj, tl = lay["states"], model.time_jump, model.time_land
    risk = model._risk_without_contacts(Z) if lay["C"] == 0 else model._risk_rows(Z, slip_rows)
    return np.concatenate([defect.reshape(-1), xs[0] - _h.state_initial, (xs[-1] - _h.state_final)[4:6], rows[stt, 0], rows[stt, 1],
                           -rows[tj:tl, 1], risk, us.reshape(-1), [Z[-2]], xs[1:, 3], xs[1:, 7], xs[1:, 6]])


class DeviceBackend:
    """the step on the MI355X for the problems of one group (same S, M, phases, method and friction fields; alpha may differ).
    Every call serves the listed problems in ONE launch each; nothing a kernel computes for a problem depends on the others."""
    name = "device"

    def __init__(self, models):
        import torch
        from . import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.models = models
        m0 = self.m0 = models[0]
        if any(m.precision != 'f64' for m in models):
            raise ValueError("the device backend needs Model(..., precision='f64')")
        self.dev = m0.device
        st = self.st = structure(m0)
        lay = m0.nlp_layout()
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
        tc = st["to_cat"]
        self.maps = dict(ent_of=up(st["ent_of"], np.int32), ptr=up(st["ptr"], np.int64), tri_a=up(tc[st["tri_a"]], np.int32),
                         tri_b=up(tc[st["tri_b"]], np.int32), tri_r=up(st["tri_r"], np.int32),
                         hess_src=up(st["hess_src"], np.int32), row_ptr=up(st["row_ptr"], np.int64),
                         row_idx=up(tc[st["row_idx"]], np.int32), row_col=up(st["row_col"], np.int32),
                         col_ptr=up(st["indptr"], np.int64), col_idx=up(tc, np.int32), col_row=up(st["rows"], np.int32))
        # the one Jacobian value that depends on alpha (row 0 of the t_risk column): patched per problem after the group's call
        self.saa = m0.method != 'baseline' and lay["C"] > 0
        self.alpha_pos = int(lay["nnz_slip"] - 1 - m0.M * lay["C"]) if self.saa else -1
        self.slot = {}                      # problem -> row of the current value arrays
        self.vals0 = self.vals1 = self.hessd = self.hess_host = self.L = None
        self.clock = dict(callbacks=0.0, normal=0.0, factor=0.0, solve=0.0)

    def _sync(self):
        self.torch.cuda.synchronize(self.dev)

    def _up(self, rows):
        return self.torch.as_tensor(np.ascontiguousarray(np.stack(rows), dtype=np.float64), device=self.dev)

    def _g_rows(self, idx, Zs, r):
        defect, rows = r["defect"].cpu().numpy(), r["rows"].cpu().numpy()
        slip = r["slip_rows"].cpu().numpy() if self.m0.nlp_layout()["C"] > 0 else [None] * len(idx)
        return [assemble_g(self.models[i], np.asarray(Z), defect[k], rows[k], slip[k]) for k, (i, Z) in enumerate(zip(idx, Zs))]

    def eval_full(self, idx, Zs, lams, sfs):
        t0 = time.perf_counter()
        torch = self.torch
        add = self._up([_obj_add(self.m0, sf) for sf in sfs])
        r = self.m0.nlp_device(self._up(Zs), self._up(lams), add=add)
        self.vals0, self.vals1, self.hessd = r["jac_values"], r["slip_jac_values"], r["hess_blocks"]
        if self.saa:
            self.vals1[:, self.alpha_pos] = torch.as_tensor([self.m0.M * float(self.models[i].alpha) for i in idx],
                                                            dtype=torch.float64, device=self.dev)
        self.slot = {i: k for k, i in enumerate(idx)}
        self.hess_host = self.hessd.cpu().numpy()
        out = self._g_rows(idx, Zs, r)
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

    def eval_g(self, idx, Zs):
        t0 = time.perf_counter()
        out = self._g_rows(idx, Zs, self.m0.nlp_device(self._up(Zs)))
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

    def set_values(self, vals, hess):
        """install given Jacobian values (K, nnz) on the full CSC pattern and step blocks (K, S+1, 78) as the current
        evaluation of problems 0 .. K-1 (what eval_full leaves), split into the two arrays the kernels read"""
        lay = self.m0.nlp_layout()
        vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
        self.vals0, self.vals1 = self._up(vals[:, lay["pos_det"]]), self._up(vals[:, lay["pos_slip"]])
        self.hess_host = np.ascontiguousarray(hess, dtype=np.float64)
        self.hessd = self._up(self.hess_host)
        self.slot = {i: i for i in range(vals.shape[0])}

    def hess_blocks(self, i):
        return self.hess_host[self.slot[i]]

    def hess_apply(self, idx, X):
        return [_hess_apply(self.st, self.hess_host[self.slot[i]], x) for i, x in zip(idx, X)]

    def _sel(self, idx):
        """the value arrays of the listed problems, in place when they are all of them in order"""
        rows = [self.slot[i] for i in idx]
        if rows == list(range(self.vals0.shape[0])):
            return self.vals0, self.vals1, self.hessd
        sel = self.torch.as_tensor(rows, device=self.dev)
        return tuple(t.index_select(0, sel).contiguous() for t in (self.vals0, self.vals1, self.hessd))

    def _list_matvec(self, entry, name, idx, X, n_out, ptr, lidx, other):
        _lib, st = self._lib, self.st
        v0, v1, _ = self._sel(idx)
        x = self._up(X)
        K = x.shape[0]
        out = self.torch.empty((K, n_out), dtype=self.torch.float64, device=self.dev)
        with self.torch.cuda.device(self.dev):
            _lib.check(entry(K, st["ncon"], st["n"], _lib.ptr(v0), v0.shape[1], st["n_det"], _lib.ptr(v1), v1.shape[1],
                             st["n_slip"], _lib.ptr(self.maps[ptr]), _lib.ptr(self.maps[lidx]), _lib.ptr(self.maps[other]),
                             _lib.ptr(x), x.shape[1], _lib.ptr(out), n_out, _lib.current_stream()), name)
        return list(out.cpu().numpy())

    def matvec(self, idx, X):
        return self._list_matvec(self.lib.rato_csc_matvec_f64, "rato_csc_matvec_f64", idx, X, self.st["ncon"], "row_ptr", "row_idx",
                                 "row_col")

    def tmatvec(self, idx, W):
        return self._list_matvec(self.lib.rato_csc_tmatvec_f64, "rato_csc_tmatvec_f64", idx, W, self.st["n"], "col_ptr", "col_idx",
                                 "col_row")

    def normal_matrix(self, idx, D, diags, with_hess=True, out=None):
        """-> Kc (K, n, lda) device tensor (lower triangle; ``out``: a contiguous (K, n, lda >= n) tensor to write into)"""
        _lib, st, torch, mp = self._lib, self.st, self.torch, self.maps
        v0, v1, hs = self._sel(idx)
        d, dg = self._up(D), (self._up(diags) if diags is not None else None)
        K, n = d.shape[0], st["n"]
        Kc = torch.empty((K, n, n), dtype=torch.float64, device=self.dev) if out is None else out
        if tuple(Kc.shape[:2]) != (K, n) or Kc.shape[2] < n or Kc.dtype != torch.float64 or not Kc.is_contiguous():
            raise ValueError(f"out must be a contiguous device float64 tensor ({K}, {n}, >= {n})")
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.rato_normal_matrix_f64(
                K, n, Kc.shape[2], _lib.ptr(v0), v0.shape[1], st["n_det"], _lib.ptr(v1), v1.shape[1], st["n_slip"], _lib.ptr(d), st["ncon"],
                _lib.ptr(hs if with_hess else None), hs.shape[1] * hs.shape[2], _lib.ptr(dg), _lib.ptr(mp["ent_of"]),
                _lib.ptr(mp["ptr"]), _lib.ptr(mp["tri_a"]), _lib.ptr(mp["tri_b"]), _lib.ptr(mp["tri_r"]), _lib.ptr(mp["hess_src"]),
                _lib.ptr(Kc), _lib.current_stream()), "rato_normal_matrix_f64")
        return Kc

    def factor(self, idx, D, diags):
        torch = self.torch
        t0 = time.perf_counter()
        Kc = self.normal_matrix(idx, D, diags)
        self._sync()
        t1 = time.perf_counter()
        info = chol_factor(Kc)
        if self.L is None or self.L.shape[0] < len(self.models):
            self.L = torch.empty((len(self.models),) + tuple(Kc.shape[1:]), dtype=torch.float64, device=self.dev)
        self.L[torch.as_tensor(list(idx), device=self.dev)] = Kc
        info = info.cpu().numpy()
        self.clock["normal"] += t1 - t0
        self.clock["factor"] += time.perf_counter() - t1
        return [int(v) for v in info]

    def solve(self, idx, B):
        t0 = time.perf_counter()
        L = self.L.index_select(0, self.torch.as_tensor(list(idx), device=self.dev))
        b = self._up(B)[:, None, :].contiguous()
        chol_solve(L, b)
        out = list(b[:, 0].cpu().numpy())
        self.clock["solve"] += time.perf_counter() - t0
        return out


def chol_panel_width():
    from . import _lib
    return int(_lib.load().rato_chol_panel_width())


def chol_factor(A):
    """rato_chol_factor_batch_f64 in place on a device fp64 tensor A (K, n, lda) (row-major lower triangle; lda >= n)
    -> info (K,) int32 device tensor: 0, or j + 1 for the first pivot j that is not positive and finite"""
    import torch
    from . import _lib
    if A.dim() != 3 or A.dtype != torch.float64 or not A.is_cuda or not A.is_contiguous() or A.shape[2] < A.shape[1] or A.shape[1] < 1:
        raise ValueError(f"A must be a contiguous device float64 tensor (K, n, lda >= n), got {tuple(A.shape)}")
    info = torch.empty(A.shape[0], dtype=torch.int32, device=A.device)
    with torch.cuda.device(A.device):
        _lib.check(_lib.load().rato_chol_factor_batch_f64(_lib.ptr(A), A.shape[1], A.shape[2], A.shape[0], _lib.ptr(info),
                                                          _lib.current_stream()), "rato_chol_factor_batch_f64")
    return info


def chol_solve(L, B):
    """rato_chol_solve_batch_f64: L (K, n, lda) as chol_factor leaves it, B (K, nrhs, ldb >= n) device fp64, solved in place"""
    import torch
    from . import _lib
    if L.dim() != 3 or B.dim() != 3 or L.dtype != torch.float64 or B.dtype != torch.float64 or not (L.is_contiguous() and B.is_contiguous()) \
            or B.shape[0] != L.shape[0] or B.shape[2] < L.shape[1] or L.shape[2] < L.shape[1] or L.device != B.device or not L.is_cuda:
        raise ValueError("chol_solve: L (K, n, lda >= n) and B (K, nrhs, ldb >= n) contiguous device float64 tensors")
    with torch.cuda.device(L.device):
        _lib.check(_lib.load().rato_chol_solve_batch_f64(_lib.ptr(L), L.shape[1], L.shape[2], L.shape[0], _lib.ptr(B), B.shape[1],
                                                         B.shape[2], _lib.current_stream()), "rato_chol_solve_batch_f64")
    return B


# ---- the arrowhead step: ys eliminated exactly (newton='arrow') ------------------------------------------------
def arrow_structure(model):
    """Host-only index lists of the arrowhead step; nothing in it grows faster than O(M C).  z = (core, y): the core
    c = (xs, us, slack, t_risk) has n_c = 8(S+1) + 4S + 2 columns, y = ys has M.
      n, nc, ncon, M, C, saa, q = 5C + 2, r0 (g index of the slip row of sample 0, contact 0), rr (the sum row; -1: baseline)
      core_z (nc,)       z index of a core column;  y0: z index of y_0
      qcol (q,), qz (q,) core / z index of the touched columns: per contact (x0, x2, x3, fx, fz) of its step, then slack, t_risk
      det                ``_pattern_maps`` of the deterministic rows on the core columns (value index = position in
                         ``nlp_layout()``'s det values; ent_of is n_c x n_c whatever M is)
      det_rows, det_cols_z   the deterministic pattern as coordinate lists in z numbering
      pos_det, pos_slip  where the two value arrays lie in the full pattern (the NumPy twin splits injected values with them)"""
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
    model._ipm_arrow = st
    return st


ArrowStructure = arrow_structure


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


class ArrowNumpyBackend:
    """The arrowhead step on the host: the same elimination as ``ArrowDeviceBackend``, from injected callbacks (or the Model's,
    one problem at a time).  ``callbacks[i]`` as for ``NumpyBackend``; of jac_values only the deterministic values and the slip
    partials dh/d(x0, x2, x3), dh/dfz are kept.  After ``factor``, ``parts[i]`` holds Shat (nc, nc) with ``arrow_terms``' pieces."""
    name, newton = "numpy", "arrow"

    def __init__(self, models, callbacks=None):
        self.models = models
        self.cb = [ModelCallbacks(m) for m in models] if callbacks is None else list(callbacks)
        self.st = arrow_structure(models[0])
        self.det, self.dx, self.dfz, self.hess, self.parts, self.L = {}, {}, {}, {}, {}, {}
        self.clock = dict(callbacks=0.0, normal=0.0, factor=0.0, solve=0.0)

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
        t0 = time.perf_counter()
        out = []
        for i, Z, lam, sf in zip(idx, Zs, lams, sfs):
            self.set_values(i, self.cb[i].jac_values(Z), self.cb[i].hess_blocks(Z, lam, sf))
            out.append(np.asarray(self.cb[i].g(Z), dtype=np.float64))
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

    def eval_g(self, idx, Zs):
        t0 = time.perf_counter()
        out = [np.asarray(self.cb[i].g(Z), dtype=np.float64) for i, Z in zip(idx, Zs)]
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

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
            t0 = time.perf_counter()
            Sh = normal_matrix_host(st["det"], self.det[i], d, self.hess[i], dg[st["core_z"]])
            P = arrow_terms(st, self.dx[i], self.dfz[i], d, dg[st["y0"]:st["y0"] + st["M"]], self._malpha(i))
            Sh[np.ix_(st["qcol"], st["qcol"])] += P["T"]
            P["Shat"] = Sh
            self.parts[i] = P
            t1 = time.perf_counter()
            ok = bool(np.all(np.isfinite(Sh))) and bool(np.all(P["e"] > 0.0))
            if ok:
                try:
                    self.L[i] = np.linalg.cholesky(Sh)
                except np.linalg.LinAlgError:
                    ok = False
            self.clock["normal"] += t1 - t0
            self.clock["factor"] += time.perf_counter() - t1
            info.append(0 if ok else 1)
        return info

    def solve(self, idx, B):
        from scipy.linalg import solve_triangular
        st = self.st
        t0 = time.perf_counter()
        out = []
        for i, b in zip(idx, B):
            P, L = self.parts[i], self.L[i]
            u = 1.0 / P["e"]
            einv = (lambda v: u * (v - P["k"] * (u @ v))) if st["saa"] else (lambda v: u * v)
            rc, ry = b[st["core_z"]].copy(), b[st["y0"]:st["y0"] + st["M"]]
            t = einv(ry)
            if st["saa"]:
                bt = P["Bq"].T @ t
                bt[-1] += P["beta"] * np.sum(t)
                rc[st["qcol"]] -= bt
            xc = solve_triangular(L, solve_triangular(L, rc, lower=True), lower=True, trans='T')
            if st["saa"]:
                ry = ry - (P["Bq"] @ xc[st["qcol"]] + P["beta"] * xc[-1])
            x = np.empty(st["n"])
            x[st["core_z"]] = xc
            x[st["y0"]:st["y0"] + st["M"]] = einv(ry)
            out.append(x)
        self.clock["solve"] += time.perf_counter() - t0
        return out


class ArrowDeviceBackend:
    """The arrowhead step on the MI355X for the problems of one group (csrc/hopper_arrow.hip on the partials rato_hopper_slip_f64
    leaves in HBM; the core through rato_normal_matrix_f64 on the deterministic pattern and the Cholesky of ``DeviceBackend``).
    eval_full keeps the partials: neither the slip CSC values nor the tril-packed Hessian are ever formed.  What travels to the
    host per call is the vectors the driver works on and O(q) sums."""
    name, newton = "device", "arrow"

    def __init__(self, models):
        import torch
        from . import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.models = models
        m0 = self.m0 = models[0]
        if any(m.precision != 'f64' for m in models):
            raise ValueError("the device backend needs Model(..., precision='f64')")
        self.dev = m0.device
        st = self.st = arrow_structure(m0)
        det, lay = st["det"], m0.nlp_layout()
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
        self.maps = dict(ent_of=up(det["ent_of"], np.int32), ptr=up(det["ptr"], np.int64), tri_a=up(det["tri_a"], np.int32),
                         tri_b=up(det["tri_b"], np.int32), tri_r=up(det["tri_r"], np.int32), hess_src=up(det["hess_src"], np.int32),
                         row_ptr=up(det["row_ptr"], np.int64), row_idx=up(det["row_idx"], np.int32),
                         row_col=up(st["core_z"][det["row_col"]], np.int32), col_ptr=up(st["det_indptr_z"], np.int64),
                         col_idx=up(np.arange(det["nnz"]), np.int32), col_row=up(st["det_rows"], np.int32),
                         qcol=up(st["qcol"], np.int32), map_defect=up(lay["map_defect"], np.int64),
                         map_rows=up(lay["map_rows"], np.int64), scale_rows=up(lay["scale_rows"], np.float64),
                         det_const=up(lay["det_const"], np.float64))
        self.params = _h.nlp_params(m0.S, m0.time_jump, m0.time_land, m0.dt)
        self.nch = int(self.lib.rato_hopper_arrow_nchunks(st["M"]))
        self.npart = int(self.lib.rato_hopper_arrow_npart(st["C"]))
        if self.nch < 1 or self.npart < 1:
            raise ValueError(f"newton='arrow' on the device serves 1 <= C <= 50 contact steps, got C = {st['C']}")
        self.slot = {}
        self.vals0 = self.dx = self.dfz = self.hessd = self.hess_host = None
        n_all = len(models)
        e = lambda *s: torch.empty(s, dtype=torch.float64, device=self.dev)
        self.L, self.e, self.d = e(n_all, st["nc"], st["nc"]), e(n_all, st["M"]), e(n_all, st["ncon"])
        self.kk, self.beta = np.zeros(n_all), np.zeros(n_all)
        self.clock = dict(callbacks=0.0, normal=0.0, factor=0.0, solve=0.0, reduction=0.0, assembly=0.0, products=0.0)

    def _sync(self):
        self.torch.cuda.synchronize(self.dev)

    def _up(self, rows):
        return self.torch.as_tensor(np.ascontiguousarray(np.stack(rows), dtype=np.float64), device=self.dev)

    def _empty(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.dev)

    def _malpha(self, idx):
        return np.array([self.st["M"] * float(self.models[i].alpha) for i in idx])

    def _g_rows(self, idx, Zs, lin, h):
        defect, rows = lin["defect"].cpu().numpy(), lin["rows"].cpu().numpy()
        slip = np.ascontiguousarray(h.cpu().numpy().transpose(0, 2, 1)).reshape(len(idx), -1)          # row order i C + c
        return [assemble_g(self.models[i], np.asarray(Z), defect[k], rows[k], slip[k]) for k, (i, Z) in enumerate(zip(idx, Zs))]

    def eval_full(self, idx, Zs, lams, sfs):
        t0 = time.perf_counter()
        m0, mp, K = self.m0, self.maps, len(idx)
        Zd, lamd = self._up(Zs), self._up(lams)
        lin = _h.nlp_linearize_device(self.params, Zd)
        jac = mp["det_const"][None].repeat(K, 1).contiguous()
        _h.scatter_f64(lin["d_defect"].view(K, -1), mp["map_defect"], jac)
        _h.scatter_f64(lin["d_rows"].view(K, -1), mp["map_rows"], jac, mp["scale_rows"])
        slip = m0.slip_device_f64(Zd, lamd, want=("h", "dh_dfz", "dh_dx"))
        add = self._up([_obj_add(m0, sf) for sf in sfs])
        m0.slip_hess_blocks_device_f64(Zd, slip["D"], add)
        lam_dyn, lam_rows = m0.fold_multipliers(np.stack(lams))
        self.hessd = _h.nlp_hessian_device(self.params, Zd, self._up(list(lam_dyn)), self._up(list(lam_rows)), add)
        self.vals0, self.dx, self.dfz = jac, slip["dh_dx"], slip["dh_dfz"]
        self.slot = {i: k for k, i in enumerate(idx)}
        self.hess_host = self.hessd.cpu().numpy()
        out = self._g_rows(idx, Zs, lin, slip["h"])
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

    def eval_g(self, idx, Zs):
        t0 = time.perf_counter()
        Zd = self._up(Zs)
        lin = _h.nlp_linearize_device(self.params, Zd, want=("defect", "rows"))
        out = self._g_rows(idx, Zs, lin, self.m0.slip_device_f64(Zd, want=("h",))["h"])
        self.clock["callbacks"] += time.perf_counter() - t0
        return out

    def hess_apply(self, idx, X):
        return [_hess_apply(self.st["hess"], self.hess_host[self.slot[i]], x) for i, x in zip(idx, X)]

    def _sel(self, idx):
        rows = [self.slot[i] for i in idx]
        if rows == list(range(self.vals0.shape[0])):
            return self.vals0, self.dx, self.dfz, self.hessd
        sel = self.torch.as_tensor(rows, device=self.dev)
        return tuple(t.index_select(0, sel).contiguous() for t in (self.vals0, self.dx, self.dfz, self.hessd))

    def _call(self, name, *args):
        with self.torch.cuda.device(self.dev):
            self._lib.check(getattr(self.lib, name)(*args, self._lib.current_stream()), name)

    def _det_matvec(self, name, v0, x, n_out, ptr, lidx, other):
        st, p = self.st, self._lib.ptr
        K = x.shape[0]
        out = self._empty(K, n_out)
        self._call(name, K, st["ncon"], st["n"], p(v0), v0.shape[1], v0.shape[1], None, 0, 0, p(self.maps[ptr]),
                   p(self.maps[lidx]), p(self.maps[other]), p(x), x.shape[1], p(out), n_out)
        return out

    def matvec(self, idx, X):
        t0 = time.perf_counter()
        st, p = self.st, self._lib.ptr
        M, Cn, K = st["M"], st["C"], len(idx)
        v0, dx, dfz, _ = self._sel(idx)
        xh = np.stack(X)
        x = self._up(X)
        out = self._det_matvec("rato_csc_matvec_f64", v0, x, st["ncon"], "row_ptr", "row_idx", "row_col")
        xq, xy = self._up(list(xh[:, st["qz"]])), x[:, st["y0"]:st["y0"] + M].contiguous()
        part, red = self._empty(self.nch, K), self._empty(K)
        self._call("rato_hopper_arrow_rows_f64", K, M, Cn, int(st["saa"]), 0, p(dx), p(dfz), p(xq), p(xy), None, 0, st["r0"], None,
                   p(out), st["ncon"], p(part), p(red))
        o = out.cpu().numpy()
        if st["saa"]:
            o[:, st["rr"]] = self._malpha(idx) * xh[:, st["n"] - 1] + red.cpu().numpy()
        self.clock["products"] += time.perf_counter() - t0
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
        t0 = time.perf_counter()
        st = self.st
        M, Cn, K = st["M"], st["C"], len(idx)
        v0, dx, dfz, _ = self._sel(idx)
        wh = np.stack(W)
        w = self._up(W)
        out = self._det_matvec("rato_csc_tmatvec_f64", v0, w, st["n"], "col_ptr", "col_idx", "col_row")
        yout = self._empty(K, M)
        red = self._cols(0, dx, dfz, w, None, yout)
        o = out.cpu().numpy()
        tot = self._minus_fx_total(red)
        o[:, st["qz"][:5 * Cn]] += red[:, :5 * Cn]
        o[:, st["n"] - 2] += tot
        if st["saa"]:
            o[:, st["n"] - 1] += self._malpha(idx) * wh[:, st["rr"]] + tot
            o[:, st["y0"]:st["y0"] + M] = yout.cpu().numpy()
        self.clock["products"] += time.perf_counter() - t0
        return list(o)

    def schur(self, idx, D, diags, out=None):
        """-> (Shat (K, nc, lda) device tensor, lower triangle; e (K, M) and d (K, ncon) device; red (K, n_part) and d on the
        host): the core's Schur complement of the listed problems (``out``: a contiguous (K, nc, lda >= nc) tensor to write into)"""
        st, torch, mp, p = self.st, self.torch, self.maps, self._lib.ptr
        M, Cn, nc, K = st["M"], st["C"], st["nc"], len(idx)
        v0, dx, dfz, hs = self._sel(idx)
        dh = np.stack(D)
        d, dgh = self._up(D), np.stack(diags)
        dg, yd = self._up(list(dgh[:, st["core_z"]])), self._up(list(dgh[:, st["y0"]:st["y0"] + M]))
        Sh = self._empty(K, nc, nc) if out is None else out
        if tuple(Sh.shape[:2]) != (K, nc) or Sh.shape[2] < nc or Sh.dtype != torch.float64 or not Sh.is_contiguous():
            raise ValueError(f"out must be a contiguous device float64 tensor ({K}, {nc}, >= {nc})")
        t0 = time.perf_counter()
        self._call("rato_normal_matrix_f64", K, nc, Sh.shape[2], p(v0), v0.shape[1], v0.shape[1], None, 0, 0, p(d), st["ncon"], p(hs),
                   hs.shape[1] * hs.shape[2], p(dg), p(mp["ent_of"]), p(mp["ptr"]), p(mp["tri_a"]), p(mp["tri_b"]), p(mp["tri_r"]),
                   p(mp["hess_src"]), p(Sh))
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
        info = chol_factor(Sh).cpu().numpy()
        sel = torch.as_tensor(list(idx), device=self.dev)
        self.L[sel], self.e[sel], self.d[sel] = Sh, e, d
        if st["saa"]:
            q = st["q"]
            s = red[:, q * (q + 1) // 2 + 2 * q]
            d0 = dh[:, st["rr"]]
            self.kk[list(idx)] = d0 / (1.0 + d0 * s)
            self.beta[list(idx)] = d0 * self._malpha(idx)
        self.clock["factor"] += time.perf_counter() - t1
        return [int(v) for v in info]

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
        t0 = time.perf_counter()
        st, p = self.st, self._lib.ptr
        M, Cn, K, q = st["M"], st["C"], len(idx), st["q"]
        rows = [self.slot[i] for i in idx]
        sel = self.torch.as_tensor(list(idx), device=self.dev)
        ssel = self.torch.as_tensor(rows, device=self.dev)
        L, e, d = (t.index_select(0, sel) for t in (self.L, self.e, self.d))
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
        xc = self._up(list(rc))[:, None, :].contiguous()
        chol_solve(L, xc)
        xch = xc[:, 0].cpu().numpy()
        if st["saa"]:
            rem = self._empty(K, M)                                    # r_y - B x_c
            xq, addc = self._up(list(xch[:, st["qcol"]])), self._up([beta * xch[:, -1]])[0].contiguous()
            self._call("rato_hopper_arrow_rows_f64", K, M, Cn, 1, 1, p(dx), p(dfz), p(xq), p(ry), p(d), st["ncon"], st["r0"], p(addc),
                       p(rem), M, None, None)
            ry = rem
        ry = self._einv(e, ry, kk)
        out = np.empty((K, st["n"]))
        out[:, st["core_z"]] = xch
        out[:, st["y0"]:st["y0"] + M] = ry.cpu().numpy()
        self.clock["solve"] += time.perf_counter() - t0
        return list(out)


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


def _solve_group(models, Z0s, tol, max_iter, be, verbose):
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
            print("it %4d " % it + " | ".join("mu %.1e E0 %.2e pr %.1e du %.1e a %.1e dw %.0e" %
                                               (p.mu, p.E0, p.prim, p.dual, getattr(p, "alpha", 0.0), p.dw) for p in act))
    out = []
    for p in ps:
        if p.status is None:
            p.status = "max_iter"
        info = dict(status=p.status, iterations=p.iterations, factorizations=p.factorizations, E0=float(p.E0),
                    primal_infeasibility=float(p.prim), dual_infeasibility=float(p.dual), f=p.model.f(p.z), mu=p.mu, sf=p.sf,
                    y=p.y.copy(), zl=p.zl.copy(), zu=p.zu.copy(), s=p.v[p.n:].copy(), backend=be.name)
        out.append((p.z.copy(), info))
    return out


def _group_key(m):
    f = tuple(np.asarray(x).tobytes() for x in (getattr(m, "intensities", None), getattr(m, "thetas", None), getattr(m, "taus", None))
              if x is not None) or (id(m),)
    return (m.method, m.S, m.M, m.time_jump, m.time_land, f)


def solve_batch(models, Z0s=None, tol=1e-3, max_iter=3000, backend='device', callbacks=None, verbose=False, clocks=None,
                newton='dense'):
    """Solve the models' NLPs in lockstep -> list of (Z, info), in the models' order.  The K problems share S, M and the phases;
    problems of one method and one set of friction fields (alpha may differ) form a group that moves through the K-problem
    kernels together, the groups one after the other.  A problem that has ended stops changing and leaves the launches; its Z is
    bitwise what its own K = 1 run returns.
      Z0s        starting points (default: ``model.initial_guess()``)
      backend    'device' (csrc/hopper_ipm.hip) or 'numpy' (the step on the host)
      callbacks  backend='numpy' only: one object per model with g(Z), jac_values(Z), hess_blocks(Z, lam, obj_factor)
      clocks     a dict that receives the seconds spent in callbacks / normal / factor / solve and the wall clock
      newton     'dense': the condensed matrix over all n = 8(S+1) + 4S + M + 2 variables (the default; n^2 memory, right at the
                 script's M = 30); 'arrow': the M sample variables ys are eliminated exactly and the 8(S+1) + 4S + 2 core is
                 factored (``ArrowDeviceBackend`` / ``ArrowNumpyBackend``): memory and work are O(M C), for any M
    info: status ('converged' | 'max_iter' | 'line_search'), iterations, factorizations, E0, primal_infeasibility,
    dual_infeasibility, f, and the final multipliers y, zl, zu with the slacks s and the objective scale sf."""
    if backend not in ('device', 'numpy'):
        raise ValueError(f"backend must be 'device' or 'numpy', got {backend!r}")
    if newton not in ('dense', 'arrow'):
        raise ValueError(f"newton must be 'dense' or 'arrow', got {newton!r}")
    if callbacks is not None and backend != 'numpy':
        raise ValueError("callbacks are the numpy backend's")
    models = list(models)
    Z0s = [m.initial_guess() for m in models] if Z0s is None else [np.asarray(Z, dtype=np.float64) for Z in Z0s]
    if len(Z0s) != len(models) or any(Z.shape != (m.num_vars,) for Z, m in zip(Z0s, models)):
        raise ValueError("Z0s must hold one (num_vars,) vector per model")
    if len({(m.S, m.M, m.time_jump, m.time_land) for m in models}) > 1:
        raise ValueError("the problems of a batch share S, M and the phases")
    groups = {}
    for i, m in enumerate(models):
        groups.setdefault(_group_key(m), []).append(i)
    out = [None] * len(models)
    t0 = time.perf_counter()
    for members in groups.values():
        ms = [models[i] for i in members]
        cbs = None if callbacks is None else [callbacks[i] for i in members]
        if newton == 'arrow':
            be = ArrowDeviceBackend(ms) if backend == 'device' else ArrowNumpyBackend(ms, cbs)
        else:
            be = DeviceBackend(ms) if backend == 'device' else NumpyBackend(ms, cbs)
        for i, r in zip(members, _solve_group(ms, [Z0s[i] for i in members], tol, max_iter, be, verbose)):
            out[i] = r
        if clocks is not None:
            for k, v in be.clock.items():
                clocks[k] = clocks.get(k, 0.0) + v
    if clocks is not None:
        clocks["wall"] = clocks.get("wall", 0.0) + time.perf_counter() - t0
    return out
