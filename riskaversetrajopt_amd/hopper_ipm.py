"""The hopper NLP (hopper/hopper.py:486-669: what the script hands to IPOPT, ``hopper.Model.ipopt_callbacks()``) by the batched
interior-point method of ``ipm``: the fixed sparse structure of its Newton step and the two backends that do it.
(Relaxing the bounds outward makes the constant row ``0 <= 0`` of the SAA group harmless; delta_c tolerates the script's
redundant rows.)

'device' works with csrc/hopper_ipm.hip and csrc/chol.hip on the values ``Model.nlp_device`` leaves in HBM, K problems per
launch; 'numpy' does the whole step on the host, callbacks injected or taken one problem at a time from the Model.  The three
kernels of csrc/hopper_ipm.hip are bound once, as ``normal_matrix``, ``csc_matvec`` and ``csc_tmatvec`` on device tensors (with
``upload_maps`` for their index lists): both hopper device backends, on lists and on tensors, are adapters over them, and
``ipm.Backend`` / ``ipm.DeviceBase`` supply factor and solve.  Neither backend evaluates the NLP itself: ``HopperDeviceBase``
holds what they share (the models, ``GroupFields``, M alpha per problem, g and W x on either driver) over the stages of
``hopper.Model``, and ``DeviceBackend`` / ``hopper_arrow.ArrowDeviceBackend`` add the slip outputs they keep, their products and
their matrix.

driver='device' (``ipm.solve_group_device``) keeps the iterate in HBM: the device backend then serves device
tensors (eval_full_t ... normal_matrix_t below), g is assembled by rato_hopper_g_f64, W x is rato_hopper_block_symv_f64 and the
multipliers are folded by rato_scatter_f64 (csrc/hopper_g.hip, ``Model.fold_multipliers_device``, as under the host driver);
nothing but the scalar record and the factorization's info comes back during an iteration.  Both Newton steps are served: the
arrow backend's host-side fix-ups are the ``arrow_*`` bindings below.

newton='arrow' (``hopper_arrow``) is the same step for any M: the M variables ys are eliminated exactly and the
Cholesky factors the core's Schur complement; newton='dense' (the default) is the step over all variables.
"""
import numpy as np
import torch

from . import _lib
from . import hopper as _h
from . import ipm as _ipm


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
    """sf hess_f as step blocks (S+1, 78): ``hopper.objective_blocks``"""
    return _h.objective_blocks(model.S, sf)


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


class NumpyBackend(_ipm.Backend):
    """the whole step on the host.  ``callbacks[i]`` serves models[i]: g(Z) (ncon,), jac_values(Z) (nnz,) on the full CSC
    pattern, hess_blocks(Z, lam, obj_factor) (S+1, 78)"""
    name = "numpy"

    def __init__(self, models, callbacks=None):
        self.models = models
        self.cb = [ModelCallbacks(m) for m in models] if callbacks is None else list(callbacks)
        super().__init__()
        self.st = structure(models[0])
        self.vals, self.hess = {}, {}

    def eval_full(self, idx, Zs, lams, sfs):
        with self.timed("callbacks"):
            out = []
            for i, Z, lam, sf in zip(idx, Zs, lams, sfs):
                self.vals[i] = np.asarray(self.cb[i].jac_values(Z), dtype=np.float64)
                self.hess[i] = np.asarray(self.cb[i].hess_blocks(Z, lam, sf), dtype=np.float64)
                out.append(np.asarray(self.cb[i].g(Z), dtype=np.float64))
        return out

    def eval_g(self, idx, Zs):
        with self.timed("callbacks"):
            return [np.asarray(self.cb[i].g(Z), dtype=np.float64) for i, Z in zip(idx, Zs)]

    def hess_apply(self, idx, X):
        return [_hess_apply(self.st, self.hess[i], x) for i, x in zip(idx, X)]

    def matvec(self, idx, X):
        st = self.st
        return [np.bincount(st["rows"], weights=self.vals[i] * x[st["cols"]], minlength=st["ncon"]) for i, x in zip(idx, X)]

    def tmatvec(self, idx, W):
        st = self.st
        return [np.bincount(st["cols"], weights=self.vals[i] * w[st["rows"]], minlength=st["n"]) for i, w in zip(idx, W)]

    def normal_matrix_host(self, i, d, diag):
        return normal_matrix_host(self.st, self.vals[i], d, self.hess[i], diag)


assemble_g = _h.Model.assemble_g     # (model, Z, defect, rows, slip_rows) -> g of one problem on the host; ``Model.g`` calls the same


# ---- the kernels of csrc/hopper_ipm.hip on device fp64 tensors: each entry point is called here and nowhere else ----------------
def upload_maps(pm, dev, to_value=None, to_col=None, col_ptr=None):
    """the index lists of a ``_pattern_maps`` dict as the device tensors the three kernels read.  ``to_value`` translates the
    pattern's value index into the index in the value arrays (None: the same), ``to_col`` the pattern's column into the column
    of x (None: the same), and ``col_ptr`` is the column list's pointer over the columns of J'w (None: the pattern's indptr)."""
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    val = (lambda a: a) if to_value is None else (lambda a: to_value[a])
    return dict(ent_of=up(pm["ent_of"], np.int32), ptr=up(pm["ptr"], np.int64), tri_a=up(val(pm["tri_a"]), np.int32),
                tri_b=up(val(pm["tri_b"]), np.int32), tri_r=up(pm["tri_r"], np.int32), hess_src=up(pm["hess_src"], np.int32),
                row_ptr=up(pm["row_ptr"], np.int64), row_idx=up(val(pm["row_idx"]), np.int32),
                row_col=up(pm["row_col"] if to_col is None else to_col[pm["row_col"]], np.int32),
                col_ptr=up(pm["indptr"] if col_ptr is None else col_ptr, np.int64),
                col_idx=up(val(np.arange(pm["nnz"])), np.int32), col_row=up(pm["rows"], np.int32))


def _bad(t, K, ld):
    return t.dim() != 2 or t.shape[0] != K or t.shape[1] < ld or t.dtype != torch.float64 or not t.is_contiguous()


def _values(v0, v1):
    """the value arrays as the kernels take them: pointer, ld and count of the deterministic rows' values v0 (K, n_det) and of
    the slip rows' v1 (K, n_slip); v1 None: the arrow backend's deterministic block alone"""
    if v1 is None:
        return _lib.ptr(v0), v0.shape[1], v0.shape[1], None, 0, 0
    return _lib.ptr(v0), v0.shape[1], v0.shape[1], _lib.ptr(v1), v1.shape[1], v1.shape[1]


def _csc(name, st, maps, lists, v0, v1, x, n_in, n_out):
    K = v0.shape[0]
    if _bad(x, K, n_in):
        raise ValueError(f"{name}: the vector must be a contiguous device float64 tensor ({K}, >= {n_in})")
    if v1 is not None and (v0.shape[1] != st["n_det"] or v1.shape != (K, st["n_slip"])):
        raise ValueError(f"{name}: the values must be ({K}, {st['n_det']}) and ({K}, {st['n_slip']})")
    out = torch.empty((K, n_out), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.load(), name)(K, st["ncon"], st["n"], *_values(v0, v1), _lib.ptr(maps[lists[0]]),
                                              _lib.ptr(maps[lists[1]]), _lib.ptr(maps[lists[2]]), _lib.ptr(x), x.shape[1],
                                              _lib.ptr(out), n_out, _lib.current_stream()), name)
    return out


def csc_matvec(st, maps, v0, v1, x):
    """rato_csc_matvec_f64: x (K, ld >= n) -> J x (K, ncon), J's values in v0 and v1 as ``_values`` takes them"""
    return _csc("rato_csc_matvec_f64", st, maps, ("row_ptr", "row_idx", "row_col"), v0, v1, x, st["n"], st["ncon"])


def csc_tmatvec(st, maps, v0, v1, w):
    """rato_csc_tmatvec_f64: w (K, ld >= ncon) -> J' w (K, n)"""
    return _csc("rato_csc_tmatvec_f64", st, maps, ("col_ptr", "col_idx", "col_row"), v0, v1, w, st["ncon"], st["n"])


def normal_matrix(n, ncon, maps, v0, v1, d, hess, diag, out=None):
    """rato_normal_matrix_f64: values as ``_values`` takes them, d (K, ldd >= ncon), hess (K, S+1, 78) step blocks or None, diag
    (K, n) or None -> Kc (K, n, lda), lower triangle (``out``: a contiguous (K, n, lda >= n) tensor to write into)"""
    K = v0.shape[0]
    if _bad(d, K, ncon) or (diag is not None and (_bad(diag, K, n) or diag.shape[1] != n)):
        raise ValueError(f"d must be a contiguous device float64 tensor ({K}, >= {ncon}) and diag ({K}, {n})")
    if hess is not None and (hess.dim() != 3 or hess.shape[0] != K or hess.dtype != torch.float64 or not hess.is_contiguous()):
        raise ValueError(f"hess must be a contiguous device float64 tensor ({K}, S + 1, 78)")
    Kc = torch.empty((K, n, n), dtype=torch.float64, device=d.device) if out is None else out
    if tuple(Kc.shape[:2]) != (K, n) or Kc.shape[2] < n or Kc.dtype != torch.float64 or not Kc.is_contiguous():
        raise ValueError(f"out must be a contiguous device float64 tensor ({K}, {n}, >= {n})")
    with torch.cuda.device(d.device):
        _lib.check(_lib.load().rato_normal_matrix_f64(
            K, n, Kc.shape[2], *_values(v0, v1), _lib.ptr(d), d.shape[1], _lib.ptr(hess),
            0 if hess is None else hess.shape[1] * hess.shape[2], _lib.ptr(diag), _lib.ptr(maps["ent_of"]), _lib.ptr(maps["ptr"]),
            _lib.ptr(maps["tri_a"]), _lib.ptr(maps["tri_b"]), _lib.ptr(maps["tri_r"]), _lib.ptr(maps["hess_src"]), _lib.ptr(Kc),
            _lib.current_stream()), "rato_normal_matrix_f64")
    return Kc


# ---- the fix-up kernels of csrc/hopper_arrow.hip on device fp64 tensors (``hopper_arrow.ArrowDeviceBackend`` on tensors): a 2-D
# argument is (K, >= cols) with contiguous rows -- a column range of a wider tensor is fine, its row stride is the ld
def _rows_ld(t, K, cols, name, dtype=torch.float64):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != K or t.shape[1] < cols or t.dtype != dtype or not t.is_cuda \
            or t.stride(1) != 1 or (K > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name} must be a device {str(dtype).split('.')[-1]} tensor ({K}, >= {cols}) with contiguous rows")
    return t.stride(0) if K > 1 else max(t.stride(0), t.shape[1])


def _per_problem(K, **tensors):
    for name, t in tensors.items():
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (K,) or t.dtype != torch.float64 or not t.is_cuda
                              or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous device float64 tensor ({K},)")


def _index_list(t, length, name, dtype=torch.int32):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] < length or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous device {str(dtype).split('.')[-1]} tensor (>= {length},)")


def _launch(dev, name, *args):
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), name)(*args, _lib.current_stream()), name)


def scatter_rows(src, n, index_map, dst, n_dst):
    """rato_scatter_f64 between padded tensors: dst[k][map[i]] = src[k][i] for i < n; map (n,) device int64, an entry outside
    [0, n_dst) is not emitted (a gather takes the inverse map, -1 where a column has no target).  What the map does not point at
    is left alone."""
    K = src.shape[0]
    ld_src, ld_dst = _rows_ld(src, K, n, "src"), _rows_ld(dst, K, n_dst, "dst")
    _index_list(index_map, n, "map", torch.int64)
    if index_map.shape[0] != n:
        raise ValueError(f"map must hold {n} entries")
    _launch(src.device, "rato_scatter_f64", K, n, _lib.ptr(src), ld_src, _lib.ptr(index_map), None, _lib.ptr(dst), ld_dst, n_dst)
    return dst


def arrow_scale(a, x, col, add, out, ocol):
    """rato_hopper_arrow_scale_f64: out[k][ocol] = a[k] x[k][col] (+ add[k]); out 1-D (K,): out[k]"""
    K = a.shape[0]
    _per_problem(K, a=a, add=add)
    o2 = out[:, None] if out.dim() == 1 else out
    ldx, ldo = _rows_ld(x, K, col + 1, "x"), _rows_ld(o2, K, ocol + 1, "out")
    if col < 0 or ocol < 0:
        raise ValueError("col and ocol must not be negative")
    _launch(x.device, "rato_hopper_arrow_scale_f64", K, _lib.ptr(a), _lib.ptr(x), ldx, col, _lib.ptr(add), _lib.ptr(o2), ldo, ocol)
    return out


def arrow_tfix(M, Cn, saa, n, qz, red, malpha, w, rr, yout, out):
    """rato_hopper_arrow_tfix_f64: finishes J' w (K, >= n) in z numbering from the red (K, >= 5C + 1) and yout (K, M) of cols mode 0"""
    K = out.shape[0]
    ldo, ldr = _rows_ld(out, K, n, "out"), _rows_ld(red, K, 5 * Cn + 1, "red")
    _index_list(qz, 5 * Cn, "qz")
    ldw = 0
    if saa:
        ldw = _rows_ld(w, K, rr + 1, "w")
        _per_problem(K, malpha=malpha)
        if malpha is None or _rows_ld(yout, K, M, "yout") != M:
            raise ValueError(f"saa: malpha ({K},) and a contiguous yout ({K}, {M})")
    _launch(out.device, "rato_hopper_arrow_tfix_f64", K, M, Cn, int(bool(saa)), n, _lib.ptr(qz), _lib.ptr(red), ldr,
            _lib.ptr(malpha if saa else None), _lib.ptr(w if saa else None), ldw, rr if saa else 0, _lib.ptr(yout if saa else None),
            _lib.ptr(out), ldo)
    return out


def arrow_kkbeta(Cn, d, rr, red, malpha, kk, beta):
    """rato_hopper_arrow_kkbeta_f64: kk = d0 / (1 + d0 s), beta = d0 malpha from d (K, > rr) and the red (K, >= n_part) of reduce"""
    K = d.shape[0]
    _per_problem(K, malpha=malpha, kk=kk, beta=beta)
    q = 5 * Cn + 2
    ldd, ldr = _rows_ld(d, K, rr + 1, "d"), _rows_ld(red, K, q * (q + 1) // 2 + 2 * q + 1 + 15 * Cn, "red")
    _launch(d.device, "rato_hopper_arrow_kkbeta_f64", K, Cn, _lib.ptr(d), ldd, rr, _lib.ptr(red), ldr, _lib.ptr(malpha), _lib.ptr(kk),
            _lib.ptr(beta))


def arrow_einv(e, v, kk, red, out):
    """rato_hopper_arrow_einv_f64: out = (1 / e) o (v - kk red) for e (K, M) contiguous, v and out (K, >= M), kk and red (K,) (both
    None: (1 / e) o v, the baseline's)"""
    K, M = e.shape
    if _rows_ld(e, K, M, "e") != M:
        raise ValueError(f"e must be a contiguous device float64 tensor ({K}, {M})")
    _per_problem(K, kk=kk, red=red)
    if (kk is None) != (red is None):
        raise ValueError("kk and red come together")
    ldv, ldo = _rows_ld(v, K, M, "v"), _rows_ld(out, K, M, "out")
    _launch(e.device, "rato_hopper_arrow_einv_f64", K, M, _lib.ptr(e), _lib.ptr(v), ldv, _lib.ptr(kk), _lib.ptr(red), _lib.ptr(out), ldo)
    return out


def arrow_rhsfix(Cn, nc, qcol, red, beta, rc):
    """rato_hopper_arrow_rhsfix_f64: rc (K, >= nc, core numbering) -= B' t from the red (K, >= 5C + 1) of cols mode 1"""
    K = rc.shape[0]
    _per_problem(K, beta=beta)
    _index_list(qcol, 5 * Cn, "qcol")
    ldrc, ldr = _rows_ld(rc, K, nc, "rc"), _rows_ld(red, K, 5 * Cn + 1, "red")
    _launch(rc.device, "rato_hopper_arrow_rhsfix_f64", K, Cn, nc, _lib.ptr(qcol), _lib.ptr(red), ldr, _lib.ptr(beta), _lib.ptr(rc), ldrc)
    return rc


def _fields_key(m):
    """what tells one set of friction fields from another: the bytes of the host arrays, or the device arrays' addresses"""
    host = tuple(getattr(m, name, None) for name in ("intensities", "thetas", "taus"))
    if all(x is not None for x in host):
        return tuple(np.asarray(x).tobytes() for x in host)
    return tuple(t.data_ptr() for t in (m._a, m._th, m._tau))


class GroupFields:
    """The friction fields of a group's models for the slip kernel.  Models that share one set keep the shared call (``of`` gives
    None: models[0]'s fields serve every problem, as before fields per problem existed).  Otherwise the fields are stacked once
    as (a, theta, tau), each (K, 30, M) (``hopper.stack_fields_f64``: K x 3 x 30 x M x 8 bytes), and ``of(idx)`` gives the rows of
    the listed problems: the whole stack in place when they are all of them in order, a gathered copy when some have left."""

    def __init__(self, models):
        self.K = len(models)
        key0 = _fields_key(models[0])
        self.stack = None if all(_fields_key(m) == key0 for m in models[1:]) else _h.stack_fields_f64(models)

    def of(self, idx=None):
        if self.stack is None:
            return None
        if idx is None or list(idx) == list(range(self.K)):
            return self.stack
        sel = torch.as_tensor(list(idx), device=self.stack[0].device)
        return tuple(t.index_select(0, sel) for t in self.stack)


class HopperDeviceBase(_ipm.DeviceBase):
    """What the hopper's two backends on the device share, for the problems of one group (same S, M, phases and method; alpha
    and the friction fields may differ: models that do not share one set of fields are served from a stack of theirs,
    ``GroupFields``): the models, M alpha per problem on the device, g on either driver from the stages of ``hopper.Model``, and
    W x.  A subclass sets ``st`` and ``hess_st`` (the ``block_vars`` and n that ``_hess_apply`` reads) and defines
    ``_evaluate(Z, Y, add, idx)`` on device tensors -- the call sequence over the Model's stages that leaves ``hessd`` and the
    slip outputs it keeps, for the listed problems (None: the whole group), and returns (defect, rows, slip_h) -- then its
    products and its matrix."""
    name = "device"

    def __init__(self, models, *more_clocks, chol='workgroup'):
        self.models = models
        m0 = self.m0 = models[0]
        if any(m.precision != 'f64' for m in models):
            raise ValueError("the device backend needs Model(..., precision='f64')")
        super().__init__(m0.device, len(models), *more_clocks, chol=chol)
        lay = m0.nlp_layout()
        self.Cn, self.saa = lay["C"], m0.method != 'baseline'
        # M alpha per problem, uploaded once: the sum row of g and the one Jacobian value that depends on alpha (row 0 of the
        # t_risk column, at ``alpha_pos`` of the slip CSC values; -1 where there is none)
        self.malpha = torch.as_tensor([m0.M * float(m.alpha) for m in models], dtype=torch.float64, device=self.dev)
        self.alpha_pos = int(lay["nnz_slip"] - 1 - m0.M * lay["C"]) if self.saa and lay["C"] > 0 else -1
        self.fields = GroupFields(models)
        self.hessd = self.hess_host = None

    def eval_full(self, idx, Zs, lams, sfs):
        with self.timed("callbacks"):
            parts = self._evaluate(self._up(Zs), self._up(lams), self._up([_obj_add(self.m0, sf) for sf in sfs]), idx)
            self.slot = {i: k for k, i in enumerate(idx)}
            self.hess_host = self.hessd.cpu().numpy()
            return self._g_rows(idx, Zs, *parts)

    def _g_rows(self, idx, Zs, defect, rows, slip_h):
        """g of the listed problems as host vectors, from the device tensors defect (K, S, 8), rows (K, S+1, 2) and the slip
        values h (K, C, M), ordered i C + c here on the host"""
        defect, rows = defect.cpu().numpy(), rows.cpu().numpy()
        slip = np.ascontiguousarray(slip_h.cpu().numpy().transpose(0, 2, 1)).reshape(len(idx), self.m0.M * self.Cn)
        return [assemble_g(self.models[i], np.asarray(Z), defect[k], rows[k], slip[k]) for k, (i, Z) in enumerate(zip(idx, Zs))]

    def eval_g(self, idx, Zs):
        with self.timed("callbacks"):
            r = self.m0.g_values_device(self._up(Zs), self.fields.of(idx))
            return self._g_rows(idx, Zs, r["defect"], r["rows"], r["slip_h"])

    def hess_apply(self, idx, X):
        return [_hess_apply(self.hess_st, self.hess_host[self.slot[i]], x) for i, x in zip(idx, X)]

    # ---- the same on device tensors, for ``ipm.solve_group_device``: the whole group, nothing waits or moves to the host
    def eval_full_t(self, Z, Y, add=None):
        """Z (K, n) and the multipliers Y (K, ld >= ncon), read where they lie -> g (K, ncon); leaves what the subclass keeps of
        the evaluation and the step blocks of hess(Y . g) for its other calls.  The objective's curvature is NOT in the blocks:
        the driver's diagonal carries it."""
        parts = self._evaluate(Z, Y, add, None)
        self.slot = {i: i for i in range(Z.shape[0])}
        return self._g_t(Z, *parts)

    def _g_t(self, Z, defect, rows, slip_h):
        m0 = self.m0
        return _h.g_device(m0._slip_params(), m0.M, self.saa, Z, defect, rows, slip_h if self.Cn > 0 else None, (1, m0.M), self.malpha)

    def eval_g_t(self, Z):
        r = self.m0.g_values_device(Z, self.fields.of())
        return self._g_t(Z, r["defect"], r["rows"], r["slip_h"])

    def hess_apply_t(self, X):
        """W x of the constraints' part alone (K, n): the objective's sf curv x is added where the result is used
        (csrc/ipm_driver.hip)"""
        return _h.block_symv(self.m0.S, self.hessd, X, self.st["n"])


class DeviceBackend(HopperDeviceBase):
    """the dense step on the MI355X: the slip CSC values are kept next to the deterministic rows', and the normal matrix is
    J' D J + W over all variables.  Every call serves the listed problems in ONE launch each; nothing a kernel computes for a
    problem depends on the others."""

    def __init__(self, models, chol='workgroup'):
        super().__init__(models, chol=chol)
        st = self.st = self.hess_st = structure(self.m0)
        self.maps = upload_maps(st, self.dev, to_value=st["to_cat"])
        self.vals0 = self.vals1 = None

    def _evaluate(self, Z, Y, add, idx):
        """``nlp_device`` on device tensors for the listed problems (None: the whole group): keeps both value arrays, with M alpha
        patched in per problem, and the step blocks -> (defect, rows, slip_h), what g is assembled from"""
        r = self.m0.nlp_device(Z, Y, add=add, fold='device', fields=self.fields.of(idx))
        self.vals0, self.vals1, self.hessd = r["jac_values"], r["slip_jac_values"], r["hess_blocks"]
        if self.alpha_pos >= 0:
            self.vals1[:, self.alpha_pos] = self.malpha if idx is None else self.malpha[list(idx)]
        return r["defect"], r["rows"], r["slip_h"]

    def set_values(self, vals, hess):
        """install given Jacobian values (K, nnz) on the full CSC pattern and step blocks (K, S+1, 78) as the current
        evaluation of problems 0 .. K-1 (what eval_full leaves), split into the two arrays the kernels read"""
        lay = self.m0.nlp_layout()
        vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
        self.vals0, self.vals1 = self._up(vals[:, lay["pos_det"]]), self._up(vals[:, lay["pos_slip"]])
        self.hess_host = np.ascontiguousarray(hess, dtype=np.float64)
        self.hessd = self._up(self.hess_host)
        self.slot = {i: i for i in range(vals.shape[0])}

    def _sel(self, idx):
        return self._rows(idx, self.vals0, self.vals1, self.hessd)

    def matvec(self, idx, X):
        v0, v1, _ = self._sel(idx)
        return list(csc_matvec(self.st, self.maps, v0, v1, self._up(X)).cpu().numpy())

    def tmatvec(self, idx, W):
        v0, v1, _ = self._sel(idx)
        return list(csc_tmatvec(self.st, self.maps, v0, v1, self._up(W)).cpu().numpy())

    def normal_matrix(self, idx, D, diags, with_hess=True, out=None):
        """-> Kc (K, n, lda) device tensor (lower triangle; ``out``: a contiguous (K, n, lda >= n) tensor to write into)"""
        v0, v1, hs = self._sel(idx)
        d, dg = self._up(D), (self._up(diags) if diags is not None else None)
        return normal_matrix(self.st["n"], self.st["ncon"], self.maps, v0, v1, d, hs if with_hess else None, dg, out=out)

    # ---- the same on device tensors, for ``ipm.solve_group_device``: every call serves the whole group, takes and returns
    # (K, ld) tensors, waits for nothing and moves nothing to the host.  ``factor_t`` and ``solve_t`` are DeviceBase's, the
    # evaluation and W x HopperDeviceBase's.
    def matvec_t(self, X):
        """X (K, ld >= n) -> J x (K, ncon)"""
        return csc_matvec(self.st, self.maps, self.vals0, self.vals1, X)

    def tmatvec_t(self, W):
        """W (K, ld >= ncon) -> J' w (K, n)"""
        return csc_tmatvec(self.st, self.maps, self.vals0, self.vals1, W)

    def normal_matrix_t(self, d, diag, out=None):
        """d (K, ld >= ncon), diag (K, n) with the objective's curvature already in it -> Kc (K, n, lda)"""
        return normal_matrix(self.st["n"], self.st["ncon"], self.maps, self.vals0, self.vals1, d, self.hessd, diag, out=out)


def _group_key(m):
    return (m.method, m.S, m.M, m.time_jump, m.time_land)


def solve_batch(models, Z0s=None, tol=1e-3, max_iter=3000, backend='device', callbacks=None, verbose=False, clocks=None,
                newton='dense', driver='host', chol='workgroup'):
    """Solve the models' NLPs in lockstep -> list of (Z, info), in the models' order.  The K problems share S, M and the phases;
    problems of one method form a group that moves through the K-problem kernels together (alpha and the friction fields may
    differ from problem to problem: a grid of alphas x resampled terrains is ONE group), the groups one after the other.  A
    problem that has ended stops changing and leaves the launches; its Z and info are bitwise what its own K = 1 run returns.
    On the device a group whose models do not share their fields holds them stacked, K x 3 x 30 x M x 8 bytes (``GroupFields``;
    fields='device' / ``from_device`` models take part through ``fields_f64()``), and must be on one device.
      Z0s        starting points (default: ``model.initial_guess()``)
      backend    'device' (csrc/hopper_ipm.hip, csrc/chol.hip) or 'numpy' (the step on the host)
      callbacks  backend='numpy' only: one object per model with g(Z), jac_values(Z), hess_blocks(Z, lam, obj_factor)
      clocks     a dict that receives the seconds spent in callbacks / normal / factor / solve and the wall clock
      newton     'dense': the condensed matrix over all n = 8(S+1) + 4S + M + 2 variables (the default; n^2 memory, right at the
                 script's M = 30); 'arrow': the M sample variables ys are eliminated exactly and the 8(S+1) + 4S + 2 core is
                 factored (``hopper_arrow``): memory and work are O(M C), for any M
      driver     'host' (``ipm.solve_group``: the iterate and the vector algebra on the host) or 'device'
                 (``ipm.solve_group_device``, backend='device' only: the iterate stays on the device, csrc/ipm_driver.hip and
                 csrc/hopper_g.hip, and the clocks hold the time to launch; info["driver"] = 'device'.  With newton='arrow' the
                 models must be on a GPU with precision='f64'), or 'device_grid': 'device' with the driver's own vector kernels
                 spread over the rows (csrc/ipm_driver_grid.hip, DESIGN §7.al: the same bits, so Z and info do not depend on
                 it but for info["driver"] = 'device_grid'; it pays where a problem has many thousands of rows)
      chol       'workgroup' (csrc/chol.hip: one workgroup per problem) or 'grid' (csrc/chol_grid.hip: every factorization a
                 sequence of launches over the whole device; the same bits, so Z and info do not depend on it).  backend='numpy'
                 ignores it: its Cholesky is NumPy's
    info: status ('converged' | 'max_iter' | 'line_search'), iterations, factorizations, E0, primal_infeasibility,
    dual_infeasibility, f, and the final multipliers y, zl, zu with the slacks s and the objective scale sf."""
    if backend not in ('device', 'numpy'):
        raise ValueError(f"backend must be 'device' or 'numpy', got {backend!r}")
    if newton not in ('dense', 'arrow'):
        raise ValueError(f"newton must be 'dense' or 'arrow', got {newton!r}")
    _ipm.check_driver(driver, backend)
    _ipm.check_chol(chol)
    if callbacks is not None and backend != 'numpy':
        raise ValueError("callbacks are the numpy backend's")
    models = list(models)
    if _ipm.on_device(driver) and newton == 'arrow' and any(m.device.type != 'cuda' or m.precision != 'f64' for m in models):
        raise ValueError("newton='arrow' under driver='device' works on the partials the fp64 slip kernel leaves on the device: "
                         "every model needs a GPU and precision='f64'")
    Z0s = [m.initial_guess() for m in models] if Z0s is None else [np.asarray(Z, dtype=np.float64) for Z in Z0s]
    if len(Z0s) != len(models) or any(Z.shape != (m.num_vars,) for Z, m in zip(Z0s, models)):
        raise ValueError("Z0s must hold one (num_vars,) vector per model")
    if len({(m.S, m.M, m.time_jump, m.time_land) for m in models}) > 1:
        raise ValueError("the problems of a batch share S, M and the phases")
    groups = {}
    for i, m in enumerate(models):
        groups.setdefault(_group_key(m), []).append(i)
    if newton == 'arrow':
        from . import hopper_arrow
        on_device, on_host = hopper_arrow.ArrowDeviceBackend, hopper_arrow.ArrowNumpyBackend
    else:
        on_device, on_host = DeviceBackend, NumpyBackend

    def setup(members):
        ms = [models[i] for i in members]
        cbs = None if callbacks is None else [callbacks[i] for i in members]
        return ms, (on_device(ms, chol=chol) if backend == 'device' else on_host(ms, cbs))

    return _ipm.solve_groups(list(groups.values()), setup, Z0s, tol, max_iter, verbose, clocks, driver=driver)

