"""GPU: the hopper NLP kernels (csrc/hopper_nlp.hip) and ``hopper.Model``'s NLP members against the fp64 restatement
(tests/_hopper_nlp.py) and the reference's own numbers (tests/golden/ref_hopper_nlp.npz).

Errors are relative to each array's max |entry|, the Hessian's per step block.  DEV_TOL is 100 x the worst error measured on
the MI355X over the sweep of test_kernels_equal_the_restatement (device sin / cos and FMA contraction differ from the host's
by ulps).  No board was available when this was written: the sweep is UNMEASURED on a device and DEV_TOL stays at the value
the Gaussian kernels needed, 2.3e-12.  (On the host, the kernels' device functions compiled as a host program agree with the
restatement to 4.5e-16 over S in {1, 6, 30, 65}.)
"""
import os

import numpy as np
import pytest

import _hopper_nlp as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV_TOL = 2.3e-12
FD_TOL = 1e-8
ALPHA = 0.2
EPS = np.finfo(np.float64).eps
E = {(r, c): r * (r + 1) // 2 + c for r in range(12) for c in range(r + 1)}      # np.tril_indices(12) position of (r, c)
SLIP_ENTRIES = [E[p] for p in ((0, 0), (2, 0), (3, 0), (2, 2), (3, 2), (3, 3), (11, 0), (11, 2), (11, 3))]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_hopper_nlp.npz"))


def dev_model(S, M=2, method="saa", phases=None, fields=None):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, ALPHA, S=S, fields=fields, rng=np.random.RandomState(1), phases=phases)


def problems(m, K, seed=0):
    Zs = np.stack([R.problem(m.S, m.M, seed + k) for k in range(K)])
    lams = np.random.RandomState(50 + seed + m.S).uniform(-1, 1, (K, m.nlp_layout()["ncon"]))
    return Zs, lams


def upload(m, Zs, pad=0):
    """Zs (K, nvar) -> device tensor [K][nvar + pad]; the padding holds NaN, which no kernel may read"""
    import torch
    buf = torch.full((Zs.shape[0], Zs.shape[1] + pad), float("nan"), dtype=torch.float64, device=m.device)
    buf[:, :Zs.shape[1]] = torch.as_tensor(Zs, device=m.device)
    return buf


def phase_cases(S):
    return [None, (0, 0), (0, S), (S, S), (S // 2, S // 2)]


# ---- 7. kernels against the restatement --------------------------------------------------------------------------------------
_WORST = {}


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 3, 6, 30, 65])
def test_kernels_equal_the_restatement(S, K):
    worst = {}
    for phases in phase_cases(S):
        m = dev_model(S, phases=phases)
        tj, tl = m.time_jump, m.time_land
        Zs, lams = problems(m, K)
        ref = []
        for k in range(K):
            loc = R.local(Zs[k], S)
            loc["hess_blocks"] = R.tril78(R.blocks_of(loc, *R.fold_lam(lams[k], S, m.M, tj, tl, "saa")))
            ref.append(loc)
        for pad in (0, 5):
            r = m.nlp_device(upload(m, Zs, pad), lams)
            for k in range(K):
                for name in ("defect", "d_defect", "rows", "d_rows"):
                    got = r[name][k].cpu().numpy()
                    assert np.all(np.isfinite(got))
                    worst[name] = max(worst.get(name, 0.0), R.rel_err(got, ref[k][name]))
                got = r["hess_blocks"][k].cpu().numpy()
                assert np.all(np.isfinite(got)) and not np.any(got[S, 36:]), "the u part of the last block is exactly 0.0"
                worst["hess_blocks"] = max(worst.get("hess_blocks", 0.0), R.rel_err_blocks(got, ref[k]["hess_blocks"], 1))
                # the emission is exact: the tril-packed Hessian and the CSC values hold the kernel's own numbers
                nvar = m.num_vars
                dense = R.dense_from_blocks(R.untril78(got), S, nvar)
                np.testing.assert_array_equal(r["hess_tril"][k].cpu().numpy(), dense[np.tril_indices(nvar)])
                lay = m.nlp_layout()
                want = lay["det_const"].copy()
                for mp, src in ((lay["map_defect"], r["d_defect"][k].cpu().numpy().reshape(-1)),
                                (lay["map_rows"], r["d_rows"][k].cpu().numpy().reshape(-1) * lay["scale_rows"])):
                    want[mp[mp >= 0]] = src[mp >= 0]
                np.testing.assert_array_equal(r["jac_values"][k].cpu().numpy(), want)
    print("S", S, "K", K, {k: float("%.3g" % v) for k, v in worst.items()})
    for name, err in worst.items():
        _WORST[name] = max(_WORST.get(name, 0.0), err)
    print("worst so far", {k: float("%.3g" % v) for k, v in _WORST.items()})
    for name, err in worst.items():
        assert err <= DEV_TOL, (name, err)


# ---- 8. exact zeros and NULL outputs ---------------------------------------------------------------------------------------------
def test_exact_zeros_null_outputs_and_add():
    import torch
    from riskaversetrajopt_amd import hopper
    S, K = 7, 2
    m = dev_model(S)
    p = hopper.nlp_params(S)
    Zs, _ = problems(m, K)
    Zd = upload(m, Zs)
    lam_dyn, lam_rows = (torch.as_tensor(np.stack(a), device=m.device) for a in zip(*(R.lam_pair(S, k) for k in range(K))))
    zero = hopper.nlp_hessian_device(p, Zd, torch.zeros_like(lam_dyn), torch.zeros_like(lam_rows))
    assert not bool(zero.any()), "lam = 0 and add = NULL: every block is exactly 0.0"
    base = hopper.nlp_hessian_device(p, Zd, lam_dyn, lam_rows)
    assert not bool(base[:, S, 36:].any()) and bool(base[:, S, :36].any()), "the last block's u part is exactly 0.0"
    dead = [E[(r, c)] for (r, c) in E if {r, c} & {0, 1, 4, 5}]
    assert not bool(base[:, :, dead].any()), "pairs that hold x0, x1, x4 or x5 carry no second derivative"
    # x2 = 0 exactly: what vanishes with sin x2 is exactly 0.0 (rows only: lam_dyn = 0)
    Z0 = Zs.copy()
    Z0[:, 2:8 * (S + 1):8] = 0.0
    Z0d = upload(m, Z0)
    rows_only = hopper.nlp_hessian_device(p, Z0d, torch.zeros_like(lam_dyn), lam_rows).cpu().numpy()
    assert not np.any(rows_only[:, :, [E[(3, 2)], E[(6, 2)]]])
    assert np.all(rows_only[:, :, [E[(2, 2)], E[(7, 2)], E[(6, 3)]]] != 0.0)
    lin0 = hopper.nlp_linearize_device(p, Z0d)
    d_rows = lin0["d_rows"].cpu().numpy()
    assert not np.any(d_rows[:, :, 0, 3]) and not np.any(d_rows[:, :, 1, 0]) and not np.any(d_rows[:, :, 1, 2:])
    # NULL optional outputs leave the others bitwise unchanged
    full = hopper.nlp_linearize_device(p, Zd)
    for want in (("defect",), ("d_defect",), ("rows",), ("d_rows",), ("defect", "d_rows"), ("d_defect", "rows")):
        part = hopper.nlp_linearize_device(p, Zd, want=want)
        assert set(part) == set(want)
        for name in want:
            assert torch.equal(part[name], full[name]), name
    assert hopper.nlp_linearize_device(p, Zd, want=()) == {}
    # add is added exactly: (with - without) equals add to one rounding
    add = np.random.RandomState(4).uniform(-3, 3, (K, S + 1, 78))
    w = hopper.nlp_hessian_device(p, Zd, lam_dyn, lam_rows, torch.as_tensor(add, device=m.device)).cpu().numpy()
    wo = base.cpu().numpy()
    scale = np.maximum(np.maximum(np.abs(w), np.abs(wo)), np.abs(add))
    assert np.all(np.abs((w - wo) - add) <= 2 * EPS * scale)
    np.testing.assert_array_equal(w[:, :, dead], add[:, :, dead])
    np.testing.assert_array_equal(w[:, S, 36:], add[:, S, 36:])


# ---- 9. finite differences on the device -----------------------------------------------------------------------------------------
def deterministic_g(m, r, k, Z):
    """every row of g but the risk group's (left 0), from the device tensors of one nlp_device call"""
    lay = m.nlp_layout()
    off, S, tj, tl = lay["off"], m.S, m.time_jump, m.time_land
    defect, rows = r["defect"][k].cpu().numpy(), r["rows"][k].cpu().numpy()
    xs, us = R.split(Z, S)
    g = np.zeros(lay["ncon"])
    g[:off["x0"]] = defect.reshape(-1)
    g[off["x0"]:off["xf"]] = xs[0] - R.STATE_INITIAL
    g[off["xf"]:off["slip"]] = (xs[-1] - R.STATE_FINAL)[4:6]
    g[off["slip"]:off["contact"]] = rows[lay["states"], 0]
    g[off["contact"]:off["over"]] = rows[lay["states"], 1]
    g[off["over"]:off["risk"]] = -rows[tj:tl, 1]
    g[off["control"]:off["slack"]] = us.reshape(-1)
    g[off["slack"]] = Z[-2]
    g[off["len"]:] = np.concatenate([xs[1:, 3], xs[1:, 7], xs[1:, 6]])
    return g


def deterministic_J(m, r, k):
    import scipy.sparse as sp
    lay = m.nlp_layout()
    return sp.csc_matrix((r["jac_values"][k].cpu().numpy(), lay["det_indices"], lay["det_indptr"]),
                         shape=(lay["ncon"], lay["nvar"])).toarray()


def test_finite_differences_on_the_device():
    S, M = 30, 30
    m = dev_model(S, M)
    Z = R.problem(S, M, 0)
    lam = problems(m, 1)[1][0]
    dirs = R.directions(Z.size)
    h = 1e-5
    Zs = np.stack([Z] + [Z + s * h * v for v in dirs for s in (1, -1)])
    r = m.nlp_device(Zs, np.tile(lam, (Zs.shape[0], 1)))
    J = deterministic_J(m, r, 0)
    tril = r["hess_tril"][0].cpu().numpy()
    H = np.zeros((Z.size, Z.size))
    H[np.tril_indices(Z.size)] = tril
    H = H + np.tril(H, -1).T
    assert np.max(np.abs(J)) > 1.0 and np.max(np.abs(H)) > 1.0
    for i, v in enumerate(dirs):
        kp, km = 1 + 2 * i, 2 + 2 * i
        e_g = np.max(np.abs((deterministic_g(m, r, kp, Zs[kp]) - deterministic_g(m, r, km, Zs[km])) / (2 * h) - J @ v))
        e_h = np.max(np.abs((deterministic_J(m, r, kp) - deterministic_J(m, r, km)).T @ lam / (2 * h) - H @ v))
        e_g, e_h = e_g / np.max(np.abs(J)), e_h / np.max(np.abs(H))
        print("fd on the device", e_g, e_h)
        assert e_g <= FD_TOL and e_h <= FD_TOL


# ---- 10. facade against the fixture --------------------------------------------------------------------------------------------
def _fixture_case(fx, pre):
    import scipy.sparse as sp
    S, M = int(fx[pre + "S"]), int(fx[pre + "M"])
    fields = (fx[pre + "intensities"], fx[pre + "thetas"], fx[pre + "taus"])
    dense = lambda key: sp.csc_matrix((fx[pre + key + "_data"], fx[pre + key + "_indices"], fx[pre + key + "_indptr"]),
                                      shape=tuple(fx[pre + key + "_shape"])).toarray()
    return S, M, fields, dense("J"), dense("H")


@pytest.mark.parametrize("pre", ["", "s6_"])
def test_facade_equals_the_reference(fx, pre):
    from tests.test_gpu_hopper import H_ATOL                    # the bound of the existing slip-row tests, unchanged
    S, M, fields, J_ref, H_ref = _fixture_case(fx, pre)
    Z, lam = fx[pre + "Z"], fx[pre + "lam"]
    errs = {}
    for method in ("saa", "baseline"):
        m = dev_model(S, M, method, fields=fields)
        lay = m.nlp_layout()
        risk = slice(lay["off"]["risk"], lay["off"]["control"])
        det = np.ones(lay["ncon"], dtype=bool)
        det[risk] = False
        g, ref = m.g(Z), fx[pre + "g_" + method]
        assert g.dtype == np.float64 and g.shape == ref.shape
        errs["g " + method] = R.rel_err(g[det], ref[det])
        np.testing.assert_allclose(g[risk], ref[risk], rtol=0, atol=H_ATOL)
    m = dev_model(S, M, "saa", fields=fields)
    lay = m.nlp_layout()
    risk = slice(lay["off"]["risk"], lay["off"]["control"])
    det = np.ones(lay["ncon"], dtype=bool)
    det[risk] = False
    A = m.jac_g(Z)
    assert A.shape == J_ref.shape and A.nnz == lay["jac_indices"].size
    np.testing.assert_array_equal(A.indices, lay["jac_indices"])
    np.testing.assert_array_equal(A.indptr, lay["jac_indptr"])
    assert np.array_equal(m.jac_g(R.problem(S, M, 3)).indices, A.indices), "the same pattern at every Z"
    J = A.toarray()
    errs["jac_g"] = R.rel_err(J[det], J_ref[det])
    # the slip rows: the bounds test_gpu_hopper.py applies to slip_jacobian (rtol 1e-4, atol 3e-5)
    np.testing.assert_allclose(J[risk], J_ref[risk], rtol=1e-4, atol=3e-5)
    # the Hessian of lam . g: obj_factor = 0 is what hess_lagrange_dot_g returns
    B = m.hess_lagrangian_blocks(Z, lam, 0.0)
    tril = m.hess_lagrangian(Z, lam, 0.0)
    nvar = m.num_vars
    np.testing.assert_array_equal(tril, R.dense_from_blocks(B, S, nvar)[np.tril_indices(nvar)])
    B_ref, rest = R.blocks_from_dense(H_ref, S)
    assert not np.any(rest)
    got, ref = R.tril78(B), R.tril78(B_ref)
    slip_ref = R.tril78(R.slip_blocks(Z, lam, S, M, "saa", ALPHA, fields)[0])
    touched = np.zeros_like(ref, dtype=bool)
    touched[m.contact_steps()[:, None], np.array(SLIP_ENTRIES)[None, :]] = True
    assert not np.any(slip_ref[~touched])
    block_max = np.max(np.abs(ref), axis=1, keepdims=True)
    errs["hess (no slip)"] = float(np.max(np.where(touched, 0.0, np.abs(got - ref)) / block_max))
    # entries that receive a slip contribution: the bound test_gpu_hopper.py applies to slip_hessian (rtol 1e-4, atol 2e-5 of
    # the slip Hessian's largest entry), on top of the deterministic part's
    bound = 1e-4 * np.abs(slip_ref) + 2e-5 * np.max(np.abs(slip_ref)) + DEV_TOL * block_max
    assert np.all(np.abs(got - ref)[touched] <= np.broadcast_to(bound, ref.shape)[touched])
    print(pre, errs)
    for what, err in errs.items():
        assert err <= DEV_TOL, (what, err)
    # obj_factor hess_f: 2 R on the diagonal of u0 and u1
    B1 = m.hess_lagrangian_blocks(Z, lam, 0.7)
    d = B1 - B
    want = np.zeros_like(d)
    want[:S, 8, 8] = want[:S, 9, 9] = 1.4
    np.testing.assert_allclose(d, want, rtol=0, atol=4 * EPS * np.max(np.abs(B)))


# ---- 11. ipopt_callbacks -----------------------------------------------------------------------------------------------------------
def test_ipopt_callbacks(fx):
    S, M, fields, _, _ = _fixture_case(fx, "s6_")
    Z, lam = fx["s6_Z"], fx["s6_lam"]
    m = dev_model(S, M, "saa", fields=fields)
    cb = m.ipopt_callbacks()
    nvar, ncon = cb["nvar"], cb["ncon"]
    assert (nvar, ncon) == (m.num_vars, m.nlp_layout()["ncon"])
    np.testing.assert_array_equal(cb["eval_g"](Z, np.empty(ncon)), m.g(Z))
    J = m.jac_g(Z).toarray()
    np.testing.assert_array_equal(cb["eval_jac_g"](Z, np.empty(ncon * nvar)).reshape(ncon, nvar), J)
    h = cb["eval_h"](Z, lam, 0.7, np.empty(nvar * (nvar + 1) // 2))
    np.testing.assert_array_equal(h, m.hess_lagrangian(Z, lam, 0.7))
    assert cb["eval_f"](Z) == m.f(Z) == pytest.approx(float(fx["s6_f"]), rel=1e-15)
    np.testing.assert_array_equal(cb["eval_grad_f"](Z, np.empty(nvar)), m.grad_f(Z))
    i1, i2 = np.indices((ncon, nvar))
    np.testing.assert_array_equal(cb["eval_jac_g_sparsity_indices"][0], i1.flatten())
    np.testing.assert_array_equal(cb["eval_jac_g_sparsity_indices"][1], i2.flatten())
    r, c = np.tril_indices(nvar)
    np.testing.assert_array_equal(cb["eval_h_sparsity_indices"][0], r)
    np.testing.assert_array_equal(cb["eval_h_sparsity_indices"][1], c)
    for a, b in zip((cb["g_L"], cb["g_U"]), m.gL_gU()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip((cb["x_L"], cb["x_U"]), m.x_bounds()):
        np.testing.assert_array_equal(a, b)
    sp_cb = m.ipopt_callbacks(sparse=True)
    jr, jc = sp_cb["eval_jac_g_sparsity_indices"]
    vals = sp_cb["eval_jac_g"](Z, np.empty(jr.size))
    Js = np.zeros((ncon, nvar))
    Js[jr, jc] = vals
    np.testing.assert_array_equal(Js, J)
    hr, hc = sp_cb["eval_h_sparsity_indices"]
    assert np.all(hr >= hc) and hr.size == (S + 1) * 78 - 42
    hv = sp_cb["eval_h"](Z, lam, 0.7, np.empty(hr.size))
    Hs = np.zeros((nvar, nvar))
    Hs[hr, hc] = hv
    np.testing.assert_array_equal(Hs[np.tril_indices(nvar)], h)
    np.testing.assert_array_equal(sp_cb["eval_g"](Z, np.empty(ncon)), m.g(Z))


# ---- 12. emission ------------------------------------------------------------------------------------------------------------------
def test_scatter_is_exact():
    import torch
    from riskaversetrajopt_amd import hopper
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(6)
    K, n, n_dst = 2, 999, 1500                                  # more than one workgroup, no multiple of it
    src = rng.uniform(-1, 1, (K, n))
    perm = rng.permutation(n_dst)[:n].astype(np.int64)
    dst = torch.zeros((K, n_dst), dtype=torch.float64, device=dev)
    hopper.scatter_f64(torch.as_tensor(src, device=dev), torch.as_tensor(perm, device=dev), dst)
    want = np.zeros((K, n_dst))
    want[:, perm] = src
    np.testing.assert_array_equal(dst.cpu().numpy(), want)
    assert np.count_nonzero(want[0] == 0.0) == n_dst - n, "zeroed destinations stay zero where the map does not point"
    # entries outside [0, n_dst) are not emitted; the scale is applied exactly
    skip = perm.copy()
    skip[::7] = -1
    skip[3::7] = n_dst
    scale = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    dst2 = torch.full((K, n_dst), 5.0, dtype=torch.float64, device=dev)
    hopper.scatter_f64(torch.as_tensor(src, device=dev), torch.as_tensor(skip, device=dev), dst2,
                       torch.as_tensor(scale, device=dev))
    want2 = np.full((K, n_dst), 5.0)
    ok = (skip >= 0) & (skip < n_dst)
    want2[:, skip[ok]] = (src * scale)[:, ok]
    np.testing.assert_array_equal(dst2.cpu().numpy(), want2)
    # a full permutation of a whole array
    full = rng.permutation(n).astype(np.int64)
    dst3 = torch.zeros((K, n), dtype=torch.float64, device=dev)
    hopper.scatter_f64(torch.as_tensor(src, device=dev), torch.as_tensor(full, device=dev), dst3)
    np.testing.assert_array_equal(dst3.cpu().numpy()[:, full], src)


# ---- 13. batch against singles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [6, 65])
def test_batch_equals_singles_bitwise(S):
    import torch
    m = dev_model(S)
    Zs, lams = problems(m, 3, seed=20)
    add = np.random.RandomState(8).uniform(-1, 1, (3, S + 1, 78))
    batch = m.nlp_device(Zs, lams, add=add)
    assert set(batch) == {"defect", "d_defect", "rows", "d_rows", "jac_values", "hess_blocks", "hess_tril"}
    for k in range(3):
        one = m.nlp_device(Zs[k:k + 1], lams[k:k + 1], add=add[k:k + 1])
        for name, t in batch.items():
            assert torch.equal(t[k], one[name][0]), name
