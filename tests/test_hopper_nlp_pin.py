"""CPU: the hopper's whole NLP (hopper/hopper.py:491-640) without a device.

  * the fp64 NumPy restatement (tests/_hopper_nlp.py: values, Jacobian, Hessian blocks) equals what the reference's own text
    gives on the stand-in (tests/golden/ref_hopper_nlp.npz, make_reference_golden_hopper_nlp.py) at S = 30, M = 30 and at
    S = 6, M = 4, for 'saa' and 'baseline'.  Errors are relative to each array's max |entry|, the Hessian's per step block.
    Measured here: g 2.0e-16, jacrev(g) 1.6e-16, Hessian blocks 6.9e-16; PIN is 100 x the worst of them;
  * the structure the kernels and the facade rely on, in the reference's own numbers: nothing of the Hessian lies outside the
    S + 1 step blocks, the facade's structural Jacobian pattern holds every non-zero, and the index maps the facade uploads
    place every block entry where np.tril_indices(nvar) has it;
  * central differences on the restatement (h = 1e-5, three seeded directions with max |v| = 1): g against J v and J' lam
    against H v within 1e-8 of max |J| / max |H| (measured here: 2.9e-10 and 2.8e-10);
  * gL_gU, x_bounds, f and grad_f against the fixture and the literal values of :599-620;
  * the params struct's Python layout equals the library's bytes query, and the RATO_EINVAL cases, which return before any
    device call.
"""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _hopper_nlp as R

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = 7e-14                  # 100 x 6.9e-16, the worst error measured over both cases (the Hessian blocks at S = 30)
FD_TOL = 1e-8
ALPHA = 0.2
CASES = ["", "s6_"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_hopper_nlp.npz"))


def case(fx, pre):
    S, M = int(fx[pre + "S"]), int(fx[pre + "M"])
    fields = (fx[pre + "intensities"], fx[pre + "thetas"], fx[pre + "taus"])
    return S, M, int(fx[pre + "time_jump"]), int(fx[pre + "time_land"]), fields


def dense(fx, pre, key):
    return sp.csc_matrix((fx[pre + key + "_data"], fx[pre + key + "_indices"], fx[pre + key + "_indptr"]),
                         shape=tuple(fx[pre + key + "_shape"])).toarray()


@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def host_model(S, M, method="saa", phases=None):
    from riskaversetrajopt_amd import hopper
    return hopper.Model.host_only(M, method, ALPHA, S=S, phases=phases)


def test_fixture_is_the_documented_case(fx):
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_reference_golden_hopper_nlp as gen
    assert float(fx["alpha"]) == ALPHA and "jax_standin" in str(fx["notes"])
    for pre, S, M, tj, tl in gen.CASES:
        assert case(fx, pre)[:4] == (S, M, tj, tl) and (tj, tl) == (S // 3, 2 * S // 3)
        nvar = R.nvar_of(S, M)
        L = R.layout(S, M, tj, tl, "saa")
        assert float(fx[pre + "dt"]) == 2.0 / S
        np.testing.assert_array_equal(fx[pre + "Z"], gen.G.hopper_Z(S, M, nvar))
        np.testing.assert_array_equal(fx[pre + "lam"], gen.lam_mixed(L["ncon"]))
        assert np.any(fx[pre + "lam"] > 0.5) and np.any(fx[pre + "lam"] < -0.5)
        assert fx[pre + "g_saa"].shape == (L["ncon"],) and tuple(fx[pre + "J_shape"]) == (L["ncon"], nvar)
        assert fx[pre + "g_baseline"].shape == (R.layout(S, M, tj, tl, "baseline")["ncon"],)
        assert tuple(fx[pre + "H_shape"]) == (nvar, nvar)
    assert R.nvar_of(30, 30) == 400 and R.layout(30, 30, 10, 20, "saa")["ncon"] == 1145


def test_fixture_was_generated_from_this_reference(fx):
    import hashlib
    key = fx["ref_sha256__hopper__hopper_py"]
    assert key.dtype == np.uint8 and key.shape == (32,)
    path = os.path.join(os.environ.get("RATO_REFERENCE", "/root/reference"), "hopper", "hopper.py")
    if os.path.exists(path):
        assert hashlib.sha256(open(path, "rb").read()).digest() == key.tobytes()


# ---- 1. the restatement against the fixture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", CASES)
def test_restatement_equals_reference(fx, pre):
    S, M, tj, tl, fields = case(fx, pre)
    Z, lam = fx[pre + "Z"], fx[pre + "lam"]
    loc = R.local(Z, S)
    errs = {}
    for method in ("saa", "baseline"):
        errs["g " + method] = R.rel_err(R.g_full(Z, S, M, method, ALPHA, fields, loc), fx[pre + "g_" + method])
    errs["jacrev(g)"] = R.rel_err(R.jac_dense(Z, S, M, "saa", ALPHA, fields, loc), dense(fx, pre, "J"))
    ref_blocks, rest = R.blocks_from_dense(dense(fx, pre, "H"), S)
    assert not np.any(rest)
    got = R.hess_blocks_full(Z, lam, S, M, "saa", ALPHA, fields, 0.0, loc)
    assert all(np.max(np.abs(b)) > 0.1 for b in ref_blocks), "every block carries curvature at this iterate"
    errs["hess blocks"] = R.rel_err_blocks(got, ref_blocks)
    print(pre, errs)
    for what, err in errs.items():
        assert err <= PIN, (what, err)
    assert R.objective(Z, S) == pytest.approx(float(fx[pre + "f"]), rel=1e-15)


# ---- 2. structure -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", CASES)
def test_hessian_is_block_diagonal_in_the_references_numbers(fx, pre):
    S, M, tj, tl, _ = case(fx, pre)
    H = dense(fx, pre, "H")
    blocks, rest = R.blocks_from_dense(H, S)
    assert not np.any(rest), "every entry outside the S + 1 step blocks is exactly 0"
    nX = 8 * (S + 1)
    assert not np.any(H[nX + 4 * S:]) and not np.any(H[:, nX + 4 * S:]), "ys, slack and t_risk rows and columns are exactly 0"
    dead = [1, 4, 5]                                             # x1, x4, x5 never carry curvature; x0 only through the slip rows
    assert not np.any(blocks[:, dead, :]) and not np.any(blocks[:, :, dead])
    flight = np.arange(tj, tl)
    assert not np.any(blocks[flight, 0, :]) and np.any(blocks[:tj, 0, :]), "x0 is active on contact steps only"
    assert not np.any(blocks[S, 8:, :]) and not np.any(blocks[S, :, 8:]), "the last block is x_S alone"
    np.testing.assert_array_equal(R.dense_from_blocks(blocks, S, H.shape[0]), H)


@pytest.mark.parametrize("pre", CASES)
@pytest.mark.parametrize("method", ["saa", "baseline"])
def test_structural_jacobian_pattern_holds_every_nonzero(fx, lib, pre, method):
    S, M, tj, tl, fields = case(fx, pre)
    lay = host_model(S, M, method).nlp_layout()
    L = R.layout(S, M, tj, tl, method)
    assert lay["ncon"] == L["ncon"] and all(lay["off"][k] == L[k] for k in lay["off"])
    J = dense(fx, pre, "J") if method == "saa" else R.jac_dense(fx[pre + "Z"], S, M, method, ALPHA, fields)
    pat = sp.csc_matrix((np.ones(lay["jac_indices"].size), lay["jac_indices"], lay["jac_indptr"]), shape=J.shape)
    assert pat.has_sorted_indices or np.all(np.diff(pat.indptr) >= 0)
    P = pat.toarray()
    assert P.max() == 1.0, "no entry twice"
    assert not np.any((J != 0.0) & (P == 0.0))
    assert np.array_equal(np.sort(np.concatenate([lay["pos_det"], lay["pos_slip"]])), np.arange(lay["jac_indices"].size))
    # the emission maps, run on the restatement's local quantities in NumPy, give the reference's deterministic rows
    loc = R.local(fx[pre + "Z"], S)
    det = lay["det_const"].copy()
    for m, src in ((lay["map_defect"], loc["d_defect"].reshape(-1)), (lay["map_rows"], loc["d_rows"].reshape(-1) * lay["scale_rows"])):
        assert np.unique(m[m >= 0]).size == np.count_nonzero(m >= 0)
        det[m[m >= 0]] = src[m >= 0]
    Jd = sp.csc_matrix((det, lay["det_indices"], lay["det_indptr"]), shape=J.shape).toarray()
    Jref = J.copy()
    Jref[L["risk"]:L["control"]] = 0.0
    assert R.rel_err(Jd, Jref) <= PIN
    mr = lay["map_rows"].reshape(S + 1, 2, 4)
    assert np.all(mr[tj:tl, 0] == -1) and np.all(mr[:, 1, 2:] == -1), "no no-slip row in flight; the height ignores x6, x7"
    assert np.all(lay["scale_rows"].reshape(S + 1, 2, 4)[tj:tl, 1, :2] == -1.0)


@pytest.mark.parametrize("S,M,phases", [(30, 30, None), (6, 4, None), (3, 2, (0, 3)), (1, 1, (1, 1)), (5, 2, (0, 0))])
def test_hessian_map_reproduces_tril_placement(lib, S, M, phases):
    m = host_model(S, M, phases=phases)
    lay = m.nlp_layout()
    nvar = lay["nvar"]
    rng = np.random.RandomState(S)
    blocks = rng.uniform(-1, 1, (S + 1, 12, 12))
    blocks = blocks + np.swapaxes(blocks, 1, 2)
    blocks[S, 8:, :] = 0.0
    blocks[S, :, 8:] = 0.0
    dense_H = R.dense_from_blocks(blocks, S, nvar)              # the dense scatter, in NumPy
    want = dense_H[np.tril_indices(nvar)]
    got = np.zeros(nvar * (nvar + 1) // 2)
    mp, v = lay["map_hess"].reshape(-1), R.tril78(blocks).reshape(-1)
    assert np.unique(mp[mp >= 0]).size == np.count_nonzero(mp >= 0) == (S + 1) * 78 - (78 - 36)
    got[mp[mp >= 0]] = v[mp >= 0]
    np.testing.assert_array_equal(got, want)
    from riskaversetrajopt_amd import hopper
    for t in range(S + 1):
        np.testing.assert_array_equal(hopper.block_variables(S, t), R.block_vars(S, t))


# ---- 3. finite differences on the restatement -------------------------------------------------------------------------------
def test_finite_differences_on_the_restatement(fx):
    S, M, tj, tl, fields = case(fx, "")
    Z, lam = R.problem(S, M, 0), fx["lam"]
    J = R.jac_dense(Z, S, M, "saa", ALPHA, fields)
    assert np.count_nonzero(J) == 7560
    H = R.dense_from_blocks(R.hess_blocks_full(Z, lam, S, M, "saa", ALPHA, fields), S, Z.size)
    h = 1e-5
    for v in R.directions(Z.size):
        assert np.max(np.abs(v)) == 1.0
        gp, gm = (R.g_full(Z + s * h * v, S, M, "saa", ALPHA, fields) for s in (1, -1))
        e_g = np.max(np.abs((gp - gm) / (2 * h) - J @ v)) / np.max(np.abs(J))
        Jp, Jm = (R.jac_dense(Z + s * h * v, S, M, "saa", ALPHA, fields) for s in (1, -1))
        e_h = np.max(np.abs((Jp - Jm).T @ lam / (2 * h) - H @ v)) / np.max(np.abs(H))
        print("fd", e_g, e_h)
        assert e_g <= FD_TOL and e_h <= FD_TOL


# ---- 4. bounds and objective ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", CASES)
def test_bounds_and_objective(fx, lib, pre):
    S, M, tj, tl, _ = case(fx, pre)
    m = host_model(S, M)
    Z = fx[pre + "Z"]
    g_L, g_U = m.gL_gU()
    np.testing.assert_array_equal(g_L, fx[pre + "gL"])
    np.testing.assert_array_equal(g_U, fx[pre + "gU"])
    for a, b in zip(R.bounds_g(S, M, tj, tl, "saa"), (g_L, g_U)):
        np.testing.assert_array_equal(a, b)
    x_L, x_U = m.x_bounds()
    assert x_L.shape == x_U.shape == (R.nvar_of(S, M),)
    for t in (0, S):
        np.testing.assert_array_equal(x_L[8 * t:8 * t + 8], [-3, 0.5, -np.pi / 2, 0.1, -500, -500, -500, -500])
        np.testing.assert_array_equal(x_U[8 * t:8 * t + 8], [3, 10, np.pi / 2, 3, 500, 500, 500, 500])
    assert np.all(x_L[8 * (S + 1):] == -1000.0) and np.all(x_U[8 * (S + 1):] == 1000.0)
    assert m.f(Z) == pytest.approx(float(fx[pre + "f"]), rel=1e-15)
    gf = m.grad_f(Z)
    np.testing.assert_array_equal(gf, R.grad_objective(Z, S))
    h = 1e-6
    for v in R.directions(Z.size, 2, seed=9):
        assert (m.f(Z + h * v) - m.f(Z - h * v)) / (2 * h) == pytest.approx(gf @ v, rel=1e-6)
    # the baseline has no SAA rows: M C risk rows instead of 1 + M + M C + 1
    assert host_model(S, M, "baseline").nlp_layout()["ncon"] == m.nlp_layout()["ncon"] - 2 - M


# ---- 5. / 6. the binding ----------------------------------------------------------------------------------------------------
def test_params_struct_layout_matches_the_library(lib):
    from riskaversetrajopt_amd import _lib, hopper
    assert C.sizeof(_lib.HopperNlpParams) == lib.rato_hopper_nlp_params_bytes() == 4 * 4 + 8 * 6 + 8 * 16
    p = hopper.nlp_params(30)
    assert (p.S, p.time_jump, p.time_land, p.dt) == (30, 10, 20, 2.0 / 30)
    assert (p.mass_body, p.mass_leg, p.inertia_body, p.inertia_leg, p.gravity) == (3.0, 0.3, 0.75, 0.075, 9.81)
    np.testing.assert_array_equal(list(p.state_initial), R.STATE_INITIAL)
    np.testing.assert_array_equal(list(p.state_final), R.STATE_FINAL)


def test_invalid_arguments_are_refused_without_a_launch(lib):
    """every case returns RATO_EINVAL before the first device call: the pointers below are never dereferenced"""
    from riskaversetrajopt_amd import hopper
    EINVAL = -1
    P = C.c_void_p(4096)
    S = 6
    nvar = 8 * (S + 1) + 4 * S
    good = hopper.nlp_params(S)

    def lin(p, K=1, Z=P, ldz=nvar):
        return lib.rato_hopper_nlp_linearize(C.byref(p), K, Z, ldz, P, P, P, P, None)

    def hes(p, K=1, Z=P, ldz=nvar, lam_dyn=P, lam_rows=P, out=P):
        return lib.rato_hopper_nlp_hessian(C.byref(p), K, Z, ldz, lam_dyn, lam_rows, None, out, None)
    for call in (lin, hes):
        assert call(hopper.nlp_params(0, 0, 0, dt=1.0)) == EINVAL                       # S < 1
        assert call(good, K=0) == EINVAL
        assert call(good, ldz=nvar - 1) == EINVAL
        assert call(good, Z=None) == EINVAL
        for tj, tl in ((-1, 3), (4, 3), (2, S + 1)):
            assert call(hopper.nlp_params(S, tj, tl)) == EINVAL
    assert hes(good, lam_dyn=None) == EINVAL and hes(good, lam_rows=None) == EINVAL and hes(good, out=None) == EINVAL
    assert lib.rato_hopper_nlp_linearize(None, 1, P, nvar, P, P, P, P, None) == EINVAL

    def sc(K=1, n=4, src=P, ld_src=4, mp=P, dst=P, ld_dst=8, n_dst=8):
        return lib.rato_scatter_f64(K, n, src, ld_src, mp, None, dst, ld_dst, n_dst, None)
    assert sc(K=0) == EINVAL and sc(n=0) == EINVAL and sc(ld_src=3) == EINVAL and sc(ld_dst=7) == EINVAL
    assert sc(src=None) == EINVAL and sc(mp=None) == EINVAL and sc(dst=None) == EINVAL and sc(n_dst=0) == EINVAL


def test_fold_multipliers_owns_the_phase_masks(lib):
    for S, phases in ((6, None), (3, (0, 0)), (3, (0, 3)), (3, (3, 3)), (4, (2, 2))):
        m = host_model(S, 2, phases=phases)
        tj, tl = m.time_jump, m.time_land
        ncon = m.nlp_layout()["ncon"]
        lam = np.random.RandomState(S).uniform(-1, 1, (2, ncon))
        ld, lr = m.fold_multipliers(lam)
        for k in range(2):
            ld2, lr2 = R.fold_lam(lam[k], S, 2, tj, tl, "saa")
            np.testing.assert_array_equal(ld[k], ld2)
            np.testing.assert_array_equal(lr[k], lr2)
        assert np.all(lr[:, tj:tl, 0] == 0.0)
